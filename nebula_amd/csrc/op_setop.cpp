// UNION DISTINCT / INTERSECT / MINUS of two device-resident GO results (ngx_set_op, ngx_go_set): the host driver of
// setop.hip.
#include "engine_ctx.h"

// ============================================================================ UNION DISTINCT / INTERSECT / MINUS
namespace {

using SetResultHolder = CellResult<ngx_set_result>;

// one side's columns as the kernels read them (as orderBy lays a GO result's columns out)
int32_t setColumns(ngx_ctx* c, const ngx_go_result* r, std::vector<OrderEmitCol>& ecols) {
    ecols.assign(r->ncols, OrderEmitCol{});
    for (int32_t y = 0; y < r->ncols; y++) {
        const int32_t t = r->col_types[y];
        OrderEmitCol& e = ecols[y];
        e.cell = t;                                               // NGX_CELL_* numbers its kinds as NGX_T_*
        e.c.kind = t == NGX_T_STRING ? kGroupString : t == NGX_T_DOUBLE || t == NGX_T_FLOAT ? kGroupDouble : kGroupInt;
        e.c.w = t == NGX_T_STRING || t == NGX_T_DOUBLE || t == NGX_T_FLOAT ? 8 : r->dev_col_w ? r->dev_col_w[y] : 8;
        e.c.konst = r->dev_col_const ? r->dev_col_const[y] : 0;
        if (!r->nrows) continue;
        e.c.x = e.c.w ? r->dev_cols[y].x : nullptr;
        e.c.len = r->dev_cols[y].len;
        if (e.c.w && !e.c.x) return fail(c, NGX_E_BAD_ARGUMENT, "set op: column without values");
        if (e.c.w != 0 && e.c.w != 1 && e.c.w != 2 && e.c.w != 4 && e.c.w != 8) return fail(c, NGX_E_BAD_ARGUMENT, "set op: column width");
        if (t == NGX_T_STRING && !e.c.len) return fail(c, NGX_E_BAD_ARGUMENT, "set op: string column without lengths");
    }
    return NGX_OK;
}

int32_t setOp(ngx_ctx* c, const ngx_go_result* L, const ngx_go_result* Rt, const ngx_set_plan* sp, SetResultHolder& R) {
    const ngx_go_result* side[2] = {L, Rt};
    for (const ngx_go_result* r : side)
        if (r->code != NGX_OK || (r->nrows && r->ncols && !r->dev_cols)) return fail(c, NGX_E_BAD_ARGUMENT, "set op: not a device-resident result");
    if (sp->op == NGX_SET_UNION_ALL) return fail(c, NGX_E_UNSUPPORTED, "set op: UNION ALL needs no kernel (the caller concatenates)");
    if (sp->op != NGX_SET_UNION_DISTINCT && sp->op != NGX_SET_INTERSECT && sp->op != NGX_SET_MINUS)
        return fail(c, NGX_E_BAD_ARGUMENT, "set op: unknown operator");
    if (L->ncols != Rt->ncols) return fail(c, NGX_E_BAD_ARGUMENT, "Field count not match.");      // SetExecutor.cpp:166-171
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "set op: world > 1 needs the shards' tables merged");
    const int32_t ncols = L->ncols;
    if (ncols > kSetMaxCols) return fail(c, NGX_E_UNSUPPORTED, "set op: more than 16 columns");
    const uint64_t n[2] = {L->nrows, Rt->nrows};
    R.r.left_rows = n[0];
    R.r.right_rows = n[1];
    R.r.ncols = ncols;
    R.colTypes.assign(L->col_types, L->col_types + ncols);
    R.r.col_types = R.colTypes.data();
    if (ncols == 0 || (n[0] == 0 && n[1] == 0)) {                 // onEmptyInputs: the column names and no rows
        c->setOpDevice++;
        return NGX_OK;
    }
    // one side empty (SetExecutor.cpp:202-213, 308-312, 358-368): the other side as it is, or nothing; no table
    int pass = -1;                                                // the side handed through whole
    if (n[0] == 0 || n[1] == 0) {
        if (sp->op == NGX_SET_UNION_DISTINCT) pass = n[0] ? 0 : 1;
        else if (sp->op == NGX_SET_MINUS && n[0]) pass = 0;
        else {
            c->setOpDevice++;
            return NGX_OK;
        }
    }
    for (int s = 0; s < 2; s++)
        for (int32_t y = 0; y < ncols; y++)
            if (side[s]->col_types[y] == 0 || (n[s] && side[s]->dev_cols[y].type))
                return fail(c, NGX_E_UNSUPPORTED, "set op: UNKNOWN-typed column (per-row value types)");
    if (pass < 0)
        for (int32_t y = 0; y < ncols; y++)
            if (L->col_types[y] != Rt->col_types[y]) return fail(c, NGX_E_UNSUPPORTED, "set op: column types differ (casting stays on the host)");
    if (n[0] >= (1ULL << 31) || n[1] >= (1ULL << 31)) return fail(c, NGX_E_UNSUPPORTED, "set op: 2^31 rows or more on a side");
    if (pass >= 0 && n[pass] > static_cast<uint64_t>(c->setRowsMax)) return fail(c, NGX_E_UNSUPPORTED, "set op: output rows above set_rows_max");
    if (pass == 1) R.colTypes.assign(Rt->col_types, Rt->col_types + ncols);

    std::vector<OrderEmitCol> ecols[2];
    bool anyString = false;
    for (int s = 0; s < 2; s++) {
        if (int32_t rc = setColumns(c, side[s], ecols[s])) return rc;
        for (const OrderEmitCol& e : ecols[s]) anyString |= e.c.kind == kGroupString;
    }

    resultEvents(c);
    const hipEvent_t ev0 = c->gbEv[0], ev1 = c->gbEv[1];
    HIP_OK(hipEventRecord(ev0, c->stream));

    // ---- descriptors: per side its emit columns, then its key columns
    const size_t perSide = ncols * (sizeof(OrderEmitCol) + sizeof(GroupCol));
    char* desc = c->sbDesc.get<char>(2 * perSide);
    OrderEmitCol* ecolsDev[2];
    GroupCol* colsDev[2];
    std::vector<GroupCol> cols[2];
    for (int s = 0; s < 2; s++) {
        ecolsDev[s] = reinterpret_cast<OrderEmitCol*>(desc + s * perSide);
        colsDev[s] = reinterpret_cast<GroupCol*>(ecolsDev[s] + ncols);
        cols[s].resize(ncols);
        for (int32_t y = 0; y < ncols; y++) cols[s][y] = ecols[s][y].c;
        HIP_OK(hipMemcpyAsync(ecolsDev[s], ecols[s].data(), ncols * sizeof(OrderEmitCol), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(colsDev[s], cols[s].data(), ncols * sizeof(GroupCol), hipMemcpyHostToDevice, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));                      // the host vectors are pageable: copied before they go

    // ---- build and probe: the kept rows of either side, in no order
    std::vector<uint32_t> kept[2];
    uint32_t* keepDev[2] = {nullptr, nullptr};
    if (pass < 0) {
        // a string longer than kOrderMaxStr in a key column: one lane would hash and compare it byte by byte
        if (anyString) {
            uint32_t* mx = c->obMax.get<uint32_t>(1);
            for (int s = 0; s < 2; s++)
                for (int32_t y = 0; y < ncols; y++) {
                    if (cols[s][y].kind != kGroupString) continue;
                    if (launchOrderMaxLen(cols[s][y].len, n[s], mx, c->stream)) throw Error{NGX_E_DEVICE, "set max length"};
                    if (readScalar(c, mx) > kOrderMaxStr) return fail(c, NGX_E_UNSUPPORTED, "set op: a string longer than 256 bytes");
                }
        }
        const bool uni = sp->op == NGX_SET_UNION_DISTINCT;
        const uint64_t nBuild = uni ? n[0] + n[1] : n[1];
        uint64_t slots = 64;
        while (slots < 2 * nBuild) slots <<= 1;
        SetArgs a{};
        a.n[0] = n[0];
        a.n[1] = n[1];
        a.cols[0] = colsDev[0];
        a.cols[1] = colsDev[1];
        a.nc = ncols;
        a.op = uni ? kSetUnionDistinct : sp->op == NGX_SET_INTERSECT ? kSetIntersect : kSetMinus;
        a.table = c->sbTable.get<uint64_t>(slots);
        a.mask = slots - 1;
        HIP_OK(hipMemsetAsync(a.table, 0, slots * sizeof(uint64_t), c->stream));
        if (a.op == kSetIntersect) {
            a.count = c->sbCount.get<uint32_t>(slots);
            a.taken = c->sbTaken.get<uint32_t>(slots);
            HIP_OK(hipMemsetAsync(a.count, 0, slots * sizeof(uint32_t), c->stream));
            HIP_OK(hipMemsetAsync(a.taken, 0, slots * sizeof(uint32_t), c->stream));
        }
        a.keep[0] = keepDev[0] = c->sbKeep[0].get<uint32_t>(std::max<uint64_t>(n[0], 1));
        a.keep[1] = keepDev[1] = c->sbKeep[1].get<uint32_t>(std::max<uint64_t>(n[1], 1));
        a.S = c->sbState.get<SetState>(1);
        a.gridMax = c->setGridMax;
        HIP_OK(hipMemsetAsync(a.S, 0, sizeof(SetState), c->stream));
        uint64_t rowBytes[2] = {0, 0};                            // value bytes a pass over a side's rows reads
        for (int s = 0; s < 2; s++)
            for (const GroupCol& g : cols[s]) rowBytes[s] += n[s] * static_cast<uint64_t>(g.w + (g.kind == kGroupString ? 4 : 0));
        c->timed("set_build", (uni ? rowBytes[0] : 0) + rowBytes[1] + nBuild * 16, [&] {
            if (uni && launchSetBuild(a, 0, c->stream)) throw Error{NGX_E_DEVICE, "set build"};
            if (launchSetBuild(a, 1, c->stream)) throw Error{NGX_E_DEVICE, "set build"};
        });
        c->timed("set_probe", rowBytes[0] + (uni ? rowBytes[1] : 0) + (n[0] + (uni ? n[1] : 0)) * 16, [&] {
            if (launchSetProbe(a, 0, c->stream)) throw Error{NGX_E_DEVICE, "set probe"};
            if (uni && launchSetProbe(a, 1, c->stream)) throw Error{NGX_E_DEVICE, "set probe"};
        });
        SetState st{};
        HIP_OK(hipMemcpyAsync(&st, a.S, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        c->setLoopFlushes += st.loopFlushes;
        if (st.err || st.fill[0] > n[0] || st.fill[1] > n[1]) throw Error{NGX_E_DEVICE, "set op: inconsistent counts"};
        if (st.fill[0] + st.fill[1] > static_cast<uint64_t>(c->setRowsMax)) return fail(c, NGX_E_UNSUPPORTED, "set op: output rows above set_rows_max");
        // the kept rows of each side in that side's row order (MINUS / INTERSECT: left order; UNION DISTINCT: the
        // left leaders, then the right ones)
        for (int s = 0; s < 2; s++) {
            kept[s].resize(st.fill[s]);
            if (st.fill[s]) HIP_OK(hipMemcpyAsync(kept[s].data(), keepDev[s], st.fill[s] * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        HIP_OK(hipStreamSynchronize(c->stream));
        for (int s = 0; s < 2; s++) {
            std::sort(kept[s].begin(), kept[s].end());
            if (!kept[s].empty()) HIP_OK(hipMemcpyAsync(keepDev[s], kept[s].data(), kept[s].size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        }
        HIP_OK(hipStreamSynchronize(c->stream));                  // kept[] is pageable
    }

    // ---- emit: the left rows, then the right rows
    const uint64_t mSide[2] = {pass < 0 ? kept[0].size() : pass == 0 ? n[0] : 0, pass < 0 ? kept[1].size() : pass == 1 ? n[1] : 0};
    const uint64_t m = mSide[0] + mSide[1];
    if (m == 0) {
        HIP_OK(hipEventRecord(ev1, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        float ms0 = 0;
        HIP_OK(hipEventElapsedTime(&ms0, ev0, ev1));
        c->collectTimings();
        R.r.device_ms = ms0;
        c->setOpDevice++;
        return NGX_OK;
    }
    GroupCell* cellsDev = c->sbCells.get<GroupCell>(m * ncols);
    OrderEmitArgs ea[2] = {};
    for (int s = 0; s < 2; s++) {
        ea[s].n = n[s];
        ea[s].m = mSide[s];
        ea[s].rows = pass < 0 ? keepDev[s] : nullptr;
        ea[s].ncols = ncols;
        ea[s].cols = ecolsDev[s];
        ea[s].cells = cellsDev + (s ? mSide[0] * ncols : 0);
    }
    uint64_t strBytes = 0;
    if (anyString) {
        uint64_t* slen = c->sbSlen.get<uint64_t>(m + 1);
        uint64_t* spre = c->sbSpre.get<uint64_t>(m + 1);
        uint64_t* tiles = c->sbTiles.get<uint64_t>((m + kTile - 1) / kTile + 1);
        for (int s = 0; s < 2; s++)
            if (launchOrderStrLen(ea[s], slen + (s ? mSide[0] : 0), c->stream)) throw Error{NGX_E_DEVICE, "set string lengths"};
        if (launchScanU64(slen, m, spre, tiles, c->stream)) throw Error{NGX_E_DEVICE, "set string scan"};
        strBytes = readScalar(c, spre + m);
        char* strOut = c->sbStr.get<char>(std::max<uint64_t>(strBytes, 1));
        for (int s = 0; s < 2; s++) {
            ea[s].strPre = spre + (s ? mSide[0] : 0);             // one scan over both sides: one string block
            ea[s].strOut = strOut;
        }
    }
    c->timed("set_emit", m * ncols * sizeof(GroupCell) + strBytes, [&] {
        for (int s = 0; s < 2; s++)
            if (launchOrderEmit(ea[s], c->stream)) throw Error{NGX_E_DEVICE, "set emit"};
    });
    finishCells(c, R, cellsDev, m * ncols, ea[0].strOut, strBytes);
    R.r.nrows = m;
    c->setOpDevice++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_set_op(ngx_ctx* c, const ngx_go_result* left, const ngx_go_result* right, const ngx_set_plan* plan,
                              ngx_set_result** out) {
    if (!c || !left || !right || !plan || !out) return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left reading the descriptors
    return abiCall<SetResultHolder>(c, out, OnFail::kSync, [&](SetResultHolder& R) { return setOp(c, left, right, plan, R); });
}

extern "C" void ngx_set_result_free(ngx_set_result* r) {
    if (r) delete reinterpret_cast<SetResultHolder*>(r);
}

// Both traversals with their results left in HBM, then ngx_set_op over them. A device-resident result is valid
// until the next call on the context, so the right traversal runs on the second query lane (LaneState: its
// own scratch, result rows and reservation state, as ngx_go_batch rotates them) and with string arenas of its
// own; the left result is not copied. The traversals run one after the other on the context's stream.
extern "C" int32_t ngx_go_set(ngx_ctx* c, const ngx_go_plan* left, const ngx_go_plan* right, const ngx_set_plan* plan,
                              ngx_set_result** out) {
    if (!c || !left || !right || !plan || !out) return NGX_E_BAD_ARGUMENT;
    return abiCall<SetResultHolder>(c, out, OnFail::kNoSync, [&](SetResultHolder& R) {
        ngx_go_result *rl = nullptr, *rr = nullptr;
        int32_t rc = NGX_OK;
        if (!left->result_on_device || !right->result_on_device || left->distinct || right->distinct || left->input_vid_col ||
            right->input_vid_col)
            rc = fail(c, NGX_E_BAD_ARGUMENT, "set op: both plans are device-resident GOs without DISTINCT or input");
        else if (c->world > 1)
            rc = fail(c, NGX_E_UNSUPPORTED, "set op: world > 1 needs the shards' tables merged");
        if (rc == NGX_OK) {
            if (c->activeLane != 0) c->useLane(0);
            rc = goCall(c, left, &rl);
        }
        if (rc == NGX_OK) {
            uint64_t d0[3] = {0, 0, 0}, d1[3] = {0, 0, 0};
            // string and untyped columns have no digest: the check covers integer / double / bool results
            const bool check = c->setCheckLeft && rl->nrows && resultDigest(c, rl, d0) == NGX_OK;
            c->useLane(1);
            std::swap(c->strArena, c->setArena);
            rc = goCall(c, right, &rr);
            if (rc == NGX_OK && check) {
                if (resultDigest(c, rl, d1) != NGX_OK || d0[0] != d1[0] || d0[1] != d1[1] || d0[2] != d1[2])
                    rc = fail(c, NGX_E_DEVICE, "set op: the left result changed during the right traversal");
                else
                    c->setLeftChecks++;
            }
            if (rc == NGX_OK) rc = guarded(c, OnFail::kNoSync, [&] { return setOp(c, rl, rr, plan, R); });
            if (rc != NGX_OK) (void)hipStreamSynchronize(c->stream);
            std::swap(c->strArena, c->setArena);
            c->useLane(0);
        }
        const std::string err = c->lastError;
        if (rr) ngx_go_result_free(rr);
        if (rl) ngx_go_result_free(rl);
        c->lastError = err;
        return rc;
    });
}

