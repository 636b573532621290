// GROUP BY, ORDER BY / LIMIT and GROUP BY | ORDER BY | LIMIT over a device-resident GO result (ngx_go_group_by,
// ngx_go_order_by, ngx_go_group_order_by): the host drivers of groupby.hip and orderby.hip.
#include "engine_ctx.h"

// ============================================================================ GROUP BY
namespace {

using GroupResultHolder = CellResult<ngx_group_result>;
using OrderResultHolder = CellResult<ngx_order_result>;

bool intLike(int32_t t) { return t == NGX_T_INT || t == NGX_T_VID || t == NGX_T_TIMESTAMP; }

// The grouping up to its state words, shared by ngx_go_group_by (which emits cells from it) and
// ngx_go_group_order_by (which turns it into columns): groupPrepare checks the plan and lays out columns, state
// slots and yield descriptors on the host; groupAccumulate runs assign + scan + accumulate and leaves the
// device state in the context's gb* buffers.
struct GroupStage {
    uint64_t n = 0, ngroups = 0;
    std::vector<GroupCol> cols;                                   // the result columns the kernels read
    std::vector<int32_t> typeOf, keyIdx, distinctCol;             // distinctCol: value column of each COUNT_DISTINCT pass
    std::vector<GroupSlot> slots;
    std::vector<GroupEmit> emit;
    std::vector<uint8_t> isCount;                                 // per yield: a COUNT / COUNT_DISTINCT state word, in [0, n]
    GroupCol* colsDev = nullptr;
    GroupSlot* slotsDev = nullptr;
    GroupEmit* emitDev = nullptr;
    uint32_t* leader = nullptr;
    uint64_t* flag = nullptr;
    uint64_t* pre = nullptr;
    uint64_t* tiles = nullptr;
    uint64_t* state = nullptr;
    bool lds = false;
};

int32_t groupPrepare(ngx_ctx* c, const ngx_go_result* r, const ngx_group_plan* gp, GroupStage& G) {
    if (r->code != NGX_OK || (r->nrows && r->ncols && !r->dev_cols)) return fail(c, NGX_E_BAD_ARGUMENT, "group by: not a device-resident result");
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "group by: world > 1 needs mergeable partial states");
    if (gp->nkeys < 1 || gp->nyields < 1 || !gp->key_cols || !gp->yields) return fail(c, NGX_E_BAD_ARGUMENT, "group by: no key or yield columns");
    if (gp->nkeys > kGroupMaxKeys) return fail(c, NGX_E_UNSUPPORTED, "group by: more than 4 keys");
    if (gp->nyields > kMaxDistinctCols) return fail(c, NGX_E_UNSUPPORTED, "group by: more than 64 yields");
    const uint64_t n = G.n = r->nrows;
    if (n >= (1ULL << 32)) return fail(c, NGX_E_UNSUPPORTED, "group by: 2^32 rows or more");

    std::vector<GroupCol>& cols = G.cols;
    std::vector<int32_t> colOf(std::max<int32_t>(r->ncols, 1), -1);
    std::vector<int32_t>& typeOf = G.typeOf;
    auto useCol = [&](int32_t y, bool key, int32_t* idx) -> int32_t {
        if (y < 0 || y >= r->ncols) return fail(c, NGX_E_BAD_ARGUMENT, "group by: no such result column");
        const int32_t t = r->col_types[y];
        if (t == 0 || (n && r->dev_cols[y].type)) return fail(c, NGX_E_UNSUPPORTED, "group by: UNKNOWN-typed column (per-row value types)");
        if (t == NGX_T_FLOAT) return fail(c, NGX_E_UNSUPPORTED, "group by: FLOAT column");
        if (key && t == NGX_T_DOUBLE) return fail(c, NGX_E_UNSUPPORTED, "group by: DOUBLE key column");
        if (colOf[y] < 0) {
            GroupCol gc{};
            gc.kind = t == NGX_T_STRING ? kGroupString : t == NGX_T_DOUBLE ? kGroupDouble : kGroupInt;
            gc.w = t == NGX_T_STRING || t == NGX_T_DOUBLE ? 8 : r->dev_col_w ? r->dev_col_w[y] : 8;
            gc.konst = r->dev_col_const ? r->dev_col_const[y] : 0;
            if (n) {
                gc.x = gc.w ? r->dev_cols[y].x : nullptr;
                gc.len = r->dev_cols[y].len;
                if (gc.w && !gc.x) return fail(c, NGX_E_BAD_ARGUMENT, "group by: column without values");
                if (gc.w != 0 && gc.w != 1 && gc.w != 2 && gc.w != 4 && gc.w != 8) return fail(c, NGX_E_BAD_ARGUMENT, "group by: column width");
            }
            colOf[y] = static_cast<int32_t>(cols.size());
            cols.push_back(gc);
            typeOf.push_back(t);
        }
        *idx = colOf[y];
        return NGX_OK;
    };
    std::vector<int32_t>& keyIdx = G.keyIdx;
    keyIdx.assign(gp->nkeys, -1);
    for (int32_t k = 0; k < gp->nkeys; k++)
        if (int32_t rc = useCol(gp->key_cols[k], true, &keyIdx[k])) return rc;

    // per yield column: its state words and how its cell is finalised
    std::vector<GroupSlot>& slots = G.slots;
    std::vector<GroupEmit>& emit = G.emit;
    std::vector<int32_t>& distinctCol = G.distinctCol;
    emit.assign(gp->nyields, GroupEmit{});
    G.isCount.assign(gp->nyields, 0);
    auto slot = [&](int32_t op, int32_t src, int32_t col) {
        GroupSlot s{};
        s.op = op, s.src = src, s.col = col;
        slots.push_back(s);
        return static_cast<int32_t>(slots.size() - 1);
    };
    auto constant = [&](GroupEmit& e, int32_t kind, int64_t bits) { e.kind = kind, e.src = kEmitConst, e.konst = bits; };
    for (int32_t y = 0; y < gp->nyields; y++) {
        const ngx_agg_col& a = gp->yields[y];
        GroupEmit& e = emit[y];
        if (a.fn == NGX_AGG_STD) return fail(c, NGX_E_UNSUPPORTED, "group by: STD keeps every value of a group");
        if (a.fn < NGX_AGG_GROUP || a.fn > NGX_AGG_BIT_XOR) return fail(c, NGX_E_BAD_ARGUMENT, "group by: unknown function");
        int32_t ci = -1, t = 0;
        if (a.col >= 0) {
            if (int32_t rc = useCol(a.col, false, &ci)) return rc;
            t = typeOf[ci];
        } else {                                                  // a constant: a column of width 0
            const int32_t k = a.konst.kind;
            if (k != NGX_CELL_INT && k != NGX_CELL_DOUBLE && a.fn != NGX_AGG_COUNT && a.fn != NGX_AGG_COUNT_DISTINCT)
                return fail(c, NGX_E_UNSUPPORTED, "group by: constant that is neither integer nor double");
            t = k == NGX_CELL_INT ? NGX_T_INT : k == NGX_CELL_DOUBLE ? NGX_T_DOUBLE : NGX_T_STRING;
            if (a.fn != NGX_AGG_GROUP && a.fn != NGX_AGG_COUNT && a.fn != NGX_AGG_COUNT_DISTINCT) {
                GroupCol gc{};
                gc.kind = t == NGX_T_DOUBLE ? kGroupDouble : kGroupInt;
                gc.w = 0;
                gc.konst = a.konst.v.i;
                ci = static_cast<int32_t>(cols.size());
                cols.push_back(gc);
                typeOf.push_back(t);
            }
        }
        switch (a.fn) {
            case NGX_AGG_GROUP:
                if (a.col < 0) { constant(e, a.konst.kind, a.konst.v.i); break; }
                if (std::find(keyIdx.begin(), keyIdx.end(), ci) == keyIdx.end())
                    return fail(c, NGX_E_UNSUPPORTED, "group by: a bare yield column that is not a key");
                e.kind = t, e.src = kEmitKey, e.a = ci;
                break;
            case NGX_AGG_COUNT:
                e.kind = NGX_CELL_INT, e.src = kEmitState, e.a = slot(kGroupAdd, kGroupSrcOne, -1);
                G.isCount[y] = 1;
                break;
            case NGX_AGG_COUNT_DISTINCT:
                if (a.col < 0) { constant(e, NGX_CELL_INT, 1); break; }
                e.kind = NGX_CELL_INT, e.src = kEmitState, e.a = slot(kGroupAdd, kGroupSrcFlag, static_cast<int32_t>(distinctCol.size()));
                distinctCol.push_back(ci);
                G.isCount[y] = 1;
                break;
            case NGX_AGG_SUM:
                if (intLike(t)) e.kind = t, e.src = kEmitState, e.a = slot(kGroupAdd, kGroupSrcCol, ci);
                else if (t == NGX_T_DOUBLE) e.kind = NGX_CELL_DOUBLE, e.src = kEmitState, e.a = slot(kGroupAddF64, kGroupSrcCol, ci);
                else constant(e, NGX_CELL_INT, 0);                // Sum ignores values it cannot add
                break;
            case NGX_AGG_AVG:
                if (t == NGX_T_VID || t == NGX_T_TIMESTAMP)
                    return fail(c, NGX_E_UNSUPPORTED, "group by: AVG of a VID / TIMESTAMP column (the reference reads the sum as a double)");
                e.kind = NGX_CELL_DOUBLE;
                if (t == NGX_T_INT) e.src = kEmitAvgInt, e.a = slot(kGroupAdd, kGroupSrcCol, ci), slot(kGroupAdd, kGroupSrcOne, -1);
                else if (t == NGX_T_DOUBLE) e.src = kEmitAvgF64, e.a = slot(kGroupAddF64, kGroupSrcCol, ci), slot(kGroupAdd, kGroupSrcOne, -1);
                else constant(e, NGX_CELL_DOUBLE, 0);             // 0 / count
                break;
            case NGX_AGG_MAX:
            case NGX_AGG_MIN: {
                const int32_t op = a.fn == NGX_AGG_MAX ? kGroupMax : kGroupMin;
                if (intLike(t)) e.kind = t, e.src = kEmitState, e.a = slot(op, kGroupSrcCol, ci);
                else if (t == NGX_T_DOUBLE) e.kind = NGX_CELL_DOUBLE, e.src = kEmitOrdered, e.a = slot(op, kGroupSrcOrdered, ci);
                else return fail(c, NGX_E_UNSUPPORTED, "group by: MAX / MIN of a BOOL or STRING column");
                break;
            }
            default:                                              // BIT_*: integers only, anything else is ignored
                if (t == NGX_T_INT)
                    e.kind = NGX_CELL_INT, e.src = kEmitState,
                    e.a = slot(a.fn == NGX_AGG_BIT_AND ? kGroupAnd : a.fn == NGX_AGG_BIT_OR ? kGroupOr : kGroupXor, kGroupSrcCol, ci);
                else constant(e, NGX_CELL_INT, 0);
                break;
        }
    }
    return NGX_OK;
}

// assign + accumulate of a prepared stage with rows (G.n > 0)
void groupAccumulate(ngx_ctx* c, const ngx_group_plan* gp, GroupStage& G) {
    const uint64_t n = G.n;
    std::vector<GroupCol>& cols = G.cols;
    std::vector<GroupSlot>& slots = G.slots;
    std::vector<GroupEmit>& emit = G.emit;
    const std::vector<int32_t>& keyIdx = G.keyIdx;
    const std::vector<int32_t>& distinctCol = G.distinctCol;

    // ---- assign: leaders, group numbers
    uint64_t cap = 1024;
    while (cap < 2 * n) cap <<= 1;
    GroupAssignArgs aa{};
    aa.n = n;
    aa.nk = gp->nkeys;
    for (int32_t k = 0; k < gp->nkeys; k++) aa.k[k] = cols[keyIdx[k]];
    aa.table = c->gbTable.get<uint64_t>(cap);
    aa.mask = cap - 1;
    aa.leader = c->gbLeader.get<uint32_t>(n);
    aa.flag = c->gbFlag.get<uint64_t>(n + 1);
    uint64_t* pre = c->gbPre.get<uint64_t>(n + 1);
    uint64_t* tiles = c->gbTiles.get<uint64_t>((n + kTile - 1) / kTile + 1);
    uint64_t* dflags = c->gbDistinct.get<uint64_t>(std::max<uint64_t>(distinctCol.size(), 1) * n);
    c->timed("group_assign", n * 8 * static_cast<uint64_t>(gp->nkeys), [&] {
        HIP_OK(hipMemsetAsync(aa.table, 0, cap * 8, c->stream));
        if (launchGroupAssign(aa, c->stream)) throw Error{NGX_E_DEVICE, "group assign"};
        if (launchScanU64(aa.flag, n, pre, tiles, c->stream)) throw Error{NGX_E_DEVICE, "group scan"};
        for (size_t d = 0; d < distinctCol.size(); d++) {         // (keys, value) leaders per COUNT_DISTINCT
            GroupAssignArgs da = aa;
            da.k[da.nk++] = cols[distinctCol[d]];
            da.leader = nullptr;
            da.flag = dflags + d * n;
            HIP_OK(hipMemsetAsync(da.table, 0, cap * 8, c->stream));
            if (launchGroupAssign(da, c->stream)) throw Error{NGX_E_DEVICE, "group distinct"};
        }
    });
    const uint64_t ngroups = readScalar(c, pre + n);
    if (ngroups == 0 || ngroups > n) throw Error{NGX_E_DEVICE, "group by: group count out of range"};

    // ---- accumulate
    const size_t descBytes = cols.size() * sizeof(GroupCol) + slots.size() * sizeof(GroupSlot) + emit.size() * sizeof(GroupEmit);
    char* desc = c->gbDesc.get<char>(descBytes);
    GroupCol* colsDev = reinterpret_cast<GroupCol*>(desc);
    GroupSlot* slotsDev = reinterpret_cast<GroupSlot*>(colsDev + cols.size());
    GroupEmit* emitDev = reinterpret_cast<GroupEmit*>(slotsDev + slots.size());
    for (GroupSlot& s : slots)
        if (s.src == kGroupSrcFlag) s.flag = dflags + static_cast<uint64_t>(s.col) * n;
    HIP_OK(hipMemcpyAsync(colsDev, cols.data(), cols.size() * sizeof(GroupCol), hipMemcpyHostToDevice, c->stream));
    if (!slots.empty())
        HIP_OK(hipMemcpyAsync(slotsDev, slots.data(), slots.size() * sizeof(GroupSlot), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(emitDev, emit.data(), emit.size() * sizeof(GroupEmit), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));                      // the host vectors are pageable: copied before they go
    GroupAccumArgs ga{};
    ga.n = n;
    ga.ngroups = ngroups;
    ga.nslots = static_cast<int32_t>(slots.size());
    ga.slots = slotsDev;
    ga.cols = colsDev;
    ga.leader = aa.leader;
    ga.pre = pre;
    ga.state = c->gbState.get<uint64_t>(std::max<uint64_t>(ngroups * slots.size(), 1));
    const uint64_t stateBytes = ngroups * slots.size() * 8;
    // LDS when the workgroup's copy is small next to the rows it folds (by default up to 32 KiB of state)
    const bool lds = !slots.empty() && stateBytes <= kGroupLdsBytes &&
                     (c->groupLdsMax < 0 ? stateBytes <= 32 * 1024 : ngroups <= static_cast<uint64_t>(c->groupLdsMax));
    c->timed(lds ? "group_accum_lds" : "group_accum", n * 8 * (slots.size() + 1), [&] {
        if (launchGroupAccum(ga, lds, c->groupGridMax, c->stream)) throw Error{NGX_E_DEVICE, "group accumulate"};
    });
    G.ngroups = ngroups;
    G.colsDev = colsDev, G.slotsDev = slotsDev, G.emitDev = emitDev;
    G.leader = aa.leader, G.flag = aa.flag, G.pre = pre, G.tiles = tiles, G.state = ga.state;
    G.lds = lds;
}

int32_t groupBy(ngx_ctx* c, const ngx_go_result* r, const ngx_group_plan* gp, GroupResultHolder& R) {
    GroupStage G;
    if (int32_t rc = groupPrepare(c, r, gp, G)) return rc;
    const uint64_t n = G.n;
    const std::vector<GroupCol>& cols = G.cols;
    const std::vector<GroupEmit>& emit = G.emit;
    R.r.ncols = gp->nyields;
    R.colTypes.assign(gp->nyields, 0);
    R.r.col_types = R.colTypes.data();
    if (n == 0) {
        c->groupByDevice++;
        return NGX_OK;
    }
    for (int32_t y = 0; y < gp->nyields; y++) R.colTypes[y] = emit[y].kind;

    resultEvents(c);
    HIP_OK(hipEventRecord(c->gbEv[0], c->stream));
    groupAccumulate(c, gp, G);
    const uint64_t ngroups = G.ngroups;
    uint64_t* tiles = G.tiles;
    const bool lds = G.lds;

    // ---- emit
    GroupEmitArgs ea{};
    ea.n = n;
    ea.ngroups = ngroups;
    ea.ny = gp->nyields;
    ea.emit = G.emitDev;
    ea.cols = G.colsDev;
    ea.flag = G.flag;
    ea.pre = G.pre;
    ea.state = G.state;
    ea.cells = c->gbCells.get<GroupCell>(ngroups * gp->nyields);
    bool anyString = false;
    for (const GroupEmit& e : emit) anyString |= e.src == kEmitKey && cols[e.a].kind == kGroupString;
    uint64_t strBytes = 0;
    if (anyString) {
        uint64_t* slen = c->gbSlen.get<uint64_t>(n + 1);
        uint64_t* spre = c->gbSpre.get<uint64_t>(n + 1);
        if (launchGroupStrLen(ea, slen, c->stream)) throw Error{NGX_E_DEVICE, "group string lengths"};
        if (launchScanU64(slen, n, spre, tiles, c->stream)) throw Error{NGX_E_DEVICE, "group string scan"};
        strBytes = readScalar(c, spre + n);
        ea.strPre = spre;
        ea.strOut = c->gbStr.get<char>(std::max<uint64_t>(strBytes, 1));
    }
    c->timed("group_emit", ngroups * gp->nyields * sizeof(GroupCell), [&] {
        if (launchGroupEmit(ea, c->stream)) throw Error{NGX_E_DEVICE, "group emit"};
    });
    finishCells(c, R, ea.cells, ngroups * gp->nyields, ea.strOut, strBytes);
    R.r.ngroups = ngroups;
    c->groupByDevice++;
    if (lds) c->groupByLds++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_go_group_by(ngx_ctx* c, const ngx_go_result* r, const ngx_group_plan* plan, ngx_group_result** out) {
    if (!c || !r || !plan || !out) return NGX_E_BAD_ARGUMENT;
    return abiCall<GroupResultHolder>(c, out, OnFail::kNoSync, [&](GroupResultHolder& R) { return groupBy(c, r, plan, R); });
}

extern "C" void ngx_group_result_free(ngx_group_result* r) {
    if (r) delete reinterpret_cast<GroupResultHolder*>(r);
}

// ============================================================================ ORDER BY / LIMIT
namespace {

// the word the device orders a double by (orderby.hip kOrdDouble): the winners' host sort uses the same
uint64_t orderDoubleKey(int64_t bits) {
    uint64_t b = static_cast<uint64_t>(bits);
    double d;
    std::memcpy(&d, &b, sizeof d);
    if (d == 0.0) b = 0;
    return b ^ (static_cast<uint64_t>(static_cast<int64_t>(b) >> 63) | 0x8000000000000000ULL);
}

// the plan's own limits, before any column is looked at
int32_t orderPlanCheck(ngx_ctx* c, const ngx_order_plan* op) {
    if (op->nfactors < 0 || (op->nfactors && !op->factors) || op->offset < 0) return fail(c, NGX_E_BAD_ARGUMENT, "order by: factors or offset");
    if (op->count < 0) return fail(c, NGX_E_UNSUPPORTED, "order by: no LIMIT (every row crosses anyway)");
    if (op->nfactors > kOrderMaxFactors) return fail(c, NGX_E_UNSUPPORTED, "order by: more than 8 factors");
    if (op->offset > c->orderKMax || op->count > c->orderKMax - op->offset)
        return fail(c, NGX_E_UNSUPPORTED, "order by: offset + count above order_k_max");
    return NGX_OK;
}

int32_t orderRows(ngx_ctx* c, uint64_t n, int32_t ncols, const int32_t* types, const std::vector<OrderEmitCol>& ecols, bool anyString,
                  const ngx_order_plan* op, bool started, OrderResultHolder& R);

int32_t orderBy(ngx_ctx* c, const ngx_go_result* r, const ngx_order_plan* op, OrderResultHolder& R) {
    if (r->code != NGX_OK || (r->nrows && r->ncols && !r->dev_cols)) return fail(c, NGX_E_BAD_ARGUMENT, "order by: not a device-resident result");
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "order by: world > 1 needs the shards' winners merged");
    if (int32_t rc = orderPlanCheck(c, op)) return rc;
    const uint64_t n = r->nrows;
    if (n >= (1ULL << 32)) return fail(c, NGX_E_UNSUPPORTED, "order by: 2^32 rows or more");
    const int32_t ncols = r->ncols;
    for (int32_t f = 0; f < op->nfactors; f++) {
        const int32_t y = op->factors[f].col;
        if (y < 0 || y >= ncols) return fail(c, NGX_E_BAD_ARGUMENT, "order by: no such result column");
        if (r->col_types[y] == 0 || (n && r->dev_cols[y].type))
            return fail(c, NGX_E_UNSUPPORTED, "order by: UNKNOWN-typed factor column (per-row value types)");
    }
    R.r.input_rows = n;
    R.r.ncols = ncols;
    R.colTypes.assign(r->col_types, r->col_types + ncols);
    R.r.col_types = R.colTypes.data();
    if (op->count == 0 || static_cast<uint64_t>(op->offset) >= n || ncols == 0) {   // the column names and no rows: nothing to launch
        c->orderByDevice++;
        return NGX_OK;
    }

    // every column as the emit kernel reads it; the factors' among them feed the levels
    std::vector<OrderEmitCol> ecols(ncols);
    bool anyString = false;
    for (int32_t y = 0; y < ncols; y++) {
        const int32_t t = r->col_types[y];
        OrderEmitCol& e = ecols[y];
        e.type = r->dev_cols[y].type;
        if (t == 0 && !e.type) return fail(c, NGX_E_UNSUPPORTED, "order by: a column of UNKNOWN type without per-row types");
        e.cell = t;                                               // NGX_CELL_* numbers its kinds as NGX_T_*
        e.c.kind = t == NGX_T_STRING ? kGroupString : t == NGX_T_DOUBLE || t == NGX_T_FLOAT ? kGroupDouble : kGroupInt;
        e.c.w = e.type || t == NGX_T_STRING || t == NGX_T_DOUBLE || t == NGX_T_FLOAT ? 8 : r->dev_col_w ? r->dev_col_w[y] : 8;
        e.c.konst = r->dev_col_const ? r->dev_col_const[y] : 0;
        e.c.x = e.c.w ? r->dev_cols[y].x : nullptr;
        e.c.len = r->dev_cols[y].len;
        if (e.c.w && !e.c.x) return fail(c, NGX_E_BAD_ARGUMENT, "order by: column without values");
        if (e.c.w != 0 && e.c.w != 1 && e.c.w != 2 && e.c.w != 4 && e.c.w != 8) return fail(c, NGX_E_BAD_ARGUMENT, "order by: column width");
        anyString |= t == NGX_T_STRING || e.type != nullptr;
    }
    if (int32_t rc = orderRows(c, n, ncols, r->col_types, ecols, anyString, op, false, R)) return rc;
    c->orderByDevice++;
    return NGX_OK;
}

// Levels -> select -> emit -> host sort of the winners, over n rows of ncols columns as the kernels read them
// (a GO result's columns for ngx_go_order_by, the group columns for ngx_go_group_order_by; types: NGX_T_* per
// column). The window has rows (count > 0, offset < n, ncols > 0). started: the caller recorded gbEv[0] already
// and device_ms counts from there.
int32_t orderRows(ngx_ctx* c, uint64_t n, int32_t ncols, const int32_t* types, const std::vector<OrderEmitCol>& ecols, bool anyString,
                  const ngx_order_plan* op, bool started, OrderResultHolder& R) {
    const uint64_t offset = static_cast<uint64_t>(op->offset), K = offset + static_cast<uint64_t>(op->count);
    std::vector<GroupCol> cols(ncols);
    for (int32_t y = 0; y < ncols; y++) cols[y] = ecols[y].c;

    resultEvents(c);
    if (!started) HIP_OK(hipEventRecord(c->gbEv[0], c->stream));

    // ---- the levels: per factor its words, then the row index
    std::vector<OrderLevel> levels;
    auto bitsFor = [](uint64_t maxValue) {
        int32_t bits = 8;
        while (bits < 64 && (maxValue >> bits)) bits += 8;
        return bits;
    };
    for (int32_t f = 0; f < op->nfactors; f++) {
        const int32_t y = op->factors[f].col, t = types[y];
        const int32_t desc = op->factors[f].desc ? 1 : 0;
        if (t == NGX_T_STRING) {
            uint32_t* mx = c->obMax.get<uint32_t>(1);
            if (launchOrderMaxLen(cols[y].len, n, mx, c->stream)) throw Error{NGX_E_DEVICE, "order max length"};
            const uint32_t maxLen = readScalar(c, mx);
            if (maxLen > kOrderMaxStr) return fail(c, NGX_E_UNSUPPORTED, "order by: a factor string longer than 256 bytes");
            for (uint32_t w = 0; w < (maxLen + 7) / 8; w++) levels.push_back(OrderLevel{y, kOrdStrWord, static_cast<int32_t>(w), desc, 64, 0});
            if (maxLen) levels.push_back(OrderLevel{y, kOrdStrLen, 0, desc, bitsFor(maxLen), 0});
        } else if ((t == NGX_T_DOUBLE || t == NGX_T_FLOAT) && cols[y].w) {
            levels.push_back(OrderLevel{y, kOrdDouble, 0, desc, 64, 0});
        } else if (cols[y].w) {                                   // width 0: a constant ties every row
            levels.push_back(OrderLevel{y, kOrdInt, 0, desc, cols[y].w * 8, 0});
        }
    }
    const bool select = !levels.empty() && K < n;                 // else the winners are a range of rows as stored
    levels.push_back(OrderLevel{0, kOrdRow, 0, 0, bitsFor(n - 1), 0});

    // ---- descriptors
    const size_t descBytes = cols.size() * sizeof(GroupCol) + ecols.size() * sizeof(OrderEmitCol) + levels.size() * sizeof(OrderLevel);
    char* desc = c->obDesc.get<char>(descBytes);
    OrderEmitCol* ecolsDev = reinterpret_cast<OrderEmitCol*>(desc);
    GroupCol* colsDev = reinterpret_cast<GroupCol*>(ecolsDev + ecols.size());
    OrderLevel* levelsDev = reinterpret_cast<OrderLevel*>(colsDev + cols.size());
    HIP_OK(hipMemcpyAsync(ecolsDev, ecols.data(), ecols.size() * sizeof(OrderEmitCol), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(colsDev, cols.data(), cols.size() * sizeof(GroupCol), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(levelsDev, levels.data(), levels.size() * sizeof(OrderLevel), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));                      // the host vectors are pageable: copied before they go

    // ---- select: the rows of the K first places, in no order
    OrderEmitArgs ea{};
    ea.n = n;
    ea.ncols = ncols;
    ea.cols = ecolsDev;
    if (select) {
        OrderArgs oa{};
        oa.n = n;
        oa.cols = colsDev;
        oa.levels = levelsDev;
        oa.nlevels = static_cast<int32_t>(levels.size());
        oa.mark = c->obMark.get<uint8_t>(n);
        oa.listCap = n / kOrderCompactDiv + 1;
        oa.list[0] = c->obList[0].get<uint32_t>(oa.listCap);
        oa.list[1] = c->obList[1].get<uint32_t>(oa.listCap);
        oa.hist = c->obHist.get<uint64_t>(256);
        oa.S = c->obState.get<OrderState>(1);
        oa.win = c->obWin.get<uint32_t>(K);
        oa.winCap = K;
        oa.gridMax = c->orderGridMax;
        OrderState st{};
        st.rank = K - 1;
        st.nTied = n;
        HIP_OK(hipMemsetAsync(oa.mark, kOrdTied, n, c->stream));
        HIP_OK(hipMemsetAsync(oa.hist, 0, 256 * sizeof(uint64_t), c->stream));
        HIP_OK(hipMemcpyAsync(oa.S, &st, sizeof st, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));                  // st is on the stack
        uint64_t bytes = 0;
        for (const OrderLevel& L : levels) bytes += n * static_cast<uint64_t>(L.bits / 8 + 1);   // upper bound: every step over all rows
        c->timed("order_select", bytes, [&] {
            for (size_t l = 0; l < levels.size(); l++) {
                for (int shift = levels[l].bits - 8; shift >= 0; shift -= 8)
                    if (launchOrderStep(oa, static_cast<int>(l), shift, l + 1 == levels.size() && shift == 0, c->stream))
                        throw Error{NGX_E_DEVICE, "order step"};
                HIP_OK(hipMemcpyAsync(&st, oa.S, sizeof st, hipMemcpyDeviceToHost, c->stream));   // once per level, not per digit
                HIP_OK(hipStreamSynchronize(c->stream));
                if (st.err) throw Error{NGX_E_DEVICE, "order by: inconsistent counts"};
                if (st.done) break;
            }
            if (launchOrderGather(oa, c->stream)) throw Error{NGX_E_DEVICE, "order gather"};
        });
        HIP_OK(hipMemcpyAsync(&st, oa.S, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        c->orderCompactions += st.compactions;
        c->orderListCompactions += st.listCompactions;
        c->orderLoopFlushes += st.loopFlushes;
        if (st.err || !st.done || st.nWin != K) throw Error{NGX_E_DEVICE, "order by: winner count out of range"};
        ea.rows = oa.win;
        ea.m = K;
    } else if (levels.size() == 1) {                              // LIMIT alone, or only constant factors: rows as stored
        ea.base = offset;
        ea.m = std::min(K, n) - offset;
    } else {                                                      // K >= n: every row, ordered below
        ea.m = n;
    }
    const uint64_t m = ea.m;

    // ---- emit
    ea.cells = c->obCells.get<GroupCell>(m * ncols);
    uint64_t strBytes = 0;
    if (anyString) {
        uint64_t* slen = c->obSlen.get<uint64_t>(m + 1);
        uint64_t* spre = c->obSpre.get<uint64_t>(m + 1);
        uint64_t* tiles = c->obTiles.get<uint64_t>((m + kTile - 1) / kTile + 1);
        if (launchOrderStrLen(ea, slen, c->stream)) throw Error{NGX_E_DEVICE, "order string lengths"};
        if (launchScanU64(slen, m, spre, tiles, c->stream)) throw Error{NGX_E_DEVICE, "order string scan"};
        strBytes = readScalar(c, spre + m);
        ea.strPre = spre;
        ea.strOut = c->obStr.get<char>(std::max<uint64_t>(strBytes, 1));
    }
    c->timed("order_emit", m * ncols * sizeof(GroupCell) + strBytes, [&] {
        if (launchOrderEmit(ea, c->stream)) throw Error{NGX_E_DEVICE, "order emit"};
    });
    std::vector<uint32_t> rows(m);
    finishCells(c, R, ea.cells, m * ncols, ea.strOut, strBytes, [&] {
        if (ea.rows) HIP_OK(hipMemcpyAsync(rows.data(), ea.rows, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    });
    std::vector<ngx_cell> cells = std::move(R.cells);                 // the winners as emitted; R.cells takes them in order
    R.cells.clear();

    // ---- the winners in order (factors, then the row index), less the first `offset`
    const auto t0 = std::chrono::steady_clock::now();
    if (levels.size() == 1) {
        R.cells = std::move(cells);
    } else {
        if (!ea.rows)
            for (uint64_t i = 0; i < m; i++) rows[i] = static_cast<uint32_t>(i);
        std::vector<uint32_t> perm(m);
        for (uint64_t i = 0; i < m; i++) perm[i] = static_cast<uint32_t>(i);
        const char* sbase = R.strings.data();
        auto less = [&](uint32_t a, uint32_t b) {
            for (int32_t f = 0; f < op->nfactors; f++) {
                const int32_t y = op->factors[f].col, t = types[y];
                const ngx_cell* x = &cells[static_cast<uint64_t>(a) * ncols + y];
                const ngx_cell* z = &cells[static_cast<uint64_t>(b) * ncols + y];
                if (op->factors[f].desc) std::swap(x, z);
                if (t == NGX_T_STRING) {
                    const size_t common = static_cast<size_t>(std::min(x->str_len, z->str_len));
                    const int cmp = common ? std::memcmp(sbase + x->v.str_off, sbase + z->v.str_off, common) : 0;
                    if (cmp) return cmp < 0;
                    if (x->str_len != z->str_len) return x->str_len < z->str_len;
                } else if (t == NGX_T_DOUBLE || t == NGX_T_FLOAT) {
                    const uint64_t kx = orderDoubleKey(x->v.i), kz = orderDoubleKey(z->v.i);
                    if (kx != kz) return kx < kz;
                } else if (x->v.i != z->v.i) {
                    return x->v.i < z->v.i;
                }
            }
            return rows[a] < rows[b];
        };
        std::sort(perm.begin(), perm.end(), less);
        const uint64_t keep = m > offset ? m - offset : 0;
        R.cells.resize(keep * ncols);
        for (uint64_t i = 0; i < keep; i++)
            std::memcpy(&R.cells[i * ncols], &cells[static_cast<uint64_t>(perm[offset + i]) * ncols], ncols * sizeof(ngx_cell));
    }
    R.r.host_sort_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    R.r.nrows = ncols ? R.cells.size() / ncols : 0;
    R.r.cells = R.cells.data();
    R.r.strings = R.strings.data();
    R.r.strings_len = strBytes;
    return NGX_OK;
}

// GO | GROUP BY | [ORDER BY |] LIMIT: the grouping's state becomes columns (k_group_columns) and the select
// reads those; only the window's group rows cross.
int32_t groupOrderBy(ngx_ctx* c, const ngx_go_result* r, const ngx_group_plan* gp, const ngx_order_plan* op, OrderResultHolder& R) {
    GroupStage G;
    if (int32_t rc = groupPrepare(c, r, gp, G)) return rc;
    if (int32_t rc = orderPlanCheck(c, op)) return rc;
    const int32_t ny = gp->nyields;
    for (int32_t f = 0; f < op->nfactors; f++)
        if (op->factors[f].col < 0 || op->factors[f].col >= ny) return fail(c, NGX_E_BAD_ARGUMENT, "order by: no such result column");
    const uint64_t n = G.n;
    R.r.ncols = ny;
    R.colTypes.assign(ny, 0);
    R.r.col_types = R.colTypes.data();
    if (n == 0) {                                                 // no groups: nothing to launch
        c->groupOrderDevice++;
        return NGX_OK;
    }
    for (int32_t y = 0; y < ny; y++) R.colTypes[y] = G.emit[y].kind;

    resultEvents(c);
    HIP_OK(hipEventRecord(c->gbEv[0], c->stream));
    groupAccumulate(c, gp, G);
    const uint64_t ngroups = G.ngroups;
    R.r.input_rows = ngroups;

    // ---- the group rows as columns: a COUNT / COUNT_DISTINCT lies in [0, n] and takes the narrowest signed
    // width that holds n (the select pays one step per byte of an integer factor); the rest 8 bytes
    const int32_t countW = n <= 0x7F ? 1 : n <= 0x7FFF ? 2 : n <= 0x7FFFFFFF ? 4 : 8;
    std::vector<GroupColumnOut> outs(ny);
    std::vector<OrderEmitCol> ecols(ny);
    uint64_t colBytes = 0, lenCols = 0;
    bool anyString = false;
    for (int32_t y = 0; y < ny; y++) {
        const GroupEmit& e = G.emit[y];
        OrderEmitCol& oc = ecols[y];
        oc.cell = e.kind;                                         // NGX_CELL_* numbers its kinds as NGX_T_*
        oc.c.kind = e.kind == NGX_T_STRING ? kGroupString : e.kind == NGX_T_DOUBLE ? kGroupDouble : kGroupInt;
        oc.c.konst = e.konst;
        oc.c.w = e.src == kEmitConst ? 0 : G.isCount[y] ? countW : 8;
        outs[y].w = oc.c.w;
        colBytes += (ngroups * static_cast<uint64_t>(oc.c.w) + 7) / 8 * 8;
        if (oc.c.kind == kGroupString) lenCols++, anyString = true;
    }
    char* colMem = c->goCols.get<char>(std::max<uint64_t>(colBytes, 1));
    uint32_t* lenMem = c->goLen.get<uint32_t>(std::max<uint64_t>(lenCols * ngroups, 1));
    uint64_t at = 0, lenAt = 0;
    for (int32_t y = 0; y < ny; y++) {
        OrderEmitCol& oc = ecols[y];
        if (!oc.c.w) continue;
        outs[y].x = colMem + at;
        oc.c.x = outs[y].x;
        at += (ngroups * static_cast<uint64_t>(oc.c.w) + 7) / 8 * 8;
        if (oc.c.kind == kGroupString) {
            outs[y].len = lenMem + lenAt;
            oc.c.len = outs[y].len;
            lenAt += ngroups;
        }
    }
    GroupColumnOut* outsDev = c->goDesc.get<GroupColumnOut>(ny);
    HIP_OK(hipMemcpyAsync(outsDev, outs.data(), outs.size() * sizeof(GroupColumnOut), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));                      // the host vector is pageable: copied before it goes
    GroupColumnsArgs ca{};
    ca.n = n;
    ca.ngroups = ngroups;
    ca.ny = ny;
    ca.emit = G.emitDev;
    ca.cols = G.colsDev;
    ca.flag = G.flag;
    ca.pre = G.pre;
    ca.state = G.state;
    ca.out = outsDev;
    c->timed("group_columns", n * 8 + colBytes + lenCols * ngroups * 4, [&] {
        if (launchGroupColumns(ca, c->stream)) throw Error{NGX_E_DEVICE, "group columns"};
    });

    int32_t rc = NGX_OK;
    if (op->count != 0 && static_cast<uint64_t>(op->offset) < ngroups)
        rc = orderRows(c, ngroups, ny, R.colTypes.data(), ecols, anyString, op, true, R);
    else
        HIP_OK(hipStreamSynchronize(c->stream));
    c->collectTimings();
    if (rc) return rc;
    c->groupOrderDevice++;
    if (G.lds) c->groupByLds++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_go_order_by(ngx_ctx* c, const ngx_go_result* r, const ngx_order_plan* plan, ngx_order_result** out) {
    if (!c || !r || !plan || !out) return NGX_E_BAD_ARGUMENT;
    // after an Error no kernel is left reading the descriptors
    return abiCall<OrderResultHolder>(c, out, OnFail::kSyncIfThrown, [&](OrderResultHolder& R) { return orderBy(c, r, plan, R); });
}

extern "C" void ngx_order_result_free(ngx_order_result* r) {
    if (r) delete reinterpret_cast<OrderResultHolder*>(r);
}

extern "C" int32_t ngx_go_group_order_by(ngx_ctx* c, const ngx_go_result* r, const ngx_group_plan* group, const ngx_order_plan* order,
                                         ngx_order_result** out) {
    if (!c || !r || !group || !order || !out) return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left reading the descriptors
    return abiCall<OrderResultHolder>(c, out, OnFail::kSync, [&](OrderResultHolder& R) { return groupOrderBy(c, r, group, order, R); });
}

