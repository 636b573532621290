// FETCH PROP ON tags and edges (ngx_fetch, ngx_go_fetch): the host driver of fetch.hip.
#include "engine_ctx.h"

// ------------------------------------------------------------------------ FETCH PROP ON (ngx_fetch, ngx_go_fetch)
namespace {

using FetchResultHolder = CellResult<ngx_fetch_result>;

bool fetchIntType(int32_t t) { return t == NGX_T_INT || t == NGX_T_VID || t == NGX_T_TIMESTAMP; }

// Every refusal and every prepare-time error is decided before the first launch.
int32_t fetchOp(ngx_ctx* c, const ngx_go_result* r, const ngx_fetch_plan* p, FetchResultHolder& R) {
    if (p->kind != NGX_FETCH_VERTEX && p->kind != NGX_FETCH_EDGE) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: unknown kind");
    if (r && (r->code != NGX_OK || (r->nrows && r->ncols && !r->dev_cols))) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: not a device-resident result");
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "fetch: world > 1 needs the keys sent to their owners");
    Space* spp = findSpace(c, p->space);
    if (!spp || !spp->dev) return fail(c, NGX_E_NOT_LOADED, "space not committed");
    const Space& sp = *spp;
    const DeviceGraph& d = *sp.dev;
    const bool edge = p->kind == NGX_FETCH_EDGE;
    const int nkey = edge ? 3 : 1;
    if (p->nyields < 0 || p->nyields + nkey > kFetchMaxCols) return fail(c, NGX_E_UNSUPPORTED, "fetch: more than 16 columns");
    if (p->nyields && !p->yields) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: yields missing");
    // ---- ON
    std::vector<int32_t> tagSlot;
    const SchemaSet* es = nullptr;
    int32_t eslot = -1;
    if (!edge) {
        if (p->ntags == 0) return fail(c, NGX_E_UNSUPPORTED, "fetch: ON * (the column set depends on every tag of the space)");
        if (p->ntags < 0 || !p->tags) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: tags missing");
        if (p->ntags > kFetchMaxTags) return fail(c, NGX_E_UNSUPPORTED, "fetch: more than 8 tags");
        for (int32_t t = 0; t < p->ntags; t++) {
            const SchemaSet* ts = sp.tag(p->tags[t]);
            if (!ts) return fail(c, NGX_E_QUERY, "Unknown error(406): ");               // Status::TagNotFound()
            for (int32_t u = 0; u < t; u++)
                if (p->tags[u] == p->tags[t]) return fail(c, NGX_E_QUERY, "tag(" + ts->name + ") was dup");
            int32_t col;
            int64_t dur;
            if (ttlInfo(ts, col, dur)) return fail(c, NGX_E_UNSUPPORTED, "fetch: a TTL tag schema");
            tagSlot.push_back(sp.tagSlotOf(p->tags[t]));
        }
    } else {
        es = sp.edge(std::abs(p->edge_type));
        if (!es || p->edge_type <= 0) return fail(c, NGX_E_QUERY, "Unknown error(407): ");  // Status::EdgeNotFound()
        int32_t col;
        int64_t dur;
        if (ttlInfo(es, col, dur)) return fail(c, NGX_E_UNSUPPORTED, "fetch: a TTL edge schema");
        eslot = sp.slotOf(p->edge_type);
        if (eslot >= 0 && d.slots[eslot].hasFlags) return fail(c, NGX_E_UNSUPPORTED, "fetch: edges with empty or unreadable values");
    }
    if (edge && p->distinct && r) return fail(c, NGX_E_UNSUPPORTED, "fetch: DISTINCT over device-resident edge keys");
    // ---- keys
    const uint64_t n = r ? r->nrows : p->nkeys;
    if (n >= (1ULL << 31)) return fail(c, NGX_E_UNSUPPORTED, "fetch: 2^31 keys or more");
    const int nk = edge ? (p->key_cols[2] >= 0 ? 3 : 2) : 1;
    const bool hasRank = edge && p->key_cols[2] >= 0;
    auto inputCol = [&](int32_t col, GroupCol& g, int32_t& type, bool keyCol) -> int32_t {
        if (!r) {                                                 // host keys: column k is key array k
            if (col < 0 || col >= nk) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: input column out of range");
            type = col == 2 ? NGX_T_INT : NGX_T_VID;
            g = GroupCol{nullptr, nullptr, 0, 8, kGroupInt};
            return NGX_OK;
        }
        if (col < 0 || col >= r->ncols) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: input column out of range");
        type = r->col_types[col];
        if (type == 0 || (r->nrows && r->dev_cols[col].type))
            return fail(c, NGX_E_UNSUPPORTED, "fetch: UNKNOWN-typed column (per-row value types)");
        if (keyCol && !fetchIntType(type)) return fail(c, NGX_E_UNSUPPORTED, "fetch: a non-integer key column");
        const bool wide = type == NGX_T_STRING || type == NGX_T_DOUBLE || type == NGX_T_FLOAT;
        g.kind = type == NGX_T_STRING ? kGroupString : wide ? kGroupDouble : kGroupInt;
        g.w = wide ? 8 : r->dev_col_w ? r->dev_col_w[col] : 8;
        g.konst = r->dev_col_const ? r->dev_col_const[col] : 0;
        g.x = nullptr;
        g.len = nullptr;
        if (r->nrows) {
            g.x = g.w ? r->dev_cols[col].x : nullptr;
            g.len = r->dev_cols[col].len;
            if (g.w && !g.x) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: column without values");
            if (g.w != 0 && g.w != 1 && g.w != 2 && g.w != 4 && g.w != 8) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: column width");
            if (type == NGX_T_STRING && !g.len) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: string column without lengths");
        }
        return NGX_OK;
    };
    FetchArgs a{};
    int32_t keyType[3] = {NGX_T_VID, NGX_T_VID, NGX_T_INT};
    for (int k = 0; k < nk; k++) {
        int32_t t;
        if (int32_t rc = inputCol(r ? p->key_cols[k] : k, a.key[k], t, true)) return rc;
    }
    if (!r && n) {
        const int64_t* src[3] = {p->key_vid, p->key_dst, p->key_rank};
        for (int k = 0; k < nk; k++)
            if (!src[k]) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: key array missing");
    }
    // ---- yields
    std::vector<FetchYield> ys(p->nyields);
    R.colTypes.assign(keyType, keyType + nkey);
    bool anyString = false;
    for (int32_t y = 0; y < p->nyields; y++) {
        const ngx_fetch_yield& q = p->yields[y];
        FetchYield& f = ys[y];
        f = FetchYield{};
        int32_t type = NGX_T_INT;
        if (q.kind == NGX_FY_TAG_PROP && !edge) {
            int32_t t = 0;
            while (t < p->ntags && p->tags[t] != q.tag) t++;
            if (t == p->ntags) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: a yield's tag is not in ON");
            const SchemaSet* ts = sp.tag(q.tag);
            const std::string field = q.field ? q.field : "";
            const int32_t fi = ts->latest().index(field);
            if (fi < 0) return fail(c, NGX_E_QUERY, "`" + ts->name + "' is not a prop of `" + field + "'");
            type = ts->latest().fields[fi].type;
            f.src = kFyTagProp;
            f.a = t;
            if (tagSlot[t] >= 0) f.col = d.cols[d.tags[tagSlot[t]].colBase + fi];
        } else if (q.kind == NGX_FY_EDGE_PROP && edge) {
            const std::string field = q.field ? q.field : "";
            const int32_t fi = es->latest().index(field);
            if (fi < 0) return fail(c, NGX_E_QUERY, "`" + field + "' is not a prop of `" + es->name + "'");
            type = es->latest().fields[fi].type;
            f.src = kFyEdgeProp;
            if (eslot >= 0) f.col = d.cols[d.slots[eslot].colBase + fi];
        } else if (q.kind == NGX_FY_EDGE_KEY && edge) {
            if (q.key < NGX_EK_SRC || q.key > NGX_EK_TYPE) return fail(c, NGX_E_BAD_ARGUMENT, "fetch: unknown key prop");
            type = q.key <= NGX_EK_DST ? NGX_T_VID : NGX_T_INT;
            f.src = q.key == NGX_EK_TYPE ? kFyEdgeType : kFyKey;
            f.a = q.key;
            f.konst = p->edge_type;
        } else if (q.kind == NGX_FY_INPUT_COL) {
            f.src = kFyInput;
            if (int32_t rc = inputCol(q.col, f.in, type, false)) return rc;
            f.a = q.col;
        } else {
            return fail(c, NGX_E_UNSUPPORTED, "fetch: a YIELD column that is no plain prop, key prop or input column");
        }
        if (type != NGX_T_BOOL && !fetchIntType(type) && type != NGX_T_FLOAT && type != NGX_T_DOUBLE && type != NGX_T_STRING)
            return fail(c, NGX_E_UNSUPPORTED, "fetch: a column of an unknown type");
        f.cell = type;                                            // NGX_CELL_* numbers its kinds as NGX_T_*
        anyString |= type == NGX_T_STRING;
        R.colTypes.push_back(type);
    }
    const int32_t ncols = nkey + p->nyields;
    R.r.ncols = ncols;
    R.r.col_types = R.colTypes.data();
    R.r.input_rows = n;
    if (n == 0) {                                                 // onEmptyInputs: the columns and no rows
        c->fetchDevice++;
        return NGX_OK;
    }

    resultEvents(c);
    const hipEvent_t ev0 = c->gbEv[0], ev1 = c->gbEv[1];
    HIP_OK(hipEventRecord(ev0, c->stream));
    if (!r) {
        const int64_t* src[3] = {p->key_vid, p->key_dst, p->key_rank};
        for (int k = 0; k < nk; k++) {
            int64_t* dev = c->fxKeys[k].get<int64_t>(n);
            HIP_OK(hipMemcpyAsync(dev, src[k], n * 8, hipMemcpyHostToDevice, c->stream));
            a.key[k].x = dev;
        }
        for (FetchYield& f : ys)
            if (f.src == kFyInput) f.in = a.key[f.a];
    }
    const uint64_t chunks = (n + 255) / 256;
    a.n = n;
    a.edge = edge ? 1 : 0;
    a.nparts = sp.numParts;
    a.hasRank = hasRank ? 1 : 0;
    a.ntags = edge ? 0 : p->ntags;
    a.vindex = d.vindex;
    for (int32_t t = 0; t < a.ntags; t++) a.present[t] = tagSlot[t] >= 0 ? d.tags[tagSlot[t]].present : nullptr;
    if (eslot >= 0) a.slot = d.slots[eslot];
    a.keepMissing = !edge && p->keep_missing ? 1 : 0;
    a.ny = p->nyields;
    FetchYield* ysDev = c->fxDesc.get<FetchYield>(std::max<size_t>(ys.size(), 1));
    if (!ys.empty()) HIP_OK(hipMemcpyAsync(ysDev, ys.data(), ys.size() * sizeof(FetchYield), hipMemcpyHostToDevice, c->stream));
    a.ys = ysDev;
    a.row = c->fxRow.get<uint32_t>(n);
    a.eidx = c->fxEidx.get<uint64_t>(edge ? n : 1);
    a.hits = c->fxHits.get<uint16_t>(n);
    a.chunkCount = c->fxCount.get<uint64_t>(chunks + 1);
    uint64_t* base = c->fxBase.get<uint64_t>(chunks + 1);
    uint64_t* tiles = c->fxTiles.get<uint64_t>((chunks + kTile - 1) / kTile + 1);
    a.chunkBase = base;
    a.seen = c->fxSeen.get<uint32_t>(1);
    a.gridMax = c->fetchGridMax;
    HIP_OK(hipMemsetAsync(a.seen, 0, sizeof(uint32_t), c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));                      // ys and the host keys are pageable: copied before they go
    uint64_t keyBytes = 0;
    for (int k = 0; k < nk; k++) keyBytes += n * static_cast<uint64_t>(a.key[k].w);
    c->timed("fetch_keys", keyBytes + n * (16 + 4 + 2 + (edge ? 8 : 0)), [&] {
        if (launchFetchKeys(a, c->stream)) throw Error{NGX_E_DEVICE, "fetch keys"};
    });
    uint64_t m = 0;
    c->timed("fetch_scan", chunks * 16, [&] {
        if (launchScanU64(a.chunkCount, chunks, base, tiles, c->stream)) throw Error{NGX_E_DEVICE, "fetch scan"};
    });
    m = readScalar(c, base + chunks);
    if (m > n) throw Error{NGX_E_DEVICE, "fetch: inconsistent counts"};
    uint32_t seen = readScalar(c, a.seen);
    R.r.tags_seen = seen;
    if (m == 0) {
        HIP_OK(hipEventRecord(ev1, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        float ms0 = 0;
        HIP_OK(hipEventElapsedTime(&ms0, ev0, ev1));
        c->collectTimings();
        R.r.device_ms = ms0;
        c->fetchDevice++;
        return NGX_OK;
    }
    uint64_t strBytes = 0;
    if (anyString) {
        uint64_t* slen = c->fxSlen.get<uint64_t>(m + 1);
        uint64_t* spre = c->fxSpre.get<uint64_t>(m + 1);
        uint64_t* stiles = c->fxTiles.get<uint64_t>(std::max((m + kTile - 1) / kTile + 1, (chunks + kTile - 1) / kTile + 1));
        a.lenOut = slen;
        c->timed("fetch_emit", m * 8, [&] {
            if (launchFetchEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "fetch string lengths"};
        });
        c->timed("fetch_scan", m * 16, [&] {
            if (launchScanU64(slen, m, spre, stiles, c->stream)) throw Error{NGX_E_DEVICE, "fetch string scan"};
        });
        strBytes = readScalar(c, spre + m);
        a.lenOut = nullptr;
        a.strPre = spre;
        a.strOut = c->fxStr.get<char>(std::max<uint64_t>(strBytes, 1));
    }
    a.cells = c->fxCells.get<GroupCell>(m * ncols);
    c->timed("fetch_emit", m * ncols * sizeof(GroupCell) + strBytes, [&] {
        if (launchFetchEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "fetch emit"};
    });
    finishCells(c, R, a.cells, m * ncols, a.strOut, strBytes);
    R.r.nrows = m;
    c->fetchDevice++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_fetch(ngx_ctx* c, const ngx_go_result* r, const ngx_fetch_plan* plan, ngx_fetch_result** out) {
    if (!c || !plan || !out) return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left reading the descriptors
    return abiCall<FetchResultHolder>(c, out, OnFail::kSync, [&](FetchResultHolder& R) { return fetchOp(c, r, plan, R); });
}

extern "C" void ngx_fetch_result_free(ngx_fetch_result* r) {
    if (r) delete reinterpret_cast<FetchResultHolder*>(r);
}

// The GO with its result left in HBM, then ngx_fetch over its columns, then the result freed: the traversal's rows
// never cross to the host.
extern "C" int32_t ngx_go_fetch(ngx_ctx* c, const ngx_go_plan* go, const ngx_fetch_plan* plan, ngx_fetch_result** out) {
    if (!c || !go || !plan || !out) return NGX_E_BAD_ARGUMENT;
    return abiCall<FetchResultHolder>(c, out, OnFail::kNoSync, [&](FetchResultHolder& R) {
        ngx_go_result* gr = nullptr;
        int32_t rc = NGX_OK;
        if (!go->result_on_device || go->distinct || go->input_vid_col)
            rc = fail(c, NGX_E_BAD_ARGUMENT, "fetch: the plan is a device-resident GO without DISTINCT or input");
        else if (c->world > 1)
            rc = fail(c, NGX_E_UNSUPPORTED, "fetch: world > 1 needs the keys sent to their owners");
        if (rc == NGX_OK) {
            if (c->activeLane != 0) c->useLane(0);
            rc = goCall(c, go, &gr);
        }
        if (rc == NGX_OK) rc = guarded(c, OnFail::kSync, [&] { return fetchOp(c, gr, plan, R); });
        const std::string err = c->lastError;
        if (gr) ngx_go_result_free(gr);
        c->lastError = err;
        return rc;
    });
}

