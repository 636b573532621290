// LOOKUP ON tags and edges (ngx_lookup): the host driver of lookup.hip.
#include "engine_ctx.h"

// ------------------------------------------------------------------------ LOOKUP ON (ngx_lookup)
namespace {

using LookupResultHolder = CellResult<ngx_lookup_result>;

int32_t lookupKindOf(int32_t t) {
    switch (t) {
        case NGX_T_BOOL: return kLkBool;
        case NGX_T_INT: case NGX_T_VID: case NGX_T_TIMESTAMP: return kLkInt;
        case NGX_T_FLOAT: case NGX_T_DOUBLE: return kLkDouble;
        case NGX_T_STRING: return kLkString;
        default: return -1;
    }
}

// Every refusal but one is decided before the first launch; an output above lookup_rows_max is known only after
// the keep and scan passes and is refused before the emit. Nothing enumerates the Engine's rows on the host, so a
// refusal is the caller's error: there is no host leg to fall back to (FETCH has one).
// keep_bytes is the columns' stored widths times the rows scanned: an upper estimate for fixed-width columns (a row
// rejected by an earlier condition does not read the later ones) and a lower one for a STRING condition, which
// counts its two offsets' 8 bytes and not the string bytes compared.
int32_t lookupOp(ngx_ctx* c, const ngx_lookup_plan* p, LookupResultHolder& R) {
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "lookup: world > 1 needs every shard's rows concatenated");
    Space* spp = findSpace(c, p->space);
    if (!spp || !spp->dev) return fail(c, NGX_E_NOT_LOADED, "space not committed");
    const Space& sp = *spp;
    const DeviceGraph& d = *sp.dev;
    const bool edge = p->is_edge != 0;
    const int nkey = edge ? 3 : 1;
    if (p->nfields < 0 || p->nterms < 0 || p->nyields < 0) return fail(c, NGX_E_BAD_ARGUMENT, "lookup: negative count");
    if (p->nfields > kLookupMax) return fail(c, NGX_E_UNSUPPORTED, "lookup: more than 16 scanned fields");
    if (p->nterms > kLookupMax) return fail(c, NGX_E_UNSUPPORTED, "lookup: more than 16 residual terms");
    if (p->nyields + nkey > kLookupMax) return fail(c, NGX_E_UNSUPPORTED, "lookup: more than 16 columns");
    if ((p->nfields && !p->fields) || (p->nterms && !p->terms) || (p->nyields && !p->yields))
        return fail(c, NGX_E_BAD_ARGUMENT, "lookup: array missing");
    const SchemaSet* ss = edge ? sp.edge(p->schema_id) : sp.tag(p->schema_id);
    if (!ss || (edge && p->schema_id <= 0)) return fail(c, NGX_E_QUERY, edge ? "Unknown error(407): " : "Unknown error(406): ");
    int32_t tcol;
    int64_t tdur;
    if (ttlInfo(ss, tcol, tdur)) return fail(c, NGX_E_UNSUPPORTED, edge ? "lookup: a TTL edge schema" : "lookup: a TTL tag schema");
    const int32_t slot = edge ? sp.slotOf(p->schema_id) : sp.tagSlotOf(p->schema_id);
    if (edge && slot >= 0 && d.slots[slot].hasFlags) return fail(c, NGX_E_UNSUPPORTED, "lookup: edges with empty or unreadable values");
    const int32_t colBase = slot < 0 ? 0 : edge ? d.slots[slot].colBase : d.tags[slot].colBase;
    auto column = [&](const char* name, DCol& col, int32_t& type) -> int32_t {
        const std::string field = name ? name : "";
        const int32_t fi = ss->latest().index(field);
        if (fi < 0) return fail(c, NGX_E_QUERY, "Unknown column `" + field + "' in schema");
        type = ss->latest().fields[fi].type;
        if (lookupKindOf(type) < 0) return fail(c, NGX_E_UNSUPPORTED, "lookup: a column of an unknown type");
        col = DCol{};
        if (slot >= 0) {
            col = d.cols[colBase + fi];
            if (col.valid) return fail(c, NGX_E_UNSUPPORTED, "lookup: field `" + field + "' is missing from some row's schema version");
        }
        return NGX_OK;
    };
    std::vector<LookupCond> conds(p->nfields + p->nterms);
    std::string pool;
    uint64_t rowBytes = edge ? 0 : 1;                             // present[]
    for (int32_t i = 0; i < p->nfields + p->nterms; i++) {
        const bool term = i >= p->nfields;
        const ngx_lookup_cond& q = term ? p->terms[i - p->nfields] : p->fields[i];
        LookupCond& k = conds[i];
        k = LookupCond{};
        int32_t type;
        if (int32_t rc = column(q.field, k.col, type)) return rc;
        k.kind = lookupKindOf(type);
        if (q.kind < NGX_LK_INT || q.kind > NGX_LK_STRING) return fail(c, NGX_E_BAD_ARGUMENT, "lookup: unknown constant kind");
        k.ckind = q.kind;
        k.op = q.op;
        if (term) {
            if (q.op < kLkLT || q.op > kLkNE) return fail(c, NGX_E_BAD_ARGUMENT, "lookup: unknown operator");
            k.lo = static_cast<uint64_t>(q.kind == NGX_LK_BOOL ? (q.bits ? 1 : 0) : q.bits);
        } else {
            if (q.kind != k.kind) return fail(c, NGX_E_BAD_ARGUMENT, "lookup: a scanned field's constant is not of the field's type");
            k.lo = k.kind == kLkBool ? (q.bits ? 1 : 0) : q.lo;
            k.hi = q.hi;
        }
        if (q.kind == NGX_LK_STRING) {
            if (q.str_len >= (1ULL << 31) || (q.str_len && !q.str)) return fail(c, NGX_E_BAD_ARGUMENT, "lookup: string constant");
            k.soff = pool.size();
            k.slen = static_cast<int32_t>(q.str_len);
            pool.append(q.str ? q.str : "", q.str_len);
        }
        rowBytes += k.kind == kLkInt ? k.col.width : k.kind == kLkBool ? 1 : 8;
    }
    std::vector<LookupYield> ys(p->nyields);
    static const int32_t keyTypeV[1] = {NGX_T_VID}, keyTypeE[3] = {NGX_T_VID, NGX_T_VID, NGX_T_INT};
    R.colTypes.assign(edge ? keyTypeE : keyTypeV, (edge ? keyTypeE : keyTypeV) + nkey);
    bool anyString = false;
    for (int32_t y = 0; y < p->nyields; y++) {
        int32_t type;
        ys[y] = LookupYield{};
        if (int32_t rc = column(p->yields[y], ys[y].col, type)) return rc;
        ys[y].cell = type;                                        // NGX_CELL_* numbers its kinds as NGX_T_*
        anyString |= type == NGX_T_STRING;
        R.colTypes.push_back(type);
    }
    const int32_t ncols = nkey + p->nyields;
    R.r.ncols = ncols;
    R.r.col_types = R.colTypes.data();
    HIP_OK(hipSetDevice(c->device));
    uint64_t n = 0;
    if (slot >= 0) n = edge ? (d.V ? readScalar(c, d.slots[slot].off + d.V) : 0) : d.V;
    R.r.scanned_rows = n;
    R.r.keep_bytes = n * rowBytes;
    if (n == 0) {                                                 // no row of the tag / no edge of the type
        c->lookupDevice++;
        return NGX_OK;
    }
    resultEvents(c);
    HIP_OK(hipEventRecord(c->gbEv[0], c->stream));
    LookupArgs a{};
    a.n = n;
    a.V = d.V;
    a.edge = edge ? 1 : 0;
    a.nf = p->nfields;
    a.nt = p->nterms;
    a.ny = p->nyields;
    a.vid = d.vid;
    if (edge) a.slot = d.slots[slot];
    else a.present = d.tags[slot].present;
    LookupCond* condsDev = c->lkConds.get<LookupCond>(std::max<size_t>(conds.size(), 1));
    if (!conds.empty()) HIP_OK(hipMemcpyAsync(condsDev, conds.data(), conds.size() * sizeof(LookupCond), hipMemcpyHostToDevice, c->stream));
    char* poolDev = c->lkPool.get<char>(std::max<size_t>(pool.size(), 1));
    if (!pool.empty()) HIP_OK(hipMemcpyAsync(poolDev, pool.data(), pool.size(), hipMemcpyHostToDevice, c->stream));
    LookupYield* ysDev = c->lkYs.get<LookupYield>(std::max<size_t>(ys.size(), 1));
    if (!ys.empty()) HIP_OK(hipMemcpyAsync(ysDev, ys.data(), ys.size() * sizeof(LookupYield), hipMemcpyHostToDevice, c->stream));
    a.conds = condsDev;
    a.pool = poolDev;
    a.ys = ysDev;
    const uint64_t chunks = (n + 255) / 256;
    a.keep = c->lkKeep.get<uint8_t>(n);
    a.chunkCount = c->lkCount.get<uint64_t>(chunks + 1);
    uint64_t* base = c->lkBase.get<uint64_t>(chunks + 1);
    uint64_t* tiles = c->lkTiles.get<uint64_t>((chunks + kTile - 1) / kTile + 1);
    a.chunkBase = base;
    a.gridMax = c->lookupGridMax;
    HIP_OK(hipStreamSynchronize(c->stream));                      // the descriptors are pageable: copied before they go
    c->timed("lookup_keep", n * rowBytes + n, [&] {
        if (launchLookupKeep(a, c->stream)) throw Error{NGX_E_DEVICE, "lookup keep"};
    });
    c->timed("lookup_scan", chunks * 16, [&] {
        if (launchScanU64(a.chunkCount, chunks, base, tiles, c->stream)) throw Error{NGX_E_DEVICE, "lookup scan"};
    });
    const uint64_t m = readScalar(c, base + chunks);
    if (m > n) throw Error{NGX_E_DEVICE, "lookup: inconsistent counts"};
    if (m > static_cast<uint64_t>(c->lookupRowsMax))
        return fail(c, NGX_E_UNSUPPORTED, "lookup: " + std::to_string(m) + " rows, above lookup_rows_max");
    uint64_t strBytes = 0;
    if (m) {
        if (anyString) {
            uint64_t* slen = c->lkSlen.get<uint64_t>(m + 1);
            uint64_t* spre = c->lkSpre.get<uint64_t>(m + 1);
            uint64_t* stiles = c->lkTiles.get<uint64_t>(std::max((m + kTile - 1) / kTile + 1, (chunks + kTile - 1) / kTile + 1));
            a.lenOut = slen;
            c->timed("lookup_emit", m * 8, [&] {
                if (launchLookupEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "lookup string lengths"};
            });
            c->timed("lookup_scan", m * 16, [&] {
                if (launchScanU64(slen, m, spre, stiles, c->stream)) throw Error{NGX_E_DEVICE, "lookup string scan"};
            });
            strBytes = readScalar(c, spre + m);
            a.lenOut = nullptr;
            a.strPre = spre;
            a.strOut = c->lkStr.get<char>(std::max<uint64_t>(strBytes, 1));
        }
        a.cells = c->lkCells.get<GroupCell>(m * ncols);
        c->timed("lookup_emit", n + m * ncols * sizeof(GroupCell) + strBytes, [&] {
            if (launchLookupEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "lookup emit"};
        });
    }
    finishCells(c, R, a.cells, m * ncols, a.strOut, strBytes);
    R.r.nrows = m;
    c->lookupDevice++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_lookup(ngx_ctx* c, const ngx_lookup_plan* plan, ngx_lookup_result** out) {
    if (!c || !plan || !out) return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left reading the descriptors
    return abiCall<LookupResultHolder>(c, out, OnFail::kSync, [&](LookupResultHolder& R) { return lookupOp(c, plan, R); });
}

extern "C" void ngx_lookup_result_free(ngx_lookup_result* r) {
    if (r) delete reinterpret_cast<LookupResultHolder*>(r);
}

