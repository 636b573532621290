// FIND SHORTEST | ALL | NOLOOP PATH (ngx_find_path): the host driver of findpath.hip.
#include <unordered_map>
#include <unordered_set>

#include "engine_ctx.h"

// ------------------------------------------------------------------------ FIND SHORTEST PATH (ngx_find_path)
namespace {

struct PathResultHolder {
    ngx_path_result r{};
    std::vector<std::string> names;
    std::vector<const char*> cnames;
    std::vector<int32_t> types, etype;
    std::vector<int64_t> src, dst, rank;
    std::vector<uint64_t> mask;
    std::vector<uint8_t> layer;
};

// one side's levels: device lists of (row, bits) and their sizes
struct PathLevels {
    std::vector<const uint32_t*> rows;
    std::vector<const uint64_t*> masks;
    std::vector<uint64_t> n;
};

// the rows of the sentence's vids, the sources first (kNoRow: a vid without a vertex, which takes no part)
const uint32_t* pathSeedRows(ngx_ctx* c, const Space& sp, const DeviceGraph& d, const ngx_path_plan& p) {
    std::vector<int32_t> parts;
    std::vector<int64_t> vids(p.from, p.from + p.nfrom);
    vids.insert(vids.end(), p.to, p.to + p.nto);
    for (int64_t v : vids) parts.push_back(idHash(v, sp.numParts));
    const uint64_t n = vids.size();
    int64_t* dv = c->seedVid.get<int64_t>(n * 2);                 // vids, then parts
    int32_t* dpart = reinterpret_cast<int32_t*>(dv + n);
    stageSeeds(c, parts, vids, dpart, dv);
    uint32_t* rowsIn = c->fpSeed.get<uint32_t>(n);
    if (launchIndexLookup(dpart, dv, n, d.vindex, rowsIn, c->stream)) throw Error{NGX_E_DEVICE, "lookup"};
    return rowsIn;
}

void pathLevelBufs(ngx_ctx* c, int side, size_t level, uint64_t n, uint32_t*& rows, uint64_t*& masks) {
    if (c->fpRows[side].size() <= level) { c->fpRows[side].resize(level + 1); c->fpMasks[side].resize(level + 1); }
    rows = c->fpRows[side][level].get<uint32_t>(std::max<uint64_t>(n, 1));
    masks = c->fpMasks[side][level].get<uint64_t>(std::max<uint64_t>(n, 1));
}

// the device's edges into the result's arrays
void pathEdgesOut(PathResultHolder& R, const std::vector<PathEdge>& host) {
    const uint64_t m = host.size();
    R.src.resize(m); R.dst.resize(m); R.rank.resize(m); R.etype.resize(m); R.mask.resize(m);
    for (uint64_t i = 0; i < m; i++) {
        R.src[i] = host[i].src; R.dst[i] = host[i].dst; R.rank[i] = host[i].rank; R.etype[i] = host[i].type; R.mask[i] = host[i].mask;
    }
    R.r.nedges = m;
    R.r.src = R.src.data(); R.r.dst = R.dst.data(); R.r.rank = R.rank.data(); R.r.type = R.etype.data(); R.r.mask = R.mask.data();
}

// FIND ALL / NOLOOP PATH (flag find_path_all): the to side's cumulative target sets per depth, then the
// from side layer by layer. hs[0]: the sentence's types, hs[1]: the opposite ones.
int32_t findAllPaths(ngx_ctx* c, const ngx_path_plan& p, const Space& sp, const DeviceGraph& d, const HopSlots (&hs)[2], PathResultHolder& R) {
    const uint64_t nS = p.nfrom, nT = p.nto, upto = p.upto;
    resultEvents(c);
    const hipEvent_t ev0 = c->gbEv[0], ev1 = c->gbEv[1];
    HIP_OK(hipEventRecord(ev0, c->stream));
    const uint64_t G = std::max<uint64_t>(d.vglobal, 1);
    uint64_t* inc = c->fpInc[1].get<uint64_t>(G);
    uint64_t* seen = c->fpSeen[1].get<uint64_t>(G);
    uint8_t* lvl = c->fpLvl[1].get<uint8_t>(G);                   // the settle writes it; nothing here reads it
    uint32_t* touched = c->fpTouched[1].get<uint32_t>(G);
    uint64_t* cum = c->fpCum.get<uint64_t>(upto * G);             // cum[d]: every depth reached is copied whole, none is read before
    uint32_t* stamp = c->fpStamp.get<uint32_t>(G);
    uint32_t* layerRows[2] = {c->fpTouched[0].get<uint32_t>(G), touched};   // the to side is done with its list when the layers start
    HIP_OK(hipMemsetAsync(inc, 0, G * 8, c->stream));
    HIP_OK(hipMemsetAsync(seen, 0, G * 8, c->stream));
    HIP_OK(hipMemsetAsync(stamp, 0, G * 4, c->stream));
    const uint64_t cap = static_cast<uint64_t>(c->pathRowsMax);
    PathEdge* outDev = c->fpOut.get<PathEdge>(cap);
    PathState* S = c->fpState.get<PathState>(1);
    HIP_OK(hipMemsetAsync(S, 0, sizeof(PathState), c->stream));
    PathState st{};
    auto readState = [&] {
        HIP_OK(hipMemcpyAsync(&st, S, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (st.err) throw Error{NGX_E_DEVICE, "find path: inconsistent counts"};
    };

    // ---- depth 0 and layer 0: the vids' rows
    const uint32_t* rowsIn = pathSeedRows(c, sp, d, p);
    uint32_t *rowsF, *rowsT;
    uint64_t *masksF, *masksT;
    pathLevelBufs(c, 0, 0, nS, rowsF, masksF);
    pathLevelBufs(c, 1, 0, nT, rowsT, masksT);
    if (launchPathSeed(rowsIn, nS, 0, nullptr, nullptr, nullptr, rowsF, nullptr, &S->nLevel[0], c->stream) ||
        launchPathSeed(rowsIn + nS, nT, 1, seen, nullptr, lvl, rowsT, masksT, &S->nLevel[1], c->stream))
        throw Error{NGX_E_DEVICE, "path seed"};
    HIP_OK(hipMemcpyAsync(cum, seen, G * 8, hipMemcpyDeviceToDevice, c->stream));
    readState();
    uint64_t nLayer = st.nLevel[0], nLevel = st.nLevel[1];

    // ---- the to side: cum[d] = the targets within d edges of each row, d = 0 .. UPTO - 1, until a level is empty
    int32_t depths = 0;
    uint64_t last = 0;                                            // the last depth copied: a deeper one reads as this one
    for (uint64_t dep = 1; dep < upto && nLevel; dep++) {
        HIP_OK(hipMemsetAsync(S, 0, offsetof(PathState, edges), c->stream));
        c->timed("path_expand", 0, [&] {
            if (launchPathExpand(rowsT, masksT, nLevel, hs[1], inc, touched, G, S, 1, c->stream)) throw Error{NGX_E_DEVICE, "path expand"};
        });
        depths++;
        readState();                                              // the rows reached: they size the new level's lists
        const uint64_t nTouched = st.touched[1];
        pathLevelBufs(c, 1, dep, nTouched, rowsT, masksT);
        c->timed("path_settle", 0, [&] {
            if (launchPathSettle(touched, nTouched, inc, seen, nullptr, lvl, static_cast<uint8_t>(dep), rowsT, masksT, S, 1, c->stream))
                throw Error{NGX_E_DEVICE, "path settle"};
            HIP_OK(hipMemcpyAsync(cum + dep * G, seen, G * 8, hipMemcpyDeviceToDevice, c->stream));
        });
        last = dep;
        readState();
        nLevel = st.nLevel[1];
    }

    // ---- the from side: layer i's edges into rows that a target is within UPTO - 1 - i edges of
    int32_t layers = 0;
    bool tooMany = false;
    const uint32_t* cur = rowsF;
    for (uint64_t i = 0; i < upto && nLayer; i++) {
        HIP_OK(hipMemsetAsync(S, 0, offsetof(PathState, edges), c->stream));
        PathWalkArgs a{};
        a.rows = cur;
        a.n = nLayer;
        a.hs = hs[0];
        a.vid = d.vid;
        a.cum = cum + std::min(upto - 1 - i, last) * G;
        a.stamp = stamp;
        a.next = i + 1 < upto ? layerRows[i & 1] : nullptr;
        a.nextCap = G;
        a.out = outDev;
        a.cap = cap;
        a.S = S;
        a.layer = static_cast<int32_t>(i);
        a.gridMax = c->pathGridMax;
        c->timed("path_walk", 0, [&] { if (launchPathWalk(a, c->stream)) throw Error{NGX_E_DEVICE, "path walk"}; });
        layers++;
        readState();                                              // the next layer's rows, the edges so far
        if (st.edges > cap) { tooMany = true; break; }
        cur = layerRows[i & 1];
        nLayer = st.touched[0];
    }
    c->findPathLoopFlushes += st.loopFlushes;
    if (tooMany) {
        c->collectTimings();
        return fail(c, NGX_E_UNSUPPORTED, "find path: path edges above path_rows_max");
    }
    HIP_OK(hipEventRecord(ev1, c->stream));
    std::vector<PathEdge> host(st.edges);
    if (!host.empty()) HIP_OK(hipMemcpyAsync(host.data(), outDev, host.size() * sizeof(PathEdge), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
    c->collectTimings();
    pathEdgesOut(R, host);
    std::unordered_map<int64_t, uint64_t> bitOf;
    for (uint64_t j = 0; j < nT; j++) bitOf[p.to[j]] = 1ULL << j;
    R.layer.resize(host.size());
    uint64_t found = 0;
    for (size_t i = 0; i < host.size(); i++) {
        R.layer[i] = static_cast<uint8_t>(host[i].layer);
        auto it = bitOf.find(host[i].dst);
        if (it != bitOf.end()) found |= it->second;
    }
    R.r.layer = R.layer.data();
    R.r.found = found;
    R.r.levels = depths + layers;
    R.r.device_ms = ms;
    c->findPathDevice++;
    c->findPathLevels += static_cast<uint64_t>(depths + layers);
    c->findPathLayers += static_cast<uint64_t>(layers);
    c->findPathEdges += host.size();
    return NGX_OK;
}

int32_t findPath(ngx_ctx* c, const ngx_path_plan& p, PathResultHolder& R) {
    const bool layered = p.kind == NGX_PATH_ALL || p.kind == NGX_PATH_NOLOOP;
    if (p.kind != NGX_PATH_SHORTEST && !(layered && c->findPathAll))
        return fail(c, NGX_E_UNSUPPORTED, "find path: ALL and NOLOOP enumerate walks, not levels");
    if (p.direction != NGX_DIR_FORWARD && p.direction != NGX_DIR_REVERSELY) return fail(c, NGX_E_UNSUPPORTED, "find path: BIDIRECT");
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "find path: world > 1 needs the levels exchanged");
    if (p.upto < 1 || p.upto > 500) return fail(c, NGX_E_UNSUPPORTED, "find path: UPTO outside 1 .. 500");
    if (layered && p.upto > kPathAllUpto) return fail(c, NGX_E_UNSUPPORTED, "find path: UPTO above 8 for ALL and NOLOOP");
    Space* spp = findSpace(c, p.space);
    if (!spp || !spp->dev) return fail(c, NGX_E_NOT_LOADED, "space not committed");
    const Space& sp = *spp;
    const DeviceGraph& d = *sp.dev;
    if (c->maxEdgesPerVertex < INT32_MAX) return fail(c, NGX_E_UNSUPPORTED, "find path: max_edge_returned_per_vertex is set");
    std::vector<int32_t> over;
    if (p.over_all) {
        for (auto& name : sp.edgeOrder) { R.names.push_back(name); over.push_back(sp.edgeByName.at(name)); }
    } else {
        for (int32_t i = 0; i < p.nover; i++) {
            const std::string name = p.over_names[i];
            auto it = sp.edgeByName.find(name);
            if (it == sp.edgeByName.end()) return fail(c, NGX_E_QUERY, "Edge `" + name + "' not found");
            if (std::find(over.begin(), over.end(), it->second) != over.end()) return fail(c, NGX_E_UNSUPPORTED, "find path: an edge listed twice");
            R.names.push_back(name);
            over.push_back(it->second);
        }
    }
    R.types = over;
    for (auto& n : R.names) R.cnames.push_back(n.c_str());
    R.r.nedge_names = static_cast<int32_t>(over.size());
    R.r.edge_names = R.cnames.data();
    R.r.edge_types = R.types.data();
    for (int32_t t : over) {
        int32_t col;
        int64_t dur;
        if (ttlInfo(sp.edge(std::abs(t)), col, dur)) return fail(c, NGX_E_UNSUPPORTED, "find path: a TTL edge schema");
    }
    const uint64_t nS = p.nfrom, nT = p.nto;
    {
        std::unordered_set<int64_t> fs, ts;
        for (uint64_t i = 0; i < nS; i++) if (!fs.insert(p.from[i]).second) return fail(c, NGX_E_UNSUPPORTED, "find path: a vid listed twice");
        for (uint64_t i = 0; i < nT; i++) if (!ts.insert(p.to[i]).second) return fail(c, NGX_E_UNSUPPORTED, "find path: a vid listed twice");
        if (nT > 64) return fail(c, NGX_E_UNSUPPORTED, "find path: more than 64 targets");
        for (uint64_t i = 0; i < nS; i++) if (ts.count(p.from[i])) return fail(c, NGX_E_UNSUPPORTED, "find path: a vertex on both sides");
    }
    if (nS == 0 || nT == 0) {                                     // getNeighborsAndFindPath: a dead end finishes
        c->findPathDevice++;
        return NGX_OK;
    }
    if (nS >= (1ULL << 31)) return fail(c, NGX_E_UNSUPPORTED, "find path: 2^31 sources or more");
    std::vector<int32_t> typesSide[2], hopTypes;
    for (int32_t t : over) {
        typesSide[0].push_back(p.direction == NGX_DIR_FORWARD ? t : -t);
        typesSide[1].push_back(p.direction == NGX_DIR_FORWARD ? -t : t);
    }
    HopSlots hs[2];
    for (int side = 0; side < 2; side++) {
        hs[side] = makeHopSlots(sp, d, typesSide[side], hopTypes);
        for (int s = 0; s < hs[side].n; s++)
            if (hs[side].eflags[s]) return fail(c, NGX_E_UNSUPPORTED, "find path: edges with empty or unreadable values");
    }
    if (layered) return findAllPaths(c, p, sp, d, hs, R);

    resultEvents(c);
    const hipEvent_t ev0 = c->gbEv[0], ev1 = c->gbEv[1];
    HIP_OK(hipEventRecord(ev0, c->stream));
    const uint64_t G = std::max<uint64_t>(d.vglobal, 1);
    uint64_t *inc[2], *seen[2], *newD[2] = {nullptr, nullptr}, *keep[3];
    uint8_t* lvl[2];
    uint32_t* touched[2];
    for (int side = 0; side < 2; side++) {
        inc[side] = c->fpInc[side].get<uint64_t>(G);
        seen[side] = c->fpSeen[side].get<uint64_t>(G);
        lvl[side] = c->fpLvl[side].get<uint8_t>(G);
        touched[side] = c->fpTouched[side].get<uint32_t>(G);
        HIP_OK(hipMemsetAsync(inc[side], 0, G * 8, c->stream));
        HIP_OK(hipMemsetAsync(seen[side], 0, G * 8, c->stream));
        HIP_OK(hipMemsetAsync(lvl[side], 0xFF, G, c->stream));
    }
    newD[1] = c->fpNew.get<uint64_t>(G);
    for (int k = 0; k < 3; k++) {
        keep[k] = c->fpKeep[k].get<uint64_t>(G);
        HIP_OK(hipMemsetAsync(keep[k], 0, G * 8, c->stream));
    }
    const uint64_t cap = static_cast<uint64_t>(c->pathRowsMax);
    PathEdge* outDev = c->fpOut.get<PathEdge>(cap);
    PathState* S = c->fpState.get<PathState>(1);
    HIP_OK(hipMemsetAsync(S, 0, sizeof(PathState), c->stream));

    // ---- level 0: the vids' rows (a vid without a vertex has none and takes no part)
    PathLevels lv[2];
    auto levelBufs = [&](int side, size_t level, uint64_t n, uint32_t*& rows, uint64_t*& masks) { pathLevelBufs(c, side, level, n, rows, masks); };
    {
        const uint32_t* rowsIn = pathSeedRows(c, sp, d, p);
        for (int side = 0; side < 2; side++) {
            uint32_t* rows;
            uint64_t* masks;
            levelBufs(side, 0, side ? nT : nS, rows, masks);
            if (launchPathSeed(rowsIn + (side ? nS : 0), side ? nT : nS, side, seen[side], newD[side], lvl[side], rows, masks,
                               &S->nLevel[side], c->stream))
                throw Error{NGX_E_DEVICE, "path seed"};
            lv[side].rows.push_back(rows);
            lv[side].masks.push_back(masks);
        }
    }
    PathState st{};
    auto readState = [&] {
        HIP_OK(hipMemcpyAsync(&st, S, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (st.err) throw Error{NGX_E_DEVICE, "find path: inconsistent counts"};
    };
    readState();
    lv[0].n.push_back(st.nLevel[0]);
    lv[1].n.push_back(st.nLevel[1]);

    // keep masks: [0] the from side's seeds, [1] the to side's, [2] the spare; all zero between sweeps
    auto sweepSide = [&](int side, int level, int cur) {
        int next = 2;
        for (int j = level - 1; j >= 0; j--) {
            PathSweepArgs a{};
            a.rows = lv[side].rows[j];
            a.masks = side ? lv[side].masks[j] : nullptr;
            a.n = lv[side].n[j];
            a.hs = hs[side];
            a.vid = d.vid;
            a.keepCur = keep[cur];
            a.keepNext = keep[next];
            a.out = outDev;
            a.cap = cap;
            a.S = S;
            a.reverse = side;
            a.gridMax = c->pathGridMax;
            c->timed("path_sweep", 0, [&] {
                if (launchPathSweep(a, false, c->stream)) throw Error{NGX_E_DEVICE, "path sweep"};
                if (launchPathClear(lv[side].rows[j + 1], lv[side].n[j + 1], keep[cur], c->stream)) throw Error{NGX_E_DEVICE, "path clear"};
            });
            std::swap(cur, next);
        }
        // level 0's keep masks go too: all three arrays are zero again
        if (launchPathClear(lv[side].rows[0], lv[side].n[0], keep[cur], c->stream)) throw Error{NGX_E_DEVICE, "path clear"};
    };
    const uint64_t all = nT == 64 ? ~0ULL : (1ULL << nT) - 1;
    const uint32_t steps = p.upto / 2 + p.upto % 2;
    uint64_t found = 0;
    int32_t levels = 0;
    bool tooMany = false;
    for (uint32_t k = 1; k <= steps && !tooMany; k++) {
        if (lv[0].n[k - 1] == 0 || lv[1].n[k - 1] == 0) break;    // a side without vids ends the search
        const bool even = 2ULL * k <= p.upto;                     // an even path of 2k edges is within UPTO
        HIP_OK(hipMemsetAsync(S, 0, offsetof(PathState, edges), c->stream));
        // odd meet: level k - 1 of the from side over its edges into level k - 1 of the to side (2k - 2 <= UPTO holds)
        {
            PathSweepArgs a{};
            a.rows = lv[0].rows[k - 1];
            a.n = lv[0].n[k - 1];
            a.hs = hs[0];
            a.vid = d.vid;
            a.keepNext = keep[0];
            a.tLvl = lvl[1];
            a.tNew = newD[1];
            a.keepT = keep[1];
            a.notFound = all & ~found;
            a.level = static_cast<uint8_t>(k - 1);
            a.out = outDev;
            a.cap = cap;
            a.S = S;
            a.gridMax = c->pathGridMax;
            c->timed("path_meet", 0, [&] { if (launchPathSweep(a, true, c->stream)) throw Error{NGX_E_DEVICE, "path meet"}; });
        }
        readState();                                              // the odd meet's targets: they may end the search
        if (st.edges > cap) { tooMany = true; break; }
        if (st.found[0]) {
            found |= st.found[0];
            sweepSide(0, static_cast<int>(k) - 1, 0);
            sweepSide(1, static_cast<int>(k) - 1, 1);
        }
        if (found == all || !even) break;
        c->timed("path_expand", 0, [&] {
            for (int side = 0; side < 2; side++)
                if (launchPathExpand(lv[side].rows[k - 1], side ? lv[side].masks[k - 1] : nullptr, lv[side].n[k - 1], hs[side], inc[side],
                                     touched[side], G, S, side, c->stream))
                    throw Error{NGX_E_DEVICE, "path expand"};
        });
        levels += 2;
        readState();                                              // the rows the expansions reached: they size the new levels
        if (st.edges > cap) { tooMany = true; break; }
        uint32_t* rows[2];
        uint64_t* masks[2];
        c->timed("path_settle", 0, [&] {
            for (int side = 0; side < 2; side++) {
                levelBufs(side, k, st.touched[side], rows[side], masks[side]);
                if (launchPathSettle(touched[side], st.touched[side], inc[side], seen[side], newD[side], lvl[side], static_cast<uint8_t>(k),
                                     rows[side], masks[side], S, side, c->stream))
                    throw Error{NGX_E_DEVICE, "path settle"};
                lv[side].rows.push_back(rows[side]);
                lv[side].masks.push_back(masks[side]);
            }
        });
        c->timed("path_meet", 0, [&] {
            if (launchPathMeetEven(rows[1], masks[1], st.touched[1], lvl[0], static_cast<uint8_t>(k), found, keep[0], keep[1], S, c->stream))
                throw Error{NGX_E_DEVICE, "path meet"};
        });
        readState();                                              // the new levels' sizes, the even meet's targets
        lv[0].n.push_back(st.nLevel[0]);
        lv[1].n.push_back(st.nLevel[1]);
        if (st.found[1]) {
            found |= st.found[1];
            sweepSide(0, static_cast<int>(k), 0);
            sweepSide(1, static_cast<int>(k), 1);
        }
        if (found == all) break;
    }
    if (!tooMany) {
        readState();                                              // the last sweeps' edges
        tooMany = st.edges > cap;
    }
    c->findPathLoopFlushes += st.loopFlushes;
    if (tooMany) {
        c->collectTimings();
        return fail(c, NGX_E_UNSUPPORTED, "find path: path edges above path_rows_max");
    }
    HIP_OK(hipEventRecord(ev1, c->stream));
    const uint64_t m = st.edges;
    std::vector<PathEdge> host(m);
    if (m) HIP_OK(hipMemcpyAsync(host.data(), outDev, m * sizeof(PathEdge), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
    c->collectTimings();
    pathEdgesOut(R, host);
    R.r.found = found;
    R.r.levels = levels;
    R.r.device_ms = ms;
    c->findPathDevice++;
    c->findPathLevels += static_cast<uint64_t>(levels);
    c->findPathEdges += m;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_find_path(ngx_ctx* c, const ngx_path_plan* plan, ngx_path_result** out) {
    if (!c || !plan || !out || (plan->nfrom && !plan->from) || (plan->nto && !plan->to) || (plan->nover && !plan->over_names))
        return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left writing the scratch
    return abiCall<PathResultHolder>(c, out, OnFail::kSync, [&](PathResultHolder& R) {
        if (c->activeLane != 0) c->useLane(0);
        return findPath(c, *plan, R);
    });
}

extern "C" void ngx_path_result_free(ngx_path_result* r) {
    if (r) delete reinterpret_cast<PathResultHolder*>(r);
}
