// The engine's context as its host files share it: the buffers that own device and page-locked memory, the
// uploaded snapshot, a query lane's state, the context itself, and the pieces every operator's entry point and
// result tail are made of. Host only: not part of the prefix of generated kernels.
//
// engine.cpp         context open / close, schema, upload, commit, flags, stats, the GO driver, pipes, the
//                    batch pipeline, GetNeighbors
// op_group_order.cpp GROUP BY, ORDER BY / LIMIT and GROUP BY | ORDER BY
// op_setop.cpp       UNION DISTINCT / INTERSECT / MINUS
// op_fetch.cpp       FETCH PROP ON
// op_lookup.cpp      LOOKUP ON
// op_findpath.cpp    FIND SHORTEST PATH
// op_yield.cpp       | YIELD ... [WHERE ...]
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include <sys/mman.h>
#include <ucontext.h>

#include "exprc.h"
#include "jit.h"
#include "kernels.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { throw Error{NGX_E_DEVICE, std::string("HIP: ") + hipGetErrorString(e_) + " at " #x}; } } while (0)
#define NCCL_OK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) { throw Error{NGX_E_DEVICE, std::string("RCCL: ") + ncclGetErrorString(r_)}; } } while (0)

namespace ngx {

struct DeviceGraph {
    uint64_t V = 0, vglobal = 0, gbase = 0;
    std::vector<uint64_t> shardBase;
    int32_t* vpart = nullptr;
    int64_t* vid = nullptr;
    int32_t vidW = 8;                                   // narrowest signed width holding every vid of vid[]
    VIndex vindex{nullptr, 0};                          // (part, vid) -> row hash index (seed lookup)
    std::vector<DSlot> slots;
    // per slot: the row holding CSR position c * kChunk, for every chunk c of the slot (+ a last row): the
    // chunk map of a final hop over the whole slot (FinalArgs::denseMark)
    std::vector<const uint64_t*> chunkRow;
    std::vector<int32_t> mirror;                        // per slot: the slot holding its exact transpose, or -1
    // per slot with a mirror: the pull hop's head image of the in-lists (kernels.h PullArgs)
    struct PullHead { const uint32_t* perm = nullptr; const uint32_t* head = nullptr; const uint8_t* nk = nullptr;
                      uint64_t slices = 0, longRows = 0; };
    std::vector<PullHead> pullHead;
    // $$ props across shards: every tag table over ALL global rows (replicas of the other shards'
    // rows), gathered on the first query that reads a $$ prop, kept until the next commit
    bool replicas = false;
    std::vector<HostColumn> repHost;                    // host copies (string bytes back result cells)
    DTag* rtags = nullptr;
    DCol* rcols = nullptr;
    std::vector<DTag> tags;
    std::vector<DCol> cols;
    DSlot* dslots = nullptr;
    DTag* dtags = nullptr;
    DCol* dcols = nullptr;
    std::vector<void*> allocs;
    uint64_t bytes = 0;
    struct Range { uint64_t dev; const char* host; uint64_t len; };
    std::vector<Range> strRanges;                       // device string bytes -> host copy
    ~DeviceGraph() { for (void* p : allocs) (void)hipFree(p); }

    template <typename T>
    T* upload(const T* src, uint64_t n) {
        if (n == 0) return nullptr;
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, n * sizeof(T)));
        HIP_OK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        allocs.push_back(p);
        bytes += n * sizeof(T);
        return static_cast<T*>(p);
    }
};

// Ownership: a DBuf or PinBuf frees its block when it is destroyed, assigned to or grown, through freeDevice /
// freeHost, which park the block until the batch's end while a pipelined batch runs on the thread (engine.cpp);
// release() frees at once. `bytes` is the block's share of the gauge dbuf_live_bytes, which it leaves when it is
// really freed.
void freeDevice(void* p, size_t bytes);
void freeHost(void* p);

// growable device buffer
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    uint64_t gen = 0;                                   // unique per allocation (hipMalloc may hand back a freed address)
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : p(o.p), cap(o.cap), gen(o.gen) { o.p = nullptr; o.cap = 0; o.gen = 0; }
    DBuf& operator=(DBuf&& o) noexcept {
        if (this != &o) {
            freeDevice(p, cap);
            p = o.p, cap = o.cap, gen = o.gen;
            o.p = nullptr, o.cap = 0, o.gen = 0;
        }
        return *this;
    }
    ~DBuf() { freeDevice(p, cap); }
    template <typename T>
    T* get(size_t n) {
        const size_t bytes = std::max<size_t>(n * sizeof(T), 64);
        if (bytes > cap) grow(bytes);
        return static_cast<T*>(p);
    }
    void grow(size_t bytes);                            // a new block of at least `bytes`; the contents go
    void release();
};

// page-locked host staging (result D2H, program and seed uploads)
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            freeHost(p);
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~PinBuf() { freeHost(p); }
    char* get(size_t bytes) {
        if (bytes > cap) {
            freeHost(p);
            p = nullptr;
            // 25 % headroom: result sizes vary from query to query, and re-pinning a GB-sized
            // staging block costs more than the copy itself
            size_t c = std::max(bytes + bytes / 4, cap * 3 / 2);
            cap = 0;
            // coherent (fine-grained): kernels read the seeds / inputs the host just wrote, and the copy
            // kernel stores results the host reads after the stream synchronises; neither may meet a
            // stale line the GPU kept cached from an earlier query (hipHostMallocDefault is non-coherent)
            HIP_OK(hipHostMalloc(&p, c, hipHostMallocMapped | hipHostMallocCoherent));
            cap = c;
        }
        return static_cast<char*>(p);
    }
    // grow keeping the first `keep` bytes (the caller has synchronised with copies out of the old block)
    char* getKeep(size_t bytes, size_t keep) {
        if (bytes <= cap) return static_cast<char*>(p);
        std::vector<char> save(static_cast<char*>(p), static_cast<char*>(p) + std::min(keep, cap));
        char* n = get(bytes);
        std::memcpy(n, save.data(), save.size());
        return n;
    }
};

struct ColBuf { DBuf x, len, t; };

// the $$ owner fetch of one lane (fetchDstProps): request lists, exchange blocks, the global row ->
// fetched-row map, and per record hop of the running query the fetched tag tables (device) with the host
// copy of their string bytes (result cells read strings back through it)
struct DstLane {
    DBuf req, counts, recv, blobS, blobR, rows, map;
    uint64_t mapRows = 0;
    std::vector<DBuf> data;                             // per record hop: present / values / strings
    std::vector<std::string> hostStr;                   // per record hop: its string bytes (host copy)
    std::vector<const char*> devStr;                    // ... and where they live on the device
    uint64_t bytes() const {
        uint64_t b = req.cap + counts.cap + recv.cap + blobS.cap + blobR.cap + rows.cap + map.cap;
        for (const DBuf& d : data) b += d.cap;
        return b;
    }
};

// A query lane: the per-query scratch of the hop loop, its result rows and their reservation state (a query's
// final hop writes its lane's arrays, so its k_final_close may run beside the next query's final hop) and its
// publication slots (words [pinLane, pinLane + ngx_ctx::kLaneWords) of the host-mapped block). ngx_go_batch runs
// consecutive queries on rotating lanes, so that one query's hops run on the device beside the earlier queries'
// final hops (GoPipe). The context is its active lane (ngx_ctx : LaneState); lane k is parked in
// ngx_ctx::parked[k] while it is not active. A per-lane field is a member here and nothing else names it.
struct LaneState {
    DBuf visited, F0, F1, estart, ebase, chunkFirst, tileSums, counters, lbStatus, seedPart, seedVid;
    DBuf cmpStatus[2];                                  // compaction tile / wave totals (kernels.h CompactArgs)
    DBuf frontierBits;                                  // the pull's frontier bitmap over global rows
    DBuf localBits;                                     // world > 1 pull: this shard's frontier bitmap
    DBuf edgeMask, progBuf;
    // pull expansion (kernels.h launchPull): segment queue + its counters, kept zero between launches
    DBuf pullSeg, pullCtl;
    uint64_t pullSegWords = 0;
    DBuf sparseCtl;                                     // the sparse kernel's counters, kept zero between launches
    DBuf estart2, ebase2, chunkFirst2;                  // the next hop's entry arrays while the sparse kernel reads this hop's
    DBuf dynStats;                                      // per hop: packed (|F|, E) written by seed / compaction
    uint64_t visitedSize = 0;
    uint8_t epoch = 0;
    // the frontier bitmap is known to be all zero (a sparse hop's dedup set starts from it): set by a
    // compaction that wrote zeros, cleared by every other writer. Keyed on the allocation (pointer and
    // DBuf::gen) and the words zeroed: a query in a space with more rows needs more zero words
    bool bitsClean = false;
    const void* bitsCleanPtr = nullptr;
    uint64_t bitsCleanGen = 0, bitsCleanWords = 0;
    std::string progLast;                               // the bytes of the last program upload ...
    const char* progLastPtr = nullptr;                  // ... and where they went (uploadPrograms skips a repeat)
    PinBuf inStage, seedStage;
    uint32_t pinLane = 0;
    DBuf oSrc, oDst, oRank, oType, oColDesc;
    DBuf resvTab, resvCtl;                              // GO final hop: block tables, counters (kargs.h resv*)
    std::vector<ColBuf> oCols;                          // result columns (columnar, HBM)
    std::vector<OutCol> oColView;                       // their device pointers, as uploaded to oColDesc
    uint64_t resvTabWords = 0;
    uint32_t resvLastG = 0, resvLastStride = 0, resvParity = 0;
    bool resvClosePending = false;                      // counters handed out, their k_final_close not enqueued
    DstLane dst;                                        // the $$ owner fetch's buffers
    // device bytes the lane holds (flag released_lane_bytes): the one list of a lane's buffers
    uint64_t bytes() const {
        uint64_t b = dst.bytes();
        for (const DBuf* d : {&visited, &F0, &F1, &estart, &ebase, &chunkFirst, &tileSums, &counters, &lbStatus, &seedPart,
                              &seedVid, &cmpStatus[0], &cmpStatus[1], &frontierBits, &localBits, &edgeMask, &progBuf, &pullSeg,
                              &pullCtl, &sparseCtl, &estart2, &ebase2, &chunkFirst2, &dynStats, &oSrc, &oDst, &oRank, &oType,
                              &oColDesc, &resvTab, &resvCtl})
            b += d->cap;
        for (const ColBuf& cb : oCols) b += cb.x.cap + cb.len.cap + cb.t.cap;
        return b;
    }
};

// ROCTX range on the host timeline of rocprofv3 (--marker-trace): a query, each hop, each kernel class
// launch (the reference's FLAGS_trace_go step log, GoExecutor.cpp:559-569). Without a
// tool attached a push / pop is a check of a registration flag.
struct RoctxRange {
    explicit RoctxRange(const char* name) { roctxRangePushA(name); }
    ~RoctxRange() { roctxRangePop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};

}  // namespace ngx

using namespace ngx;

struct ngx_ctx : LaneState {
    int32_t device = 0, rank = 0, world = 1;
    hipStream_t stream = nullptr;
    ncclComm_t comm = nullptr;
    ngx_exchange_fn xchg = nullptr;                    // host collective instead of RCCL (tests)
    uint64_t* pin = nullptr;                           // host-mapped [value, seq]: scan totals published by
    uint64_t* pinDev = nullptr;                        // k_scan_tiles (kernels.h Publish)
    uint64_t pinSeq = 0;                               // words [0, 2): scan totals; [kTailOff ..): query tail
    static constexpr size_t kPinBytes = 16384;          // up to eight lanes of 256 words (LaneState)
    static constexpr size_t kTailOff = 8;               // k_publish_tail: seq, error bits, extra words
    static constexpr uint32_t kSeedSlot = 80;           // the seed hop's publication (nextPub)
    static constexpr uint32_t kRowsSlot = 88;           // a record hop's row count (k_final_close)
    // ngx_go_batch: the next query's host preparation and first hops enqueued while this one's final hop
    // runs (flag "batch_pipeline"; read-only "batch_overlaps" counts the queries that overlapped)
    bool batchPipeline = true;
    struct GoPipe* pipe = nullptr;
    uint64_t pipeOverlaps = 0;
    void* xchgUser = nullptr;
    std::map<int32_t, std::unique_ptr<Space>> spaces;
    std::string lastError;
    std::mutex mu;
    // scratch shared by the lanes (the per-lane scratch is LaneState's)
    DBuf oEntry, sendBits, recvBits, vcells, misc;
    uint32_t resvSeq = 0;
    const uint64_t* resvRows = nullptr;                 // this query's last GO final launch's row count (device word)
    uint64_t strArenaMax = uint64_t(8) << 30;           // bytes of one record hop's result string arena (flag str_arena_max)
    DBuf oFlags, rowCols, rowLen, rowOff, rowBytes;     // GetNeighbors response rows (encode_rows)
    DBuf dkTable, dkKeep, dkPre, dSrc, dDst, dRank, dType;   // YIELD DISTINCT (table, marks, compacted rows)
    std::vector<DBuf> strArena;                         // result string arenas, one per record hop (FinalArgs::strOut)
    DBuf roots[2], rootBits;                            // multi-root walk: root sets over rows, per-entry bits
    DBuf rootSend, rootRecv;                            // world > 1: root sets of peer rows, both ways
    DBuf pwF, pwIn, pwEst, pwCf;                        // ... reading $-: (row, input row) entries, their estart / heads
    DBuf inX, inLen, inT, inStr, inDesc;                // ... the pipe's input table
    uint64_t pipeWalks = 0;                             // walks run for FROM $- / $var sentences (flag pipe_walks)
    // ngx_go_group_by: key table, leaders / flags / group numbers, COUNT_DISTINCT flags, state words, descriptors,
    // string lengths and their scan, output cells and string bytes, scan tiles
    DBuf gbTable, gbLeader, gbFlag, gbPre, gbDistinct, gbState, gbDesc, gbSlen, gbSpre, gbCells, gbStr, gbTiles;
    hipEvent_t gbEv[2] = {nullptr, nullptr};            // ngx_group_result / ngx_order_result.device_ms: made on the first call, kept
    uint64_t groupByDevice = 0, groupByLds = 0;        // calls completed on the device / through the LDS path
    int64_t groupLdsMax = -1;                           // flag group_lds_max: -1 by size, else the largest group count
    uint32_t groupGridMax = 0;                          // flag group_grid_max: most accumulation workgroups, 0: built-in
    // ngx_go_order_by: row marks, the two tied-row lists, digit counters, state, descriptors, string-length maxima,
    // winners' rows, their string lengths and scan, output cells and string bytes, scan tiles
    DBuf obMark, obList[2], obHist, obState, obDesc, obMax, obWin, obSlen, obSpre, obCells, obStr, obTiles;
    uint64_t orderByDevice = 0;                         // calls completed on the device (flag order_by_device)
    int64_t orderKMax = 65536;                          // flag order_k_max: the largest offset + count selected on the device
    uint32_t orderGridMax = 0;                          // flag order_grid_max: most workgroups of a sweep, 0: built-in
    // paths the selections took so far (OrderState's counters summed; flags order_compactions, ...)
    uint64_t orderCompactions = 0, orderListCompactions = 0, orderLoopFlushes = 0;
    // ngx_go_group_order_by: the group rows as columns (values, string lengths) and their descriptors
    DBuf goCols, goLen, goDesc;
    uint64_t groupOrderDevice = 0;                      // calls completed on the device (flag group_order_device)
    // ngx_set_op: row-tuple table, per-slot counts and tickets, the kept rows of either side, state, descriptors,
    // string lengths and their scan, output cells and string bytes, scan tiles
    DBuf sbTable, sbCount, sbTaken, sbKeep[2], sbState, sbDesc, sbSlen, sbSpre, sbCells, sbStr, sbTiles;
    uint64_t setOpDevice = 0;                           // calls completed on the device (flag set_op_device)
    int64_t setRowsMax = int64_t(1) << 20;              // flag set_rows_max: the most output rows answered on the device
    uint32_t setGridMax = 0;                            // flag set_grid_max: most workgroups of a sweep, 0: built-in
    uint64_t setLoopFlushes = 0;                        // SetState::loopFlushes summed (flag set_loop_flushes)
    // ngx_fetch: per key its vertex row, edge index and hit bits; per 256-key chunk the kept keys and their scan;
    // the tags seen; yield descriptors; uploaded host keys; string lengths and their scan; output cells and bytes
    DBuf fxRow, fxEidx, fxHits, fxCount, fxBase, fxTiles, fxSeen, fxDesc, fxKeys[3], fxSlen, fxSpre, fxCells, fxStr;
    uint64_t fetchDevice = 0;                           // calls completed on the device (flag fetch_device)
    uint32_t fetchGridMax = 0;                          // flag fetch_grid_max: most workgroups of a sweep, 0: built-in
    // ngx_lookup: per row its keep byte; per 256-row chunk the kept rows and their scan; the plan's conditions, string
    // constants and yield descriptors; string lengths and their scan; output cells and bytes
    DBuf lkKeep, lkCount, lkBase, lkTiles, lkConds, lkPool, lkYs, lkSlen, lkSpre, lkCells, lkStr;
    uint64_t lookupDevice = 0;                          // calls completed (flag lookup_device)
    uint32_t lookupGridMax = 0;                         // flag lookup_grid_max: most workgroups of a sweep, 0: built-in
    int64_t lookupRowsMax = int64_t(1) << 26;           // flag lookup_rows_max: the most output rows
    // ngx_go_yield: the keep bitmap; per 256-row chunk the kept rows and their scan; column and yield descriptors,
    // programs and their constant strings; state words, error words and probed values; string lengths and their
    // scan; output cells and bytes
    DBuf yKeep, yCount, yBase, yTiles, yDesc, yCode, yPool, yState, ySlen, ySpre, yCells, yStr;
    uint64_t yieldDevice = 0;                           // calls completed on the device (flag yield_device)
    uint32_t yieldGridMax = 0;                          // flag yield_grid_max: most workgroups of a sweep, 0: built-in
    // ngx_go_set: the string arenas of the left traversal while the right one runs on the second lane
    std::vector<DBuf> setArena;
    // flag set_check_left (debug): ngx_go_set digests the left result before and after the right traversal
    // (ngx_go_result_digest) and fails the call if they differ; set_left_checks counts the digests that agreed
    bool setCheckLeft = false;
    uint64_t setLeftChecks = 0;
    // ngx_find_path: per side (0 from, 1 to) the incoming / seen bits over rows, the latest level per row (the to side's
    // with its bits), the rows an expansion reached; per side and level the compacted rows and bits; the sweeps' keep
    // masks; looked-up seed rows; the path-DAG edges; the state words
    DBuf fpInc[2], fpSeen[2], fpNew, fpLvl[2], fpTouched[2], fpKeep[3], fpSeed, fpOut, fpState;
    std::vector<DBuf> fpRows[2], fpMasks[2];
    int64_t pathRowsMax = int64_t(1) << 20;             // flag path_rows_max: the most path-DAG edges answered on the device
    uint32_t pathGridMax = 0;                           // flag path_grid_max: most workgroups of a sweep, 0: built-in
    uint64_t findPathDevice = 0, findPathLevels = 0, findPathEdges = 0, findPathLoopFlushes = 0;
    // FIND ALL / NOLOOP PATH: the to side's seen words after each depth (UPTO per row), the layer that listed a row last
    DBuf fpCum, fpStamp;
    bool findPathAll = false;                           // flag find_path_all: ngx_find_path answers ALL and NOLOOP too
    uint64_t findPathLayers = 0;                        // flag find_path_layers: from-side layers launched for them
    DBuf pullGather;                                    // world > 1 pull: all shards' frontier bitmaps
    struct { int64_t qps = 0, errorQps = 0, latencySum = 0, latencyCount = 0, latencyMax = 0; } gbStats;
    std::vector<ngx_stat> statList;                     // ngx_stats view
    int64_t maxEdgesPerVertex = INT32_MAX;             // storaged FLAGS_max_edge_returned_per_vertex (GO hops)
    PinBuf hostStage;                                   // result D2H
    std::string progImg;                                // this call's program bytes (compared before staging)
    std::vector<ColBuf> dCols;                          // DISTINCT: the other half of each column's double buffer
    int32_t compactLaneRows = 0;                        // compaction rows per lane: 0 = by shard size, else 4 / 8 / 16
    int32_t compactWg = 0;                              // compaction workgroup threads: 0 = auto, 256 or 1024
    // generated GO final hops store result rows / load columns non-temporally (flags final_nt_stores /
    // final_nt_loads). r06, both on: the batch 0.2796 vs 0.2833 ms/step on one box (8 rounds), 0.2898 vs
    // 0.2901 on another (6); the final hop alone ~1% slower; either alone slower than neither. Kept off.
    bool finalNtStores = false;
    bool finalNtLoads = false;
    uint32_t resvGroups = kResvGroups;                  // GO final hop row-reservation groups (flag resv_groups, 1 .. kResvMaxGroups)
    int64_t pullFactor = 200;                           // pull when 100 x hop edges >= pullFactor x shard rows (0: never)
    uint64_t pullHops = 0;
    // sparse intermediate hops (kernels.h SparseArgs): a push hop with E * sparseFactor <= V builds the next
    // frontier in the expansion itself (flag "sparse_factor", 0 = never, < 0 = every push hop; read-only
    // "sparse_hops")
    int64_t sparseFactor = 16;
    uint64_t sparseHops = 0;
    bool pullPredict = false;                           // hop 2 of the last query pulled (world 1): launch it early
    // world > 1 push hops: frontier exchanged as vid lists instead of bitmaps (flag "xchg_lists": -1 by the
    // hop's size, 0 bitmaps, 1 lists; read-only "xchg_list_hops")
    int64_t xchgLists = -1;
    uint64_t xchgListHops = 0;
    DBuf xListSend, xListRecv, xCounts;
    // device-driven hops (no host round trip per hop). Off by default: on MI355X the upper-bound grids
    // and the idle launch of the expansion not taken cost what the round trips saved (C2 step: device
    // 680 vs 656 us, profiles/r02_dyn_*); kept as an option ("dyn_hops", NGX_DYN_HOPS=1)
    bool dynHops = false;
    bool deviceLibm = false;                            // inexact libm of row values on the device (exprc.cpp)
    bool reservoirSampling = false;                     // storaged FLAGS_enable_reservoir_sampling: refused
    bool narrowColumns = true;                          // integer columns at their narrowest width (at commit)
    bool traceGo = false;                               // graphd FLAGS_trace_go: per-step log on stderr
    int cus = 256;                                      // compute units of the device
    // RCCL watchdog: collective work must finish within this; else the communicator is aborted
    int64_t rcclTimeoutMs = 120000;
    bool broken = false;                                // communicator aborted: every later call fails
    uint64_t lastXchgBytes = 0;                         // bytes this shard sent in the last exchange
    // per-query kernels (hipRTC)
    bool jitOn = true;
    JitCache jit;
    std::string jitNote;
    // profiling
    bool prof = false;
    struct Stat { std::string name; uint32_t launches = 0; double ms = 0; uint64_t bytes = 0; };
    std::vector<Stat> stats;
    std::vector<ngx_kernel_stat> statView;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
    std::vector<hipEvent_t> eventPool;
    size_t eventNext = 0;

    // the lanes (LaneState above): the context is the active one, lane k is parked in parked[k] while it is not
    // (parked[activeLane] holds an empty set); useLane swaps sets
    static constexpr uint32_t kLaneWords = 256;
    static constexpr int kMaxLanes = 8;                 // kPinBytes / (8 * kLaneWords)
    LaneState parked[kMaxLanes];
    int activeLane = 0;
    // lanes of a pipelined batch (flag "batch_lanes", 2 .. kMaxLanes): up to lanes - 1 queries wait at their
    // deferral point while the next one runs its hops
    int32_t batchLanes = 4;                            // r06, two final streams: 4 lanes 0.299 vs 3 lanes 0.303 ms per step
    // ngx_go_batch's streams (GoPipe, created with the context at world 1): the queries' hops on the front
    // stream, the last final hop of each overlapped query on the final stream; finalStream is set while a
    // pipelined batch runs. The coroutine stacks of the batch's queries (one per lane).
    // [0] front (hops), [1] final (final hops), [2] the second front stream (flag batch_fronts 2: consecutive
    // queries' hops on alternate front streams, so two queries' hop chains run at once beside a final hop)
    // or the close stream (k_final_close of an overlapped final hop beside the next query's final hop: the
    // close reads and moves its own lane's rows only)
    hipStream_t pipeStreams[4] = {nullptr, nullptr, nullptr, nullptr};   // + [3] the close stream
    hipEvent_t pipeEv[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // a ring of events for the batch's cross-stream waits: each wait gets an event no later record re-arms
    // while the wait may be pending (flag batch_event_ring; 0: the fixed pipeEv per role)
    static constexpr int kPipeRing = 64;
    hipEvent_t pipeRing[kPipeRing] = {};
    uint32_t pipeRingNext = 0;
    bool batchEventRing = true;
    hipEvent_t pipeEvent(int role) {
        if (!batchEventRing || !pipeRing[0]) return pipeEv[role];
        return pipeRing[pipeRingNext++ % kPipeRing];
    }
    // set while a pipelined batch runs with flag batch_close_stream (default on since the second front
    // stream: C2 0.310 vs 0.317 ms per step; with one front stream it measured 0.330 vs 0.324, the next final
    // hop waiting for its front-stream dependency anyway)
    hipStream_t closeStream = nullptr;
    bool batchCloseStream = true;
    int32_t batchFronts = 2;                           // front streams of a pipelined batch (1 or 2)
    // flag batch_cu_split N > 0: the batch's front streams on N CUs (every CU i with (i / 8) % (256 / N / 8)
    // == 0, spread over the XCDs), its final stream on the others, so the hops' waves do not take slots
    // from the final hop (streams created on first use with that split)
    int32_t batchCuSplit = 0, cuSplitMade = 0;
    hipStream_t splitStreams[4] = {nullptr, nullptr, nullptr, nullptr};
    int32_t pipeFronts = 1;                            // ... of the batch that runs
    hipStream_t finalStream = nullptr;
    // flag batch_finals 2: consecutive queries' final hops on two final streams (the close after its final
    // hop on the same stream, no close stream), so one final hop starts while the other drains its tail;
    // finalCur is the running query's
    int32_t batchFinals = 2;
    // per lane: the event after its last overlapped final hop's close. The lane's next final hop waits for it:
    // that close still moves the earlier query's rows inside the lane's result arrays and reads its block
    // table after the earlier query has read its row count (published by the close's first workgroup), and
    // with two final streams nothing else orders the two (r06: a C2 batch at 4 groups failed on it)
    hipEvent_t laneCloseEv[kMaxLanes] = {};
    bool laneClosePending[kMaxLanes] = {};                           // C2: 0.302 vs 0.309 ms per step (tools/ab_batch.py, 10 rounds)
    hipStream_t finalStream2 = nullptr, finalCur = nullptr;
    void* coStack[kMaxLanes] = {};
    static constexpr size_t kCoStackBytes = size_t(16) << 20;   // + a guard page below each
    void swapLane(LaneState& L) { std::swap(static_cast<LaneState&>(*this), L); }
    void initLanes() {
        for (int k = 1; k < kMaxLanes; k++) parked[k].pinLane = k * kLaneWords;
    }
    void useLane(int k) {
        if (k == activeLane) return;
        swapLane(parked[activeLane]);                  // park the active lane (the empty set comes in) ...
        swapLane(parked[k]);                           // ... and bring lane k in (the empty set goes to its slot)
        activeLane = k;
    }

    // the active lane's buffers freed and its state reset; it keeps its publication slots
    void releaseLane() {
        const uint32_t slots = pinLane;
        static_cast<LaneState&>(*this) = LaneState{};
        pinLane = slots;
    }
    // the parked lanes' scratch and result rows freed (flag batch_release_lanes, or release_lanes = 1 once):
    // a pipelined batch leaves lanes 1 .. kMaxLanes - 1 holding buffers as large as lane 0's. Called with no
    // batch running; hipFree waits for the work that still reads them.
    uint64_t releaseParked() {
        uint64_t freed = 0;
        const int was = activeLane;
        for (int k = 0; k < kMaxLanes; k++) {
            if (k == was) continue;
            useLane(k);
            freed += bytes();
            releaseLane();
        }
        useLane(was);
        return freed;
    }
    uint64_t releasedBytes = 0;
    bool batchReleaseLanes = false;
    // $$ props at world > 1 (flag dst_props): -1 by size (replicas while every shard's tag data fits
    // dstReplicaMax bytes), 0 replicas of every tag table over the global rows (gathered once per snapshot),
    // 1 the owner fetch per record hop (GoExecutor::fetchVertexProps -> QueryVertexPropsProcessor)
    int32_t dstProps = -1;
    // the final hop over every CSR position of its slot, reading the frontier from the marks (no next-frontier
    // list, no entry arrays): after a pulled hop at world 1 with one OVER type (flag dense_final)
    bool denseFinal = true;
    bool denseCloseTotal = true;                        // its frontier total summed by the close (flag dense_close_total)
    bool denseWorldDev = true;                          // world > 1: its totals kept on the device (flag dense_world_dev)
    uint64_t denseFinals = 0;
    // a dense final hop of an eligible generated kernel (jit.h jitDenseEligible) issues its edge-column loads
    // ahead of the frontier bits (final_kernels.h finalBodyDense; flag dense_early_loads); 0: the generic body
    bool denseEarlyLoads = true;
    uint64_t denseEarlyFinals = 0;                      // launches that took it (flag dense_early_finals, read-only)
    // ngx_go_batch: queries 2k and 2k + 1 whose dense, loads-first final hops differ only in their frontier run
    // them as one launch that scans the slot's columns once (final_kernels.h finalBodyDense2; engine.cpp
    // HeldFinal; flag batch_pair_finals, world 1 only). C2: 0.2198 vs 0.2438 ms per step (tools/ab_batch.py, 100
    // steps, 8 rounds, ranges apart), the paired launch 417 us for two queries against 2 x 234
    bool batchPairFinals = true;
    uint64_t pairedFinals = 0;                          // launches that served two queries (flag paired_finals, read-only)
    hipEvent_t heldFrontEv[kMaxLanes] = {};             // per lane: its held query's front stream at the hand-off
    // two final streams: each final-hop launch of a batch (a single hop, a pair, a flushed held hop) goes to the
    // final stream the launch before it did not use (engine.cpp FinalStreamScope; flag batch_final_turns, world 1
    // only). 0: query i's on final stream i & 1, which with pairing on puts every pair kernel and both its closes
    // on the second stream (the pair is launched by its odd query), one behind the other. C2: 0.2088 vs 0.2289
    // ms per step (tools/ab_batch.py, 100 steps, 8 rounds, ranges apart; profiles/r12_turns_summary.md)
    bool batchFinalTurns = true;
    int finalTurn = 0;                                  // the final stream (0 / 1) the batch's next launch takes
    uint64_t finalLaunches[2] = {0, 0};                 // final-hop launches enqueued per final stream (final_launches_s0 / _s1)
    hipStream_t turnStream() const { return finalTurn && finalStream2 ? finalStream2 : finalStream; }
    void countFinalLaunch(hipStream_t s) {
        if (s && s == finalStream) finalLaunches[0]++;
        else if (s && s == finalStream2) finalLaunches[1]++;
    }
    uint64_t dstReplicaMax = uint64_t(1) << 30;
    uint64_t dstFetches = 0, dstFetchRows = 0;
    // Also the cleanup of ngx_open's error paths. What is no buffer goes here; the buffers free themselves as the
    // members go, after this body: by then every stream has been synchronised, so no work reads them, and the
    // device selected here is still the current one.
    ~ngx_ctx() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto st : pipeStreams) if (st) (void)hipStreamSynchronize(st);
        for (auto st : splitStreams) if (st) (void)hipStreamSynchronize(st);
        spaces.clear();
        for (auto e : eventPool) (void)hipEventDestroy(e);
        for (auto e : gbEv) if (e) (void)hipEventDestroy(e);
        for (auto e : pipeEv) if (e) (void)hipEventDestroy(e);
        for (auto e : laneCloseEv) if (e) (void)hipEventDestroy(e);
        for (auto e : heldFrontEv) if (e) (void)hipEventDestroy(e);
        for (auto e : pipeRing) if (e) (void)hipEventDestroy(e);
        for (auto st : pipeStreams) if (st) (void)hipStreamDestroy(st);
        for (auto st : splitStreams) if (st) (void)hipStreamDestroy(st);
        for (void* st : coStack) if (st) munmap(st, kCoStackBytes + 4096);
        if (comm) (void)ncclCommDestroy(comm);
        if (pin) (void)hipHostFree(pin);
        if (stream) (void)hipStreamDestroy(stream);
    }

    hipEvent_t ev() {
        if (eventNext == eventPool.size()) {
            hipEvent_t e;
            HIP_OK(hipEventCreate(&e));
            eventPool.push_back(e);
        }
        return eventPool[eventNext++];
    }
    int statIndex(const char* name) {
        for (size_t i = 0; i < stats.size(); i++) if (stats[i].name == name) return static_cast<int>(i);
        stats.push_back(Stat{name});
        return static_cast<int>(stats.size()) - 1;
    }
    // host timeline of a query (NGX_HOST_TRACE=1): launches and publication waits, printed per query
    bool htrace = false;
    // pipelined batch host timeline (NGX_PIPE_TRACE=1): the same marks, tagged with the running query and
    // kept with absolute CLOCK_MONOTONIC times until the batch ends (the pipeline stays on)
    bool ptrace = false;
    int32_t ptraceQuery = -1;
    std::vector<std::pair<std::string, int64_t>> pmarks;
    void pmark(const std::string& what) {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        pmarks.emplace_back("q" + std::to_string(ptraceQuery) + " " + what,
                            static_cast<int64_t>(ts.tv_sec) * 1000000000LL + ts.tv_nsec);
    }
    std::vector<std::pair<std::string, std::chrono::steady_clock::time_point>> hmarks;
    void hmark(const std::string& what) {
        if (htrace) hmarks.emplace_back(what, std::chrono::steady_clock::now());
        if (ptrace) pmark(what);
    }
    void hflush() {
        if (!htrace || hmarks.empty()) return;
        std::string line = "[ngx host]";
        for (auto& m : hmarks)
            line += " " + m.first + "@" + std::to_string(std::chrono::duration<double, std::micro>(m.second - hmarks[0].second).count()).substr(0, 7);
        std::fprintf(stderr, "%s\n", line.c_str());
        hmarks.clear();
    }
    // bracket a launch group with events when profiling
    template <typename F>
    void timed(const char* name, uint64_t algoBytes, F&& f) {
        RoctxRange range(name);                        // a ROCTX range per kernel class launch (rocprofv3 --marker-trace)
        if (htrace || ptrace) hmark(std::string("L:") + name);
        if (!prof) { f(); if (htrace || ptrace) hmark(std::string("l:") + name); return; }
        int k = statIndex(name);
        hipEvent_t a = ev(), b = ev();
        HIP_OK(hipEventRecord(a, stream));
        f();
        HIP_OK(hipEventRecord(b, stream));
        pending.push_back({k, {a, b}});
        stats[k].launches++;
        stats[k].bytes += algoBytes;
    }
    void addBytes(const char* name, uint64_t b) {
        if (prof) stats[statIndex(name)].bytes += b;
    }
    void collectTimings() {
        if (!prof) return;
        for (auto& p : pending) {
            HIP_OK(hipEventSynchronize(p.second.second));
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, p.second.first, p.second.second));
            stats[p.first].ms += ms;
        }
        pending.clear();
        eventNext = 0;
    }
};

namespace ngx {

inline int32_t fail(ngx_ctx* c, int32_t code, const std::string& msg) {
    c->lastError = msg;
    return code;
}

inline Space* findSpace(ngx_ctx* c, int32_t id) {
    auto it = c->spaces.find(id);
    return it == c->spaces.end() ? nullptr : it->second.get();
}

template <typename T>
T readScalar(ngx_ctx* c, const T* dev) {
    T v;
    HIP_OK(hipMemcpyAsync(&v, dev, sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return v;
}

// engine.cpp's pieces the operators build on
bool ttlInfo(const SchemaSet* ss, int32_t& col, int64_t& dur);
HopSlots makeHopSlots(const Space& sp, const DeviceGraph& d, const std::vector<int32_t>& types, std::vector<int32_t>& hopTypes);
void stageSeeds(ngx_ctx* c, const std::vector<int32_t>& parts, const std::vector<int64_t>& vids, int32_t* dpart, int64_t* dvid);
int32_t goCall(ngx_ctx* c, const ngx_go_plan* p, ngx_go_result** out);   // ngx_go under the caller's lock of c->mu
int32_t resultDigest(ngx_ctx* c, const ngx_go_result* r, uint64_t out[3]);

// The result of an operator that answers in cells (ngx_group_result, ngx_order_result, ngx_set_result,
// ngx_fetch_result, ngx_lookup_result): the C struct points into these vectors.
template <typename Res>
struct CellResult {
    Res r{};
    std::vector<int32_t> colTypes;
    std::vector<ngx_cell> cells;
    std::string strings;
};
static_assert(sizeof(GroupCell) == sizeof(ngx_cell) && offsetof(GroupCell, v) == offsetof(ngx_cell, v), "GroupCell is ngx_cell");

// body() under try / catch: an Error becomes the context's last error and the call's code. A failed call may leave
// kernels enqueued that read descriptors or scratch the next call rewrites; `sync` says when the stream is drained.
enum class OnFail { kNoSync, kSyncIfThrown, kSync };
template <typename Body>
int32_t guarded(ngx_ctx* c, OnFail sync, Body&& body) {
    int32_t rc;
    bool thrown = false;
    try {
        rc = body();
    } catch (const Error& e) {
        rc = fail(c, e.code, e.msg);
        thrown = true;
    }
    if (rc != NGX_OK && (sync == OnFail::kSync || (sync == OnFail::kSyncIfThrown && thrown))) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// A C entry point after its argument checks: the context's lock, a holder H (its .r is the C result), body(H&)
// guarded, the code and *out set.
template <typename H, typename Res, typename Body>
int32_t abiCall(ngx_ctx* c, Res** out, OnFail sync, Body&& body) {
    std::lock_guard<std::mutex> g(c->mu);
    auto R = std::make_unique<H>();
    const int32_t rc = guarded(c, sync, [&] { return body(*R); });
    R->r.code = rc;
    *out = &R.release()->r;
    return rc;
}

// the two events device_ms is measured between (made on the first call, kept); [0] is recorded by the operator
inline void resultEvents(ngx_ctx* c) {
    HIP_OK(hipSetDevice(c->device));
    for (hipEvent_t& e : c->gbEv)
        if (!e) HIP_OK(hipEventCreate(&e));
}

// The tail of an operator that answers in cells: the second event, the cells and string bytes copied to the
// holder (enqueueMore() adds the operator's own copies), the stream synchronised, device_ms and the timings read,
// the result pointed at the holder.
template <typename H, typename More>
void finishCells(ngx_ctx* c, H& R, const GroupCell* cellsDev, uint64_t ncells, const char* strDev, uint64_t strBytes, More&& enqueueMore) {
    HIP_OK(hipEventRecord(c->gbEv[1], c->stream));
    R.cells.resize(ncells);
    if (ncells) HIP_OK(hipMemcpyAsync(R.cells.data(), cellsDev, ncells * sizeof(ngx_cell), hipMemcpyDeviceToHost, c->stream));
    R.strings.resize(strBytes);
    if (strBytes) HIP_OK(hipMemcpyAsync(&R.strings[0], strDev, strBytes, hipMemcpyDeviceToHost, c->stream));
    enqueueMore();
    HIP_OK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, c->gbEv[0], c->gbEv[1]));
    c->collectTimings();
    R.r.device_ms = ms;
    R.r.cells = R.cells.data();
    R.r.strings = R.strings.data();
    R.r.strings_len = strBytes;
}
template <typename H>
void finishCells(ngx_ctx* c, H& R, const GroupCell* cellsDev, uint64_t ncells, const char* strDev, uint64_t strBytes) {
    finishCells(c, R, cellsDev, ncells, strDev, strBytes, [] {});
}

}  // namespace ngx
