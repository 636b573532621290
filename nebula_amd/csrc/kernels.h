// Host-visible launchers and argument blocks of kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "kargs.h"

namespace ngx {

// host-mapped publication slot of a scan total: slot[0] = value, slot[2] = an extra word (the final
// hop's error bits), slot[1] = pubTag(seq, value, extra). The three are relaxed system-scope stores: a
// release would make the kernel write back every dirty L2 line first (buffer_wbl2, measured on the
// critical path of the seed / compaction / close kernels), and the host needs no device data ordered
// before the value, only the value itself, which it accepts when slot[1] matches the tag of what it
// read (a slot caught between stores mismatches and is polled again).
struct Publish {
    uint64_t* slot;
    uint64_t seq;
};
__host__ __device__ inline uint64_t pubMix(uint64_t x) {
    x ^= x >> 31;
    x *= 0x7fb5d329728ea185ULL;
    x ^= x >> 27;
    x *= 0x81dadef4bc2dd44dULL;
    return x ^ (x >> 33);
}
__host__ __device__ inline uint64_t pubTag(uint64_t seq, uint64_t value, uint64_t extra, uint64_t extra2) {
    return pubMix(seq ^ pubMix(value + 0x9e3779b97f4a7c15ULL) ^ pubMix(extra ^ 0x2545f4914f6cdd1dULL) * 3 ^
                  pubMix(extra2 + 0x632be59bd9b4e019ULL) * 5);
}
// slot[3]: a second extra word (the final hop's packed (|F|, E) when its grid came from the device)
__device__ inline void publishWords(uint64_t* slot, uint64_t seq, uint64_t value, uint64_t extra, uint64_t extra2 = 0) {
    __hip_atomic_store(slot, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 2, extra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 3, extra2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 1, pubTag(seq, value, extra, extra2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (part, vid) -> shard vertex row: open-addressing table (linear probing, power-of-two capacity
// >= 2V, built at commit) so a seed lookup is ~1 probe instead of a binary search over V rows
struct VIndexSlot {
    int64_t vid;
    int32_t part;
    uint32_t row;                       // kNoRow: empty
};
struct VIndex {
    const VIndexSlot* slots;
    uint64_t mask;                      // capacity - 1
};
__host__ __device__ inline uint64_t vindexHash(int32_t part, int64_t vid) {
    uint64_t h = static_cast<uint64_t>(vid) * 0x9E3779B97F4A7C15ULL ^ static_cast<uint64_t>(static_cast<uint32_t>(part)) * 0xC2B2AE3D27D4EB4FULL;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ULL;
    return h ^ (h >> 32);
}

#ifdef __HIPCC__
// linear probing, two slots per round trip: both loads issue before either is compared (most keys
// resolve in the first pair at the index's load factor)
// Two slots per round trip, each one 16-byte load, both issued before either is examined, and the
// outcome picked by selects (a probe written with early returns let the compiler split each slot
// into a row load and a key load behind branches: four dependent loads per probe pair, r04 ISA).
__device__ __forceinline__ uint4 vindexSlot(const VIndex& idx, uint64_t h) {
    return reinterpret_cast<const uint4*>(idx.slots)[h];
}
__device__ __forceinline__ uint32_t vindexFind(const VIndex& idx, int32_t part, int64_t vid) {
    uint64_t h = vindexHash(part, vid) & idx.mask;
    const uint32_t vlo = static_cast<uint32_t>(vid), vhi = static_cast<uint32_t>(static_cast<uint64_t>(vid) >> 32);
    for (uint64_t probe = 0; probe <= idx.mask; probe += 2) {
        const uint4 a = vindexSlot(idx, h), b = vindexSlot(idx, (h + 1) & idx.mask);
        const bool aHit = a.x == vlo && a.y == vhi && a.z == static_cast<uint32_t>(part) && a.w != kNoRow;
        const bool bHit = b.x == vlo && b.y == vhi && b.z == static_cast<uint32_t>(part) && b.w != kNoRow;
        const bool done = aHit || a.w == kNoRow || bHit || b.w == kNoRow;   // found, or an empty slot ends the run
        const uint32_t r = aHit ? a.w : a.w == kNoRow ? kNoRow : bHit ? b.w : kNoRow;
        if (done) return r;
        h = (h + 2) & idx.mask;
    }
    return kNoRow;
}
#endif

// seed hop (n seeds, n * hs.n <= kSeedFuseMax entries): launchSeedFrontierCf below
constexpr uint64_t kSeedFuseMax = 4096;

// multi-root walk (engine.cpp runPipe): the roots of one walk, one bit of a row's 64-bit root set each
constexpr uint64_t kRootBatch = 64;

int launchIndexLookup(const int32_t* qpart, const int64_t* qvid, uint64_t n, VIndex idx, uint32_t* out, hipStream_t s);
int launchLookup(const int32_t* qpart, const int64_t* qvid, uint64_t n, const int32_t* vpart, const int64_t* vid,
                 uint64_t V, uint32_t* out, hipStream_t s);
// estart must hold nEnt + 1 entries; estart[nEnt] receives E
int launchDegreeScan(const uint32_t* F, uint64_t nEnt, const HopSlots& hs, uint64_t* estart, uint64_t* tileSums,
                     hipStream_t s, Publish pub = Publish{nullptr, 0});
// chunkFirst must hold ceil(E / kChunk) entries (estart[nEnt] = E)
int launchChunkFirst(const uint64_t* estart, uint64_t nEnt, uint64_t* chunkFirst, hipStream_t s, uint64_t* zero = nullptr,
                     uint64_t nzero = 0);
// mask (nullptr: every edge): only hop edges e with mask[e] != 0 are expanded
// dyn != nullptr (device-driven hop): E / nEnt are upper bounds, the real ones are read from *dyn; the
// kernel does nothing when the real E >= pullMinE (the pull kernels take that hop)
constexpr uint64_t kDynGrid = 2048;                // workgroups of a device-driven (grid-stride) launch
int launchExpandMark(const uint32_t* F, const uint64_t* estart, const uint64_t* chunkFirst, uint64_t nEnt, uint64_t E,
                     const HopSlots& hs, uint8_t* visited, uint8_t epoch, bool pos32, hipStream_t s,
                     const uint8_t* mask = nullptr, const uint64_t* dyn = nullptr, uint64_t pullMinE = ~0ULL,
                     const uint64_t* ebase = nullptr);   // ebase: FinalArgs::ebase
// storage outcome per hop edge (a.E entries of out: 1 = emitted) for the max-edges / TTL mask path;
// a's F / estart / chunkFirst / hs / env / P / propsMask / ttl fields are read
int launchStoragePass(const FinalArgs& a, uint8_t* out, hipStream_t s);
// keep the first `cap` set flags of every frontier entry's hop edges, clear the others
int launchCap(const uint64_t* estart, uint64_t nEnt, uint8_t* mask, int64_t cap, hipStream_t s);
int launchCompact(const uint8_t* visited, uint64_t gbase, uint64_t V, uint8_t epoch, uint32_t* outF,
                  uint64_t* tileSums, uint64_t* count, hipStream_t s);
// fused compaction + next-hop degree scan (kernels.hip FlagDegIn): outF gets the next frontier,
// estart its entries' edge offsets (|F| * hs.n + 1 entries, the last = E), *packedTotal = |F| << kFdShift | E.
// Requires V < 2^(64 - kFdShift) and the slots' total edges < 2^kFdShift.
constexpr int kFdShift = kDynShift;
constexpr uint64_t kFdMask = kDynMask;
int launchCompactDegrees(const uint8_t* visited, uint64_t gbase, uint64_t V, uint8_t epoch, const HopSlots& hs,
                         uint32_t* outF, uint64_t* estart, uint64_t* tileSums, uint64_t* packedTotal, hipStream_t s,
                         Publish pub = Publish{nullptr, 0});
// Compaction of an intermediate hop (kernels.hip k_compact_count + k_compact_write): visited[row] ==
// epoch -> next frontier outF (row order), its entries' estart (|F| * hs.n + 1 entries, the last = E)
// and the next hop's chunk heads chunkFirst (what k_chunk_first computes). Two launches over tiles of
// kCompactTile rows: the first writes each tile's and each wave's packed (count << kFdShift | degree)
// total, the second sums the totals before its tile (no inter-workgroup waiting: the r02 single-pass
// look-back spent most of its 20-38 us on tickets and polling) and writes the rows. Wave w of a tile
// owns rows w * 1024 + k * 64 + lane (k < 16): every mark / offset load of a wave is one coalesced
// access. bits != nullptr: also the frontier bitmap (one 64-bit word per 64 rows, every word of the
// shard written) for the next hop's pull.
struct CompactArgs {
    const uint8_t* visited;             // this shard's rows (visited + gbase)
    uint64_t V;
    HopSlots hs;
    uint32_t* outF;
    uint64_t* estart;
    uint64_t* ebase;                    // optional: the entries' CSR positions (FinalArgs::ebase)
    uint64_t* chunkFirst;
    uint64_t cfCap;                     // entries of chunkFirst (overflow sets err[3])
    uint64_t* tileSum;                  // one word per tile (written by the count launch)
    uint64_t* waveSum;                  // NW words per tile
    uint64_t* total;                    // device copy of the packed total
    Publish pub;
    uint64_t* zero;                     // words the next final kernel needs cleared (zero[k * kDoneOff], k < nzero)
    uint32_t nzero;
    uint32_t* clear32;                  // optional word cleared by the count launch (the pull's segment counter)
    uint32_t* err;
    uint8_t epoch;
    uint64_t* bits;                     // optional frontier bitmap of this shard's rows (V / 64 words, rounded up)
    int32_t laneRows;                   // rows per lane, 4 / 8 / 16; 0: the launcher picks by V (kernels.hip)
    int32_t wgThreads;                  // 1024 (0) or 256 threads per workgroup (256: 16 rows per lane, the same
                                        // 4096-row tile; a workgroup that fits beside another query's final hop)
    int32_t bitsZero;                   // write every word of `bits` as 0 (no hop reads this frontier's bitmap:
                                        // the next hop is the final one), leaving it clean for a sparse hop
    int32_t countOnly;                  // dense final hop next (FinalArgs::denseMark): the count launch, then
                                        // one workgroup summing its tile totals into *total; no rows written
    int32_t totalByClose;               // countOnly, the total read on the device only: no summing launch, the
                                        // final hop's close sums the tile words (FinalArgs::dynTiles)
};
// Sparse intermediate hop (world 1, push, E far below the shard's rows): the expansion builds the next
// frontier itself instead of a compaction sweeping every row (kernels.hip k_expand_sparse). Per edge one
// 64-bit atomicOr on the frontier bitmap (all zero before the launch) dedups the destination and sets the
// pull's bitmap; the rows whose bit an edge set are the next frontier. Each workgroup reserves its new
// rows' places and edge offsets with one packed atomicAdd, so every entry gets estart / ebase / chunk
// heads without a scan; the last workgroup writes the tail estart[|F| ns] = E, the packed total and its
// publication, and clears the counters. Frontier order = reservation order (a set: GoExecutor keeps the
// dsts of a hop in an unordered set too, GoExecutor.cpp:675-718).
struct SparseArgs {
    const uint32_t* F;
    const uint64_t* estart;
    const uint64_t* chunkFirst;
    const uint64_t* ebase;              // optional (FinalArgs::ebase)
    uint64_t nEnt;
    uint64_t E;
    const uint64_t* dynIn;              // or null: packed (|F| << kDynShift | E) of this hop on the device (the
                                        // launch is then a fixed grid striding over the hop's slices)
    HopSlots hs;
    uint64_t* bits;                     // the shard's frontier bitmap, zero before the launch
    uint64_t bitWords;                  // its words
    uint32_t* outF;
    uint64_t* outEst;                   // next hop: estart, |F| * ns + 1 entries
    uint64_t* outEbase;                 // next hop: the entries' CSR positions, or null
    uint64_t* outCf;                    // next hop: chunk heads
    uint64_t cfCap;
    uint64_t* ctl;                      // [0] packed (rows << kFdShift | edges) reserved, [1] finished workgroups
    uint64_t* total;                    // device copy of the packed total
    Publish pub;
    uint32_t* err;
};
int launchExpandSparse(const SparseArgs& a, bool pos32, hipStream_t s);
constexpr uint64_t kCompactLbMaxV = 1ULL << (62 - kFdShift);
constexpr uint64_t kCompactTile = 4096;     // the smallest compaction tile (1024 threads x 4 rows; 8 or 16 per lane on larger shards): sizes the per-tile words
// GO final kernel words: kargs.h (kResv*, kDoneOff). The seed / compaction kernels clear zero[k * kDoneOff]
// for k < nzero.
int launchCompactLb(const CompactArgs& a, hipStream_t s);
// tile words the count launch of launchCompactLb(a) writes (a.tileSum[0 .. n))
uint64_t compactLbTiles(const CompactArgs& a);
// seed hop variant that also writes chunkFirst (cfCap entries) and clears zero[0 .. nzero)
int launchSeedFrontierCf(const int32_t* qpart, const int64_t* qvid, uint64_t n, VIndex idx, const HopSlots& hs,
                         uint32_t* F, uint64_t* estart, Publish pub, uint64_t* chunkFirst, uint64_t cfCap,
                         uint64_t* zero, uint32_t nzero, uint32_t* err, hipStream_t s, uint64_t* packedOut = nullptr,
                         uint64_t* zero8 = nullptr,      // zero8: 8 words cleared first (the query's counters)
                         uint64_t* ebase = nullptr);     // ebase: the entries' CSR positions (FinalArgs::ebase)
// QueryResponse rows of GetNeighbors (storage.thrift IdAndProp.props): per returned edge, the RowWriter
// row of its type's response edge schema (QueryBoundProcessor.cpp:38-43 with collectProps,
// QueryBaseProcessor.inl:325-399). Two launches: write == false stores each row's length in rowLen,
// write == true writes the bytes at rowOff (the exclusive scan of rowLen).
constexpr int32_t kRcSrc = -1, kRcRank = -2, kRcType = -3;    // key props of a response column
constexpr int kMaxRespCols = 128;                             // response columns per edge type
struct RowEncArgs {
    uint64_t n;
    const int32_t* oType;               // signed type per row
    const int64_t* oSrc;
    const int64_t* oRank;
    const uint8_t* oFlags;              // EF_* per row (EF_EMPTY_VALUE: no RowReader), nullptr: none
    const OutCol* cols;                 // the request's return columns (device array)
    int32_t nslots;
    int32_t etype[kMaxSlots];
    int32_t cbeg[kMaxSlots + 1];        // response columns of slot s: [cbeg[s], cbeg[s + 1])
    const int32_t* rcSrc;               // request column index, or kRcSrc / kRcRank / kRcType
    const int32_t* rcType;              // response field type (NGX_T_*)
    uint64_t* rowLen;
    const uint64_t* rowOff;
    uint8_t* out;
};
int launchEncodeRows(const RowEncArgs& a, bool write, hipStream_t s);
// out[0 .. n) = exclusive prefix of in, out[n] = total (3-phase scan, tileSums as launchDegreeScan)
int launchScanU64(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* tileSums, hipStream_t s);
// v[0 .. n) -> exclusive prefix in place, v[n] = total (one 1024-thread workgroup: n up to ~1e6)
int launchScanInPlace(uint64_t* v, uint64_t n, hipStream_t s);

// ngx_go_result_digest: per row h = mix64(... mix64(mix64(kDigestSeed ^ key) ^ col0) ...) over the row's
// src vid and each listed column's value bits (integers sign-extended from their width w, or the constant
// c when w == 0); out[0] += h (mod 2^64), out[1] ^= h, out[2] += rows. Order-independent, so two result
// multisets compare without a sort (oracle/orc_digest.cpp restates it on the host).
constexpr int kDigestMaxCols = 16;
constexpr uint64_t kDigestSeed = 0x9E3779B97F4A7C15ULL;
struct DigestArgs {
    uint64_t n;
    int32_t ncols;                      // columns after the key
    const void* x[kDigestMaxCols + 1];  // [0] the src vids, then the columns
    int32_t w[kDigestMaxCols + 1];      // bytes per element, 0: constant
    int64_t c[kDigestMaxCols + 1];
    uint64_t* out;                      // 3 words, zeroed by the launcher
};
int launchRowDigest(const DigestArgs& a, hipStream_t s);

// k_final_close_cols: the arrays a close moves (kind 0: plain, w bytes; 1: 8-byte string values
// rebased with their arena slots; 2: 8-byte word w of each row's string-arena block)
struct CloseCol {
    void* p;
    int32_t w;
    int32_t kind;
};
constexpr int kCloseMaxCols = 32;
// the FinalArgs fields k_final_close_cols reads (same names and meaning)
struct CloseArgs {
    uint64_t* resvCtl;
    uint64_t* resvTab;
    uint64_t* resvNext;
    uint32_t* err;
    uint64_t* rowsPub;
    uint64_t rowsSeq;
    char* strOut;
    uint64_t oBase;
    const uint64_t* dynTotal;           // the final hop's packed (|F|, E) on the device, published beside R
    const uint64_t* dynTiles;           // when set: *dynTotal = the sum of these words, written by the close
    uint64_t nDynTiles;
    uint32_t resvTB, resvSeq, resvG, resvShift, resvStride, nStrOut;
};
struct CloseCols {
    CloseCol c[kCloseMaxCols];
    int32_t n;
};

// final hop, one pass (interpreter kernel). a.oEntry set (GetNeighbors): a.lbStatus zeroed, ceil(E /
// kChunk) + 1 words; outputs sized for a.oBase + a.E rows; rows in edge order, rows written = the
// inclusive status of the last chunk. Else (GO): the kResv words of a.lbStatus zeroed, outputs sized for
// a.oBase + a.E + resvSlack() rows, chunks' rows in per-group blocks; launchFinalClose must follow.
int launchFinal(const FinalArgs& a, hipStream_t s, unsigned grid = 0);   // grid 0: one workgroup per chunk of a.E
// GO final hop, after the final kernel (generated or interpreter) on the same stream: the rows past the
// row count moved into the holes of the groups' last blocks, then rows = lbStatus[0] and the row count
// and the query's error bits (bit k = a.err[k] != 0) published to a.rowsPub when set
int launchFinalClose(const FinalArgs& a, hipStream_t s);
// resident workgroups per CU of the interpreter final kernel launchFinal would run for `a`
int finalOccupancy(const FinalArgs& a);

// Direction-optimizing ("pull", Beamer et al. SC'12) intermediate hop, one shard holding every row:
// row r joins the next frontier iff one of its in-neighbours over a hop slot's MIRROR slot (-t for t,
// verified at commit to be the exact transpose of t) is in the current frontier (cur[g] == curEp).
// Same set as the push expansion (getDstIdsFromResp, GoExecutor.cpp:675-718), fewer random accesses
// when the frontier's edges outnumber the shard's rows.
//
// Row pass over a per-slot "head" image built at commit (sliced ELLPACK, SELL-64-sigma): rows are
// taken in slices of 64 (one wave each); inside windows of kPullWindow rows the rows are ordered by
// min(in-degree, kPullK) descending (perm), and the first kPullK in-neighbours of every row are stored
// column-major per slice (head[slice][k][lane]), largest source out-degree first, so one probe round
// of a wave is ONE coalesced 256-byte load and most reached rows hit on their first probe (a frontier
// reached by expansion is hub-heavy). The old row-per-thread pass loaded 8 in-neighbours of its own
// in-list per lane: ~54 distinct cache lines per wave load, address-unit bound (r02: 60 us at C2).
// Rows still open after their kPullK head entries (in-degree > kPullK) reserve segment words; the
// segment pass probes their whole in-list in the mirror CSR (kPullSeg in-edges per workgroup, so a
// supernode spreads over many workgroups). Reached rows get out[r] = ep. ctl[0..3) is zero between
// launches (the segment pass's last workgroup leaves it so).
constexpr int kPullMaxSlots = 4;
constexpr int kPullK = 16;                  // head entries per row (a multiple of 4)
constexpr uint64_t kPullWindow = 2048;      // rows sorted by head length inside windows of this size
constexpr uint32_t kPullLong = 0x80000000u; // perm word flag: in-degree > kPullK (row = word & ~flag)
constexpr uint64_t kPullSeg = 1024;
struct PullArgs {
    int32_t n;
    const uint64_t* ioff[kPullMaxSlots];   // mirror slot CSR offsets (V + 1)
    const uint32_t* isrc[kPullMaxSlots];   // mirror slot dgid: global row of each in-neighbour
    const uint32_t* perm[kPullMaxSlots];   // [slice * 64 + lane]: row | kPullLong, kNoRow past the rows
    const uint32_t* head[kPullMaxSlots];   // [(slice * kPullK + k) * 64 + lane]: k-th in-neighbour or kNoRow
    const uint8_t* nk[kPullMaxSlots];      // per slice: max over its rows of min(in-degree, kPullK)
    uint64_t sliceEnd[kPullMaxSlots];      // inclusive prefix of the slots' slice counts
    const uint64_t* curBits;               // frontier bitmap over global rows (bit g of word g / 64)
    uint8_t* out;                          // this shard's marks (marks + gbase)
    uint64_t V;
    uint64_t* seg;
    uint64_t segCap;
    uint32_t* ctl;                         // [0] segments reserved (zero between hops: CompactArgs::clear32)
    uint32_t* err;                         // [3] queue overflow / spin limit (device fault)
    uint8_t curEp, ep;
    const uint64_t* dyn;                   // device-driven hop: packed totals; the row pass does nothing when
    uint64_t minE;                         // the hop's E < minE (the push expansion takes it)
};
// worst-case queue words: (rows with in-degree > kPullK) * n + in-edges / kPullSeg + 1
int launchPull(const PullArgs& a, hipStream_t s);
// marks[F[i]] = ep for the rows of a frontier list (kNoRow entries skipped)
int launchMarkRows(const uint32_t* F, uint64_t n, uint8_t* marks, uint8_t ep, hipStream_t s);
// end of a query: err[0..4) as bits and extra[0 .. nExtra) to host-mapped slot[1 ..], then slot[0] = seq
int launchPublishTail(const uint32_t* err, const uint64_t* extra, int nExtra, uint64_t* slot, uint64_t seq, hipStream_t s);
// bits of a frontier list's rows set in a bitmap (zeroed by the caller)
int launchMarkBits(const uint32_t* F, uint64_t n, uint64_t* bits, hipStream_t s);
// world > 1 pull: the all-gathered shard bitmaps (segWords words each, local row order) -> one bitmap
// over global rows (shard q's rows start at sb[q])
constexpr int kMaxWorld = 64;
struct RepackArgs {
    const uint64_t* seg;
    uint64_t segWords;
    uint64_t sb[kMaxWorld + 1];
    int world;
    uint64_t* out;
    uint64_t outWords;
};
int launchRepackBits(const RepackArgs& a, hipStream_t s);
// multi-root walk (pipes): every destination of a frontier row ORs in the row's root set (64-bit
// masks over rows) and is marked `epoch`; roots[F[i]] |= bits[i]; out[i] = roots[F[i]]
int launchExpandRoots(const uint32_t* F, uint64_t nF, const HopSlots& hs, const uint64_t* rootsCur, uint64_t* rootsNext,
                      uint8_t* visited, uint8_t epoch, hipStream_t s);
int launchScatterRoots(const uint32_t* F, uint64_t n, const uint64_t* bits, uint64_t* roots, hipStream_t s);
int launchGatherRoots(const uint32_t* F, uint64_t n, const uint64_t* roots, uint64_t* out, hipStream_t s);
// world > 1 multi-root walk: out[i] = own[i] | recv[q * stride + i] over the peers q != rank (the root
// sets the peers' expansions gave this shard's rows), i < n
int launchMergeRoots(const uint64_t* own, const uint64_t* recv, uint64_t stride, uint64_t n, int world, int rank,
                     uint64_t* out, hipStream_t s);
// YIELD DISTINCT on the device (GoExecutor::processFinalResult, GoExecutor.cpp:1298-1305): one row of
// every group of rows with equal YIELD values is kept. Values are equal when their value types are
// equal and their bits are, doubles by value (0.0 == -0.0, NaN == NaN: what the reference's
// boost::hash_range key makes equal), strings by bytes. An open-addressing table (capacity a power of
// two >= 2n, zeroed) holds (hash high 32 bits << 32 | row + 1); a row either claims an empty slot
// (keep[r] = 1) or meets an equal row's slot (keep[r] = 0). Which of equal rows is kept is not fixed
// (GO rows have no fixed order; only the values are returned).
constexpr int kMaxDistinctCols = 64;
struct DistinctArgs {
    uint64_t n;
    int32_t nY;
    const OutCol* cols;                 // nY result columns (device array)
    uint8_t vt[kMaxDistinctCols];       // V_* of column y's rows when cols[y].t is null
    uint64_t* table;
    uint64_t mask;
    uint64_t* keep;                     // n entries
};
int launchDistinctMark(const DistinctArgs& a, hipStream_t s);
// rows r with keep[r] move to pre[r] (exclusive scan of keep) in every array: k arrays of esz-byte
// elements, src -> dst
constexpr int kMaxScatter = 48;
struct ScatterArgs {
    uint64_t n;
    const uint64_t* keep;
    const uint64_t* pre;
    int32_t k;
    const uint8_t* src[kMaxScatter];
    uint8_t* dst[kMaxScatter];
    uint8_t esz[kMaxScatter];
};
int launchScatterKept(const ScatterArgs& a, hipStream_t s);
// GROUP BY over a device-resident result (groupby.hip; ngx_go_group_by). A column as the kernels read it:
// `w` bytes per element of x (1 / 2 / 4 signed, 8; 0: no array, every row holds konst); strings are
// 8-byte device pointers with their lengths in len.
constexpr int kGroupMaxKeys = 4;
constexpr uint64_t kGroupLdsBytes = 64 * 1024;      // the LDS copy of the state one workgroup may hold
constexpr uint32_t kGroupLdsGridMax = 1024;         // workgroups of the LDS accumulation (each flushes its copy once)
enum { kGroupInt = 0, kGroupDouble = 1, kGroupString = 2 };
struct GroupCol {
    const void* x;
    const uint32_t* len;
    int64_t konst;
    int32_t w;
    int32_t kind;                       // kGroupInt (int / vid / timestamp / bool bits), kGroupDouble, kGroupString
};
// rows with equal values in the nk columns share a leader (the row that claimed their table slot):
// flag[r] = 1 for leaders, leader[r] = the leader's row (may be null: only the flags are wanted).
// table: capacity mask + 1 >= 2n, a power of two, zeroed.
struct GroupAssignArgs {
    uint64_t n;
    int32_t nk;
    GroupCol k[kGroupMaxKeys + 1];      // the keys, plus the value column of a COUNT_DISTINCT pass
    uint64_t* table;
    uint64_t mask;
    uint32_t* leader;
    uint64_t* flag;
};
int launchGroupAssign(const GroupAssignArgs& a, hipStream_t s);
// one 64-bit state word per (slot, group): state[slot * ngroups + g] op= the row's value
enum { kGroupAdd = 0, kGroupAddF64, kGroupAnd, kGroupOr, kGroupXor, kGroupMax, kGroupMin };
enum { kGroupSrcOne = 0, kGroupSrcCol, kGroupSrcOrdered, kGroupSrcFlag };   // 1, cols[col], its order key (double), flag[r]
struct GroupSlot {
    int32_t op;
    int32_t src;
    int32_t col;
    int32_t pad;
    const uint64_t* flag;
};
struct GroupAccumArgs {
    uint64_t n, ngroups;
    int32_t nslots;
    const GroupSlot* slots;             // device arrays
    const GroupCol* cols;
    const uint32_t* leader;
    const uint64_t* pre;                // exclusive scan of the leader flags: pre[leader row] = group id
    uint64_t* state;                    // nslots * ngroups words, initialised by the launcher
};
// lds: every workgroup aggregates into an LDS copy of the state (nslots * ngroups * 8 <= kGroupLdsBytes).
// gridMax (flag group_grid_max): most workgroups of either accumulation, 0: the built-in caps
int launchGroupAccum(const GroupAccumArgs& a, bool lds, uint32_t gridMax, hipStream_t s);
// one output cell per (group, yield column), laid out as ngx_cell
struct GroupCell {
    int32_t kind;
    int32_t len;
    int64_t v;                          // value bits, or the offset of a string's bytes in strOut
};
enum { kEmitKey = 0, kEmitState, kEmitOrdered, kEmitAvgInt, kEmitAvgF64, kEmitConst };
struct GroupEmit {
    int32_t kind;                       // NGX_CELL_*
    int32_t src;                        // kEmit*
    int32_t a;                          // kEmitKey: column; state kinds: slot (AVG: sum slot, count slot + 1)
    int32_t pad;
    int64_t konst;
};
struct GroupEmitArgs {
    uint64_t n, ngroups;
    int32_t ny;
    const GroupEmit* emit;              // device arrays
    const GroupCol* cols;
    const uint64_t* flag;
    const uint64_t* pre;
    const uint64_t* state;
    const uint64_t* strPre;             // exclusive scan of launchGroupStrLen's lengths; null: no string cells
    char* strOut;
    GroupCell* cells;                   // ngroups * ny
};
int launchGroupStrLen(const GroupEmitArgs& a, uint64_t* slen, hipStream_t s);
int launchGroupEmit(const GroupEmitArgs& a, hipStream_t s);
// the group rows as columns instead of cells (ngx_go_group_order_by: the radix select of orderby.hip reads them
// in place as GroupCols). One array of ngroups values per yield column, indexed by the group id: `w` bytes a
// value (8, or the narrowest signed width that holds the input's row count for a COUNT / COUNT_DISTINCT); a
// string key keeps its bytes where they are and writes its device pointer (8 bytes) and its length.
// x null: a constant yield, no array (the column has width 0).
struct GroupColumnOut {
    void* x;
    uint32_t* len;                      // string key columns only
    int32_t w;                          // 1 / 2 / 4 / 8
    int32_t pad;
};
struct GroupColumnsArgs {
    uint64_t n, ngroups;
    int32_t ny;
    const GroupEmit* emit;              // device arrays
    const GroupCol* cols;
    const uint64_t* flag;
    const uint64_t* pre;
    const uint64_t* state;
    const GroupColumnOut* out;          // ny entries
};
int launchGroupColumns(const GroupColumnsArgs& a, hipStream_t s);
// ORDER BY ... LIMIT over a device-resident result (orderby.hip; ngx_go_order_by): the K first rows of the
// order are selected by an MSD radix select over levels. A level is one order-preserving unsigned word per
// row of `bits` significant bits (a multiple of 8), consumed 8 bits a step from the top:
//   kOrdInt     the value sign-extended from its stored width plus 2^(bits - 1): bits = 8 * stored width
//   kOrdDouble  the bits with -0.0 read as +0.0, then all flipped for a negative value, else the sign bit
//               (a NaN is placed by its bits)
//   kOrdStrWord bytes [8 * word, 8 * word + 8) of the string, big-endian, zero-padded
//   kOrdStrLen  the string's length (after its ceil(maxlen / 8) words: a proper prefix orders first)
//   kOrdRow     the row's index in the result, always ascending: the last level, which makes the order total
// desc complements the word within its bits.
constexpr int kOrderMaxFactors = 8;
constexpr uint32_t kOrderMaxStr = 256;              // bytes of the longest string a factor column may hold
constexpr uint32_t kOrderCompactDiv = 16;           // the tied rows are listed once they are <= 1 / 16 of the rows read
constexpr uint32_t kOrderAppendBuf = 2048;          // row ids a workgroup collects in LDS before it reserves list space
constexpr uint32_t kOrderGridMax = 2048;            // workgroups (of 256 rows a sweep) of the count / collect kernels
enum { kOrdInt = 0, kOrdDouble, kOrdStrWord, kOrdStrLen, kOrdRow };
enum { kOrdTied = 0, kOrdWin = 1, kOrdOut = 2 };   // a row's mark
struct OrderLevel {
    int32_t col;                        // index into OrderArgs::cols
    int32_t kind;                       // kOrd*
    int32_t word;                       // kOrdStrWord: which 8 bytes
    int32_t desc;
    int32_t bits;
    int32_t pad;
};
// the selection's state, one copy in device memory. The pivot is the row of 0-based rank `rank` among the
// tied rows; rows below it win, rows above it are out. k_order_pick is the only writer of every field but
// the append counters (fill, nWin: one atomicAdd per LDS buffer flush), loopFlushes and err.
struct OrderState {
    uint64_t rank;
    uint64_t nTied;
    uint64_t listLen;                   // listed: entries of list[cur]
    uint64_t fill;                      // entries appended to list[cur ^ 1] by the running compaction
    uint64_t nWin;                      // entries appended to the winners
    uint32_t hasPrev, pLevel, pShift, pDigit;   // the digit decided last: rows marked lazily by the next pass
    uint32_t listed;                    // 0: the tied rows are the rows marked kOrdTied among all n; 1: list[cur] holds them
    uint32_t cur;
    uint32_t compacted;                 // the compaction after the last pick listed the tied rows in list[cur ^ 1]
    uint32_t done;                      // the pivot is known: no more counting
    uint32_t err;                       // a count that cannot be (no bucket holds the rank, a list past its capacity)
    // which paths the call took (flags order_compactions / order_list_compactions / order_loop_flushes)
    uint32_t compactions;               // picks that read the counts of a freshly compacted list
    uint32_t listCompactions;           // ... whose compaction read a list already (list -> list)
    uint32_t loopFlushes;               // LDS buffer flushes inside a sweep loop of k_order_collect: one atomicAdd each
};
struct OrderArgs {
    uint64_t n;
    const GroupCol* cols;               // device arrays
    const OrderLevel* levels;
    int32_t nlevels;
    uint8_t* mark;                      // n marks, kOrdTied at the start
    uint32_t* list[2];                  // listCap row ids each
    uint64_t listCap;
    uint64_t* hist;                     // 256 words, zero between steps (k_order_pick clears what it read)
    OrderState* S;
    uint32_t* win;                      // winCap winners' rows
    uint64_t winCap;
    uint32_t gridMax;                   // most workgroups of a sweep (flag order_grid_max); 0: kOrderGridMax
};
// max over len[0 .. n) into *out (zeroed by the launcher)
int launchOrderMaxLen(const uint32_t* len, uint64_t n, uint32_t* out, hipStream_t s);
// one step: count the tied rows' digit (level, shift) per workgroup in LDS, one flush each; pick the digit
// holding the rank; list the tied rows if they became few. Nothing runs once S->done is set.
int launchOrderStep(const OrderArgs& a, int level, int shift, bool last, hipStream_t s);
// after the last step: win[0 .. S->nWin) = the rows below the pivot and the pivot, in no order
int launchOrderGather(const OrderArgs& a, hipStream_t s);
// the rows' cells (as k_group_emit): every column of rows[i] (rows null: row base + i), i < m
struct OrderEmitCol {
    GroupCol c;
    const uint8_t* type;                // per-row value types of an UNKNOWN-typed column, else null
    int32_t cell;                       // NGX_CELL_* of a statically typed column
    int32_t pad;
};
struct OrderEmitArgs {
    uint64_t n, m, base;
    const uint32_t* rows;
    int32_t ncols;
    const OrderEmitCol* cols;           // device array
    const uint64_t* strPre;             // exclusive scan of launchOrderStrLen's lengths; null: no string cells
    char* strOut;
    GroupCell* cells;                   // m * ncols
};
int launchOrderStrLen(const OrderEmitArgs& a, uint64_t* slen, hipStream_t s);
int launchOrderEmit(const OrderEmitArgs& a, hipStream_t s);
// UNION DISTINCT / INTERSECT / MINUS over two device-resident results (setop.hip; ngx_set_op). Rows are named
// by one id over both sides: left row r is r, right row r is nL + r (nL + nR < 2^32 - 1). The table holds
// hash tag | id + 1 per slot, keyed on the whole row tuple (every column; as k_group_assign keys its key
// columns): integers compare sign-extended from their stored widths, so one value stored at two widths on the
// two sides is one key; doubles by value (-0.0 == 0.0); strings by length and bytes. A row with a NaN in any
// double column equals no row, itself included: it is never inserted and never found.
constexpr int kSetMaxCols = 16;
constexpr uint32_t kSetGridMax = 2048;              // workgroups (of 256 rows a sweep) of the build / probe kernels
enum { kSetUnionDistinct = 0, kSetIntersect = 1, kSetMinus = 2 };
struct SetState {
    uint64_t fill[2];                   // row ids appended to keep[side]: one atomicAdd per LDS buffer flush
    uint32_t err;                       // a table without a free slot, a list past its capacity: cannot be
    uint32_t loopFlushes;               // LDS buffer flushes inside a sweep loop of k_set_probe
};
struct SetArgs {
    uint64_t n[2];                      // rows of the left / right result
    const GroupCol* cols[2];            // device arrays, nc columns each
    int32_t nc;
    int32_t op;                         // kSet*
    uint64_t* table;                    // mask + 1 slots >= 2 * the rows inserted, a power of two, zeroed
    uint64_t mask;
    uint32_t* count;                    // kSetIntersect: per slot the rows equal to its leader (zeroed), else null
    uint32_t* taken;                    // kSetIntersect: per slot the tickets handed out (zeroed)
    uint32_t* keep[2];                  // kept rows of each side (local row ids), n[side] entries each, in no order
    SetState* S;
    uint32_t gridMax;                   // most workgroups of a sweep (flag set_grid_max); 0: kSetGridMax
};
// every row of `side` goes into the table: the row that claims a slot leads, count[slot] counts the rows equal to it
int launchSetBuild(const SetArgs& a, int side, hipStream_t s);
// every row of `side` looks its tuple up. kSetMinus keeps the rows not found; kSetIntersect those whose ticket
// (atomicAdd on taken[slot]) is below count[slot]; kSetUnionDistinct the rows that lead their slot (and NaN rows)
int launchSetProbe(const SetArgs& a, int side, hipStream_t s);
// FIND SHORTEST PATH over breadth-first levels (findpath.hip; ngx_find_path). A side (0: from the sources over the
// sentence's types, 1: from the targets over the opposite ones) keeps per row a 64-bit set: on the to side bit j is
// target j, on the from side bit 0 is "a source". A level is the compacted list of (row, the bits that reached the
// row at exactly that distance). Kernel boundaries order every hand-off; inside a kernel rows are shared through
// atomicOr only.
constexpr uint32_t kPathBuf = 1024;                 // path-DAG edges a workgroup collects in LDS before it reserves output space
constexpr uint32_t kPathGridMax = 2048;
constexpr uint32_t kPathAllUpto = 8;                // FIND ALL / NOLOOP PATH: the most UPTO (cum[] is UPTO words a row)
struct PathEdge {                                   // one edge of the path DAG, in path orientation (src nearer the sources)
    int64_t src, dst, rank;
    uint64_t mask;                                  // the targets whose shortest paths use it
    int32_t type;                                   // signed, as the path prints it
    int32_t layer;                                  // ALL / NOLOOP: the step of a walk the edge is (from 0); SHORTEST: 0
};
struct PathState {
    uint64_t touched[2];                            // rows an expansion reached first, per side
    uint64_t nLevel[2];                             // rows of the level a settle wrote, per side
    uint64_t found[2];                              // targets met by this step's odd / even meet
    uint64_t edges;                                 // path-DAG edges appended (may pass the capacity: nothing is written there)
    uint32_t loopFlushes;                           // LDS buffer flushes inside a sweep's edge loop
    uint32_t err;                                   // a list past its capacity: cannot be
};
// level 0 of a side: every looked-up row (kNoRow: the vid has no vertex) gets bit `firstBit + (perEntry ? i : 0)`;
// seen, newD, lvl and outMask may be null (the from side of ALL / NOLOOP needs the list of rows only)
int launchPathSeed(const uint32_t* rowsIn, uint64_t n, int perEntry, uint64_t* seen, uint64_t* newD, uint8_t* lvl,
                   uint32_t* outRows, uint64_t* outMask, uint64_t* count, hipStream_t s);
// every edge of a level's rows ORs the row's bits into inc[dst]; the lane whose OR found inc[dst] == 0 lists dst
int launchPathExpand(const uint32_t* rows, const uint64_t* masks, uint64_t n, const HopSlots& hs, uint64_t* inc, uint32_t* touched,
                     uint64_t cap, PathState* S, int side, hipStream_t s);
// after the expansion's ORs are complete: per touched row new = inc & ~seen, seen |= new, inc = 0; rows with new != 0
// form the next level (newD / lvl: the row's latest level and its bits, for the odd meet)
int launchPathSettle(const uint32_t* touched, uint64_t n, uint64_t* inc, uint64_t* seen, uint64_t* newD, uint8_t* lvl, uint8_t level,
                     uint32_t* outRows, uint64_t* outMask, PathState* S, int side, hipStream_t s);
// even meet: the to side's level-k rows that are the from side's level-k rows too. S->found[1] |= the targets not
// found before (foundPrev | S->found[0]); keepF / keepT[row] = those bits
int launchPathMeetEven(const uint32_t* rowsT, const uint64_t* masksT, uint64_t nMax, const uint8_t* fLvl, uint8_t level,
                       uint64_t foundPrev, uint64_t* keepF, uint64_t* keepT, PathState* S, hipStream_t s);
struct PathSweepArgs {
    const uint32_t* rows;                           // a level's rows, a wave per (row, slot)
    const uint64_t* masks;                          // their own bits; null: every bit (the from side)
    uint64_t n;
    HopSlots hs;
    const int64_t* vid;
    const uint64_t* keepCur;                        // sweep: the keep masks of the level beyond
    uint64_t* keepNext;                             // the rows' own keep masks (meet: the from side's)
    const uint8_t* tLvl;                            // meet: the to side's latest level per row and its bits
    const uint64_t* tNew;
    uint64_t* keepT;
    uint64_t notFound;
    PathEdge* out;
    uint64_t cap;
    PathState* S;
    uint8_t level;
    int32_t reverse;                                // to side: an edge row -> dst is the path step dst -> row, type negated
    uint32_t gridMax;
};
// meet == false: an edge into a row whose keepCur shares bits with this row's own mask is a path-DAG edge with those
// bits, and they join keepNext[row]. meet == true (odd meet): an edge into a row of the to side's level `level`
// whose bits are not found yet; the bits join keepNext[row], keepT[dst] and S->found[0]
int launchPathSweep(const PathSweepArgs& a, bool meet, hipStream_t s);
int launchPathClear(const uint32_t* rows, uint64_t n, uint64_t* arr, hipStream_t s);
// FIND ALL / NOLOOP PATH: one layer of the from side's walk. An edge of a layer row into row r is the layer-th step of
// a walk that can still end at a target iff m = cum[r] != 0, cum being the to side's "targets within UPTO - 1 - layer
// edges" word per row: it is emitted with m, and r is listed in `next` (null on the last layer) once, by the lane
// whose atomicMax raised stamp[r] to layer + 2. S->touched[0] counts the listed rows.
struct PathWalkArgs {
    const uint32_t* rows;                           // the layer's rows, a wave per (row, slot)
    uint64_t n;
    HopSlots hs;
    const int64_t* vid;
    const uint64_t* cum;
    uint32_t* stamp;
    uint32_t* next;
    uint64_t nextCap;
    PathEdge* out;
    uint64_t cap;
    PathState* S;
    int32_t layer;
    uint32_t gridMax;
};
int launchPathWalk(const PathWalkArgs& a, hipStream_t s);

// FETCH PROP ON tags / an edge type over keys in HBM (fetch.hip; ngx_fetch). Keys are read in place at their stored
// widths, sign-extended (GroupCol, as the set operator reads a result's columns). Three steps, every one a sweep of
// 256 keys a workgroup and turn:
//   keys   a thread per key: the vertex row through the (part, vid) index, part = (uint64)vid % nparts + 1; FETCH
//          on tags: one hit bit per ON tag from DTag::present; FETCH on an edge: a binary search of the source row's
//          adjacency for (rank, dst) under the stored order. keep = a hit, or keepMissing. The kept keys of each
//          256-key chunk are counted by ballot / popcount into chunkCount[chunk].
//   scan   launchScanU64 over the chunk counts: exclusive bases; the total sizes the output exactly.
//   emit   re-derives a key's place, base[chunk] + its rank among the chunk's kept keys (ballot / popcount), and
//          writes the row's cells there, so rows keep the order of the keys. Run twice when a yield is a string:
//          first with lenOut to write each output row's string bytes (scanned into strPre), then for the cells.
constexpr int kFetchMaxTags = 8;
constexpr int kFetchMaxCols = 16;
constexpr uint32_t kFetchGridMax = 2048;            // workgroups (of 256 keys a sweep) of the key and emit kernels
constexpr uint64_t kFetchNoEdge = ~0ULL;
enum { kFyTagProp = 0, kFyEdgeProp, kFyKey, kFyEdgeType, kFyInput };
struct FetchYield {
    int32_t src;                        // kFy*
    int32_t a;                          // kFyTagProp: index into the ON tags; kFyKey: 0 vid / src, 1 dst, 2 rank
    int32_t cell;                       // NGX_CELL_* of the output cell
    int32_t pad;
    DCol col;                           // kFyTagProp / kFyEdgeProp: the stored column
    GroupCol in;                        // kFyInput: the input column (a string: device pointers and lengths)
    int64_t konst;                      // kFyEdgeType: the type
};
struct FetchArgs {
    uint64_t n;                         // keys
    int32_t edge;                       // 0: FETCH on tags, 1: on an edge type
    int32_t nparts;
    GroupCol key[3];                    // vid | src, dst, rank (hasRank 0: rank 0)
    int32_t hasRank;
    int32_t ntags;
    VIndex vindex;
    const uint8_t* present[kFetchMaxTags];
    DSlot slot;                         // edge: the type's out-slot
    int32_t keepMissing;                // a key without data keeps its row (the yields read the input)
    int32_t ny;
    const FetchYield* ys;               // device array
    uint32_t* row;                      // per key: the vertex row (kNoRow: none)
    uint64_t* eidx;                     // edge: per key the edge's index in the slot (kFetchNoEdge: none)
    uint16_t* hits;                     // per key: bit t = the vertex has a row of ON tag t; edge: bit 0 = found; bit 15 = keep
    uint64_t* chunkCount;               // per 256-key chunk: kept keys
    const uint64_t* chunkBase;          // exclusive scan of chunkCount (emit)
    uint32_t* seen;                     // one word: OR of every key's tag hit bits
    uint64_t* lenOut;                   // emit, length pass: per output row its string bytes; null: the cell pass
    const uint64_t* strPre;             // cell pass: exclusive scan of the lengths; null: no string yields
    char* strOut;
    GroupCell* cells;                   // m * (nkey + ny): nkey = 1 (VertexID) or 3 (src, dst, rank)
    uint32_t gridMax;                   // most workgroups of a sweep (flag fetch_grid_max); 0: kFetchGridMax
};
int launchFetchKeys(const FetchArgs& a, hipStream_t s);
int launchFetchEmit(const FetchArgs& a, hipStream_t s);

// LOOKUP ON a tag / an edge type as a column scan in HBM (lookup.hip; ngx_lookup). Three steps, every one a sweep
// of 256 rows a workgroup and turn, so rows keep storage order under every grid size:
//   keep   a thread per row of the tag table (present[row] set) or per edge of the type's out-slot: the scanned
//          fields encoded to their index key and compared with [lo, hi) (lo == hi: equality, the reference's prefix
//          scan), BOOL / STRING fields compared typed, then the residual terms. keep[row] and the kept rows of each
//          256-row chunk (ballot / popcount) are written.
//   scan   launchScanU64 over the chunk counts: exclusive bases; the total sizes the output exactly.
//   emit   VertexID | SrcVID, DstVID, Ranking and the YIELD columns of the kept rows at base[chunk] + rank in chunk;
//          an edge's source row is the last row with off[row] <= e. Run twice when a yield is a string (lengths,
//          then cells), as FETCH's emit.
constexpr int kLookupMax = 16;                      // scanned fields, residual terms, YIELD columns: each at most
constexpr uint32_t kLookupGridMax = 2048;
enum { kLkInt = 0, kLkDouble, kLkBool, kLkString };                 // how a column is stored / what a constant is
enum { kLkLT = 0, kLkLE, kLkGT, kLkGE, kLkEQ, kLkNE };              // RelationalExpression::Operator
struct LookupCond {
    DCol col;
    int32_t kind;                       // kLk* of the column
    int32_t ckind;                      // term: kLk* of the constant
    int32_t op;                         // term: kLk?? operator (column op constant)
    int32_t slen;                       // string constant: its length
    uint64_t lo, hi;                    // scanned INT / DOUBLE field: key range; BOOL field: lo = the constant;
                                        // term: lo = the constant's bits (int64 / double / 0, 1)
    uint64_t soff;                      // string constant: its offset in pool
};
struct LookupYield {
    DCol col;
    int32_t cell;                       // NGX_CELL_* of the output cell
    int32_t pad;
};
struct LookupArgs {
    uint64_t n;                         // rows scanned: V (tag) or the slot's edges
    uint64_t V;
    int32_t edge;
    int32_t nf, nt, ny;
    const uint8_t* present;             // tag: DTag::present
    const int64_t* vid;                 // the vertex table's vids
    DSlot slot;                         // edge: the type's out-slot
    const LookupCond* conds;            // device array: nf scanned fields, then nt residual terms
    const char* pool;                   // string constants
    const LookupYield* ys;              // device array
    uint8_t* keep;                      // per row
    uint64_t* chunkCount;               // per 256-row chunk: kept rows
    const uint64_t* chunkBase;          // exclusive scan of chunkCount (emit)
    uint64_t* lenOut;                   // emit, length pass: per output row its string bytes; null: the cell pass
    const uint64_t* strPre;             // cell pass: exclusive scan of the lengths; null: no string yields
    char* strOut;
    GroupCell* cells;                   // m * (nkey + ny): nkey = 1 (VertexID) or 3 (SrcVID, DstVID, Ranking)
    uint32_t gridMax;                   // most workgroups of a sweep (flag lookup_grid_max); 0: kLookupGridMax
};
int launchLookupKeep(const LookupArgs& a, hipStream_t s);
int launchLookupEmit(const LookupArgs& a, hipStream_t s);

// `| YIELD <columns> [WHERE <expr>]` over a device-resident result (yield.hip; ngx_go_yield). Every kernel sweeps
// 256 rows a workgroup and turn, so rows keep their order under every grid size:
//   keep   a thread per row evaluates WHERE (vmEval<true>); the wave's ballot is one word of the keep bitmap (a word
//          per 64 rows), the popcounts of a 256-row chunk its count. No WHERE: not launched, keepBits is null and
//          every row is kept.
//   emit   (projection) a kept row's output index is base[chunk] + the kept rows before it in the chunk
//          (launchScanU64 over the chunk counts); a yield is a column copied at its stored width or a program's value.
//          Run twice when a yield is a STRING column (lengths, then cells), as LOOKUP's emit.
//   agg    (aggregates) per kept row every yield's value goes into its state words: reduced across the wave's lanes,
//          across the workgroup's waves in LDS, then one 64-bit atomic per workgroup and word.
//   probe  one thread evaluates every program on one row: the first input row types the columns, the last kept
//          row gives a function-less expression its value.
// An evaluation that fails sets err[0] bit 0, a value of another type than the first row's bit 1; err[1] is the
// VM's host-only mark (VmEnv::unsupported).
constexpr int kYieldMax = 64;                       // yield columns
constexpr uint32_t kYieldGridMax = 1024;
enum { kYieldCol = 0, kYieldEval, kYieldNone };     // a column's copy, a program's value, not evaluated (COUNT of a constant)
enum { kYieldSrcOne = 0, kYieldSrcValue, kYieldSrcOrdered, kYieldSrcRow };   // 1, the value, its order key (double), row + 1
struct YieldItem {
    int32_t mode;                       // kYield*
    int32_t a;                          // kYieldCol: the column; kYieldEval: the program's first Insn in code
    int32_t cell;                       // projection: NGX_CELL_* of the output cell
    int32_t vt;                         // kYieldEval: the V_* every kept row's value has
    uint64_t poolOff;                   // kYieldEval: the program's constant strings in pool
};
struct YieldSlot {
    int32_t op;                         // kGroup* (groupby.hip's state operators)
    int32_t src;                        // kYieldSrc*
    int32_t y;                          // the yield whose value it takes
    int32_t pad;
};
struct YieldProbe {
    int64_t x;
    uint32_t len;
    uint32_t vt;                        // V_*; V_ERR: the evaluation failed
};
struct YieldArgs {
    uint64_t n;
    const DResultCol* cols;             // device array: every column of the result
    const Insn* code;                   // the programs, each ending in OP_END
    const char* pool;
    int32_t whereOff;                   // keep: WHERE's first Insn
    int32_t ny, nslots;
    uint64_t wherePool;
    const YieldItem* items;             // device arrays
    const YieldSlot* slots;             // ordered by y
    uint64_t* keepBits;                 // a word per 64 rows; null: every row kept
    uint64_t* chunkCount;               // keep: kept rows per 256-row chunk
    const uint64_t* chunkBase;          // emit with keepBits: exclusive scan of chunkCount
    uint64_t* lenOut;                   // emit, length pass: per output row its string bytes; null: the cell pass
    const uint64_t* strPre;             // cell pass: exclusive scan of the lengths; null: no string yields
    char* strOut;
    GroupCell* cells;                   // m * ny
    uint64_t* state;                    // agg: nslots words, initialised by the launcher
    uint32_t* err;                      // two words, zeroed by the caller
    uint32_t gridMax;                   // most workgroups of a sweep (flag yield_grid_max); 0: kYieldGridMax
};
int launchYieldKeep(const YieldArgs& a, hipStream_t s);
int launchYieldEmit(const YieldArgs& a, hipStream_t s);
int launchYieldAgg(const YieldArgs& a, hipStream_t s);
int launchYieldProbe(const YieldArgs& a, uint64_t row, YieldProbe* out, hipStream_t s);

// Batched device -> host copy by a kernel: every array is streamed with 16-byte loads and stores into
// page-locked host memory mapped into the device address space (dst = hipHostGetDevicePointer), so
// the copy runs at the PCIe write rate on all CUs instead of on one DMA engine.
constexpr int kMaxCopies = 32;
struct CopyBatch {
    int32_t n;
    const uint8_t* src[kMaxCopies];
    uint8_t* dst[kMaxCopies];
    uint64_t bytes[kMaxCopies];
    uint64_t start[kMaxCopies + 1];     // exclusive prefix of 16-byte units per array
};
int launchCopyBatch(const CopyBatch& b, hipStream_t s);
int launchVertexCells(const VertexCellArgs& a, hipStream_t s);
// frontier exchange, one launch each side: pack every peer q's marked rows into bits + q * words;
// merge ORs the world - 1 received bitmaps (bits + q * words, over this shard's rows) into the marks
constexpr int kXchgBlock = 256;                      // k_pack / k_merge: rows per workgroup (four ballot words)
struct ExchangeArgs {
    uint8_t* visited;
    uint8_t epoch;
    uint64_t sb[kMaxWorld + 1];                      // shard q's rows are [sb[q], sb[q + 1])
    int world, rank;
    uint64_t words;                                  // bitmap stride per peer
    uint64_t* bits;
};
int launchPackPeers(const ExchangeArgs& a, hipStream_t s);
int launchMergePeers(const ExchangeArgs& a, hipStream_t s);
// The list form of the same exchange, for hops whose frontier is far smaller than the peers' rows
// (counts, then the vids): per peer q != rank the marked rows of q's range as u32 offsets
// from sb[q], appended to list[q * cap ..] (one atomic per workgroup and peer; counts[q] zeroed by the
// host first), then each owner marks the rows it received (k_merge_list).
constexpr int kListThreads = 1024;                   // k_pack_list: threads per workgroup
constexpr int kListTile = 4096;                      // k_pack_list: rows per workgroup (kListThreads x 4)
constexpr int kXchgListFactor = 32;                  // lists when kXchgListFactor * (largest shard's E) < smallest shard's rows
struct ListXchgArgs {
    const uint8_t* visited;
    uint8_t epoch;
    uint64_t sb[kMaxWorld + 1];
    int world, rank;
    uint32_t* list;
    uint64_t cap;                                    // entries per peer in `list`
    unsigned long long* counts;                      // world words
    int includeSelf;                                 // also list this rank's own rows (the $$ owner fetch)
};
int launchPackLists(const ListXchgArgs& a, hipStream_t s);
// map[rows[i]] = i for i < n (the $$ owner fetch: global row -> index of its fetched tag values)
int launchScatterIndex(const uint32_t* rows, uint64_t n, uint32_t* map, hipStream_t s);
// own[rows[i]] = epoch for i < n
int launchMergeList(const uint32_t* rows, uint64_t n, uint8_t* own, uint8_t epoch, hipStream_t s);


}  // namespace ngx
