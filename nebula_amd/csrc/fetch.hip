// FETCH PROP ON tags / an edge type over keys in HBM (ngx_fetch; FetchVerticesExecutor / FetchEdgesExecutor with
// QueryVertexPropsProcessor / QueryEdgePropsProcessor behind them). kernels.h FetchArgs states the three steps.
//
// The edge lookup searches a source row's adjacency [off[row], off[row + 1]) for (rank, dst). An adjacency is
// stored in the KV store's bytewise key order (exporter.cpp: ranks and dsts are little-endian in the key, so the
// order is the unsigned order of bswap64(rank), then of bswap64(dst)), not in numeric order, and its columns are
// narrowed to 1 / 2 / 4 / 8 bytes or hold one constant rank. Both sides of every comparison are therefore the
// full 64-bit values (stored ones sign-extended on load): a key outside a narrowed column's range compares unequal
// to every stored value and misses, it never wraps into a hit.
//
// These are dependent-load chains (index probe -> present bytes / offsets -> log2(degree) probes -> column
// values), not streams: a thread owns a key, 256 keys a workgroup, and nothing is staged in LDS but the four wave
// counts a chunk's ranks need.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

constexpr int32_t kCellInt = 2, kCellStr = 6;

// value bits of row r, integers sign-extended from the stored width; width 0: the column's constant
__device__ __forceinline__ int64_t fRead(const GroupCol& c, uint64_t r) {
    switch (c.w) {
        case 0: return c.konst;
        case 1: return static_cast<const int8_t*>(c.x)[r];
        case 2: return static_cast<const int16_t*>(c.x)[r];
        case 4: return static_cast<const int32_t*>(c.x)[r];
        default: return static_cast<const int64_t*>(c.x)[r];
    }
}
__device__ __forceinline__ int64_t fLoadW(const void* p, int32_t w, uint64_t i) {
    switch (w) {
        case 1: return static_cast<const int8_t*>(p)[i];
        case 2: return static_cast<const int16_t*>(p)[i];
        case 4: return static_cast<const int32_t*>(p)[i];
        default: return static_cast<const int64_t*>(p)[i];
    }
}

__device__ __forceinline__ uint64_t fOrd(int64_t v) { return __builtin_bswap64(static_cast<uint64_t>(v)); }

// the index of edge (rank, dst) in [lo, hi) of the slot, kFetchNoEdge if it is not there
__device__ uint64_t fFindEdge(const DSlot& sl, uint64_t lo, uint64_t hi, int64_t rank, int64_t dst) {
    const uint64_t kr = fOrd(rank), kd = fOrd(dst);
    const uint64_t end = hi;
    while (lo < hi) {                                             // lower bound of (kr, kd)
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const int64_t r = sl.rank ? fLoadW(sl.rank, sl.rankW, mid) : sl.rankConst;
        const int64_t d = fLoadW(sl.dst, sl.dstW, mid);
        const uint64_t er = fOrd(r), ed = fOrd(d);
        const bool less = er < kr || (er == kr && ed < kd);
        if (less) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= end) return kFetchNoEdge;
    const int64_t r = sl.rank ? fLoadW(sl.rank, sl.rankW, lo) : sl.rankConst;
    const int64_t d = fLoadW(sl.dst, sl.dstW, lo);
    return r == rank && d == dst ? lo : kFetchNoEdge;
}

__global__ __launch_bounds__(256) void k_fetch_keys(FetchArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    uint32_t seen = 0;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        bool keep = false;
        if (i < a.n) {
            const int64_t vid = fRead(a.key[0], i);
            const int32_t part = static_cast<int32_t>(static_cast<uint64_t>(vid) % static_cast<uint64_t>(a.nparts)) + 1;
            const uint32_t row = a.vindex.slots ? vindexFind(a.vindex, part, vid) : kNoRow;
            uint32_t hits = 0;
            if (a.edge) {
                uint64_t e = kFetchNoEdge;
                if (row != kNoRow && a.slot.off) {
                    const int64_t dst = fRead(a.key[1], i);
                    const int64_t rank = a.hasRank ? fRead(a.key[2], i) : 0;
                    e = fFindEdge(a.slot, a.slot.off[row], a.slot.off[row + 1], rank, dst);
                }
                a.eidx[i] = e;
                hits = e != kFetchNoEdge ? 1u : 0u;
            } else if (row != kNoRow) {
                for (int t = 0; t < a.ntags; t++)
                    if (a.present[t] && a.present[t][row]) hits |= 1u << t;
            }
            keep = hits != 0 || a.keepMissing;
            a.row[i] = row;
            a.hits[i] = static_cast<uint16_t>(hits | (keep ? 0x8000u : 0u));
            seen |= hits;
        }
        const uint64_t kept = __ballot(keep);
        if (lane == 0) waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
        __syncthreads();
        if (threadIdx.x == 0) a.chunkCount[b0 >> 8] = static_cast<uint64_t>(waveCount[0]) + waveCount[1] + waveCount[2] + waveCount[3];
        __syncthreads();                                          // the counts are read before the next turn's writes
    }
    // one OR per wave that saw a tag, not one per key
    for (int off = 32; off; off >>= 1) seen |= __shfl_xor(seen, off);
    if (lane == 0 && seen) atomicOr(a.seen, seen);
}

__device__ __forceinline__ GroupCell fDefault(int32_t cell) {
    GroupCell c;
    c.kind = cell;
    c.len = 0;
    c.v = 0;                                                      // RowReader::getDefaultProp: 0, 0.0, false, ""
    return c;
}

// the stored column's value of row r as a cell; a string's bytes go to strOut + *soff (null: only counted)
__device__ GroupCell fColumn(const FetchYield& y, uint64_t r, char* strOut, uint64_t* soff) {
    GroupCell c = fDefault(y.cell);
    const DCol& col = y.col;
    if (col.valid && !col.valid[r]) return c;                     // the row's schema version lacks the field
    if (y.cell == kCellStr) {
        const uint64_t b = col.soff[r], e = col.soff[r + 1];
        const uint64_t len = e - b;
        if (strOut)
            for (uint64_t j = 0; j < len; j++) strOut[*soff + j] = col.sbytes[b + j];
        c.len = static_cast<int32_t>(len);
        c.v = static_cast<int64_t>(*soff);
        *soff += len;
    } else if (col.type == 4 || col.type == 5) {                  // FLOAT (widened at export) / DOUBLE
        c.v = static_cast<const int64_t*>(col.data)[r];
    } else if (col.type == 1) {                                   // BOOL
        c.v = static_cast<const uint8_t*>(col.data)[r] ? 1 : 0;
    } else {
        c.v = fLoadW(col.data, col.width, r);
    }
    return c;
}

__global__ __launch_bounds__(256) void k_fetch_emit(FetchArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkey = a.edge ? 3 : 1;
    const int ncols = nkey + a.ny;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        const uint32_t hits = i < a.n ? a.hits[i] : 0;
        const bool keep = (hits & 0x8000u) != 0;
        const uint64_t kept = __ballot(keep);
        if (lane == 0) waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
        __syncthreads();
        uint64_t o = a.chunkBase[b0 >> 8] + static_cast<uint64_t>(__popcll(kept & ((1ULL << lane) - 1)));
        for (uint32_t w = 0; w < wave; w++) o += waveCount[w];
        __syncthreads();
        if (!keep) continue;
        const uint32_t row = a.row[i];
        const uint64_t e = a.edge ? a.eidx[i] : 0;
        char* strOut = a.lenOut ? nullptr : a.strOut;
        uint64_t soff = a.lenOut || !a.strPre ? 0 : a.strPre[o];
        const uint64_t soff0 = soff;
        GroupCell* out = a.lenOut ? nullptr : a.cells + o * ncols;
        if (out) {
            for (int k = 0; k < nkey; k++) {
                GroupCell c;
                c.kind = k == 2 ? kCellInt : 3;                   // VertexID / _src / _dst: VID; _rank: INT
                c.len = 0;
                c.v = k == 2 && !a.hasRank ? 0 : fRead(a.key[k], i);
                out[k] = c;
            }
        }
        for (int y = 0; y < a.ny; y++) {
            const FetchYield& fy = a.ys[y];
            GroupCell c = fDefault(fy.cell);
            if (fy.src == kFyTagProp) {
                if (hits & (1u << fy.a)) c = fColumn(fy, row, strOut, &soff);
            } else if (fy.src == kFyEdgeProp) {
                if (e != kFetchNoEdge) c = fColumn(fy, e, strOut, &soff);
            } else if (fy.src == kFyKey) {
                c.v = fy.a == 2 && !a.hasRank ? 0 : fRead(a.key[fy.a], i);
            } else if (fy.src == kFyEdgeType) {
                c.v = fy.konst;
            } else {                                              // kFyInput: handed through, strings included
                const int64_t x = fRead(fy.in, i);
                if (fy.cell == kCellStr) {
                    const uint32_t len = fy.in.len ? fy.in.len[i] : 0;
                    const char* p = reinterpret_cast<const char*>(x);
                    if (strOut)
                        for (uint32_t j = 0; j < len; j++) strOut[soff + j] = p[j];
                    c.len = static_cast<int32_t>(len);
                    c.v = static_cast<int64_t>(soff);
                    soff += len;
                } else {
                    c.v = x;
                }
            }
            if (out) out[nkey + y] = c;
        }
        if (a.lenOut) a.lenOut[o] = soff - soff0;
    }
}

unsigned fetchGrid(uint64_t n, uint32_t gridMax) {
    return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, gridMax ? gridMax : kFetchGridMax));
}

bool fetchArgsOk(const FetchArgs& a) {
    if (a.n >= (1ULL << 31) || a.nparts < 1 || a.ntags < 0 || a.ntags > kFetchMaxTags || a.ny < 0 || a.ny > kFetchMaxCols) return false;
    if (!a.row || !a.hits || !a.chunkCount || !a.seen || (a.ny && !a.ys)) return false;
    if (a.edge && !a.eidx) return false;
    for (int k = 0; k < (a.edge ? (a.hasRank ? 3 : 2) : 1); k++) {
        const int32_t w = a.key[k].w;
        if ((w != 0 && w != 1 && w != 2 && w != 4 && w != 8) || (w && !a.key[k].x)) return false;
    }
    return true;
}

}  // namespace

int launchFetchKeys(const FetchArgs& a, hipStream_t s) {
    if (!fetchArgsOk(a)) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_fetch_keys, dim3(fetchGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchFetchEmit(const FetchArgs& a, hipStream_t s) {
    if (!fetchArgsOk(a) || !a.chunkBase || (!a.lenOut && !a.cells)) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_fetch_emit, dim3(fetchGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
