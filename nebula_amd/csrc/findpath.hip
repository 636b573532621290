// FIND SHORTEST PATH in HBM (ngx_find_path; FindPathExecutor, src/graph/FindPathExecutor.cpp, which extends every
// kept walk by every neighbour on graphd, from both ends).
//
// For SHORTEST the result is, per target t, every path of L_t = min_s d(s, t) edges from a source at that distance
// (DESIGN §7.8), so breadth-first levels replace the walks:
//   expand   a wave per (level row, slot), lanes striding over its edges: inc[dst] |= the row's bits (atomicOr);
//            the lane whose OR found inc[dst] == 0 lists dst once (one atomicAdd per wave and 64 edges, by ballot)
//   settle   after that launch, so every OR is complete: per listed row new = inc & ~seen, seen |= new, inc = 0;
//            new != 0 puts (row, new) into the next level. On the to side bit j is target j, so a (vertex, target)
//            pair enters exactly one level, its distance; on the from side the one bit makes plain BFS levels.
//   meet     odd (2k - 1 edges): an edge from a row of the from side's level k - 1 into a row of the to side's level
//            k - 1 (k_path_sweep<true>); even (2k): a row in both sides' level k (k_path_meet_even). Only targets not
//            found before count; their bits start the keep masks of the meeting rows.
//   sweep    back from a meet, level by level and side by side (k_path_sweep<false>): an edge of a level-j row into a
//            row whose keep mask at level j + 1 shares bits with the row's own level bits is an edge of the path DAG
//            for those bits, and they join the row's keep mask. Edges collect in LDS and leave a buffer at a time:
//            one atomicAdd reserves the buffer's place in the output (as k_order_collect / k_set_probe).
// Every hand-off between these steps is a kernel boundary on one stream.
//
// FIND ALL / NOLOOP PATH (flag find_path_all) return every walk of 1 .. UPTO edges from a source to a target, NOLOOP
// those without a repeated vertex, so the answer is a layered edge set and not walks:
//   to side  seed / expand / settle from the targets, to depth UPTO - 1; after depth d the seen words are copied to
//            cum[d]: the targets within d edges of each row
//   walk     one launch per layer i of the from side (k_path_walk), layer 0 being the source rows: an edge into row r
//            with m = cum[UPTO - 1 - i][r] != 0 is the i-th step of a walk that can still arrive, and is emitted with
//            (i, m); r joins layer i + 1 once (a per-row stamp raised by atomicMax), whatever layers it was in before
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

// the index of this lane's entry in a list that `counter` counts: one atomicAdd per wave for its `want` lanes.
// Called by every active lane of the wave together.
__device__ __forceinline__ uint64_t waveAppend(bool want, unsigned long long* counter) {
    const unsigned long long b = __ballot(want);
    if (b == 0) return 0;
    const int lane = threadIdx.x & 63;
    const int lead = __ffsll(b) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(counter, static_cast<unsigned long long>(__popcll(b)));
    base = __shfl(base, lead);
    return base + static_cast<uint64_t>(__popcll(b & ((1ULL << lane) - 1)));
}

__device__ __forceinline__ uint64_t waveOr(uint64_t x) {
    for (int o = 32; o; o >>= 1) x |= __shfl_xor(static_cast<unsigned long long>(x), o);
    return x;
}

__device__ __forceinline__ int64_t pathRank(const HopSlots& hs, int s, uint64_t p) {
    const void* r = hs.rank[s];
    if (!r) return hs.rankC[s];
    switch (hs.rankW[s]) {
        case 1: return static_cast<const int8_t*>(r)[p];
        case 2: return static_cast<const int16_t*>(r)[p];
        case 4: return static_cast<const int32_t*>(r)[p];
        default: return static_cast<const int64_t*>(r)[p];
    }
}

__global__ __launch_bounds__(256) void k_path_seed(const uint32_t* rowsIn, uint64_t n, int perEntry, uint64_t* seen, uint64_t* newD,
                                                   uint8_t* lvl, uint32_t* outRows, uint64_t* outMask, unsigned long long* count) {
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256; i0 < n; i0 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t g = i < n ? rowsIn[i] : kNoRow;
        const bool keep = g != kNoRow;
        const uint64_t m = perEntry ? 1ULL << (i & 63) : 1ULL;
        const uint64_t idx = waveAppend(keep, count);
        if (keep) {                                               // distinct vids: distinct rows, one writer each
            if (seen) seen[g] = m;
            if (newD) newD[g] = m;
            if (lvl) lvl[g] = 0;
            outRows[idx] = g;
            if (outMask) outMask[idx] = m;
        }
    }
}

__global__ __launch_bounds__(256) void k_path_expand(const uint32_t* rows, const uint64_t* masks, uint64_t n, HopSlots hs,
                                                     unsigned long long* inc, uint32_t* touched, uint64_t cap,
                                                     unsigned long long* nTouched, uint32_t* err) {
    const int lane = threadIdx.x & 63;
    const uint64_t nEnt = n * static_cast<uint64_t>(hs.n);
    const uint64_t nw = static_cast<uint64_t>(gridDim.x) * 4;
    for (uint64_t w = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6; w < nEnt; w += nw) {
        const uint64_t i = w / hs.n;
        const int s = static_cast<int>(w % hs.n);
        const uint32_t row = rows[i];
        const unsigned long long m = masks ? masks[i] : 1ULL;
        const uint64_t b = hs.off[s][row], e = hs.off[s][row + 1];
        for (uint64_t p0 = b; p0 < e; p0 += 64) {                 // uniform in the wave
            const uint64_t p = p0 + lane;
            uint32_t g = kNoRow;
            bool first = false;
            if (p < e) {
                g = hs.dgid[s][p];
                if (g != kNoRow) first = atomicOr(inc + g, m) == 0;
            }
            const uint64_t idx = waveAppend(first, nTouched);
            if (first) {
                if (idx < cap) touched[idx] = g;
                else *err = 1;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_path_settle(const uint32_t* touched, uint64_t n, uint64_t* inc, uint64_t* seen, uint64_t* newD,
                                                     uint8_t* lvl, uint8_t level, uint32_t* outRows, uint64_t* outMask,
                                                     unsigned long long* count) {
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256; i0 < n; i0 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t g = kNoRow;
        uint64_t nw = 0;
        if (i < n) {                                              // a row is listed once: this thread owns it
            g = touched[i];
            const uint64_t in = inc[g];
            inc[g] = 0;
            nw = in & ~seen[g];
            if (nw) {
                seen[g] |= nw;
                if (newD) newD[g] = nw;
                lvl[g] = level;
            }
        }
        const uint64_t idx = waveAppend(nw != 0, count);          // at most n entries: the lists hold n
        if (nw) {
            outRows[idx] = g;
            outMask[idx] = nw;
        }
    }
}

__global__ __launch_bounds__(256) void k_path_meet_even(const uint32_t* rowsT, const uint64_t* masksT, const uint8_t* fLvl, uint8_t level,
                                                        uint64_t foundPrev, uint64_t* keepF, uint64_t* keepT, PathState* S) {
    const uint64_t n = S->nLevel[1];                              // written by the settle launch before this one
    const uint64_t had = foundPrev | S->found[0];                 // ... and by the odd meet before that
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256; i0 < n; i0 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t mm = 0;
        if (i < n) {
            const uint32_t v = rowsT[i];
            if (fLvl[v] == level) mm = masksT[i] & ~had;
            if (mm) {                                             // a row is once in a level's list
                keepF[v] = mm;
                keepT[v] = mm;
            }
        }
        const uint64_t all = waveOr(mm);
        if ((threadIdx.x & 63) == 0 && all) atomicOr(reinterpret_cast<unsigned long long*>(&S->found[1]), static_cast<unsigned long long>(all));
    }
}

template <bool MEET>
__global__ __launch_bounds__(256) void k_path_sweep(PathSweepArgs a) {
    __shared__ PathEdge buf[kPathBuf];
    __shared__ uint32_t cnt;
    __shared__ uint64_t base;
    __shared__ uint32_t trips[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* fill = reinterpret_cast<unsigned long long*>(&a.S->edges);
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    auto flush = [&](uint32_t have) {                             // called by the whole workgroup, after a barrier
        if (threadIdx.x == 0) base = atomicAdd(fill, static_cast<unsigned long long>(have));
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < have; j += 256) {
            const uint64_t o = base + j;
            if (o < a.cap) a.out[o] = buf[j];                     // past the capacity only the count goes on: the host refuses
        }
        __syncthreads();
        if (threadIdx.x == 0) cnt = 0;
        __syncthreads();
    };
    const uint64_t nEnt = a.n * static_cast<uint64_t>(a.hs.n);
    for (uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * 4; e0 < nEnt; e0 += static_cast<uint64_t>(gridDim.x) * 4) {   // uniform in the workgroup
        const uint64_t w = e0 + wave;
        uint32_t row = 0;
        int s = 0;
        uint64_t own = ~0ULL, b = 0, e = 0;
        if (w < nEnt) {
            const uint64_t i = w / a.hs.n;
            s = static_cast<int>(w % a.hs.n);
            row = a.rows[i];
            if (a.masks) own = a.masks[i];
            b = a.hs.off[s][row];
            e = a.hs.off[s][row + 1];
        }
        if (lane == 0) trips[wave] = static_cast<uint32_t>((e - b + 63) / 64);
        __syncthreads();
        const uint32_t T = max(max(trips[0], trips[1]), max(trips[2], trips[3]));
        uint64_t acc = 0;
        for (uint32_t it = 0; it < T; it++) {                     // uniform in the workgroup: the barriers below
            const uint64_t p = b + static_cast<uint64_t>(it) * 64 + lane;
            uint64_t m = 0;
            uint32_t g = kNoRow;
            if (p < e) {
                g = a.hs.dgid[s][p];
                if (g != kNoRow) {
                    if (MEET) m = (a.tLvl[g] == a.level ? a.tNew[g] : 0) & a.notFound;
                    else m = a.keepCur[g] & own;
                }
            }
            if (m) {
                if (MEET) atomicOr(reinterpret_cast<unsigned long long*>(a.keepT + g), static_cast<unsigned long long>(m));
                acc |= m;
                PathEdge pe;
                pe.src = a.vid[a.reverse ? g : row];
                pe.dst = a.vid[a.reverse ? row : g];
                pe.rank = pathRank(a.hs, s, p);
                pe.mask = m;
                pe.type = a.reverse ? -a.hs.etype[s] : a.hs.etype[s];
                pe.layer = 0;
                buf[atomicAdd(&cnt, 1u)] = pe;                    // cnt <= kPathBuf - 256 before the adds
            }
            __syncthreads();
            const uint32_t have = cnt;
            __syncthreads();                                      // everyone has read cnt before the next adds
            if (have > kPathBuf - 256) {
                flush(have);
                if (threadIdx.x == 0) atomicAdd(&a.S->loopFlushes, 1u);
            }
        }
        acc = waveOr(acc);
        if (lane == 0 && acc) {                                   // a row's slots are several waves: OR
            atomicOr(reinterpret_cast<unsigned long long*>(a.keepNext + row), static_cast<unsigned long long>(acc));
            if (MEET) atomicOr(reinterpret_cast<unsigned long long*>(&a.S->found[0]), static_cast<unsigned long long>(acc));
        }
        __syncthreads();                                          // trips[] is read before the next round writes it
    }
    __syncthreads();
    const uint32_t have = cnt;
    if (have) flush(have);
}

// FIND ALL / NOLOOP PATH, one layer of the from side: k_path_sweep's loop, LDS buffer and flush with another
// test per edge. Nothing a lane reads here is written by this launch but stamp[], and that only through its atomicMax.
__global__ __launch_bounds__(256) void k_path_walk(PathWalkArgs a) {
    __shared__ PathEdge buf[kPathBuf];
    __shared__ uint32_t cnt;
    __shared__ uint64_t base;
    __shared__ uint32_t trips[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* fill = reinterpret_cast<unsigned long long*>(&a.S->edges);
    unsigned long long* listed = reinterpret_cast<unsigned long long*>(&a.S->touched[0]);
    const uint32_t mark = static_cast<uint32_t>(a.layer) + 2;     // stamp[r] = 2 + the last layer that listed r; 0: none
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    auto flush = [&](uint32_t have) {                             // called by the whole workgroup, after a barrier
        if (threadIdx.x == 0) base = atomicAdd(fill, static_cast<unsigned long long>(have));
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < have; j += 256) {
            const uint64_t o = base + j;
            if (o < a.cap) a.out[o] = buf[j];                     // past the capacity only the count goes on: the host refuses
        }
        __syncthreads();
        if (threadIdx.x == 0) cnt = 0;
        __syncthreads();
    };
    const uint64_t nEnt = a.n * static_cast<uint64_t>(a.hs.n);
    for (uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * 4; e0 < nEnt; e0 += static_cast<uint64_t>(gridDim.x) * 4) {   // uniform in the workgroup
        const uint64_t w = e0 + wave;
        uint32_t row = 0;
        int s = 0;
        uint64_t b = 0, e = 0;
        if (w < nEnt) {
            s = static_cast<int>(w % a.hs.n);
            row = a.rows[w / a.hs.n];
            b = a.hs.off[s][row];
            e = a.hs.off[s][row + 1];
        }
        if (lane == 0) trips[wave] = static_cast<uint32_t>((e - b + 63) / 64);
        __syncthreads();
        const uint32_t T = max(max(trips[0], trips[1]), max(trips[2], trips[3]));
        for (uint32_t it = 0; it < T; it++) {                     // uniform in the workgroup: the barriers below
            const uint64_t p = b + static_cast<uint64_t>(it) * 64 + lane;
            uint64_t m = 0;
            uint32_t g = kNoRow;
            if (p < e) {
                g = a.hs.dgid[s][p];
                if (g != kNoRow) m = a.cum[g];
            }
            bool list = false;
            if (m) {
                PathEdge pe;
                pe.src = a.vid[row];
                pe.dst = a.vid[g];
                pe.rank = pathRank(a.hs, s, p);
                pe.mask = m;
                pe.type = a.hs.etype[s];
                pe.layer = a.layer;
                buf[atomicAdd(&cnt, 1u)] = pe;                    // cnt <= kPathBuf - 256 before the adds
                if (a.next) list = atomicMax(a.stamp + g, mark) < mark;   // a row may be in many layers, once in each
            }
            const uint64_t idx = waveAppend(list, listed);        // every lane of the wave is here: T is uniform
            if (list) {
                if (idx < a.nextCap) a.next[idx] = g;
                else a.S->err = 1;
            }
            __syncthreads();
            const uint32_t have = cnt;
            __syncthreads();                                      // everyone has read cnt before the next adds
            if (have > kPathBuf - 256) {
                flush(have);
                if (threadIdx.x == 0) atomicAdd(&a.S->loopFlushes, 1u);
            }
        }
        __syncthreads();                                          // trips[] is read before the next round writes it
    }
    __syncthreads();
    const uint32_t have = cnt;
    if (have) flush(have);
}

__global__ __launch_bounds__(256) void k_path_clear(const uint32_t* rows, uint64_t n, uint64_t* arr) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * 256) arr[rows[i]] = 0;
}

unsigned pathGrid(uint64_t items, uint64_t perBlock, uint32_t gridMax = 0) {
    return static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>((items + perBlock - 1) / perBlock, gridMax ? gridMax : kPathGridMax)));
}

}  // namespace

int launchPathSeed(const uint32_t* rowsIn, uint64_t n, int perEntry, uint64_t* seen, uint64_t* newD, uint8_t* lvl, uint32_t* outRows,
                   uint64_t* outMask, uint64_t* count, hipStream_t s) {
    if (!rowsIn || !outRows || !count || (perEntry && n > 64)) return 1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_path_seed, dim3(pathGrid(n, 256)), dim3(256), 0, s, rowsIn, n, perEntry, seen, newD, lvl, outRows, outMask,
                       reinterpret_cast<unsigned long long*>(count));
    return static_cast<int>(hipGetLastError());
}

int launchPathExpand(const uint32_t* rows, const uint64_t* masks, uint64_t n, const HopSlots& hs, uint64_t* inc, uint32_t* touched,
                     uint64_t cap, PathState* S, int side, hipStream_t s) {
    if (!rows || !inc || !touched || !S || (side != 0 && side != 1)) return 1;
    if (n == 0 || hs.n == 0) return 0;
    hipLaunchKernelGGL(k_path_expand, dim3(pathGrid(n * hs.n, 4)), dim3(256), 0, s, rows, masks, n, hs,
                       reinterpret_cast<unsigned long long*>(inc), touched, cap, reinterpret_cast<unsigned long long*>(&S->touched[side]),
                       &S->err);
    return static_cast<int>(hipGetLastError());
}

int launchPathSettle(const uint32_t* touched, uint64_t n, uint64_t* inc, uint64_t* seen, uint64_t* newD, uint8_t* lvl, uint8_t level,
                     uint32_t* outRows, uint64_t* outMask, PathState* S, int side, hipStream_t s) {
    if (!touched || !inc || !seen || !lvl || !outRows || !outMask || !S || (side != 0 && side != 1)) return 1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_path_settle, dim3(pathGrid(n, 256)), dim3(256), 0, s, touched, n, inc, seen, newD, lvl, level, outRows, outMask,
                       reinterpret_cast<unsigned long long*>(&S->nLevel[side]));
    return static_cast<int>(hipGetLastError());
}

int launchPathMeetEven(const uint32_t* rowsT, const uint64_t* masksT, uint64_t nMax, const uint8_t* fLvl, uint8_t level, uint64_t foundPrev,
                       uint64_t* keepF, uint64_t* keepT, PathState* S, hipStream_t s) {
    if (!rowsT || !masksT || !fLvl || !keepF || !keepT || !S) return 1;
    if (nMax == 0) return 0;
    hipLaunchKernelGGL(k_path_meet_even, dim3(pathGrid(nMax, 256)), dim3(256), 0, s, rowsT, masksT, fLvl, level, foundPrev, keepF, keepT, S);
    return static_cast<int>(hipGetLastError());
}

int launchPathSweep(const PathSweepArgs& a, bool meet, hipStream_t s) {
    if (!a.rows || !a.vid || !a.keepNext || !a.out || !a.S) return 1;
    if (meet ? (!a.tLvl || !a.tNew || !a.keepT) : !a.keepCur) return 1;
    if (a.n == 0 || a.hs.n == 0) return 0;
    const dim3 grid(pathGrid(a.n * a.hs.n, 4, a.gridMax));
    if (meet) hipLaunchKernelGGL(k_path_sweep<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_path_sweep<false>, grid, dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchPathWalk(const PathWalkArgs& a, hipStream_t s) {
    if (!a.rows || !a.vid || !a.cum || !a.stamp || !a.out || !a.S || a.layer < 0) return 1;
    if (a.n == 0 || a.hs.n == 0) return 0;
    hipLaunchKernelGGL(k_path_walk, dim3(pathGrid(a.n * a.hs.n, 4, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchPathClear(const uint32_t* rows, uint64_t n, uint64_t* arr, hipStream_t s) {
    if (!rows || !arr) return 1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_path_clear, dim3(pathGrid(n, 256)), dim3(256), 0, s, rows, n, arr);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
