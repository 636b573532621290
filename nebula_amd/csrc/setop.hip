// UNION DISTINCT / INTERSECT / MINUS over two device-resident GO results (ngx_set_op; SetExecutor::doUnion +
// doDistinct, doIntersect, doMinus, src/graph/SetExecutor.cpp:200-410, whose INTERSECT and MINUS are nested
// loops over both row vectors).
//
// Two steps over both results' columns, read in place at their stored widths (kernels.h GroupCol, SetArgs):
//   build   every row of the build side (the right result; for UNION DISTINCT the left, then the right, one
//           launch each) goes into an open-addressing table (>= 2n slots, CAS on hash tag | row id + 1, as
//           k_group_assign) keyed on the whole row tuple: the row that claims a slot leads. For INTERSECT
//           count[slot] counts the rows equal to the leader, one atomic per row; a wave whose rows all met one
//           slot adds once (cdna_hip_programming.md Guideline 12: no chip-wide atomics into one hot address,
//           as k_order_count does for equal digits).
//   probe   every left row looks its tuple up. MINUS keeps the rows not found. INTERSECT takes a ticket,
//           atomicAdd(&taken[slot], 1) (a wave on one slot: one add for all its tickets), and keeps the row
//           iff the ticket is below count[slot]: a value occurring cL times left and cR times right comes out
//           min(cL, cR) times (doIntersect moves the matched right row out, so it matches once); equal rows
//           are equal in every column, so which of them win does not change the output. UNION DISTINCT runs
//           the probe over either side and keeps the leaders.
//           Kept row ids collect in LDS; a full buffer reserves its list space with one atomicAdd and is
//           copied out (as k_order_collect).
// A row with a NaN in a double column equals no row (ColumnValue == on doubles is plain ==), itself included:
// it is never inserted and never found; MINUS and UNION DISTINCT keep it, INTERSECT drops it.
// The host sorts the kept row ids per side and k_order_emit (orderby.hip) writes their cells.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

constexpr uint64_t kNoSlot = ~0ULL;

__device__ __forceinline__ uint64_t smix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// value bits of row r, integers sign-extended from the stored width; width 0: the column's constant
__device__ __forceinline__ int64_t sRead(const GroupCol& c, uint64_t r) {
    switch (c.w) {
        case 0: return c.konst;
        case 1: return static_cast<const int8_t*>(c.x)[r];
        case 2: return static_cast<const int16_t*>(c.x)[r];
        case 4: return static_cast<const int32_t*>(c.x)[r];
        default: return static_cast<const int64_t*>(c.x)[r];
    }
}
// doubles compare by value (ColumnValue ==): -0.0 == 0.0
__device__ __forceinline__ uint64_t sCanon(const GroupCol& c, int64_t x) {
    if (c.kind == kGroupDouble && __longlong_as_double(x) == 0.0) return 0;
    return static_cast<uint64_t>(x);
}

// the hash of row r's tuple (k_group_assign's, over every column); *nan: a double column holds a NaN
__device__ uint64_t sHash(const GroupCol* cols, int nc, uint64_t r, bool* nan) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    bool isNan = false;
    for (int k = 0; k < nc; k++) {
        const GroupCol c = cols[k];
        const int64_t x = sRead(c, r);
        if (c.kind == kGroupString) {
            const uint32_t len = c.len ? c.len[r] : 0;
            const char* p = reinterpret_cast<const char*>(x);
            uint64_t w = len;
            for (uint32_t i = 0; i < len; i++) w = (w ^ static_cast<uint8_t>(p[i])) * 0x100000001B3ULL;
            h = smix(h ^ w);
        } else {
            if (c.kind == kGroupDouble) {
                const double d = __longlong_as_double(x);
                isNan |= d != d;
            }
            h = smix(h ^ sCanon(c, x));
        }
    }
    *nan = isNan;
    return h;
}

// row r of columns ca against row o of columns cb (either side's; neither row holds a NaN)
__device__ bool sEqual(const GroupCol* ca, uint64_t r, const GroupCol* cb, uint64_t o, int nc) {
    for (int k = 0; k < nc; k++) {
        const GroupCol a = ca[k], b = cb[k];
        const int64_t x = sRead(a, r), y = sRead(b, o);
        if (a.kind == kGroupString) {
            const uint32_t l1 = a.len ? a.len[r] : 0, l2 = b.len ? b.len[o] : 0;
            if (l1 != l2) return false;
            const char* p1 = reinterpret_cast<const char*>(x);
            const char* p2 = reinterpret_cast<const char*>(y);
            for (uint32_t i = 0; i < l1; i++) if (p1[i] != p2[i]) return false;
        } else if (sCanon(a, x) != sCanon(b, y)) {
            return false;
        }
    }
    return true;
}

// the slot of row i of `side`'s tuple: inserted when INSERT and not there yet. kNoSlot: a NaN row, or
// (!INSERT) not in the table. *self: the slot holds this very row (it leads).
template <bool INSERT>
__device__ uint64_t sSlot(const SetArgs& a, uint32_t side, uint64_t i, bool* nanRow, bool* self) {
    const GroupCol* cols = a.cols[side];
    *self = false;
    const uint64_t h = sHash(cols, a.nc, i, nanRow);
    if (*nanRow) return kNoSlot;
    const uint64_t id = (side ? a.n[0] : 0) + i;
    const uint64_t tag = (h >> 32) << 32;
    const uint64_t mine = tag | (id + 1);
    uint64_t slot = h & a.mask;
    for (uint64_t probes = 0; probes <= a.mask; probes++) {
        // a slot is written once (0 -> tag | id + 1), so a non-zero load is final
        uint64_t cur = __hip_atomic_load(a.table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            if (!INSERT) return kNoSlot;
            cur = atomicCAS(reinterpret_cast<unsigned long long*>(a.table + slot), 0ULL, static_cast<unsigned long long>(mine));
            if (cur == 0) { *self = true; return slot; }
        }
        if ((cur >> 32) << 32 == tag) {
            const uint64_t o = (cur & 0xFFFFFFFFULL) - 1;
            if (o == id) { *self = true; return slot; }
            const bool right = o >= a.n[0];
            if (sEqual(cols, i, a.cols[right ? 1 : 0], right ? o - a.n[0] : o, a.nc)) return slot;
        }
        slot = (slot + 1) & a.mask;
    }
    if (INSERT) a.S->err = 1;                                     // no free slot in >= 2n: cannot be
    return kNoSlot;
}

__global__ __launch_bounds__(256) void k_set_build(SetArgs a, uint32_t side) {
    const uint64_t n = a.n[side];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < n; b0 += stride) {     // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        uint64_t slot = kNoSlot;
        if (i < n) {
            bool nanRow, self;
            slot = sSlot<true>(a, side, i, &nanRow, &self);
        }
        if (!a.count) continue;                                   // uniform: only INTERSECT counts
        const uint64_t active = __ballot(slot != kNoSlot);
        if (active) {
            const int lead = __ffsll(static_cast<unsigned long long>(active)) - 1;
            const uint64_t s0 = __shfl(static_cast<unsigned long long>(slot), lead);
            if (__ballot(slot != kNoSlot && slot != s0) == 0) {   // one slot in the wave: one add
                if (static_cast<int>(lane) == lead) atomicAdd(&a.count[s0], static_cast<uint32_t>(__popcll(active)));
            } else if (slot != kNoSlot) {
                atomicAdd(&a.count[slot], 1u);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_set_probe(SetArgs a, uint32_t side) {
    __shared__ uint32_t buf[kOrderAppendBuf];
    __shared__ uint32_t cnt;
    __shared__ uint64_t base;
    const uint64_t n = a.n[side];
    uint32_t* dst = a.keep[side];
    unsigned long long* fill = reinterpret_cast<unsigned long long*>(&a.S->fill[side]);
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    auto flush = [&](uint32_t have) {                             // called by the whole workgroup, after a barrier
        if (threadIdx.x == 0) base = atomicAdd(fill, static_cast<unsigned long long>(have));
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < have; j += 256) {
            const uint64_t o = base + j;
            if (o < n) dst[o] = buf[j];
            else a.S->err = 1;
        }
        __syncthreads();
        if (threadIdx.x == 0) cnt = 0;
        __syncthreads();
    };
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < n; b0 += stride) {     // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        uint64_t slot = kNoSlot;
        bool nanRow = false, self = false;
        if (i < n) slot = sSlot<false>(a, side, i, &nanRow, &self);
        bool keep = false;
        if (a.op == kSetMinus) {
            keep = i < n && slot == kNoSlot;
        } else if (a.op == kSetUnionDistinct) {
            keep = i < n && (nanRow || self);
        } else {                                                  // kSetIntersect: a ticket per found row
            const bool want = slot != kNoSlot;
            const uint64_t active = __ballot(want);
            uint32_t ticket = 0;
            if (active) {
                const int lead = __ffsll(static_cast<unsigned long long>(active)) - 1;
                const uint64_t s0 = __shfl(static_cast<unsigned long long>(slot), lead);
                if (__ballot(want && slot != s0) == 0) {          // one slot in the wave: one add hands out its tickets
                    uint32_t t0 = 0;
                    if (static_cast<int>(lane) == lead) t0 = atomicAdd(&a.taken[s0], static_cast<uint32_t>(__popcll(active)));
                    t0 = __shfl(t0, lead);
                    ticket = t0 + static_cast<uint32_t>(__popcll(active & ((1ULL << lane) - 1)));
                } else if (want) {
                    ticket = atomicAdd(&a.taken[slot], 1u);
                }
            }
            keep = want && ticket < a.count[slot];
        }
        if (keep) buf[atomicAdd(&cnt, 1u)] = static_cast<uint32_t>(i);        // cnt <= kOrderAppendBuf - 256 before the adds
        __syncthreads();
        const uint32_t have = cnt;
        __syncthreads();                                          // everyone has read cnt before the next adds
        if (have > kOrderAppendBuf - 256) {
            flush(have);
            if (threadIdx.x == 0) atomicAdd(&a.S->loopFlushes, 1u);
        }
    }
    __syncthreads();
    const uint32_t have = cnt;
    if (have) flush(have);
}

unsigned setGrid(uint64_t n, uint32_t gridMax) {
    return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, gridMax ? gridMax : kSetGridMax));
}

bool setArgsOk(const SetArgs& a, int side) {
    return (side == 0 || side == 1) && a.nc >= 1 && a.nc <= kSetMaxCols && a.n[0] + a.n[1] < 0xFFFFFFFFULL && a.table &&
           (a.mask & (a.mask + 1)) == 0 && a.cols[0] && a.cols[1] && a.S;
}

}  // namespace

int launchSetBuild(const SetArgs& a, int side, hipStream_t s) {
    if (!setArgsOk(a, side) || (a.op == kSetIntersect && (!a.count || !a.taken))) return 1;
    if (a.n[side] == 0) return 0;
    hipLaunchKernelGGL(k_set_build, dim3(setGrid(a.n[side], a.gridMax)), dim3(256), 0, s, a, static_cast<uint32_t>(side));
    return static_cast<int>(hipGetLastError());
}

int launchSetProbe(const SetArgs& a, int side, hipStream_t s) {
    if (!setArgsOk(a, side) || !a.keep[side] || (a.op == kSetIntersect && (!a.count || !a.taken))) return 1;
    if (a.n[side] == 0) return 0;
    hipLaunchKernelGGL(k_set_probe, dim3(setGrid(a.n[side], a.gridMax)), dim3(256), 0, s, a, static_cast<uint32_t>(side));
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
