// GROUP BY over a device-resident GO result (ngx_go_group_by; GroupByExecutor::groupingData,
// src/graph/GroupByExecutor.cpp:236-331, with the functions of src/graph/AggregateFunction.h).
//
// Three steps over the result's columns, read in place at their stored widths (kernels.h GroupCol):
//   assign      every row's key tuple goes into an open-addressing table (>= 2n slots, CAS on
//               hash tag | row + 1, as k_distinct_mark): the row that claims a slot leads its group, the
//               others learn their leader's row. An exclusive scan of the leader flags numbers the groups.
//               COUNT_DISTINCT runs the same pass keyed on (keys, value): its leaders are counted per group.
//   accumulate  per state word (count, int64 sum / and / or / xor / max / min, double sum) one atomic per
//               row. With few groups every workgroup first aggregates into an LDS copy of the state and
//               flushes it once (cdna_hip_programming.md Guideline 12: no chip-wide atomics into a few hot
//               addresses); with many groups the global 64-bit atomics are spread by group already.
//               Double MAX / MIN run as int64 MAX / MIN on an order-preserving key of the bits.
//   emit        one thread per leader writes its group's row of cells: keys from the leader row (string
//               bytes copied to the result's string block), finalised aggregates (AVG = (double)sum / count).
// Integer results are exact in any arrival order (wraparound +, &, |, ^, max, min are associative and
// commutative); double SUM / AVG depend on the order the atomics land in and are not bit-reproducible,
// like the reference's own sum over responses in arrival order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

__device__ __forceinline__ uint64_t gmix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// value bits of row r, integers sign-extended from the stored width; width 0: the column's constant
__device__ __forceinline__ int64_t gRead(const GroupCol& c, uint64_t r) {
    switch (c.w) {
        case 0: return c.konst;
        case 1: return static_cast<const int8_t*>(c.x)[r];
        case 2: return static_cast<const int16_t*>(c.x)[r];
        case 4: return static_cast<const int32_t*>(c.x)[r];
        default: return static_cast<const int64_t*>(c.x)[r];
    }
}
// doubles compare by value (ColumnValue ==): -0.0 == 0.0
__device__ __forceinline__ uint64_t gCanon(const GroupCol& c, int64_t x) {
    if (c.kind == kGroupDouble && __longlong_as_double(x) == 0.0) return 0;
    return static_cast<uint64_t>(x);
}
__device__ __forceinline__ int64_t gOrderKey(int64_t bits) {      // double bits -> int64 with the same order
    return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}

__device__ uint64_t gHash(const GroupAssignArgs& a, uint64_t r) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    for (int k = 0; k < a.nk; k++) {
        const GroupCol& c = a.k[k];
        const int64_t x = gRead(c, r);
        if (c.kind == kGroupString) {
            const uint32_t len = c.len ? c.len[r] : 0;
            const char* p = reinterpret_cast<const char*>(x);
            uint64_t w = len;
            for (uint32_t i = 0; i < len; i++) w = (w ^ static_cast<uint8_t>(p[i])) * 0x100000001B3ULL;
            h = gmix(h ^ w);
        } else {
            h = gmix(h ^ gCanon(c, x));
        }
    }
    return h;
}
__device__ bool gEqual(const GroupAssignArgs& a, uint64_t r, uint64_t o) {
    for (int k = 0; k < a.nk; k++) {
        const GroupCol& c = a.k[k];
        const int64_t x = gRead(c, r), y = gRead(c, o);
        if (c.kind == kGroupString) {
            const uint32_t l1 = c.len ? c.len[r] : 0, l2 = c.len ? c.len[o] : 0;
            if (l1 != l2) return false;
            const char* p1 = reinterpret_cast<const char*>(x);
            const char* p2 = reinterpret_cast<const char*>(y);
            for (uint32_t i = 0; i < l1; i++) if (p1[i] != p2[i]) return false;
        } else if (gCanon(c, x) != gCanon(c, y)) {
            return false;
        }
    }
    return true;
}

__global__ __launch_bounds__(256) void k_group_assign(GroupAssignArgs a) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t h = gHash(a, r);
    const uint64_t tag = (h >> 32) << 32;
    const uint64_t mine = tag | (r + 1);
    uint64_t slot = h & a.mask;
    uint64_t lead = r, first = 1;
    for (uint64_t probes = 0; probes <= a.mask; probes++) {
        // a slot is written once (0 -> tag | row + 1), so a non-zero load is final: only the rows that find
        // their slot still empty pay the CAS (few groups: ~ngroups CASes a wave in flight, not one per row)
        uint64_t cur = __hip_atomic_load(a.table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0)
            cur = atomicCAS(reinterpret_cast<unsigned long long*>(a.table + slot), 0ULL,
                            static_cast<unsigned long long>(mine));
        if (cur == 0) break;
        const uint64_t o = (cur & 0xFFFFFFFFULL) - 1;
        if ((cur >> 32) << 32 == tag && gEqual(a, r, o)) { lead = o; first = 0; break; }
        slot = (slot + 1) & a.mask;
    }
    if (a.leader) a.leader[r] = static_cast<uint32_t>(lead);
    a.flag[r] = first;
}

__device__ __forceinline__ uint64_t gIdentity(int op) {
    switch (op) {
        case kGroupAnd: return ~0ULL;
        case kGroupMax: return 0x8000000000000000ULL;
        case kGroupMin: return 0x7FFFFFFFFFFFFFFFULL;
        default: return 0;
    }
}
__global__ __launch_bounds__(256) void k_group_init(const GroupSlot* slots, int nslots, uint64_t ngroups, uint64_t* state) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < ngroups * static_cast<uint64_t>(nslots)) state[i] = gIdentity(slots[i / ngroups].op);
}

// one state word takes one value: a single 64-bit atomic each (LDS or global by the pointer's address space)
template <typename W>
__device__ __forceinline__ void gApply(int op, W* p, uint64_t v) {
    switch (op) {
        case kGroupAddF64: atomicAdd(reinterpret_cast<double*>(p), __longlong_as_double(static_cast<int64_t>(v))); break;
        case kGroupAnd: atomicAnd(p, static_cast<unsigned long long>(v)); break;
        case kGroupOr: atomicOr(p, static_cast<unsigned long long>(v)); break;
        case kGroupXor: atomicXor(p, static_cast<unsigned long long>(v)); break;
        case kGroupMax: atomicMax(reinterpret_cast<long long*>(p), static_cast<long long>(v)); break;
        case kGroupMin: atomicMin(reinterpret_cast<long long*>(p), static_cast<long long>(v)); break;
        default: atomicAdd(p, static_cast<unsigned long long>(v)); break;      // kGroupAdd
    }
}
__device__ __forceinline__ uint64_t gSlotValue(const GroupAccumArgs& a, const GroupSlot& s, uint64_t r) {
    if (s.src == kGroupSrcOne) return 1;
    if (s.src == kGroupSrcFlag) return s.flag[r];
    const int64_t x = gRead(a.cols[s.col], r);
    return static_cast<uint64_t>(s.src == kGroupSrcOrdered ? gOrderKey(x) : x);
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_group_accum(GroupAccumArgs a) {
    extern __shared__ unsigned long long gLds[];
    const uint64_t words = a.ngroups * static_cast<uint64_t>(a.nslots);
    if (LDS) {
        for (uint64_t i = threadIdx.x; i < words; i += blockDim.x) gLds[i] = gIdentity(a.slots[i / a.ngroups].op);
        __syncthreads();
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < a.n; r += stride) {
        const uint64_t g = a.pre[a.leader[r]];
        for (int s = 0; s < a.nslots; s++) {
            const GroupSlot sl = a.slots[s];
            const uint64_t v = gSlotValue(a, sl, r);
            if (LDS) gApply(sl.op, gLds + s * a.ngroups + g, v);
            else gApply(sl.op, reinterpret_cast<unsigned long long*>(a.state) + s * a.ngroups + g, v);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint64_t i = threadIdx.x; i < words; i += blockDim.x) {
            const int op = a.slots[i / a.ngroups].op;
            const uint64_t v = gLds[i];
            if (v != gIdentity(op)) gApply(op, reinterpret_cast<unsigned long long*>(a.state) + i, v);
        }
    }
}

// bytes of the string cells a leader row emits (0 for the other rows)
__global__ __launch_bounds__(256) void k_group_strlen(GroupEmitArgs a, uint64_t* slen) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    uint64_t total = 0;
    if (a.flag[r])
        for (int y = 0; y < a.ny; y++) {
            const GroupEmit e = a.emit[y];
            if (e.src == kEmitKey && a.cols[e.a].kind == kGroupString && a.cols[e.a].len) total += a.cols[e.a].len[r];
        }
    slen[r] = total;
}

// the finalised value bits of a yield column kept in state words (every kEmit* but kEmitKey / kEmitConst)
__device__ __forceinline__ int64_t gFinal(const GroupEmit& e, const uint64_t* state, uint64_t ngroups, uint64_t g) {
    switch (e.src) {
        case kEmitOrdered: return gOrderKey(static_cast<int64_t>(state[e.a * ngroups + g]));
        case kEmitAvgInt:
            return __double_as_longlong(static_cast<double>(static_cast<int64_t>(state[e.a * ngroups + g])) /
                                        static_cast<double>(state[(e.a + 1) * ngroups + g]));
        case kEmitAvgF64:
            return __double_as_longlong(__longlong_as_double(static_cast<int64_t>(state[e.a * ngroups + g])) /
                                        static_cast<double>(state[(e.a + 1) * ngroups + g]));
        default: return static_cast<int64_t>(state[e.a * ngroups + g]);      // kEmitState
    }
}

__global__ __launch_bounds__(256) void k_group_emit(GroupEmitArgs a) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n || !a.flag[r]) return;
    const uint64_t g = a.pre[r];
    uint64_t soff = a.strPre ? a.strPre[r] : 0;
    for (int y = 0; y < a.ny; y++) {
        const GroupEmit e = a.emit[y];
        GroupCell out;
        out.kind = e.kind;
        out.len = 0;
        out.v = 0;
        switch (e.src) {
            case kEmitKey: {
                const GroupCol& c = a.cols[e.a];
                const int64_t x = gRead(c, r);
                if (c.kind == kGroupString) {
                    const uint32_t len = c.len ? c.len[r] : 0;
                    const char* p = reinterpret_cast<const char*>(x);
                    for (uint32_t i = 0; i < len; i++) a.strOut[soff + i] = p[i];
                    out.len = static_cast<int32_t>(len);
                    out.v = static_cast<int64_t>(soff);
                    soff += len;
                } else {
                    out.v = x;
                }
                break;
            }
            case kEmitConst: out.v = e.konst; break;
            default: out.v = gFinal(e, a.state, a.ngroups, g); break;
        }
        a.cells[g * a.ny + y] = out;
    }
}

// the group rows as columns: one thread per leader row writes one value per yield column at its group id
// (what k_group_emit writes as cells; the same expressions, so the bits are equal)
__global__ __launch_bounds__(256) void k_group_columns(GroupColumnsArgs a) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n || !a.flag[r]) return;
    const uint64_t g = a.pre[r];
    if (g >= a.ngroups) return;
    for (int y = 0; y < a.ny; y++) {
        const GroupColumnOut o = a.out[y];
        if (!o.x) continue;                                       // kEmitConst: the column has no array
        const GroupEmit e = a.emit[y];
        int64_t v;
        if (e.src == kEmitKey) {
            const GroupCol& c = a.cols[e.a];
            v = gRead(c, r);
            if (o.len) o.len[g] = c.len ? c.len[r] : 0;
        } else {
            v = gFinal(e, a.state, a.ngroups, g);
        }
        switch (o.w) {
            case 1: static_cast<int8_t*>(o.x)[g] = static_cast<int8_t>(v); break;
            case 2: static_cast<int16_t*>(o.x)[g] = static_cast<int16_t>(v); break;
            case 4: static_cast<int32_t*>(o.x)[g] = static_cast<int32_t>(v); break;
            default: static_cast<int64_t*>(o.x)[g] = v; break;
        }
    }
}

}  // namespace

int launchGroupAssign(const GroupAssignArgs& a, hipStream_t s) {
    if (a.n == 0) return 0;
    if (a.n >= (1ULL << 32) || a.nk < 1 || a.nk > kGroupMaxKeys + 1) return 1;
    hipLaunchKernelGGL(k_group_assign, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchGroupAccum(const GroupAccumArgs& a, bool lds, uint32_t gridMax, hipStream_t s) {
    if (a.ngroups == 0 || a.nslots == 0) return 0;
    const uint64_t words = a.ngroups * static_cast<uint64_t>(a.nslots);
    hipLaunchKernelGGL(k_group_init, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, s, a.slots, a.nslots,
                       a.ngroups, a.state);
    if (a.n == 0) return static_cast<int>(hipGetLastError());
    if (lds) {
        if (words * 8 > kGroupLdsBytes) return 1;
        // few groups: each workgroup folds many rows into its LDS copy before the one flush
        const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((a.n + 255) / 256, gridMax ? gridMax : kGroupLdsGridMax));
        hipLaunchKernelGGL(k_group_accum<true>, dim3(grid), dim3(256), words * 8, s, a);
    } else {
        const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((a.n + 255) / 256, gridMax ? gridMax : 1u << 20));
        hipLaunchKernelGGL(k_group_accum<false>, dim3(grid), dim3(256), 0, s, a);
    }
    return static_cast<int>(hipGetLastError());
}

int launchGroupStrLen(const GroupEmitArgs& a, uint64_t* slen, hipStream_t s) {
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_group_strlen, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, s, a, slen);
    return static_cast<int>(hipGetLastError());
}

int launchGroupEmit(const GroupEmitArgs& a, hipStream_t s) {
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_group_emit, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchGroupColumns(const GroupColumnsArgs& a, hipStream_t s) {
    if (a.n == 0 || a.ngroups == 0) return 0;
    if (a.ny < 1 || !a.out) return 1;
    hipLaunchKernelGGL(k_group_columns, dim3(static_cast<unsigned>((a.n + 255) / 256)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
