// `| YIELD <columns> [WHERE <expr>]` over a device-resident GO result (ngx_go_yield; YieldExecutor::executeInputs,
// src/graph/YieldExecutor.cpp:171-279). kernels.h YieldArgs states the steps.
//
// The result's columns are read in place at their stored widths through the VM's result getter (vm.h vmEval<true>,
// opResultCol). keep and agg are streams: a thread owns a row, consecutive lanes read consecutive elements of every
// column. Rows are swept 256 a workgroup and turn, so a kept row's place in the output depends on its index alone:
// the projection comes out in the order of the rows in the device result under every grid size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"
#include "vm.h"

namespace ngx {
namespace {

constexpr int32_t kCellStr = 6;

__device__ __forceinline__ VmEnv yEnv(const YieldArgs& a, uint64_t poolOff) {
    VmEnv env{};
    env.pool = a.pool + poolOff;
    env.unsupported = a.err + 1;
    env.input = reinterpret_cast<const DInputCol*>(a.cols);
    return env;
}
__device__ __forceinline__ EdgeCtx yRow(uint64_t r) {
    EdgeCtx ec{};
    ec.pos = r;
    return ec;
}

__device__ __forceinline__ int64_t yOrderKey(int64_t bits) {      // double bits -> int64 with the same order
    return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}
__device__ __forceinline__ uint64_t yIdentity(int op) {
    switch (op) {
        case kGroupAnd: return ~0ULL;
        case kGroupMax: return 0x8000000000000000ULL;
        case kGroupMin: return 0x7FFFFFFFFFFFFFFFULL;
        case kGroupAddF64: return 0x8000000000000000ULL;          // -0.0: x + -0.0 is x for every x, -0.0 included
        default: return 0;
    }
}
__device__ __forceinline__ uint64_t yCombine(int op, uint64_t x, uint64_t y) {
    switch (op) {
        case kGroupAddF64:
            return static_cast<uint64_t>(__double_as_longlong(__longlong_as_double(static_cast<int64_t>(x)) +
                                                              __longlong_as_double(static_cast<int64_t>(y))));
        case kGroupAnd: return x & y;
        case kGroupOr: return x | y;
        case kGroupXor: return x ^ y;
        case kGroupMax: return static_cast<int64_t>(x) > static_cast<int64_t>(y) ? x : y;
        case kGroupMin: return static_cast<int64_t>(x) < static_cast<int64_t>(y) ? x : y;
        default: return x + y;                                    // kGroupAdd
    }
}
// one state word takes one value: a single 64-bit atomic (LDS or global by the pointer's address space)
template <typename W>
__device__ __forceinline__ void yApply(int op, W* p, uint64_t v) {
    switch (op) {
        case kGroupAddF64: atomicAdd(reinterpret_cast<double*>(p), __longlong_as_double(static_cast<int64_t>(v))); break;
        case kGroupAnd: atomicAnd(p, static_cast<unsigned long long>(v)); break;
        case kGroupOr: atomicOr(p, static_cast<unsigned long long>(v)); break;
        case kGroupXor: atomicXor(p, static_cast<unsigned long long>(v)); break;
        case kGroupMax: atomicMax(reinterpret_cast<long long*>(p), static_cast<long long>(v)); break;
        case kGroupMin: atomicMin(reinterpret_cast<long long*>(p), static_cast<long long>(v)); break;
        default: atomicAdd(p, static_cast<unsigned long long>(v)); break;
    }
}

// whether row i (< n) is kept, and the wave's kept lanes: keepBits' word, or every lane below n
__device__ __forceinline__ uint64_t yWaveKept(const YieldArgs& a, uint64_t b0, uint32_t wave) {
    const uint64_t first = b0 + 64ull * wave;                     // the wave's first row
    if (first >= a.n) return 0;
    if (a.keepBits) return a.keepBits[first >> 6];
    const uint64_t left = a.n - first;
    return left >= 64 ? ~0ULL : (1ULL << left) - 1;
}

__global__ __launch_bounds__(256) void k_yield_keep(YieldArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    const VmEnv env = yEnv(a, a.wherePool);
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        bool keep = false;
        if (i < a.n) {
            const Val v = vmEval<true>(a.code + a.whereOff, env, yRow(i));
            if (v.t == V_ERR) atomicOr(a.err, 1u);
            else keep = asBool(v);
        }
        const uint64_t kept = __ballot(keep);
        if (lane == 0) {
            waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
            if (b0 + 64ull * wave < a.n) a.keepBits[(b0 >> 6) + wave] = kept;
        }
        __syncthreads();
        if (threadIdx.x == 0) a.chunkCount[b0 >> 8] = static_cast<uint64_t>(waveCount[0]) + waveCount[1] + waveCount[2] + waveCount[3];
        __syncthreads();                                          // the counts are read before the next turn's writes
    }
}

// yield y of row r: the column's value (strings: pointer and length) or the program's; `ok` false when it failed
// or has another type than the first row's
__device__ __forceinline__ Val yValue(const YieldArgs& a, const YieldItem& it, uint64_t r, bool* ok) {
    if (it.mode == kYieldCol) return opResultCol(yEnv(a, 0), yRow(r), it.a);
    const Val v = vmEval<true>(a.code + it.a, yEnv(a, it.poolOff), yRow(r));
    if (v.t == V_ERR) { atomicOr(a.err, 1u); *ok = false; }
    else if (v.t != it.vt) { atomicOr(a.err, 2u); *ok = false; }
    return v;
}

__global__ __launch_bounds__(256) void k_yield_emit(YieldArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t kept = yWaveKept(a, b0, wave);
        const bool keep = (kept >> lane) & 1;
        uint64_t o = i;
        if (a.keepBits) {
            if (lane == 0) waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
            __syncthreads();
            o = a.chunkBase[b0 >> 8] + static_cast<uint64_t>(__popcll(kept & ((1ULL << lane) - 1)));
            for (uint32_t w = 0; w < wave; w++) o += waveCount[w];
            __syncthreads();
        }
        if (keep) {                                               // every lane reaches the next turn's barriers the same way
            uint64_t soff = a.lenOut || !a.strPre ? 0 : a.strPre[o];
            const uint64_t soff0 = soff;
            for (int y = 0; y < a.ny; y++) {
                const YieldItem it = a.items[y];
                if (a.lenOut) {                                       // the length pass: string columns only
                    if (it.mode == kYieldCol && it.cell == kCellStr && a.cols[it.a].len) soff += a.cols[it.a].len[i];
                    continue;
                }
                bool ok = true;
                const Val v = yValue(a, it, i, &ok);
                GroupCell c;
                c.kind = it.cell;
                c.len = 0;
                c.v = ok ? v.x : 0;
                if (it.cell == kCellStr) {
                    const char* p = reinterpret_cast<const char*>(v.x);
                    for (uint32_t j = 0; j < v.len; j++) a.strOut[soff + j] = p[j];
                    c.len = static_cast<int32_t>(v.len);
                    c.v = static_cast<int64_t>(soff);
                    soff += v.len;
                }
                a.cells[o * a.ny + y] = c;
            }
            if (a.lenOut) a.lenOut[o] = soff - soff0;
        }
    }
}

__global__ __launch_bounds__(256) void k_yield_agg(YieldArgs a) {
    __shared__ unsigned long long lds[2 * kYieldMax];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = threadIdx.x; s < a.nslots; s += 256) lds[s] = yIdentity(a.slots[s].op);
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t kept = yWaveKept(a, b0, wave);
        if (kept == 0) continue;                                  // uniform in the wave; no barrier below
        const bool keep = (kept >> lane) & 1;
        int curY = -1;
        bool ok = true;
        int64_t bits = 0;
        for (int s = 0; s < a.nslots; s++) {
            const YieldSlot sl = a.slots[s];
            if (sl.y != curY) {                                   // a yield's value serves all its slots
                curY = sl.y;
                ok = true;
                bits = 0;
                const YieldItem it = a.items[sl.y];
                if (keep && it.mode != kYieldNone) bits = yValue(a, it, i, &ok).x;
            }
            uint64_t v = yIdentity(sl.op);
            if (keep && ok) {
                switch (sl.src) {
                    case kYieldSrcOne: v = 1; break;
                    case kYieldSrcOrdered: v = static_cast<uint64_t>(yOrderKey(bits)); break;
                    case kYieldSrcRow: v = i + 1; break;
                    default: v = static_cast<uint64_t>(bits); break;
                }
            }
            for (int off = 32; off > 0; off >>= 1)
                v = yCombine(sl.op, v, static_cast<uint64_t>(__shfl_xor(static_cast<long long>(v), off, 64)));
            if (lane == 0) yApply(sl.op, lds + s, v);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < a.nslots; s += 256) {
        const int op = a.slots[s].op;
        const uint64_t v = lds[s];
        if (v != yIdentity(op)) yApply(op, reinterpret_cast<unsigned long long*>(a.state) + s, v);
    }
}

__global__ void k_yield_init(const YieldSlot* slots, int nslots, uint64_t* state) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nslots) state[s] = yIdentity(slots[s].op);
}

__global__ void k_yield_probe(YieldArgs a, uint64_t row, YieldProbe* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0 || row >= a.n) return;
    for (int y = 0; y < a.ny; y++) {
        const YieldItem it = a.items[y];
        YieldProbe p{0, 0, V_ERR};
        if (it.mode == kYieldEval) {
            const Val v = vmEval<true>(a.code + it.a, yEnv(a, it.poolOff), yRow(row));
            p.x = v.x, p.len = v.len, p.vt = v.t;
        }
        out[y] = p;
    }
}

unsigned yieldGrid(uint64_t n, uint32_t gridMax) {
    return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, gridMax ? gridMax : kYieldGridMax));
}

bool yieldArgsOk(const YieldArgs& a) {
    if (a.n >= (1ULL << 32) || a.ny < 0 || a.ny > kYieldMax || a.nslots < 0 || a.nslots > 2 * kYieldMax) return false;
    return a.cols && a.err && (!a.ny || a.items);
}

}  // namespace

int launchYieldKeep(const YieldArgs& a, hipStream_t s) {
    if (!yieldArgsOk(a) || !a.code || a.whereOff < 0 || !a.keepBits || !a.chunkCount) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_yield_keep, dim3(yieldGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchYieldEmit(const YieldArgs& a, hipStream_t s) {
    if (!yieldArgsOk(a) || a.ny < 1 || (a.keepBits && !a.chunkBase) || (!a.lenOut && !a.cells)) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_yield_emit, dim3(yieldGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchYieldAgg(const YieldArgs& a, hipStream_t s) {
    if (!yieldArgsOk(a) || a.nslots < 1 || !a.slots || !a.state) return 1;
    hipLaunchKernelGGL(k_yield_init, dim3(1), dim3(2 * kYieldMax), 0, s, a.slots, a.nslots, a.state);
    if (a.n == 0) return static_cast<int>(hipGetLastError());
    hipLaunchKernelGGL(k_yield_agg, dim3(yieldGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchYieldProbe(const YieldArgs& a, uint64_t row, YieldProbe* out, hipStream_t s) {
    if (!yieldArgsOk(a) || !out || row >= a.n) return 1;
    hipLaunchKernelGGL(k_yield_probe, dim3(1), dim3(64), 0, s, a, row, out);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
