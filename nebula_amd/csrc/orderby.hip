// ORDER BY ... LIMIT over a device-resident GO result (ngx_go_order_by; OrderByExecutor's comparator,
// src/graph/OrderByExecutor.cpp:14-105, and LimitExecutor's window, src/graph/LimitExecutor.cpp:52-61).
//
// The K = offset + count first rows of the order are selected without sorting: an MSD radix select over
// levels (kernels.h OrderLevel: one order-preserving unsigned word per row and level, the row's index last,
// so the order is total and exactly K rows win). One step takes 8 bits of the current level:
//   count    every tied row's digit goes into its workgroup's LDS histogram (a wave whose rows share one
//            digit adds once), flushed once per workgroup into the 256 global counters
//            (cdna_hip_programming.md Guideline 12: no chip-wide atomics into a few hot addresses);
//   pick     one workgroup finds the digit where the running count crosses the pivot's rank: rows below it
//            win, rows above it are out, rows on it stay tied. The next pass over the tied rows marks them
//            so (lazily: the decision lives in OrderState), so a step reads each tied row's column once;
//   compact  once the tied rows are <= 1 / kOrderCompactDiv of the rows the count read, they are listed by
//            row id (collected in LDS, list space reserved a buffer at a time) and later steps read the list.
// The host enqueues the steps of a level back to back and reads the state once per level (to stop at a
// pivot found early); no digit costs a host round trip. A final pass gathers the winners' row ids; the emit
// kernel writes their cells and string bytes (as k_group_emit). The <= K winners are ordered on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

// value bits of row r, integers sign-extended from the stored width; width 0: the column's constant
__device__ __forceinline__ int64_t oRead(const GroupCol& c, uint64_t r) {
    switch (c.w) {
        case 0: return c.konst;
        case 1: return static_cast<const int8_t*>(c.x)[r];
        case 2: return static_cast<const int16_t*>(c.x)[r];
        case 4: return static_cast<const int32_t*>(c.x)[r];
        default: return static_cast<const int64_t*>(c.x)[r];
    }
}

// the level's word of row r: L.bits significant bits, the rest zero
__device__ uint64_t oWord(const OrderArgs& a, const OrderLevel& L, uint64_t r) {
    if (L.kind == kOrdRow) return r;
    const GroupCol& c = a.cols[L.col];
    const uint64_t mask = L.bits >= 64 ? ~0ULL : (1ULL << L.bits) - 1;
    uint64_t w = 0;
    switch (L.kind) {
        case kOrdInt:
            w = static_cast<uint64_t>(oRead(c, r)) + (1ULL << (L.bits - 1));
            break;
        case kOrdDouble: {
            uint64_t b = static_cast<uint64_t>(oRead(c, r));
            if (__longlong_as_double(static_cast<int64_t>(b)) == 0.0) b = 0;          // -0.0 == 0.0
            w = b ^ (static_cast<uint64_t>(static_cast<int64_t>(b) >> 63) | 0x8000000000000000ULL);
            break;
        }
        case kOrdStrWord: {
            const uint8_t* p = reinterpret_cast<const uint8_t*>(oRead(c, r));
            const uint32_t len = c.len ? c.len[r] : 0;
            const uint32_t at = static_cast<uint32_t>(L.word) * 8;
            for (uint32_t j = 0; j < 8; j++) w = (w << 8) | (at + j < len ? p[at + j] : 0);
            break;
        }
        default:                                                  // kOrdStrLen
            w = c.len ? c.len[r] : 0;
            break;
    }
    w &= mask;
    return L.desc ? ~w & mask : w;
}

// the rows a pass after the last pick reads: the list the compaction behind that pick filled, else the
// current list, else every row
struct OrderDomain {
    const uint32_t* list;               // null: rows 0 .. len
    uint64_t len;
};
__device__ __forceinline__ OrderDomain oDomain(const OrderArgs& a, const OrderState& S) {
    if (S.compacted) return {a.list[S.cur ^ 1], S.nTied};
    if (S.listed) return {a.list[S.cur], S.listLen};
    return {nullptr, a.n};
}

__global__ __launch_bounds__(256) void k_order_maxlen(const uint32_t* len, uint64_t n, uint32_t* out) {
    __shared__ uint32_t m;
    if (threadIdx.x == 0) m = 0;
    __syncthreads();
    uint32_t mine = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) mine = max(mine, len[r]);
    if (mine) atomicMax(&m, mine);
    __syncthreads();
    if (threadIdx.x == 0 && m) atomicMax(out, m);
}

__global__ __launch_bounds__(256) void k_order_count(OrderArgs a, uint32_t level, uint32_t shift) {
    __shared__ uint32_t h[256];
    const OrderState S = *a.S;
    if (S.done) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const OrderDomain D = oDomain(a, S);
    const OrderLevel L = a.levels[level];
    OrderLevel P{};
    if (S.hasPrev) P = a.levels[S.pLevel];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < D.len; b0 += stride) {   // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        int d = -1;
        if (i < D.len) {
            const uint64_t r = D.list ? D.list[i] : i;
            if (r < a.n && a.mark[r] == kOrdTied) {
                bool tied = true;
                if (S.hasPrev) {                                  // the digit decided last: mark the rows that left
                    const uint32_t pd = static_cast<uint32_t>(oWord(a, P, r) >> S.pShift) & 255;
                    if (pd != S.pDigit) {
                        a.mark[r] = pd < S.pDigit ? kOrdWin : kOrdOut;
                        tied = false;
                    }
                }
                if (tied) d = static_cast<int>(oWord(a, L, r) >> shift) & 255;
            }
        }
        const uint64_t active = __ballot(d >= 0);
        if (active) {
            const int lead = __ffsll(static_cast<unsigned long long>(active)) - 1;
            const int d0 = __shfl(d, lead);
            if (__ballot(d >= 0 && d != d0) == 0) {              // one digit in the wave: one add
                if (static_cast<int>(lane) == lead) atomicAdd(&h[d0], static_cast<uint32_t>(__popcll(active)));
            } else if (d >= 0) {
                atomicAdd(&h[d], 1u);
            }
        }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(a.hist) + threadIdx.x, static_cast<unsigned long long>(h[threadIdx.x]));
}

__global__ __launch_bounds__(256) void k_order_pick(OrderArgs a, uint32_t level, uint32_t shift, uint32_t last) {
    __shared__ uint64_t c[256];
    OrderState* S = a.S;
    if (S->done) return;                                          // read by every thread before thread 0 writes (barrier below)
    c[threadIdx.x] = a.hist[threadIdx.x];
    a.hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (S->compacted) {                                           // the counts came from the new list: it is the current one now
        S->compactions++;
        if (S->listed) S->listCompactions++;                      // the compaction read a list already
        S->cur ^= 1;
        S->listed = 1;
        S->listLen = S->nTied;
        S->fill = 0;
        S->compacted = 0;
    }
    const uint64_t rank = S->rank;
    uint64_t below = 0;
    uint32_t b = 0;
    for (; b < 256; b++) {
        if (rank < below + c[b]) break;
        below += c[b];
    }
    if (b == 256) {                                               // the tied rows are fewer than the rank: cannot be
        S->err = 1;
        S->done = 1;
        return;
    }
    S->rank = rank - below;
    S->nTied = c[b];
    S->hasPrev = 1;
    S->pLevel = level;
    S->pShift = shift;
    S->pDigit = b;
    if (c[b] == 1 || last) {
        S->done = 1;
        return;
    }
    const uint64_t dom = S->listed ? S->listLen : a.n;
    if (c[b] * kOrderCompactDiv <= dom && c[b] <= a.listCap) S->compacted = 1;
}

// GATHER false: the compaction (when the last pick asked for it): the rows still tied go to list[cur ^ 1],
// the others of the current domain are marked. GATHER true: the winners (marked, or tied at or below the
// pivot's digit) of all n rows go to win. Row ids collect in LDS; a full buffer reserves its space with one
// atomicAdd and is copied out.
template <bool GATHER>
__global__ __launch_bounds__(256) void k_order_collect(OrderArgs a) {
    __shared__ uint32_t buf[kOrderAppendBuf];
    __shared__ uint32_t cnt;
    __shared__ uint64_t base;
    const OrderState S = *a.S;
    if (!GATHER && (!S.compacted || S.done)) return;
    const uint32_t* list = !GATHER && S.listed ? a.list[S.cur] : nullptr;
    const uint64_t dom = list ? S.listLen : a.n;
    uint32_t* dst = GATHER ? a.win : a.list[S.cur ^ 1];
    const uint64_t cap = GATHER ? a.winCap : a.listCap;
    unsigned long long* fill = reinterpret_cast<unsigned long long*>(GATHER ? &a.S->nWin : &a.S->fill);
    OrderLevel P{};
    if (S.hasPrev) P = a.levels[S.pLevel];
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    auto flush = [&](uint32_t have) {                             // called by the whole workgroup, after a barrier
        if (threadIdx.x == 0) base = atomicAdd(fill, static_cast<unsigned long long>(have));
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < have; j += 256) {
            const uint64_t o = base + j;
            if (o < cap) dst[o] = buf[j];
            else a.S->err = 1;
        }
        __syncthreads();
        if (threadIdx.x == 0) cnt = 0;
        __syncthreads();
    };
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < dom; b0 += stride) {     // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        bool keep = false;
        uint64_t r = 0;
        if (i < dom) {
            r = list ? list[i] : i;
            const uint8_t m = r < a.n ? a.mark[r] : static_cast<uint8_t>(kOrdOut);
            if (m == kOrdTied) {
                if (S.hasPrev) {
                    const uint32_t pd = static_cast<uint32_t>(oWord(a, P, r) >> S.pShift) & 255;
                    if (GATHER) {
                        keep = pd <= S.pDigit;
                    } else {
                        keep = pd == S.pDigit;
                        if (!keep) a.mark[r] = pd < S.pDigit ? kOrdWin : kOrdOut;
                    }
                } else {
                    keep = true;
                }
            } else if (GATHER) {
                keep = m == kOrdWin;
            }
        }
        if (keep) buf[atomicAdd(&cnt, 1u)] = static_cast<uint32_t>(r);       // cnt <= kOrderAppendBuf - 256 before the adds
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

constexpr int kCellEmpty = 0, kCellInt = 2, kCellDouble = 5, kCellStr = 6;    // NGX_CELL_*
// the cell kind of a value of per-row type t (ngx_dev_column::type: 1 int, 2 double, 3 bool, 4 string), as
// the cell path types an UNKNOWN column: a bool stays an EMPTY cell with len 1 and its value
__device__ __forceinline__ int oCellKind(const OrderEmitCol& e, uint64_t r, bool* isStr, int32_t* len) {
    int kind = e.cell;
    *len = 0;
    if (e.type) {
        const uint8_t t = e.type[r];
        kind = t == 1 ? kCellInt : t == 2 ? kCellDouble : t == 4 ? kCellStr : kCellEmpty;
        if (t == 3) *len = 1;
    }
    *isStr = kind == kCellStr;
    return kind;
}

__global__ __launch_bounds__(256) void k_order_strlen(OrderEmitArgs a, uint64_t* slen) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= a.m) return;
    const uint64_t r = a.rows ? a.rows[i] : a.base + i;
    uint64_t total = 0;
    if (r < a.n)
        for (int y = 0; y < a.ncols; y++) {
            const OrderEmitCol& e = a.cols[y];
            bool isStr;
            int32_t l;
            oCellKind(e, r, &isStr, &l);
            if (isStr && e.c.len) total += e.c.len[r];
        }
    slen[i] = total;
}

__global__ __launch_bounds__(256) void k_order_emit(OrderEmitArgs a) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= a.m) return;
    const uint64_t r = a.rows ? a.rows[i] : a.base + i;
    uint64_t soff = a.strPre ? a.strPre[i] : 0;
    for (int y = 0; y < a.ncols; y++) {
        const OrderEmitCol& e = a.cols[y];
        GroupCell out;
        out.kind = kCellEmpty;
        out.len = 0;
        out.v = 0;
        if (r < a.n) {
            bool isStr;
            int32_t l;
            out.kind = oCellKind(e, r, &isStr, &l);
            out.len = l;
            const int64_t x = oRead(e.c, r);
            if (isStr) {
                const uint32_t len = e.c.len && a.strOut ? e.c.len[r] : 0;
                const char* p = reinterpret_cast<const char*>(x);
                for (uint32_t j = 0; j < len; j++) a.strOut[soff + j] = p[j];
                out.len = static_cast<int32_t>(len);
                out.v = static_cast<int64_t>(soff);
                soff += len;
            } else if (out.kind != kCellEmpty || l) {
                out.v = x;
            }
        }
        a.cells[i * a.ncols + y] = out;
    }
}

unsigned orderGrid(uint64_t n, uint32_t gridMax = 0) {
    return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, gridMax ? gridMax : kOrderGridMax));
}

}  // namespace

int launchOrderMaxLen(const uint32_t* len, uint64_t n, uint32_t* out, hipStream_t s) {
    if (hipMemsetAsync(out, 0, sizeof(uint32_t), s) != hipSuccess) return 1;
    if (n == 0 || !len) return 0;
    hipLaunchKernelGGL(k_order_maxlen, dim3(std::min(orderGrid(n), 1024u)), dim3(256), 0, s, len, n, out);
    return static_cast<int>(hipGetLastError());
}

int launchOrderStep(const OrderArgs& a, int level, int shift, bool last, hipStream_t s) {
    if (a.n == 0 || a.n >= (1ULL << 32) || level < 0 || level >= a.nlevels || shift < 0 || shift > 56 || shift % 8) return 1;
    hipLaunchKernelGGL(k_order_count, dim3(orderGrid(a.n, a.gridMax)), dim3(256), 0, s, a, static_cast<uint32_t>(level), static_cast<uint32_t>(shift));
    hipLaunchKernelGGL(k_order_pick, dim3(1), dim3(256), 0, s, a, static_cast<uint32_t>(level), static_cast<uint32_t>(shift),
                       last ? 1u : 0u);
    if (!last) hipLaunchKernelGGL(k_order_collect<false>, dim3(orderGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchOrderGather(const OrderArgs& a, hipStream_t s) {
    if (a.n == 0 || a.n >= (1ULL << 32)) return 1;
    hipLaunchKernelGGL(k_order_collect<true>, dim3(orderGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchOrderStrLen(const OrderEmitArgs& a, uint64_t* slen, hipStream_t s) {
    if (a.m == 0) return 0;
    hipLaunchKernelGGL(k_order_strlen, dim3(static_cast<unsigned>((a.m + 255) / 256)), dim3(256), 0, s, a, slen);
    return static_cast<int>(hipGetLastError());
}

int launchOrderEmit(const OrderEmitArgs& a, hipStream_t s) {
    if (a.m == 0) return 0;
    hipLaunchKernelGGL(k_order_emit, dim3(static_cast<unsigned>((a.m + 255) / 256)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
