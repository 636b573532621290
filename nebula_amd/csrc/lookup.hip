// LOOKUP ON a tag / an edge type as a column scan in HBM (ngx_lookup; LookupExecutor with LookUpIndexProcessor /
// IndexExecutor behind it). kernels.h LookupArgs states the three steps.
//
// The reference scans a sorted copy of the indexed fields (index keys in the KV store) between two byte strings and
// filters what the bounds do not express. Here the fields are the tag's / the edge type's stored columns, so the
// scan is one pass over them: every row's scanned fields are encoded to the 64-bit key the index would hold for
// them (NebulaKeyUtils::encodeInt64 / encodeDouble: the 8 big-endian key bytes read as a u64) and compared with the
// plan's [lo, hi); BOOL and STRING fields are compared typed; residual terms are evaluated with
// RelationalExpression::eval's typing over the values as the index key would give them back.
//
// keep is a stream: a thread owns a row, consecutive lanes read consecutive elements of every column (a wave's
// load of a w-byte column is one 64 * w byte line), nothing is gathered. emit gathers only the kept rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace ngx {
namespace {

constexpr int32_t kCellInt = 2, kCellVid = 3, kCellStr = 6;
constexpr uint64_t kTop = 1ULL << 63;

// integers sign-extended from the stored width
__device__ __forceinline__ int64_t lLoadW(const void* p, int32_t w, uint64_t i) {
    switch (w) {
        case 1: return static_cast<const int8_t*>(p)[i];
        case 2: return static_cast<const int16_t*>(p)[i];
        case 4: return static_cast<const int32_t*>(p)[i];
        default: return static_cast<const int64_t*>(p)[i];
    }
}

// encodeInt64: the sign bit flipped, big-endian
__device__ __forceinline__ uint64_t lKeyInt(int64_t v) { return static_cast<uint64_t>(v) ^ kTop; }

// encodeDouble: a value below zero has its bits replaced by -(INT64_MAX + bits), then the top bit is flipped
// (-0.0 is not below zero: its key is 0)
__device__ __forceinline__ uint64_t lKeyDouble(uint64_t bits) {
    if (__longlong_as_double(static_cast<long long>(bits)) < 0) bits = 0 - (0x7FFFFFFFFFFFFFFFULL + bits);
    return bits ^ kTop;
}
// decodeDouble of that key: what a residual term compares
__device__ __forceinline__ double lKeyDoubleBack(uint64_t key) {
    uint64_t bits = key ^ kTop;
    if (__longlong_as_double(static_cast<long long>(bits)) < 0) bits = 0 - (0x7FFFFFFFFFFFFFFFULL + bits);
    return __longlong_as_double(static_cast<long long>(bits));
}

// memcmp order, the shorter a prefix of the longer: std::string's
__device__ int lStrCmp(const char* a, uint64_t na, const char* b, uint64_t nb) {
    const uint64_t n = na < nb ? na : nb;
    for (uint64_t j = 0; j < n; j++) {
        const uint8_t x = static_cast<uint8_t>(a[j]), y = static_cast<uint8_t>(b[j]);
        if (x != y) return x < y ? -1 : 1;
    }
    return na < nb ? -1 : na > nb ? 1 : 0;
}

template <typename T>
__device__ __forceinline__ bool lRel(int32_t op, T a, T b) {
    switch (op) {
        case kLkLT: return a < b;
        case kLkLE: return a <= b;
        case kLkGT: return a > b;
        case kLkGE: return a >= b;
        case kLkEQ: return a == b;
        default: return a != b;
    }
}

// a scanned field of row r against the plan's bounds
__device__ bool lScan(const LookupCond& f, uint64_t r, const char* pool) {
    if (f.kind == kLkInt || f.kind == kLkDouble) {
        const uint64_t k = f.kind == kLkInt ? lKeyInt(lLoadW(f.col.data, f.col.width, r))
                                            : lKeyDouble(static_cast<const uint64_t*>(f.col.data)[r]);
        return f.lo == f.hi ? k == f.lo : (k >= f.lo && k < f.hi);       // begin == end is a prefix scan
    }
    if (f.kind == kLkBool) return (static_cast<const uint8_t*>(f.col.data)[r] != 0) == (f.lo != 0);
    const uint64_t b = f.col.soff[r], e = f.col.soff[r + 1];
    if (e - b != static_cast<uint64_t>(f.slen)) return false;
    return lStrCmp(f.col.sbytes + b, e - b, pool + f.soff, static_cast<uint64_t>(f.slen)) == 0;
}

// a residual term: RelationalExpression::eval (implicitCasting bool -> int -> double; a string against a
// non-string fails the row; == / != on doubles within 1e-8)
__device__ bool lTerm(const LookupCond& t, uint64_t r, const char* pool) {
    if (t.kind == kLkString || t.ckind == kLkString) {
        if (t.kind != t.ckind) return false;
        const uint64_t b = t.col.soff[r], e = t.col.soff[r + 1];
        return lRel<int>(t.op, lStrCmp(t.col.sbytes + b, e - b, pool + t.soff, static_cast<uint64_t>(t.slen)), 0);
    }
    int64_t vi = 0;
    double vd = 0;
    if (t.kind == kLkInt) vi = lLoadW(t.col.data, t.col.width, r);
    else if (t.kind == kLkBool) vi = static_cast<const uint8_t*>(t.col.data)[r] ? 1 : 0;
    else vd = lKeyDoubleBack(lKeyDouble(static_cast<const uint64_t*>(t.col.data)[r]));
    if (t.kind == kLkDouble || t.ckind == kLkDouble) {
        const double a = t.kind == kLkDouble ? vd : static_cast<double>(vi);
        const double b = t.ckind == kLkDouble ? __longlong_as_double(static_cast<long long>(t.lo))
                                              : static_cast<double>(static_cast<int64_t>(t.lo));
        if (t.op == kLkEQ) return fabs(a - b) < 1e-8;
        if (t.op == kLkNE) return !(fabs(a - b) < 1e-8);
        return lRel<double>(t.op, a, b);
    }
    return lRel<int64_t>(t.op, vi, static_cast<int64_t>(t.lo));       // int / bool (0, 1) on both sides
}

__global__ __launch_bounds__(256) void k_lookup_keep(LookupArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        bool keep = false;
        if (i < a.n) {
            keep = a.edge || a.present[i] != 0;
            for (int f = 0; keep && f < a.nf; f++) keep = lScan(a.conds[f], i, a.pool);
            for (int t = 0; keep && t < a.nt; t++) keep = lTerm(a.conds[a.nf + t], i, a.pool);
            a.keep[i] = keep ? 1 : 0;
        }
        const uint64_t kept = __ballot(keep);
        if (lane == 0) waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
        __syncthreads();
        if (threadIdx.x == 0) a.chunkCount[b0 >> 8] = static_cast<uint64_t>(waveCount[0]) + waveCount[1] + waveCount[2] + waveCount[3];
        __syncthreads();                                          // the counts are read before the next turn's writes
    }
}

// the stored column's value of row r as a cell; a string's bytes go to strOut + *soff (null: only counted)
__device__ GroupCell lColumn(const LookupYield& y, uint64_t r, char* strOut, uint64_t* soff) {
    GroupCell c;
    c.kind = y.cell;
    c.len = 0;
    c.v = 0;
    const DCol& col = y.col;
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
        c.v = lLoadW(col.data, col.width, r);
    }
    return c;
}

// the row owning edge e: the last row with off[row] <= e. Rows with empty adjacencies share their offset with
// the next row, so the search is an upper bound (the first row whose offset is above e, minus one): a lower bound
// would land on the first of the rows sharing the offset, an empty one.
__device__ uint64_t lSourceRow(const uint64_t* off, uint64_t V, uint64_t e) {
    uint64_t lo = 0, hi = V + 1;                                  // off[V] = the slot's edges > e
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;                                                // off[0] = 0 <= e: lo >= 1
}

__global__ __launch_bounds__(256) void k_lookup_emit(LookupArgs a) {
    __shared__ uint32_t waveCount[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkey = a.edge ? 3 : 1;
    const int ncols = nkey + a.ny;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * 256; b0 < a.n; b0 += stride) {       // uniform in the workgroup
        const uint64_t i = b0 + threadIdx.x;
        const bool keep = i < a.n && a.keep[i] != 0;
        const uint64_t kept = __ballot(keep);
        if (lane == 0) waveCount[wave] = static_cast<uint32_t>(__popcll(kept));
        __syncthreads();
        uint64_t o = a.chunkBase[b0 >> 8] + static_cast<uint64_t>(__popcll(kept & ((1ULL << lane) - 1)));
        for (uint32_t w = 0; w < wave; w++) o += waveCount[w];
        __syncthreads();
        if (!keep) continue;
        char* strOut = a.lenOut ? nullptr : a.strOut;
        uint64_t soff = a.lenOut || !a.strPre ? 0 : a.strPre[o];
        const uint64_t soff0 = soff;
        GroupCell* out = a.lenOut ? nullptr : a.cells + o * ncols;
        if (out) {
            GroupCell c;
            c.len = 0;
            c.kind = kCellVid;
            if (a.edge) {
                c.v = a.vid[lSourceRow(a.slot.off, a.V, i)];
                out[0] = c;
                c.v = lLoadW(a.slot.dst, a.slot.dstW, i);
                out[1] = c;
                c.kind = kCellInt;
                c.v = a.slot.rank ? lLoadW(a.slot.rank, a.slot.rankW, i) : a.slot.rankConst;
                out[2] = c;
            } else {
                c.v = a.vid[i];
                out[0] = c;
            }
        }
        for (int y = 0; y < a.ny; y++) {
            const GroupCell c = lColumn(a.ys[y], i, strOut, &soff);
            if (out) out[nkey + y] = c;
        }
        if (a.lenOut) a.lenOut[o] = soff - soff0;
    }
}

unsigned lookupGrid(uint64_t n, uint32_t gridMax) {
    return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, gridMax ? gridMax : kLookupGridMax));
}

bool lookupArgsOk(const LookupArgs& a) {
    if (a.n >= (1ULL << 40) || a.nf < 0 || a.nt < 0 || a.ny < 0 || a.nf > kLookupMax || a.nt > kLookupMax || a.ny > kLookupMax) return false;
    if (!a.keep || !a.chunkCount || ((a.nf || a.nt) && !a.conds) || (a.ny && !a.ys)) return false;
    if (a.edge ? (!a.slot.off || !a.slot.dst || !a.vid) : (!a.present || !a.vid)) return false;
    return true;
}

}  // namespace

int launchLookupKeep(const LookupArgs& a, hipStream_t s) {
    if (!lookupArgsOk(a)) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_lookup_keep, dim3(lookupGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

int launchLookupEmit(const LookupArgs& a, hipStream_t s) {
    if (!lookupArgsOk(a) || !a.chunkBase || (!a.lenOut && !a.cells)) return 1;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(k_lookup_emit, dim3(lookupGrid(a.n, a.gridMax)), dim3(256), 0, s, a);
    return static_cast<int>(hipGetLastError());
}

}  // namespace ngx
