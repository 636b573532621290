// Frontier bits of one chunk of the dense final hop (final_kernels.h finalBodyDense), without a chunk
// map: bit p of the chunk (word p / 64, bit p % 64: the layout of the kernel's ballot words, so a word
// is wave-uniform) says whether the row of the chunk's edge p is in the frontier.
//
// Every frontier row toggles the bit where its clipped edge range starts and the bit one past its end
// (when that lies inside the chunk); an inclusive prefix XOR over the CE bits then turns the toggles
// into runs. Two adjacent frontier rows toggle their shared boundary twice, which cancels, so their
// runs join. The cost is two LDS atomics per row and one pass of one wave over the words: nothing per
// edge and no loop over a degree.
//
// The arithmetic is plain C++ (the LDS atomics and the cross-lane carry stay in the kernel), so a host
// program runs the same source (tools/dense_mask_check.cpp).
#pragma once

#ifndef __HIPCC_RTC__
#include <cstdint>
#endif

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define NGX_HD __host__ __device__ __forceinline__
#else
#define NGX_HD inline
#endif

namespace ngx {

constexpr uint32_t kMaskBits = 2048;                   // == kChunk (kargs.h): edges of a chunk
constexpr uint32_t kMaskWords = kMaskBits / 64;

// The edges [e, e1) of a row clipped to the chunk [base, base + cnt), relative to base: [s, t), t <=
// cnt <= kMaskBits. False when the row has no edge in the chunk.
NGX_HD bool denseRowSpan(uint64_t e, uint64_t e1, uint64_t base, uint32_t cnt, uint32_t& s, uint32_t& t) {
    const uint64_t lo = e > base ? e : base;
    const uint64_t hi = e1 < base + cnt ? e1 : base + cnt;
    if (lo >= hi) return false;
    s = static_cast<uint32_t>(lo - base);
    t = static_cast<uint32_t>(hi - base);
    return true;
}

// inclusive prefix XOR of a word's bits: bit j of the result = XOR of bits 0 .. j
NGX_HD uint64_t densePrefixXor(uint64_t w) {
    w ^= w << 1;
    w ^= w << 2;
    w ^= w << 4;
    w ^= w << 8;
    w ^= w << 16;
    w ^= w << 32;
    return w;
}

// parity of a word's toggles: what it carries into every later word
NGX_HD uint32_t denseParity(uint64_t w) {
    w ^= w >> 32;
    w ^= w >> 16;
    w ^= w >> 8;
    w ^= w >> 4;
    w ^= w >> 2;
    w ^= w >> 1;
    return static_cast<uint32_t>(w & 1u);
}

// a word of toggles -> its run bits, given the parity of the toggles in all words before it
NGX_HD uint64_t denseRunWord(uint64_t toggles, uint32_t carryIn) {
    const uint64_t x = densePrefixXor(toggles);
    return carryIn ? ~x : x;
}

}  // namespace ngx
