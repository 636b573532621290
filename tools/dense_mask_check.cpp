// Host check of the dense final hop's frontier bits (nebula_amd/csrc/dense_mask.h): the same range and
// prefix-XOR arithmetic the kernel runs, with the LDS atomics as plain XORs and the wave's carry as a
// loop, against a per-edge loop over the chunk's rows. Built with ASan + UBSan and run by
// tests/test_dense_mask_host.py.
//
// Input (text, argv[1]): any number of cases
//   base cnt lo hi ep      the chunk's first CSR position and edge count, its rows lo .. hi, the epoch
//   off[lo] .. off[hi + 1] (hi - lo + 2 values)
//   mark[lo] .. mark[hi]   (hi - lo + 1 values)
// Output: one line per case, the 32 mask words in hex; exit status 1 on the first mismatch.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "dense_mask.h"

using namespace ngx;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: dense_mask_check CASES\n"); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t base, lo, hi;
    uint32_t cnt, ep;
    int ncase = 0;
    while (std::fscanf(f, "%" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu32, &base, &cnt, &lo, &hi, &ep) == 5) {
        if (hi < lo || cnt == 0 || cnt > kMaskBits) { std::fprintf(stderr, "case %d: bad header\n", ncase); return 2; }
        const uint64_t n = hi - lo + 1;
        std::vector<uint64_t> off(n + 1);
        std::vector<uint32_t> mark(n);
        for (auto& v : off) if (std::fscanf(f, "%" SCNu64, &v) != 1) return 2;
        for (auto& v : mark) if (std::fscanf(f, "%" SCNu32, &v) != 1) return 2;
        // the kernel's construction
        uint64_t tg[kMaskWords] = {};
        for (uint64_t i = 0; i < n; i++) {
            uint32_t s = 0, t = 0;
            if (mark[i] != ep || !denseRowSpan(off[i], off[i + 1], base, cnt, s, t)) continue;
            tg[s >> 6] ^= 1ULL << (s & 63u);
            if (t < kMaskBits) tg[t >> 6] ^= 1ULL << (t & 63u);
        }
        uint64_t run[kMaskWords];
        uint32_t carry = 0;
        for (uint32_t w = 0; w < kMaskWords; w++) {
            run[w] = denseRunWord(tg[w], carry);
            carry ^= denseParity(tg[w]);
        }
        // per edge
        std::vector<uint8_t> want(kMaskBits, 0);
        for (uint64_t i = 0; i < n; i++) {
            if (mark[i] != ep) continue;
            for (uint64_t e = off[i]; e < off[i + 1]; e++)
                if (e >= base && e < base + cnt) want[e - base] = 1;
        }
        for (uint32_t p = 0; p < kMaskBits; p++) {
            const uint8_t got = static_cast<uint8_t>((run[p >> 6] >> (p & 63u)) & 1u);
            if (got != want[p]) {
                std::fprintf(stderr, "case %d: bit %u is %u, want %u\n", ncase, p, got, want[p]);
                return 1;
            }
        }
        for (uint32_t w = 0; w < kMaskWords; w++) std::printf("%016" PRIx64 "%c", run[w], w + 1 < kMaskWords ? ' ' : '\n');
        ncase++;
    }
    std::fclose(f);
    std::fprintf(stderr, "dense_mask_check: %d cases ok\n", ncase);
    return 0;
}
