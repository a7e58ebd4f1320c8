// tests/cpuwave/frag_check.cpp -- test infrastructure (host build, no GPU).
// bgx_frag.h's host side of the split-fp16 MLP, checked on one weight file:
// the scaling exponent e, every fragment half finite, (hi + lo) 2^-e equal to
// -log2(e) w within 2^-25 2^-e absolute (the fp16 subnormal spacing of the lo
// term) or 2^-21 relative (lo's own rounding), and the fragment index mapping
// back to the right (hidden row, feature) of the v_mfma_f32_32x32x16_f16 A
// operand. Built with -fsanitize=address,undefined: a log2 / int cast of a
// non-finite maximum aborts.
// Usage: frag_check w.bin <e>         the set must be accepted, with this e
//        frag_check w.bin bad:<name>  the set must be rejected, naming <name>
//   w.bin: W1 [128][198], b1 [128], w2 [128], b2 [1] (float32)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bgx_frag.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::vector<float> w(128 * 198 + 128 + 128 + 1);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return 2;
    fclose(f);
    const float* W1 = w.data();
    const float* b1 = W1 + 128 * 198;
    const float* w2 = b1 + 128;
    const float* b2 = w2 + 128;
    bool nonfinite = false;
    int at = -1;
    const char* bad = bgx_frag::unrepresentable(W1, b1, w2, b2, &nonfinite, &at);
    std::vector<uint16_t> frag;
    if (!strncmp(argv[2], "bad:", 4)) {
        if (!bad || strcmp(bad, argv[2] + 4)) {
            printf("{\"error\": \"expected a rejection naming %s, got %s\"}\n", argv[2] + 4, bad ? bad : "none");
            return 1;
        }
        // W1 / b1 outside the limit: build_fragments itself refuses (no log2, no cast)
        const bool wb = !strcmp(bad, "W1") || !strcmp(bad, "b1");
        const int e = bgx_frag::build_fragments(W1, b1, frag);
        if (wb && (e != bgx_frag::kBadWeights || !frag.empty())) {
            printf("{\"error\": \"build_fragments built fragments (e = %d) from rejected weights\"}\n", e);
            return 1;
        }
        printf("{\"rejected\": \"%s\", \"nonfinite\": %d, \"at\": %d}\n", bad, (int)nonfinite, at);
        return 0;
    }
    if (bad) {
        printf("{\"error\": \"rejected (%s[%d])\"}\n", bad, at);
        return 1;
    }
    const int want_e = atoi(argv[2]);
    const int e = bgx_frag::build_fragments(W1, b1, frag);
    if (e != want_e || frag.size() != (size_t)bgx_frag::NFRAG * 8) {
        printf("{\"error\": \"e = %d, expected %d (%zu fragment halves)\"}\n", e, want_e, frag.size());
        return 1;
    }
    const int K = bgx_frag::KSTEPS;
    const double unscale = std::ldexp(1.0, -e);
    const double abs_tol = std::ldexp(1.0, -25) * unscale, rel_tol = std::ldexp(1.0, -21);
    long bad_n = 0, nonfin = 0, rel_cases = 0;
    double worst_abs = 0.0, worst_rel = 0.0;
    std::vector<int> seen(128 * 208, 0);
    auto half_at = [&](int t, int m, int s, int l, int jj) {
        _Float16 h;
        std::memcpy(&h, &frag[((((size_t)t * 4 + m) * K + s) * 64 + l) * 8 + jj], 2);
        return (double)(float)h;
    };
    for (int m = 0; m < 4; ++m)
        for (int s = 0; s < K; ++s)
            for (int l = 0; l < 64; ++l)
                for (int jj = 0; jj < 8; ++jj) {
                    // A operand of the 32x32x16 MFMA: lane l holds hidden row l % 32 of the
                    // m-tile and the 8 consecutive features of k-step s in half l / 32
                    const int row = 32 * m + l % 32, k = 16 * s + 8 * (l / 32) + jj;
                    const double hi = half_at(0, m, s, l, jj), lo = half_at(1, m, s, l, jj);
                    if (!std::isfinite(hi) || !std::isfinite(lo)) {
                        ++nonfin;
                        continue;
                    }
                    double want = 0.0;
                    if (k < 198) {
                        want = (double)W1[row * 198 + k];
                        if (k == 193 || k == 195) want /= 15.0;
                        want *= -bgx_frag::kLog2e;
                    } else if (k == 198) {
                        want = -bgx_frag::kLog2e * (double)b1[row];
                    }
                    ++seen[row * 208 + k];
                    const double err = std::fabs((hi + lo) * unscale - want);
                    if (err > abs_tol) {
                        ++rel_cases;
                        if (err > rel_tol * std::fabs(want)) {
                            if (!bad_n) printf("{\"first_bad\": [%d, %d], \"got\": %.17g, \"want\": %.17g}\n", row, k,
                                               (hi + lo) * unscale, want);
                            ++bad_n;
                        }
                        if (want != 0.0 && err / std::fabs(want) > worst_rel) worst_rel = err / std::fabs(want);
                    } else if (err > worst_abs) {
                        worst_abs = err;
                    }
                }
    long unmapped = 0;
    for (int v : seen) unmapped += v != 1;
    printf("{\"e\": %d, \"nonfinite\": %ld, \"mismatches\": %ld, \"unmapped\": %ld, \"relative_cases\": %ld, "
           "\"worst_abs_over_tol\": %.3g, \"worst_rel_over_tol\": %.3g}\n",
           e, nonfin, bad_n, unmapped, rel_cases, worst_abs / abs_tol, worst_rel / rel_tol);
    return nonfin || bad_n || unmapped ? 1 : 0;
}
