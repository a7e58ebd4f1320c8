// tests/cpuwave/feature_emu.cpp -- test infrastructure (host build).
// The batched trainer's live-feature rule (csrc/bgx_train_tile.h) on the host,
// both ways it is read: composed per feature (tb_feature) and as the backward
// kernel reads it, a field locator per feature (tb_field) kept in registers
// and a [224][16] field value -> feature value table (tb_lut_entry). The two must
// agree bit for bit on every feature slot 0..223 (198..223 are padding: zero);
// the 198 live ones are written out. The rows sit in an exact-size buffer under
// AddressSanitizer: a locator that reads word 7 of the last row is a report.
// Usage:
//   feature_emu rows.bin out.bin
//     rows: n x 7 packed words (uint32); out: n x 198 features (float32).
#include <cstdio>
#include <cstring>
#include <memory>

#include "hip/hip_runtime.h"

#include "bgx_train_tile.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % 28) return 2;
    const size_t n = (size_t)bytes / 28;
    std::unique_ptr<uint32_t[]> rows(new uint32_t[n * 7]);
    if (fread(rows.get(), 4, n * 7, f) != n * 7) return 2;
    fclose(f);

    static float LUT[224][16];
    bgx::TbField fd[224];
    for (int k = 0; k < 224; ++k) {
        fd[k] = bgx::tb_field(k);
        for (int v = 0; v < 16; ++v) LUT[k][v] = bgx::tb_lut_entry(k, v);
    }
    std::unique_ptr<float[]> out(new float[n * 198]);
    for (size_t r = 0; r < n; ++r) {
        const uint32_t* w = rows.get() + r * 7;
        for (int k = 0; k < 224; ++k) {
            const float a = bgx::tb_feature(w, k);
            const float b = LUT[k][(w[fd[k].word] >> fd[k].shift) & (uint32_t)fd[k].mask];
            if (memcmp(&a, &b, 4) != 0) return 3;
            if (k < 198) out[r * 198 + k] = a;
            else if (a != 0.0f) return 3;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.get(), 4, n * 198, f);
    fclose(f);
    return 0;
}
