// tests/cpuwave/zs_emu.cpp -- test infrastructure (host build, emulated workgroups).
// The target stage of the batched update with zero-sum targets on the host:
// both instances of tl_target_kernel (bgx_train_lambda.hip) through the
// launcher, against tests/cpuwave/hip/hip_runtime.h with exact-size buffers
// under AddressSanitizer.
// Usage:
//   zs_emu rec.bin offs.bin y.bin gamma lambda zero_sum out.bin
//     rec: n_rec x 12 record words (uint32); offs: n_eps + 1 int32; y: n_rec
//     float32 (V of every record); zero_sum: 0 the plain instance, 1 the zero-sum
//     one; out: tgt (n_rec float32), then target_out (n_rec float32). Both start
//     as 7.0: the launcher zeroes what no episode covers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"

#include "bgx_train_lambda.hip"

template <class T> static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    T x;
    while (fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    std::vector<uint32_t> rec;
    std::vector<int32_t> offs;
    std::vector<float> y;
    if (!read_all(argv[1], rec) || !read_all(argv[2], offs) || !read_all(argv[3], y)) return 2;
    const int n_rec = (int)rec.size() / 12;
    if (n_rec < 1 || rec.size() % 12 || offs.size() < 2 || (int)y.size() != n_rec) return 2;
    const int zs = atoi(argv[6]);
    if (zs != 0 && zs != 1) return 2;
    std::vector<float> tgt(n_rec, 7.0f), out(n_rec, 7.0f);
    bgx::TrainBatchArgs a{};
    a.rec = rec.data();
    a.offs = offs.data();
    a.n_eps = (int)offs.size() - 1;
    a.n_rec = n_rec;
    a.gamma = strtof(argv[4], nullptr);
    a.lambda = strtof(argv[5], nullptr);
    a.zero_sum = zs;
    a.Y = y.data();
    a.tgt = tgt.data();
    a.target_out = out.data();
    if (bgx_launch_lambda_targets(&a, nullptr) != hipSuccess) return 3;
    FILE* f = fopen(argv[7], "wb");
    if (!f) return 2;
    fwrite(tgt.data(), 4, tgt.size(), f);
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
