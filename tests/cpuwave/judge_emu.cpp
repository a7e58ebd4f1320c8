// tests/cpuwave/judge_emu.cpp -- test infrastructure (host build).
// judge() (bgx_engine.h: the env step's reward, done flag, win type and the
// close-out / prime shaping rewards with their once-per-player flag bits) on
// the host, as the kernels compile it, against tests/cpuwave/hip/hip_runtime.h
// under AddressSanitizer.
// Usage:
//   judge_emu in.bin out.bin
//     in:  n x 10 uint32: a packed board row (8 words), the mover, the lane's
//          flag word before the step
//     out: n x 6 uint32: the reward's bits, done, win_type, close, prime, the
//          flag word after the step
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"
// what bgx_engine.h uses beyond the emulation header
#define __constant__
#define __expf(x) std::exp((float)(x))
inline uint32_t __float_as_uint(float f) { uint32_t v; std::memcpy(&v, &f, 4); return v; }

#include "bgx_engine.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> in;
    uint32_t x;
    while (fread(&x, 4, 1, f) == 1) in.push_back(x);
    fclose(f);
    if (in.empty() || in.size() % 10) return 2;
    const size_t n = in.size() / 10;
    std::vector<uint32_t> out(n * 6);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[8];   // exactly a row: a read past word 7 is an ASan report
        std::memcpy(w, &in[i * 10], sizeof w);
        const int pl = (int)in[i * 10 + 8];
        if (pl != 0 && pl != 1) return 2;
        uint32_t flags = in[i * 10 + 9];
        const bgx::Outcome o = bgx::judge(w, pl, flags);
        uint32_t* q = &out[i * 6];
        q[0] = __float_as_uint(o.reward);
        q[1] = (uint32_t)o.done;
        q[2] = (uint32_t)o.win_type;
        q[3] = (uint32_t)o.close;
        q[4] = (uint32_t)o.prime;
        q[5] = flags;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
