// tests/cpuwave/rollout_emu.cpp -- test infrastructure (host build, emulated workgroups).
// The rollout mode's device code on the host: rollout_tally_kernel
// (bgx_rollout.hip) through its launcher, and engine_reset_kernel
// (bgx_engine.hip) with a start table (start_game, bgx_engine.h), against
// tests/cpuwave/hip/hip_runtime.h with exact-size buffers under
// AddressSanitizer.
// Usage:
//   rollout_emu tally hdr.bin sp.bin n_pos max_ep1 max_ep2 out.bin
//     hdr: n x 16 header words (uint32; an empty file: the launcher alone);
//     sp: n_pos start-player bytes; two accumulating calls over all headers,
//     with max_episode = max_ep1, then max_ep2; out: n_pos x 8 uint64 counts
//   rollout_emu reset tab.bin L lane_base strat_stride seed out.bin
//     tab: n_pos x 8 start-table words (EngineDev::start_tab); out: rows
//     (L x 8 uint32), then per lane player, dice0, dice1, 0 (4 bytes), then
//     the lanes' Philox counters (L x uint64)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"
// what bgx_engine.h / bgx_engine.hip use beyond the emulation header
#define __constant__
#define __expf(x) std::exp((float)(x))
inline uint32_t __float_as_uint(float f) { uint32_t v; std::memcpy(&v, &f, 4); return v; }
template <class T> inline T atomicExch(T* p, std::type_identity_t<T> v) { return __atomic_exchange_n(p, v, __ATOMIC_SEQ_CST); }

#include "bgx_engine.hip"
#include "bgx_rollout.hip"

template <class T> static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    T x;
    while (fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

static int run_tally(char** a) {
    std::vector<uint32_t> hdr;
    std::vector<uint8_t> sp;
    if (!read_all(a[2], hdr) || !read_all(a[3], sp)) return 2;
    const int n = (int)hdr.size() / bgx::EP_WORDS, n_pos = atoi(a[4]);
    if ((int)sp.size() != n_pos) return 2;
    std::vector<unsigned long long> counts((size_t)n_pos * 8, 0ull);
    for (int k = 0; k < 2; ++k)
        if (bgx_launch_rollout_tally(n ? hdr.data() : nullptr, n, sp.data(), n_pos, (uint32_t)strtoul(a[5 + k], nullptr, 10),
                                     counts.data(), nullptr) != hipSuccess)
            return 3;
    FILE* f = fopen(a[7], "wb");
    if (!f) return 2;
    fwrite(counts.data(), 8, counts.size(), f);
    fclose(f);
    return 0;
}

static int run_reset(char** a) {
    std::vector<uint32_t> tab;
    if (!read_all(a[2], tab) || tab.empty() || tab.size() % 8) return 2;
    const int L = atoi(a[3]);
    std::vector<uint32_t> rows((size_t)L * 8, 0xDEADBEEFu), flags(L, 7u), epi(L, 7u), rec(L, 7u), first(L, 7u), harv(L, 7u);
    std::vector<uint8_t> player(L, 9), dice(2 * (size_t)L, 9);
    std::vector<int32_t> step(L, 7);
    std::vector<uint64_t> rng(L, 77ull);
    unsigned err = 0;
    bgx::EngineDev e{};
    e.L = L;
    e.lane_base = atoi(a[4]);
    e.seed = strtoull(a[6], nullptr, 10);
    e.rows = rows.data();
    e.player = player.data();
    e.dice = dice.data();
    e.step = step.data();
    e.flags = flags.data();
    e.epi = epi.data();
    e.rng = rng.data();
    e.rec_count = rec.data();
    e.ep_first = first.data();
    e.harv = harv.data();
    e.err_flags = &err;
    e.start_tab = tab.data();
    e.n_pos = (int)tab.size() / 8;
    e.strat_stride = (uint32_t)strtoul(a[5], nullptr, 10);
    if (bgx_launch_engine_reset(&e, nullptr) != hipSuccess) return 3;
    for (int i = 0; i < L; ++i)
        if (step[i] || flags[i] || epi[i] || rec[i] || first[i] || harv[i]) return 4;
    if (err) return 5;
    FILE* f = fopen(a[7], "wb");
    if (!f) return 2;
    fwrite(rows.data(), 4, rows.size(), f);
    for (int i = 0; i < L; ++i) {
        const uint8_t q[4] = {player[i], dice[2 * i], dice[2 * i + 1], 0};
        fwrite(q, 1, 4, f);
    }
    fwrite(rng.data(), 8, rng.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 8 && !strcmp(argv[1], "tally")) return run_tally(argv);
    if (argc == 8 && !strcmp(argv[1], "reset")) return run_reset(argv);
    return 2;
}
