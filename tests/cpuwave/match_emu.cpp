// tests/cpuwave/match_emu.cpp -- test infrastructure (host build, emulated workgroups).
// The match mode's routed MLP launch as bgx_value_boards_routed issues it
// (bgx_match.hip: route_ids_kernel sorts the rows into one index list per
// network, mlp_kernel_routed evaluates list n under network n), on the host:
// the kernels' source (a copy with the dynamic LDS array bound to the emulated
// workgroup's buffer) against tests/cpuwave/hip/hip_runtime.h, with exact-size
// buffers under AddressSanitizer.
// Usage: match_emu rows.bin w0.bin w1.bin ids.bin nt out.bin
//   rows: n x 8 packed words (uint32); w0 / w1: W1 [128][198], b1 [128],
//   w2 [128], b2 [1] (float32) of network 0 / 1; ids: n bytes in {0, 1};
//   nt 1 or 2 (the single-tile and the two-tile form); out: n float32 V
//   (-12345 where the launch stored nothing)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bgx_frag.h"
#include "bgx_match.hip"

static_assert(bgx_frag::NFRAG == bgx::NFRAG, "fragment count");

struct Net {
    std::vector<float> w;
    std::vector<uint16_t> frag;
    float fs = 1.0f;
    bool load(const char* path) {
        w.resize(128 * 198 + 128 + 128 + 1);
        FILE* f = fopen(path, "rb");
        if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return false;
        fclose(f);
        const int e = bgx_frag::build_fragments(w.data(), w.data() + 128 * 198, frag);
        fs = (float)std::ldexp(1.0, -e);
        return true;
    }
    const float* w2() const { return w.data() + 128 * 198 + 128; }
};

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    std::vector<uint32_t> rows;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        uint32_t v[8];
        while (fread(v, 4, 8, f) == 8) rows.insert(rows.end(), v, v + 8);
        fclose(f);
    }
    const int n = (int)rows.size() / 8;
    Net nets[2];
    if (!nets[0].load(argv[2]) || !nets[1].load(argv[3])) return 2;
    std::vector<uint8_t> ids(n);
    {
        FILE* f = fopen(argv[4], "rb");
        if (!f || fread(ids.data(), 1, ids.size(), f) != ids.size()) return 2;
        fclose(f);
    }
    std::vector<float> out(n, -12345.0f);
    std::vector<int32_t> list0(n, -1), list1(n, -1);
    std::vector<unsigned> ctr(4, 0u);
    if (bgx_launch_route_ids(ids.data(), n, list0.data(), list1.data(), ctr.data(), nullptr) != hipSuccess) return 3;
    int want[2] = {0, 0};
    for (int i = 0; i < n; ++i) ++want[ids[i] & 1];
    if ((int)ctr[0] != want[0] || (int)ctr[1] != want[1]) return 4;
    bgx::MatchMlpArgs m{};
    m.rows = rows.data();
    m.out = out.data();
    m.n_max = n;
    m.list_cap = n;
    m.nt = atoi(argv[5]);
    m.n_hint = n;
    m.list[0] = list0.data();
    m.list[1] = list1.data();
    for (int k = 0; k < 2; ++k) {
        m.count[k] = ctr.data() + k;
        m.claim[k] = ctr.data() + 2 + k;
        m.wfrag[k] = (const uint4*)nets[k].frag.data();
        m.rowc[k] = nets[k].w2();
        m.b2[k] = nets[k].w2()[128];
        m.feat_scale[k] = nets[k].fs;
    }
    if (bgx_launch_mlp_routed(&m, nullptr) != hipSuccess) return 3;
    FILE* f = fopen(argv[6], "wb");
    if (!f) return 2;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
