// tests/cpuwave/pack_emu.cpp -- test infrastructure (host build, no GPU).
// The learner's device-side hand-offs (csrc/bgx_pack.h) under the wave
// emulation of hip/hip_runtime.h, built with -fsanitize=address,undefined:
//
//   pack_emu pack w.bin [w.bin ...]
//     each file: 25,601 float32 in the trainer's flat order (W1 [128][198], b1,
//     w2, b2: tests/value_cases.py write_weights). Runs the check kernel (one
//     workgroup of 1,024) and the pack kernel (13 workgroups of 256) on output
//     buffers filled with a pattern, and bgx_frag.h's unrepresentable /
//     build_fragments on the same floats. One JSON line per file: the host's
//     verdict (rule, flat index, e), the kernels' (rule, index, e, b2 bits),
//     whether the fragments equal build_fragments' byte for byte, whether the
//     fp32 copies equal the input, and whether every output byte still holds
//     the pattern.
//
//   pack_emu offs hdr.bin n out.bin [hdr.bin n out.bin ...]
//     hdr.bin: n headers of 16 uint32; out.bin receives the n + 1 int32 offsets
//     of the offsets kernel (one workgroup of 1,024), written into a buffer of
//     exactly that size.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bgx_frag.h"
#include "bgx_pack.h"

namespace {

void check_kernel(const float* p, bgx::PackInfo* info) { bgx::pack_check_body(p, info); }
void pack_kernel(const float* p, const bgx::PackInfo* info, uint4* frag, float* W1, float* b1, float* w2, float* rowc) {
    bgx::pack_frag_body(p, info, frag, W1, b1, w2, rowc);
}
void offs_kernel(const uint32_t* hdr, int n, int32_t* offs) { bgx::episode_offsets_body(hdr, n, offs); }

constexpr unsigned char PATTERN = 0xA5;

template <class T>
bool all_pattern(const std::vector<T>& v) {
    const unsigned char* b = (const unsigned char*)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); ++i)
        if (b[i] != PATTERN) return false;
    return true;
}

int run_pack(const char* path) {
    std::vector<float> w(bgx::PK_PARAMS);
    FILE* f = fopen(path, "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return 2;
    fclose(f);
    const float* W1 = w.data();
    const float* b1 = W1 + bgx::PK_B1;
    const float* w2 = W1 + bgx::PK_W2;
    const float* b2 = W1 + bgx::PK_B2;
    // the host's verdict
    bool nonfinite = false;
    int at = -1;
    const char* bad = bgx_frag::unrepresentable(W1, b1, w2, b2, &nonfinite, &at);
    int host_rule = 0, host_index = 0, host_e = 0;
    std::vector<uint16_t> want;
    if (bad) {
        host_rule = nonfinite ? bgx::PK_RULE_NONFINITE : bgx::PK_RULE_LIMIT;
        host_index = at + (!strcmp(bad, "W1") ? 0 : !strcmp(bad, "b1") ? bgx::PK_B1 : !strcmp(bad, "w2") ? bgx::PK_W2 : bgx::PK_B2);
    } else {
        host_e = bgx_frag::build_fragments(W1, b1, want);
    }
    // the kernels'
    std::vector<uint4> frag(bgx::PK_NFRAG);
    std::vector<float> oW1(bgx::PK_W1), ob1(128), ow2(128), orowc(128);
    std::memset(frag.data(), PATTERN, frag.size() * sizeof(uint4));
    std::memset(oW1.data(), PATTERN, oW1.size() * 4);
    std::memset(ob1.data(), PATTERN, 128 * 4);
    std::memset(ow2.data(), PATTERN, 128 * 4);
    std::memset(orowc.data(), PATTERN, 128 * 4);
    bgx::PackInfo info;
    std::memset(&info, PATTERN, sizeof(info));
    hipLaunchKernelGGL(check_kernel, dim3(1), dim3(bgx::PK_CHECK_THREADS), 0, nullptr, (const float*)w.data(), &info);
    const int blocks = (bgx::PK_PACK_ITEMS + bgx::PK_PACK_THREADS - 1) / bgx::PK_PACK_THREADS;
    hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(bgx::PK_PACK_THREADS), 0, nullptr, (const float*)w.data(),
                       (const bgx::PackInfo*)&info, frag.data(), oW1.data(), ob1.data(), ow2.data(), orowc.data());
    const bool untouched = all_pattern(frag) && all_pattern(oW1) && all_pattern(ob1) && all_pattern(ow2) && all_pattern(orowc);
    const bool frag_equal = !bad && want.size() * 2 == frag.size() * sizeof(uint4) &&
                            !std::memcmp(want.data(), frag.data(), want.size() * 2);
    const bool copies_equal = !std::memcmp(oW1.data(), W1, bgx::PK_W1 * 4) && !std::memcmp(ob1.data(), b1, 128 * 4) &&
                              !std::memcmp(ow2.data(), w2, 128 * 4) && !std::memcmp(orowc.data(), w2, 128 * 4);
    uint32_t b2_bits;
    std::memcpy(&b2_bits, b2, 4);
    // the lo halves that are fp16 subnormals (exponent field 0, mantissa not 0)
    long lo_subnormal = 0;
    if (frag_equal) {
        const uint16_t* h = (const uint16_t*)frag.data() + (size_t)bgx::PK_NFRAG * 4;
        for (size_t i = 0; i < (size_t)bgx::PK_NFRAG * 4; ++i) lo_subnormal += (h[i] & 0x7C00u) == 0 && (h[i] & 0x03FFu) != 0;
    }
    printf("{\"file\": \"%s\", \"host_rule\": %d, \"host_index\": %d, \"host_e\": %d, \"rule\": %u, \"index\": %d, "
           "\"e\": %d, \"b2_ok\": %s, \"frag_equal\": %s, \"copies_equal\": %s, \"untouched\": %s, \"lo_subnormal\": %ld}\n",
           path, host_rule, host_index, host_e, info.rule, info.index, info.e, info.b2_bits == b2_bits ? "true" : "false",
           frag_equal ? "true" : "false", copies_equal ? "true" : "false", untouched ? "true" : "false", lo_subnormal);
    return 0;
}

int run_offs(const char* hdr_path, int n, const char* out_path) {
    std::vector<uint32_t> hdr((size_t)n * 16);
    if (n > 0) {
        FILE* f = fopen(hdr_path, "rb");
        if (!f || fread(hdr.data(), 4, hdr.size(), f) != hdr.size()) return 2;
        fclose(f);
    }
    // exactly n + 1 offsets (a write past them is AddressSanitizer's to report) ...
    std::vector<int32_t> offs((size_t)n + 1);
    std::memset(offs.data(), PATTERN, offs.size() * 4);
    hipLaunchKernelGGL(offs_kernel, dim3(1), dim3(bgx::PK_OFFS_THREADS), 0, nullptr, (const uint32_t*)hdr.data(), n,
                       offs.data());
    FILE* o = fopen(out_path, "wb");
    if (!o || fwrite(offs.data(), 4, offs.size(), o) != offs.size()) return 2;
    fclose(o);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "pack")) {
        for (int i = 2; i < argc; ++i)
            if (int rc = run_pack(argv[i])) return rc;
        return 0;
    }
    if (!strcmp(argv[1], "offs")) {
        if ((argc - 2) % 3 != 0) return 2;
        for (int i = 2; i + 2 < argc; i += 3)
            if (int rc = run_offs(argv[i], atoi(argv[i + 1]), argv[i + 2])) return rc;
        return 0;
    }
    return 2;
}
