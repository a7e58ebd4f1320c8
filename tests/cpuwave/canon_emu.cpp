// tests/cpuwave/canon_emu.cpp -- test infrastructure (host build, no GPU).
// The canonical harvest order (csrc/bgx_canon.h) under the wave emulation of
// hip/hip_runtime.h, built with -fsanitize=address,undefined:
//
//   canon_emu hdr.bin rec.bin n m lane_base lanes out [hdr.bin rec.bin n m lane_base lanes out ...]
//     hdr.bin: n headers of 16 uint32, rec.bin: m records of 12 uint32. Runs
//     what bgx_harvest_canonical launches: the index kernel (one workgroup of
//     1,024; the LDS form up to CN_LDS_LANES lanes, as the launcher chooses)
//     and the copy kernel (headers and records, a wave per episode; here at
//     most 3 workgroups, so the waves stride), or for n = 0 the offsets kernel
//     alone. Every input,
//     output and the workspace is allocated at exactly its size (a read or
//     write past one is AddressSanitizer's to report) and the outputs start
//     out filled with a pattern. Writes out.hdr, out.rec and out.offs and
//     prints one JSON line per case with the status word.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bgx_canon.h"

namespace {

void index_lds(const uint32_t* hdr, int n, int m, uint32_t lane_base, int lanes, int32_t* out_offs, uint32_t* status,
               bgx::CanonWork w) {
    bgx::canon_index_body<true>(hdr, n, m, lane_base, lanes, out_offs, status, w);
}
void index_global(const uint32_t* hdr, int n, int m, uint32_t lane_base, int lanes, int32_t* out_offs, uint32_t* status,
                  bgx::CanonWork w) {
    bgx::canon_index_body<false>(hdr, n, m, lane_base, lanes, out_offs, status, w);
}
void copy_kernel(const uint32_t* hdr, const uint32_t* rec, int n, int m, const int32_t* perm, const int32_t* in_offs,
                 const int32_t* out_offs, uint32_t* out_hdr, uint32_t* out_rec) {
    bgx::canon_copy_body(hdr, rec, n, m, perm, in_offs, out_offs, out_hdr, out_rec);
}
void offs_kernel(const uint32_t* hdr, int n, int32_t* offs) { bgx::episode_offsets_body(hdr, n, offs); }

constexpr unsigned char PATTERN = 0xA5;

bool read_words(const char* path, void* dst, size_t words) {
    if (words == 0) return true;
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 4, words, f) == words;
    fclose(f);
    return ok;
}

bool write_bytes(const std::string& path, const void* src, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(src, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

int run_case(char** a) {
    const int n = atoi(a[2]), m = atoi(a[3]), lane_base = atoi(a[4]), lanes = atoi(a[5]);
    const std::string out = a[6];
    if (n < 0 || m < 0 || lane_base < 0 || lanes < 1) return 2;
    // uint4 vectors: 16-byte aligned, exactly n x 64 and m x 48 bytes
    std::vector<uint4> hdr((size_t)n * 4), rec((size_t)m * 3), out_hdr((size_t)n * 4), out_rec((size_t)m * 3);
    std::vector<int32_t> out_offs((size_t)n + 1);
    if (!read_words(a[0], hdr.data(), (size_t)n * 16) || !read_words(a[1], rec.data(), (size_t)m * 12)) return 2;
    if (n > 0) std::memset(out_hdr.data(), PATTERN, out_hdr.size() * 16);
    if (m > 0) std::memset(out_rec.data(), PATTERN, out_rec.size() * 16);
    std::memset(out_offs.data(), PATTERN, out_offs.size() * 4);
    uint32_t status = 0;
    if (n == 0) {
        hipLaunchKernelGGL(offs_kernel, dim3(1), dim3(bgx::PK_OFFS_THREADS), 0, nullptr, (const uint32_t*)nullptr, 0,
                           out_offs.data());
    } else {
        std::vector<uint4> work(bgx::canon_work_bytes(n, lanes) / 16);
        std::memset(work.data(), PATTERN, work.size() * 16);
        const bgx::CanonWork w = bgx::canon_work(work.data(), n, lanes);
        if (lanes <= bgx::CN_LDS_LANES)
            hipLaunchKernelGGL(index_lds, dim3(1), dim3(bgx::CN_INDEX_THREADS), 0, nullptr, (const uint32_t*)hdr.data(), n,
                               m, (uint32_t)lane_base, lanes, out_offs.data(), &status, w);
        else
            hipLaunchKernelGGL(index_global, dim3(1), dim3(bgx::CN_INDEX_THREADS), 0, nullptr,
                               (const uint32_t*)hdr.data(), n, m, (uint32_t)lane_base, lanes, out_offs.data(), &status, w);
        int blocks = (n + 3) / 4;
        blocks = blocks > 3 ? 3 : blocks;
        hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(bgx::CN_COPY_THREADS), 0, nullptr, (const uint32_t*)hdr.data(),
                           (const uint32_t*)rec.data(), n, m, (const int32_t*)w.perm, (const int32_t*)w.in_offs,
                           (const int32_t*)out_offs.data(), (uint32_t*)out_hdr.data(), (uint32_t*)out_rec.data());
    }
    if (!write_bytes(out + ".hdr", out_hdr.data(), out_hdr.size() * 16) ||
        !write_bytes(out + ".rec", out_rec.data(), out_rec.size() * 16) ||
        !write_bytes(out + ".offs", out_offs.data(), out_offs.size() * 4))
        return 2;
    printf("{\"out\": \"%s\", \"n\": %d, \"m\": %d, \"lanes\": %d, \"status\": %u}\n", out.c_str(), n, m, lanes, status);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 8 || (argc - 1) % 7 != 0) return 2;
    for (int i = 1; i + 6 < argc; i += 7)
        if (int rc = run_case(argv + i)) return rc;
    return 0;
}
