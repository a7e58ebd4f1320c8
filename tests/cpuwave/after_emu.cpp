// tests/cpuwave/after_emu.cpp -- test infrastructure (host build, emulated workgroups).
// The afterstate rows of the batched update (bgx_td_afterstate_update_batched) on
// the host: the index launch's afterstate form (tb_index<true>), the staging of a
// tile's source indices into LDS (tb_stage_src) and the tile loader
// (tb_load_tile_after), all from csrc/bgx_train_tile.h, in the order the forward
// and backward kernels run them, against tests/cpuwave/hip/hip_runtime.h with
// exact-size rec, hdr, offs and workspace buffers under AddressSanitizer. Only
// index, staging and loader are emulated: the forward
// and backward kernels around them (csrc/bgx_train_batch.hip) are f32-input MFMA
// code on ext_vector_type registers, which this g++ build does not provide; they
// are the code the GPU tests compare bit for bit with the existing call.
// Usage:
//   after_emu rec.bin hdr.bin offs.bin out.bin
//     rec: n_rec x 12 record words (uint32); hdr: n_eps x 16 header words
//     (uint32); offs: n_eps + 1 int32; out: srcidx (n_rec int32), then every
//     tile's LDS rows as the loader leaves them (n_tiles x 128 x 8 uint32).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "hip/hip_runtime.h"

#include "bgx_train_tile.h"

namespace {

// exactly n elements on the heap: one element past either end is a sanitizer report
template <class T> struct Buf {
    std::unique_ptr<T[]> p;
    size_t n = 0;
};

template <class T> bool read_all(const char* path, Buf<T>& b) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) {
        fclose(f);
        return false;
    }
    b.n = (size_t)bytes / sizeof(T);
    b.p.reset(new T[b.n]);
    const bool ok = fread(b.p.get(), sizeof(T), b.n, f) == b.n;
    fclose(f);
    return ok;
}

void index_kernel(bgx::TrainBatchArgs a) { bgx::tb_index<true>(a); }

// workgroup g takes tiles g, g + G, ... as the forward and backward launches do:
// the first tile's source indices are requested before the loop, the next
// tile's once this tile's rows are in
void load_kernel(bgx::TrainBatchArgs a, uint32_t* rows) {
    __shared__ uint32_t RW[bgx::TB_TILE][8];
    __shared__ int32_t SRC[bgx::TB_TILE];
    bgx::tb_stage_src(a.srcidx, a.n_rec, (long long)blockIdx.x * bgx::TB_TILE, SRC);
    for (int tile = (int)blockIdx.x; tile < a.n_tiles; tile += (int)gridDim.x) {
        const long long base = (long long)tile * bgx::TB_TILE;
        __builtin_amdgcn_s_waitcnt(0xF70);
        __syncthreads();
        bgx::tb_load_tile_after(a.rec, a.hdr, SRC, a.n_rec, base, RW);
        __syncthreads();
        bgx::tb_stage_src(a.srcidx, a.n_rec, base + (long long)gridDim.x * bgx::TB_TILE, SRC);
        for (int idx = (int)threadIdx.x; idx < bgx::TB_TILE * 8; idx += bgx::TB_T)
            rows[(size_t)base * 8 + idx] = RW[idx >> 3][idx & 7];
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    Buf<uint32_t> rec, hdr;
    Buf<int32_t> offs;
    if (!read_all(argv[1], rec) || !read_all(argv[2], hdr) || !read_all(argv[3], offs)) return 2;
    if (rec.n < 12 || rec.n % 12 || hdr.n % 16 || offs.n < 2 || hdr.n / 16 != offs.n - 1) return 2;
    const int n_rec = (int)(rec.n / 12), n_eps = (int)offs.n - 1;
    const int n_tiles = (n_rec + bgx::TB_TILE - 1) / bgx::TB_TILE;
    std::unique_ptr<int32_t[]> info(new int32_t[n_rec]), srcidx(new int32_t[n_rec]);
    std::unique_ptr<uint32_t[]> rows(new uint32_t[(size_t)n_tiles * bgx::TB_TILE * 8]);
    int step = 0;
    // the launcher's fills: a record in no episode keeps 0 in both
    hipMemsetAsync(info.get(), 0, (size_t)n_rec * sizeof(int32_t), nullptr);
    hipMemsetAsync(srcidx.get(), 0, (size_t)n_rec * sizeof(int32_t), nullptr);
    memset(rows.get(), 0xEE, (size_t)n_tiles * bgx::TB_TILE * 8 * sizeof(uint32_t));
    bgx::TrainBatchArgs a{};
    a.rec = rec.p.get();
    a.offs = offs.p.get();
    a.n_eps = n_eps;
    a.n_rec = n_rec;
    a.step = &step;
    a.info = info.get();
    a.hdr = hdr.p.get();
    a.srcidx = srcidx.get();
    a.n_tiles = n_tiles;
    const int grid = n_tiles < 2 ? n_tiles : 2;   // two workgroups: with three tiles one of them takes two
    hipLaunchKernelGGL(index_kernel, dim3((n_eps + bgx::TB_T - 1) / bgx::TB_T), dim3(bgx::TB_T), 0, nullptr, a);
    hipLaunchKernelGGL(load_kernel, dim3(grid), dim3(bgx::TB_T), 0, nullptr, a, rows.get());
    if (step != 1) return 3;
    FILE* f = fopen(argv[4], "wb");
    if (!f) return 2;
    fwrite(srcidx.get(), 4, (size_t)n_rec, f);
    fwrite(rows.get(), 4, (size_t)n_tiles * bgx::TB_TILE * 8, f);
    fclose(f);
    return 0;
}
