// bgx_canon.hip — the two launches of bgx_harvest_canonical (bodies and
// contracts in bgx_canon.h): the index launch, one workgroup, and the copy of
// headers and records, a wave per episode.
#include "bgx_canon.h"

namespace bgx {

template <bool LDS>
__global__ __launch_bounds__(CN_INDEX_THREADS) void canon_index_kernel(const uint32_t* __restrict__ hdr, int n,
                                                                       int n_records, uint32_t lane_base, int lanes,
                                                                       int32_t* out_offs, uint32_t* status,
                                                                       CanonWork w) {
    canon_index_body<LDS>(hdr, n, n_records, lane_base, lanes, out_offs, status, w);
}

__global__ __launch_bounds__(CN_COPY_THREADS) void canon_copy_kernel(const uint32_t* __restrict__ hdr,
                                                                     const uint32_t* __restrict__ rec, int n,
                                                                     int n_records, const int32_t* __restrict__ perm,
                                                                     const int32_t* __restrict__ in_offs,
                                                                     const int32_t* __restrict__ out_offs,
                                                                     uint32_t* __restrict__ out_hdr,
                                                                     uint32_t* __restrict__ out_rec) {
    canon_copy_body(hdr, rec, n, n_records, perm, in_offs, out_offs, out_hdr, out_rec);
}

}  // namespace bgx

extern "C" hipError_t bgx_launch_canon_index(const uint32_t* headers, int n, int n_records, uint32_t lane_base,
                                             int lanes, int32_t* out_offs, uint32_t* status, bgx::CanonWork w,
                                             hipStream_t stream) {
    if (lanes <= bgx::CN_LDS_LANES)
        hipLaunchKernelGGL(bgx::canon_index_kernel<true>, dim3(1), dim3(bgx::CN_INDEX_THREADS), 0, stream, headers, n,
                           n_records, lane_base, lanes, out_offs, status, w);
    else
        hipLaunchKernelGGL(bgx::canon_index_kernel<false>, dim3(1), dim3(bgx::CN_INDEX_THREADS), 0, stream, headers, n,
                           n_records, lane_base, lanes, out_offs, status, w);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_canon_copy(const uint32_t* headers, const uint32_t* records, int n, int n_records,
                                            bgx::CanonWork w, const int32_t* out_offs, uint32_t* out_headers,
                                            uint32_t* out_records, hipStream_t stream) {
    constexpr int per_block = bgx::CN_COPY_THREADS / 64;
    int blocks = (n + per_block - 1) / per_block;
    blocks = blocks > bgx::CN_COPY_MAX_BLOCKS ? bgx::CN_COPY_MAX_BLOCKS : blocks;
    if (blocks < 1) return hipSuccess;
    hipLaunchKernelGGL(bgx::canon_copy_kernel, dim3(blocks), dim3(bgx::CN_COPY_THREADS), 0, stream, headers, records, n,
                       n_records, (const int32_t*)w.perm, (const int32_t*)w.in_offs, out_offs, out_headers,
                       out_records);
    return hipGetLastError();
}
