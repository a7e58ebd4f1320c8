// bgx_pack.hip — the learner's device-side hand-offs (bodies and contracts in
// bgx_pack.h): the check and pack launches of bgx_set_weights_device and the
// episode-offsets launch of bgx_episode_offsets.
#include "bgx_pack.h"

namespace bgx {

__global__ __launch_bounds__(PK_CHECK_THREADS) void weights_check_kernel(const float* __restrict__ p,
                                                                         PackInfo* __restrict__ info) {
    pack_check_body(p, info);
}

__global__ __launch_bounds__(PK_PACK_THREADS) void weights_pack_kernel(const float* __restrict__ p,
                                                                       const PackInfo* __restrict__ info,
                                                                       uint4* __restrict__ frag, float* __restrict__ W1,
                                                                       float* __restrict__ b1, float* __restrict__ w2,
                                                                       float* __restrict__ rowc) {
    pack_frag_body(p, info, frag, W1, b1, w2, rowc);
}

__global__ __launch_bounds__(PK_OFFS_THREADS) void episode_offsets_kernel(const uint32_t* __restrict__ hdr, int n,
                                                                          int32_t* __restrict__ offs) {
    episode_offsets_body(hdr, n, offs);
}

}  // namespace bgx

extern "C" hipError_t bgx_launch_weights_check(const float* params, bgx::PackInfo* info, hipStream_t stream) {
    hipLaunchKernelGGL(bgx::weights_check_kernel, dim3(1), dim3(bgx::PK_CHECK_THREADS), 0, stream, params, info);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_weights_pack(const float* params, const bgx::PackInfo* info, uint4* frag, float* W1,
                                              float* b1, float* w2, float* rowc, hipStream_t stream) {
    constexpr int blocks = (bgx::PK_PACK_ITEMS + bgx::PK_PACK_THREADS - 1) / bgx::PK_PACK_THREADS;
    hipLaunchKernelGGL(bgx::weights_pack_kernel, dim3(blocks), dim3(bgx::PK_PACK_THREADS), 0, stream, params, info,
                       frag, W1, b1, w2, rowc);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_episode_offsets(const uint32_t* headers, int n, int32_t* offs, hipStream_t stream) {
    hipLaunchKernelGGL(bgx::episode_offsets_kernel, dim3(1), dim3(bgx::PK_OFFS_THREADS), 0, stream, headers,
                       n < 0 ? 0 : n, offs);
    return hipGetLastError();
}
