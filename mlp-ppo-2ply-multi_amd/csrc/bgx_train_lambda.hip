// bgx_train_lambda.hip — the target stage of the batched TD(lambda) update
// (bgx_tdlambda_update_batched): between the forward and the backward launch of
// bgx_train_batch.hip it turns Y of every record into the lambda-return
//   G_{b-1} = r_{b-1}
//   G_s     = r_s + gamma ((1 - lambda) Y_{s+1} + lambda G_{s+1}),   a <= s < b - 1
// of its episode [a, b), a backward linear recurrence along each episode:
//   G_s = a_s + c G_{s+1},  a_s = r_s + gamma (1 - lambda) Y_{s+1} (r_s on the
//   last record),  c = gamma lambda.
//
// One wave per episode (waves take episodes w, w + W, ...). A wave walks its
// episode from the end in 64-record chunks; lane i of a chunk that ends at
// record `hi` holds record hi - 64 + i, so only the chunk at the episode's start
// is ragged, in its low lanes, which no other lane reads. Per chunk:
//   scan    six steps d = 1, 2, 4, .. 32 of x_i = fma(c^d, x_{i+d}, x_i) (a lane
//           past 63 reads 0): x_i = sum_{j < 64 - i} c^j a_{i+j}
//   carry   x_i = fma(c^(64-i), G_hi, x_i), G_hi = lane 0 of the chunk before
// c^d and c^(64-i) come from c by repeated squaring in a fixed order. Every
// record's G is one fixed fma chain: the same inputs give the same bits on every
// call and on every grid. Nothing episode-sized lives in LDS (no LDS at all), so
// there is no episode-length limit; the stores are plain per-lane stores, no
// atomics. With lambda = 0 (c = 0) the chain is fma(gamma, Y_{s+1}, r_s).
//
// The zero-sum instance (ZS; bgx_td_update_batched with BGX_TDF_ZERO_SUM) takes
// the next record from the opponent's side when the mover changes between the
// two: f_s = m_s ^ m_{s+1} (word 11 bit 9; 0 on an episode's last record), and
//   G_s = r_s + gamma ((1 - lambda) B_s(Y_{s+1}) + lambda B_s(G_{s+1})),
//   B_s(x) = 1 - x on a flip, x otherwise,
// which is G_s = a_s + sigma_s c G_{s+1} with sigma_s = -1 and
// a_s = (r_s + gamma) - gamma (1 - lambda) Y_{s+1} on a flip. With S_i = the
// product of sigma over lanes i .. 63 of the chunk (the parity of a ballot of f
// above the lane), H_i = S_i G_i obeys H_i = S_i a_i + c H_{i+1} and H_64 = G_hi:
// the same scan and the same carry on S_i a_i, and G_i = S_i H_i. Lane 63's flip
// is the one into the chunk before (the record at `end`). The products by +-1
// are exact, so an episode without a flip gets the plain instance's bits.
// c^64 by repeated fp32 squaring is off by +5.4e-7 relative at c = 0.99 (c^32:
// +2.9e-7), the largest share of the stage's error at lambda = 1. The plain
// instance keeps that table (its bits are fixed), and so do the chunks of the
// zero-sum instance that no flip has reached yet, walking from the episode's
// end; from the first flip on, where no plain result exists to agree with, the
// powers are double products rounded once.
//
// No MFMA and nothing but wave shuffles: the host emulation (tests/cpuwave)
// compiles this unit alone.
#include "bgx_device.h"
#include "bgx_kernels.h"

namespace bgx {

constexpr int TL_T = 256;   // threads per workgroup: 4 waves, an episode each at a time

template <bool ZS>
__global__ __launch_bounds__(TL_T) void tl_target_kernel(TrainBatchArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int wave = (int)blockIdx.x * (TL_T / 64) + ((int)threadIdx.x >> 6);
    const int n_waves = (int)gridDim.x * (TL_T / 64);
    const float g1 = a.gamma * (1.0f - a.lambda), c = a.gamma * a.lambda;
    // c^1, c^2, c^4, .. c^64
    float cp[7];
    cp[0] = c;
#pragma unroll
    for (int k = 1; k < 7; ++k) cp[k] = cp[k - 1] * cp[k - 1];
    // c^(64 - lane): the set bits of the exponent, low to high
    float ccarry = 1.0f;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        if (((64 - lane) >> k) & 1) ccarry *= cp[k];
    // ZS: the same powers as double products rounded once (cpx, ccarryx), for the
    // chunks from an episode's first mover change (seen from its end) on
    [[maybe_unused]] float cpx[6];
    [[maybe_unused]] float ccarryx = 1.0f;
    if constexpr (ZS) {
        double cd[7], cc = 1.0;
        cd[0] = (double)c;
#pragma unroll
        for (int k = 1; k < 7; ++k) cd[k] = cd[k - 1] * cd[k - 1];
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (((64 - lane) >> k) & 1) cc *= cd[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) cpx[k] = (float)cd[k];
        ccarryx = (float)cc;
    }

    for (int e = wave; e < a.n_eps; e += n_waves) {
        int lo = a.offs[e], hi = a.offs[e + 1];   // clamped as tb_index_kernel clamps them
        lo = lo < 0 ? 0 : (lo > a.n_rec ? a.n_rec : lo);
        hi = hi < 0 ? 0 : (hi > a.n_rec ? a.n_rec : hi);
        const int last = hi - 1;
        float carry = 0.0f;   // G of the record after the chunk (no carry into an episode's last chunk)
        [[maybe_unused]] bool seen = false;   // ZS: a mover change in this chunk or one nearer the end (wave-uniform)
        for (int end = hi; end > lo; end -= 64) {
            const int s = end - 64 + lane;   // may be negative below lo
            const bool live = s >= lo;
            float x = 0.0f;
            [[maybe_unused]] float sg = 1.0f;   // ZS: S_lane
            if constexpr (ZS) {
                const bool flip = live && s < last &&
                                  (((a.rec[(size_t)s * 12 + 11] ^ a.rec[(size_t)(s + 1) * 12 + 11]) >> 9) & 1u);
                if (live) {
                    x = __int_as_float((int)a.rec[(size_t)s * 12 + 9]);
                    if (flip) x += a.gamma;
                    if (s < last && g1 != 0.0f) x = fmaf(flip ? -g1 : g1, a.Y[s + 1], x);
                }
                const unsigned long long flips = __ballot(flip);
                seen = seen || flips != 0ull;
                if (__popcll(flips >> lane) & 1) sg = -1.0f;   // flips of lanes lane .. 63
                x *= sg;
            } else if (live) {
                x = __int_as_float((int)a.rec[(size_t)s * 12 + 9]);
                if (s < last && g1 != 0.0f) x = fmaf(g1, a.Y[s + 1], x);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int d = 1 << k;
                const float up = __shfl(x, (lane + d) & 63, 64);
                float p = cp[k];
                if constexpr (ZS) p = seen ? cpx[k] : p;
                x = fmaf(p, lane + d < 64 ? up : 0.0f, x);
            }
            if constexpr (ZS) {
                x = fmaf(seen ? ccarryx : ccarry, carry, x);
                x *= sg;
            } else {
                x = fmaf(ccarry, carry, x);
            }
            if (live) {
                a.tgt[s] = x;
                if (a.target_out) a.target_out[s] = x;
            }
            carry = __shfl(x, 0, 64);   // used only when the chunk was full
        }
    }
}

}  // namespace bgx

// args->zero_sum picks the instance
extern "C" hipError_t bgx_launch_lambda_targets(const bgx::TrainBatchArgs* args, hipStream_t stream) {
    using namespace bgx;
    static int n_cu_dev[64];
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || cur < 0 || cur >= 64) cur = 0;
    int& n_cu = n_cu_dev[cur];
    if (!n_cu && (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, cur) != hipSuccess || n_cu <= 0))
        n_cu = 256;
    const TrainBatchArgs& a = *args;
    // records in no episode keep target 0
    hipError_t e = hipMemsetAsync(a.tgt, 0, (size_t)a.n_rec * sizeof(float), stream);
    if (e == hipSuccess && a.target_out) e = hipMemsetAsync(a.target_out, 0, (size_t)a.n_rec * sizeof(float), stream);
    if (e != hipSuccess) return e;
    // 8 workgroups (32 waves) a CU: the waves wait on one gather of 64 reward words a chunk
    int blocks = (a.n_eps + TL_T / 64 - 1) / (TL_T / 64);
    if (blocks > 8 * n_cu) blocks = 8 * n_cu;
    if (a.zero_sum) hipLaunchKernelGGL(tl_target_kernel<true>, dim3(blocks), dim3(TL_T), 0, stream, a);
    else hipLaunchKernelGGL(tl_target_kernel<false>, dim3(blocks), dim3(TL_T), 0, stream, a);
    return hipGetLastError();
}
