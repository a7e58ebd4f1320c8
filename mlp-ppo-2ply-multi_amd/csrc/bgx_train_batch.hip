// bgx_train_batch.hip — the batched TD update (DeviceTrainer batched=True) on
// the whole GPU: ONE Adam step per call on the mean of the per-episode losses,
//   loss = (1/E) sum_e (1/T_e) sum_s (Y_s - tgt_s)^2,
//   tgt_s = r_s + gamma Y_{s+1} (detached; r_s alone on an episode's last record),
// where bgx_train.hip walks the episodes one after another in one workgroup.
//
// One launcher (bgx_launch_td_batched) and one argument struct (TrainBatchArgs)
// serve the four entry points: the TD(0) update below and its three options.
// Five launches on the caller's stream, no host synchronisation:
//   index     one thread per episode: info[s] = T_e | last << 31 for its records
//             (offs clamped to [0, n_records]; a record in no episode keeps 0 and
//             takes no part), and the Adam step count + 1
//   forward   Y[s] = V(x_s) for every record (a target needs the next record's Y,
//             which may sit in another tile or workgroup)
//   backward  workgroup g takes the 128-record tiles g, g + G, ...: recomputes
//             S = sigmoid(W1 x + b1) with the forward launch's code, forms
//             d_s = 2 (Y_s - tgt_s) / (E T_e), dh = ((d w2)(1 - S)) S, and keeps
//             dW1 += dh^T X, db1, dw2, db2 in registers across all its tiles;
//             then one store of its partial gradient (25,601 fp32) into its row
//   reduce    gradient = the partial rows summed in workgroup order; per-block
//             sums of squares (double)
//   adam      norm, clip coefficient and the Adam step over the parameters
// Every sum has a fixed order (no float atomics): the same inputs give the same
// bits on every call.
// The options:
//   TrainBatchArgs::tgt (bgx_tdlambda_update_batched): the lambda-return as the
//   target. The target stage of bgx_train_lambda.hip runs between forward and
//   backward, and the backward launch reads tgt[s] (its LAM instance).
//   TrainBatchArgs::zero_sum (bgx_td_update_batched with BGX_TDF_ZERO_SUM): the
//   stage's zero-sum instance, at every lambda.
//   TrainBatchArgs::hdr / srcidx (bgx_td_afterstate_update_batched): afterstate
//   rows, the AFTER instances of the index, forward and backward kernels (below).
//
// Both GEMMs run on the f32-input MFMA (v_mfma_f32_32x32x2_f32: an exact k-ordered
// fp32 fma chain, so no weight scaling and no dh underflow). A workgroup is 4
// waves; wave w owns hidden units [32 w, 32 w + 32):
//   forward   H[record][unit] = sum_k X[record][k] W1[unit][k]: A = the features
//             of record 32 c + (lane & 31), built in registers from the lane's
//             packed words (k = 2 s + (lane >> 5)), B = the wave's W1 slice, 99
//             registers per lane loaded once per launch; one accumulator tile per
//             32-record chunk c, initialised with b1
//   backward  dW1[unit][k] = sum_record dh[record][unit] X[record][k]: the forward
//             result has the unit on the lane and the records in its 16 registers,
//             so register t of chunk c IS the A operand of a k-step over the two
//             records 32 c + row(t, lane half) with no lane movement and no LDS;
//             B = the feature nt * 32 + (lane & 31) of those two records, from
//             the tile's packed words (the feature's field, tb_field) and a [224][16]
//             field value -> feature value table in LDS (tb_lut_entry; rows of 17 words).
//             7 accumulator tiles (224 >= 198 features) per wave.
// Nothing episode-sized lives in LDS: no episode-length limit.
//
// Afterstate rows: V is fitted on the board each mover leaves, under the mover's
// indicator, the positions the engine rates. The index, forward and backward
// kernels are templates on AFTER; with it the index launch also writes where
// each record's row comes from (the next record, or the episode header's final
// board) and the forward and backward launches load those rows
// (bgx_train_tile.h). Nothing else differs: everything downstream of the loader
// is the same code, and the backward launch always reads the target stage's G.
#include "bgx_device.h"
#include "bgx_kernels.h"
#include "bgx_train_tile.h"

namespace bgx {

namespace {

constexpr int TB_C = TB_TILE / 32;                 // 32-record chunks per tile
constexpr int TB_KS = 99;                          // forward k-steps (198 features, 2 per step)
constexpr int TB_NT = 7;                           // backward feature tiles of 32
constexpr int TB_LUTW = 17;                        // words per row of the nibble -> feature value table
constexpr int TB_NW1 = 128 * 198;
constexpr int TB_NP = TRAIN_BATCH_PARAMS;
constexpr int TB_PS = TRAIN_BATCH_PSTRIDE;
constexpr int TB_NB = (TB_NP + TB_T - 1) / TB_T;   // blocks of the reduce / adam launches
static_assert(TB_NB <= TRAIN_BATCH_SQ, "sum-of-squares slots");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// features 2 S (lane half 0) and 2 S + 1 (lane half 1) of packed words wd[0..6];
// off1 / off2 = the lane's borne-off features 193 / 195 (the table's values)
template <int S>
BGX_DEV float tb_feat_pair(const uint32_t (&wd)[7], int h, float off1, float off2) {
    constexpr int f = 2 * S;
    if constexpr (f < 192) {
        constexpr int pl = f / 96, i = (f - 96 * pl) >> 2;
        const int n = (int)((wd[3 * pl + (i >> 3)] >> ((i & 7) * 4)) & 15u);
        if constexpr ((f & 3) == 0) return n >= 1 + h ? 1.0f : 0.0f;
        const float lo = n >= 3 ? 1.0f : 0.0f, hi = n > 3 ? (float)(n - 3) * 0.5f : 0.0f;
        return h ? hi : lo;
    } else {
        const uint32_t s6 = wd[6];
        if constexpr (f == 192) return h ? off1 : (float)(s6 & 15u) * 0.5f;
        if constexpr (f == 194) return h ? off2 : (float)((s6 >> 4) & 15u) * 0.5f;
        return (int)((s6 >> 16) & 1u) == h ? 1.0f : 0.0f;
    }
}

BGX_DEV float tb_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// accumulator register t of lane half h holds row (record) ...
BGX_DEV constexpr int tb_row(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// the tile's rows into LDS: the records' own words, or their afterstate rows
// (SRC: the tile's source indices, bgx_train_tile.h)
template <bool AFTER>
BGX_DEV void tb_load_rows(const TrainBatchArgs& a, const int32_t* SRC, long long base, uint32_t (*RW)[8]) {
    if constexpr (AFTER) tb_load_tile_after(a.rec, a.hdr, SRC, a.n_rec, base, RW);
    else tb_load_tile(a.rec, a.n_rec, base, RW);
}

// k-steps S .. TB_KS - 1 of the forward GEMM (a compile-time chain: W[S] and the
// feature's field are constants, so W stays in registers)
template <int S>
BGX_DEV void tb_forward_steps(const float (&W)[TB_KS], const uint32_t (&wd)[TB_C][7], int h,
                              const float (&off1)[TB_C], const float (&off2)[TB_C], f32x16 (&acc)[TB_C]) {
#pragma unroll
    for (int c = 0; c < TB_C; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(tb_feat_pair<S>(wd[c], h, off1[c], off2[c]), W[S], acc[c], 0, 0, 0);
    if constexpr (S + 1 < TB_KS) tb_forward_steps<S + 1>(W, wd, h, off1, off2, acc);
}

// the wave's 32 hidden units' pre-activations of the tile's records:
// acc[c][t] = H[record 32 c + tb_row(t, lane half)][unit lane & 31]
BGX_DEV void tb_forward(const float (&W)[TB_KS], float b1v, const uint32_t (*RW)[8], const float* off15, int lane,
                        f32x16 (&acc)[TB_C]) {
    const int r = lane & 31, h = lane >> 5;
    uint32_t wd[TB_C][7];
    float off1[TB_C], off2[TB_C];
#pragma unroll
    for (int c = 0; c < TB_C; ++c) {
#pragma unroll
        for (int k = 0; k < 7; ++k) wd[c][k] = RW[32 * c + r][k];
        off1[c] = off15[(wd[c][6] >> 8) & 15u];
        off2[c] = off15[(wd[c][6] >> 12) & 15u];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[c][t] = b1v;
    }
    tb_forward_steps<0>(W, wd, h, off1, off2, acc);
}

template <int S>
BGX_DEV void tb_load_w_steps(const float* row, float (&W)[TB_KS]) {
    W[S] = row[2 * S];
    if constexpr (S + 1 < TB_KS) tb_load_w_steps<S + 1>(row, W);
}

// the wave's W1 slice as the B operand: W[s] = W1[32 w + (lane & 31)][2 s + (lane >> 5)]
BGX_DEV void tb_load_w(const float* params, int wave, int lane, float (&W)[TB_KS]) {
    const float* row = params + (size_t)(32 * wave + (lane & 31)) * 198 + (lane >> 5);
    tb_load_w_steps<0>(row, W);
}

// k-steps I .. 16 TB_C - 1 of the backward GEMM: register I & 15 of chunk I >> 4
// is the A operand (dh of two records, one per lane half), B the lane's feature
// of those records
template <int I>
BGX_DEV void tb_backward_steps(const f32x16 (&acc)[TB_C], const uint32_t (*RW)[8], const float (*LUT)[TB_LUTW], int lane,
                               const int (&fw)[TB_NT], const int (&fsh)[TB_NT], const int (&fmask)[TB_NT],
                               f32x16 (&dW)[TB_NT]) {
    constexpr int c = I >> 4, k = I & 15;
    const uint32_t* rw = RW[32 * c + tb_row(k, lane >> 5)];
#pragma unroll
    for (int nt = 0; nt < TB_NT; ++nt) {
        const int n = (int)((rw[fw[nt]] >> fsh[nt]) & (uint32_t)fmask[nt]);
        const float x = LUT[32 * nt + (lane & 31)][n];
        dW[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[c][k], x, dW[nt], 0, 0, 0);
    }
    if constexpr (I + 1 < 16 * TB_C) tb_backward_steps<I + 1>(acc, RW, LUT, lane, fw, fsh, fmask, dW);
}

// sum of v over the block's threads (double), fixed order; the result in every thread
BGX_DEV double tb_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < TB_T / 64; ++w) s += red[w];
    return s;
}

}  // namespace

// ---------------------------------------------------------------- index
template <bool AFTER>
__global__ __launch_bounds__(TB_T) void tb_index_kernel(TrainBatchArgs a) {
    tb_index<AFTER>(a);
}

// ---------------------------------------------------------------- forward
template <bool AFTER>
__global__ __launch_bounds__(TB_T) void tb_forward_kernel(TrainBatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t RW[TB_TILE][8];
    __shared__ float P[TB_TILE][65];    // w2_j S[record][j], units j and j + 16 of a wave summed (65: conflict-free columns)
    __shared__ float off15[16];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5;
    const int unit = 32 * wave + (lane & 31);
    if (t < 16) off15[t] = tb_lut_entry(193, t);
    float W[TB_KS];
    tb_load_w(a.params, wave, lane, W);
    const float b1v = a.params[TB_NW1 + unit], w2v = a.params[TB_NW1 + 128 + unit];
    const float b2 = a.params[TB_NW1 + 256];
    __shared__ int32_t SRC[TB_TILE];   // afterstate rows only
    if constexpr (AFTER) tb_stage_src(a.srcidx, a.n_rec, (long long)blockIdx.x * TB_TILE, SRC);
    for (int tile = (int)blockIdx.x; tile < a.n_tiles; tile += (int)gridDim.x) {
        const long long base = (long long)tile * TB_TILE;
        if constexpr (AFTER) __builtin_amdgcn_s_waitcnt(0xF70);   // vmcnt(0): the requested SRC entries are in LDS
        __syncthreads();   // the previous tile's P / RW readers are done
        tb_load_rows<AFTER>(a, SRC, base, RW);
        __syncthreads();
        if constexpr (AFTER)   // the next tile's, under this tile's MFMA chains
            tb_stage_src(a.srcidx, a.n_rec, base + (long long)gridDim.x * TB_TILE, SRC);
        f32x16 acc[TB_C];
        tb_forward(W, b1v, RW, off15, lane, acc);
#pragma unroll
        for (int c = 0; c < TB_C; ++c)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                float pv = w2v * tb_sigmoid(acc[c][k]);
                pv += __shfl_xor(pv, 16, 64);
                if (!(lane & 16)) P[32 * c + tb_row(k, h)][16 * wave + (lane & 15)] = pv;
            }
        __syncthreads();
        if (t < TB_TILE && base + t < a.n_rec) {
            float y = 0.0f;
            for (int u = 0; u < 64; ++u) y += P[t][u];
            a.Y[base + t] = y + b2;
        }
    }
}

// ---------------------------------------------------------------- backward
// LAM: the target is the target stage's tgt[s] (TD(lambda)), not the inline TD(0) one
template <bool LAM, bool AFTER>
__global__ __launch_bounds__(TB_T) void tb_backward_kernel(TrainBatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t RW[TB_TILE][8];
    __shared__ __attribute__((aligned(16))) float D[TB_TILE];   // dL/dY of the tile's records
    __shared__ float LUT[32 * TB_NT][TB_LUTW];   // rows padded to 17: a lane per row, conflict-free
    __shared__ double red[4][2];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5;
    const int unit = 32 * wave + (lane & 31);
    for (int idx = t; idx < 32 * TB_NT * 16; idx += TB_T) LUT[idx >> 4][idx & 15] = tb_lut_entry(idx >> 4, idx & 15);
    const float* off15 = LUT[193];
    float W[TB_KS];
    tb_load_w(a.params, wave, lane, W);
    const float b1v = a.params[TB_NW1 + unit], w2v = a.params[TB_NW1 + 128 + unit];
    // feature nt * 32 + (lane & 31): the word it reads, the field's shift and mask
    int fw[TB_NT], fsh[TB_NT], fmask[TB_NT];
#pragma unroll
    for (int nt = 0; nt < TB_NT; ++nt) {
        const TbField fd = tb_field(32 * nt + (lane & 31));
        fw[nt] = fd.word;
        fsh[nt] = fd.shift;
        fmask[nt] = fd.mask;
    }
    f32x16 dW[TB_NT];
#pragma unroll
    for (int nt = 0; nt < TB_NT; ++nt)
#pragma unroll
        for (int k = 0; k < 16; ++k) dW[nt][k] = 0.0f;
    float gb1 = 0.0f, gw2 = 0.0f, gb2 = 0.0f;
    double m_loss = 0.0, m_td = 0.0, m_y = 0.0, m_rw = 0.0;   // threads < TB_TILE: their records' shares
    const float n_eps = (float)a.n_eps;
    __shared__ int32_t SRC[TB_TILE];   // afterstate rows only
    if constexpr (AFTER) tb_stage_src(a.srcidx, a.n_rec, (long long)blockIdx.x * TB_TILE, SRC);

    for (int tile = (int)blockIdx.x; tile < a.n_tiles; tile += (int)gridDim.x) {
        const long long base = (long long)tile * TB_TILE;
        if constexpr (AFTER) __builtin_amdgcn_s_waitcnt(0xF70);   // vmcnt(0): the requested SRC entries are in LDS
        __syncthreads();   // the previous tile's readers are done
        tb_load_rows<AFTER>(a, SRC, base, RW);
        if (t < TB_TILE) {
            const long long s = base + t;
            float d = 0.0f;
            if (s < a.n_rec) {
                const int inf = a.info[s], T = inf & 0x7FFFFFFF;
                if (T > 0) {
                    const float rew = __uint_as_float(a.rec[(size_t)s * 12 + 9]);
                    const float y = a.Y[s];
                    float tg;
                    if constexpr (LAM) {
                        tg = a.tgt[s];
                    } else {
                        const bool boot = inf >= 0 && s + 1 < a.n_rec;
                        tg = boot ? rew + a.gamma * a.Y[s + 1] : rew;
                    }
                    const float diff = y - tg, fT = (float)T;
                    d = 2.0f * diff / (n_eps * fT);
                    m_loss += (double)(diff * diff / fT);
                    m_td += (double)(fabsf(diff) / fT);
                    m_y += (double)(y / fT);
                    m_rw += (double)rew;
                }
            }
            D[t] = d;
        }
        __syncthreads();
        if constexpr (AFTER)   // the next tile's, under this tile's MFMA chains
            tb_stage_src(a.srcidx, a.n_rec, base + (long long)gridDim.x * TB_TILE, SRC);
        f32x16 acc[TB_C];
        tb_forward(W, b1v, RW, off15, lane, acc);
        // dL/dh in place (torch's sigmoid_backward order), and the small gradients
#pragma unroll
        for (int c = 0; c < TB_C; ++c)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float d = D[32 * c + tb_row(k, h)];
                const float s = tb_sigmoid(acc[c][k]);
                const float dh = ((d * w2v) * (1.0f - s)) * s;
                gw2 = fmaf(d, s, gw2);
                gb1 += dh;
                gb2 += d;
                acc[c][k] = dh;
            }
        // dW1 += dh^T X, two records per k-step
        tb_backward_steps<0>(acc, RW, LUT, lane, fw, fsh, fmask, dW);
    }

    // ---- the workgroup's partial gradient into its row (zeros if it had no tile)
    float* P = a.partial + (size_t)blockIdx.x * TB_PS;
#pragma unroll
    for (int nt = 0; nt < TB_NT; ++nt) {
        const int k = 32 * nt + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (k < 198) P[(32 * wave + tb_row(r, h)) * 198 + k] = dW[nt][r];
    }
    gb1 += __shfl_xor(gb1, 32, 64);   // the two lane halves hold the two halves of the records
    gw2 += __shfl_xor(gw2, 32, 64);
    gb2 += __shfl_xor(gb2, 32, 64);
    if (h == 0) {
        P[TB_NW1 + unit] = gb1;
        P[TB_NW1 + 128 + unit] = gw2;
    }
    if (t == 0) P[TB_NW1 + 256] = gb2;
    // ---- metrics: threads 0 .. TB_TILE - 1 (waves 0, 1) hold the shares
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m_loss += __shfl_xor(m_loss, off, 64);
        m_td += __shfl_xor(m_td, off, 64);
        m_y += __shfl_xor(m_y, off, 64);
        m_rw += __shfl_xor(m_rw, off, 64);
    }
    __syncthreads();
    if (lane == 0 && wave < 2) {
        red[0][wave] = m_loss;
        red[1][wave] = m_td;
        red[2][wave] = m_y;
        red[3][wave] = m_rw;
    }
    __syncthreads();
    if (t < 4) a.mpart[(size_t)blockIdx.x * 4 + t] = red[t][0] + red[t][1];
}

// ---------------------------------------------------------------- reduce
__global__ __launch_bounds__(TB_T) void tb_reduce_kernel(TrainBatchArgs a) {
    __shared__ double red[TB_T / 64];
    const int i = (int)(blockIdx.x * TB_T + threadIdx.x);
    float g = 0.0f;
    if (i < TB_NP) {
        for (int w = 0; w < a.grid; ++w) g += a.partial[(size_t)w * TB_PS + i];
        a.grad[i] = g;
        if (a.grad_out) a.grad_out[i] = g;
    }
    const double sq = tb_block_sum((double)g * (double)g, red);
    if (threadIdx.x == 0) a.sqpart[blockIdx.x] = sq;
}

// ---------------------------------------------------------------- clip + Adam
__global__ __launch_bounds__(TB_T) void tb_adam_kernel(TrainBatchArgs a) {
#pragma clang fp contract(off)
    __shared__ float sh[4];
    if (threadIdx.x == 0) {
        double sq = 0.0;
        for (int b = 0; b < TB_NB; ++b) sq += a.sqpart[b];
        const float norm = (float)sqrt(sq);
        float scale = 1.0f;
        if (a.grad_clip > 0.0f) {   // clip_grad_norm_: coef = clip / (norm + 1e-6), applied when below 1
            const float coef = a.grad_clip / (norm + 1e-6f);
            scale = coef < 1.0f ? coef : 1.0f;
        }
        // torch.optim.Adam, non-capturable: bias corrections in double (td0_train_kernel)
        const int step = *a.step;
        const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
        sh[0] = scale;
        sh[1] = (float)(a.lr / bc1);
        sh[2] = (float)sqrt(bc2);
        sh[3] = norm * scale;
        if (blockIdx.x == 0) {
            double m[4] = {0.0, 0.0, 0.0, 0.0};
            for (int w = 0; w < a.grid; ++w)
                for (int k = 0; k < 4; ++k) m[k] += a.mpart[(size_t)w * 4 + k];
            a.metrics[0] += m[0];
            a.metrics[1] += (double)a.n_eps * (double)sh[3];
            a.metrics[2] += m[1];
            a.metrics[3] += m[2];
            a.metrics[4] += m[3];
        }
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * TB_T + threadIdx.x);
    if (i >= TB_NP) return;
    const float scale = sh[0], step_size = sh[1], bc2s = sh[2];
    const float w1m = (float)(1.0 - 0.9), w2v = (float)(1.0 - 0.999);
    float g = a.grad[i];
    if (a.grad_clip > 0.0f) g = g * scale;
    float p = a.params[i], m = a.adam_m[i], v = a.adam_v[i];
    m = m + w1m * (g - m);                                             // lerp(m, g, 1 - beta1)
    v = v * 0.999f + (w2v * g) * g;                                    // mul(beta2).addcmul(g, g, 1 - beta2)
    // one step per call, not one per episode as in td0_train_kernel: the correctly
    // rounded square root and divisions, in torch's own order
    const float den = sqrtf(v) / bc2s + 1e-8f;                         // sqrt(v) / sqrt(bc2) + eps
    p = p + ((-step_size) * m) / den;                                  // addcdiv(m, den, -step_size)
    a.params[i] = p;
    a.adam_m[i] = m;
    a.adam_v[i] = v;
}

}  // namespace bgx

// The launch sequence of every entry point. The target stage runs when the
// backward launch reads its targets (lam below) or the caller wants them
// (target_out); the records' movers and rewards it reads (words 11 and 9) are
// the same under AFTER.
template <bool AFTER>
static hipError_t tb_launch(bgx::TrainBatchArgs a, hipStream_t stream) {
    using namespace bgx;
    a.n_tiles = (int)(((long long)a.n_rec + TB_TILE - 1) / TB_TILE);
    a.grid = a.n_tiles < TRAIN_BATCH_GRID ? a.n_tiles : TRAIN_BATCH_GRID;
    // a record in no episode keeps 0 in both: it takes no part, its row is its own words
    hipError_t e = hipMemsetAsync(a.info, 0, (size_t)a.n_rec * sizeof(int32_t), stream);
    if (AFTER && e == hipSuccess) e = hipMemsetAsync(a.srcidx, 0, (size_t)a.n_rec * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tb_index_kernel<AFTER>, dim3((a.n_eps + TB_T - 1) / TB_T), dim3(TB_T), 0, stream, a);
    hipLaunchKernelGGL(tb_forward_kernel<AFTER>, dim3(a.grid), dim3(TB_T), 0, stream, a);
    // lambda = 0 keeps the TD(0) backward launch (the same bits by construction); the
    // stage then runs only to fill target_out. Zero-sum targets: the inline TD(0)
    // target knows no movers, so the stage and the backward launch on its targets
    // run at lambda = 0 too. Afterstates: always both
    if (!a.tgt) a.zero_sum = 0;
    const bool lam = AFTER || (a.tgt && (a.lambda != 0.0f || a.zero_sum));
    if (lam || (a.tgt && a.target_out)) {
        e = bgx_launch_lambda_targets(&a, stream);
        if (e != hipSuccess) return e;
    }
    if (lam) hipLaunchKernelGGL((tb_backward_kernel<true, AFTER>), dim3(a.grid), dim3(TB_T), 0, stream, a);
    else if constexpr (!AFTER) hipLaunchKernelGGL((tb_backward_kernel<false, false>), dim3(a.grid), dim3(TB_T), 0, stream, a);
    hipLaunchKernelGGL(tb_reduce_kernel, dim3(TB_NB), dim3(TB_T), 0, stream, a);
    hipLaunchKernelGGL(tb_adam_kernel, dim3(TB_NB), dim3(TB_T), 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_td_batched(const bgx::TrainBatchArgs* args, hipStream_t stream) {
    if (!args->hdr && !args->srcidx) return tb_launch<false>(*args, stream);
    if (!args->tgt || !args->hdr || !args->srcidx) return hipErrorInvalidValue;
    return tb_launch<true>(*args, stream);
}
