// bgx_pack.h — the learner's two device-side hand-offs (bgx_pack.hip launches
// them; the host emulation of tests/cpuwave/ compiles the same bodies):
//   * trainer parameters -> the engine's network, without the host: a check
//     launch (bgx_frag::unrepresentable's rules, the scale exponent) and a pack
//     launch (bgx_frag::build_fragments' arithmetic per element, plus the fp32
//     copies a bgx_net keeps), bgx_set_weights_device;
//   * a harvest's headers -> episode offsets, bgx_episode_offsets.
// Plain loads and vector stores only: no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bgx {

// the trainer's flat parameters (state_dict order): fc1.weight [128][198],
// fc1.bias [128], value_head.weight [128], value_head.bias [1]
constexpr int PK_W1 = 128 * 198;
constexpr int PK_B1 = PK_W1, PK_W2 = PK_W1 + 128, PK_B2 = PK_W1 + 256;
constexpr int PK_PARAMS = PK_B2 + 1;                // 25,601
constexpr int PK_KSTEPS = 13;                       // bgx_frag::KSTEPS
constexpr int PK_NFRAG = 2 * 4 * PK_KSTEPS * 64;    // bgx_frag::NFRAG, 16-byte fragments
constexpr int PK_CHECK_THREADS = 1024;              // the check launch: one workgroup
constexpr int PK_PACK_THREADS = 256;
constexpr int PK_PACK_ITEMS = PK_NFRAG / 2;         // one thread packs the hi and the lo fragment of 8 weights
constexpr int PK_OFFS_THREADS = 1024;               // the offsets launch: one workgroup

constexpr double PK_LOG2E = 1.4426950408889634;     // bgx_frag::kLog2e
constexpr double PK_MAX_SCALED = 67108864.0;        // bgx_frag::kMaxScaled, 2^26

enum { PK_RULE_OK = 0, PK_RULE_NONFINITE = 1, PK_RULE_LIMIT = 2 };

// the check launch's verdict, 16 bytes: what the pack launch and the host read
struct PackInfo {
    uint32_t rule;      // PK_RULE_*
    int32_t index;      // flat index of the offending entry (rule != 0)
    int32_t e;          // the scale exponent build_fragments returns
    uint32_t b2_bits;   // value_head.bias, for the launch arguments (set_net)
};

__device__ inline uint32_t pk_f32_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}

// max / min over the 64 lanes of a wave, every lane gets the result
__device__ inline int pk_wave_min(int v) {
    for (int m = 32; m > 0; m >>= 1) {
        const int o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline double pk_wave_max(double v) {
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// One workgroup of PK_CHECK_THREADS over the 25,601 parameters: the lowest flat
// index of a non-finite entry; failing that the lowest index in W1, then in b1,
// whose log2(e) |w| (columns 193 / 195 of W1 divided by 15) reaches 2^26, in
// unrepresentable's own operations; failing that mx and e as build_fragments
// takes them. Thread 0 writes *info.
__device__ inline void pack_check_body(const float* __restrict__ p, PackInfo* __restrict__ info) {
    constexpr int NONE = 0x7FFFFFFF;
    constexpr int NW = PK_CHECK_THREADS / 64;
    __shared__ int s_nf[NW], s_lim[NW];
    __shared__ double s_mx[NW];
    const int t = (int)threadIdx.x;
    int nf = NONE, lim = NONE;
    double mx = 0.0;
    for (int i = t; i < PK_PARAMS; i += PK_CHECK_THREADS) {   // ascending: a thread's first hit is its lowest
        const float w = p[i];
        if ((pk_f32_bits(w) & 0x7F800000u) == 0x7F800000u) {
            if (nf == NONE) nf = i;
        } else if (i < PK_W2) {
            const int k = i < PK_W1 ? i % 198 : 198;
            const bool off = k == 193 || k == 195;   // feature = integer borne-off count
            const double a = __builtin_fabs((double)w);
            const double lv = off ? PK_LOG2E * a / 15.0 : PK_LOG2E * a;   // unrepresentable's form
            if (lv >= PK_MAX_SCALED && lim == NONE) lim = i;
            const double v = off ? (double)w / 15.0 : (double)w;          // build_fragments' form
            const double m = __builtin_fabs(-PK_LOG2E * v);
            mx = m > mx ? m : mx;
        }
    }
    nf = pk_wave_min(nf);
    lim = pk_wave_min(lim);
    mx = pk_wave_max(mx);
    if ((t & 63) == 0) {
        s_nf[t >> 6] = nf;
        s_lim[t >> 6] = lim;
        s_mx[t >> 6] = mx;
    }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < NW; ++w) {
        nf = s_nf[w] < nf ? s_nf[w] : nf;
        lim = s_lim[w] < lim ? s_lim[w] : lim;
        mx = s_mx[w] > mx ? s_mx[w] : mx;
    }
    // e = clamp(14 - floor(log2(mx)), -11, 13), 0 for mx == 0. floor(log2(mx)) is
    // the double's exponent field, read from its bits: exact for every mx, where
    // the host's std::floor(std::log2(mx)) may round up to the next integer for
    // an mx one ulp below a power of two. (A subnormal mx reads as 2^-1023 and
    // clamps to 13 like its true exponent.)
    int e = 0;
    if (mx > 0.0) {
        uint64_t b;
        __builtin_memcpy(&b, &mx, 8);
        e = 14 - ((int)((b >> 52) & 0x7FFu) - 1023);
        e = e > 13 ? 13 : (e < -11 ? -11 : e);
    }
    PackInfo r;
    r.rule = nf != NONE ? PK_RULE_NONFINITE : (lim != NONE ? PK_RULE_LIMIT : PK_RULE_OK);
    r.index = nf != NONE ? nf : (lim != NONE ? lim : 0);
    r.e = r.rule == PK_RULE_OK ? e : 0;
    r.b2_bits = pk_f32_bits(p[PK_B2]);
    *info = r;
}

// fp64 -> fp16 through fp32, two roundings, as build_fragments' (_Float16)(float)x
// gives on the host. The device compiler merges the two casts into one
// fp64 -> fp16 rounding, which differs where the fp32 value lands on an fp16
// tie (3 halves of the seed-0 set, 13 of the checkpoint's): the fp32 value
// passes through an empty asm statement there, so both conversions are issued.
__device__ inline uint16_t pk_f16_bits_via_f32(double x) {
    float f = (float)x;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(f));
#endif
    const _Float16 h = (_Float16)f;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

__device__ inline double pk_f16_value(uint16_t b) {
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (double)(float)h;
}

// A grid of at least PK_PACK_ITEMS threads. Writes nothing when the check
// failed (the previous network stays in force). Thread g < PK_PACK_ITEMS is
// (m-tile, k-step, lane) of the fragment order [2][4][13][64][8] and stores that
// position's hi fragment and its lo fragment, 8 weights each, by
// build_fragments' operations: x = (-log2(e) w) 2^e in fp64 (w / 15 first for
// columns 193 / 195, the bias as column 198, zeros up to 208), hi = fp16(fp32(x)),
// lo = fp16(fp32(x - hi)); the scale is a power of two, so x is exact and a
// contraction of the product into the difference changes no bit. fp16
// subnormals are kept (the conversions round to nearest even, no flush). All
// threads then copy W1, b1, w2 and w2 again (rowc) to the net's fp32 arrays.
__device__ inline void pack_frag_body(const float* __restrict__ p, const PackInfo* __restrict__ info,
                                      uint4* __restrict__ frag, float* __restrict__ W1, float* __restrict__ b1,
                                      float* __restrict__ w2, float* __restrict__ rowc) {
    if (info->rule != PK_RULE_OK) return;
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int n_threads = (int)(gridDim.x * blockDim.x);
    if (g < PK_PACK_ITEMS) {
        const uint64_t sb = (uint64_t)(1023 + info->e) << 52;   // 2^e, e in [-11, 13]
        double sc;
        __builtin_memcpy(&sc, &sb, 8);
        const int l = g & 63, ms = g >> 6;   // ms = m * 13 + s
        const int row = 32 * (ms / PK_KSTEPS) + (l & 31);
        const int k0 = 16 * (ms % PK_KSTEPS) + 8 * (l >> 5);
        uint32_t hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
        for (int jj = 0; jj < 8; ++jj) {
            const int k = k0 + jj;
            double wp = 0.0;   // the padding columns 199 .. 207
            if (k < 198) {
                double v = (double)p[row * 198 + k];
                if (k == 193 || k == 195) v /= 15.0;
                wp = -PK_LOG2E * v;
            } else if (k == 198) {
                wp = -PK_LOG2E * (double)p[PK_B1 + row];
            }
            const double x = wp * sc;
            const uint16_t h = pk_f16_bits_via_f32(x);
            const uint16_t r = pk_f16_bits_via_f32(x - pk_f16_value(h));
            hi[jj >> 1] |= (uint32_t)h << (16 * (jj & 1));
            lo[jj >> 1] |= (uint32_t)r << (16 * (jj & 1));
        }
        frag[g] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        frag[PK_PACK_ITEMS + g] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
    for (int i = g; i < PK_W1; i += n_threads) W1[i] = p[i];
    if (g < 128) {
        b1[g] = p[PK_B1 + g];
        const float c = p[PK_W2 + g];
        w2[g] = c;
        rowc[g] = c;
    }
}

// One workgroup of PK_OFFS_THREADS: offs[0] = 0, offs[k + 1] = offs[k] + word 3
// (n_records) of header k, the headers taken 1,024 at a time: an inclusive scan
// within each wave, the waves' totals combined through LDS, and a carry every
// thread keeps from chunk to chunk. (Header word 2 is a ring position, not an
// offset into the harvest's records.)
__device__ inline void episode_offsets_body(const uint32_t* __restrict__ hdr, int n, int32_t* __restrict__ offs) {
    constexpr int NW = PK_OFFS_THREADS / 64;
    __shared__ int32_t s_tot[NW];
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) offs[0] = 0;
    int32_t carry = 0;
    for (int base = 0; base < n; base += PK_OFFS_THREADS) {   // n is uniform: every thread makes every trip
        const int i = base + t;
        int32_t v = i < n ? (int32_t)hdr[(size_t)i * 16 + 3] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t u = __shfl(v, (lane - d) & 63);
            if (lane >= d) v += u;
        }
        if (lane == 63) s_tot[wv] = v;
        __syncthreads();
        int32_t before = 0, all = 0;
        for (int w = 0; w < NW; ++w) {
            const int32_t x = s_tot[w];
            all += x;
            if (w < wv) before += x;
        }
        if (i < n) offs[i + 1] = carry + before + v;
        carry += all;
        __syncthreads();   // s_tot is rewritten by the next chunk
    }
}

}  // namespace bgx

extern "C" {
// d_params [25601] -> *info (one workgroup)
hipError_t bgx_launch_weights_check(const float* params, bgx::PackInfo* info, hipStream_t stream);
// d_params, *info -> a bgx_net's arrays; nothing is written when info->rule != 0
hipError_t bgx_launch_weights_pack(const float* params, const bgx::PackInfo* info, uint4* frag, float* W1, float* b1,
                                   float* w2, float* rowc, hipStream_t stream);
// headers [n][16] -> offs [n + 1] (one workgroup; n = 0 writes offs[0])
hipError_t bgx_launch_episode_offsets(const uint32_t* headers, int n, int32_t* offs, hipStream_t stream);
}
