// bgx_match.hip — match mode: two networks head to head on the phased engine.
//
// In match mode (bgx_engine_set_opponent) player p of episode k on global lane
// g is played by network (p ^ g ^ k) & 1, and the mover's network evaluates
// everything its step needs (the lane row, every candidate, at ply 2 the
// replies to its candidates). The W fragments of one network take 104 KB of
// the CU's 160 KB of LDS (bgx_mlp.hip), so a workgroup holds one network at a
// time: routing kernels sort the step's rows into two index lists, one per
// network, and mlp_kernel_routed evaluates list n under network n.
//
// mlp_kernel_routed: persistent, one workgroup per CU. Workgroup b loads
// network b & 1 (fragments, w2, the feature LUT at that network's 2^-e scale),
// takes chunks of 32 NT-row tiles of that network's list from the list's atomic
// tile counter (thread 0 claims, the base goes to every wave through LDS, so
// the exit of the claim loop is workgroup-uniform), its waves gather the packed
// rows through the list and run the hi / lo MFMA chain and the canonical
// epilogue of bgx_mlp.h; V goes to out[index]. When the list is drained all
// waves meet at a barrier and the workgroup turns to the other list (loading
// the other network only if a claim there succeeds): the launch stays
// balanced whatever the lists' lengths (one may be empty). A row's V has
// the bits every other MLP kernel gives it under the same network, whichever
// tile or column it lands in (each MFMA column is one board), so the order of
// a list, which depends on atomic timing, does not matter.
// LDS: 104 KB fragments + 4 KB LUT + 512 B w2 + 16 B of claim slots = 108.5 KB
// per workgroup.
#include "bgx_mlp.h"

#include <cstdlib>

namespace bgx {

// tile `tile` of a list of n indices: column col's row (empty, idx = -1, past
// the list's end or for an index outside the rows buffer)
BGX_DEV void routed_rows(const uint32_t* rows, int n_max, const int32_t* list, int n, int tile, int col, uint4& x,
                         uint4& y, int& idx) {
    const int li = tile * 32 + col;
    x = make_uint4(0, 0, 0, 0);
    y = make_uint4(0, 0, 0, 0);
    idx = -1;
    if (li < n) {
        const int r = list[li];
        if (r >= 0 && r < n_max) {
            const uint4* p = (const uint4*)(rows + (size_t)r * 8);
            x = p[0];
            y = p[1];
            idx = r;
        }
    }
}

// NT = 32-board tiles per wave iteration (1: the root launch and the stateless
// call; 2: the reply launch, each A fragment read from LDS feeds 2 MFMAs), NW =
// waves per workgroup.
//
// Claims are per workgroup: thread 0 takes a chunk of NW x C tiles from the
// list's counter with one atomic and hands its base to the workgroup through
// LDS; wave w runs tiles base + w, base + w + NW, ... of the chunk. (One claim
// per wave and tile, the first form of this kernel, put ~16,000 atomics per
// launch on two addresses and cost more than the MFMA work: DESIGN.md
// section 4b.) The next chunk is claimed one chunk ahead, and its base read
// after the barrier that opens the current chunk's last tile, so the next
// tile's indices and rows are always loaded while the current tile's MFMAs
// run. Every branch around a barrier depends on LDS words and launch
// arguments only: workgroup-uniform.
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void mlp_kernel_routed(MatchMlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 lds[];
    uint4* wf = lds;                                   // [NFRAG]
    uint4* lut = lds + NFRAG;                          // [256]
    float* w2s = (float*)(lds + NFRAG + 256);          // [128] value-head weights
    int* slot = (int*)(lds + NFRAG + 256 + 32);        // [2] claimed chunk bases, in turn
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int wave = uniform((int)(threadIdx.x >> 6));   // (in a scalar register: the tile indices follow)
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const int net = ((int)blockIdx.x + pass) & 1;
        const int32_t* list = net ? a.list[1] : a.list[0];
        unsigned* clm = net ? a.claim[1] : a.claim[0];
        const unsigned cn = net ? *a.count[1] : *a.count[0];
        const int n = cn > (unsigned)a.list_cap ? a.list_cap : (int)cn;
        const int tiles = (n + 32 * NT - 1) / (32 * NT);
        // (the same word for every thread of the launch, written before it)
        if (tiles == 0) continue;
        // tiles per wave and chunk: about four chunks per workgroup, 1..8
        int C = tiles / ((int)gridDim.x * NW * 4);
        C = C < 1 ? 1 : (C > 8 ? 8 : C);
        const unsigned chunk = (unsigned)(NW * C);
        __syncthreads();   // every wave is done with the previous network's fragments and slots
        if (threadIdx.x == 0) slot[0] = (int)atomicAdd(clm, chunk);
        __syncthreads();
        int base = slot[0];
        if (base >= tiles) continue;   // the list is drained (or taken): no fragment load
        const float fs = net ? a.feat_scale[1] : a.feat_scale[0];
        const float b2 = net ? a.b2[1] : a.b2[0];
        const uint4* wsrc = net ? a.wfrag[1] : a.wfrag[0];
        const float* csrc = net ? a.rowc[1] : a.rowc[0];
        if (threadIdx.x == 0) slot[1] = (int)atomicAdd(clm, chunk);   // the next chunk, one ahead
        for (int i = threadIdx.x; i < NFRAG; i += blockDim.x) wf[i] = wsrc[i];
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = lut_entry((uint32_t)i, fs);
        for (int i = threadIdx.x; i < 128; i += blockDim.x) w2s[i] = csrc[i];
        int t = base + wave;
        uint4 px[NT], py[NT];
        int pidx[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) routed_rows(a.rows, a.n_max, list, n, t * NT + q, col, px[q], py[q], pidx[q]);
        __syncthreads();
        int cur = 0;   // slot[cur]: this chunk's base; slot[cur ^ 1]: the next chunk's
#pragma unroll 1
        for (int i = 0;; ++i) {
            int tn = t + NW;
            int nbase = 0;
            const bool last = i + 1 == C;
            if (last) {
                __syncthreads();   // thread 0's claim of the next chunk is in its slot
                nbase = slot[cur ^ 1];
                tn = nbase + wave;
                // the chunk after the next one into the slot every wave has read
                if (threadIdx.x == 0 && nbase < tiles) slot[cur] = (int)atomicAdd(clm, chunk);
            }
            uint4 bx[NT], by[NT];
            int idx[NT];
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                bx[q] = px[q];
                by[q] = py[q];
                idx[q] = pidx[q];
                routed_rows(a.rows, a.n_max, list, n, tn * NT + q, col, px[q], py[q], pidx[q]);   // next tile
            }
            if (t < tiles) {   // (a chunk's tail past the list's end: nothing to evaluate)
                floatx16 acc[4][NT];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int q = 0; q < NT; ++q)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.0f;
                // fragment pipeline at (k-step, m-tile) granularity, as mlp_kernel: the
                // next (hi, lo) A pair is read from LDS while the current pair's MFMAs run
                uint4 ch = wf[((0 * 4 + 0) * KSTEPS + 0) * 64 + lane];
                uint4 cl = wf[((1 * 4 + 0) * KSTEPS + 0) * 64 + lane];
                half8 b[NT];
#pragma unroll
                for (int q = 0; q < NT; ++q) b[q] = feat_frag(bx[q], by[q], 0, h, lut, fs);
#pragma unroll 1
                for (int s = 0; s < KSTEPS; ++s) {
                    const int sn = s + 1 < KSTEPS ? s + 1 : s;
                    half8 nb[NT];
#pragma unroll
                    for (int q = 0; q < NT; ++q) nb[q] = feat_frag(bx[q], by[q], sn, h, lut, fs);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int s2 = m < 3 ? s : sn, m2 = m < 3 ? m + 1 : 0;
                        const uint4 nh = wf[((0 * 4 + m2) * KSTEPS + s2) * 64 + lane];
                        const uint4 nl = wf[((1 * 4 + m2) * KSTEPS + s2) * 64 + lane];
#pragma unroll
                        for (int q = 0; q < NT; ++q) {
                            acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8*)&ch, b[q], acc[m][q], 0, 0, 0);
                            acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8*)&cl, b[q], acc[m][q], 0, 0, 0);
                        }
                        ch = nh;
                        cl = nl;
                    }
#pragma unroll
                    for (int q = 0; q < NT; ++q) b[q] = nb[q];
                }
                // sigmoid and the value head in the canonical order (bgx_mlp.h, epilogue order)
                float v[NT];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float pm[NT];
#pragma unroll
                    for (int q = 0; q < NT; ++q) pm[q] = 0.0f;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 c4 = *(const float4*)(w2s + 32 * m + 8 * g + 4 * h);
                        const float cy[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int r = 4 * g + k;
#pragma unroll
                            for (int q = 0; q < NT; ++q) {
                                const float ex = __builtin_amdgcn_exp2f(acc[m][q][r]);
                                pm[q] = fmaf(cy[k], __builtin_amdgcn_rcpf(1.0f + ex), pm[q]);
                            }
                            if ((r & 1) == 1) __builtin_amdgcn_sched_barrier(0);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NT; ++q) v[q] = m == 0 ? pm[q] : v[q] + pm[q];
                }
#pragma unroll
                for (int q = 0; q < NT; ++q) {
                    v[q] += __shfl_xor(v[q], 32, 64);
                    if (h == 0 && idx[q] >= 0) a.out[idx[q]] = v[q] + b2;
                }
            }
            t = tn;
            if (last) {
                if (nbase >= tiles) break;   // workgroup-uniform (an LDS word)
                cur ^= 1;
                i = -1;
            }
        }
    }
}

// ------------------------------------------------------------------ routing
// Root routing, one thread per lane: the lane's network takes 1 + c entries
// of its list (the lane row, then the lane's c candidate rows), reserved with
// one atomic per wave and network after a wave scan. Each thread writes the
// first 32 entries of its own lane (most lanes have fewer); the lanes with more
// are finished by the whole wave, 64 consecutive entries per store.
constexpr int ROUTE_OWN = 32;
__global__ __launch_bounds__(256) void route_root_kernel(MatchRouteArgs a) {
    const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int lane = lane_id();
    const bool live = l < a.L;
    int net = 0, off = 0, c = 0;
    if (live) {
        net = (int)(((uint32_t)a.player[l] ^ (uint32_t)(a.lane_base + l) ^ a.epi[l]) & 1u);
        // the rows the flat candidate buffer really holds (OUT_PACKED_FLAT: a job
        // that did not fit has count 0; the running count may pass the capacity)
        const unsigned fc = *a.flat_count;
        const int have = fc > (unsigned)a.cand_cap ? a.cand_cap : (int)fc;
        off = a.cand_off[l];
        c = a.cand_cnt[l];
        if (off < 0 || c < 0 || off > have) {
            off = 0;
            c = 0;
        } else if (c > have - off) {
            c = have - off;
        }
    }
    const int need = live ? 1 + c : 0;
    int base = 0;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int mine = net == n ? need : 0;
        const int incl = wave_incl_scan(mine);
        const int tot = lane63(incl);
        int b = 0;
        if (lane == 0 && tot > 0) b = (int)atomicAdd(a.count + n, (unsigned)tot);
        b = uniform(b);
        if (net == n) base = b + incl - mine;
    }
    const int cap = a.L + a.cand_cap;
    const bool slots_all = a.slot_net && a.k_top != 4;   // K = all: one byte per candidate row
    {
        int32_t* lst = net ? a.list[1] : a.list[0];
        const int nd = need < ROUTE_OWN ? need : ROUTE_OWN;
        for (int i = 0; i < nd; ++i) {
            if (base + i < cap) lst[base + i] = i == 0 ? l : a.L + off + i - 1;
            if (slots_all && i > 0 && off + i - 1 < a.n_slots) a.slot_net[off + i - 1] = (uint8_t)net;
        }
        if (a.slot_net && a.k_top == 4 && live && 4 * l + 3 < a.n_slots)   // K = 4: slots 4 l .. 4 l + 3
            *(uint32_t*)(a.slot_net + 4 * (size_t)l) = net ? 0x01010101u : 0u;
    }
    uint64_t big = ballot(need > ROUTE_OWN);
    while (big) {   // (wave-uniform: a ballot)
        const int k = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        const int kn = __builtin_amdgcn_readlane(net, k), kneed = __builtin_amdgcn_readlane(need, k),
                  kb = __builtin_amdgcn_readlane(base, k), koff = __builtin_amdgcn_readlane(off, k);
        int32_t* lst = kn ? a.list[1] : a.list[0];
        for (int i = ROUTE_OWN + lane; i < kneed; i += 64) {
            if (kb + i < cap) lst[kb + i] = a.L + koff + i - 1;
            if (slots_all && koff + i - 1 < a.n_slots) a.slot_net[koff + i - 1] = (uint8_t)kn;
        }
    }
}

// Reply routing, one thread per job: job j's rows job_off[j] .. job_off[j] +
// job_cnt[j] - 1 go to the list of its root slot's network (slot j / 21). Rows
// of no job (the reservation chunks' unwritten tails) are on neither list.
// Each workgroup owns a contiguous span of 64-job groups, which its waves
// take in turn: a first pass sums the span's rows per network, one atomic per
// workgroup and network reserves them (one per wave and group put ~21,000
// atomics per launch on two addresses: 0.16 ms), a second pass writes the
// indices, a job's rows by the whole wave (consecutive addresses).
constexpr int ROUTE_NW = 16;
__global__ __launch_bounds__(64 * ROUTE_NW) void route_reply_kernel(MatchRouteArgs a) {
    __shared__ int wtot[ROUTE_NW][2];
    __shared__ int wbase[ROUTE_NW][2];
    int nj = a.n_jobs;
    if (a.n_units_dev) nj += (int)(*a.n_units_dev) * 21;
    if (a.n_jobs_max > 0 && nj > a.n_jobs_max) nj = a.n_jobs_max;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int groups = (nj + 63) / 64;
    const int per = (groups + (int)gridDim.x - 1) / (int)gridDim.x;
    const int g0 = (int)blockIdx.x * per;
    const int g1 = g0 + per < groups ? g0 + per : groups;
    auto fetch = [&](int g, int& net, int& off, int& c) {
        const int j = g * 64 + lane;
        net = 0;
        off = 0;
        c = 0;
        if (j < nj) {
            const int slot = j / 21;
            net = slot < a.n_slots ? (int)(a.slot_net[slot] & 1u) : 0;
            off = a.job_off[j];
            c = a.job_cnt[j];
            if (off < 0 || c < 0 || off > a.reply_cap) {
                off = 0;
                c = 0;
            } else if (c > a.reply_cap - off) {
                c = a.reply_cap - off;
            }
        }
    };
    int tot[2] = {0, 0};
    for (int g = g0 + wave; g < g1; g += ROUTE_NW) {   // wave-uniform bounds
        int net, off, c;
        fetch(g, net, off, c);
        tot[0] += wave_sum(net == 0 ? c : 0);
        tot[1] += wave_sum(net == 1 ? c : 0);
    }
    if (lane == 0) {
        wtot[wave][0] = tot[0];
        wtot[wave][1] = tot[1];
    }
    __syncthreads();
    if (threadIdx.x < 2) {   // thread n reserves the workgroup's rows on list n
        const int n = (int)threadIdx.x;
        int sum = 0;
        for (int w = 0; w < ROUTE_NW; ++w) sum += wtot[w][n];
        int b = sum > 0 ? (int)atomicAdd(a.rcount + n, (unsigned)sum) : 0;
        for (int w = 0; w < ROUTE_NW; ++w) {
            wbase[w][n] = b;
            b += wtot[w][n];
        }
    }
    __syncthreads();
    int run[2] = {wbase[wave][0], wbase[wave][1]};
    for (int g = g0 + wave; g < g1; g += ROUTE_NW) {
        int net, off, c;
        fetch(g, net, off, c);
        int base = 0;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int mine = net == n ? c : 0;
            const int incl = wave_incl_scan(mine);
            if (net == n) base = run[n] + incl - mine;
            run[n] += lane63(incl);
        }
        uint64_t some = ballot(c > 0);
        while (some) {   // (wave-uniform: a ballot)
            const int k = __ffsll((unsigned long long)some) - 1;
            some &= some - 1;
            const int kc = __builtin_amdgcn_readlane(c, k), kn = __builtin_amdgcn_readlane(net, k),
                      kb = __builtin_amdgcn_readlane(base, k), koff = __builtin_amdgcn_readlane(off, k);
            int32_t* lst = kn ? a.rlist[1] : a.rlist[0];
            for (int i = lane; i < kc; i += 64)
                if (kb + i < a.reply_cap) lst[kb + i] = koff + i;
        }
    }
}

// ids[i] in {0, 1} -> row i on list ids[i] (bgx_value_boards_routed)
__global__ __launch_bounds__(256) void route_ids_kernel(const uint8_t* __restrict__ ids, int n, int32_t* list0,
                                                        int32_t* list1, unsigned* ctr) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int lane = lane_id();
    const bool live = i < n;
    const int id = live ? (int)(ids[i] & 1u) : 0;
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        const uint64_t m = ballot(live && id == net);
        int b = 0;
        if (lane == 0 && m) b = (int)atomicAdd(ctr + net, (unsigned)__popcll(m));
        b = uniform(b);
        if (live && id == net) (net ? list1 : list0)[b + mask_prefix(m)] = i;
    }
}

}  // namespace bgx

extern "C" hipError_t bgx_launch_mlp_routed(const bgx::MatchMlpArgs* args, hipStream_t stream) {
    // per device: the CU count and the kernels' dynamic-LDS opt-in (bgx_launch_mlp)
    static int n_cu_dev[64] = {0};
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || cur < 0 || cur >= 64) cur = 0;
    int& n_cu = n_cu_dev[cur];
    const int lds = bgx::NFRAG * 16 + 256 * 16 + 128 * 4 + 16;   // + the claim slots
    if (!n_cu) {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, cur) != hipSuccess || cu <= 0) cu = 256;
        if (hipFuncSetAttribute((const void*)bgx::mlp_kernel_routed<1, 16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds) != hipSuccess ||
            hipFuncSetAttribute((const void*)bgx::mlp_kernel_routed<2, 8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds) != hipSuccess)
            return hipErrorInvalidValue;
        n_cu = cu;
    }
    if (args->n_max <= 0 || args->list_cap <= 0) return hipErrorInvalidValue;
    const int nt = args->nt == 2 ? 2 : 1;
    const int nw = nt == 2 ? 8 : 16;
    int blocks = n_cu;
    if (args->n_hint > 0) {
        // at most this many tiles over the two lists (each may end in a partial
        // tile); one more workgroup so that both starting networks are taken
        const int tiles = (args->n_hint + 32 * nt - 1) / (32 * nt) + 1;
        const int need = (tiles + nw - 1) / nw + 1;
        if (need < blocks) blocks = need;
    }
    if (nt == 2)
        hipLaunchKernelGGL((bgx::mlp_kernel_routed<2, 8>), dim3(blocks), dim3(512), lds, stream, *args);
    else
        hipLaunchKernelGGL((bgx::mlp_kernel_routed<1, 16>), dim3(blocks), dim3(1024), lds, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_route_root(const bgx::MatchRouteArgs* args, hipStream_t stream) {
    if (args->L <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgx::route_root_kernel, dim3((args->L + 255) / 256), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_route_reply(const bgx::MatchRouteArgs* args, hipStream_t stream) {
    // K = 4: the job count is known here; K = all: it is read on the device, so
    // the grid covers the capacity; at most 256 workgroups, each with a
    // contiguous span of the jobs
    const long long jobs = args->n_units_dev ? (long long)args->n_jobs_max : (long long)args->n_jobs;
    if (jobs <= 0) return hipSuccess;
    long long blocks = (jobs + 64 * bgx::ROUTE_NW - 1) / (64 * bgx::ROUTE_NW);
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(bgx::route_reply_kernel, dim3((unsigned)blocks), dim3(64 * bgx::ROUTE_NW), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t bgx_launch_route_ids(const uint8_t* ids, int n, int32_t* list0, int32_t* list1, unsigned* ctr,
                                           hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgx::route_ids_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ids, n, list0, list1, ctr);
    return hipGetLastError();
}
