// bgx_rollout.hip — the rollout tally: finished-episode headers -> per-position
// result counts, on the device (bgx_rollout_tally, include/bgx.h).
//
// A rollout plays given positions out many times (bgx_engine_set_start: global
// lane g plays position g % n_pos in every episode) and asks how often the
// player on roll wins what. One thread per header adds to counts[pos][8] (u64),
// pos = header lane % n_pos, seen from the player on roll at the start:
//   0..2 regular / gammon / backgammon wins of the player on roll,
//   3..5 the same for the other player,
//   6    unfinished games (win type 0: the game hit max_steps),
//   7    the sum of the headers' env steps.
// Headers with episode no. >= max_episode are skipped (every lane contributes
// exactly max_episode games, bgx/match.py's rule). Integer adds only: the totals
// do not depend on the order, and calls accumulate into counts.
#include "bgx_device.h"
#include "bgx_kernels.h"

namespace bgx {

// With few positions every header of a harvest lands on the same few words
// (one position: seven), so a workgroup first counts into an LDS histogram and
// then issues one global 64-bit atomic per non-zero bin. The LDS form is used
// while the n_pos * 8 bins fit 2,048 u64 words (16 KiB of the workgroup's LDS:
// n_pos <= 256). Beyond that a harvest's headers spread over more than 2,048
// words, same-address contention is low, and the threads add to global memory
// directly.
constexpr int TALLY_LDS_BINS = 2048;
constexpr int TALLY_THREADS = 256;

__global__ __launch_bounds__(TALLY_THREADS) void rollout_tally_kernel(const uint32_t* __restrict__ hdr, int n,
                                                                      const uint8_t* __restrict__ start_player,
                                                                      int n_pos, uint32_t max_episode,
                                                                      unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long bins[TALLY_LDS_BINS];
    const int nb = n_pos * 8, t = (int)threadIdx.x;
    const bool lds = n_pos <= TALLY_LDS_BINS / 8;   // uniform over the grid
    if (lds) {
        for (int k = t; k < nb; k += TALLY_THREADS) bins[k] = 0ull;
        __syncthreads();
    }
    for (int idx = (int)blockIdx.x * TALLY_THREADS + t; idx < n; idx += (int)gridDim.x * TALLY_THREADS) {
        const uint4* h = (const uint4*)(hdr + (size_t)idx * EP_WORDS);   // headers are 16-byte aligned (64 B each)
        const uint4 a = h[0], b = h[1];   // global lane, episode no., ., . | env steps, win_type | winner << 8 | ., ., .
        if (a.y >= max_episode) continue;
        const uint32_t pos = a.x % (uint32_t)n_pos;
        const uint32_t wt = b.y & 0xFFu, winner = (b.y >> 8) & 1u;
        const uint32_t slot = wt == 0u ? 6u : (winner == (uint32_t)(start_player[pos] & 1) ? 0u : 3u) + (wt < 3u ? wt : 3u) - 1u;
        // two branches, not one pointer chosen at run time: the LDS form compiles
        // to LDS atomics, the other to global ones (a shared pointer gives flat)
        if (lds) {
            atomicAdd(&bins[pos * 8u + slot], 1ull);
            atomicAdd(&bins[pos * 8u + 7u], (unsigned long long)b.x);
        } else {
            atomicAdd(counts + pos * 8u + slot, 1ull);
            atomicAdd(counts + pos * 8u + 7u, (unsigned long long)b.x);
        }
    }
    if (lds) {
        __syncthreads();
        for (int k = t; k < nb; k += TALLY_THREADS) {
            const unsigned long long v = bins[k];
            if (v) atomicAdd(counts + k, v);
        }
    }
}

}  // namespace bgx

extern "C" hipError_t bgx_launch_rollout_tally(const uint32_t* headers, int n_headers, const uint8_t* start_player,
                                               int n_pos, uint32_t max_episode, unsigned long long* counts,
                                               hipStream_t stream) {
    if (n_headers <= 0) return hipSuccess;
    int blocks = (n_headers + bgx::TALLY_THREADS - 1) / bgx::TALLY_THREADS;
    if (blocks > 1024) blocks = 1024;   // then a grid-stride loop: fewer, fuller LDS flushes
    hipLaunchKernelGGL(bgx::rollout_tally_kernel, dim3(blocks), dim3(bgx::TALLY_THREADS), 0, stream, headers,
                       n_headers, start_player, n_pos, max_episode, counts);
    return hipGetLastError();
}
