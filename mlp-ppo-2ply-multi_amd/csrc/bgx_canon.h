// bgx_canon.h — a harvest in canonical order, on the device (bgx_canon.hip
// launches the bodies; the host emulation of tests/cpuwave/ compiles them too;
// the entry point is bgx_harvest_canonical, bgx_host_canon.cpp).
//
// A harvest's episodes arrive in the device's completion order. The two
// launches here re-lay them by the key (header word 0 = global lane, word 1 =
// episode number), ascending and unsigned, so that what the update reads is a
// function of the set of episodes only:
//   * the index launch, one workgroup: a per-lane histogram, an exclusive scan
//     over the lanes, a scatter of the episodes into their lane's segment, each
//     episode's rank within its segment by episode number (a count of smaller
//     keys: no order of arrival survives it), and both sets of offsets
//     (episode_offsets_body's scan over the headers as they stand and as
//     permuted, in one pass). Up to CN_LDS_LANES lanes the histogram lives in
//     LDS, beyond that in the workspace;
//   * the copy launch, a wave per episode: its header and its records, 16
//     bytes per lane.
// Integer atomics only (the histogram's and the scatter's adds, the status
// OR): the final bytes do not depend on their order. Every index read back
// from memory is clamped, so nothing outside the arrays is touched whatever
// the headers hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgx_pack.h"

namespace bgx {

constexpr int CN_INDEX_THREADS = PK_OFFS_THREADS;   // the index launch: one workgroup (episode_offsets_body's size)
constexpr int CN_COPY_THREADS = 256;                // the copy launch: 4 waves, an episode each
constexpr int CN_COPY_MAX_BLOCKS = 2048;            // ... the waves stride over the rest
constexpr int CN_LDS_LANES = 4096;                  // histogram and segment starts in LDS up to here (32 KB)

// *d_status bits, BGX_CANON_* of include/bgx.h
enum : uint32_t { CN_LANE_RANGE = 1u, CN_DUPLICATE = 2u, CN_RECORDS = 4u };

// the workspace, int32 words: start [lanes + 1] | cur [lanes] | seg_idx [n] |
// seg_key [n] | perm [n] | in_offs [n + 1]
struct CanonWork {
    int32_t* start;      // segment starts, start[lanes] = episodes with a lane in range
    int32_t* cur;        // the histogram, then each segment's fill cursor
    int32_t* seg_idx;    // the episodes by segment, any order within one
    uint32_t* seg_key;   // ... their episode numbers
    int32_t* perm;       // perm[k]: the input episode that becomes output episode k
    int32_t* in_offs;    // the input harvest's offsets
};
inline uint64_t canon_work_words(int n_eps, int lanes) {
    return 2ull * (uint64_t)lanes + 1ull + 4ull * (uint64_t)n_eps + 1ull;
}
inline uint64_t canon_work_bytes(int n_eps, int lanes) { return (canon_work_words(n_eps, lanes) * 4ull + 15ull) & ~15ull; }
inline CanonWork canon_work(void* base, int n_eps, int lanes) {
    int32_t* w = (int32_t*)base;
    CanonWork c;
    c.start = w;
    c.cur = c.start + (size_t)lanes + 1;
    c.seg_idx = c.cur + (size_t)lanes;
    c.seg_key = (uint32_t*)(c.seg_idx + (size_t)n_eps);
    c.perm = (int32_t*)c.seg_key + (size_t)n_eps;
    c.in_offs = c.perm + (size_t)n_eps;
    return c;
}

__device__ inline int32_t cn_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup of CN_INDEX_THREADS: start[l] = cur[l] = the sum of cur[0 .. l)
// for l < lanes, start[lanes] = the total; 1,024 lanes at a time, as
// episode_offsets_body scans. cur was filled by atomics: it is read at agent
// scope, past the L1.
__device__ inline void canon_scan_lanes(int32_t* cur, int lanes, int32_t* start) {
    constexpr int NW = CN_INDEX_THREADS / 64;
    __shared__ int32_t s_tot[NW];
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    int32_t carry = 0;
    for (int base = 0; base < lanes; base += CN_INDEX_THREADS) {   // lanes is uniform: every thread makes every trip
        const int i = base + t;
        const int32_t c = i < lanes ? __hip_atomic_load(&cur[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        int32_t v = c;
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
        if (i < lanes) {
            const int32_t ex = carry + before + v - c;
            start[i] = ex;
            cur[i] = ex;
        }
        carry += all;
        __syncthreads();   // s_tot is rewritten by the next chunk
    }
    if (t == 0) start[lanes] = carry;
}

// One workgroup of CN_INDEX_THREADS, n >= 1: episode_offsets_body's scan on two
// sequences at once, in_offs over word 3 of the headers as they stand and
// out_offs over word 3 of header perm[0], perm[1], ...; the two run as the
// halves of one 64-bit sum (a harvest's record count stays below 2^31, so the
// low half never carries; where the headers break that, CN_RECORDS is set and
// in_offs, the low half, is still the sum modulo 2^32).
__device__ inline void canon_offsets_pair(const uint32_t* __restrict__ hdr, const int32_t* perm, int n,
                                          int32_t* in_offs, int32_t* out_offs) {
    constexpr int NW = CN_INDEX_THREADS / 64;
    __shared__ unsigned long long s_tot[NW];
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) {
        in_offs[0] = 0;
        out_offs[0] = 0;
    }
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += CN_INDEX_THREADS) {   // n is uniform: every thread makes every trip
        const int i = base + t;
        unsigned long long v = 0;
        if (i < n) {
            const int32_t p = cn_clamp(perm[i], 0, n - 1);
            v = (unsigned long long)hdr[(size_t)i * 16 + 3] | (unsigned long long)hdr[(size_t)p * 16 + 3] << 32;
        }
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long u = __shfl(v, (lane - d) & 63);
            if (lane >= d) v += u;
        }
        if (lane == 63) s_tot[wv] = v;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (int w = 0; w < NW; ++w) {
            const unsigned long long x = s_tot[w];
            all += x;
            if (w < wv) before += x;
        }
        if (i < n) {
            const unsigned long long s = carry + before + v;
            in_offs[i + 1] = (int32_t)(uint32_t)s;
            out_offs[i + 1] = (int32_t)(uint32_t)(s >> 32);
        }
        carry += all;
        __syncthreads();   // s_tot is rewritten by the next chunk
    }
}

// The index launch: one workgroup of CN_INDEX_THREADS, n >= 1. hdr [n][16] ->
// w.perm, w.in_offs and out_offs [n + 1]; ORs CN_* into *status. LDS: the
// histogram and the starts in LDS (lanes <= CN_LDS_LANES), else in w.cur /
// w.start.
template <bool LDS>
__device__ inline void canon_index_body(const uint32_t* __restrict__ hdr, int n, int n_records, uint32_t lane_base,
                                        int lanes, int32_t* out_offs, uint32_t* status, CanonWork w) {
    constexpr int T = CN_INDEX_THREADS;
    __shared__ int32_t s_start[LDS ? CN_LDS_LANES + 1 : 1], s_cur[LDS ? CN_LDS_LANES : 1];
    int32_t* const start = LDS ? s_start : w.start;
    int32_t* const cur = LDS ? s_cur : w.cur;
    const int t = (int)threadIdx.x;
    uint32_t st = 0;
    for (int l = t; l < lanes; l += T) cur[l] = 0;
    for (int i = t; i < n; i += T) w.perm[i] = i;   // a permutation whatever follows (episodes of no lane keep their place)
    __syncthreads();
    // the histogram
    for (int i = t; i < n; i += T) {
        const uint32_t rel = hdr[(size_t)i * 16] - lane_base;
        if (rel < (uint32_t)lanes) atomicAdd(&cur[rel], 1);
        else st |= CN_LANE_RANGE;
        if (hdr[(size_t)i * 16 + 3] > (uint32_t)n_records) st |= CN_RECORDS;
    }
    __syncthreads();
    canon_scan_lanes(cur, lanes, start);
    __syncthreads();
    // the scatter: each segment in the order of arrival at its cursor
    for (int i = t; i < n; i += T) {
        const uint32_t rel = hdr[(size_t)i * 16] - lane_base;
        if (rel < (uint32_t)lanes) {
            const int32_t pos = atomicAdd(&cur[rel], 1);
            if ((uint32_t)pos < (uint32_t)n) {
                w.seg_idx[pos] = i;
                w.seg_key[pos] = hdr[(size_t)i * 16 + 1];
            }
        }
    }
    __syncthreads();
    // the rank of every episode in its segment: the keys below its own (an equal
    // key is a duplicate; the earlier slot goes first, so perm stays a permutation)
    const int32_t total = cn_clamp(start[lanes], 0, n);
    for (int pos = t; pos < total; pos += T) {
        const int32_t idx = cn_clamp(w.seg_idx[pos], 0, n - 1);
        const uint32_t key = w.seg_key[pos];
        const uint32_t rel = hdr[(size_t)idx * 16] - lane_base;
        if (rel >= (uint32_t)lanes) continue;   // (it was scattered, so it is not)
        const int32_t a = cn_clamp(start[rel], 0, total), b = cn_clamp(start[rel + 1], a, total);
        int32_t rank = 0;
        bool dup = false;
        for (int32_t j = a; j < b; ++j) {
            const uint32_t k = w.seg_key[j];
            rank += (k < key || (k == key && j < pos)) ? 1 : 0;
            dup |= k == key && j != pos;
        }
        if (a + rank < total) w.perm[a + rank] = idx;
        if (dup) st |= CN_DUPLICATE;
    }
    __syncthreads();
    canon_offsets_pair(hdr, w.perm, n, w.in_offs, out_offs);
    if (t == 0 && w.in_offs[n] != n_records) st |= CN_RECORDS;   // (thread 0 wrote it itself when n = 0)
    if (st) atomicOr(status, st);
}

// The copy launch: a grid of CN_COPY_THREADS workgroups, wave k, k + waves, ...
// copies header perm[k] of hdr [n][16] to out_hdr [k] (its first four lanes) and
// that episode's records from rec [n_records][12] to out_rec [n_records][12],
// 16 bytes per lane and four of them in flight; all four arrays 16-byte
// aligned. Source and destination ranges are clamped to [0, n_records].
__device__ inline void canon_copy_body(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ rec, int n,
                                       int n_records, const int32_t* __restrict__ perm,
                                       const int32_t* __restrict__ in_offs, const int32_t* __restrict__ out_offs,
                                       uint32_t* __restrict__ out_hdr, uint32_t* __restrict__ out_rec) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int k = wave; k < n; k += n_waves) {
        const int32_t p = cn_clamp(perm[k], 0, n - 1);
        if (lane < 4) ((uint4*)out_hdr)[(size_t)k * 4 + lane] = ((const uint4*)hdr)[(size_t)p * 4 + lane];
        const int32_t s0 = cn_clamp(in_offs[p], 0, n_records), s1 = cn_clamp(in_offs[p + 1], s0, n_records);
        const int32_t d0 = cn_clamp(out_offs[k], 0, n_records);
        const int32_t len = s1 - s0 < n_records - d0 ? s1 - s0 : n_records - d0;
        const uint4* __restrict__ src = (const uint4*)rec + (size_t)s0 * 3;
        uint4* __restrict__ dst = (uint4*)out_rec + (size_t)d0 * 3;
        const int32_t n4 = len * 3;   // 48-byte records
        for (int32_t j = lane; j < n4; j += 256) {
            const bool b1 = j + 64 < n4, b2 = j + 128 < n4, b3 = j + 192 < n4;
            const uint4 v0 = src[j];
            const uint4 v1 = src[b1 ? j + 64 : j], v2 = src[b2 ? j + 128 : j], v3 = src[b3 ? j + 192 : j];
            dst[j] = v0;
            if (b1) dst[j + 64] = v1;
            if (b2) dst[j + 128] = v2;
            if (b3) dst[j + 192] = v3;
        }
    }
}

}  // namespace bgx

extern "C" {
// headers [n][16], n >= 1 -> the workspace's perm and in_offs, out_offs [n + 1], *status (one workgroup)
hipError_t bgx_launch_canon_index(const uint32_t* headers, int n, int n_records, uint32_t lane_base, int lanes,
                                  int32_t* out_offs, uint32_t* status, bgx::CanonWork w, hipStream_t stream);
// headers, records [n_records][12] -> out_headers, out_records, by the index launch's perm / in_offs / out_offs
hipError_t bgx_launch_canon_copy(const uint32_t* headers, const uint32_t* records, int n, int n_records,
                                 bgx::CanonWork w, const int32_t* out_offs, uint32_t* out_headers,
                                 uint32_t* out_records, hipStream_t stream);
}
