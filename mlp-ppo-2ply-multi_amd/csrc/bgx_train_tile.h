// bgx_train_tile.h — what the trainer units share apart from the MFMA code, so
// that the host emulation (tests/cpuwave/after_emu.cpp, feature_emu.cpp)
// compiles it alone, plain loads and stores: the live-feature rule of the batched
// backward kernel (tb_field, tb_lut_entry), the index launch and the tile
// loaders of the batched update (bgx_train_batch.hip).
//
// Afterstate rows (bgx_td_afterstate_update_batched). The row of record s of an
// episode [a, b) is the board the mover leaves, under the mover's indicator:
//   src    = words 0..6 of record s + 1             if s < b - 1
//            words 6..12 of the episode's header    if s = b - 1
//   A_s[k] = src[k], k = 0..5;  A_s[6] = (src[6] & 0xFFFF) | m_s << 16,
//   m_s = (record s word 11 >> 9) & 1
// (whatever indicator src carries is ignored). The index launch, which walks
// each episode's records anyway, writes where a record's row comes from:
//   srcidx[s] = s + 1 (always >= 1)   the next record
//               ~e    (negative)      header e, on the episode's last record
//               0     (the fill)      a record in no episode: its own words
// and the loader reads rec[12 srcidx + k] or hdr[16 e + 6 + k]. s + 1 < b <=
// n_rec and e < n_eps, so nothing is read at or past rec + 12 n_rec or
// hdr + 16 n_eps, though a tile's last record may take its row from the next
// tile's first one. No afterstate row is ever stored in HBM.
// The row's address depends on srcidx[s], a second memory round trip per tile
// that nothing would hide (the loader runs between two barriers). So a workgroup
// keeps the tile's 128 source indices in LDS (tb_stage_src): those of its first
// tile are requested before its loop, those of the next tile when the current
// one's rows are in, and land while its MFMA chains run. They go global -> LDS
// with no register in between: the backward kernel is at its register cap.
#pragma once
#include "bgx_device.h"
#include "bgx_kernels.h"

namespace bgx {

constexpr int TB_T = 256;                          // threads of every launch of the batched update
constexpr int TB_TILE = TRAIN_BATCH_TILE;          // records per tile

// The live encoding (immutable_board.py:86-128) of packed words w[0..6], in two
// steps: the field that feature k reads, n = (w[word] >> shift) & mask (a point's
// checker count, a bar / off count, or the indicator bit; k >= 198: mask 0), and
// the feature's value as a function of n.
struct TbField {
    int word, shift, mask;
};
BGX_DEV TbField tb_field(int k) {
    if (k < 192) {
        const int pl = k / 96, i = (k - 96 * pl) >> 2;
        return {3 * pl + (i >> 3), (i & 7) * 4, 15};
    }
    if (k < 196) {   // bar1, off1, bar2, off2
        const int q = k - 192;
        return {6, 4 * (q >> 1) + ((q & 1) ? 8 : 0), 15};
    }
    return {6, 16, k < 198 ? 1 : 0};
}
BGX_DEV float tb_lut_entry(int k, int n) {
    if (k >= 198) return 0.0f;
    if (k >= 196) return n == k - 196 ? 1.0f : 0.0f;
    if (k >= 192) return (k & 1) ? (float)((double)n / 15.0) : (float)n * 0.5f;
    switch (k & 3) {
        case 0: return n >= 1 ? 1.0f : 0.0f;
        case 1: return n >= 2 ? 1.0f : 0.0f;
        case 2: return n >= 3 ? 1.0f : 0.0f;
        default: return n > 3 ? (float)(n - 3) * 0.5f : 0.0f;
    }
}
// feature f of packed words w[0..6]: the two composed. bgx_train.hip's
// live_feature states the same rule in one function of its own: as this
// composition its chunk loader compiled to a sequential kernel 2.4 % slower
// (profiles/train_refactor/README.md)
BGX_DEV float tb_feature(const uint32_t* w, int f) {
    const TbField fd = tb_field(f);
    return tb_lut_entry(f, (int)((w[fd.word] >> fd.shift) & (uint32_t)fd.mask));
}

// one thread per episode: info[s] = T_e | last << 31 for its records (offs
// clamped to [0, n_rec]), the Adam step count + 1; AFTER: srcidx[s] as above
template <bool AFTER>
BGX_DEV void tb_index(const TrainBatchArgs& a) {
    const int e = (int)(blockIdx.x * TB_T + threadIdx.x);
    if (e == 0) *a.step += 1;
    if (e >= a.n_eps) return;
    int lo = a.offs[e], hi = a.offs[e + 1];
    lo = lo < 0 ? 0 : (lo > a.n_rec ? a.n_rec : lo);
    hi = hi < 0 ? 0 : (hi > a.n_rec ? a.n_rec : hi);
    const int T = hi - lo;
    for (int s = lo; s < hi; ++s) {
        a.info[s] = T | (s == hi - 1 ? (int)0x80000000u : 0);
        if constexpr (AFTER) a.srcidx[s] = s == hi - 1 ? ~e : s + 1;
    }
}

// the tile's records into LDS: words 0..6 (the board before the move, the
// mover's flag) and the reward in slot 7; zeros past the last record
BGX_DEV void tb_load_tile(const uint32_t* rec, int n_rec, long long base, uint32_t (*RW)[8]) {
    for (int idx = (int)threadIdx.x; idx < TB_TILE * 8; idx += TB_T) {
        const int r = idx >> 3, k = idx & 7;
        const long long s = base + r;
        RW[r][k] = s < n_rec ? rec[(size_t)s * 12 + (k < 7 ? k : 9)] : 0u;
    }
}

// SRC[r] (LDS, [TB_TILE]) = srcidx[base + r] for the tile at `base`: thread t < TB_TILE requests its entry,
// lane l of a wave into the wave's 64-entry slice + l; entries past the last record stay as they are and
// are never read. Before SRC is read the caller waits for the requests (vmcnt(0)) and passes a barrier
BGX_DEV void tb_stage_src(const int32_t* srcidx, int n_rec, long long base, int32_t* SRC) {
    const int t = (int)threadIdx.x;
    if (t < TB_TILE && base + t < n_rec)
        __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(void*)(srcidx + base + t),
                                         (__attribute__((address_space(3))) void*)(void*)(SRC + (t & ~63)), 4, 0, 0);
}

// the same with the afterstate row A_s in words 0..6; the reward stays in slot 7.
// src_tile[r] = srcidx[base + r] (tb_stage_src)
BGX_DEV void tb_load_tile_after(const uint32_t* rec, const uint32_t* hdr, const int32_t* src_tile, int n_rec,
                                long long base, uint32_t (*RW)[8]) {
    for (int idx = (int)threadIdx.x; idx < TB_TILE * 8; idx += TB_T) {
        const int r = idx >> 3, k = idx & 7;
        const long long s = base + r;
        uint32_t w = 0u;
        if (s < n_rec) {
            const uint32_t* own = rec + (size_t)s * 12;
            if (k == 7) {
                w = own[9];
            } else {
                const int v = src_tile[r];
                const uint32_t* src = v > 0 ? rec + (size_t)v * 12 : (v < 0 ? hdr + (size_t)(~v) * 16 + 6 : own);
                w = src[k];
                if (k == 6) w = (w & 0xFFFFu) | (((own[11] >> 9) & 1u) << 16);
            }
        }
        RW[r][k] = w;
    }
}

}  // namespace bgx
