// bgx_abi.cpp — the extern "C" boundary of libbgx.so (declared in include/bgx.h):
// the error string, and the stateless operations with their scratch pool.
//
// Host-side orchestration only: argument checks, device buffers, launches and
// error reporting. All game logic runs in the HIP kernels (bgx_movegen.hip,
// bgx_mlp.hip, bgx_encode.hip, bgx_engine.hip). The engine's entry points are
// in bgx_host_engine.cpp (lifetime, modes) and bgx_host_step.cpp (stepping,
// harvest), the copies in bgx_host_copy.cpp.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "bgx_domain.h"
#include "bgx_frag.h"
#include "bgx_host.h"
#include "bgx_pack.h"

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

using bgx_frag::build_fragments;
using bgx_frag::NFRAG;

int net_upload(bgx_net* n, const float* W1, const float* b1, const float* w2, const float* b2) {
    // the scheme's input limit (include/bgx.h), before anything of `n` changes:
    // a rejected upload leaves the previous network in force
    bool nonfinite = false;
    int at = 0;
    if (const char* bad = bgx_frag::unrepresentable(W1, b1, w2, b2, &nonfinite, &at)) {
        if (nonfinite) return fail(BGX_E_ARG, "weights: %s[%d] is not finite", bad, at);
        return fail(BGX_E_ARG, "weights: %s[%d] = %g: max|log2(e) w| must stay below 2^26 (split-fp16 scaling limit)",
                    bad, at, (double)(bad[0] == 'W' ? W1 : b1)[at]);
    }
    std::vector<uint16_t> frag;
    const int e = build_fragments(W1, b1, frag);
    if (e == bgx_frag::kBadWeights) return fail(BGX_E_ARG, "weights: W1 / b1 outside the split-fp16 scaling limit");
    n->feat_scale = (float)std::ldexp(1.0, -e);
    HIP_TRY(hipMemcpy(n->W1, W1, 128 * 198 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n->b1, b1, 128 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n->w2, w2, 128 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n->wfrag, frag.data(), frag.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n->rowc, w2, 128 * 4, hipMemcpyHostToDevice));
    n->b2 = b2[0];
    return BGX_OK;
}

// ---------------------------------------------------------------- stateless-call scratch
// The stateless entry points need a few device words (validation flags,
// movegen overflow counters), an overflow list, a fallback workspace and (for
// bgx_value_boards) packed boards. Each call leases one scratch set from a
// per-device pool: a set is handed out only when no call holds it and the
// stream work of its last user has finished (an event recorded at release),
// so calls from several host threads or on several streams never share one.
// Sets are kept for reuse; the pool grows to the peak number of calls in flight.
namespace {

struct Scratch {
    int dev = -1;
    bool busy = false;
    Event done;
    DevBuf<unsigned> words;     // [16]: [0..1] validation flags, [2] ovf count, [3] err flags
    HostWords h_words;          // pinned host copy of words[0..1]
    DevBuf<int32_t> ovf;        // movegen overflow list (lazy)
    DevBuf<uint32_t> ws;        // movegen fallback workspace (lazy)
    DevBuf<uint32_t> packed;    // bgx_value_boards packed boards, 8 words each (lazy, grows)
    DevBuf<int32_t> lists;      // bgx_value_boards_routed: two row-index lists, count() / 2 entries each (lazy, grows)
};

constexpr int SC_OVF_CAP = 1 << 16, SC_WS_WAVES = 256, SC_WS_SLOTS = 16384;

std::mutex g_pool_mu;
std::vector<Scratch*> g_pool;   // kept for the life of the process

struct Lease {
    Scratch* sc = nullptr;
    hipStream_t stream = nullptr;
    ~Lease() {
        if (!sc) return;
        (void)hipEventRecord(sc->done, stream);
        std::lock_guard<std::mutex> g(g_pool_mu);
        sc->busy = false;
    }
};

int lease_scratch(hipStream_t stream, Lease& L) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (Scratch* sc : g_pool) {
            if (sc->dev != dev || sc->busy || hipEventQuery(sc->done) != hipSuccess) continue;
            sc->busy = true;
            L.sc = sc;
            L.stream = stream;
            return BGX_OK;
        }
    }
    std::unique_ptr<Scratch> sc(new Scratch());
    sc->dev = dev;
    sc->busy = true;
    if (sc->words.alloc(16)) return BGX_E_HIP;
    if (hipHostMalloc((void**)sc->h_words.put(), 4 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(sc->done.put(), hipEventDisableTiming) != hipSuccess)
        return fail(BGX_E_HIP, "scratch: pinned buffer / event creation failed");
    HIP_TRY(hipMemset(sc->words, 0, sc->words.bytes()));
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        g_pool.push_back(sc.get());
    }
    L.sc = sc.release();
    L.stream = stream;
    return BGX_OK;
}

int lease_movegen_space(Scratch* sc) {
    if (!sc->ovf && sc->ovf.alloc(SC_OVF_CAP)) return BGX_E_HIP;
    if (!sc->ws && sc->ws.alloc((size_t)SC_WS_WAVES * 5 * SC_WS_SLOTS)) return BGX_E_HIP;
    return BGX_OK;
}

// the input-domain check (include/bgx.h, BGX_BADF_*): flags into the lease's
// words, copied to pinned memory, one stream synchronization
int check_domain(Scratch* sc, const uint8_t* boards, const uint8_t* player, const uint8_t* dice, int n,
                 hipStream_t s, uint32_t* flags, int32_t* first) {
    HIP_TRY(bgx_launch_validate(boards, player, dice, n, sc->words, s));
    HIP_TRY(hipMemcpyAsync(sc->h_words, sc->words, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *flags = sc->h_words[0];
    *first = sc->h_words[0] ? (int32_t)sc->h_words[1] : -1;
    return BGX_OK;
}

int require_domain(const char* what, Scratch* sc, const uint8_t* boards, const uint8_t* player,
                   const uint8_t* dice, int n, hipStream_t s) {
    uint32_t f = 0;
    int32_t first = -1;
    if (int rc = check_domain(sc, boards, player, dice, n, s, &f, &first)) return rc;
    if (f)
        return fail(BGX_E_ARG,
                    "%s: input %d is outside the board domain (bits 0x%x: 1 a point held by both players, 2 more "
                    "than 15 checkers of a player, 4 a count above 15, 8 a die outside 1..6, 16 a player not 0/1)",
                    what, first, f);
    return BGX_OK;
}

// The stateless 2-ply reply expansion (bgx_reply_moves, bgx_two_ply_sampled):
// every legal reply of the opponent to each of n boards for the 21 distinct
// rolls, as packed rows out[cap][8] (word 7 = the root slot, job / 21) with
// off / cnt per (board, roll) job. `after(roots, n_rows)` enqueues the
// caller's own launches on the stream (roots: the n packed boards; n_rows: the
// device count of reply rows); then the call's one synchronization. Returns
// the movegen's overflow flag word (>= 0), or BGX_E_HIP (the caller words the
// message).
template <typename After>
int expand_replies(const uint8_t* d_boards, const uint8_t* d_opponent, int n, uint32_t* d_out, int cap,
                   int32_t* d_off, int32_t* d_cnt, hipStream_t s, After&& after) {
    constexpr int ws_waves = 64, ws_slots = 16384, ovf_cap = 1 << 16;
    DevBuf<uint8_t> mover;
    DevBuf<uint32_t> rows, ws;
    DevBuf<unsigned> ctr;   // [0] reply rows, [2] overflow count, [3] error flags
    DevBuf<int32_t> ovf;
    if (mover.alloc(n) || rows.alloc((size_t)n * 8) || ctr.alloc(8) || ovf.alloc(ovf_cap) ||
        ws.alloc((size_t)ws_waves * 5 * ws_slots))
        return BGX_E_HIP;
    // the candidate board's indicator = the player who just moved = 1 - opponent
    std::vector<uint8_t> hm(n);
    if (hipMemcpy(hm.data(), d_opponent, n, hipMemcpyDeviceToHost) != hipSuccess) return BGX_E_HIP;
    for (int i = 0; i < n; ++i) hm[i] = (uint8_t)(1 - (hm[i] & 1));
    if (hipMemcpy(mover, hm.data(), n, hipMemcpyHostToDevice) != hipSuccess) return BGX_E_HIP;
    if (hipMemsetAsync(ctr, 0, ctr.bytes(), s) != hipSuccess) return BGX_E_HIP;
    if (bgx_launch_pack(d_boards, mover, n, rows, s) != hipSuccess) return BGX_E_HIP;
    bgx::MovegenArgs b{};
    b.n_jobs = n * 21;
    b.in_mode = bgx::IN_TWOPLY;
    b.in_packed = rows;
    b.out_mode = bgx::OUT_PACKED_FLAT;
    b.out_packed = d_out;
    b.flat_count = ctr;
    b.flat_cap = cap;
    b.flat_chunk = 256;
    b.job_off = d_off;
    b.job_cnt = d_cnt;
    set_fallback(b, ctr + 2, ovf, ovf_cap, ws, ws_waves, ws_slots, ctr + 3);
    if (bgx_launch_movegen(&b, s) != hipSuccess) return BGX_E_HIP;
    if (!after(rows.get(), ctr.get())) return BGX_E_HIP;
    unsigned flags = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(&flags, ctr + 3, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return BGX_E_HIP;
    return (int)flags;
}

}  // namespace

extern "C" {

int bgx_abi_version(void) { return BGX_ABI_VERSION; }
const char* bgx_last_error(void) { return g_err.c_str(); }

int bgx_check_boards_host(const uint8_t* h_boards, const uint8_t* h_player, const uint8_t* h_dice, int n,
                          uint32_t* h_flags, int32_t* h_first_bad) {
    return guarded("bgx_check_boards_host", [&]() -> int {
        if (n < 0 || !h_flags || !h_first_bad || (n > 0 && !h_boards))
            return fail(BGX_E_ARG, "bgx_check_boards_host: bad arguments (n=%d)", n);
        uint32_t f = 0;
        int32_t first = -1;
        for (int i = 0; i < n; ++i) {
            const unsigned b = bgx::domain_bits(h_boards + (size_t)i * 52, h_player ? (int)h_player[i] : -1,
                                                h_dice ? h_dice + 2 * (size_t)i : nullptr);
            if (b && first < 0) first = i;
            f |= b;
        }
        *h_flags = f;
        *h_first_bad = first;
        return BGX_OK;
    });
}

int bgx_check_boards(const uint8_t* d_boards, const uint8_t* d_player, const uint8_t* d_dice, int n,
                     uint32_t* h_flags, int32_t* h_first_bad, void* stream) {
    return guarded("bgx_check_boards", [&]() -> int {
        if (n < 0 || !h_flags || !h_first_bad || (n > 0 && !d_boards))
            return fail(BGX_E_ARG, "bgx_check_boards: bad arguments (n=%d)", n);
        *h_flags = 0;
        *h_first_bad = -1;
        if (n == 0) return BGX_OK;
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        Lease L;
        if (int rc = lease_scratch((hipStream_t)stream, L)) return rc;
        return check_domain(L.sc, d_boards, d_player, d_dice, n, (hipStream_t)stream, h_flags, h_first_bad);
    });
}

int bgx_movegen(const uint8_t* d_boards, const uint8_t* d_player, const uint8_t* d_dice, int n,
                uint8_t* d_out_boards, int32_t* d_out_count, int cap, void* stream) {
    return guarded("bgx_movegen", [&]() -> int {
        if (n < 0 || cap < 0) return fail(BGX_E_ARG, "bgx_movegen: n=%d cap=%d", n, cap);
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_player || !d_dice || !d_out_count || (cap > 0 && !d_out_boards))
            return fail(BGX_E_ARG, "bgx_movegen: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        hipStream_t s = (hipStream_t)stream;
        Lease L;
        if (int rc = lease_scratch(s, L)) return rc;
        if (int rc = require_domain("bgx_movegen", L.sc, d_boards, d_player, d_dice, n, s)) return rc;
        if (int rc = lease_movegen_space(L.sc)) return rc;
        unsigned* ctr = L.sc->words + 2;   // [0] overflow count, [1] error flags
        // The overflow list holds SC_OVF_CAP jobs and every job of a launch may
        // leave tier 1 (push_ovf drops what does not fit: a dropped job's
        // out_count would never be written), so a call runs as launches of at
        // most SC_OVF_CAP jobs each, one after the other on the stream, the
        // input and output pointers offset. The slices are equal (n / k rounded
        // up, k the fewest slices that fit), so each holds more than SC_OVF_CAP / 2
        // jobs and takes the tier-1 kernel the whole call would have taken.
        const int n_slices = (int)(((int64_t)n + SC_OVF_CAP - 1) / SC_OVF_CAP);
        const int per = (int)(((int64_t)n + n_slices - 1) / n_slices);
        for (int j0 = 0; j0 < n; j0 += per) {
            bgx::MovegenArgs a{};
            a.n_jobs = n - j0 < per ? n - j0 : per;
            a.in_mode = bgx::IN_U8;
            a.in_u8 = d_boards + (size_t)j0 * 52;
            a.in_player = d_player + j0;
            a.in_dice = d_dice + (size_t)j0 * 2;
            a.out_mode = bgx::OUT_U8;
            a.cap = cap;
            a.out_u8 = d_out_boards ? d_out_boards + (size_t)j0 * cap * 52 : nullptr;
            a.out_count = d_out_count + j0;
            set_fallback(a, ctr, L.sc->ovf, SC_OVF_CAP, L.sc->ws, SC_WS_WAVES, SC_WS_SLOTS, ctr + 1);
            HIP_TRY(bgx_launch_movegen(&a, s));
        }
        return BGX_OK;
    });
}

int bgx_encode(const uint8_t* d_boards, const uint8_t* d_player, int n, float* d_out, int layout,
               void* stream) {
    return guarded("bgx_encode", [&]() -> int {
        if (n < 0 || (layout != 0 && layout != 1)) return fail(BGX_E_ARG, "bgx_encode: n=%d layout=%d", n, layout);
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_player || !d_out) return fail(BGX_E_ARG, "bgx_encode: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        Lease L;
        if (int rc = lease_scratch((hipStream_t)stream, L)) return rc;
        if (int rc = require_domain("bgx_encode", L.sc, d_boards, d_player, nullptr, n, (hipStream_t)stream)) return rc;
        HIP_TRY(bgx_launch_encode(d_boards, d_player, n, d_out, layout, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_encode_packed(const uint32_t* d_packed, int n, float* d_out, int layout, void* stream) {
    return guarded("bgx_encode_packed", [&]() -> int {
        if (n < 0 || (layout != 0 && layout != 1))
            return fail(BGX_E_ARG, "bgx_encode_packed: n=%d layout=%d", n, layout);
        if (n == 0) return BGX_OK;
        if (!d_packed || !d_out) return fail(BGX_E_ARG, "bgx_encode_packed: null pointer");
        DeviceScope ds(d_packed);
        HIP_TRY(ds.err);
        HIP_TRY(bgx_launch_encode_packed(d_packed, n, d_out, layout, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_td0_update(const uint32_t* d_records, const int32_t* d_offs, int n_eps, float* d_params,
                   float* d_adam_m, float* d_adam_v, int* d_step, float lr, float gamma, float grad_clip,
                   double* d_metrics, void* stream) {
    return guarded("bgx_td0_update", [&]() -> int {
        if (n_eps < 0 || (n_eps > 0 && (!d_records || !d_offs || !d_params || !d_adam_m || !d_adam_v || !d_step ||
                                        !d_metrics)))
            return fail(BGX_E_ARG, "bgx_td0_update: bad arguments (n_eps=%d)", n_eps);
        DeviceScope ds(d_params);   // the kernel runs on the device holding the parameters
        HIP_TRY(ds.err);
        bgx::TrainArgs a{};
        a.rec = d_records;
        a.offs = d_offs;
        a.n_eps = n_eps;
        a.params = d_params;
        a.adam_m = d_adam_m;
        a.adam_v = d_adam_v;
        a.step = d_step;
        a.lr = lr;
        a.gamma = gamma;
        a.grad_clip = grad_clip;
        a.metrics = d_metrics;
        HIP_TRY(bgx_launch_td0(&a, (hipStream_t)stream));
        return BGX_OK;
    });
}

// the three workspace queries: `size` is the entry's total in the layout
static int batch_workspace(const char* name, uint64_t bgx::TrainBatchLayout::*size, int n_records, uint64_t* bytes) {
    return guarded(name, [&]() -> int {
        if (n_records <= 0 || !bytes) return fail(BGX_E_ARG, "%s: n_records=%d", name, n_records);
        *bytes = bgx::train_batch_layout(n_records).*size;
        return BGX_OK;
    });
}

int bgx_td0_batch_workspace(int n_records, uint64_t* bytes) {
    return batch_workspace("bgx_td0_batch_workspace", &bgx::TrainBatchLayout::bytes, n_records, bytes);
}

int bgx_td0_batch_shape(int* tile, int* grid) {
    return guarded("bgx_td0_batch_shape", [&]() -> int {
        if (!tile || !grid) return fail(BGX_E_ARG, "bgx_td0_batch_shape: null pointer");
        *tile = bgx::TRAIN_BATCH_TILE;
        *grid = bgx::TRAIN_BATCH_GRID;
        return BGX_OK;
    });
}

// the batched update behind all its entry points; lam: the TD(lambda) ones (their
// workspace carries the targets after the TD(0) layout); flags: BGX_TDF_* (the
// lambda ones only); after: the afterstate one (d_headers required, the source
// index behind the targets)
static int update_batched(const char* name, bool lam, bool after, const uint32_t* d_records,
                          const uint32_t* d_headers, const int32_t* d_offs, int n_eps,
                          int n_records, float* d_params, float* d_adam_m, float* d_adam_v, int* d_step, float lr,
                          float gamma, float lambda, uint32_t flags, float grad_clip, double* d_metrics,
                          float* d_grad_out, float* d_target_out, void* d_work, uint64_t work_bytes, void* stream) {
    return guarded(name, [&]() -> int {
        if (n_eps <= 0 || n_records < n_eps) return fail(BGX_E_ARG, "%s: n_eps=%d n_records=%d", name, n_eps, n_records);
        if (!d_records || !d_offs || !d_params || !d_adam_m || !d_adam_v || !d_step || !d_metrics || !d_work ||
            (after && !d_headers))
            return fail(BGX_E_ARG, "%s: null pointer", name);
        if (lam && !(lambda >= 0.0f && lambda <= 1.0f))   // a NaN fails both comparisons
            return fail(BGX_E_ARG, "%s: lambda=%g is not in [0, 1]", name, (double)lambda);
        if (flags & ~(uint32_t)BGX_TDF_ZERO_SUM) return fail(BGX_E_ARG, "%s: unknown flags=0x%x", name, (unsigned)flags);
        const bgx::TrainBatchLayout l = bgx::train_batch_layout(n_records);
        const uint64_t need = after ? l.bytes_after : lam ? l.bytes_lambda : l.bytes;
        if (work_bytes < need)
            return fail(BGX_E_ARG, "%s: work_bytes=%llu < %llu (%s)", name, (unsigned long long)work_bytes,
                        (unsigned long long)need,
                        after ? "bgx_td_afterstate_batch_workspace"
                              : lam ? "bgx_tdlambda_batch_workspace" : "bgx_td0_batch_workspace");
        if ((uintptr_t)d_work % 16 != 0) return fail(BGX_E_ARG, "%s: d_work is not 16-byte aligned", name);
        DeviceScope ds(d_params);   // the kernels run on the device holding the parameters
        HIP_TRY(ds.err);
        char* w = (char*)d_work;
        bgx::TrainBatchArgs a{};
        a.rec = d_records;
        a.offs = d_offs;
        a.n_eps = n_eps;
        a.n_rec = n_records;
        a.params = d_params;
        a.adam_m = d_adam_m;
        a.adam_v = d_adam_v;
        a.step = d_step;
        a.lr = lr;
        a.gamma = gamma;
        a.grad_clip = grad_clip;
        a.metrics = d_metrics;
        a.grad_out = d_grad_out;
        a.Y = (float*)(w + l.Y);
        a.info = (int32_t*)(w + l.info);
        a.partial = (float*)(w + l.partial);
        a.grad = (float*)(w + l.grad);
        a.mpart = (double*)(w + l.mpart);
        a.sqpart = (double*)(w + l.sqpart);
        if (lam) {
            a.lambda = lambda;
            a.tgt = (float*)(w + l.tgt);
            a.target_out = d_target_out;
            a.zero_sum = (flags & BGX_TDF_ZERO_SUM) ? 1 : 0;
        }
        if (after) {
            a.hdr = d_headers;
            a.srcidx = (int32_t*)(w + l.srcidx);
        }
        HIP_TRY(bgx_launch_td_batched(&a, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_td0_update_batched(const uint32_t* d_records, const int32_t* d_offs, int n_eps, int n_records,
                           float* d_params, float* d_adam_m, float* d_adam_v, int* d_step, float lr, float gamma,
                           float grad_clip, double* d_metrics, float* d_grad_out, void* d_work, uint64_t work_bytes,
                           void* stream) {
    return update_batched("bgx_td0_update_batched", false, false, d_records, nullptr, d_offs, n_eps, n_records,
                          d_params, d_adam_m, d_adam_v, d_step, lr, gamma, 0.0f, 0u, grad_clip, d_metrics, d_grad_out,
                          nullptr, d_work, work_bytes, stream);
}

int bgx_tdlambda_batch_workspace(int n_records, uint64_t* bytes) {
    return batch_workspace("bgx_tdlambda_batch_workspace", &bgx::TrainBatchLayout::bytes_lambda, n_records, bytes);
}

int bgx_tdlambda_update_batched(const uint32_t* d_records, const int32_t* d_offs, int n_eps, int n_records,
                                float* d_params, float* d_adam_m, float* d_adam_v, int* d_step, float lr,
                                float gamma, float lambda, float grad_clip, double* d_metrics, float* d_grad_out,
                                float* d_target_out, void* d_work, uint64_t work_bytes, void* stream) {
    return update_batched("bgx_tdlambda_update_batched", true, false, d_records, nullptr, d_offs, n_eps, n_records,
                          d_params, d_adam_m, d_adam_v, d_step, lr, gamma, lambda, 0u, grad_clip, d_metrics,
                          d_grad_out, d_target_out, d_work, work_bytes, stream);
}

int bgx_td_update_batched(const uint32_t* d_records, const int32_t* d_offs, int n_eps, int n_records,
                          float* d_params, float* d_adam_m, float* d_adam_v, int* d_step, float lr, float gamma,
                          float lambda, uint32_t flags, float grad_clip, double* d_metrics, float* d_grad_out,
                          float* d_target_out, void* d_work, uint64_t work_bytes, void* stream) {
    return update_batched("bgx_td_update_batched", true, false, d_records, nullptr, d_offs, n_eps, n_records,
                          d_params, d_adam_m, d_adam_v, d_step, lr, gamma, lambda, flags, grad_clip, d_metrics,
                          d_grad_out, d_target_out, d_work, work_bytes, stream);
}

int bgx_td_afterstate_batch_workspace(int n_records, uint64_t* bytes) {
    return batch_workspace("bgx_td_afterstate_batch_workspace", &bgx::TrainBatchLayout::bytes_after, n_records, bytes);
}

int bgx_td_afterstate_update_batched(const uint32_t* d_records, const uint32_t* d_headers, const int32_t* d_offs,
                                     int n_eps, int n_records, float* d_params, float* d_adam_m, float* d_adam_v,
                                     int* d_step, float lr, float gamma, float lambda, uint32_t flags,
                                     float grad_clip, double* d_metrics, float* d_grad_out, float* d_target_out,
                                     void* d_work, uint64_t work_bytes, void* stream) {
    return update_batched("bgx_td_afterstate_update_batched", true, true, d_records, d_headers, d_offs, n_eps,
                          n_records, d_params, d_adam_m, d_adam_v, d_step, lr, gamma, lambda, flags, grad_clip,
                          d_metrics, d_grad_out, d_target_out, d_work, work_bytes, stream);
}

int bgx_episode_offsets(const uint32_t* d_headers, int n_eps, int32_t* d_offs, void* stream) {
    return guarded("bgx_episode_offsets", [&]() -> int {
        if (n_eps < 0 || !d_offs || (n_eps > 0 && !d_headers))
            return fail(BGX_E_ARG, "bgx_episode_offsets: bad arguments (n_eps=%d)", n_eps);
        if ((uintptr_t)d_headers % 4 != 0 || (uintptr_t)d_offs % 4 != 0)
            return fail(BGX_E_ARG, "bgx_episode_offsets: d_headers / d_offs is not 4-byte aligned");
        // one launch on the caller's current device: no allocation, no pointer
        // query and no wait, so the call can be captured into a graph
        HIP_TRY(bgx_launch_episode_offsets(d_headers, n_eps, d_offs, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_reply_moves(const uint8_t* d_boards, const uint8_t* d_opponent, int n, uint32_t* d_out, int cap,
                    int32_t* d_off, int32_t* d_cnt, void* stream) {
    return guarded("bgx_reply_moves", [&]() -> int {
        if (n < 0 || cap < 0) return fail(BGX_E_ARG, "bgx_reply_moves: n=%d cap=%d", n, cap);
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_opponent || !d_out || !d_off || !d_cnt) return fail(BGX_E_ARG, "bgx_reply_moves: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        hipStream_t s = (hipStream_t)stream;
        {
            Lease L;
            if (int rc = lease_scratch(s, L)) return rc;
            if (int rc = require_domain("bgx_reply_moves", L.sc, d_boards, d_opponent, nullptr, n, s)) return rc;
        }
        const int flags = expand_replies(d_boards, d_opponent, n, d_out, cap, d_off, d_cnt, s,
                                         [](const uint32_t*, const unsigned*) { return true; });
        if (flags < 0) return fail(flags, "bgx_reply_moves: HIP failure");
        if (flags) return fail(BGX_E_CAPACITY, "bgx_reply_moves: overflow flags 0x%x", (unsigned)flags);
        return BGX_OK;
    });
}

int bgx_pack(const uint8_t* d_boards, const uint8_t* d_player, int n, uint32_t* d_packed, void* stream) {
    return guarded("bgx_pack", [&]() -> int {
        if (n < 0) return fail(BGX_E_ARG, "bgx_pack: n=%d", n);
        HIP_TRY(bgx_launch_pack(d_boards, d_player, n, d_packed, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_unpack(const uint32_t* d_packed, int n, uint8_t* d_boards, void* stream) {
    return guarded("bgx_unpack", [&]() -> int {
        if (n < 0) return fail(BGX_E_ARG, "bgx_unpack: n=%d", n);
        HIP_TRY(bgx_launch_unpack(d_packed, n, d_boards, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_net_create(const float* h_W1, const float* h_b1, const float* h_w2, const float* h_b2,
                   bgx_net** out) {
    return guarded("bgx_net_create", [&]() -> int {
        if (!h_W1 || !h_b1 || !h_w2 || !h_b2 || !out) return fail(BGX_E_ARG, "bgx_net_create: null pointer");
        std::unique_ptr<bgx_net> n(new bgx_net());
        if (n->W1.alloc(128 * 198) || n->b1.alloc(128) || n->w2.alloc(128) || n->wfrag.alloc(NFRAG) ||
            n->rowc.alloc(128 * 4))
            return BGX_E_HIP;
        if (int rc = net_upload(n.get(), h_W1, h_b1, h_w2, h_b2)) return rc;
        *out = n.release();
        return BGX_OK;
    });
}

int bgx_net_destroy(bgx_net* n) {
    return guarded("bgx_net_destroy", [&]() -> int {
        delete n;
        return BGX_OK;
    });
}

int bgx_value(const bgx_net* net, const float* d_x, int n, float* d_out, void* stream) {
    return guarded("bgx_value", [&]() -> int {
        if (!net || n < 0) return fail(BGX_E_ARG, "bgx_value: bad arguments");
        if (n == 0) return BGX_OK;
        HIP_TRY(bgx_launch_value_f32(d_x, n, net->W1, net->b1, net->w2, net->b2, d_out, (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_value_boards(const bgx_net* net, const uint8_t* d_boards, const uint8_t* d_player, int n,
                     float* d_out, void* stream) {
    return guarded("bgx_value_boards", [&]() -> int {
        if (!net || n < 0) return fail(BGX_E_ARG, "bgx_value_boards: bad arguments");
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_player || !d_out) return fail(BGX_E_ARG, "bgx_value_boards: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        hipStream_t s = (hipStream_t)stream;
        Lease L;
        if (int rc = lease_scratch(s, L)) return rc;
        if (int rc = require_domain("bgx_value_boards", L.sc, d_boards, d_player, nullptr, n, s)) return rc;
        if (grow(L.sc->packed, (size_t)n * 8)) return BGX_E_HIP;   // the lease's last user has finished (lease_scratch)
        HIP_TRY(bgx_launch_pack(d_boards, d_player, n, L.sc->packed, s));
        bgx::MlpArgs m{};
        m.rows = L.sc->packed;
        m.n_rows = n;
        m.out = d_out;
        set_net(m, net);
        HIP_TRY(bgx_launch_mlp(&m, s));
        return BGX_OK;
    });
}

int bgx_value_boards_routed(const bgx_net* net0, const bgx_net* net1, const uint8_t* d_boards,
                            const uint8_t* d_player, const uint8_t* d_net, int n, float* d_out, void* stream) {
    return guarded("bgx_value_boards_routed", [&]() -> int {
        if (!net0 || !net1 || n < 0) return fail(BGX_E_ARG, "bgx_value_boards_routed: bad arguments");
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_player || !d_net || !d_out) return fail(BGX_E_ARG, "bgx_value_boards_routed: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        hipStream_t s = (hipStream_t)stream;
        Lease L;
        if (int rc = lease_scratch(s, L)) return rc;
        if (int rc = require_domain("bgx_value_boards_routed", L.sc, d_boards, d_player, nullptr, n, s)) return rc;
        if (grow(L.sc->packed, (size_t)n * 8)) return BGX_E_HIP;   // the lease's last user has finished (lease_scratch)
        if (grow(L.sc->lists, (size_t)n * 2)) return BGX_E_HIP;
        int32_t* const lists[2] = {L.sc->lists, L.sc->lists + L.sc->lists.count() / 2};
        unsigned* ctr = L.sc->words + 8;   // [0..1] list lengths, [2..3] tile claims
        HIP_TRY(hipMemsetAsync(ctr, 0, 16, s));
        HIP_TRY(bgx_launch_pack(d_boards, d_player, n, L.sc->packed, s));
        bgx::MatchMlpArgs m{};
        m.rows = L.sc->packed;
        m.out = d_out;
        m.n_max = n;
        m.list_cap = n;
        m.nt = 1;
        m.n_hint = n;
        const bgx_net* nets[2] = {net0, net1};
        for (int k = 0; k < 2; ++k) {
            m.list[k] = lists[k];
            m.count[k] = ctr + k;
            m.claim[k] = ctr + 2 + k;
            set_net(m, k, nets[k]);
        }
        HIP_TRY(bgx_launch_route_ids(d_net, n, lists[0], lists[1], ctr, s));
        HIP_TRY(bgx_launch_mlp_routed(&m, s));
        return BGX_OK;
    });
}

int bgx_two_ply(const bgx_net* net, const uint8_t* d_boards, const uint8_t* d_opponent, int n,
                double* d_out, void* stream) {
    return guarded("bgx_two_ply", [&]() -> int {
        return bgx_two_ply_sampled(net, d_boards, d_opponent, n, 0, 0, d_out, stream);
    });
}

int bgx_two_ply_sampled(const bgx_net* net, const uint8_t* d_boards, const uint8_t* d_opponent, int n,
                        int sample_k, uint64_t seed, double* d_out, void* stream) {
    return guarded("bgx_two_ply_sampled", [&]() -> int {
        if (!net || n < 0) return fail(BGX_E_ARG, "bgx_two_ply: bad arguments");
        if (sample_k != 0 && (sample_k < 5 || sample_k > 1024))
            return fail(BGX_E_ARG, "bgx_two_ply_sampled: sample_k=%d (0 = exact, 5..1024)", sample_k);
        if (n == 0) return BGX_OK;
        if (!d_boards || !d_opponent || !d_out) return fail(BGX_E_ARG, "bgx_two_ply: null pointer");
        DeviceScope ds(d_boards);
        HIP_TRY(ds.err);
        hipStream_t s = (hipStream_t)stream;
        {
            Lease L;
            if (int rc = lease_scratch(s, L)) return rc;
            if (int rc = require_domain("bgx_two_ply", L.sc, d_boards, d_opponent, nullptr, n, s)) return rc;
        }
        const int jobs = n * 21;
        // 768 rows per (board, roll) job ON AVERAGE, i.e. 21 * 768 = 16,128 per root:
        // a single list can be far longer (2,140 plays for 1-1 from fifteen
        // single checkers), but the heaviest root found has 10,839 replies over
        // the 21 rolls, which leaves room for a workgroup's reserved, unused row
        // chunks (tests/heavy_cases.py, test_heavy_cases.py); beyond it the call
        // fails with BGX_E_CAPACITY
        const int cap = jobs * 768;
        DevBuf<uint32_t> reply;
        DevBuf<int32_t> off, cnt;
        DevBuf<float> V, jv, zt;
        // BGX_REPLY_DELTA: the roots' hidden accumulators, for the replies by difference
        if (reply.alloc((size_t)cap * 8) || off.alloc(jobs) || cnt.alloc(jobs) || V.alloc(cap) || jv.alloc(jobs) ||
            (reply_delta() && zt.alloc((size_t)n * 128)))
            return fail(BGX_E_HIP, "bgx_two_ply: HIP failure");
        const int flags = expand_replies(d_boards, d_opponent, n, reply, cap, off, cnt, s,
                                         [&](const uint32_t* roots, const unsigned* n_rows) {
            if (zt) {   // the roots' V goes to the reply buffer's first n slots, overwritten below
                bgx::MlpArgs m{};
                m.rows = roots;
                m.n_rows = n;
                m.nt = 1;
                m.out = V;
                set_net(m, net);
                m.zout = zt;
                m.z_base = 0;
                if (bgx_launch_mlp(&m, s) != hipSuccess) return false;
            }
            bgx::MlpArgs m{};
            m.rows = reply;
            m.n_rows = 0;
            m.n_rows_dev = n_rows;
            m.n_max = cap;
            m.nt = 2;
            m.out = V;
            set_net(m, net);
            if (zt) {
                m.zt = zt;
                m.root_rows = roots;
                m.root_sel = nullptr;
                m.root_base = 0;
                m.n_roots = n;
                m.n_slots = n;
            }
            return bgx_launch_mlp(&m, s) == hipSuccess &&
                   bgx_launch_top5(V, off, cnt, jobs, nullptr, 0, jobs, jv, sample_k, seed, nullptr, nullptr, s) ==
                       hipSuccess &&
                   bgx_launch_two_ply_reduce(jv, n, d_out, s) == hipSuccess;
        });
        if (flags < 0) return fail(flags, "bgx_two_ply: HIP failure");
        if (flags) return fail(BGX_E_CAPACITY, "bgx_two_ply: overflow flags 0x%x", (unsigned)flags);
        return BGX_OK;
    });
}

int bgx_rollout_tally(const uint32_t* d_headers, int n_headers, const uint8_t* d_start_player, int n_pos,
                      uint32_t max_episode, uint64_t* d_counts, void* stream) {
    return guarded("bgx_rollout_tally", [&]() -> int {
        if (n_headers < 0 || n_pos <= 0 || (n_headers > 0 && (!d_headers || !d_start_player || !d_counts)))
            return fail(BGX_E_ARG, "bgx_rollout_tally: bad arguments (n_headers=%d, n_pos=%d)", n_headers, n_pos);
        if (n_headers == 0) return BGX_OK;
        DeviceScope ds(d_headers);
        HIP_TRY(ds.err);
        HIP_TRY(bgx_launch_rollout_tally(d_headers, n_headers, d_start_player, n_pos, max_episode,
                                         (unsigned long long*)d_counts, (hipStream_t)stream));
        return BGX_OK;
    });
}

}  // extern "C"
