// bgx_host.h — shared by the host translation units of libbgx.so (bgx_abi.cpp,
// bgx_host_*.cpp): error reporting, owners of device memory and runtime
// handles, the bgx_net / bgx_engine definitions and small argument fillers.
// Host code only: no .hip file includes it. Nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <exception>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "bgx.h"
#include "bgx_kernels.h"
#include "bgx_prof.h"

#pragma GCC visibility push(hidden)

// sets the calling thread's bgx_last_error() string and returns `code` (bgx_abi.cpp)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(BGX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));       \
    } while (0)

// Every int entry point runs inside guarded(): a C++ exception (std::bad_alloc
// from a host vector, ...) becomes an error code and bgx_last_error(), never an
// unwind across the C boundary.
template <typename F>
int guarded(const char* what, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(BGX_E_CAPACITY, "%s: host allocation failed", what);
    } catch (const std::exception& ex) {
        return fail(BGX_E_STATE, "%s: %s", what, ex.what());
    } catch (...) {
        return fail(BGX_E_STATE, "%s: unexpected C++ exception", what);
    }
}

// One hipMalloc allocation of count() elements, freed with its owner. Converts
// to the raw pointer, null while empty.
template <typename T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {   // (not onto itself)
        reset();
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~DevBuf() { reset(); }
    // n fresh elements (what it held is freed first) + 16 B of slack the kernels may read
    int alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T) + 16);
        if (e != hipSuccess) {
            p_ = nullptr;
            return fail(BGX_E_HIP, "hipMalloc(%zu B): %s", n * sizeof(T), hipGetErrorString(e));
        }
        n_ = n;
        return BGX_OK;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
};

// at least n elements: a smaller buffer is replaced (contents are not kept)
template <typename T>
int grow(DevBuf<T>& b, size_t n) {
    return b.count() >= n ? BGX_OK : b.alloc(n);
}

// a runtime handle released by Del with its owner: events, streams, graph
// execs, pinned / mapped host blocks
template <typename H, auto Del>
class Handle {
    H h_ = nullptr;

public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Handle() { (void)reset(); }
    hipError_t reset() { return h_ ? Del(std::exchange(h_, nullptr)) : hipSuccess; }
    H* put() { return (void)reset(), &h_; }   // for a create call: releases what it held
    operator H() const { return h_; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;
using HostWords = Handle<uint32_t*, hipHostFree>;

// hipSetDevice to the device holding `p` (a device pointer) for the scope; the
// caller's current device is restored at the end
struct DeviceScope {
    int prev = -1;
    int dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(const void* p) {
        err = hipGetDevice(&prev);
        if (err != hipSuccess) return;
        dev = prev;
        hipPointerAttribute_t at{};
        if (p && hipPointerGetAttributes(&at, p) == hipSuccess && at.device >= 0 && at.device != prev) {
            err = hipSetDevice(at.device);
            dev = at.device;
        }
        (void)hipGetLastError();   // a host pointer's attribute query is not an error here
    }
    ~DeviceScope() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

struct bgx_net {
    DevBuf<float> W1, b1, w2;   // fp32 copies (bgx_value)
    float b2 = 0.0f;
    DevBuf<uint4> wfrag;        // split-fp16 MFMA fragments
    DevBuf<float> rowc;         // [128] w2
    float feat_scale = 1.0f;    // 2^-e: features scaled so the accumulator is the exp2 argument
};

int net_upload(bgx_net* n, const float* W1, const float* b1, const float* w2, const float* b2);   // bgx_abi.cpp

// the network fields of a launch's arguments (MlpArgs, FusedArgs) ...
template <typename A>
void set_net(A& a, const bgx_net* n) {
    a.wfrag = n->wfrag;
    a.rowc = n->rowc;
    a.b2 = n->b2;
    a.feat_scale = n->feat_scale;
}

// ... and of network k of a routed launch's
inline void set_net(bgx::MatchMlpArgs& a, int k, const bgx_net* n) {
    a.wfrag[k] = n->wfrag;
    a.rowc[k] = n->rowc;
    a.b2[k] = n->b2;
    a.feat_scale[k] = n->feat_scale;
}

// engine counter words (bgx_engine::ctr): [3] ep, [4] err; per-step (zeroed each
// step): [8] flat, [9] reply, [10] ovf, [11] ovf2; [12..15] the balanced fused
// launch's lane-step and finished-workgroup counters (u64)
constexpr int C_EP = 3, C_ERR = 4, C_FLAT = 8, C_REPLY = 9, C_OVF = 10, C_OVF2 = 11, C_BUDGET = 12;
constexpr int kCtrWords = 16;
// stats words: [0..7] counters (bgx_get_stats), then the top-5 launch's per-wave
// reply-record counts
constexpr int kStatWords = 8 + bgx::T5_WAVES;
// harvest buffers (bgx_harvest_enqueue / _fetch): ticket t uses slot t % 3. A
// ticket's arrays live until the second harvest after it; the fused engine
// harvests inside its launches, so the launches between tickets t + 1 and
// t + 2 already fill slot (t + 2) % 3: a third slot keeps ticket t's arrays
// intact until then
constexpr int NHB = 3;
// fused engine (in-kernel harvest), bgx_engine::fh_ctr, u64 words: [b] slot b's
// running {episodes << 32 | records} appended since the previous ticket,
// [NHB] finished workgroups, [NHB + 1 + b] slot b's accumulated error flags
// (moved there from the engine's word by each launch's last workgroup),
// [2 NHB + 1 + b] slot b's commits
constexpr int kFhWords = 3 * NHB + 1;

// match mode (bgx_engine_set_opponent): network 1, the row-index lists of the
// routed launches (root: L + cand_cap entries each; reply: reply_cap each),
// the network of each 2-ply reply root slot, and the step's routing counters
// (EngineDev::match_ctr). Built whole on first entering match mode and kept
// for re-entry.
struct MatchState {
    std::unique_ptr<bgx_net> net1;
    DevBuf<int32_t> list[2], rlist[2];
    DevBuf<uint8_t> slot;
    int slots = 0;
    DevBuf<unsigned> ctr;   // [8]
};

struct bgx_engine {
    int device = 0;
    bgx_config cfg{};
    std::unique_ptr<bgx_net> net;
    bgx::EngineDev d{};   // raw copies of the pointers below, for the kernels
    hipStream_t last = nullptr;
    // device buffers
    DevBuf<uint32_t> rows;
    DevBuf<float> V;
    DevBuf<int32_t> cand_off, cand_cnt;
    DevBuf<unsigned> ctr;   // [kCtrWords], C_*
    DevBuf<unsigned long long> stats;
    struct {   // the lanes' state (EngineDev)
        DevBuf<uint8_t> player, dice;
        DevBuf<int32_t> step;
        DevBuf<uint32_t> flags, epi;
        DevBuf<uint64_t> rng;
        DevBuf<uint32_t> rec_count, ep_first, harv, ring, ep_list, hring, hepi;
    } lane;
    DevBuf<int32_t> sel;
    DevBuf<uint32_t> sel_rows, reply_rows;
    DevBuf<float> reply_V;
    DevBuf<int32_t> job_off, job_cnt;
    DevBuf<float> job_val;
    DevBuf<float> zt;   // 2-ply: the reply roots' hidden accumulators [roots][128] (K = all: every
                        // candidate, from the root launch; K = 4: the chosen rows, own launch)
    DevBuf<float> zv;   // K = 4: that launch's V output (unused)
    int jobs_cap = 0, reply_cap = 0, cand_cap = 0;
    bool match = false;              // match mode is on (m is set)
    std::unique_ptr<MatchState> m;   // complete or absent
    DevBuf<int32_t> ovf_list;
    int ovf_cap = 0;
    DevBuf<uint32_t> ws;
    int ws_waves = 0, ws_slots = 0;
    // fused 1-ply step: per-lane candidate slots and values
    bool fused = false;
    DevBuf<uint32_t> fcand;
    DevBuf<float> fvbuf;
    DevBuf<int> ft1cnt;      // fused: the lanes' next-position expansion counts (FusedArgs::t1cnt)
    bool t1_ready = false;   // ... valid: set by a fused launch, cleared by every lane reset
    int fcap = 0;
    DevBuf<unsigned long long> fprof;   // BGX_FUSED_PROF: phase clocks [kProfSlots][kProfSlotWords], printed at destroy
    // harvest: records of at most L x ring (every unharvested record of every lane), NHB slots
    DevBuf<uint32_t> out_records[NHB];
    DevBuf<uint32_t> out_headers[NHB];   // [ep_cap][16] copies of the finished episodes' headers
    DevBuf<int32_t> d_offs[NHB];         // [ep_cap + 1]
    DevBuf<uint32_t> d_info[NHB];        // [4] harvest totals
    HostWords h_info;                    // [NHB][4] host-mapped copies, written by the harvesting kernel itself
    uint32_t* h_info_dev = nullptr;      // its device address
    DevBuf<unsigned long long> fh_ctr;   // [kFhWords], fused engine only
    unsigned long long* hv_total(int b) const { return fh_ctr + b % NHB; }
    unsigned long long* hv_done() const { return fh_ctr + NHB; }
    unsigned long long* hv_flags(int b) const { return fh_ctr + NHB + 1 + b % NHB; }
    unsigned long long* hv_commit(int b) const { return fh_ctr + 2 * NHB + 1 + b % NHB; }
    bool fh_launched = false;   // a fused launch filled the current slot since the last ticket
    Event hev;                  // the engine's last step, for a harvest on another stream
    Event hdone[NHB];           // a slot's harvest finished
    hipStream_t hstream = nullptr;   // stream of the last enqueued harvest (the next step waits for it)
    int h_tickets = 0;               // harvests enqueued so far
    // timing
    bool timing = false;
    std::vector<Event> ev;   // pairs: movegen, mlp
    std::vector<int> ev_kind;
    double ms_mg = 0, ms_mlp = 0;
    int n_mg = 0, n_mlp = 0;
    // test / development hooks, read once at create: BGX_MG_TEST_TIER (fused
    // movegen tiers), BGX_FUSED_PROF (phase clocks, printed at destroy)
    int force_tier = 0;
    bool prof_enabled = false;
    int fused_fl = 0;              // BGX_FUSED_LANES: fused 1-ply lanes per workgroup (16 / 32; 0 = auto)
    int fused_pair = 1;            // BGX_FUSED_PAIR: two rule-mode non-doubles jobs per wave (0 = off; A/B, tests)
    // bgx_set_weights_device: the check launch's verdict (bgx::PackInfo, 16 B), its
    // pinned host copy, and the event that orders the hand-off behind `last`
    DevBuf<uint32_t> wd_info;
    HostWords wd_hinfo;
    Event wd_ev;
    DevBuf<uint8_t> dice_tab;      // bgx_engine_set_dice
    DevBuf<uint32_t> start_tab;    // bgx_engine_set_start (EngineDev::start_tab)
    // optional hipGraph of the last n_steps sequence
    bool use_graph = false;   // measured slower than direct launches on ROCm 7 (BGX_GRAPH=1 enables)
    Stream cap;
    GraphExec gexec;
    int g_steps = 0;
};

// a movegen launch's fallback path: the overflow list and its counter, the
// global-memory workspace (waves x 5 x slots words) and the error flag word
inline void set_fallback(bgx::MovegenArgs& a, unsigned* ovf_count, int32_t* ovf_list, int ovf_cap, uint32_t* ws,
                         int ws_waves, int ws_slots, unsigned* err_flags) {
    a.ovf_count = ovf_count;
    a.ovf_list = ovf_list;
    a.ovf_cap = ovf_cap;
    a.ws_global = ws;
    a.ws_waves = ws_waves;
    a.ws_slots = ws_slots;
    a.ws_words_per_wave = (size_t)5 * ws_slots;
    a.err_flags = err_flags;
}

int flag_error(unsigned f);        // bgx_host_step.cpp
int check_flags(bgx_engine* e);    // bgx_host_step.cpp

// the captured graph holds kernel arguments: dropped when one of them changes
inline int drop_graph(bgx_engine* e) {
    HIP_TRY(e->gexec.reset());
    return BGX_OK;
}

// BGX_REPLY_DELTA=1: the 2-ply reply values by difference from their roots
// (mlp_kernel_delta, bgx_mlp.hip) instead of in full (mlp_kernel_il, the
// default). Measured and not kept: 33 % fewer MFMAs but
// twice the VALU and 27x the SALU instructions per tile, 0.95 vs 0.69 ms per
// K = 4 reply launch. Read when an engine is created / per stateless call, so
// tests can cross-check both forms in one process.
inline bool reply_delta() {
    const char* v = getenv("BGX_REPLY_DELTA");
    return v && atoi(v) != 0;
}

// Rows per reply-launch reservation unit (MovegenArgs::flat_chunk): 512 by
// default, BGX_FLAT_CHUNK in [64, 1024] for A/B runs (the engine's reply_cap
// slack is sized from it, so it is bounded above too).
inline int reply_flat_chunk() {
    static const int chunk = [] {
        const char* v = getenv("BGX_FLAT_CHUNK");
        const int c = v ? atoi(v) : 512;
        return c < 64 ? 512 : (c > 1024 ? 1024 : c);
    }();
    return chunk;
}

#pragma GCC visibility pop
