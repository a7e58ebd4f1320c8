// bgx_host_engine.cpp — engine lifetime and modes: create / destroy, weights,
// scripted dice, match mode, rollout mode, and the host's views of the
// engine's state (stats, peek, timing).
#include <cmath>
#include <cstring>

#include "bgx_domain.h"
#include "bgx_host.h"
#include "bgx_pack.h"

// every lane restarts from BackgammonEnv.reset, or in rollout mode from its
// start-table position: new scripted dice, and entering or leaving match mode
// or rollout mode, so that every harvested game was played in one mode
static int restart_lanes(bgx_engine* e) {
    if (int rc = drop_graph(e)) return rc;
    HIP_TRY(hipMemset(e->ctr, 0, e->ctr.bytes()));
    HIP_TRY(bgx_launch_engine_reset(&e->d, nullptr));
    e->t1_ready = false;   // the fused launch's carried expansion belongs to the old positions
    HIP_TRY(hipDeviceSynchronize());
    return check_flags(e);
}

extern "C" {

void bgx_config_default(bgx_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->lanes = 4096;
    c->lane_base = 0;
    c->seed = 0;
    c->ply = 1;
    c->k_top = 4;
    c->alpha = 1.0f;
    c->beta = 0.9f;
    c->max_steps = 300;
    c->max_legal = 500;
    c->ring = 1024;
    c->ep_cap = 0;   // 0 = derived from lanes
    c->cand_per_lane = 256;
    c->reply_per_lane = 0;   // 0 = derived from k_top
    c->fused = 1;
}

int bgx_engine_destroy(bgx_engine* e) {
    return guarded("bgx_engine_destroy", [&]() -> int {
        if (!e) return BGX_OK;
        hipSetDevice(e->device);
        hipDeviceSynchronize();
        if (e->fprof) {   // development report (BGX_FUSED_PROF)
            std::vector<unsigned long long> p(e->fprof.count());
            if (hipMemcpy(p.data(), e->fprof, e->fprof.bytes(), hipMemcpyDeviceToHost) == hipSuccess)
                fused_prof_report(p.data(), kProfSlots, stderr, getenv("BGX_FUSED_PROF_DUMP"));
        }
        delete e;
        return BGX_OK;
    });
}

int bgx_engine_create(int device, const bgx_config* cfg, bgx_engine** out) {
    return guarded("bgx_engine_create", [&]() -> int {
        if (!cfg || !out) return fail(BGX_E_ARG, "bgx_engine_create: null pointer");
        if (cfg->lanes <= 0 || cfg->lanes > (1 << 24)) return fail(BGX_E_ARG, "lanes=%d", cfg->lanes);
        if (cfg->ply != 1 && cfg->ply != 2) return fail(BGX_E_ARG, "ply=%d (1 or 2)", cfg->ply);
        if (cfg->ply == 2 && cfg->k_top != 4 && cfg->k_top != 0)
            return fail(BGX_E_ARG, "k_top=%d (4 = reference, 0 = all)", cfg->k_top);
        if (cfg->reply_sample != 0 && (cfg->reply_sample < 5 || cfg->reply_sample > 1024))
            return fail(BGX_E_ARG, "reply_sample=%d (0 = exact, 5..1024; the reference samples 50)", cfg->reply_sample);
        if (cfg->max_steps <= 0 || cfg->max_legal <= 0) return fail(BGX_E_ARG, "max_steps/max_legal");
        if (cfg->ring < cfg->max_steps + 1 || cfg->ring > (1 << 16))
            return fail(BGX_E_ARG, "ring=%d (max_steps+1 .. 65536)", cfg->ring);
        // the select kernel keeps a lane's scores in a 512-entry LDS row; the fused
        // 1-ply kernel keeps its candidates in per-lane slots of max_legal
        const bool fused_cfg = cfg->fused != 0 && cfg->ply == 1;
        if (cfg->max_legal > (fused_cfg ? 2048 : 512))
            return fail(BGX_E_ARG, "max_legal=%d > %d (%s engine)", cfg->max_legal, fused_cfg ? 2048 : 512,
                        fused_cfg ? "fused" : "phased");
        if (cfg->max_steps > 511) return fail(BGX_E_ARG, "max_steps=%d > 511 (record step field)", cfg->max_steps);
        HIP_TRY(hipSetDevice(device));
        std::unique_ptr<bgx_engine> e(new bgx_engine());
        e->device = device;
        if (const char* g = getenv("BGX_GRAPH")) e->use_graph = atoi(g) != 0;
        if (const char* v = getenv("BGX_MG_TEST_TIER")) e->force_tier = atoi(v);
        e->prof_enabled = getenv("BGX_FUSED_PROF") != nullptr;
        if (const char* v = getenv("BGX_FUSED_LANES")) e->fused_fl = atoi(v);
        if (const char* v = getenv("BGX_FUSED_PAIR")) e->fused_pair = atoi(v) != 0;
        e->cfg = *cfg;
        // ring slots: a power of two (slot = record counter & (R - 1) stays exact
        // when the 32-bit counter wraps)
        int ring = 1;
        while (ring < cfg->ring) ring <<= 1;
        e->cfg.ring = ring;
        const int L = cfg->lanes;
        e->cand_cap = L * (cfg->cand_per_lane > 0 ? cfg->cand_per_lane : 256);
        // finished episodes between two harvests: at most (steps per harvest) /
        // (shortest game) + 1 per lane. A game takes >= 7 turns of the winner
        // (167 pips, at most 24 per turn) and >= 6 of the loser: >= 13 env steps.
        constexpr int kMinGameSteps = 13;
        const long long ep_need = (long long)L * ((ring - cfg->max_steps) / kMinGameSteps + 1) + 1024;
        const int ep_cap = cfg->ep_cap > 0 ? cfg->ep_cap : (int)(ep_need < (1 << 30) ? ep_need : (1 << 30));
        int rc = BGX_OK;
        bgx::EngineDev& d = e->d;
        // n elements for an owner, once an allocation has failed none; the raw
        // pointer (null then) for the kernels' copy in d
        auto take = [&rc](auto& buf, size_t n) {
            if (!rc) rc = buf.alloc(n);
            return buf.get();
        };
        d.rows = take(e->rows, (size_t)(L + e->cand_cap) * 8);
        d.V = take(e->V, (size_t)(L + e->cand_cap));
        d.cand_off = take(e->cand_off, L);
        d.cand_cnt = take(e->cand_cnt, L);
        take(e->ctr, kCtrWords);
        d.stats = take(e->stats, kStatWords);
        d.player = take(e->lane.player, L);
        d.dice = take(e->lane.dice, 2 * L);
        d.step = take(e->lane.step, L);
        d.flags = take(e->lane.flags, L);
        d.epi = take(e->lane.epi, L);
        d.rng = take(e->lane.rng, L);
        d.rec_count = take(e->lane.rec_count, L);
        d.ep_first = take(e->lane.ep_first, L);
        d.harv = take(e->lane.harv, L);
        d.ring = take(e->lane.ring, (size_t)L * ring * bgx::REC_WORDS);
        d.ep_list = take(e->lane.ep_list, (size_t)ep_cap * bgx::EP_WORDS);
        for (int b = 0; b < NHB; ++b) {
            take(e->out_records[b], (size_t)L * ring * bgx::REC_WORDS);
            take(e->out_headers[b], (size_t)ep_cap * bgx::EP_WORDS);
            take(e->d_offs[b], (size_t)ep_cap + 1);
            take(e->d_info[b], 4);
            if (!rc && hipEventCreateWithFlags(e->hdone[b].put(), hipEventDisableTiming) != hipSuccess)
                rc = fail(BGX_E_HIP, "hipEventCreate failed");
        }
        if (!rc && (hipHostMalloc((void**)e->h_info.put(), 4 * NHB * sizeof(uint32_t),
                                  hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                    hipHostGetDevicePointer((void**)&e->h_info_dev, e->h_info, 0) != hipSuccess))
            rc = fail(BGX_E_HIP, "hipHostMalloc (mapped) failed");
        e->ovf_cap = 1 << 16;
        e->ws_waves = 512;   // one global-memory fallback slice per tier-2 block / fused workgroup (<= 2 per CU)
        e->ws_slots = 16384;
        take(e->ovf_list, e->ovf_cap);
        take(e->ws, (size_t)e->ws_waves * 5 * e->ws_slots);
        e->fused = fused_cfg;
        if (e->fused) {
            e->fcap = cfg->max_legal;
            take(e->fcand, (size_t)L * e->fcap * 8);
            take(e->fvbuf, (size_t)L * (e->fcap + 1));
            take(e->ft1cnt, L);
            // per-lane episode headers for the in-kernel harvest: at most
            // (ring - max_steps) / 13 + 1 episodes finish between two harvests
            int hr = 1;
            while (hr < (ring - cfg->max_steps) / kMinGameSteps + 2) hr <<= 1;
            d.HR = hr;
            d.hring = take(e->lane.hring, (size_t)L * hr * bgx::EP_WORDS);
            d.hepi = take(e->lane.hepi, L);
            take(e->fh_ctr, kFhWords);
        }
        if (cfg->ply == 2) {
            e->jobs_cap = cfg->k_top == 4 ? L * 4 * 21 : e->cand_cap * 21;
            const int per_lane = cfg->reply_per_lane > 0 ? cfg->reply_per_lane : (cfg->k_top == 4 ? 4096 : 16384);
            int n_cu = 256;
            if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) n_cu = 256;
            // + slack for the rows reserved but left unwritten: the reply launch
            // runs two workgroups per CU (bgx_launch_movegen), each ending with at
            // most one workgroup chunk (<= 8 x flat_chunk rows) and its waves'
            // kept remainders (tails of replaced chunks, each smaller than the
            // request that replaced it); two chunks' worth per workgroup covers
            // both (measured gap rows: 2-3 % of a K = 4 step's rows, DESIGN.md
            // section 4). Running out is flagged (BGX_E_CAPACITY), not silent.
            e->reply_cap = L * per_lane + n_cu * 2 * 2 * 8 * reply_flat_chunk();
            d.sel = take(e->sel, 4 * L);
            d.sel_rows = take(e->sel_rows, (size_t)4 * L * 8);
            take(e->reply_rows, (size_t)e->reply_cap * 8);
            take(e->reply_V, e->reply_cap);
            take(e->job_off, e->jobs_cap);
            take(e->job_cnt, e->jobs_cap);
            d.job_val = take(e->job_val, e->jobs_cap);
            if (reply_delta()) {
                take(e->zt, (size_t)(cfg->k_top == 4 ? 4 * L : e->cand_cap) * 128);
                if (cfg->k_top == 4) take(e->zv, 4 * L);
            }
        }
        if (rc) return rc;
        if (hipMemset(e->ctr, 0, e->ctr.bytes()) != hipSuccess || hipMemset(e->stats, 0, e->stats.bytes()) != hipSuccess ||
            (e->fh_ctr && hipMemset(e->fh_ctr, 0, e->fh_ctr.bytes()) != hipSuccess))
            return fail(BGX_E_HIP, "hipMemset failed");
        d.L = L;
        d.lane_base = cfg->lane_base;
        d.seed = cfg->seed;
        d.temperature = 1.5f;
        d.max_steps = cfg->max_steps;
        d.max_legal = cfg->max_legal;
        d.ply = cfg->ply;
        d.k_top = cfg->k_top;
        d.alpha = cfg->alpha;
        d.greedy = cfg->greedy != 0;
        d.beta = cfg->beta;
        d.cand_cap = e->cand_cap;
        d.R = ring;
        d.dice_tab = nullptr;
        d.dice_len = 0;
        d.ep_count = e->ctr + C_EP;
        d.ep_cap = ep_cap;
        d.flat_count = e->ctr + C_FLAT;
        d.reply_count = e->ctr + C_REPLY;
        d.ovf_count = e->ctr + C_OVF;
        d.ovf_count2 = e->ctr + C_OVF2;
        d.n_jobs2 = cfg->k_top == 4 ? L * 4 * 21 : 0;
        d.err_flags = e->ctr + C_ERR;
        d.match_ctr = nullptr;
        if (bgx_launch_engine_reset(&d, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return fail(BGX_E_HIP, "engine reset failed");
        *out = e.release();
        return BGX_OK;
    });
}

int bgx_engine_set_dice(bgx_engine* e, const uint8_t* h_dice, int per_lane) {
    return guarded("bgx_engine_set_dice", [&]() -> int {
        if (!e || !h_dice || per_lane < 2) return fail(BGX_E_ARG, "bgx_engine_set_dice: bad arguments");
        if (!e->cfg.greedy) return fail(BGX_E_STATE, "bgx_engine_set_dice: scripted dice need greedy play");
        const size_t n = (size_t)e->cfg.lanes * (size_t)per_lane;
        for (size_t k = 0; k < n; ++k)
            if (h_dice[k] < 1 || h_dice[k] > 6) return fail(BGX_E_ARG, "bgx_engine_set_dice: die %d at %zu", h_dice[k], k);
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        if (e->dice_tab.alloc(n)) return BGX_E_HIP;
        HIP_TRY(hipMemcpy(e->dice_tab, h_dice, n, hipMemcpyHostToDevice));
        e->d.dice_tab = e->dice_tab;
        e->d.dice_len = per_lane;
        return restart_lanes(e);   // from BackgammonEnv.reset with its scripted dice
    });
}

int bgx_set_weights(bgx_engine* e, const float* h_W1, const float* h_b1, const float* h_w2,
                    const float* h_b2, float temperature, uint64_t version) {
    return guarded("bgx_set_weights", [&]() -> int {
        (void)version;
        if (!e) return fail(BGX_E_ARG, "bgx_set_weights: null engine");
        if (!(temperature > 0.0f)) return fail(BGX_E_ARG, "temperature=%g", (double)temperature);
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        if (!e->net) {
            bgx_net* n = nullptr;
            if (int rc = bgx_net_create(h_W1, h_b1, h_w2, h_b2, &n)) return rc;
            e->net.reset(n);
        } else if (int rc = net_upload(e->net.get(), h_W1, h_b1, h_w2, h_b2)) {
            return rc;
        }
        if (e->d.temperature != temperature)
            if (int rc = drop_graph(e)) return rc;
        e->d.temperature = temperature;
        return BGX_OK;
    });
}

int bgx_set_weights_device(bgx_engine* e, const float* d_params, float temperature, uint64_t version, void* stream) {
    return guarded("bgx_set_weights_device", [&]() -> int {
        (void)version;
        // (the argument checks read nothing of *e)
        if (!e) return fail(BGX_E_ARG, "bgx_set_weights_device: null engine");
        if (!d_params) return fail(BGX_E_ARG, "bgx_set_weights_device: null d_params");
        if ((uintptr_t)d_params % 4 != 0) return fail(BGX_E_ARG, "bgx_set_weights_device: d_params is not 4-byte aligned");
        if (!(temperature > 0.0f)) return fail(BGX_E_ARG, "temperature=%g", (double)temperature);
        HIP_TRY(hipSetDevice(e->device));
        hipStream_t s = (hipStream_t)stream;
        if (!e->wd_info || !e->wd_hinfo || !e->wd_ev) {
            if (int rc = e->wd_info.alloc(4)) return rc;
            if (hipHostMalloc((void**)e->wd_hinfo.put(), sizeof(bgx::PackInfo), hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(e->wd_ev.put(), hipEventDisableTiming) != hipSuccess)
                return fail(BGX_E_HIP, "bgx_set_weights_device: pinned buffer / event creation failed");
        }
        // an engine without a network gets one; it is kept only when the weights pass
        std::unique_ptr<bgx_net> fresh;
        bgx_net* n = e->net.get();
        if (!n) {
            fresh.reset(new bgx_net());
            n = fresh.get();
            if (n->W1.alloc(128 * 198) || n->b1.alloc(128) || n->w2.alloc(128) || n->wfrag.alloc(bgx::PK_NFRAG) ||
                n->rowc.alloc(128 * 4))
                return BGX_E_HIP;
        }
        // the engine's queued steps read the arrays the pack launch rewrites: on
        // another stream the hand-off goes behind them by an event, no host wait
        if (e->last != s) {
            HIP_TRY(hipEventRecord(e->wd_ev, e->last));
            HIP_TRY(hipStreamWaitEvent(s, e->wd_ev, 0));
        }
        bgx::PackInfo* d_info = (bgx::PackInfo*)e->wd_info.get();
        HIP_TRY(bgx_launch_weights_check(d_params, d_info, s));
        HIP_TRY(bgx_launch_weights_pack(d_params, d_info, n->wfrag, n->W1, n->b1, n->w2, n->rowc, s));
        HIP_TRY(hipMemcpyAsync(e->wd_hinfo, d_info, sizeof(bgx::PackInfo), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));   // the call's one host wait: b2 and 2^-e are launch arguments (set_net)
        bgx::PackInfo pi;
        std::memcpy(&pi, e->wd_hinfo, sizeof(pi));
        if (pi.rule != bgx::PK_RULE_OK) {   // net_upload's messages; the pack launch wrote nothing
            const int at = pi.index;
            const char* name = at < bgx::PK_B1 ? "W1" : at < bgx::PK_W2 ? "b1" : at < bgx::PK_B2 ? "w2" : "b2";
            const int idx = at < bgx::PK_B1 ? at : at < bgx::PK_W2 ? at - bgx::PK_B1 : at < bgx::PK_B2 ? at - bgx::PK_W2 : 0;
            if (pi.rule == bgx::PK_RULE_NONFINITE) return fail(BGX_E_ARG, "weights: %s[%d] is not finite", name, idx);
            float v = 0.0f;
            HIP_TRY(hipMemcpy(&v, d_params + at, 4, hipMemcpyDeviceToHost));
            return fail(BGX_E_ARG, "weights: %s[%d] = %g: max|log2(e) w| must stay below 2^26 (split-fp16 scaling limit)",
                        name, idx, (double)v);
        }
        float b2 = 0.0f;
        std::memcpy(&b2, &pi.b2_bits, 4);
        const float feat_scale = (float)std::ldexp(1.0, -pi.e);
        // a captured graph holds the temperature, and with it b2 and 2^-e, by
        // value (enqueue_steps' set_net): dropped when any of the three changes
        if (e->d.temperature != temperature || n->b2 != b2 || n->feat_scale != feat_scale)
            if (int rc = drop_graph(e)) return rc;
        n->feat_scale = feat_scale;
        n->b2 = b2;
        if (fresh) e->net = std::move(fresh);
        e->d.temperature = temperature;
        return BGX_OK;
    });
}

int bgx_engine_set_opponent(bgx_engine* e, const float* h_W1, const float* h_b1, const float* h_w2,
                            const float* h_b2) {
    return guarded("bgx_engine_set_opponent", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_engine_set_opponent: null engine");
        const bool none = !h_W1 && !h_b1 && !h_w2 && !h_b2;
        if (!none && (!h_W1 || !h_b1 || !h_w2 || !h_b2))
            return fail(BGX_E_ARG, "bgx_engine_set_opponent: all four weight arrays, or all null to leave match mode");
        if (e->fused)
            return fail(BGX_E_STATE, "bgx_engine_set_opponent: match mode needs the phased engine (fused = 0 or ply = 2)");
        if (e->zt)
            return fail(BGX_E_STATE, "bgx_engine_set_opponent: match mode does not combine with BGX_REPLY_DELTA (the "
                                     "replies would start from the wrong network's root accumulators)");
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        if (none) {
            if (!e->match) return BGX_OK;
            e->match = false;
            e->d.match_ctr = nullptr;
            return restart_lanes(e);
        }
        if (e->match) return net_upload(e->m->net1.get(), h_W1, h_b1, h_w2, h_b2);   // replace network 1: no restart
        if (e->m) {
            if (int rc = net_upload(e->m->net1.get(), h_W1, h_b1, h_w2, h_b2)) return rc;
        } else {
            std::unique_ptr<MatchState> m(new MatchState());
            bgx_net* n1 = nullptr;
            if (int rc = bgx_net_create(h_W1, h_b1, h_w2, h_b2, &n1)) return rc;
            m->net1.reset(n1);
            const size_t root_n = (size_t)e->cfg.lanes + (size_t)e->cand_cap;
            for (int n = 0; n < 2; ++n) {
                if (int rc = m->list[n].alloc(root_n)) return rc;
                HIP_TRY(hipMemset(m->list[n], 0xFF, m->list[n].bytes()));   // -1: an empty row
                if (e->cfg.ply == 2) {
                    if (int rc = m->rlist[n].alloc((size_t)e->reply_cap)) return rc;
                    HIP_TRY(hipMemset(m->rlist[n], 0xFF, m->rlist[n].bytes()));
                }
            }
            if (e->cfg.ply == 2) {
                m->slots = e->cfg.k_top == 4 ? 4 * e->cfg.lanes : e->cand_cap;
                if (int rc = m->slot.alloc((size_t)m->slots)) return rc;
                HIP_TRY(hipMemset(m->slot, 0, m->slot.bytes()));
            }
            if (int rc = m->ctr.alloc(8)) return rc;
            e->m = std::move(m);
        }
        HIP_TRY(hipMemset(e->m->ctr, 0, e->m->ctr.bytes()));
        e->match = true;
        e->d.match_ctr = e->m->ctr;
        return restart_lanes(e);
    });
}

int bgx_engine_set_start(bgx_engine* e, const uint8_t* h_boards, const uint8_t* h_player, const uint8_t* h_dice,
                         int n_pos, uint32_t strat_stride) {
    return guarded("bgx_engine_set_start", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_engine_set_start: null engine");
        const bool none = n_pos == 0 && !h_boards && !h_player && !h_dice;
        if (!none && (!h_boards || !h_player || n_pos <= 0))
            return fail(BGX_E_ARG, "bgx_engine_set_start: boards and players of n_pos > 0 positions, or all null with "
                                   "n_pos = 0 to leave rollout mode (n_pos=%d)", n_pos);
        if (e->fused)
            return fail(BGX_E_STATE, "bgx_engine_set_start: rollout mode needs the phased engine (fused = 0 or ply = 2)");
        // every position is checked before anything is uploaded
        std::vector<uint32_t> tab((size_t)(none ? 0 : n_pos) * 8);
        for (int i = 0; i < n_pos; ++i) {
            const uint8_t* b = h_boards + (size_t)i * 52;
            if (const unsigned bad = bgx::domain_bits(b, (int)h_player[i], nullptr))
                return fail(BGX_E_ARG, "bgx_engine_set_start: position %d outside the input domain (bits 0x%x: 1 shared "
                                       "point, 2 more than 15 checkers, 4 a count above 15, 16 player not 0 / 1)", i, bad);
            unsigned sum[2] = {(unsigned)b[48] + b[50], (unsigned)b[49] + b[51]};
            for (int k = 0; k < 24; ++k) {
                sum[0] += b[k];
                sum[1] += b[24 + k];
            }
            if (sum[0] != 15 || sum[1] != 15)
                return fail(BGX_E_ARG, "bgx_engine_set_start: position %d has %u and %u checkers (15 each: points + bar + "
                                       "off)", i, sum[0], sum[1]);
            if (b[50] >= 15 || b[51] >= 15)
                return fail(BGX_E_ARG, "bgx_engine_set_start: position %d is already over (15 checkers off)", i);
            const unsigned d0 = h_dice ? h_dice[2 * (size_t)i] : 0u, d1 = h_dice ? h_dice[2 * (size_t)i + 1] : 0u;
            if (!(d0 == 0 && d1 == 0) && (d0 < 1 || d0 > 6 || d1 < 1 || d1 > 6))
                return fail(BGX_E_ARG, "bgx_engine_set_start: position %d has dice %u, %u (0, 0 = roll, or two values in "
                                       "1..6)", i, d0, d1);
            uint32_t* w = tab.data() + (size_t)i * 8;
            for (int k = 0; k < 48; ++k) w[k >> 3] |= (uint32_t)b[k] << (4 * (k & 7));
            w[6] = (uint32_t)b[48] | (uint32_t)b[49] << 4 | (uint32_t)b[50] << 8 | (uint32_t)b[51] << 12 |
                   (uint32_t)h_player[i] << 16;
            w[7] = (uint32_t)h_player[i] | d0 << 8 | d1 << 16;
        }
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        if (none && !e->start_tab) return BGX_OK;
        // the new table is complete on the device before the old one goes: a
        // failure up to here leaves the engine in the mode and games it had
        DevBuf<uint32_t> fresh;
        if (!none) {
            if (int rc = fresh.alloc(tab.size())) return rc;
            const hipError_t ec = hipMemcpy(fresh, tab.data(), fresh.bytes(), hipMemcpyHostToDevice);
            if (ec != hipSuccess)
                return fail(BGX_E_HIP, "bgx_engine_set_start: table upload failed: %s", hipGetErrorString(ec));
        }
        e->start_tab = std::move(fresh);   // frees the old table
        e->d.start_tab = e->start_tab;
        e->d.n_pos = none ? 0 : n_pos;
        e->d.strat_stride = none ? 0u : strat_stride;
        return restart_lanes(e);
    });
}

int bgx_get_stats(bgx_engine* e, bgx_stats* out) {
    return guarded("bgx_get_stats", [&]() -> int {
        if (!e || !out) return fail(BGX_E_ARG, "bgx_get_stats: null pointer");
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        std::vector<unsigned long long> st(kStatWords);
        HIP_TRY(hipMemcpy(st.data(), e->stats, e->stats.bytes(), hipMemcpyDeviceToHost));
        for (int i = 8; i < kStatWords; ++i) st[7] += st[i];   // the top-5 launch's per-wave record counts
        // decisions = records written, episodes = games finished: the lanes' own counters
        const int L = e->cfg.lanes;
        std::vector<uint32_t> rec(L), epi(L);
        HIP_TRY(hipMemcpy(rec.data(), e->d.rec_count, (size_t)L * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(epi.data(), e->d.epi, (size_t)L * 4, hipMemcpyDeviceToHost));
        unsigned long long dec = 0, eps = 0;
        for (int i = 0; i < L; ++i) {
            dec += rec[i];
            eps += epi[i];
        }
        out->env_steps = st[0];
        out->decisions = dec;
        out->episodes = eps;
        out->value_rows = st[3];
        out->movegen_jobs = st[4];
        out->fallback_jobs = st[5];
        // 2-ply reply rows reserved minus the records written into them; a step
        // stopped between the top-5 launch (st[7]) and the step kernel (st[6])
        // would make the difference negative, so clamp at zero
        out->gap_rows = st[6] > st[7] ? st[6] - st[7] : 0;
        return BGX_OK;
    });
}

int bgx_engine_peek(bgx_engine* e, int buf, void* h_out, uint64_t bytes, uint64_t* needed) {
    return guarded("bgx_engine_peek", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_engine_peek: null engine");
        const size_t L = (size_t)e->cfg.lanes;
        const void* src = nullptr;
        size_t n = 0;
        if (buf == BGX_PEEK_NET_FRAG) {   // network 0 as the launches read it; fused and phased engines alike
            if (!e->net) return fail(BGX_E_STATE, "bgx_engine_peek: the engine has no network yet");
            const size_t nf = (size_t)bgx::PK_NFRAG * 16;
            if (needed) *needed = nf + 8;
            if (!h_out) return BGX_OK;
            if (bytes < nf + 8) return fail(BGX_E_ARG, "bgx_engine_peek: %llu bytes < %zu", (unsigned long long)bytes, nf + 8);
            HIP_TRY(hipSetDevice(e->device));
            if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
            HIP_TRY(hipMemcpy(h_out, e->net->wfrag, nf, hipMemcpyDeviceToHost));
            const float tail[2] = {e->net->feat_scale, e->net->b2};
            std::memcpy((char*)h_out + nf, tail, 8);
            return BGX_OK;
        }
        switch (buf) {
        case BGX_PEEK_LANE_ROWS: src = e->rows; n = L * 8 * 4; break;
        case BGX_PEEK_PLAYER: src = e->d.player; n = L; break;
        case BGX_PEEK_DICE: src = e->d.dice; n = 2 * L; break;
        case BGX_PEEK_CAND_OFF: src = e->cand_off; n = L * 4; break;
        case BGX_PEEK_CAND_CNT: src = e->cand_cnt; n = L * 4; break;
        case BGX_PEEK_CAND_ROWS: src = e->rows + L * 8; n = (size_t)e->cand_cap * 8 * 4; break;
        case BGX_PEEK_VALUES: src = e->V; n = (L + (size_t)e->cand_cap) * 4; break;
        case BGX_PEEK_SEL: src = e->sel; n = e->sel ? 4 * L * 4 : 0; break;
        case BGX_PEEK_JOB_VAL: src = e->job_val; n = e->job_val ? (size_t)e->jobs_cap * 4 : 0; break;
        default: return fail(BGX_E_ARG, "bgx_engine_peek: unknown buffer %d", buf);
        }
        if (e->fused && buf != BGX_PEEK_PLAYER && buf != BGX_PEEK_DICE)
            return fail(BGX_E_STATE, "bgx_engine_peek: buffer %d is not kept by the fused engine", buf);
        if (!src || n == 0) return fail(BGX_E_STATE, "bgx_engine_peek: buffer %d not allocated (ply %d)", buf, e->cfg.ply);
        if (needed) *needed = n;
        if (!h_out) return BGX_OK;
        if (bytes < n) return fail(BGX_E_ARG, "bgx_engine_peek: %llu bytes < %zu", (unsigned long long)bytes, n);
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        HIP_TRY(hipMemcpy(h_out, src, n, hipMemcpyDeviceToHost));
        return BGX_OK;
    });
}

int bgx_set_timing(bgx_engine* e, int enabled) {
    return guarded("bgx_set_timing", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_set_timing: null engine");
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        e->ev.clear();
        e->ev_kind.clear();
        e->ms_mg = e->ms_mlp = 0;
        e->n_mg = e->n_mlp = 0;
        e->timing = enabled != 0;
        return BGX_OK;
    });
}

int bgx_get_timing(bgx_engine* e, double* ms_movegen, int* n_movegen, double* ms_mlp, int* n_mlp) {
    return guarded("bgx_get_timing", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_get_timing: null engine");
        HIP_TRY(hipSetDevice(e->device));
        if (e->last) HIP_TRY(hipStreamSynchronize(e->last));
        for (size_t i = 0; i + 1 < e->ev.size(); i += 2) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
            if (e->ev_kind[i] == 0) { e->ms_mg += ms; e->n_mg++; }
            else { e->ms_mlp += ms; e->n_mlp++; }
        }
        e->ev.clear();
        e->ev_kind.clear();
        if (ms_movegen) *ms_movegen = e->ms_mg;
        if (n_movegen) *n_movegen = e->n_mg;
        if (ms_mlp) *ms_mlp = e->ms_mlp;
        if (n_mlp) *n_mlp = e->n_mlp;
        return BGX_OK;
    });
}

}  // extern "C"
