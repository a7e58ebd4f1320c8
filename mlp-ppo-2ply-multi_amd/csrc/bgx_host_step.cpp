// bgx_host_step.cpp — stepping and harvest: the per-step launch sequence of
// the phased engines, the fused engine's persistent launch, bgx_step /
// bgx_sync and the harvest tickets.
#include <chrono>

#include "bgx_host.h"

int flag_error(unsigned f) {
    return fail(f & BGX_ERRF_WAIT_BOUND ? BGX_E_STATE : BGX_E_CAPACITY,
                "device flags 0x%x (1 flat rows, 2 overflow list, 4 fallback workspace, 8 experience ring, "
                "16 episode list, 32 scripted dice: capacity; 64 an intra-workgroup wait hit its bound: state)", f);
}

// after the engine's stream is synchronized: the flags raised since the last
// harvest ticket (they move into a ticket's totals when it is harvested, and
// bgx_harvest_fetch reports them there). The engine word is reset here; a
// fused engine's launches have already moved theirs into the open ticket's
// accumulator, which is reported but left for the ticket.
int check_flags(bgx_engine* e) {
    unsigned f = 0;
    HIP_TRY(hipMemcpy(&f, e->ctr + C_ERR, 4, hipMemcpyDeviceToHost));
    if (f) HIP_TRY(hipMemset(e->ctr + C_ERR, 0, 4));
    if (e->fh_ctr) {
        unsigned long long acc = 0;
        HIP_TRY(hipMemcpy(&acc, e->hv_flags(e->h_tickets), 8, hipMemcpyDeviceToHost));
        f |= (unsigned)acc;
    }
    return f ? flag_error(f) : BGX_OK;
}

static void mg_common(bgx_engine* e, bgx::MovegenArgs& a) {
    set_fallback(a, e->ctr + C_OVF, e->ovf_list, e->ovf_cap, e->ws, e->ws_waves, e->ws_slots, e->ctr + C_ERR);
    a.ovf_zeroed = 1;   // the per-step memset covers it
}

static int timed(bgx_engine* e, int kind, hipStream_t s, bool start) {
    if (!e->timing) return BGX_OK;
    Event ev;
    HIP_TRY(hipEventCreate(ev.put()));
    HIP_TRY(hipEventRecord(ev, s));
    e->ev.push_back(std::move(ev));
    e->ev_kind.push_back(start ? kind : -1);
    return BGX_OK;
}

// match mode: the routing kernels' arguments (root and reply launch share them)
static bgx::MatchRouteArgs match_route_args(bgx_engine* e) {
    const int L = e->cfg.lanes;
    bgx::MatchRouteArgs a{};
    a.L = L;
    a.lane_base = e->cfg.lane_base;
    a.cand_cap = e->cand_cap;
    a.player = e->d.player;
    a.epi = e->d.epi;
    a.cand_off = e->cand_off;
    a.cand_cnt = e->cand_cnt;
    a.flat_count = e->ctr + C_FLAT;
    a.list[0] = e->m->list[0];
    a.list[1] = e->m->list[1];
    a.count = e->m->ctr;
    a.slot_net = e->m->slot;
    a.k_top = e->cfg.k_top;
    a.n_slots = e->m->slots;
    if (e->cfg.ply == 2) {
        if (e->cfg.k_top == 4) {
            a.n_jobs = L * 4 * 21;
        } else {
            a.n_units_dev = e->ctr + C_FLAT;
            a.n_jobs_max = e->jobs_cap;
        }
        a.job_off = e->job_off;
        a.job_cnt = e->job_cnt;
        a.reply_cap = e->reply_cap;
        a.rlist[0] = e->m->rlist[0];
        a.rlist[1] = e->m->rlist[1];
        a.rcount = e->m->ctr + 2;
    }
    return a;
}

// ... and a routed launch's: the root launch (lane rows + candidates, one tile
// per wave iteration) or the 2-ply reply launch (two tiles)
static bgx::MatchMlpArgs match_mlp_args(bgx_engine* e, bool reply) {
    bgx::MatchMlpArgs m{};
    m.rows = reply ? e->reply_rows : e->rows;
    m.out = reply ? e->reply_V : e->V;
    m.n_max = reply ? e->reply_cap : e->cfg.lanes + e->cand_cap;
    m.list_cap = m.n_max;
    m.nt = reply ? 2 : 1;
    const bgx_net* nets[2] = {e->net.get(), e->m->net1.get()};
    for (int n = 0; n < 2; ++n) {
        m.list[n] = reply ? e->m->rlist[n] : e->m->list[n];
        m.count[n] = e->m->ctr + (reply ? 2 : 0) + n;
        m.claim[n] = e->m->ctr + (reply ? 6 : 4) + n;
        set_net(m, n, nets[n]);
    }
    return m;
}

// the per-step launch sequence (captured into a graph by bgx_step)
static int enqueue_steps(bgx_engine* e, int n_steps, hipStream_t s) {
    const int L = e->cfg.lanes;
    for (int it = 0; it < n_steps; ++it) {
        // the per-step counters (flat, reply, ovf, ovf2) are zero here: engine
        // create zeroes them and every step's last kernel resets them
        bgx::MovegenArgs a{};
        a.n_jobs = L;
        a.in_mode = bgx::IN_PACKED;
        a.in_packed = e->rows;
        a.in_player = e->d.player;
        a.in_dice = e->d.dice;
        a.out_mode = bgx::OUT_PACKED_FLAT;
        a.out_packed = e->rows + (size_t)L * 8;
        a.flat_count = e->ctr + C_FLAT;
        a.flat_cap = e->cand_cap;
        a.job_off = e->cand_off;
        a.job_cnt = e->cand_cnt;
        mg_common(e, a);
        if (timed(e, 0, s, true)) return BGX_E_HIP;
        HIP_TRY(bgx_launch_movegen(&a, s));
        if (timed(e, 0, s, false)) return BGX_E_HIP;

        bgx::MlpArgs m{};
        m.rows = e->rows;
        m.n_rows = L;
        m.n_rows_dev = e->ctr + C_FLAT;
        m.n_max = L + e->cand_cap;
        m.out = e->V;
        set_net(m, e->net.get());
        if (e->zt && e->cfg.k_top != 4) {   // 2-ply K = all: every candidate's accumulators (the reply roots)
            m.zout = e->zt;
            m.z_base = L;
        }
        if (timed(e, 1, s, true)) return BGX_E_HIP;
        if (e->match) {   // rows sorted by the mover's network, then one routed launch
            const bgx::MatchRouteArgs ra = match_route_args(e);
            HIP_TRY(bgx_launch_route_root(&ra, s));
            const bgx::MatchMlpArgs mm = match_mlp_args(e, false);
            HIP_TRY(bgx_launch_mlp_routed(&mm, s));
        } else {
            HIP_TRY(bgx_launch_mlp(&m, s));
        }
        if (timed(e, 1, s, false)) return BGX_E_HIP;

        if (e->cfg.ply == 2) {
            bgx::MovegenArgs b{};
            b.in_mode = bgx::IN_TWOPLY;
            b.in_packed = e->rows;
            if (e->cfg.k_top == 4) {
                HIP_TRY(bgx_launch_topk(&e->d, s));
                if (e->zt) {   // the chosen rows' accumulators, indexed by reply root slot (4 lane + k)
                    bgx::MlpArgs z{};
                    z.rows = e->sel_rows;
                    z.n_rows = 4 * L;
                    z.nt = 1;
                    z.out = e->zv;
                    set_net(z, e->net.get());
                    z.zout = e->zt;
                    z.z_base = 0;
                    HIP_TRY(bgx_launch_mlp(&z, s));
                }
                b.n_jobs = L * 4 * 21;
                b.in_packed = e->sel_rows;   // the top-k kernel's copies of the chosen rows
                b.in_rows = nullptr;
                b.in_row_base = 0;
            } else {
                b.n_jobs = 0;
                b.n_jobs_dev = e->ctr + C_FLAT;
                b.jobs_per_dev_unit = 21;
                b.n_jobs_max = e->jobs_cap;
                b.in_rows = nullptr;
                b.in_row_base = L;
            }
            b.out_mode = bgx::OUT_PACKED_FLAT;
            b.out_packed = e->reply_rows;
            b.flat_count = e->ctr + C_REPLY;
            b.flat_cap = e->reply_cap;
            // output-row reservations: the reply launch's workgroups take chunks of
            // up to 8 x flat_chunk rows per global atomic (bgx_movegen.h wg_take),
            // the per-roll pool kernel's waves chunks of up to flat_chunk; a
            // chunk's unwritten tail is gap rows the reply MLP evaluates
            // (bgx_stats.gap_rows)
            b.flat_chunk = reply_flat_chunk();
            b.job_off = e->job_off;
            b.job_cnt = e->job_cnt;
            mg_common(e, b);
            b.ovf_count = e->ctr + C_OVF2;
            if (timed(e, 0, s, true)) return BGX_E_HIP;
            HIP_TRY(bgx_launch_movegen(&b, s));
            if (timed(e, 0, s, false)) return BGX_E_HIP;
            bgx::MlpArgs r{};
            r.rows = e->reply_rows;
            r.n_rows = 0;
            r.n_rows_dev = e->ctr + C_REPLY;
            r.n_max = e->reply_cap;
            r.nt = 2;
            r.out = e->reply_V;
            set_net(r, e->net.get());
            if (e->zt) {   // replies by difference from their roots (mlp_kernel_delta)
                const bool k4 = e->cfg.k_top == 4;
                r.zt = e->zt;
                r.root_rows = k4 ? e->sel_rows : e->rows;   // K = 4: the top-k kernel's copies, by slot
                r.root_sel = nullptr;
                r.root_base = k4 ? 0 : L;
                r.n_roots = k4 ? 4 * L : e->cand_cap;
                r.n_slots = r.n_roots;
            }
            if (timed(e, 1, s, true)) return BGX_E_HIP;
            if (e->match) {   // each job's rows to the list of its root slot's network
                const bgx::MatchRouteArgs ra = match_route_args(e);
                HIP_TRY(bgx_launch_route_reply(&ra, s));
                const bgx::MatchMlpArgs mm = match_mlp_args(e, true);
                HIP_TRY(bgx_launch_mlp_routed(&mm, s));
            } else {
                HIP_TRY(bgx_launch_mlp(&r, s));
            }
            if (timed(e, 1, s, false)) return BGX_E_HIP;
            // reference-sampled mode (cfg.reply_sample > 0): keyed by the seed and the
            // lane block, salted per step by the engine's env-step counter
            const uint64_t skey = e->cfg.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(e->cfg.lane_base + 1));
            if (e->cfg.k_top == 4) {
                HIP_TRY(bgx_launch_top5(e->reply_V, e->job_off, e->job_cnt, L * 4 * 21, nullptr, 0, L * 4 * 21,
                                        e->job_val, e->cfg.reply_sample, skey, e->stats, e->stats + 8, s));
            } else {
                HIP_TRY(bgx_launch_top5(e->reply_V, e->job_off, e->job_cnt, 0, e->ctr + C_FLAT, 21, e->jobs_cap,
                                        e->job_val, e->cfg.reply_sample, skey, e->stats, e->stats + 8, s));
            }
        }
        HIP_TRY(bgx_launch_select(&e->d, s));   // select + env step (one launch)
    }
    return BGX_OK;
}

// fused 1-ply: one persistent launch for all n_steps (bgx_fused.hip)
static int enqueue_fused(bgx_engine* e, int n_steps, hipStream_t s) {
    bgx::FusedArgs f{};
    f.e = e->d;
    f.cand = e->fcand;
    f.vbuf = e->fvbuf;
    f.t1cnt = e->ft1cnt;
    f.t1_ready = e->t1_ready ? 1 : 0;
    f.cap = e->fcap;
    f.n_steps = n_steps;
    set_net(f, e->net.get());
    f.ws_global = e->ws;
    f.ws_blocks = e->ws_waves;
    f.ws_slots = e->ws_slots;
    f.ws_words_per_block = (size_t)5 * e->ws_slots;
    f.force_tier = e->force_tier;
    f.lanes_per_wg = e->fused_fl;
    f.pair = e->fused_pair;
    if (e->cfg.balance) {   // n_steps x lanes lane-steps; a lane runs at most n + n/4 + 4 (ring headroom)
        f.budget = (long long)n_steps * (long long)e->cfg.lanes;
        const int headroom = e->cfg.ring - e->cfg.max_steps;
        const int cap = n_steps + n_steps / 4 + 4;
        f.n_cap = cap < headroom ? cap : headroom;
        f.budget_ctr = (unsigned long long*)(e->ctr + C_BUDGET);
    }
    {   // in-kernel harvest into the slot of the next ticket
        const int b = e->h_tickets % NHB;
        f.hv_hdr = e->out_headers[b];
        f.hv_rec = e->out_records[b];
        f.hv_ep_cap = e->d.ep_cap;
        f.hv_rec_cap = (long long)e->cfg.lanes * e->cfg.ring;
        f.hv_ctr = e->hv_total(b);
        f.hv_next = e->hv_total(b + 1);
        f.hv_flags = e->hv_flags(b);
        f.hv_next_flags = e->hv_flags(b + 1);
        f.hv_commit = e->hv_commit(b);
        f.hv_next_commit = e->hv_commit(b + 1);
        f.hv_info = e->d_info[b];
        f.hv_hinfo = e->h_info_dev + 4 * b;
        f.done_ctr = e->hv_done();
    }
    if (e->prof_enabled) {
        if (!e->fprof) {
            if (e->fprof.alloc((size_t)kProfSlots * kProfSlotWords)) return BGX_E_HIP;
            HIP_TRY(hipMemset(e->fprof, 0, e->fprof.bytes()));
        }
        f.prof = e->fprof;
    }
    if (timed(e, 0, s, true)) return BGX_E_HIP;
    HIP_TRY(bgx_launch_fused(&f, s));
    e->t1_ready = true;   // the launch ends with every lane's next position expanded
    e->fh_launched = true;
    if (timed(e, 0, s, false)) return BGX_E_HIP;
    return BGX_OK;
}

// Wait for a harvest event: poll it for up to 2 ms (a short launch's harvest
// lands within that; a blocking wait adds the runtime's wake-up after the
// kernel ends), then block. BGX_SPIN_WAIT=0: block at once (A/B).
static hipError_t wait_event(hipEvent_t ev) {
    static const int spin = [] {
        const char* v = getenv("BGX_SPIN_WAIT");
        return v ? atoi(v) : 1;
    }();
    if (spin) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipEventQuery(ev);
            if (q != hipErrorNotReady) return q;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000)) break;
        }
    }
    return hipEventSynchronize(ev);
}

extern "C" {

int bgx_step(bgx_engine* e, int n_steps, void* stream) {
    return guarded("bgx_step", [&]() -> int {
        if (!e || n_steps < 0) return fail(BGX_E_ARG, "bgx_step: bad arguments");
        if (!e->net) return fail(BGX_E_STATE, "bgx_step: bgx_set_weights first");
        if (n_steps > e->cfg.ring - e->cfg.max_steps)
            return fail(BGX_E_ARG, "bgx_step: n_steps=%d > ring - max_steps = %d (harvest more often)", n_steps,
                        e->cfg.ring - e->cfg.max_steps);
        HIP_TRY(hipSetDevice(e->device));
        hipStream_t s = (hipStream_t)stream;
        // an enqueued harvest on another stream reads the rings and resets the
        // episode list: the step waits for it (an event, no host wait)
        if (e->h_tickets > 0 && e->hstream != s)
            HIP_TRY(hipStreamWaitEvent(s, e->hdone[(e->h_tickets - 1) % NHB], 0));
        e->last = s;
        if (n_steps == 0) return BGX_OK;
        // timed runs launch directly (events between the kernels); otherwise the
        // n_steps sequence is one graph launch (kernel arguments are fixed for the
        // engine's lifetime; bgx_set_weights drops the graph: temperature is an argument)
        if (e->fused) return enqueue_fused(e, n_steps, s);
        // (a match engine launches directly too: no graph is captured in match mode)
        if (e->timing || !e->use_graph || e->match) return enqueue_steps(e, n_steps, s);
        if (!e->gexec || e->g_steps != n_steps) {
            if (int rc = drop_graph(e)) return rc;
            if (!e->cap) HIP_TRY(hipStreamCreateWithFlags(e->cap.put(), hipStreamNonBlocking));
            HIP_TRY(hipStreamBeginCapture(e->cap, hipStreamCaptureModeRelaxed));
            const int rc = enqueue_steps(e, n_steps, e->cap);
            hipGraph_t g = nullptr;
            const hipError_t ec = hipStreamEndCapture(e->cap, &g);
            if (rc) {
                if (g) (void)hipGraphDestroy(g);
                return rc;
            }
            HIP_TRY(ec);
            const hipError_t ei = hipGraphInstantiate(e->gexec.put(), g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            HIP_TRY(ei);
            e->g_steps = n_steps;
        }
        HIP_TRY(hipGraphLaunch(e->gexec, s));
        return BGX_OK;
    });
}

int bgx_sync(bgx_engine* e) {
    return guarded("bgx_sync", [&]() -> int {
        if (!e) return fail(BGX_E_ARG, "bgx_sync: null engine");
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->last));
        return check_flags(e);
    });
}

int bgx_harvest_enqueue(bgx_engine* e, int* ticket, void* stream) {
    return guarded("bgx_harvest_enqueue", [&]() -> int {
        if (!e || !ticket) return fail(BGX_E_ARG, "bgx_harvest_enqueue: null pointer");
        HIP_TRY(hipSetDevice(e->device));
        hipStream_t s = (hipStream_t)stream;
        // order after the engine's last step (another stream): an event, no host wait
        if (e->last != s) {
            if (!e->hev) HIP_TRY(hipEventCreateWithFlags(e->hev.put(), hipEventDisableTiming));
            HIP_TRY(hipEventRecord(e->hev, e->last));
            HIP_TRY(hipStreamWaitEvent(s, e->hev, 0));
        }
        const int t = e->h_tickets, b = t % NHB;
        // offsets and totals on the device (harvest_scan_kernel, which also writes
        // {episodes, records, error flags} into host-mapped memory), then the copy
        // of the finished episodes' headers and records (a persistent grid that
        // reads the episode count on the device: no host round trip in between)
        if (e->fused) {
            // the fused launches since the last ticket harvested into slot b and
            // published its totals; with none, publish the (empty) slot here
            if (!e->fh_launched)
                HIP_TRY(bgx_launch_harvest_close(e->hv_commit(b), e->hv_total(b + 1), e->hv_commit(b + 1), e->hv_flags(b),
                                                 e->hv_flags(b + 1), e->ctr + C_ERR, e->d_info[b],
                                                 e->h_info_dev + 4 * b, s));
            e->fh_launched = false;
        } else {
            HIP_TRY(bgx_launch_harvest_scan(&e->d, e->d_offs[b], e->d_info[b], e->h_info_dev + 4 * b, s));
            HIP_TRY(bgx_launch_harvest_gather(&e->d, e->d_offs[b], e->d_info[b], e->out_headers[b], e->out_records[b],
                                              s));
        }
        HIP_TRY(hipEventRecord(e->hdone[b], s));
        e->hstream = s;
        e->h_tickets = t + 1;
        *ticket = t;
        return BGX_OK;
    });
}

int bgx_harvest_fetch(bgx_engine* e, int ticket, bgx_harvest_info* out) {
    return guarded("bgx_harvest_fetch", [&]() -> int {
        if (!e || !out) return fail(BGX_E_ARG, "bgx_harvest_fetch: null pointer");
        if (ticket < 0 || ticket >= e->h_tickets || ticket < e->h_tickets - 2)
            return fail(BGX_E_ARG, "bgx_harvest_fetch: ticket %d is not one of the last two harvests (%d enqueued)",
                        ticket, e->h_tickets);
        HIP_TRY(hipSetDevice(e->device));
        const int b = ticket % NHB;
        HIP_TRY(wait_event(e->hdone[b]));
        // the ticket's own flags: its harvest (or the last launch before it)
        // moved them out of the engine word on the device, in stream order
        const uint32_t* info = e->h_info + 4 * b;
        const uint32_t flags = info[2];
        if (flags) return flag_error(flags);
        out->n_episodes = (int)info[0];
        out->n_records = (int)info[1];
        out->d_headers = e->out_headers[b];
        out->d_records = e->out_records[b];
        return BGX_OK;
    });
}

int bgx_harvest(bgx_engine* e, bgx_harvest_info* out, void* stream) {
    return guarded("bgx_harvest", [&]() -> int {
        int t = 0;
        if (int rc = bgx_harvest_enqueue(e, &t, stream)) return rc;
        return bgx_harvest_fetch(e, t, out);
    });
}

}  // extern "C"
