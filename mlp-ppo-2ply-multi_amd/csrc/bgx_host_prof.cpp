// bgx_host_prof.cpp — the fused development report (bgx_prof.h).
#include "bgx_prof.h"

#include <algorithm>
#include <utility>
#include <vector>

void fused_prof_report(const unsigned long long* p, int n_slots, FILE* out, const char* dump_path) {
    constexpr size_t W = kProfSlotWords;
    double s[W] = {0};   // every word summed over the workgroups (per-launch clocks included, unused)
    for (int b = 0; b < n_slots; ++b)
        for (size_t k = 0; k < W; ++k) s[k] += (double)p[(size_t)b * W + k];
    const double n = s[5] > 0 ? s[5] : 1;
    const double nws = s[18] > 0 ? s[18] : 1;   // wave-steps
    // (the pipelined kernel: each step is tier 2 + the row prefix, then one item
    // queue of MLP tiles, choice pairs and the next step's tier-1 jobs)
    fprintf(out, "[bgx fused prof] us per workgroup step: tier2 + prefix %.2f, queue %.2f, end barrier %.2f "
            "(%.0f workgroup steps)\n", s[1] / n / 100, s[3] / n / 100, s[4] / n / 100, n);
    fprintf(out, "[bgx fused prof] wave-us per workgroup step in items: MLP tiles %.2f, choice pairs %.2f, "
            "tier-1 jobs %.2f (%.2f per wave-step of %d waves)\n", s[8] / n / 100, s[10] / n / 100,
            (s[14] + s[16]) / n / 100, (s[8] + s[10] + s[14] + s[16]) / nws / 100, (int)(nws / n + 0.5));
    fprintf(out, "[bgx fused prof] choice per wave-step: state + Philox refill %.2f, pick %.2f, "
            "env step %.2f us\n", s[29] / nws / 100, s[30] / nws / 100, s[31] / nws / 100);
    // the draw item (one per step queue, step -1's included; words 95..97:
    // clocks, of them waiting for the step's choices, count); the first
    // figure of the line above is the state load plus the slot read
    fprintf(out, "[bgx fused prof] draw item: %.2f us each, %.2f of it waiting for the choices (%.0f items, "
            "%.2f per workgroup step)\n", s[95] / (s[97] > 0 ? s[97] : 1) / 100,
            s[96] / (s[97] > 0 ? s[97] : 1) / 100, s[97], s[97] / n);
    fprintf(out, "[bgx fused prof] MLP tiles per workgroup step: rows + k mask %.2f, MFMA chain issue %.2f, "
            "drain + epilogue %.2f wave-us\n", s[6] / n / 100, s[22] / n / 100, s[23] / n / 100);
    // step durations by index within a launch (every launch, every workgroup):
    // words 32.. the summed durations, 64.. their counts, 56 / 57 the later steps'
    fprintf(out, "[bgx fused prof] step us by index in the launch (workgroup-steps):");
    for (int k = 0; k < 24; ++k)
        fprintf(out, " %.2f (%.0f)", s[64 + k] > 0 ? s[32 + k] / s[64 + k] / 100 : 0.0, s[64 + k]);
    fprintf(out, "; later steps %.2f (%.0f)\n", s[57] > 0 ? s[56] / s[57] / 100 : 0.0, s[57]);
    fprintf(out, "[bgx fused prof] tier-2 jobs %.0f (%.0f reached tier 3), %.1f us each\n", s[12], s[13],
            s[11] / (s[12] > 0 ? s[12] : 1) / 100);
    fprintf(out, "[bgx fused prof] tier-1 job: doubles %.2f us (%.0f jobs), non-doubles %.2f us (%.0f jobs)\n",
            s[14] / (s[15] > 0 ? s[15] : 1) / 100, s[15], s[16] / (s[17] > 0 ? s[17] : 1) / 100, s[17]);
    // pairing: the non-doubles jobs that took the rule-mode two-move branch
    // alone (words 88 / 89: clocks, count) against all item clocks, how often a
    // pipelined claim of a rule-mode non-doubles lane saw a second such lane
    // ready and unclaimed (words 90..92: claims, of such a lane, with a
    // partner), and the pair items (words 93 / 94: clocks, count; their clocks
    // are in no other word)
    const double items = s[8] + s[10] + s[14] + s[16] + s[93];
    fprintf(out, "[bgx fused prof] tier-1 rule-mode two-move job: %.2f us (%.0f jobs), %.2f wave-us per workgroup "
            "step, %.1f %% of the item wave-us\n", s[88] / (s[89] > 0 ? s[89] : 1) / 100, s[89], s[88] / n / 100,
            100.0 * s[88] / (items > 0 ? items : 1));
    fprintf(out, "[bgx fused prof] pipelined job claims %.0f: %.0f of a rule-mode non-doubles lane, %.0f of them "
            "(%.1f %%) with a second such lane ready and unclaimed\n", s[90], s[91], s[92],
            100.0 * s[92] / (s[91] > 0 ? s[91] : 1));
    fprintf(out, "[bgx fused prof] tier-1 pair items: %.0f pairs formed (%.2f per workgroup step), %.2f us each, "
            "%.2f wave-us per workgroup step\n", s[94], s[94] / n, s[93] / (s[94] > 0 ? s[94] : 1) / 100,
            s[93] / n / 100);
    // the waits of every wave (words 98..100, lane 0 of each wave): the choice
    // items' wait for their tiles, the job items' claim (mask polls and
    // fetch-ands, bgx_claim.h), the step's end barrier
    fprintf(out, "[bgx fused prof] waits per wave-step: choice tile wait %.2f, job claim %.2f, end barrier %.2f us "
            "(%.2f, %.2f, %.2f wave-us per workgroup step)\n", s[98] / nws / 100, s[99] / nws / 100,
            s[100] / nws / 100, s[98] / n / 100, s[99] / n / 100, s[100] / n / 100);
    // the last launch, per workgroup: duration spread, dispatch skew, and the
    // rows / tier-2 jobs of the slowest vs the median workgroup
    std::vector<std::pair<double, int>> dur;
    unsigned long long b_min = ~0ull, b_max = 0, e_max = 0;
    for (int b = 0; b < n_slots; ++b) {
        const unsigned long long* q = &p[(size_t)b * W];
        if (q[25] <= q[24]) continue;
        dur.push_back({(double)(q[25] - q[24]) / 100.0, b});
        b_min = q[24] < b_min ? q[24] : b_min;
        b_max = q[24] > b_max ? q[24] : b_max;
        e_max = q[25] > e_max ? q[25] : e_max;
    }
    if (dump_path) {
        // the last launch per workgroup: begin / end clocks (100 MHz),
        // loop start / end, rows, tier-2 jobs, lane-steps
        if (FILE* fp = fopen(dump_path, "w")) {
            fprintf(fp, "wg,begin,end,loop0,loop1,rows,tier2,lane_steps\n");
            for (int b = 0; b < n_slots; ++b) {
                const unsigned long long* q = &p[(size_t)b * W];
                if (q[25] <= q[24]) continue;
                fprintf(fp, "%d,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n", b, q[24], q[25], q[19], q[20], q[26],
                        q[27], q[28]);
            }
            fclose(fp);
        }
    }
    if (!dur.empty()) {
        std::sort(dur.begin(), dur.end());
        double mean = 0;
        for (auto& d : dur) mean += d.first;
        mean /= (double)dur.size();
        const size_t nd = dur.size();
        const unsigned long long* qm = &p[(size_t)dur[nd / 2].second * W];
        const unsigned long long* qx = &p[(size_t)dur[nd - 1].second * W];
        fprintf(out, "[bgx fused prof] last launch, %zu workgroups: duration us min %.1f p50 %.1f mean %.1f "
                "p90 %.1f max %.1f; begin skew %.1f us, span %.1f us; lane-steps %llu; rows / tier-2 jobs: "
                "median workgroup %llu / %llu, slowest %llu / %llu\n",
                nd, dur[0].first, dur[nd / 2].first, mean, dur[(nd * 9) / 10].first, dur[nd - 1].first,
                (double)(b_max - b_min) / 100.0, (double)(e_max - b_min) / 100.0, qx[28], qm[26], qm[27],
                qx[26], qx[27]);
        // launch shape (median workgroup): prologue (W fragments, LUT, lane
        // state), the step loop, epilogue (lane state back); shader clock
        // over the workgroup's span (s_memtime cycles / 100 MHz wall clock)
        std::vector<double> pro, loop, epi, mhz;
        for (auto& d : dur) {
            const unsigned long long* q = &p[(size_t)d.second * W];
            if (q[19] < q[24] || q[20] < q[19] || q[25] < q[20]) continue;
            pro.push_back((double)(q[19] - q[24]) / 100.0);
            loop.push_back((double)(q[20] - q[19]) / 100.0);
            epi.push_back((double)(q[25] - q[20]) / 100.0);
            mhz.push_back((double)q[21] / ((double)(q[25] - q[24]) / 100.0));
        }
        if (!pro.empty()) {
            auto med = [](std::vector<double>& v) {
                std::sort(v.begin(), v.end());
                return v[v.size() / 2];
            };
            fprintf(out, "[bgx fused prof] last launch shape (median workgroup): prologue %.1f us, step loop "
                    "%.1f us, epilogue %.1f us; shader clock %.0f MHz\n", med(pro), med(loop), med(epi),
                    med(mhz));
        }
    }
}
