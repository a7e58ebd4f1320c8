// tests/cpuwave/pair_check.cpp -- test infrastructure (host build, emulated wave).
// Two rule-mode non-doubles jobs in one wave (job_records_pair, bgx_movegen.h)
// against each job alone (job_records + emit_records) on the fused kernel's
// tier-1 slice: per job the same count and byte-identical boards in the same
// order, nothing written outside each job's `cap` candidate slots (sentinel
// rows around them; the build runs under AddressSanitizer), the 64-word parent
// map zero on return, and "not pairable" with the outputs untouched when a job
// has no two-move play or the combined list does not fit a reduced list.
// Usage: pair_check positions.bin dump.bin [max_pairs]
//   positions.bin: per position 8 packed words, mover, d0, d1 (int32 x 11);
//   positions that are not rule-mode non-doubles are skipped.
//   dump.bin: per kept position its index, count and min(count, cap) rows (for
//   the oracle comparison, tests/test_cpuwave_pair.py).
//   -> one summary line, exit 0 iff clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bgx_movegen.h"

using namespace bgx;

namespace {
// the fused kernel's tier-1 slice at 12 waves (bgx_fused.hip FCfg)
constexpr int P_S = 256, P_F = 160, P_PF = 416, SLICE_WORDS = 64 + 2 * P_PF;
constexpr int CAP = 40;                 // candidate slots per job (below the larger jobs' counts: the cut)
constexpr int NJ = 5, JA = 1, JB = 3;   // output jobs: 0, 2, 4 are guards
constexpr uint32_t SENT = 0xDEADBEEFu;

struct Pos { uint32_t w[8]; int player, d0, d1; };

struct Out {
    std::vector<uint32_t> rows;   // NJ x CAP x 8
    void reset() { rows.assign((size_t)NJ * CAP * 8, SENT); }
    const uint32_t* job(int j) const { return rows.data() + (size_t)j * CAP * 8; }
    bool clean_outside(bool a_too, bool b_too) const {
        for (int j = 0; j < NJ; ++j) {
            if ((j == JA && a_too) || (j == JB && b_too)) continue;
            for (int q = 0; q < CAP * 8; ++q)
                if (job(j)[q] != SENT) return false;
        }
        return true;
    }
};

struct Shared {
    MovegenArgs a{};
    Mem M{};
    uint32_t* slice = nullptr;
    uint32_t jobw[2][8];
} S;

void set_out(Out& o) {
    S.a = MovegenArgs{};
    S.a.out_mode = OUT_PACKED_SLOT;
    S.a.cap = CAP;
    S.a.out_packed = o.rows.data();
}
}  // namespace

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 3) return 2;
    const long max_pairs = argc > 3 ? atol(argv[3]) : 1L << 30;
    std::vector<Pos> all;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t v[11];
        while (fread(v, 4, 11, f) == 11) {
            Pos p;
            for (int k = 0; k < 8; ++k) p.w[k] = (uint32_t)v[k];
            p.player = v[8];
            p.d0 = v[9];
            p.d1 = v[10];
            all.push_back(p);
        }
        fclose(f);
    }
    std::vector<uint32_t> slice(SLICE_WORDS, 0u);
    S.slice = slice.data();
    Mem& M = S.M;
    M.map = S.slice;
    M.tab = (unsigned long long*)(S.slice + 64);
    M.S = P_S;
    M.F = P_F;
    M.fa = S.slice + 64 + 2 * P_S;
    M.fb = M.fa + P_F;
    M.pa = S.slice + 64;
    M.pb = M.pa + P_PF;
    M.PF = P_PF;

    // shared between the lanes (written by lane 0 between barriers)
    std::vector<int> kept;        // indices into `all`: rule-mode non-doubles
    std::vector<int> count;       // per kept position: the job's count alone (-1: tier 2)
    std::vector<int> two;         // took the two-move branch alone
    std::vector<int> nh1;         // one high-die first move (nH == 1)
    std::vector<int> first16;     // 16 first moves in a pass
    std::vector<std::vector<uint32_t>> rows;   // per kept position: min(count, CAP) x 8
    struct Case { int a, b, pf, expect; const char* what; };   // expect: 1 pair, 0 not pairable, -1 either
    std::vector<Case> cases;
    Out ref, got;
    long long n_pairs = 0, n_expanded = 0, n_not = 0, bad = 0;
    std::barrier<> barrier(64);
    emu::bar = &barrier;

    auto lane_main = [&](int lane) {
        emu::lane = lane;
        emu::tid = lane;
        // ---- every rule-mode non-doubles position alone: the reference rows
        for (int i = 0; i < (int)all.size(); ++i) {
            const Pos& p = all[i];
            if (p.d0 == p.d1) continue;
            const JobIn in = make_job(p.w[0], p.w[1], p.w[2], p.w[3], p.w[4], p.w[5], p.w[6], p.player, p.d0, p.d1);
            if (!nd_by_rule(in.R)) continue;
            if (lane == 0) {
                ref.reset();
                set_out(ref);
            }
            emu::sync();
            uint32_t* fin = nullptr;
            int rule2 = 0;
            const int nf = job_records<false>(in, S.M, fin, &rule2);
            if (nf >= 0) emit_records<false>(S.a, JA, in, fin, nf, 0);
            emu::sync();
            if (lane == 0) {
                const int H = p.d0 > p.d1 ? p.d0 : p.d1, L = p.d0 > p.d1 ? p.d1 : p.d0;
                const uint32_t occ = occ24(in.R.m0, in.R.m1, in.R.m2);
                const int nH = __builtin_popcount(occ & ok_mask(in.R.block, H, in.R.player));
                const int nL = __builtin_popcount(occ & ok_mask(in.R.block, L, in.R.player));
                kept.push_back(i);
                count.push_back(nf);
                two.push_back(rule2);
                nh1.push_back(nH == 1);
                first16.push_back(nH >= 16 || nL >= 16);
                const int n = nf < 0 ? 0 : (nf < CAP ? nf : CAP);
                rows.emplace_back(ref.job(JA), ref.job(JA) + (size_t)n * 8);
                if (!ref.clean_outside(true, false)) {
                    printf("position %d: the single job wrote outside its slots\n", i);
                    ++bad;
                }
            }
            emu::sync();
        }
        // ---- the pairs
        if (lane == 0) {
            const int n = (int)kept.size();
            for (int i = 0; i + 1 < n; ++i) cases.push_back({i, i + 1, P_PF, -1, "consecutive"});
            int big0 = -1, big1 = -1, p0 = -1, p1 = -1, no2 = -1, yes2 = -1, h1 = -1, f16 = -1, eq = -1;
            for (int i = 0; i < n; ++i) {
                if (two[i] && (big0 < 0 || count[i] > count[big0])) { big1 = big0; big0 = i; }
                else if (two[i] && (big1 < 0 || count[i] > count[big1])) big1 = i;
                const Pos& p = all[kept[i]];
                if (two[i] && p.player == 0 && p0 < 0) p0 = i;
                if (two[i] && p.player == 1 && p1 < 0) p1 = i;
                if (!two[i] && count[i] >= 0 && no2 < 0) no2 = i;
                if (two[i] && yes2 < 0) yes2 = i;
                if (two[i] && nh1[i] && h1 < 0) h1 = i;
                if (two[i] && first16[i] && f16 < 0) f16 = i;
            }
            for (int i = 0; i < n && eq < 0; ++i)
                for (int j = i + 1; j < n && j < i + 200; ++j) {
                    const Pos &a = all[kept[i]], &b = all[kept[j]];
                    if (two[i] && two[j] && a.d0 == b.d0 && a.d1 == b.d1 && a.player != b.player) { eq = i; p0 = i; p1 = j; break; }
                }
            if (p0 >= 0 && p1 >= 0) {
                cases.push_back({p0, p1, P_PF, 1, "player 0 with player 1 (equal dice when found)"});
                cases.push_back({p1, p0, P_PF, 1, "player 1 with player 0"});
            }
            if (yes2 >= 0) cases.push_back({yes2, yes2, P_PF, 1, "a job with itself (equal dice, same root)"});
            if (big0 >= 0 && big1 >= 0) {
                cases.push_back({big0, big1, P_PF, 1, "the two largest jobs"});
                cases.push_back({big1, big0, P_PF, 1, "the two largest jobs, swapped"});
                cases.push_back({big0, big1, 80, 0, "the two largest jobs, list of 80 entries"});
            }
            if (h1 >= 0 && yes2 >= 0) {
                cases.push_back({h1, yes2, P_PF, 1, "nH == 1 first"});
                cases.push_back({yes2, h1, P_PF, 1, "nH == 1 second"});
            }
            if (f16 >= 0 && yes2 >= 0) cases.push_back({f16, yes2, P_PF, 1, "16 first moves in a pass"});
            if (no2 >= 0 && yes2 >= 0) {
                cases.push_back({no2, yes2, P_PF, 0, "no two-move play first"});
                cases.push_back({yes2, no2, P_PF, 0, "no two-move play second"});
            }
            printf("edge cases: largest %d + %d records, players %s, nH == 1 %s, 16 first moves %s, no two-move play %s\n",
                   big0 >= 0 ? count[big0] : -1, big1 >= 0 ? count[big1] : -1, p0 >= 0 && p1 >= 0 ? "found" : "none",
                   h1 >= 0 ? "found" : "none", f16 >= 0 ? "found" : "none", no2 >= 0 ? "found" : "none");
            if ((long)cases.size() > max_pairs) {   // keep the edge cases (at the end)
                const size_t drop = cases.size() - (size_t)max_pairs;
                const size_t n_cons = (size_t)(n > 0 ? n - 1 : 0);
                cases.erase(cases.begin(), cases.begin() + (drop < n_cons ? drop : n_cons));
            }
        }
        emu::sync();
        for (size_t c = 0; c < cases.size(); ++c) {
            const Case& cs = cases[c];
            const Pos &pa = all[kept[cs.a]], &pb = all[kept[cs.b]];
            if (lane == 0) {
                got.reset();
                set_out(got);
                S.M.PF = cs.pf;
                const Pos* pq[2] = {&pa, &pb};
                for (int h = 0; h < 2; ++h) {   // the jobs' words, as the fused kernel keeps them (T.job)
                    for (int k = 0; k < 7; ++k) S.jobw[h][k] = pq[h]->w[k];
                    S.jobw[h][7] = (uint32_t)pq[h]->player | (uint32_t)pq[h]->d0 << 8 | (uint32_t)pq[h]->d1 << 16;
                }
            }
            emu::sync();
            int na = -7, nb = -7;
            const bool ok = job_records_pair<false>(S.a, JA, S.jobw[0], JB, S.jobw[1], S.M, na, nb);
            emu::sync();
            if (lane == 0) {
                S.M.PF = P_PF;
                ++n_pairs;
                for (int q = 0; q < 64; ++q)
                    if (S.slice[q]) {
                        printf("case %zu (%s): map[%d] = %u on return\n", c, cs.what, q, S.slice[q]);
                        ++bad;
                        break;
                    }
                const bool both2 = two[cs.a] && two[cs.b];
                if ((cs.expect == 1 && !ok) || (cs.expect == 0 && ok) || (ok && !both2) ||
                    (!ok && both2 && cs.pf == P_PF && count[cs.a] + count[cs.b] + 64 <= P_PF)) {
                    printf("case %zu (%s): pairable %d, expected %d (two-move %d %d, counts %d %d)\n", c, cs.what,
                           (int)ok, cs.expect, two[cs.a], two[cs.b], count[cs.a], count[cs.b]);
                    ++bad;
                }
                if (!ok) {
                    ++n_not;
                    if (!got.clean_outside(false, false)) {
                        printf("case %zu (%s): not pairable, but the outputs were written\n", c, cs.what);
                        ++bad;
                    }
                } else {
                    ++n_expanded;
                    if (na != count[cs.a] || nb != count[cs.b]) {
                        printf("case %zu (%s): counts %d %d, alone %d %d\n", c, cs.what, na, nb, count[cs.a], count[cs.b]);
                        ++bad;
                    } else {
                        const int idx[2] = {cs.a, cs.b}, job[2] = {JA, JB};
                        for (int h = 0; h < 2; ++h) {
                            const std::vector<uint32_t>& want = rows[idx[h]];
                            if (memcmp(got.job(job[h]), want.data(), want.size() * 4)) {
                                printf("case %zu (%s): job %c's boards differ from the job alone\n", c, cs.what, "AB"[h]);
                                ++bad;
                            }
                            for (size_t q = want.size(); q < (size_t)CAP * 8; ++q)
                                if (got.job(job[h])[q] != SENT) {
                                    printf("case %zu (%s): job %c wrote past its count\n", c, cs.what, "AB"[h]);
                                    ++bad;
                                    break;
                                }
                        }
                    }
                    if (!got.clean_outside(true, true)) {
                        printf("case %zu (%s): written outside the two jobs' slots\n", c, cs.what);
                        ++bad;
                    }
                }
            }
            emu::sync();
        }
    };
    std::vector<std::thread> th;
    for (int l = 0; l < 64; ++l) th.emplace_back(lane_main, l);
    for (auto& t : th) t.join();
    if (FILE* f = fopen(argv[2], "wb")) {
        for (size_t i = 0; i < kept.size(); ++i) {
            const int32_t hdr[3] = {kept[i], count[i], (int32_t)(rows[i].size() / 8)};
            fwrite(hdr, 4, 3, f);
            fwrite(rows[i].data(), 4, rows[i].size(), f);
        }
        fclose(f);
    }
    printf("{\"positions\": %zu, \"pairs\": %lld, \"expanded_as_pairs\": %lld, \"not_pairable\": %lld, "
           "\"mismatches\": %lld}\n", kept.size(), n_pairs, n_expanded, n_not, bad);
    return bad ? 1 : 0;
}
