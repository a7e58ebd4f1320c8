// tests/cpuwave/draw_check.cpp -- test infrastructure (host build, one thread).
// The fused 1-ply step's draws made ahead (DrawSlot / draw_fill / SlotRng,
// csrc/bgx_engine.h) against LaneRng, the phased engine's generator, on the
// same inputs: a slot filled as the kernel's draw item fills it (one call per
// counter, k = 0 and 1) and consumed by lane_advance must give the same
// sampling uniform, dice, board words, player, counter and every other lane
// state word, the same board row, record and episode header, and the same
// error flags, on every path of lane_advance:
//   pass; move; move that ends the game (new_game); move and pass at the
//   max_steps truncation (new_game behind a roll); scripted dice, also past
//   the table's end.
// Cases: seeds x lanes {0, 1, 4095, 8191} x lane_base {0, 100000} x counters
// (small ones, both sides of 2^32, the top of the 64-bit range) and, per
// (seed, lane), counters searched so that the starter roll, the re-roll after
// it and the first roll of new_game are doubles (the loops' re-rolls, all past
// the slot). Also: the two packed dice pairs round-trip for all 36 x 36 values.
// Built with -fsanitize=address,undefined (tests/test_cpuwave_draws.py).
// Usage: draw_check -> one JSON summary line, exit 0 iff clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"
// what bgx_engine.h uses beyond the emulation header
#define __constant__
#define __expf(x) std::exp((float)(x))
inline uint32_t __float_as_uint(float f) { uint32_t v; std::memcpy(&v, &f, 4); return v; }

#include "bgx.h"
#include "bgx_engine.h"

using namespace bgx;

namespace {
constexpr int L = 8192, R = 2, HR = 2, MAX_STEPS = 6;
constexpr uint64_t STREAM = 0x5EED0000ull;

// one engine's memory as lane_advance sees it
struct World {
    std::vector<uint32_t> rows, ring, hring;
    unsigned err = 0;
    EngineDev e{};
    World() : rows((size_t)L * 8), ring((size_t)L * R * REC_WORDS), hring((size_t)L * HR * EP_WORDS) {}
    void reset(uint64_t seed, int lane_base, const uint8_t* tab, int tab_len) {
        std::fill(rows.begin(), rows.end(), 0xA5A5A5A5u);
        std::fill(ring.begin(), ring.end(), 0xA5A5A5A5u);
        std::fill(hring.begin(), hring.end(), 0xA5A5A5A5u);
        err = 0;
        e = EngineDev{};
        e.L = L;
        e.lane_base = lane_base;
        e.seed = seed;
        e.max_steps = MAX_STEPS;
        e.max_legal = 500;
        e.rows = rows.data();
        e.ring = ring.data();
        e.R = R;
        e.hring = hring.data();
        e.HR = HR;
        e.err_flags = &err;
        e.dice_tab = tab;
        e.dice_len = tab_len;
    }
};

long long bad = 0;
void fail(const char* what, uint64_t seed, int lane, int base, uint64_t ctr, const char* path) {
    if (bad < 20)
        printf("%s differs: seed %llu lane %d lane_base %d ctr %llu path %s\n", what, (unsigned long long)seed, lane,
               base, (unsigned long long)ctr, path);
    ++bad;
}

// a mid-game board (nobody has borne off) and one where `mover` has all 15 off
void midgame(uint32_t* w) {
    initial_packed(w);
    w[0] = 0x11u;   // P1: 0 and 1 split
}
void finished(uint32_t* w, int mover) {
    initial_packed(w);
    for (int k = 0; k < 3; ++k) w[3 * mover + k] = 0;
    w[6] = 15u << (8 + 4 * mover);
}

bool same_state(const LaneState& a, const LaneState& b) {
    return !memcmp(a.w, b.w, sizeof(a.w)) && a.p == b.p && a.d0 == b.d0 && a.d1 == b.d1 && a.steps == b.steps &&
           a.flags == b.flags && a.epi == b.epi && a.rec == b.rec && a.ep_first == b.ep_first && a.harv == b.harv &&
           a.hepi == b.hepi && a.ctr == b.ctr;
}

enum Path { PASS, MOVE, MOVE_END, MOVE_TRUNC, PASS_TRUNC, N_PATHS };
const char* kPath[N_PATHS] = {"pass", "move", "move ends the game", "move at max_steps", "pass at max_steps"};

World A, B;
long long n_cases = 0, n_beyond = 0, n_newgame = 0;

// one lane step on both generators; returns the draws consumed
uint64_t one_case(uint64_t seed, int lane, int base, uint64_t ctr, Path path, const uint8_t* tab, int tab_len) {
    A.reset(seed, base, tab, tab_len);
    B.reset(seed, base, tab, tab_len);
    LaneState s{};
    midgame(s.w);
    s.p = (int)((ctr ^ (uint64_t)lane) & 1u);
    set_flag(s.w, s.p);
    s.d0 = 3;
    s.d1 = 5;
    s.steps = path == MOVE_TRUNC || path == PASS_TRUNC ? MAX_STEPS - 1 : 2;
    s.epi = 7;
    s.rec = 41;
    s.ep_first = 40;
    s.harv = 40;
    s.hepi = 7;
    s.ctr = ctr;
    uint32_t nb[8];
    if (path == MOVE_END) finished(nb, s.p);
    else midgame(nb);
    nb[1] ^= 0x100u;   // (the candidate is not the board before)
    const bool pass = path == PASS || path == PASS_TRUNC;
    const int action = pass ? -1 : 3, n_full = pass ? 0 : 9;
    const uint32_t gid = (uint32_t)(base + lane);

    // the phased engine's way: LaneRng, the uniform by lane_uniform's expression
    LaneState sa = s;
    LaneRng ra;
    ra.key = lane_key(seed, gid);
    ra.ctr = ctr;
    ra.dt = lane_dice(A.e, lane);
    const float ua = unit_from(philox(ra.key, STREAM, ctr).x);
    lane_advance(A.e, lane, sa, ra, action, nb, 0.25f, 0.5f, n_full, true);

    // the fused kernel's way: the slot as the draw item fills it (thread k of
    // the lane: counter ctr + k), then SlotRng
    LaneState sb = s;
    DrawSlot slot;
    memset(&slot, 0xEE, sizeof(slot));
    draw_fill(slot, seed, gid, ctr, 0);
    draw_fill(slot, seed, gid, ctr, 1);
    SlotRng rb;
    rb.seed = seed;
    rb.gid = gid;
    rb.dt = lane_dice(B.e, lane);
    rb.load(slot, sb.ctr);
    const float ub = rb.uniform01();
    lane_advance(B.e, lane, sb, rb, action, nb, 0.25f, 0.5f, n_full, true);

    const char* pn = kPath[path];
    if (!tab && memcmp(&ua, &ub, 4)) fail("uniform", seed, lane, base, ctr, pn);
    if (sa.d0 != sb.d0 || sa.d1 != sb.d1) fail("dice", seed, lane, base, ctr, pn);
    if (memcmp(sa.w, sb.w, sizeof(sa.w))) fail("board", seed, lane, base, ctr, pn);
    if (sa.p != sb.p) fail("player", seed, lane, base, ctr, pn);
    if (sa.ctr != sb.ctr) fail("counter", seed, lane, base, ctr, pn);
    if (!same_state(sa, sb)) fail("lane state", seed, lane, base, ctr, pn);
    if (A.rows != B.rows) fail("board row", seed, lane, base, ctr, pn);
    if (A.ring != B.ring) fail("record", seed, lane, base, ctr, pn);
    if (A.hring != B.hring) fail("episode header", seed, lane, base, ctr, pn);
    if (A.err != B.err || ra.exhausted != rb.exhausted) fail("error flags", seed, lane, base, ctr, pn);
    if (sa.d0 < 1 || sa.d0 > 6 || sa.d1 < 1 || sa.d1 > 6) fail("dice range", seed, lane, base, ctr, pn);
    const uint64_t used = sa.ctr - ctr;
    // the path did what its name says
    const bool restarted = sa.epi == 8 && sa.steps == 0;
    if (restarted != (path >= MOVE_END)) fail("path taken", seed, lane, base, ctr, pn);
    if (!pass && sa.rec != 42) fail("path taken (record)", seed, lane, base, ctr, pn);
    ++n_cases;
    n_newgame += restarted;
    n_beyond += !tab && used > 2;
    return used;
}

bool doubles_at(uint64_t key, uint64_t c) {
    const u32x4 r = philox(key, STREAM, c);
    return die_from(r.x) == die_from(r.y);
}
}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    // ---- the packed dice pairs: all 36 x 36 values through the slot and back
    long long n_pack = 0;
    for (int q = 0; q < 36 * 36; ++q) {
        const int a0 = q % 6 + 1, b0 = q / 6 % 6 + 1, a1 = q / 36 % 6 + 1, b1 = q / 216 + 1;
        DrawSlot s;
        s.x = 0x12345678u;
        s.d[0] = (uint16_t)dice_pack(a0, b0);
        s.d[1] = (uint16_t)dice_pack(a1, b1);
        SlotRng r;
        r.seed = 1;
        r.gid = 0;
        r.load(s, 0xFFFFFFFFull);   // (k = ctr - base across a 32-bit carry)
        int a, b, c, d;
        r.roll(a, b);
        r.roll(c, d);
        if (a != a0 || b != b0 || c != a1 || d != b1 || r.ctr != 0x100000001ull || r.x != 0x12345678u) {
            if (bad < 20) printf("dice pairs %d-%d %d-%d came back %d-%d %d-%d\n", a0, b0, a1, b1, a, b, c, d);
            ++bad;
        }
        ++n_pack;
    }

    // ---- (seed, lane, counter) triples x paths
    const uint64_t seeds[] = {0ull, 1ull, 17ull, 0x9E3779B97F4A7C15ull, 0xFFFFFFFFFFFFFFFFull, 123456789012345ull,
                              0x100000000ull, 42ull};
    const int lanes[] = {0, 1, 4095, 8191};
    const int bases[] = {0, 100000};
    const uint64_t ctrs[] = {0ull, 1ull, 2ull, 31ull, 32ull, 1000003ull,
                             0xFFFFFFFCull, 0xFFFFFFFDull, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull,
                             0x7FFFFFFFFFFFFFF0ull, 0xFFFFFFFFFFFFFFF0ull};
    long long n_triples = 0, n_forced = 0, n_forced_long = 0;
    for (uint64_t seed : seeds)
        for (int lane : lanes)
            for (int base : bases) {
                for (uint64_t c : ctrs) {
                    ++n_triples;
                    for (int p = 0; p < N_PATHS; ++p) one_case(seed, lane, base, c, (Path)p, nullptr, 0);
                }
                // forced re-rolls. A move that ends the game at counter c draws
                // new_game's starter roll at c + 1 (the slot's second pair), a
                // truncated move at c + 2, a truncated pass at c + 1: counters
                // where the draws at c + 1, c + 2 and c + 3 are all doubles make
                // the starter loop re-roll on every one of these paths, and past
                // the slot; then counters whose first roll (behind a clean
                // starter roll) is doubles
                const uint64_t key = lane_key(seed, (uint32_t)(base + lane));
                int found = 0;
                for (uint64_t c = 0x100000000ull - 40000ull; found < 2 && c < 0x100000000ull + 400000ull; ++c) {
                    if (!(doubles_at(key, c + 1) && doubles_at(key, c + 2) && doubles_at(key, c + 3))) continue;
                    ++found;
                    ++n_triples;
                    for (int p = MOVE_END; p < N_PATHS; ++p) {
                        const uint64_t used = one_case(seed, lane, base, c, (Path)p, nullptr, 0);
                        ++n_forced;
                        n_forced_long += used >= 6;   // three doubles, a starter roll, a first roll at the least
                    }
                }
                if (found < 2) fail("no triple doubles found", seed, lane, base, 0, "search");
                found = 0;
                for (uint64_t c = 5; found < 2 && c < 100000ull; ++c) {
                    if (doubles_at(key, c + 1) || !doubles_at(key, c + 2)) continue;
                    ++found;
                    ++n_triples;
                    const uint64_t used = one_case(seed, lane, base, c, MOVE_END, nullptr, 0);   // first roll re-rolled
                    ++n_forced;
                    if (used < 4) fail("first roll not re-rolled", seed, lane, base, c, "move ends the game");
                }
                if (found < 2) fail("no first-roll doubles found", seed, lane, base, 0, "search");
            }

    // ---- scripted dice: the counter is the table cursor, the slot is unused;
    // cursors inside the table and past its end (BGX_ERRF_DICE_EXHAUSTED)
    long long n_scripted = 0, n_exhausted = 0;
    {
        constexpr int TL = 24;
        std::vector<uint8_t> tab((size_t)L * TL);
        for (size_t q = 0; q < tab.size(); ++q) tab[q] = (uint8_t)(1 + (q * 7 + q / TL) % 6);
        for (int lane : lanes)
            for (uint64_t c : {0ull, 2ull, 10ull, 20ull, 22ull, 24ull, 30ull})
                for (int p = 0; p < N_PATHS; ++p) {
                    one_case(17, lane, 0, c, (Path)p, tab.data(), TL);
                    ++n_scripted;
                    n_exhausted += (A.err & BGX_ERRF_DICE_EXHAUSTED) != 0;
                    if (((A.err ^ B.err) & BGX_ERRF_DICE_EXHAUSTED)) ++bad;
                }
        if (!n_exhausted || n_exhausted == n_scripted) {
            printf("scripted dice: %lld of %lld cases past the table's end\n", n_exhausted, n_scripted);
            ++bad;
        }
    }
    printf("{\"triples\": %lld, \"cases\": %lld, \"new_games\": %lld, \"beyond_slot\": %lld, \"forced_rerolls\": %lld, "
           "\"forced_long\": %lld, \"scripted\": %lld, \"exhausted\": %lld, \"dice_pairs\": %lld, \"mismatches\": %lld}\n",
           n_triples, n_cases, n_newgame, n_beyond, n_forced, n_forced_long, n_scripted, n_exhausted, n_pack, bad);
    return bad ? 1 : 0;
}
