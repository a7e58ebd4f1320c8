// claim_check.cpp — the fused step's claim / publish / draw-wait protocol
// (csrc/bgx_claim.h) on the host, under ThreadSanitizer: 12 std::thread
// "waves" take the items of a step queue (choice pairs, one job item per lane,
// one draw item) the way the kernel's waves do, over the two mask words.
// Per step, at 16 lanes (no pairing) and 32 lanes (pairing on or off): a
// ragged lane range [lo, hi), random classes, random delays in the choice
// items (so the lanes publish in a random order). Checked:
//  - every lane of the range is claimed exactly once, none outside it;
//  - a claimed lane's state (a plain, non-atomic word) carries this step's
//    tag when the claimer reads it: the publish's release reached the claimer
//    (a missing order is also a data race, which ThreadSanitizer reports);
//  - a partner is a pairable lane, taken only by a pairable owner, and only
//    with pairing on; the flags never claim a class the lane does not have;
//  - the items left over by the pairs end as no-ops, as many as pairs formed;
//  - the draw wait returns only after every lane of the range has published
//    (it reads every lane's state);
//  - no poll reaches the bound.
// The GPU's relaxed accesses + acquire fence are acquire accesses here
// (ThreadSanitizer does not model fences); acquire() is empty.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "bgx_claim.h"

namespace {

constexpr int NW = 12;

struct HostOps {
    bool cls_first;   // which word a poll reads first (the GPU's 128-bit read may be either)
    unsigned long long load(const unsigned long long* p) const { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    void load2(const bgx::ClaimWords& W, unsigned long long& so, unsigned long long& cls) const {
        if (cls_first) {
            cls = __atomic_load_n(&W.cls, __ATOMIC_RELAXED);
            so = __atomic_load_n(&W.so, __ATOMIC_ACQUIRE);
        } else {
            so = __atomic_load_n(&W.so, __ATOMIC_ACQUIRE);
            cls = __atomic_load_n(&W.cls, __ATOMIC_RELAXED);
        }
    }
    unsigned long long fetch_and(unsigned long long* p, unsigned long long m) const {
        return __atomic_fetch_and(p, m, __ATOMIC_ACQUIRE);
    }
    void or_relaxed(unsigned long long* p, unsigned long long m) const { __atomic_fetch_or(p, m, __ATOMIC_RELAXED); }
    void or_release(unsigned long long* p, unsigned long long m) const { __atomic_fetch_or(p, m, __ATOMIC_RELEASE); }
    void acquire() const {}
    void relax() const { std::this_thread::yield(); }
};

struct Barrier {
    std::atomic<int> n{0};
    std::atomic<unsigned> gen{0};
    void wait() {
        const unsigned g = gen.load(std::memory_order_acquire);
        if (n.fetch_add(1, std::memory_order_acq_rel) == NW - 1) {
            n.store(0, std::memory_order_relaxed);
            gen.store(g + 1, std::memory_order_release);
        } else {
            while (gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
        }
    }
};

struct Step {   // written by wave 0 between two barriers, read-only inside the queue
    int lo = 0, hi = 0;
    bool pair_on = false;
    unsigned tag = 0;
    bool dbl[32] = {}, rule[32] = {};
    int delay[16] = {};   // yields in front of choice item p
};

struct Shared {
    bgx::ClaimWords W{0, 0};
    std::atomic<int> qn{0};
    unsigned st[32] = {};               // the lanes' "state": plain words, tagged by their choice
    std::atomic<int> claimed[32];       // claims of lane v this step
    std::atomic<int> pairs{0}, noops{0}, draws{0};
    std::atomic<int> errors{0};
    long total_pairs = 0;               // wave 0's
    Step s;
    Barrier bar;
};

#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (S.errors.fetch_add(1) < 20) {          \
                fprintf(stderr, "claim_check: ");      \
                fprintf(stderr, __VA_ARGS__);          \
                fprintf(stderr, "\n");                 \
            }                                          \
        }                                              \
    } while (0)

template <int FL> void wave(Shared& S, int w, int n_steps, unsigned seed) {
    constexpr bool PAIR = FL == 32;
    std::mt19937 rng(seed);
    const HostOps ops{(w & 1) != 0};
    for (int step = 0; step < n_steps; ++step) {
        if (w == 0) {
            Step& s = S.s;
            s.lo = (int)(rng() % FL);
            s.hi = s.lo + 1 + (int)(rng() % (FL - s.lo));
            if (rng() % 4 == 0) { s.lo = 0; s.hi = FL; }
            s.pair_on = PAIR && rng() % 4 != 0;
            s.tag = 0x51000000u + (unsigned)step;
            for (int v = 0; v < FL; ++v) {
                s.dbl[v] = rng() % 6 == 0;
                s.rule[v] = !s.dbl[v] && rng() % 5 != 0;
                S.claimed[v].store(0, std::memory_order_relaxed);
            }
            for (int p = 0; p < 16; ++p) s.delay[p] = (int)(rng() % 40);
            S.pairs = 0;
            S.noops = 0;
            S.draws = 0;
            S.qn.store(NW, std::memory_order_relaxed);
            __atomic_store_n(&S.W.so, 0ull, __ATOMIC_RELAXED);
            __atomic_store_n(&S.W.cls, 0ull, __ATOMIC_RELAXED);
        }
        S.bar.wait();   // the queue's opening barrier
        const Step& s = S.s;
        const int np = (s.hi - s.lo + 1) >> 1, nj = s.hi - s.lo;
        const uint32_t range = bgx::claim_range(s.lo, s.hi);
        for (int it = w; it < np + nj + 1; it = S.qn.fetch_add(1, std::memory_order_relaxed)) {
            if (it < np) {   // a choice item: two lanes
                for (int k = 0; k < s.delay[it]; ++k) std::this_thread::yield();
                for (int h = 0; h < 2; ++h) {
                    const int v = s.lo + 2 * it + h;
                    if (v >= s.hi) continue;
                    S.st[v] = s.tag ^ (unsigned)v;
                    bgx::claim_publish_class(ops, S.W, v, s.dbl[v], PAIR && s.rule[v]);
                    bgx::claim_publish_open(ops, S.W, v);
                }
            } else if (it < np + nj) {   // a job item
                const bgx::Claim c = bgx::claim_take<PAIR>(ops, S.W, range, s.pair_on, true);
                CHECK(!(c.flags & bgx::CLAIM_BOUND), "step %d: a claim reached the poll bound", step);
                if (c.v < 0) {
                    CHECK(c.v2 < 0 && !(c.flags & (bgx::CLAIM_RULE | bgx::CLAIM_PARTNER)), "step %d: flags on a no-op", step);
                    S.noops.fetch_add(1);
                    continue;
                }
                CHECK(c.v >= s.lo && c.v < s.hi, "step %d: claimed lane %d outside [%d, %d)", step, c.v, s.lo, s.hi);
                CHECK(S.st[c.v] == (s.tag ^ (unsigned)c.v), "step %d: lane %d claimed before its state", step, c.v);
                S.claimed[c.v].fetch_add(1);
                if (c.flags & bgx::CLAIM_RULE) CHECK(PAIR && s.rule[c.v], "step %d: lane %d is not pairable", step, c.v);
                if (c.flags & bgx::CLAIM_PARTNER) CHECK(c.flags & bgx::CLAIM_RULE, "step %d: partner flag without an owner", step);
                if (c.v2 >= 0) {
                    CHECK(PAIR && s.pair_on, "step %d: a pair with pairing off", step);
                    CHECK((c.flags & bgx::CLAIM_RULE) && (c.flags & bgx::CLAIM_PARTNER), "step %d: a pair without its flags", step);
                    CHECK(c.v2 != c.v && c.v2 >= s.lo && c.v2 < s.hi, "step %d: partner %d of %d", step, c.v2, c.v);
                    CHECK(s.rule[c.v] && s.rule[c.v2], "step %d: pair (%d, %d) is not two pairable lanes", step, c.v, c.v2);
                    CHECK(S.st[c.v2] == (s.tag ^ (unsigned)c.v2), "step %d: partner %d taken before its state", step, c.v2);
                    S.claimed[c.v2].fetch_add(1);
                    S.pairs.fetch_add(1);
                }
            } else {   // the draw item
                CHECK(bgx::claim_wait_stepped(ops, S.W, range), "step %d: the draw wait reached the poll bound", step);
                for (int v = s.lo; v < s.hi; ++v)
                    CHECK(S.st[v] == (s.tag ^ (unsigned)v), "step %d: draw wait over before lane %d published", step, v);
                S.draws.fetch_add(1);
            }
        }
        S.bar.wait();   // the step's end barrier
        if (w == 0) {
            for (int v = 0; v < FL; ++v) {
                const int want = v >= s.lo && v < s.hi ? 1 : 0;
                CHECK(S.claimed[v].load() == want, "step %d: lane %d claimed %d times (want %d)", step, v, S.claimed[v].load(), want);
            }
            CHECK(S.noops.load() == S.pairs.load(), "step %d: %d no-op items for %d pairs", step, S.noops.load(), S.pairs.load());
            CHECK(S.draws.load() == 1, "step %d: %d draw items", step, S.draws.load());
            S.total_pairs += S.pairs.load();
            const unsigned long long so = __atomic_load_n(&S.W.so, __ATOMIC_RELAXED);
            CHECK((uint32_t)so == 0u && (uint32_t)(so >> 32) == range, "step %d: masks at the end %llx", step, so);
        }
        // (the other waves wait in the next opening barrier while wave 0 checks and sets up)
    }
}

template <int FL> long run(int n_steps, unsigned seed, long& pairs_total) {
    Shared S;
    for (auto& c : S.claimed) c.store(0);
    std::vector<std::thread> th;
    for (int w = 0; w < NW; ++w) th.emplace_back([&, w] { wave<FL>(S, w, n_steps, seed + 977u * (unsigned)w); });
    for (auto& t : th) t.join();
    pairs_total = S.total_pairs;
    return S.errors.load();
}

}  // namespace

int main(int argc, char** argv) {
    const int n_steps = argc > 1 ? atoi(argv[1]) : 1500;
    long p16 = 0, p32 = 0;
    const long e16 = run<16>(n_steps, 12345u, p16);
    const long e32 = run<32>(n_steps, 54321u, p32);
    printf("claim_check: %d steps each; errors at 16 lanes %ld, at 32 lanes %ld; pairs %ld, %ld\n", n_steps, e16, e32,
           p16, p32);
    // (the 32-lane run must have paired, or its pair checks checked nothing)
    return e16 || e32 || p16 != 0 || p32 <= 0 ? 1 : 0;
}
