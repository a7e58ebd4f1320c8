// bgx_claim.h — how the fused step's pipelined queue hands a stepped lane's
// next tier-1 job to a wave (bgx_fused.hip): two 64-bit mask words per
// workgroup and step, bit v = lane v (at most 32 lanes).
//   so  : bits 0..31  open     lane v is stepped and its next job is unclaimed
//         bits 32..63 stepped  lane v's choice is done this step
//   cls : bits 0..31  dbl      lane v's next roll is a double (the long jobs)
//         bits 32..63 rule     lane v's next job is pairable (non-doubles in
//                              rule mode, nd_by_rule)
// Both are zero at the step's opening barrier and bits are only set after it,
// except that a claim clears the lane's open bit.
// Publish (the choice item, one thread per lane): the lane's state first, then
// its class bits with one relaxed OR on cls, then open and stepped together
// with one release OR on so. So the ORs are ordered by release on the so OR
// and acquire on the reader (not by packing open and dbl into one word): a
// reader that sees bit v in so and then acquires sees the lane's state, and a
// read of cls made after that sees v's class bits.
// The class bits are hints. dbl only orders the candidates and rule only lets
// a wave take two lanes, and either way every job is expanded from the lane's
// own state, so a reader that misses a class bit (its poll reads the two words
// in one 128-bit access that need not be one atomic access) loses nothing but
// the hint. A bit it does see was set by the publisher, after the state.
// Every decision is taken on a 64-bit atomic access of so: a claim is the
// fetch-and that clears the open bit and is won iff the returned word had it;
// "every lane claimed" is stepped covering the range and open == 0 in one
// atomic load.
// The operations come from A (wave-uniform on the GPU: one lane acts and the
// result is broadcast; std::thread "waves" on the host, tests/cpuwave):
//   load2(W, so, cls)   one poll of both words (hint quality, see above)
//   load(p)             64-bit atomic load
//   fetch_and(p, m)     64-bit atomic AND, returns the old word
//   or_relaxed(p, m), or_release(p, m)   the publisher's ORs (its own thread)
//   acquire()           acquire fence behind the loads / fetch-ands
//   relax()             between two polls
#pragma once

#include <cstdint>

#ifndef BGX_CLAIM_FN
#define BGX_CLAIM_FN inline
#endif

namespace bgx {

struct alignas(16) ClaimWords {
    unsigned long long so;    // open | stepped << 32
    unsigned long long cls;   // dbl | rule << 32
};

constexpr unsigned CLAIM_POLL_BOUND = 1u << 24;   // polls before a wait gives up
constexpr unsigned CLAIM_BOUND = 1u;     // the poll bound was reached: nothing claimed
constexpr unsigned CLAIM_RULE = 2u;      // the claimed lane is pairable
constexpr unsigned CLAIM_PARTNER = 4u;   // ... and a second pairable lane was open at that moment

struct Claim {
    int v, v2;        // the claimed lane (-1: every lane was claimed, or the bound), the lane paired with it (-1: none)
    unsigned flags;   // CLAIM_*
};

// bits [lo, hi) of a step's lanes, 0 <= lo < hi <= 32
BGX_CLAIM_FN uint32_t claim_range(int lo, int hi) {
    return (hi >= 32 ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
}
BGX_CLAIM_FN int claim_bit_index(uint32_t bit) { return __builtin_ctz(bit); }

// lane v's choice is done, in two calls by the thread that wrote the lane's
// state: its class bits (beside the state, before the release), then open and
// stepped together (the release)
template <class A> BGX_CLAIM_FN void claim_publish_class(A& a, ClaimWords& W, int v, bool dbl, bool rule) {
    const unsigned long long bit = 1ull << v;
    const unsigned long long c = (dbl ? bit : 0ull) | (rule ? bit << 32 : 0ull);
    if (c) a.or_relaxed(&W.cls, c);
}
template <class A> BGX_CLAIM_FN void claim_publish_open(A& a, ClaimWords& W, int v) {
    const unsigned long long bit = 1ull << v;
    a.or_release(&W.so, bit | (bit << 32));
}

// One job item's claim: the lowest open doubles lane, else the lowest open
// lane; a lost race retries at once from the word the fetch-and returned; with
// nothing open it polls (relax between polls) until a lane opens, or every
// lane of `range` is stepped and claimed (v = -1: an item left over by the
// pairs), or the bound. PAIR: a pairable lane takes one more open pairable
// lane, from the word its own claim returned, in at most two fetch-ands and
// never waiting (pair_on; `survey` alone only fills the flags).
template <bool PAIR, class A>
BGX_CLAIM_FN Claim claim_take(A& a, ClaimWords& W, uint32_t range, bool pair_on, bool survey) {
    Claim r{-1, -1, 0u};
    for (unsigned spin = 0;; ++spin) {
        unsigned long long so, cls;
        a.load2(W, so, cls);
        uint32_t open = (uint32_t)so;
        while (open) {
            const uint32_t md = open & (uint32_t)cls, pick = md ? md : open;
            const uint32_t bit = pick & (0u - pick);
            const unsigned long long old = a.fetch_and(&W.so, ~(unsigned long long)bit);
            so = old & ~(unsigned long long)bit;
            if (old & bit) {
                r.v = claim_bit_index(bit);
                break;
            }
            open = (uint32_t)so;
        }
        if (r.v >= 0) {
            if (PAIR && (pair_on || survey)) {
                const uint32_t rule = (uint32_t)(cls >> 32), bit = 1u << r.v;
                if (rule & bit) {
                    r.flags |= CLAIM_RULE;
                    uint32_t mf = (uint32_t)so & rule & ~bit;
                    if (mf) r.flags |= CLAIM_PARTNER;
                    for (int att = 0; att < 2 && mf && pair_on; ++att) {
                        const uint32_t b2 = mf & (0u - mf);
                        const unsigned long long old = a.fetch_and(&W.so, ~(unsigned long long)b2);
                        if (old & b2) {
                            r.v2 = claim_bit_index(b2);
                            break;
                        }
                        mf = (uint32_t)old & rule & ~bit & ~b2;
                    }
                }
            }
            a.acquire();
            return r;
        }
        if ((uint32_t)(so >> 32) == range) {
            // nothing open and every lane stepped in what was read: decided on one atomic load
            const unsigned long long chk = a.load(&W.so);
            if ((uint32_t)(chk >> 32) == range && (uint32_t)chk == 0u) return r;
            if ((uint32_t)chk) continue;
        }
        if (spin >= CLAIM_POLL_BOUND) {
            r.flags |= CLAIM_BOUND;
            return r;
        }
        a.relax();
    }
}

// the draw item's wait: until every lane of `range` is stepped (false: the bound)
template <class A> BGX_CLAIM_FN bool claim_wait_stepped(A& a, const ClaimWords& W, uint32_t range) {
    bool ok = true;
    for (unsigned spin = 0; ((uint32_t)(a.load(&W.so) >> 32) & range) != range; ++spin) {
        if (spin >= CLAIM_POLL_BOUND) {
            ok = false;
            break;
        }
        a.relax();
    }
    a.acquire();
    return ok;
}

}  // namespace bgx
