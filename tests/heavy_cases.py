"""The heaviest legal positions move generation is tested at: domain-legal
boards (bgx_domain.h) whose play lists approach or outgrow the capacity of
each movegen tier (bgx_movegen.h: tier 1 a 4 KB LDS slice, 224-entry frontiers
or two 480-entry lists; tier 2 the 16-wave block kernel, 2,016-entry frontiers,
2,048 parents per level; tier 3 the 16,384-slot global workspace). A plain
module (imported by test_heavy_cases.py, test_oracle_golden.py,
test_cpuwave.py and test_gpu_movegen_heavy.py), not a conftest.

The positions are literals (_LITERALS, read through cases()). They were found with the CPU oracle by
`find()`, a seeded hill-climb kept here so that the list can be regenerated:

    python tests/heavy_cases.py          # prints the _LITERALS entries

A climb moves one mover checker to another point the opponent does not hold
and keeps the move if the class's score does not fall. The tests never run
the search.

Board layout (include/bgx.h): player 0's points 0..23 | player 1's 24..47 |
bar 48, 49 | borne off 50, 51. Player 0 moves towards point 23 (home 18..23),
player 1 towards point 0 (home 0..5).
"""
import os
import sys

import numpy as np

ROLLS36 = [(a, b) for a in range(1, 7) for b in range(1, 7)]
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]   # DICE_ROLLS order (two_ply.py:10-32)

# capacities the classes are defined against (bgx_movegen.h)
T1_LIST = 480        # tier 1: two 480-entry lists
T2_FRONTIER = 2016   # tier 2: S_T2 - 32
T2_PARENTS = 2048    # tier 2: K_F
FUSED_ND = 160       # the fused step's tier-1 frontier entries
RECORD_CLAMP = 4095  # the record's n_moves field

_SPREAD = [1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0]


def _board(p0, p1, bar=(0, 0), off=(0, 0)):
    b = np.zeros(52, np.uint8)
    b[0:24] = p0
    b[24:48] = p1
    b[48:50] = bar
    b[50:52] = off
    return b


def _sparse(pairs):
    v = [0] * 24
    for i, k in pairs:
        v[i] = k
    return v


def mirror(board, player):
    """The same position seen from the other side: point i becomes 23 - i and
    the two position arrays, bars and borne-off counts swap."""
    b = np.asarray(board, np.uint8)
    m = np.zeros(52, np.uint8)
    m[0:24] = b[24:48][::-1]
    m[24:48] = b[0:24][::-1]
    m[48], m[49] = b[49], b[48]
    m[50], m[51] = b[51], b[50]
    return m, 1 - int(player)


# name -> (player 0's points, player 1's points, bars, borne off, player).
# Written by find(); "spread_p0" is the hand-given start of every climb.
_LITERALS = {
    "spread_p0": (_SPREAD, _sparse([(23, 15)]), (0, 0), (0, 0), 0),
    "edge_t2": (_sparse([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (10, 1), (12, 1), (14, 1),
                         (16, 1), (17, 1), (19, 1), (21, 1)]), _sparse([(23, 15)]), (0, 0), (0, 0), 0),
    "tier2_mid": (_sparse([(0, 1), (2, 1), (4, 1), (6, 1), (8, 1), (9, 1), (11, 1), (13, 1), (14, 1), (15, 1),
                           (16, 1), (17, 1), (18, 1), (19, 1), (20, 1)]),
                  _sparse([(5, 5), (7, 3), (12, 5), (23, 2)]), (0, 0), (0, 0), 0),
    "tier2_low": (_sparse([(0, 1), (1, 1), (4, 2), (9, 1), (11, 1), (13, 1), (15, 1), (16, 3), (18, 3), (19, 1)]),
                  _sparse([(5, 5), (7, 3), (12, 5), (23, 2)]), (0, 0), (0, 0), 0),
    "blocked_t2": (_sparse([(0, 1), (1, 1), (2, 1), (4, 1), (5, 1), (6, 1), (8, 1), (9, 1), (11, 1), (12, 1),
                            (13, 1), (15, 1), (16, 1), (17, 1), (18, 1)]),
                   _sparse([(21, 3), (22, 3), (23, 9)]), (0, 0), (0, 0), 0),
    "nd_max": (_sparse([(0, 1), (1, 1), (2, 1), (4, 1), (5, 1), (7, 1), (8, 1), (10, 1), (11, 1), (13, 1), (14, 1),
                        (16, 1), (17, 1), (19, 1), (20, 1)]),
               _sparse([(6, 1), (9, 1), (12, 1), (15, 1), (18, 1), (21, 1), (23, 9)]), (0, 0), (0, 0), 0),
    "blots_over_t2": (_sparse([(0, 1), (1, 1), (3, 1), (4, 1), (5, 1), (7, 1), (8, 1), (10, 1), (11, 1), (13, 1),
                               (14, 1), (16, 1), (17, 1), (19, 1), (20, 1)]),
                      _sparse([(6, 1), (9, 1), (12, 1), (15, 1), (18, 1), (21, 1), (23, 9)]), (0, 0), (0, 0), 0),
    "hits_t2": (_sparse([(0, 2), (2, 1), (4, 1), (5, 1), (7, 1), (8, 1), (10, 1), (11, 2), (14, 2), (17, 1),
                         (18, 1), (19, 1)]),
                _sparse([(6, 1), (9, 1), (12, 1), (15, 1), (21, 3), (22, 3), (23, 5)]), (0, 0), (0, 0), 0),
    "bearoff": (_sparse([(18, 2), (19, 2), (20, 2), (21, 1), (22, 2), (23, 2)]), _sparse([(0, 15)]),
                (0, 0), (4, 0), 0),
    "bar": (_sparse([(1, 1), (3, 1), (5, 1), (6, 1), (8, 1), (10, 1), (11, 1), (12, 1), (14, 1), (15, 1), (16, 1),
                     (18, 1), (19, 1), (20, 1)]), _sparse([(23, 15)]), (1, 0), (0, 0), 0),
}

# name -> class (what test_heavy_cases.py asserts of the oracle's counts):
#   over_t2    largest doubles list >= 2,049: outgrows tier 2, ends in tier 3
#   edge_t2    largest doubles list in (2016, 2048]: between tier 2's two limits
#   tier2      largest doubles list in (480, 2016]: ends in tier 2
#   nd_max     the largest non-doubles list the search reached, > 160 (the
#              fused step's frontier entries)
#   bearoff    every mover checker in the home board, >= 3 borne off
#   bar        a mover checker on the bar, largest list >= 200
# "blots_over_t2" is the over_t2 member that differs structurally from the
# spread board (six opponent blots in the mover's path); it and "hits_t2" are
# the members with >= 4 opponent blots ahead of the mover (HITS), so that
# plays differ by what they hit.
CLASSES = {
    "spread_p0": "over_t2", "spread_p1": "over_t2", "blots_over_t2": "over_t2",
    "edge_t2": "edge_t2", "tier2_mid": "tier2", "tier2_low": "tier2", "blocked_t2": "tier2",
    "hits_t2": "tier2", "nd_max": "nd_max", "bearoff": "bearoff", "bar": "bar",
}
HITS = ("blots_over_t2", "hits_t2")


def cases():
    """[(name, board uint8[52], player)], fixed order."""
    out = []
    for name in CLASSES:
        if name == "spread_p1":
            b, pl = mirror(*cases_by_name("spread_p0"))
        else:
            p0, p1, bar, off, pl = _LITERALS[name]
            b = _board(p0, p1, bar, off)
        out.append((name, b, pl))
    return out


def cases_by_name(name):
    p0, p1, bar, off, pl = _LITERALS[name]
    return _board(p0, p1, bar, off), pl


# the six members the slower host emulation runs: one per class that takes its
# own path (over tier 2, the tier-2 edge, tier 2 with hits, the largest
# non-doubles, bear-off, bar entry)
EMU_SUBSET = ("spread_p1", "edge_t2", "hits_t2", "nd_max", "bearoff", "bar")


def counts(orc, board, player):
    """{(d0, d1): oracle count} over the 36 rolls."""
    return {(a, c): orc.movegen(board, player, a, c, cap=1)[0] for a, c in ROLLS36}


def summary(orc, board, player):
    c = counts(orc, board, player)
    dbl = max(c[(d, d)] for d in range(1, 7))
    nd = max(v for (a, k), v in c.items() if a != k)
    total21 = sum(c[r] for r in ROLLS21)
    return {"dbl": dbl, "nd": nd, "total21": total21}


def blots_ahead(board, player):
    """Opponent blots on points a mover checker has still to pass."""
    b = np.asarray(board, np.uint8)
    me, op = b[24 * player:24 * player + 24], b[24 * (1 - player):24 * (1 - player) + 24]
    if player == 0:
        back = 0 if b[48] else int(np.flatnonzero(me)[0])
        return int(sum(1 for i in range(back + 1, 24) if op[i] == 1))
    back = 23 if b[49] else int(np.flatnonzero(me)[-1])
    return int(sum(1 for i in range(0, back) if op[i] == 1))


# ------------------------------------------------------------------ the finder
def _climb(orc, rng, board, score, steps, movable=range(24), allowed=range(24), done=None):
    """Player 0 to move. One mover checker from a point of `movable` to a point
    of `allowed` the opponent does not hold; kept if score(board) does not
    fall. Stops early when done(score)."""
    b = board.copy()
    best = score(b)
    for _ in range(steps):
        if done is not None and done(best):
            break
        src = [i for i in movable if b[i]]
        i = int(rng.choice(src))
        dst = [j for j in allowed if j != i and b[24 + j] == 0]
        j = int(rng.choice(dst))
        b[i] -= 1
        b[j] += 1
        s = score(b)
        if s >= best:
            best = s
        else:
            b[i] += 1
            b[j] -= 1
    return b, best


def find(orc, log=print):
    """Regenerate _LITERALS (seeded: the same list every run)."""
    def dbl(b):
        return max(orc.movegen(b, 0, d, d, cap=1)[0] for d in range(1, 7))

    def nd(b):
        return max(orc.movegen(b, 0, a, c, cap=1)[0] for a in range(1, 7) for c in range(a + 1, 7))

    def anyroll(b):
        return max(dbl(b), nd(b))

    found = {}
    spread = _board(_SPREAD, _sparse([(23, 15)]))
    found["spread_p0"] = spread

    # the tier-2 edge: as close to the middle of (2016, 2048] as the climb gets
    rng = np.random.default_rng(2016)
    b, s = _climb(orc, rng, spread, lambda x: -abs(dbl(x) - 2032), 3000, done=lambda v: v >= -15)
    found["edge_t2"] = b
    log(f"edge_t2: largest doubles list {dbl(b)}")

    # tier 2, mid and low: towards 1,500 and 600 from the opening position's shape
    start = _board(_sparse([(0, 2), (11, 5), (16, 3), (18, 5)]), _sparse([(23, 2), (12, 5), (7, 3), (5, 5)]))
    for name, target, seed in (("tier2_mid", 1500, 1500), ("tier2_low", 600, 600)):
        rng = np.random.default_rng(seed)
        b, s = _climb(orc, rng, start, lambda x: -abs(dbl(x) - target), 1500, done=lambda v: v >= -60)
        found[name] = b
        log(f"{name}: largest doubles list {dbl(b)}")

    # blocked: the opponent holds two made points in the mover's home board
    # (the climb's best, below tier 2's frontier: blocked points cost plays)
    rng = np.random.default_rng(2049)
    start = _board(_sparse([(0, 3), (1, 3), (2, 3), (3, 3), (4, 3)]), _sparse([(21, 3), (22, 3), (23, 9)]))
    b, s = _climb(orc, rng, start, dbl, 2500, done=lambda v: v >= 2100)
    found["blocked_t2"] = b
    log(f"blocked_t2: largest doubles list {dbl(b)}")

    # over tier 2 with another structure than the spread board: six opponent
    # blots spread over the mover's path, so plays differ by what they hit
    rng = np.random.default_rng(4)
    start = _board(_sparse([(0, 3), (1, 3), (2, 3), (4, 3), (5, 3)]),
                   _sparse([(6, 1), (9, 1), (12, 1), (15, 1), (18, 1), (21, 1), (23, 9)]))
    b, s = _climb(orc, rng, start, lambda x: dbl(x) if blots_ahead(x, 0) >= 4 else -1, 3000)
    found["blots_over_t2"] = b
    log(f"blots_over_t2: largest doubles list {dbl(b)}, {blots_ahead(b, 0)} blots ahead")

    # the largest non-doubles list: from the six-blot board, whose hit plays
    # add distinct results (220; the same climb from the spread board stays at 209)
    rng = np.random.default_rng(209)
    b, s = _climb(orc, rng, found["blots_over_t2"], nd, 3000)
    found["nd_max"] = b
    log(f"nd_max: largest non-doubles list {nd(b)}")

    # hits inside tier 2: four blots and two made points, towards 1,200 plays
    rng = np.random.default_rng(5)
    start = _board(_sparse([(0, 3), (1, 3), (2, 3), (3, 3), (4, 3)]),
                   _sparse([(6, 1), (9, 1), (12, 1), (15, 1), (21, 3), (22, 3), (23, 5)]))
    b, s = _climb(orc, rng, start, lambda x: -abs(dbl(x) - 1200) if blots_ahead(x, 0) >= 4 else -9999, 2000,
                  done=lambda v: v >= -100)
    found["hits_t2"] = b
    log(f"hits_t2: largest doubles list {dbl(b)}, {blots_ahead(b, 0)} blots ahead")

    # bear-off: 11 checkers in the home board, 4 borne off
    rng = np.random.default_rng(18)
    start = _board(_sparse([(18, 6), (19, 5)]), _sparse([(0, 15)]), off=(4, 0))
    b, s = _climb(orc, rng, start, anyroll, 1500, movable=range(18, 24), allowed=range(18, 24))
    found["bearoff"] = b
    log(f"bearoff: largest list {anyroll(b)}")

    # bar: one mover checker on the bar, the rest climbing
    rng = np.random.default_rng(48)
    start = _board(_SPREAD[:20] + [0, 0, 0, 0], _sparse([(23, 15)]), bar=(1, 0))
    b, s = _climb(orc, rng, start, anyroll, 3000)
    found["bar"] = b
    log(f"bar: largest list {anyroll(b)}")
    return found


def _literal(b, player=0):
    def sp(v):
        return "_sparse([" + ", ".join(f"({i}, {int(k)})" for i, k in enumerate(v) if k) + "])"
    return (f"({sp(b[0:24])}, {sp(b[24:48])}, ({int(b[48])}, {int(b[49])}), "
            f"({int(b[50])}, {int(b[51])}), {player})")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle as _orc
    for _name, _b in find(_orc).items():
        print(f'    "{_name}": {_literal(_b)},')
