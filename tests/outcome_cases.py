"""Constructed positions for the env step's outcome rules (judge(),
bgx_engine.h: reward, done, win type, the close-out and prime shaping rewards).
A plain module (imported by tools/gen_golden.py, test_oracle_golden.py,
test_cpuwave_judge.py, test_outcome_cases.py and test_gpu_outcomes.py), not a
conftest.

Three tables:

  fixture_cases()   after-move boards by plain enumeration, one list per rule
                    and boundary; tools/gen_golden.py --only outcomes labels
                    them with the reference's predicates (outcomes.npz)
  positions()       start positions with a fixed roll, one move before a cell:
                    every legal afterstate falls in the cell (pure), so the
                    first record of an episode is known before the run
  sequences()       scripted lines (fixed first roll, then scripted dice), pure
                    at every step: the once-per-player rule over a game

The start positions are literals. They were found with the CPU oracle by
`find()`, a seeded random search over a template per cell, kept here so that
the list can be regenerated:

    python tests/outcome_cases.py          # prints the _LITERALS entries

The tests never run the search.

Board layout (include/bgx.h): player 0's points 0..23 | player 1's 24..47 |
bar 48, 49 | borne off 50, 51. Player 0 moves towards point 23 (home 18..23),
player 1 towards point 0 (home 0..5). Everything below is built in the mover's
view (the mover runs towards 23) and mirrored for player 1, so "behind a run"
is always "on a higher point".
"""
import os
import sys

import numpy as np

KEYS = ("game_over", "gammon", "backgammon", "prime", "closed_out")
FNS = {"game_over": "check_game_over", "gammon": "check_for_gammon", "backgammon": "check_for_backgammon",
       "prime": "made_at_least_five_prime", "closed_out": "is_closed_out"}


def mirror(board):
    """The same position seen from the other side: point i becomes 23 - i and
    the two position arrays, bars and borne-off counts swap."""
    b = np.asarray(board, np.uint8)
    m = np.zeros(52, np.uint8)
    m[0:24] = b[24:48][::-1]
    m[24:48] = b[0:24][::-1]
    m[48], m[49] = b[49], b[48]
    m[50], m[51] = b[51], b[50]
    return m


def make(mine, theirs, bar_o=0, off_m=None, off_o=None, bar_m=0, mover=0):
    """A board from the mover's view: mine / theirs {point: count}; borne-off
    counts default to whatever completes 15 a side."""
    b = np.zeros(52, np.uint8)
    for i, k in mine.items():
        b[i] = k
    for i, k in theirs.items():
        assert b[i] == 0 or k == 0, (mine, theirs)
        b[24 + i] = k
    b[48], b[49] = bar_m, bar_o
    b[50] = 15 - int(b[0:24].sum()) - bar_m if off_m is None else off_m
    b[51] = 15 - int(b[24:48].sum()) - bar_o if off_o is None else off_o
    return mirror(b) if mover else b


def view(board, pl):
    """(mine[24], theirs[24], bar_m, bar_o, off_m, off_o) in the mover's view."""
    b = np.asarray(board, np.uint8)
    if pl:
        b = mirror(b)
    return b[0:24].astype(int), b[24:48].astype(int), int(b[48]), int(b[49]), int(b[50]), int(b[51])


def features(board, pl):
    """What the rules look at, read off the board alone (mover's view): the
    longest run of made points (the first of equals) and where the opponent
    sits relative to it, the home board, bar and borne-off counts."""
    mine, theirs, bar_m, bar_o, off_m, off_o = view(board, pl)
    made = mine >= 2
    best, i = (0, 0), 0
    while i < 24:
        if made[i]:
            j = i
            while j < 24 and made[j]:
                j += 1
            if j - i > best[1]:
                best = (i, j - i)
            i = j
        else:
            i += 1
    s, n = best
    e = s + n - 1
    return dict(mine=mine, theirs=theirs, bar_m=bar_m, bar_o=bar_o, off_m=off_m, off_o=off_o,
                run_start=s, run_len=n, run_end=e, n_made=int(made.sum()),
                first_behind=bool(n and e < 23 and theirs[e + 1] > 0),
                far_behind=bool(n and theirs[e + 2:].sum() > 0),
                ahead=bool(theirs[:s].sum() > 0), n_theirs=int(theirs.sum()),
                home_made=int(made[18:].sum()), max_stack=int(mine.max()))


# ---------------------------------------------------------------- fixture boards
def _run(s, n, k=2):
    return {i: k for i in range(s, s + n)}


def _prime_cases():
    out = []
    for n in (5, 6, 7):
        for s in range(0, 25 - n):
            run, e = _run(s, n), s + n - 1
            free = [i for i in range(24) if not s <= i <= e]
            tag = f"run{n}" + ("_edge" if e == 23 else "")
            if e < 23:
                out.append((tag + "/first_behind", make(run, {e + 1: 1})))
                if e + 1 < 23:
                    out.append((tag + "/farthest_behind", make(run, {23: 1})))
            if s > 0:
                out.append((tag + "/ahead_only", make(run, {s - 1: 1})))
                if s > 1:
                    out.append((tag + "/ahead_only", make(run, {0: 1})))
            out.append((tag + "/bar_only", make(run, {}, bar_o=1)))
            out.append((tag + "/all_off", make(run, {})))
            for i in free:
                out.append((tag + "/free_sweep", make(run, {i: 1})))
            # spare checkers: one more on a run point, one on a point elsewhere
            # (not next to the run), and for a run of 5 a stack of 7 on one point
            opp = {e + 1: 1} if e < 23 else {s - 1: 1}
            out.append((tag + "/spare_on_run", make({**run, s + n // 2: 3}, opp)))
            away = [i for i in free if i not in opp and abs(i - s) > 1 and abs(i - e) > 1]
            out.append((tag + "/spare_elsewhere", make({**run, away[0]: 1}, opp)))
            if n == 5:
                for k in (s, e):
                    out.append((tag + "/stack7", make({**run, k: 7}, opp)))
    # negatives, the opponent behind wherever a point behind exists
    for s in range(0, 21):
        opp = {23: 1} if s + 4 < 23 else {0: 1}
        out.append(("neg/run4", make(_run(s, 4), opp)))
        if s + 4 < 23:
            out.append(("neg/run4", make(_run(s, 4), {s + 4: 1})))
    for s in range(0, 20):
        opp = {s + 5: 1} if s + 5 < 24 else {0: 1}
        for k in range(5):
            out.append(("neg/run5_single", make({**_run(s, 5), s + k: 1}, opp)))
    # two runs around a gap: 4 + gap + 3 and 3 + gap + 4, the most 15 checkers
    # allow (4 + gap + 4 would take 16), the gap empty or holding one checker
    for s in range(0, 16):
        for a, c in ((4, 3), (3, 4)):
            for g in (0, 1):
                mine = {**_run(s, a), **_run(s + a + 1, c)}
                if g:
                    mine[s + a] = 1
                opp = {s + 8: 1} if s + 8 < 24 else {0: 1}
                out.append(("neg/gap", make(mine, opp)))
    # a stack of 8..15 (the nibble's high bit) next to the longest run the
    # other checkers can still make
    for k in range(8, 16):
        m = (15 - k) // 2
        for mine in ({0: k, **_run(1, m)}, {9: k, **_run(10, m)}, {23: k, **_run(23 - m, m)}):
            out.append(("neg/stack_hi", make(mine, {i: 1 for i in (0, 8, 23) if i not in mine})))
    return out


def _close_cases():
    out = []
    for base, tag in ((18, "close/home"), (17, "close/shifted")):
        for h in range(base, base + 6):
            for v in (0, 1, 2, 5):
                for bar in (0, 1, 2, 15):
                    mine = _run(base, 6)
                    mine[h] = v
                    out.append((tag, make(mine, {}, bar_o=bar)))
    return out


def _over_cases():
    """The mover has 15 off; the loser: borne off 0 / 1 / 14, bar 0 / 1, one
    checker on each point alone or on none (14 + 1 + 1 = 16 checkers is outside
    the domain and left out)."""
    out = []
    for off in (0, 1, 14):
        for bar in (0, 1):
            for p in [None] + list(range(24)):
                if off + bar + (p is not None) > 15:
                    continue
                out.append(("over", make({}, {} if p is None else {p: 1}, bar_o=bar, off_m=15, off_o=off)))
    return out


def fixture_cases():
    """[(cell, board uint8[52], mover)], fixed order, both players."""
    out = []
    for cell, b in _prime_cases() + _close_cases() + _over_cases():
        for mover in (0, 1):
            out.append((cell, mirror(b) if mover else b, mover))
    return out


def fixture_rows():
    """(boards [2n, 52], player [2n], mover_row [2n] bool): every board once
    with its mover (the player who just moved) and once with the other player."""
    cs = fixture_cases()
    boards = np.repeat(np.stack([c[1] for c in cs]), 2, axis=0)
    player = np.array([p for c in cs for p in (c[2], 1 - c[2])], np.uint8)
    return boards, player, np.tile([True, False], len(cs))


# ---------------------------------------------------------------- start positions
# cell -> the first record of an episode from a pure position of that cell:
# (done, win_type, close_out, prime, reward)
F32 = np.float32
CELLS = {
    "regular_loser_on_bar": (1, 1, 0, 0, F32(1.0)),
    "gammon_first_point_outside": (1, 2, 0, 0, F32(2.0)),
    "backgammon_bar_only": (1, 3, 0, 0, F32(2.5)),
    "backgammon_home_edge_18": (1, 3, 0, 0, F32(2.5)),
    "backgammon_home_edge_23": (1, 3, 0, 0, F32(2.5)),
    "close_out": (0, 0, 1, 0, F32(0.0) + F32(0.30)),
    "open_five_points_bar": (0, 0, 0, 0, F32(0.0)),
    "open_home_made_bar_empty": (0, 0, 0, 0, F32(0.0)),
    "prime5_first_behind": (0, 0, 0, 1, F32(0.0) + F32(0.20)),
    "prime6_first_behind": (0, 0, 0, 1, F32(0.0) + F32(0.20)),
    "prime7_first_behind": (0, 0, 0, 1, F32(0.0) + F32(0.20)),
    "run_at_edge": (0, 0, 0, 0, F32(0.0)),
    "run_opponent_ahead_or_bar": (0, 0, 0, 0, F32(0.0)),
}


def start_holds(cell, board, pl):
    """The cell's condition on the position before the move (only the prime
    cells have one: the run's length and the opponent exactly behind it)."""
    f = features(board, pl)
    if cell.startswith("prime"):
        return f["run_len"] == int(cell[5]) and f["first_behind"] and not f["far_behind"]
    return True


def cell_holds(cell, after, pl):
    """The cell's condition on a board after `pl` moved (mover's view: home
    18..23). The home-edge cells name the points in that view."""
    f = features(after, pl)
    t = f["theirs"]
    over = f["off_m"] == 15
    if cell == "regular_loser_on_bar":
        return over and f["off_o"] >= 1 and f["bar_o"] >= 1
    if cell == "gammon_first_point_outside":
        return over and f["off_o"] == 0 and f["bar_o"] == 0 and t[17] > 0 and t[18:].sum() == 0
    if cell == "backgammon_bar_only":
        return over and f["off_o"] == 0 and f["bar_o"] > 0 and t[18:].sum() == 0
    if cell == "backgammon_home_edge_18":
        return over and f["off_o"] == 0 and f["bar_o"] == 0 and t[18] > 0 and t[19:].sum() == 0
    if cell == "backgammon_home_edge_23":
        return over and f["off_o"] == 0 and f["bar_o"] == 0 and t[23] > 0 and t[18:23].sum() == 0
    if over:
        return False
    if cell == "close_out":
        return f["home_made"] == 6 and f["bar_o"] > 0
    if cell == "open_five_points_bar":
        return f["home_made"] == 5 and f["bar_o"] > 0 and not (f["run_len"] >= 5 and (f["first_behind"] or f["far_behind"]))
    if cell == "open_home_made_bar_empty":
        return f["home_made"] == 6 and f["bar_o"] == 0
    if cell.startswith("prime"):
        # a run of 7 cannot stand still (its last checker always has a move
        # inside the run), so a cell keeps "a run of >= 5, the opponent exactly
        # behind it"; prime5 keeps the run at 5
        ok = f["run_len"] >= 5 and f["first_behind"] and not f["far_behind"] and not (f["home_made"] == 6 and f["bar_o"])
        return ok and (cell[5] != "5" or f["run_len"] == 5)
    if cell == "run_at_edge":
        return f["run_len"] >= 5 and f["run_end"] == 23 and not (f["home_made"] == 6 and f["bar_o"])
    if cell == "run_opponent_ahead_or_bar":
        return (f["run_len"] >= 5 and f["run_end"] < 23 and not f["first_behind"] and not f["far_behind"]
                and (f["ahead"] or f["bar_o"] > 0) and not (f["home_made"] == 6 and f["bar_o"]))
    raise KeyError(cell)


def _sparse(pairs):
    v = [0] * 24
    for i, k in pairs:
        v[i] = k
    return v


def _board(p0, p1, bar=(0, 0), off=(0, 0)):
    b = np.zeros(52, np.uint8)
    b[0:24] = p0
    b[24:48] = p1
    b[48:50] = bar
    b[50:52] = off
    return b


# (cell, player on roll) -> (player 0's points, player 1's points, bars, borne off, roll).
# Written by find().
_LITERALS = {
    ("regular_loser_on_bar", 0): (
        _sparse([(21, 1)]),
        _sparse([(6, 3), (8, 2), (14, 4), (16, 4)]),
        (0, 1), (14, 1), (6, 4)),
    ("regular_loser_on_bar", 1): (
        _sparse([(7, 3), (14, 5), (16, 5)]),
        _sparse([(1, 1)]),
        (1, 0), (1, 14), (3, 4)),
    ("gammon_first_point_outside", 0): (
        _sparse([(23, 1)]),
        _sparse([(8, 5), (11, 4), (12, 5), (17, 1)]),
        (0, 0), (14, 0), (2, 4)),
    ("gammon_first_point_outside", 1): (
        _sparse([(6, 1), (8, 2), (15, 5), (17, 7)]),
        _sparse([(1, 1)]),
        (0, 0), (0, 14), (6, 4)),
    ("backgammon_bar_only", 0): (
        _sparse([(19, 1)]),
        _sparse([(7, 1), (10, 4), (11, 8)]),
        (0, 2), (14, 0), (2, 4)),
    ("backgammon_bar_only", 1): (
        _sparse([(9, 4), (12, 1), (13, 2), (16, 6)]),
        _sparse([(5, 1)]),
        (2, 0), (0, 14), (5, 6)),
    ("backgammon_home_edge_18", 0): (
        _sparse([(19, 1)]),
        _sparse([(7, 1), (8, 5), (9, 3), (10, 5), (18, 1)]),
        (0, 0), (14, 0), (5, 3)),
    ("backgammon_home_edge_18", 1): (
        _sparse([(5, 1), (8, 3), (9, 3), (10, 6), (17, 2)]),
        _sparse([(3, 1)]),
        (0, 0), (0, 14), (2, 6)),
    ("backgammon_home_edge_23", 0): (
        _sparse([(19, 1)]),
        _sparse([(10, 7), (15, 2), (16, 5), (23, 1)]),
        (0, 0), (14, 0), (6, 6)),
    ("backgammon_home_edge_23", 1): (
        _sparse([(0, 1), (11, 5), (14, 6), (17, 3)]),
        _sparse([(2, 1)]),
        (0, 0), (0, 14), (6, 1)),
    ("close_out", 0): (
        _sparse([(1, 3), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2), (23, 2)]),
        _sparse([(0, 3), (3, 3), (5, 3), (11, 3), (12, 1)]),
        (0, 2), (0, 0), (6, 6)),
    ("close_out", 1): (
        _sparse([(11, 2), (16, 6), (19, 5)]),
        _sparse([(0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (22, 2), (23, 1)]),
        (2, 0), (0, 0), (6, 6)),
    ("open_five_points_bar", 0): (
        _sparse([(2, 2), (3, 2), (18, 1), (19, 2), (20, 2), (21, 2), (22, 2), (23, 2)]),
        _sparse([(0, 8), (8, 1), (10, 5)]),
        (0, 1), (0, 0), (6, 6)),
    ("open_five_points_bar", 1): (
        _sparse([(7, 3), (9, 3), (11, 2), (20, 5), (22, 1)]),
        _sparse([(0, 2), (2, 2), (3, 2), (4, 2), (5, 2), (18, 3), (19, 2)]),
        (1, 0), (0, 0), (6, 6)),
    ("open_home_made_bar_empty", 0): (
        _sparse([(1, 2), (5, 1), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2), (23, 2)]),
        _sparse([(7, 5), (11, 5), (14, 5)]),
        (0, 0), (0, 0), (6, 1)),
    ("open_home_made_bar_empty", 1): (
        _sparse([(6, 8), (9, 7)]),
        _sparse([(0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (14, 2), (21, 1)]),
        (0, 0), (0, 0), (6, 6)),
    ("prime5_first_behind", 0): (
        _sparse([(6, 1), (7, 3), (14, 1), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2)]),
        _sparse([(2, 6), (4, 1), (10, 1), (16, 5), (23, 2)]),
        (0, 0), (0, 0), (6, 6)),
    ("prime5_first_behind", 1): (
        _sparse([(0, 2), (6, 6), (8, 4), (16, 2), (23, 1)]),
        _sparse([(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (9, 2), (14, 1), (18, 2)]),
        (0, 0), (0, 0), (6, 5)),
    ("prime6_first_behind", 0): (
        _sparse([(5, 1), (13, 2), (17, 2), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2)]),
        _sparse([(2, 3), (8, 2), (11, 1), (12, 1), (16, 6), (23, 2)]),
        (0, 0), (0, 0), (6, 6)),
    ("prime6_first_behind", 1): (
        _sparse([(0, 2), (13, 5), (18, 2), (19, 2), (23, 4)]),
        _sparse([(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (17, 3)]),
        (0, 0), (0, 0), (6, 6)),
    ("prime7_first_behind", 0): (
        _sparse([(8, 1), (16, 2), (17, 2), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2)]),
        _sparse([(0, 6), (9, 1), (14, 4), (15, 2), (23, 2)]),
        (0, 0), (0, 0), (6, 6)),
    ("prime7_first_behind", 1): (
        _sparse([(0, 2), (8, 6), (10, 4), (11, 1), (13, 2)]),
        _sparse([(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (17, 1)]),
        (0, 0), (0, 0), (6, 6)),
    ("run_at_edge", 0): (
        _sparse([(2, 1), (6, 1), (12, 1), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2), (23, 2)]),
        _sparse([(4, 6), (15, 9)]),
        (0, 0), (0, 0), (5, 5)),
    ("run_at_edge", 1): (
        _sparse([(9, 3), (17, 8), (21, 4)]),
        _sparse([(0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (11, 3)]),
        (0, 0), (0, 0), (6, 6)),
    ("run_opponent_ahead_or_bar", 0): (
        _sparse([(13, 3), (15, 2), (18, 2), (19, 2), (20, 2), (21, 2), (22, 2)]),
        _sparse([(2, 10), (10, 3), (16, 2)]),
        (0, 0), (0, 0), (6, 6)),
    ("run_opponent_ahead_or_bar", 1): (
        _sparse([(8, 1), (15, 5), (20, 5), (21, 3)]),
        _sparse([(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (13, 3), (16, 1), (17, 1)]),
        (1, 0), (0, 0), (6, 6)),
}


def positions():
    """[(cell, board uint8[52], player on roll, (d0, d1))], fixed order."""
    return [(cell, _board(p0, p1, bar, off), pl, roll) for (cell, pl), (p0, p1, bar, off, roll) in _LITERALS.items()]


def afterstates(orc, board, pl, roll):
    n, res, _ = orc.movegen(board, pl, roll[0], roll[1])
    return res[:n]


def is_pure(orc, cell, board, pl, roll):
    """Every legal afterstate under the roll is in the cell and the oracle's
    five predicates give the cell's outcome on each."""
    if not start_holds(cell, board, pl):
        return False
    res = afterstates(orc, board, pl, roll)
    if len(res) == 0:
        return False
    done, wt, close, prime, _ = CELLS[cell]
    for a in res:
        if not cell_holds(cell, a, pl):
            return False
        p = {k: orc.predicate(FNS[k], a, pl) for k in KEYS}
        got_wt = 0 if not p["game_over"] else 3 if p["backgammon"] else 2 if p["gammon"] else 1
        if (int(p["game_over"]), got_wt) != (done, wt):
            return False
        if not done and (int(p["closed_out"]), int(p["prime"])) != (close, prime):
            return False
    return True


# ---------------------------------------------------------------- scripted lines
def _seq(board, player, first, script, steps, records, flags):
    return dict(board=board, player=player, first=first, script=script, steps=steps, records=records, flags=flags)


def sequences():
    """{name: line}. A line: the start board, the player on roll, the fixed first
    roll, the scripted rolls that follow (one per env step, the last one unused),
    the env steps of an episode (the engine's max_steps) and what the episode
    must hold: records [(mover, close_out, prime, reward)] in order and the
    header's flag field. In the mover's view (shown for player 0):

    close_out  home board made, three spares on point 0, the opponent on the
               bar: 6-6 moves spares only (12 moves would bring them home, two
               turns play 8). Closed out after either turn, paid once; the
               opponent cannot enter in between (no record).
    prime      points 18..22 made, two opponent checkers behind them on 23,
               five spares on point 6: 6-6 moves spares only. The opponent
               plays 2-1 inside their own home board in between.
    both       each side holds six points (17..22 / 1..6) with two opponent
               checkers behind them and one spare, which is all 6-6 can move:
               each earns its prime once, then both are stuck (two passes)."""
    out = {}
    for pl in (0, 1):
        sfx = f"_p{pl}"
        spare = make({**_run(18, 6), 0: 3}, {1: 7, 2: 7}, bar_o=1, mover=pl)
        out["close_out" + sfx] = _seq(spare, pl, (6, 6), [(3, 4), (6, 6), (1, 1)], 3,
                                      [(pl, 1, 0, F32(0.0) + F32(0.30)), (pl, 0, 0, F32(0.0))], (1 << pl) | (16 << pl))
        pr = make({**_run(18, 5), 6: 5}, {23: 2, 1: 6, 2: 7}, mover=pl)
        out["prime" + sfx] = _seq(pr, pl, (6, 6), [(2, 1), (6, 6), (1, 1)], 3,
                                  [(pl, 0, 1, F32(0.0) + F32(0.20)), (1 - pl, 0, 0, F32(0.0)), (pl, 0, 0, F32(0.0))],
                                  (4 << pl) | 48)
        both = make({**_run(17, 6), 0: 2, 7: 1}, {**_run(1, 6), 23: 2, 16: 1}, mover=pl)
        out["both" + sfx] = _seq(both, pl, (6, 6), [(6, 6), (6, 6), (6, 6), (1, 1)], 4,
                                 [(pl, 0, 1, F32(0.0) + F32(0.20)), (1 - pl, 0, 1, F32(0.0) + F32(0.20))], 4 | 8 | 48)
    return out


def walk(orc, line):
    """Play a line over every legal choice: per env step the set of boards it
    can stand on, and per step either "pass" (no board has a move) or the
    afterstates' outcomes (closed_out, prime, game_over) as a set. A line is
    pure when every step's set has one member."""
    boards = {line["board"].tobytes()}
    pl = line["player"]
    rolls = [line["first"]] + list(line["script"])
    out = []
    for k in range(line["steps"]):
        nxt, kinds = set(), set()
        for raw in boards:
            b = np.frombuffer(raw, np.uint8)
            res = afterstates(orc, b, pl, rolls[k])
            if len(res) == 0:
                kinds.add("pass")
                nxt.add(raw)
            for a in res:
                kinds.add((pl, orc.predicate("is_closed_out", a, pl), orc.predicate("made_at_least_five_prime", a, pl),
                           orc.predicate("check_game_over", a, pl)))
                nxt.add(a.tobytes())
        out.append(kinds)
        boards, pl = nxt, 1 - pl
    return out


# ---------------------------------------------------------------- the finder
def _scatter(rng, n, points, lo=1, hi=6):
    """n checkers in stacks on random points of `points`."""
    out = {}
    points = list(points)
    while n > 0 and points:
        i = int(rng.choice(points))
        k = int(min(n, rng.integers(lo, hi + 1)))
        out[i] = out.get(i, 0) + k
        n -= k
    return out, n


def _candidate(rng, cell):
    """A random member of the cell's template in the mover's view: (board, roll)."""
    roll = (int(rng.integers(1, 7)), int(rng.integers(1, 7)))
    if cell in ("regular_loser_on_bar", "gammon_first_point_outside", "backgammon_bar_only",
                "backgammon_home_edge_18", "backgammon_home_edge_23"):
        last = int(rng.integers(18, 24))
        fixed, bar, off = {}, 0, 0
        if cell == "regular_loser_on_bar":
            bar, off = 1, 1   # one checker off: the gammon test's edge
        elif cell == "gammon_first_point_outside":
            fixed = {17: 1}
        elif cell == "backgammon_bar_only":
            bar = int(rng.integers(1, 3))
        else:
            fixed = {int(cell[-2:]): 1}
        if last in fixed:
            return None
        # the loser's other checkers: outside both home boards, so that the cell's checker alone decides
        rest, left = _scatter(rng, 15 - bar - off - sum(fixed.values()), range(6, 17))
        return make({last: 1}, {**rest, **fixed}, bar_o=bar, off_m=14, off_o=off + left), roll
    if cell in ("close_out", "open_five_points_bar", "open_home_made_bar_empty"):
        mine = _run(18, 6)
        if cell == "open_five_points_bar":
            mine[int(rng.integers(18, 24))] = int(rng.integers(0, 2))
        bar = 0 if cell == "open_home_made_bar_empty" else int(rng.integers(1, 3))
        sp, left = _scatter(rng, 15 - sum(mine.values()), range(0, 12), 1, 3)
        rest, left_o = _scatter(rng, 15 - bar, [i for i in range(0, 18) if i not in sp])
        return make({**mine, **sp}, rest, bar_o=bar, off_m=left, off_o=left_o), roll
    if cell.startswith("prime") or cell in ("run_at_edge", "run_opponent_ahead_or_bar"):
        n = int(cell[5]) if cell.startswith("prime") else int(rng.integers(5, 8))
        s = 24 - n if cell == "run_at_edge" else int(rng.integers(8, 24 - n))
        run, e = _run(s, n), s + n - 1
        sp, left = _scatter(rng, 15 - 2 * n, range(0, s), 1, 3)
        behind = {e + 1: int(rng.integers(1, 3))} if cell.startswith("prime") else {}
        bar = int(rng.integers(0, 2)) if cell == "run_opponent_ahead_or_bar" else 0
        rest, left_o = _scatter(rng, 15 - bar - sum(behind.values()), [i for i in range(0, s) if i not in sp])
        if cell == "run_opponent_ahead_or_bar" and not rest and not bar:
            return None
        return make({**run, **sp}, {**rest, **behind}, bar_o=bar, off_m=left, off_o=left_o), roll
    raise KeyError(cell)


def find(orc, log=print, tries=200000):
    """Regenerate _LITERALS (seeded: the same list every run): per cell and
    player the first pure candidate of a seeded stream."""
    found = {}
    for c, cell in enumerate(CELLS):
        for pl in (0, 1):
            rng = np.random.default_rng(1000 * c + pl)
            for t in range(tries):
                cand = _candidate(rng, cell)
                if cand is None:
                    continue
                b, roll = cand
                if pl:
                    b = mirror(b)
                if b[50 + pl] < 15 and is_pure(orc, cell, b, pl, roll):
                    found[(cell, pl)] = (b, roll)
                    log(f"{cell} p{pl}: candidate {t}")
                    break
            else:
                log(f"{cell} p{pl}: NOT FOUND")
    return found


def _literal(b, roll):
    def sp(v):
        return "_sparse([" + ", ".join(f"({i}, {int(k)})" for i, k in enumerate(v) if k) + "])"
    return (f"(\n        {sp(b[0:24])},\n        {sp(b[24:48])},\n"
            f"        ({int(b[48])}, {int(b[49])}), ({int(b[50])}, {int(b[51])}), ({roll[0]}, {roll[1]}))")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle as _orc
    for (_cell, _pl), (_b, _roll) in find(_orc, log=lambda s: print("#", s)).items():
        print(f'    ("{_cell}", {_pl}): {_literal(_b, _roll)},')
