"""The env step's outcome rules on the GPU, from positions one move before each
cell (tests/outcome_cases.py).

A position of the table is pure: under its fixed roll every legal afterstate
falls in one cell (tests/test_outcome_cases.py checks that on the oracle), so
the first record of every episode from it is known before the run, whatever
the network picks: done, win type, close-out and prime flags and the reward's
bits are stated here from the case table, and every harvested transition is
also replayed through the oracle. The scripted lines check the once-per-player
rule over a game and the episode header's flag field. Episodes are cut short
by a small max_steps, so every lane restarts from its position several times.
"""
import numpy as np
import pytest

import outcome_cases as oc
from test_gpu_engine import _by_episode, _check_transitions, _collect, _engine

pytestmark = pytest.mark.gpu

MAX_STEPS = 8


def _table(ps):
    return (np.stack([p[1] for p in ps]), np.array([p[2] for p in ps], np.uint8),
            np.array([p[3] for p in ps], np.uint8))


def _bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def _check_first_records(ps, eps, lanes, min_episodes):
    """The first record of every episode against the case table; returns the
    episodes seen per lane."""
    seen = np.zeros(lanes, np.int64)
    for (lane, k), (row, d) in eps.items():
        cell, board, pl, roll = ps[lane % len(ps)]
        done, wt, close, prime, reward = oc.CELLS[cell]
        what = (cell, pl, lane, k)
        assert int(row[0]) >= 1, what
        np.testing.assert_array_equal(d["before"][0], board, err_msg=str(what))
        assert (int(d["mover"][0]), int(d["step"][0]), tuple(int(x) for x in d["dice"][0])) == (pl, 0, roll), what
        got = (int(d["done"][0]), int(d["win_type"][0]), int(d["close_out"][0]), int(d["prime"][0]))
        assert got == (done, wt, close, prime), (what, got)
        assert _bits(d["reward"][0]) == _bits(reward), (what, d["reward"][0])
        if done:   # a one-step game: the header carries the win and the winner, no shaping bit
            assert int(row[0]) == 1 and int(row[1]) == 1 and int(row[2]) == wt | (pl << 8) | ((16 << pl) << 16), what
        else:      # what the first record earned is in the header whatever followed
            want = (close | 4 * prime | 16) << pl
            assert (int(row[2]) >> 16) & want == want, what
        seen[lane] += 1
    assert seen.min() >= min_episodes, seen
    return seen


def _check_rules(hdrs, recs):
    """Reward, done, win type and shaping flags of every record from its
    afterstate alone (the oracle's predicates, flags per episode), and the
    header's flag field; for runs whose V the single-network replay of
    _check_transitions cannot follow (match mode)."""
    import oracle as orc
    n = 0
    for hdr, d in zip(hdrs, recs):
        o = 0
        for row in hdr:
            flags = 0
            for k in range(o, o + int(row[3])):
                a, pl = d["after"][k], int(d["mover"][k])
                flags |= 16 << pl
                if orc.predicate("check_game_over", a, pl):
                    wt = 3 if orc.predicate("check_for_backgammon", a, pl) else (
                        2 if orc.predicate("check_for_gammon", a, pl) else 1)
                    want = (1, wt, 0, 0, _bits({1: 1.0, 2: 2.0, 3: 2.5}[wt]))
                else:
                    co = orc.predicate("is_closed_out", a, pl) and not (flags >> pl) & 1
                    pr = orc.predicate("made_at_least_five_prime", a, pl) and not (flags >> (2 + pl)) & 1
                    flags |= (int(co) << pl) | (int(pr) << (2 + pl))
                    r = np.float32(0.0)
                    if co:
                        r = np.float32(r + np.float32(0.30))
                    if pr:
                        r = np.float32(r + np.float32(0.20))
                    want = (0, 0, int(co), int(pr), _bits(r))
                got = (int(d["done"][k]), int(d["win_type"][k]), int(d["close_out"][k]), int(d["prime"][k]),
                       _bits(d["reward"][k]))
                assert got == want, (row[:6], k - o, got, want)
                n += 1
            assert int(row[5]) >> 16 == flags, (row[:6], flags)
            o += int(row[3])
    return n


def test_first_records_1ply_whole_table(weights_seed0):
    """Phased 1-ply, sampling, the whole table with its fixed rolls, two lanes
    per position, 24 steps of 8-step episodes: at least three episodes per lane
    (24 from a terminal cell). Every episode's first record carries its cell's
    outcome, restarts included (fresh flags: the close-out and the prime are
    paid again in every episode), and every transition is the oracle's."""
    ps = oc.positions()
    boards, player, dice = _table(ps)
    lanes = 2 * len(ps)
    e = _engine(weights_seed0, lanes=lanes, seed=41, ply=1, fused=False, max_steps=MAX_STEPS)
    e.set_start(boards, player, dice=dice)
    hdrs, recs = _collect(e, 3 * MAX_STEPS, chunk=3 * MAX_STEPS)
    st = e.stats()
    e.close()
    assert st["env_steps"] == lanes * 3 * MAX_STEPS
    eps = _by_episode(hdrs, recs)
    seen = _check_first_records(ps, eps, lanes, 3)
    for lane in range(lanes):
        cell = ps[lane % len(ps)][0]
        if oc.CELLS[cell][0]:   # one-step games
            assert seen[lane] == 3 * MAX_STEPS, (cell, seen[lane])
    paid = [k for (lane, k), (_, d) in eps.items() if k >= 1 and (d["close_out"][0] or d["prime"][0])]
    assert len(paid) >= 2 * 2 * 2 * 4   # 2 lanes x 2 restarts x 2 players x (close-out + three primes)
    assert _check_transitions(weights_seed0, hdrs, recs, 1, max_steps=MAX_STEPS) > 3 * lanes
    assert _check_rules(hdrs, recs) == sum(len(d["action"]) for d in recs)


@pytest.mark.parametrize("k_top", [4, 0])
def test_first_records_2ply(weights_seed0, k_top):
    """ply = 2 (the top 4 by 1-ply value, and every candidate), one lane per
    cell and player, two 4-step episodes each."""
    ps = oc.positions()
    boards, player, dice = _table(ps)
    e = _engine(weights_seed0, lanes=len(ps), seed=43, ply=2, k_top=k_top, max_steps=4)
    e.set_start(boards, player, dice=dice)
    hdrs, recs = _collect(e, 8, chunk=8)
    e.close()
    _check_first_records(ps, _by_episode(hdrs, recs), len(ps), 2)
    assert _check_transitions(weights_seed0, hdrs, recs, 2, max_steps=4) > 4 * len(ps)
    _check_rules(hdrs, recs)


def test_first_records_match_mode(weights_ckpt, weights_seed0):
    """Match mode, two different networks (player p of episode k on lane g is
    played by network (p ^ g ^ k) & 1): two lanes per position and three
    episodes, so either network makes every cell's move."""
    ps = oc.positions()
    boards, player, dice = _table(ps)
    lanes = 2 * len(ps)
    e = _engine(weights_ckpt, lanes=lanes, seed=47, ply=1, fused=False, max_steps=MAX_STEPS)
    e.set_opponent(weights_seed0)
    e.set_start(boards, player, dice=dice)
    hdrs, recs = _collect(e, 3 * MAX_STEPS, chunk=3 * MAX_STEPS)
    e.close()
    eps = _by_episode(hdrs, recs)
    _check_first_records(ps, eps, lanes, 3)
    nets = {(lane % len(ps), (ps[lane % len(ps)][2] ^ lane ^ k) & 1) for lane, k in eps}
    assert nets == {(i, n) for i in range(len(ps)) for n in (0, 1)}
    assert _check_rules(hdrs, recs) > 3 * lanes


@pytest.mark.parametrize("steps", [3, 4])
def test_shaping_rewards_are_paid_once_per_player(weights_ckpt, steps):
    """The scripted lines of outcome_cases.sequences() (greedy, fixed first
    roll, then scripted dice; pure at every step), three episodes on two lanes
    each. steps = 3: a close-out that holds again after the opponent's pass and
    a prime that stands over the opponent's move pay once (the second record
    has close_out = prime = 0 and reward +0.0), for either player. steps = 4:
    both players earn their prime in one game, then both pass. The header's
    flag field is the OR of what the records earned plus a "moved" bit for each
    player with a record."""
    lines = [(name, ln) for name, ln in oc.sequences().items() if ln["steps"] == steps]
    assert len(lines) == (4 if steps == 3 else 2)
    n_ep, lanes = 3, 2 * len(lines)
    boards = np.stack([ln["board"] for _, ln in lines])
    player = np.array([ln["player"] for _, ln in lines], np.uint8)
    first = np.array([ln["first"] for _, ln in lines], np.uint8)
    script = np.stack([np.tile(np.array(lines[g % len(lines)][1]["script"], np.uint8).reshape(-1), n_ep)
                       for g in range(lanes)])
    assert script.shape == (lanes, 2 * steps * n_ep)
    e = _engine(weights_ckpt, lanes=lanes, seed=53, ply=1, fused=False, greedy=True, max_steps=steps)
    e.set_start(boards, player, dice=first)   # first: the restart set_dice makes then draws nothing
    e.set_dice(script)
    hdrs, recs = _collect(e, steps * n_ep, chunk=steps * n_ep)
    e.close()
    eps = _by_episode(hdrs, recs)
    assert sorted(eps) == [(g, k) for g in range(lanes) for k in range(n_ep)]
    for (lane, k), (row, d) in eps.items():
        name, ln = lines[lane % len(lines)]
        got = [(int(d["mover"][i]), int(d["close_out"][i]), int(d["prime"][i]), _bits(d["reward"][i]))
               for i in range(int(row[0]))]
        assert got == [(m, c, p, _bits(r)) for m, c, p, r in ln["records"]], (name, lane, k, got)
        assert not d["done"].any()
        assert (int(row[1]), int(row[2]) & 0xFFFF, int(row[2]) >> 16) == (steps, 0xFF00, ln["flags"]), (name, row[:3])
        np.testing.assert_array_equal(d["before"][0], ln["board"])
    if steps == 3:   # the repeat: the predicate holds, nothing is paid, the reward is +0.0
        for name, ln in lines:
            assert ln["records"][-1][1:3] == (0, 0) and _bits(ln["records"][-1][3]) == 0
    assert _check_transitions(weights_ckpt, hdrs, recs, 1, max_steps=steps) == sum(int(r[0]) for r, _ in eps.values())
    _check_rules(hdrs, recs)
