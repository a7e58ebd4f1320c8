"""Position rollouts on the GPU: the start table and the restart path
(bgx_engine_set_start), first rolls (fixed, stratified, rolled, scripted), the
device tally (bgx_rollout_tally) and bgx.rollout.rollout() on positions with
known answers (A-D of tests/test_rollout_tally.py, checked against the oracle
for all 36 rolls), at ply 1 and 2 and combined with match mode.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden
from test_gpu_engine import _by_episode, _check_transitions, _collect, _engine, _same_runs
from test_rollout_tally import POS_A, POS_B, POS_C, POS_D

pytestmark = pytest.mark.gpu


def _midgame():
    """A contact position from the movegen cases with player 1 on roll."""
    from bgx.rollout import check_positions
    b = golden("movegen_cases.npz")["boards"][105]
    check_positions(b, 1)
    assert not np.array_equal(b, golden("movegen_cases.npz")["boards"][0]) and not b[48:].any()
    return b


def _table():
    return np.stack([POS_C, POS_D, _midgame()]), np.array([0, 0, 1], np.uint8)


def _packed(boards, player):
    from test_cpuwave import _pack
    return _pack(boards, player)


def _check_starts(boards, player, hdrs, recs, lane_pos):
    """Every harvested episode starts from its lane's position: the first
    record's before-board, every record's mover = start player ^ (step & 1).
    Returns the episodes seen per position."""
    seen = np.zeros(len(boards), np.int64)
    for hdr, d in zip(hdrs, recs):
        o = 0
        for row in hdr:
            n, pos = int(row[3]), lane_pos(int(row[0]))
            assert n > 0
            np.testing.assert_array_equal(d["before"][o], boards[pos], err_msg=str(row[:5]))
            np.testing.assert_array_equal(d["mover"][o:o + n], int(player[pos]) ^ (d["step"][o:o + n] & 1))
            seen[pos] += 1
            o += n
    return seen


def test_starts_and_restarts_from_the_table(weights_seed0):
    """70 lanes from global lane 5, positions C, D and a contact position
    (player 1 on roll), rolled first rolls: before any step every lane holds its
    position and player; after 120 steps every harvested episode (the lanes'
    first and their restarts) starts from its position with the right mover,
    the D lanes' first step is a pass, every transition is the oracle's (fresh
    shaping flags per episode, rewards, win types), and doubles occur among the
    C lanes' first rolls (a mid-game roll, not the opening's)."""
    boards, player = _table()
    e = _engine(weights_seed0, lanes=70, lane_base=5, seed=3, ply=1, fused=False)
    e.set_start(boards, player)
    g = 5 + np.arange(70)
    np.testing.assert_array_equal(e.peek("lane_rows")[:70], _packed(boards, player)[g % 3])
    np.testing.assert_array_equal(e.peek("player")[:70], player[g % 3])
    hdrs, recs = _collect(e, 120)
    e.close()
    seen = _check_starts(boards, player, hdrs, recs, lambda lane: lane % 3)
    assert seen[0] > 1000 and seen[1] > 0 and seen[2] > 0, seen
    first_c, restarts = [], 0
    for hdr, d in zip(hdrs, recs):
        o = 0
        for row in hdr:
            n, pos = int(row[3]), int(row[0]) % 3
            restarts += int(row[1]) > 0
            if pos == 0:
                assert d["step"][o] == 0 and n == 2 and int(row[4]) == 2
                first_c.append(tuple(d["dice"][o]))
            if pos == 1:
                assert d["step"][o] >= 1 and d["mover"][o] == 1   # player 0 had no move
            o += n
    assert restarts > 1000
    assert any(a == b for a, b in first_c) and any(a != b for a, b in first_c)
    assert _check_transitions(weights_seed0, hdrs, recs, 1) > 3000


def test_fixed_and_stratified_first_rolls(weights_seed0):
    """Positions [C rolled, C with fixed dice 6-5], 24 lanes from global lane
    6, strat_stride = J = 12, 12 steps = G = 6 two-step games per lane: every
    episode of the fixed position starts with 6-5; episode k of lane g of the
    rolled one starts with roll t % 36 of trial t = 12 k + g // 2, and over the
    J * G = 72 trials each of the 36 ordered rolls occurs exactly twice."""
    boards = np.stack([POS_C, POS_C])
    e = _engine(weights_seed0, lanes=24, lane_base=6, seed=9, ply=1, fused=False, greedy=True)
    e.set_start(boards, [0, 0], dice=[[0, 0], [6, 5]], strat_stride=12)
    hdrs, recs = _collect(e, 12, chunk=5)
    e.close()
    eps = _by_episode(hdrs, recs)
    assert sorted(eps) == [(g, k) for g in range(6, 30) for k in range(6)]
    rolls = []
    for (g, k), (_, d) in eps.items():
        assert d["step"][0] == 0
        if g % 2:
            assert tuple(d["dice"][0]) == (6, 5)
        else:
            r = (12 * k + g // 2) % 36
            assert tuple(d["dice"][0]) == (r // 6 + 1, r % 6 + 1), (g, k)
            rolls.append(tuple(d["dice"][0]))
    assert len(rolls) == 72 and all(rolls.count((a, b)) == 2 for a in range(1, 7) for b in range(1, 7))
    _check_starts(boards, [0, 0], hdrs, recs, lambda lane: lane % 2)


@pytest.mark.parametrize("fixed", [False, True])
def test_scripted_dice_are_consumed_in_order(weights_seed0, fixed):
    """Greedy lanes with scripted dice on position C (two-step games: player
    0's move, then player 1's winning move). Rolled first rolls: each episode
    takes four draws, the restart's first roll and the roll after player 0's
    move (none after the terminal move), so a lane's records carry its script
    pair by pair. Fixed dice 6-5: the restart draws nothing, the records
    alternate 6-5 and the script's pairs. set_dice before set_start, and the
    other way round."""
    rng = np.random.default_rng(17)
    script = rng.integers(1, 7, (8, 128)).astype(np.uint8)
    runs = []
    for dice_first in (True, False):
        e = _engine(weights_seed0, lanes=8, seed=2, ply=1, fused=False, greedy=True)
        if dice_first:
            e.set_dice(script)
        e.set_start(POS_C, [0], dice=(6, 5) if fixed else None)
        if not dice_first:
            e.set_dice(script)
        hdrs, recs = _collect(e, 40, chunk=15)
        e.close()
        eps = _by_episode(hdrs, recs)
        assert sorted(eps) == [(g, k) for g in range(8) for k in range(20)]
        for g in range(8):
            got = np.concatenate([eps[(g, k)][1]["dice"] for k in range(20)])
            pairs = script[g].reshape(-1, 2)
            if fixed:
                np.testing.assert_array_equal(got[0::2], np.tile([6, 5], (20, 1)))
                np.testing.assert_array_equal(got[1::2], pairs[:20])
            else:
                np.testing.assert_array_equal(got, pairs[:40])
        runs.append(eps)
    _same_runs(*runs)


def test_rollout_known_answers(weights_seed0):
    """rollout() on A, B and C together (trials=72, lanes=64: 21 lanes per
    position, 12 games each = 252 stratified trials): equity exactly 3.0, 1.0
    and -2.0 with standard error 0.0, nothing unfinished, 1, 1 and 2 env steps
    per game. A alone with 64 lanes and 64 * 200 trials: 207 one-step games per
    lane finish without overflowing the episode list."""
    from bgx.rollout import rollout
    res = rollout(weights_seed0, np.stack([POS_A, POS_B, POS_C]), [0, 0, 0], trials=72, lanes=64)
    assert (res["lanes"], res["lanes_per_position"], res["games_per_lane"], res["trials"]) == (63, 21, 12, 252)
    assert res["tallied_steps"] == 252 * (1 + 1 + 2) and res["env_steps"] == 63 * 128
    want = [(3.0, 1.0, ("on_roll", "backgammon")), (1.0, 1.0, ("on_roll", "regular")), (-2.0, 2.0, ("other", "gammon"))]
    for pos, (eq, steps, (side, wt)) in zip(res["positions"], want):
        assert pos["games"] == 252 and pos["unfinished"] == 0
        assert pos["equity"] == eq and pos["equity_se"] == 0.0 and pos["mean_steps"] == steps
        assert pos["wins"][side][wt] == 252
    res = rollout(weights_seed0, POS_A, [0], trials=64 * 200, lanes=64)
    assert (res["lanes"], res["games_per_lane"], res["trials"]) == (64, 207, 64 * 207)
    pos = res["positions"][0]
    assert pos["games"] == 64 * 207 and pos["wins"]["on_roll"]["backgammon"] == 64 * 207
    assert pos["equity"] == 3.0 and pos["equity_se"] == 0.0 and pos["mean_steps"] == 1.0
    assert res["tallied_steps"] == 64 * 207 <= res["env_steps"]   # one env step per counted game


@pytest.mark.parametrize("ply", [1, 2])
def test_device_tally_equals_host_tally(weights_seed0, ply):
    """rollout(return_episodes=True) on C, D and the contact position, 21 lanes
    each, two games per lane: the device counts equal tally_counts of the
    returned headers exactly, every (lane, game) is there once, the same seed
    gives the same counts, and (ply 1) so does another harvest cadence."""
    from bgx.rollout import rollout, tally_counts
    boards, player = _table()
    kw = dict(trials=42, lanes=63, ply=ply, k_top=4, greedy=False, seed=5, stratify=False, return_episodes=True)
    res = rollout(weights_seed0, boards, player, chunk=50, **kw)
    assert (res["lanes"], res["games_per_lane"]) == (63, 2)
    h = res["headers"]
    assert sorted(zip(h[:, 0].tolist(), h[:, 1].tolist())) == [(g, k) for g in range(63) for k in range(2)]
    assert res["records"].shape[0] == int(h[:, 3].sum())
    np.testing.assert_array_equal(res["counts"], tally_counts(h, player, 3, 2))
    assert [p["games"] for p in res["positions"]] == [42, 42, 42]
    assert res["positions"][0]["equity"] == -2.0 and res["positions"][0]["mean_steps"] == 2.0
    # the perspective: the contact position's player on roll is player 1
    won = int(np.sum((h[:, 0] % 3 == 2) & ((h[:, 5] & 0xFF) > 0) & (((h[:, 5] >> 8) & 0xFF) == 1)))
    assert sum(res["positions"][2]["wins"]["on_roll"].values()) == won
    again = rollout(weights_seed0, boards, player, chunk=50, **kw)
    np.testing.assert_array_equal(again["counts"], res["counts"])
    if ply == 1:
        other = rollout(weights_seed0, boards, player, chunk=16, **kw)
        np.testing.assert_array_equal(other["counts"], res["counts"])


@pytest.mark.parametrize("k_top", [4, 0])
def test_two_ply_starts_from_the_table(weights_seed0, k_top):
    boards, player = _table()
    e = _engine(weights_seed0, lanes=63, seed=3, ply=2, k_top=k_top)
    e.set_start(boards, player)
    hdrs, recs = _collect(e, 40)
    e.close()
    seen = _check_starts(boards, player, hdrs, recs, lambda lane: lane % 3)
    assert seen[0] >= 21 * 19, seen
    assert _check_transitions(weights_seed0, hdrs, recs, 2) > 800


def test_match_mode_and_leaving_the_mode(weights_seed0):
    """The same network on both sides of match mode plus set_start gives the
    records of the plain set_start engine; after set_start(None) the engine
    replays a fresh self-play engine of the same seed."""
    boards, player = _table()
    runs = []
    for match in (True, False):
        e = _engine(weights_seed0, lanes=66, seed=7, ply=1, fused=False)
        if match:
            e.set_opponent(weights_seed0)
        e.set_start(boards, player, strat_stride=22)
        runs.append(_by_episode(*_collect(e, 60, chunk=25)))
        if match:
            e.close()
    _same_runs(*runs)   # (the plain engine stays open)
    e.set_start(None)
    left = _by_episode(*_collect(e, 150, chunk=60))
    e.set_start(None)   # outside the mode: a no-op (the lanes keep their games)
    e.close()
    fresh = _engine(weights_seed0, lanes=66, seed=7, ply=1, fused=False)
    want = _by_episode(*_collect(fresh, 150, chunk=60))
    fresh.close()
    _same_runs(want, left)


def test_set_start_states_and_rejections(weights_seed0):
    from bgx import BgxError
    e = _engine(weights_seed0, lanes=64, seed=3, ply=1)   # fused
    with pytest.raises(BgxError, match=r"\(-4\).*phased"):
        e.set_start(POS_C, [0])
    e.close()
    e = _engine(weights_seed0, lanes=16, seed=3, ply=1, fused=False)
    over = POS_A.copy()
    over[23], over[50] = 0, 15
    fourteen = POS_A.copy()
    fourteen[24 + 5] = 4
    shared = POS_C.copy()
    shared[1], shared[12] = 1, 4
    for boards, dice, text in [(np.stack([POS_C, over]), None, "position 1 is already over"),
                               (np.stack([POS_C, POS_D, fourteen]), None, "position 2 has 15 and 14"),
                               (np.stack([POS_C, POS_D]), [[0, 0], [0, 3]], "position 1 has dice 0, 3"),
                               (np.stack([shared, POS_D]), None, "position 0 outside the input domain")]:
        with pytest.raises(BgxError, match=rf"\(-1\).*{text}"):
            e.set_start(boards, np.zeros(len(boards), np.uint8), dice=dice)
    with pytest.raises(BgxError, match=r"\(-1\).*position 0 outside the input domain"):
        e.set_start(POS_C, [2])
    with pytest.raises(ValueError, match="player"):
        e.set_start(POS_C)
    e.step(30)   # still a self-play engine
    e.harvest()
    e.sync()
    assert e.stats()["env_steps"] == 16 * 30
    e.close()


def test_cli_opening_table(capsys):
    from bgx.rollout import main
    main([os.path.join(GOLDEN, "weights_ckpt2100000.npz"), "--opening", "--trials", "36", "--lanes", "540"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(res["positions"]) == 15 and res["trials"] == 36 and res["lanes"] == 540
    assert sorted(tuple(p["dice"]) for p in res["positions"]) == sorted(
        (a, b) for a in range(1, 7) for b in range(1, a))
    for p in res["positions"]:
        assert p["games"] == 36 and -3.0 <= p["equity"] <= 3.0 and p["mean_steps"] >= 13
