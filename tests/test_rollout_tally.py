"""The numpy side of position rollouts (bgx/rollout.py): tally_counts,
summarize and check_positions on hand-built headers and boards, exact numbers.
No GPU and no libbgx.so.

The fixture positions A-D (u8[52]: positions_0[24] | positions_1[24] | bar[2] |
off[2]; player 0 moves up, home on points 18..23; player 0 on roll) are shared
with the GPU tests (tests/test_gpu_rollout.py):
  A  every move of every roll wins a backgammon (equity 3.0, one env step);
  B  every move wins a regular game (equity 1.0);
  C  player 0 always moves and never ends the game, player 1 then wins a gammon
     with any roll (equity -2.0, two env steps and two records);
  D  player 0 is on the bar against a closed board: every first step is a pass.
"""
import numpy as np
import pytest

from bgx.records import EP_WORDS
from bgx.rollout import check_positions, plan, summarize, tally_counts


def position(p0, p1, bar=(0, 0), off=(0, 0)):
    b = np.zeros(52, np.uint8)
    for k, v in p0.items():
        b[k] = v
    for k, v in p1.items():
        b[24 + k] = v
    b[48:50] = bar
    b[50:52] = off
    return b


POS_A = position({23: 1}, {20: 2, 12: 5, 7: 3, 5: 5}, off=(14, 0))
POS_B = position({23: 1}, {20: 2, 12: 5, 7: 3, 5: 4}, off=(14, 1))
POS_C = position({12: 5, 13: 5, 14: 5}, {1: 1}, off=(0, 14))
POS_D = position({18: 5, 19: 5, 20: 4}, {0: 2, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 3}, bar=(1, 0))


def header(lane, episode, steps, win_type, winner):
    h = np.zeros(EP_WORDS, np.uint32)
    h[0], h[1], h[4] = lane, episode, steps
    h[5] = win_type | ((winner & 0xFF) << 8) | (0x30 << 16)   # the "decided" flag bits ride along
    return h


def random_headers(rng, n, lanes, episodes):
    """n headers: every win type, both winners, unfinished games (win type 0,
    winner byte 0xFF as the engine writes it)."""
    out = np.zeros((n, EP_WORDS), np.uint32)
    for i in range(n):
        wt = int(rng.integers(0, 4))
        out[i] = header(int(rng.integers(0, lanes)), int(rng.integers(0, episodes)), int(rng.integers(1, 301)), wt,
                        int(rng.integers(0, 2)) if wt else 0xFF)
    return out


def loop_counts(headers, start_player, n_pos, max_episode):
    """The tally as a plain loop (the statement of the issue's table)."""
    c = [[0] * 8 for _ in range(n_pos)]
    for h in headers:
        lane, epi, steps, w5 = int(h[0]), int(h[1]), int(h[4]), int(h[5])
        if epi >= max_episode:
            continue
        pos = lane % n_pos
        wt, winner = w5 & 0xFF, (w5 >> 8) & 0xFF
        if wt == 0:
            c[pos][6] += 1
        elif winner == start_player[pos]:
            c[pos][wt - 1] += 1
        else:
            c[pos][3 + wt - 1] += 1
        c[pos][7] += steps
    return np.array(c, np.uint64)


@pytest.mark.parametrize("n,n_pos", [(0, 1), (1, 1), (500, 1), (500, 3), (700, 600)])
def test_tally_counts_equals_plain_loop(n, n_pos):
    rng = np.random.default_rng(n + n_pos)
    h = random_headers(rng, n, lanes=1000, episodes=6)
    sp = rng.integers(0, 2, n_pos).astype(np.uint8)
    for max_ep in (0, 3, 6):
        got = tally_counts(h, sp, n_pos, max_ep)
        assert got.dtype == np.uint64 and got.shape == (n_pos, 8)
        np.testing.assert_array_equal(got, loop_counts(h, sp, n_pos, max_ep))
    # int32 headers (what a harvest tensor gives) count the same
    np.testing.assert_array_equal(tally_counts(h.view(np.int32), sp, n_pos, 6), loop_counts(h, sp, n_pos, 6))


def test_tally_episode_filter_and_both_start_players():
    """Two positions, position 0 with player 0 on roll and position 1 with
    player 1: lanes 0, 2, 4 play position 0, lanes 1, 3 position 1. Player 1
    wins a gammon on lane 0 (a loss for the player on roll) and on lane 1 (a
    win for the player on roll); episode 2 is filtered out at max_episode 2."""
    h = np.stack([header(0, 0, 10, 2, 1), header(1, 0, 11, 2, 1), header(2, 1, 5, 3, 0), header(3, 1, 300, 0, 0xFF),
                  header(4, 2, 7, 1, 0), header(1, 2, 9, 1, 0)])
    sp = np.array([0, 1], np.uint8)
    np.testing.assert_array_equal(tally_counts(h, sp, 2, 2),
                                  np.array([[0, 0, 1, 0, 1, 0, 0, 15], [0, 1, 0, 0, 0, 0, 1, 311]], np.uint64))
    np.testing.assert_array_equal(tally_counts(h, sp, 2, 3),
                                  np.array([[1, 0, 1, 0, 1, 0, 0, 22], [0, 1, 0, 1, 0, 0, 1, 320]], np.uint64))
    np.testing.assert_array_equal(tally_counts(h, sp, 2, 0), np.zeros((2, 8), np.uint64))
    # the same headers seen from the other side: wins and losses swap
    np.testing.assert_array_equal(tally_counts(h, 1 - sp, 2, 3),
                                  np.array([[0, 1, 0, 1, 0, 1, 0, 22], [1, 0, 0, 0, 1, 0, 1, 320]], np.uint64))


def test_summarize_equity_and_standard_error():
    counts = np.array([[5, 3, 1, 4, 2, 1, 2, 180],      # mixed
                       [72, 0, 0, 0, 0, 0, 0, 72],      # every game the same: se exactly 0
                       [0, 0, 0, 0, 144, 0, 0, 288],
                       [0, 0, 1, 0, 0, 0, 0, 1],        # one game: se 0.0 by definition
                       [0, 0, 0, 0, 0, 0, 0, 0]], np.uint64)
    s = summarize(counts)
    assert [p["games"] for p in s] == [18, 72, 144, 1, 0]
    # the per-game points the first row implies, spelled out
    pts = np.array([1] * 5 + [2] * 3 + [3] * 1 + [-1] * 4 + [-2] * 2 + [-3] * 1 + [0] * 2, np.float64)
    assert s[0]["equity"] == pytest.approx(pts.mean(), abs=1e-15)
    assert s[0]["equity_se"] == pytest.approx(pts.std(ddof=1) / np.sqrt(18), rel=1e-12)
    assert s[0]["wins"] == {"on_roll": {"regular": 5, "gammon": 3, "backgammon": 1},
                            "other": {"regular": 4, "gammon": 2, "backgammon": 1}}
    assert s[0]["unfinished"] == 2 and s[0]["mean_steps"] == 10.0
    assert (s[1]["equity"], s[1]["equity_se"], s[1]["mean_steps"]) == (1.0, 0.0, 1.0)
    assert (s[2]["equity"], s[2]["equity_se"], s[2]["mean_steps"]) == (-2.0, 0.0, 2.0)
    assert (s[3]["equity"], s[3]["equity_se"]) == (3.0, 0.0)
    assert (s[4]["equity"], s[4]["equity_se"], s[4]["mean_steps"]) == (0.0, 0.0, 0.0)
    # counts beyond 2^53 / 2^32 stay exact integers
    big = summarize(np.array([[1 << 40, 0, 0, 1 << 40, 0, 0, 0, 3 << 40]], np.uint64))[0]
    assert big["games"] == 1 << 41 and big["equity"] == 0.0 and big["mean_steps"] == 1.5


def test_check_positions_accepts_the_fixtures():
    b, p, d = check_positions(np.stack([POS_A, POS_B, POS_C, POS_D]), [0, 0, 0, 0])
    assert b.dtype == np.uint8 and b.shape == (4, 52) and p.tolist() == [0, 0, 0, 0] and not d.any()
    b, p, d = check_positions(np.stack([POS_C, POS_D]), [1, 0], dice=[[6, 5], [0, 0]])
    assert d.tolist() == [[6, 5], [0, 0]] and p.tolist() == [1, 0]
    b, p, d = check_positions(POS_A, 0, dice=(3, 3))
    assert b.shape == (1, 52) and d.tolist() == [[3, 3]]


def _bad_cases():
    over = position({}, {20: 2, 12: 5, 7: 3, 5: 5}, off=(15, 0))
    fourteen = POS_A.copy()
    fourteen[24 + 5] = 4
    sixteen = POS_A.copy()
    sixteen[24 + 5] = 6
    shared = POS_C.copy()
    shared[1], shared[12] = 1, 4
    value = position({12: 15}, {1: 1}, off=(0, 14))
    value[12], value[13] = 16, 0
    return [("over", over, 0, (0, 0), "already over"), ("14 checkers", fourteen, 0, (0, 0), "checkers"),
            ("16 checkers", sixteen, 0, (0, 0), "checkers"), ("shared point", shared, 0, (0, 0), "both players"),
            ("count above 15", value, 0, (0, 0), "outside 0..15"), ("player", POS_A, 2, (0, 0), "player 2"),
            ("dice 0-3", POS_A, 0, (0, 3), "dice 0, 3"), ("dice 7", POS_A, 0, (7, 1), "dice 7, 1")]


@pytest.mark.parametrize("k", range(8))
def test_check_positions_each_rejection_names_the_first_bad_index(k):
    name, board, player, dice, text = _bad_cases()[k]
    boards = np.stack([POS_A, POS_D, board, board])
    with pytest.raises(ValueError, match=rf"position 2: .*{text}"):
        check_positions(boards, [0, 0, player, player], dice=[(0, 0), (2, 1), dice, dice])


def test_check_positions_shape_errors():
    with pytest.raises(ValueError):
        check_positions(np.zeros((0, 52), np.uint8), [])
    with pytest.raises(ValueError):
        check_positions(np.stack([POS_A, POS_B]), [0])


def test_plan_lanes_games_and_stride():
    """J = max(1, min(lanes // n_pos, trials)), G = ceil(trials / J), stratified:
    G rounded up until J * G is a multiple of 36."""
    assert plan(3, 72, 64, True) == (21, 12, 21)       # 21 * 4 = 84 >= 72 -> G = 4 -> 12 (252 = 7 * 36)
    assert plan(3, 72, 64, False) == (21, 4, 0)
    assert plan(1, 64 * 200, 64, True) == (64, 207, 64)
    assert plan(15, 36, 540, True) == (36, 1, 36)
    assert plan(100, 5, 64, False) == (1, 5, 0)        # more positions than lanes: one lane each
    for args in [(7, 100, 50, True), (1, 1, 8192, True), (600, 1296, 8192, True)]:
        J, G, stride = plan(*args)
        assert (J * G) % 36 == 0 and J * G >= args[1] and stride == J
        assert J * (G - 1) < args[1] or (J * (G - 1)) % 36
