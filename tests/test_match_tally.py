"""bgx.match on the CPU: the seat rule, the tally of hand-made headers, and
the new entry points' argument checks across the ABI (no device needed)."""
import ctypes

import numpy as np
import pytest

from bgx.match import net_of_player0, tally
from bgx.records import EP_WORDS


def _hdr(lane, ep, win_type, winner, n=10, steps=20):
    h = np.zeros(EP_WORDS, np.uint32)
    h[:6] = [lane, ep, 0, n, steps, win_type | (winner << 8)]
    return h


# (lane, episode, win type, winner) -> the network that won, its points
GAMES = [
    (0, 0, 1, 0),      # player 0 is network 0: network 0 wins a regular game
    (1, 0, 2, 0),      # odd lane: player 0 is network 1: network 1 wins a gammon
    (1, 1, 3, 1),      # odd lane, odd game: player 0 is network 0, so player 1 is network 1: a backgammon
    (2, 1, 1, 1),      # even lane, odd game: player 1 is network 0: a regular win
    (3, 0, 0, 0),      # unfinished (max_steps, win type 0): no points
    (5, 2, 2, 1),      # odd lane, even game: player 1 is network 0: a gammon
    (65537, 3, 3, 0),  # a global lane id past 16 bits: 65537 ^ 3 is even, player 0 is network 0
]
DIFF = np.array([1, -2, -3, 1, 0, 2, 3], np.float64)   # points of network 0 minus network 1, per game


def test_net_of_player0_both_seat_parities():
    assert net_of_player0(0, 0) == 0 and net_of_player0(1, 0) == 1
    assert net_of_player0(0, 1) == 1 and net_of_player0(1, 1) == 0
    lanes = np.arange(8, dtype=np.uint32)[:, None]
    eps = np.arange(6, dtype=np.uint32)[None, :]
    got = net_of_player0(lanes, eps)
    assert got.shape == (8, 6)
    assert np.array_equal(got, (lanes.astype(np.int64) + eps) % 2)
    # each network sits in PLAYER1's seat in half the games of every lane and of every round
    assert np.all(got.sum(0) == 4) and np.all(got.sum(1) == 3)


def test_tally_counts_win_types_points_and_unfinished():
    t = tally(np.stack([_hdr(*g) for g in GAMES]))
    assert t["games"] == 7 and t["unfinished"] == 1
    assert t["wins"][0] == {"regular": 2, "gammon": 1, "backgammon": 1}
    assert t["wins"][1] == {"regular": 0, "gammon": 1, "backgammon": 1}
    assert t["points"] == [1 + 1 + 2 + 3, 2 + 3]
    assert t["ppg"] == pytest.approx(DIFF.mean(), abs=1e-15)
    assert t["ppg_se"] == pytest.approx(DIFF.std(ddof=1) / np.sqrt(7), abs=1e-15)
    # int32 headers (as torch hands them over) give the same result
    assert tally(np.stack([_hdr(*g) for g in GAMES]).view(np.int32)) == t


def test_tally_is_mirrored_when_the_seats_swap():
    a = tally(np.stack([_hdr(*g) for g in GAMES]))
    b = tally(np.stack([_hdr(lane + 1, ep, wt, w) for lane, ep, wt, w in GAMES]))
    assert b["wins"] == a["wins"][::-1] and b["points"] == a["points"][::-1]
    assert b["ppg"] == -a["ppg"] and b["ppg_se"] == pytest.approx(a["ppg_se"])


def test_tally_of_an_empty_harvest_and_of_one_game():
    t = tally(np.zeros((0, EP_WORDS), np.uint32))
    zero = {"regular": 0, "gammon": 0, "backgammon": 0}
    assert t == {"games": 0, "wins": [zero, zero], "points": [0, 0], "unfinished": 0, "ppg": 0.0, "ppg_se": 0.0}
    t = tally(_hdr(1, 0, 2, 0)[None])
    assert t["games"] == 1 and t["ppg"] == -2.0 and t["ppg_se"] == 0.0


def test_new_entry_points_reject_null_handles_without_a_device():
    from bgx._lib import lib
    L = lib()   # (raises when libbgx.so is not built: there is no fallback)
    assert L.bgx_engine_set_opponent(None, None, None, None, None) == -1
    assert b"bgx_engine_set_opponent" in L.bgx_last_error()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.bgx_value_boards_routed(None, None, p, p, p, 1, p, None) == -1
    assert b"bgx_value_boards_routed" in L.bgx_last_error()
