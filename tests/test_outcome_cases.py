"""CPU checks of the constructed outcome positions (tests/outcome_cases.py):
the enumerated fixture boards are inside the board domain; every start
position is accepted by bgx.rollout.check_positions, the oracle confirms that
it is pure (every legal afterstate under its roll falls in its cell, with the
cell's outcome), every required cell has one for either player; and the
scripted lines are pure at every step."""
import numpy as np
import pytest

import outcome_cases as oc

REQUIRED = ["regular_loser_on_bar", "gammon_first_point_outside", "backgammon_bar_only", "backgammon_home_edge_18",
            "backgammon_home_edge_23", "close_out", "open_five_points_bar", "open_home_made_bar_empty",
            "prime5_first_behind", "prime6_first_behind", "prime7_first_behind", "run_at_edge",
            "run_opponent_ahead_or_bar"]


def test_fixture_boards_are_in_the_board_domain():
    from test_abi import _host_check
    boards, player, mover_row = oc.fixture_rows()
    assert _host_check(boards, player) == (0, -1)
    assert len(boards) == 2 * len(oc.fixture_cases()) and mover_row.sum() * 2 == len(boards)
    assert set(player[mover_row].tolist()) == {0, 1}
    # player 1's boards are player 0's mirrored
    cs = oc.fixture_cases()
    for (c0, b0, p0), (c1, b1, p1) in zip(cs[0::2], cs[1::2]):
        assert (c0, p0, p1) == (c1, 0, 1)
        np.testing.assert_array_equal(oc.mirror(b0), b1)


def test_positions_are_accepted_by_check_positions():
    from bgx.rollout import check_positions
    ps = oc.positions()
    assert len(ps) <= 64
    b, p, d = check_positions(np.stack([x[1] for x in ps]), [x[2] for x in ps], [x[3] for x in ps])
    assert d.min() >= 1 and d.max() <= 6
    from test_abi import _host_check
    assert _host_check(b, p, d) == (0, -1)
    for line in oc.sequences().values():
        check_positions(line["board"], [line["player"]], [line["first"]])
        assert all(1 <= x <= 6 for r in line["script"] for x in r) and len(line["script"]) == line["steps"]


def test_every_position_is_pure_and_every_cell_is_there():
    orc = pytest.importorskip("oracle")
    seen = set()
    for cell, board, pl, roll in oc.positions():
        assert oc.is_pure(orc, cell, board, pl, roll), (cell, pl)
        assert len(oc.afterstates(orc, board, pl, roll)) >= 1
        seen.add((cell, pl))
    assert seen == {(c, pl) for c in REQUIRED for pl in (0, 1)}
    assert list(oc.CELLS) == REQUIRED
    # the cells differ where the rules do: the input conditions, stated on the boards
    by = {(c, pl): (b, r) for c, b, pl, r in oc.positions()}
    for pl in (0, 1):
        f = oc.features(by[("regular_loser_on_bar", pl)][0], pl)
        assert f["off_o"] == 1 and f["bar_o"] == 1 and f["off_m"] == 14
        f = oc.features(by[("gammon_first_point_outside", pl)][0], pl)
        assert f["theirs"][17] > 0 and f["theirs"][18:].sum() == 0 and f["bar_o"] == 0 and f["off_o"] == 0
        f = oc.features(by[("backgammon_bar_only", pl)][0], pl)
        assert f["theirs"][18:].sum() == 0 and f["bar_o"] > 0 and f["off_o"] == 0
        for pt in (18, 23):
            f = oc.features(by[(f"backgammon_home_edge_{pt}", pl)][0], pl)
            home = f["theirs"][18:]
            assert home[pt - 18] > 0 and home.sum() == home[pt - 18] and f["bar_o"] == 0 and f["off_o"] == 0
        for n in (5, 6, 7):
            f = oc.features(by[(f"prime{n}_first_behind", pl)][0], pl)
            assert f["run_len"] == n and f["first_behind"] and not f["far_behind"] and f["run_end"] < 23
        f = oc.features(by[("run_at_edge", pl)][0], pl)
        assert f["run_len"] >= 5 and f["run_end"] == 23


def test_an_impure_position_is_rejected():
    """is_pure is not vacuous: the close-out position under 2-1 (a home checker
    may move and open a point) and a prime position with the opponent's
    checkers taken from behind the run both fail."""
    orc = pytest.importorskip("oracle")
    by = {(c, pl): (b, r) for c, b, pl, r in oc.positions()}
    b, r = by[("close_out", 0)]
    assert oc.is_pure(orc, "close_out", b, 0, r) and not oc.is_pure(orc, "close_out", b, 0, (2, 1))
    b, r = by[("prime5_first_behind", 0)]
    c = b.copy()
    c[51] += c[24 + 23]
    c[24 + 23] = 0
    assert not oc.is_pure(orc, "prime5_first_behind", c, 0, r)
    assert oc.is_pure(orc, "run_opponent_ahead_or_bar", c, 0, r)


def test_scripted_lines_are_pure_at_every_step():
    orc = pytest.importorskip("oracle")
    lines = oc.sequences()
    assert set(lines) == {f"{k}_p{pl}" for k in ("close_out", "prime", "both") for pl in (0, 1)}
    for name, line in lines.items():
        steps = oc.walk(orc, line)
        assert all(len(s) == 1 for s in steps), (name, steps)
        flags, recs = 0, []
        for s in steps:
            (kind,) = s
            if kind == "pass":
                continue
            pl, closed, prime, over = kind
            assert not over
            co = closed and not (flags >> pl) & 1
            pr = prime and not (flags >> (2 + pl)) & 1
            flags |= (co << pl) | (pr << (2 + pl)) | (16 << pl)
            r = oc.F32(0.0)
            if co:
                r = oc.F32(r + oc.F32(0.30))
            if pr:
                r = oc.F32(r + oc.F32(0.20))
            recs.append((pl, int(co), int(pr), r))
        assert recs == line["records"], (name, recs)
        assert flags == line["flags"], (name, flags)
    # the lines hold what they are for: a predicate true again after its reward was given
    for pl in (0, 1):
        assert [r[1] for r in lines[f"close_out_p{pl}"]["records"]] == [1, 0]
        assert [r[2] for r in lines[f"prime_p{pl}"]["records"] if r[0] == pl] == [1, 0]
        assert sorted((r[0], r[2]) for r in lines[f"both_p{pl}"]["records"]) == [(0, 1), (1, 1)]
