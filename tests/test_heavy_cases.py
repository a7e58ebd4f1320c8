"""CPU checks of the heavy movegen positions (tests/heavy_cases.py): every
board is inside the board domain, the oracle puts each member in the count
class it is listed under, no list exceeds the record field's clamp, and a
root's replies over the 21 rolls fit the rows bgx_two_ply allocates per root."""
import numpy as np
import pytest

import heavy_cases as hc

TWO_PLY_ROWS_PER_ROOT = 21 * 768   # bgx_abi.cpp bgx_two_ply_sampled: cap = jobs * 768, jobs = 21 per root


@pytest.fixture(scope="module")
def sums():
    orc = pytest.importorskip("oracle")
    return {name: (b, pl, hc.counts(orc, b, pl), hc.summary(orc, b, pl)) for name, b, pl in hc.cases()}


def test_heavy_boards_are_in_the_board_domain():
    from test_abi import _host_check
    cs = hc.cases()
    assert [c[0] for c in cs] == list(hc.CLASSES)
    boards = np.stack([c[1] for c in cs for _ in hc.ROLLS36])
    player = np.array([c[2] for c in cs for _ in hc.ROLLS36], np.uint8)
    dice = np.array([r for _ in cs for r in hc.ROLLS36], np.uint8)
    assert _host_check(boards, player, dice) == (0, -1)
    assert {c[2] for c in cs} == {0, 1}
    # reachable positions: 15 checkers a side
    for _, b, _pl in cs:
        assert int(b[0:24].sum()) + int(b[48]) + int(b[50]) == 15
        assert int(b[24:48].sum()) + int(b[49]) + int(b[51]) == 15


def test_mirror_gives_the_mirrored_lists():
    orc = pytest.importorskip("oracle")
    b0, p0 = hc.cases_by_name("spread_p0")
    b1, p1 = hc.mirror(b0, p0)
    assert p1 == 1 and np.array_equal(hc.mirror(b1, p1)[0], b0)
    got = dict((n, b) for n, b, _ in hc.cases())["spread_p1"]
    np.testing.assert_array_equal(got, b1)
    for a, c in hc.ROLLS36:
        n0, r0, _ = orc.movegen(b0, p0, a, c)
        n1, r1, _ = orc.movegen(b1, p1, a, c)
        assert n0 == n1, (a, c, n0, n1)
        # the same boards; their order is not mirrored (the reference scans the
        # points by index for either player), it is pinned by movegen_heavy.npz
        m0 = sorted(hc.mirror(r, 0)[0].tobytes() for r in r0)
        assert m0 == sorted(r.tobytes() for r in r1), (a, c)
        assert len(set(m0)) == n0


def test_oracle_counts_match_each_members_class(sums):
    for name, (b, pl, c, s) in sums.items():
        cls = hc.CLASSES[name]
        if cls == "over_t2":
            assert s["dbl"] > hc.T2_PARENTS, (name, s)
        elif cls == "edge_t2":
            assert hc.T2_FRONTIER < s["dbl"] <= hc.T2_PARENTS, (name, s)
        elif cls == "tier2":
            assert hc.T1_LIST < s["dbl"] <= hc.T2_FRONTIER, (name, s)
        elif cls == "nd_max":
            assert s["nd"] > hc.FUSED_ND, (name, s)
            assert s["nd"] == max(v["nd"] for _, _, _, v in sums.values()) == 220
        elif cls == "bearoff":
            home = b[18:24] if pl == 0 else b[24:30]
            assert int(home.sum()) + int(b[50 + pl]) == 15 and b[50 + pl] >= 3 and b[48 + pl] == 0
            assert max(c.values()) >= 64, (name, s)
        elif cls == "bar":
            assert b[48 + pl] >= 1 and max(c.values()) >= 200, (name, s)
        else:
            raise AssertionError(cls)
    for name in hc.HITS:
        b, pl, c, s = sums[name]
        assert hc.blots_ahead(b, pl) >= 4 and s["dbl"] > hc.T1_LIST, (name, s)
    assert sum(1 for n in sums if hc.CLASSES[n] == "tier2") >= 2
    # the pinned counts of the spread board
    c = sums["spread_p0"][2]
    assert [c[(d, d)] for d in range(1, 7)] == [2140, 2027, 1225, 1079, 1044, 621] and c[(1, 2)] == 209
    assert set(hc.EMU_SUBSET) <= set(sums)


def test_counts_fit_the_record_field_and_the_two_ply_rows(sums):
    worst = 0
    for name, (b, pl, c, s) in sums.items():
        assert max(c.values()) <= hc.RECORD_CLAMP, (name, max(c.values()))
        print(f"{name}: largest list {max(c.values())}, replies over the 21 rolls {s['total21']}")
        worst = max(worst, s["total21"])
        assert s["total21"] <= TWO_PLY_ROWS_PER_ROOT, (name, s)
    print(f"largest per-root total {worst} of {TWO_PLY_ROWS_PER_ROOT} rows")
    # per job the figure 768 does not hold: that is why the bound is stated for the total
    assert max(max(c.values()) for _, _, c, _ in sums.values()) > 768
