"""CPU checks of the shared value-network cases (tests/value_cases.py): the
edge boards are inside the board domain and encode as get_board_features
states; every weight set lands on the scaling exponent it is meant to test."""
import numpy as np
import pytest

import value_cases as vc


def test_edge_boards_are_in_the_board_domain():
    from test_abi import _host_check
    boards, player = vc.edge_boards()
    assert boards.shape[1] == 52 and len(boards) == len(player) == 2 * (2 * 12 * 136 + 2 * 32 + 2 * 24)
    assert _host_check(boards, player) == (0, -1)
    assert set(np.unique(player)) == {0, 1}
    # every count 0..15 in both nibbles of every packed point byte, and on the bars / off fields
    for j in range(24):
        for nib in (0, 1):
            assert set(np.unique(boards[:, 2 * j + nib])) == set(range(16)), (j, nib)
    for f in range(48, 52):
        assert set(np.unique(boards[:, f])) == set(range(16)), f
    # every byte value a legal board can hold (lo + hi <= 15) in every packed byte
    for j in range(24):
        pairs = set(zip(boards[:, 2 * j].tolist(), boards[:, 2 * j + 1].tolist()))
        assert {(a, c) for a in range(16) for c in range(16 - a)} <= pairs, j


def test_edge_boards_encode_as_get_board_features():
    orc = pytest.importorskip("oracle")
    boards, player = vc.edge_boards()
    np.testing.assert_array_equal(orc.encode_many(boards, player).view(np.uint32),
                                  vc.features_numpy(boards, player).view(np.uint32))
    b, p = vc.edge_sample(96)
    assert len(b) == 96 and set(np.unique(p)) == {0, 1}


def test_weight_sets_reach_the_intended_exponents():
    sets = vc.weight_sets()
    assert set(sets) == set(vc.INTENDED_E)
    for name, w in sets.items():
        assert w["W1"].shape == (128, 198) and w["W1"].dtype == np.float32
        assert all(np.isfinite(w[k]).all() for k in w), name
        assert vc.expected_e(w) == vc.INTENDED_E[name], (name, vc.expected_e(w), vc.scaled_max(w))
        assert vc.scaled_max(w) < vc.MAX_SCALED, name
    assert 2.0 ** 25 <= vc.scaled_max(sets["clamp_lo"]) < 2.0 ** 26
    assert {vc.INTENDED_E[f"ckpt_x2^{k}"] for k in vc.CKPT_K} == {13, 8, 5, 1, -3, -9}
    t = sets["tiny"]
    tiny = np.finfo(np.float32).tiny
    assert ((t["W1"] != 0) & (np.abs(t["W1"]) < tiny)).sum() >= 4 and np.signbit(t["W1"][t["W1"] == 0]).all()


def test_closed_forms_agree_with_the_oracle():
    orc = pytest.importorskip("oracle")
    b, p = vc.edge_sample(64)
    x = orc.encode_many(b, p)
    sets = vc.weight_sets()
    for name in vc.CLOSED_FORM:
        v = orc.value(sets[name], x)
        assert np.abs(v - vc.closed_form(name, sets[name])).max() < 1e-12, name
        assert np.abs(vc.value_f32(sets[name], x) - v).max() < 1e-5
