"""The fused 1-ply step with two rule-mode non-doubles jobs per wave
(BGX_FUSED_PAIR, csrc/bgx_fused.hip + job_records_pair in csrc/bgx_movegen.h)
at the smallest shapes where pairing can go wrong: several workgroups, a ragged
last one, both lane widths, both launch modes. Seed-0 weights; a shape is
lanes / BGX_FUSED_LANES / steps.
"""
import re

import numpy as np
import pytest

from test_gpu_engine import _by_episode, _collect, _engine, _same_runs

pytestmark = pytest.mark.gpu

_PHASED = {}


def _phased(weights, lanes, steps):
    """The phased engine's run of a shape (once per shape, shared, left unchanged)."""
    if (lanes, steps) not in _PHASED:
        ref = _engine(weights, lanes=lanes, seed=17, ply=1, fused=False)
        _PHASED[(lanes, steps)] = _by_episode(*_collect(ref, steps, chunk=40))
        ref.close()
    return _PHASED[(lanes, steps)]


def _fused(weights, monkeypatch, lanes, fl, steps, pair, seed=17, **kw):
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    monkeypatch.setenv("BGX_FUSED_PAIR", pair)
    e = _engine(weights, lanes=lanes, seed=seed, ply=1, fused=True, **kw)
    assert e.fused
    run = _by_episode(*_collect(e, steps, chunk=40))
    st = e.stats()
    e.close()
    return run, st


@pytest.mark.parametrize("lanes,fl,steps", [(48, "16", 120), (37, "32", 120), (96, "32", 120)])
def test_paired_step_matches_unpaired_and_phased(weights_seed0, lanes, fl, steps, monkeypatch):
    """Lockstep launches: BGX_FUSED_PAIR=1 gives the episodes and records of
    BGX_FUSED_PAIR=0 and of the phased engine (same afterstates in the same
    order, V with the same bits, same samples), and sends the same jobs to the
    workgroup tiers."""
    on, st_on = _fused(weights_seed0, monkeypatch, lanes, fl, steps, "1")
    off, st_off = _fused(weights_seed0, monkeypatch, lanes, fl, steps, "0")
    _same_runs(off, on)
    _same_runs(_phased(weights_seed0, lanes, steps), on)
    assert st_on["env_steps"] == st_off["env_steps"] == lanes * steps
    assert st_on["fallback_jobs"] == st_off["fallback_jobs"]


def test_paired_step_balanced_launch(weights_seed0, monkeypatch):
    """balance=True: every (lane, episode) both runs finished has identical
    records with the switch on and off."""
    lanes, fl, steps = 96, "32", 120
    a, _ = _fused(weights_seed0, monkeypatch, lanes, fl, steps, "0", seed=23, balance=True)
    b, _ = _fused(weights_seed0, monkeypatch, lanes, fl, steps, "1", seed=23, balance=True)
    common = a.keys() & b.keys()
    assert len(common) >= 0.8 * min(len(a), len(b)) and len(common) > 30
    for key in common:
        np.testing.assert_array_equal(a[key][0], b[key][0], err_msg=str(key))
        for f in a[key][1]:
            np.testing.assert_array_equal(a[key][1][f], b[key][1][f], err_msg=f"{key} {f}")


def test_pairs_are_formed(weights_seed0, monkeypatch, capfd):
    """The development report (BGX_FUSED_PROF=1, printed when the engine is
    closed) counts the pair items: more than none, so the tests above compare
    runs that did pair."""
    monkeypatch.setenv("BGX_FUSED_PROF", "1")
    _fused(weights_seed0, monkeypatch, 96, "32", 120, "1")
    err = capfd.readouterr().err
    m = re.search(r"tier-1 pair items: (\d+) pairs formed", err)
    assert m, err[-2000:]
    assert int(m.group(1)) > 0
