"""The fused 1-ply step hands a stepped lane's next tier-1 job to a wave from
per-step LDS bitmasks (csrc/bgx_claim.h, csrc/bgx_fused.hip): which wave
expands a lane, and whether two lanes share a wave, changes no result. These
tests run the claim at the smallest shapes where it can go wrong: a ragged
last workgroup, several workgroups, both lane widths, pairing on and off, every
job redone by the workgroup tier, and the balanced launch. Seed-0 weights, 120
steps in launches of 40; a shape is lanes / BGX_FUSED_LANES. Every harvest and
the final sync raise on any error flag (BGX_ERRF_WAIT_BOUND among them), so a
run that returns raised none.
"""
import numpy as np
import pytest

from test_gpu_engine import _by_episode, _collect, _engine, _same_runs

pytestmark = pytest.mark.gpu

STEPS = 120
_RUNS = {}


def _phased(weights, lanes):
    """The phased engine's run of a shape (once per shape, shared, left unchanged)."""
    key = ("phased", lanes)
    if key not in _RUNS:
        ref = _engine(weights, lanes=lanes, seed=17, ply=1, fused=False)
        _RUNS[key] = _by_episode(*_collect(ref, STEPS, chunk=40))
        ref.close()
    return _RUNS[key]


def _fused(weights, monkeypatch, lanes, fl, pair=None, tier=None, seed=17, **kw):
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    for name, val in (("BGX_FUSED_PAIR", pair), ("BGX_MG_TEST_TIER", tier)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    e = _engine(weights, lanes=lanes, seed=seed, ply=1, fused=True, **kw)
    assert e.fused
    run = _by_episode(*_collect(e, STEPS, chunk=40))   # harvest and sync raise on any error flag
    st = e.stats()
    e.close()
    return run, st


def _plain(weights, monkeypatch, lanes, fl):
    """The fused lockstep run of a shape with no hook set (once per shape, shared)."""
    key = ("fused", lanes, fl)
    if key not in _RUNS:
        _RUNS[key] = _fused(weights, monkeypatch, lanes, fl)
    return _RUNS[key]


@pytest.mark.parametrize("lanes,fl", [(48, "16"), (37, "32"), (96, "32")])
def test_lockstep_matches_phased(weights_seed0, lanes, fl, monkeypatch):
    """Lockstep launches: the episodes and records of the phased engine, every
    lane stepped every step, no error flag."""
    run, st = _plain(weights_seed0, monkeypatch, lanes, fl)
    _same_runs(_phased(weights_seed0, lanes), run)
    assert st["env_steps"] == lanes * STEPS


def test_pairing_on_and_off(weights_seed0, monkeypatch):
    """96 / 32: BGX_FUSED_PAIR=0 and =1 give identical output and send the same
    jobs to the workgroup tiers."""
    off, st_off = _fused(weights_seed0, monkeypatch, 96, "32", pair="0")
    on, st_on = _fused(weights_seed0, monkeypatch, 96, "32", pair="1")
    _same_runs(off, on)
    _same_runs(_phased(weights_seed0, 96), on)
    assert st_on["env_steps"] == st_off["env_steps"] == 96 * STEPS
    assert st_on["fallback_jobs"] == st_off["fallback_jobs"]


def test_every_job_redone_by_the_workgroup_tier(weights_seed0, monkeypatch):
    """96 / 32 with BGX_MG_TEST_TIER=2: every job is claimed, skipped by its
    wave and redone by the workgroup; the output of the untiered run."""
    plain, _ = _plain(weights_seed0, monkeypatch, 96, "32")
    tiered, st = _fused(weights_seed0, monkeypatch, 96, "32", tier="2")
    _same_runs(plain, tiered)
    assert st["env_steps"] == 96 * STEPS
    assert st["fallback_jobs"] > 0


def test_balanced_launch(weights_seed0, monkeypatch):
    """96 / 32 with balance=True (workgroups stop at different steps): every
    (lane, episode) both the fused and the phased run finished has identical
    records."""
    ref = _engine(weights_seed0, lanes=96, seed=23, ply=1, fused=False)
    a = _by_episode(*_collect(ref, STEPS, chunk=40))
    ref.close()
    b, _ = _fused(weights_seed0, monkeypatch, 96, "32", seed=23, balance=True)
    common = a.keys() & b.keys()
    assert len(common) >= 0.8 * min(len(a), len(b)) and len(common) > 30
    for key in common:
        np.testing.assert_array_equal(a[key][0], b[key][0], err_msg=str(key))
        for f in a[key][1]:
            np.testing.assert_array_equal(a[key][1][f], b[key][1][f], err_msg=f"{key} {f}")
