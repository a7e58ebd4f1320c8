"""The fused 1-ply step reads its launch constants (FusedArgs / EngineDev, and
the MovegenArgs built from them) from the launch's kernarg segment at the head
of each queue item (csrc/bgx_fused.hip, launch_args) instead of keeping them
from the prologue. These tests run every item kind's loader at the smallest
shapes where it can go wrong: several workgroups, a ragged last one, both lane
widths, both launch modes, the workgroup tiers' workspace arguments, two
engines whose launches alternate, and constants that change between two
launches of one engine. Seed-0 weights; a shape is lanes / BGX_FUSED_LANES /
steps; every comparison is bit for bit.
"""
import numpy as np
import pytest

from test_gpu_engine import _by_episode, _same_runs

pytestmark = pytest.mark.gpu

CHUNK = 40
_RUNS = {}


def _make(weights, fused, lanes, seed=17, temperature=1.5, **kw):
    from bgx import Engine
    e = Engine(lanes=lanes, seed=seed, ply=1, fused=fused, **kw)
    assert bool(e.fused) == fused
    e.set_weights(weights, temperature=temperature, version=1)
    return e


def _chunk(e, hdrs, recs):
    """One launch of CHUNK steps and its harvest, appended to hdrs / recs."""
    from bgx.episodes import decode_records
    e.step(CHUNK)
    h = e.harvest()
    hdr = h.headers.cpu().numpy().view(np.uint32)
    hdrs.append(hdr)
    recs.append(decode_records(hdr, h.records))


def _run(weights, fused, lanes, steps, **kw):
    e = _make(weights, fused, lanes, **kw)
    hdrs, recs = [], []
    for _ in range(steps // CHUNK):
        _chunk(e, hdrs, recs)
    e.sync()
    st = e.stats()
    e.close()
    return _by_episode(hdrs, recs), st


def _shared(weights, monkeypatch, fused, lanes, fl, steps):
    """A lockstep run of a shape with no test hook set (once per shape, shared,
    left unchanged): the phased engine's (fl None) or the fused engine's."""
    key = (fused, lanes, fl, steps)
    if key not in _RUNS:
        monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
        if fl:
            monkeypatch.setenv("BGX_FUSED_LANES", fl)
        _RUNS[key] = _run(weights, fused, lanes, steps)
    return _RUNS[key]


def _same_where_both_finished(a, b, least):
    common = a.keys() & b.keys()
    assert len(common) >= 0.8 * min(len(a), len(b)) and len(common) > least
    for key in common:
        np.testing.assert_array_equal(a[key][0], b[key][0], err_msg=str(key))
        for f in a[key][1]:
            np.testing.assert_array_equal(a[key][1][f], b[key][1][f], err_msg=f"{key} {f}")


@pytest.mark.parametrize("lanes,fl,steps", [(37, "32", 120), (96, "32", 120), (48, "16", 120)])
def test_fused_matches_phased(weights_seed0, lanes, fl, steps, monkeypatch):
    """Lockstep launches: the fused engine's episodes and records are the
    phased engine's (every item kind read the right rows, slots, capacities,
    bias and scale)."""
    ref, _ = _shared(weights_seed0, monkeypatch, False, lanes, None, steps)
    run, st = _shared(weights_seed0, monkeypatch, True, lanes, fl, steps)
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * steps


def test_balanced_launch(weights_seed0, monkeypatch):
    """balance=True (the ticket code reads the budget, the step cap and the
    counter): every (lane, episode) that this run and the lockstep one both
    finished is identical."""
    lanes, fl, steps = 96, "32", 120
    ref, _ = _shared(weights_seed0, monkeypatch, True, lanes, fl, steps)
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    run, st = _run(weights_seed0, True, lanes, steps, balance=True)
    assert st["env_steps"] >= lanes * steps
    _same_where_both_finished(ref, run, 30)


@pytest.mark.parametrize("tier", ["2", "3"])
def test_forced_tiers(weights_seed0, tier, monkeypatch):
    """BGX_MG_TEST_TIER=2 / 3: every job is redone by the workgroup in the
    32 KB slice / in its global workspace (ws_global, ws_slots and the
    per-block workspace size come from the arguments), with the records of the
    unforced run."""
    lanes, fl, steps = 37, "32", 120
    ref, st_ref = _shared(weights_seed0, monkeypatch, True, lanes, fl, steps)
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    monkeypatch.setenv("BGX_MG_TEST_TIER", tier)
    run, st = _run(weights_seed0, True, lanes, steps)
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * steps
    assert st["fallback_jobs"] > st_ref["fallback_jobs"]


def test_two_engines_at_once(weights_seed0, monkeypatch):
    """Two fused engines alive in one process (one on the 32-lane kernel, one
    on the 16-lane kernel; other seed, temperature and max_legal), stepped
    alternately in launches of 40: each gives exactly the records of its solo
    run, so every launch read its own arguments."""
    monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
    steps = 120
    cfgs = [dict(lanes=37, fl="32", seed=17, temperature=1.5, max_legal=500),
            dict(lanes=48, fl="16", seed=29, temperature=0.6, max_legal=7)]
    solo = []
    for c in cfgs:
        monkeypatch.setenv("BGX_FUSED_LANES", c["fl"])
        solo.append(_run(weights_seed0, True, c["lanes"], steps, seed=c["seed"], temperature=c["temperature"],
                         max_legal=c["max_legal"])[0])
    engines, out = [], []
    for c in cfgs:
        monkeypatch.setenv("BGX_FUSED_LANES", c["fl"])   # read when the engine is created
        engines.append(_make(weights_seed0, True, c["lanes"], seed=c["seed"], temperature=c["temperature"],
                             max_legal=c["max_legal"]))
        out.append(([], []))
    for _ in range(steps // CHUNK):
        for e, (hdrs, recs) in zip(engines, out):
            _chunk(e, hdrs, recs)
    for e in engines:
        e.sync()
        e.close()
    for want, (hdrs, recs) in zip(solo, out):
        _same_runs(want, _by_episode(hdrs, recs))
    assert solo[0].keys() != solo[1].keys()


@pytest.mark.parametrize("lanes,fl", [(37, "32"), (48, "16")])
def test_constants_that_change_between_launches(weights_seed0, weights_ckpt, lanes, fl, monkeypatch):
    """One engine: 40 steps, then set_weights with the second golden weight
    set and another temperature (b2, the feature scale, the temperature and
    the fragment pointer change), then 40 more: equal to the phased engine
    driven the same way. Episodes end after 30 steps at the latest here, so
    every lane has finished an episode before the change and one across it."""
    monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    runs = []
    for fused in (False, True):
        e = _make(weights_seed0, fused, lanes, max_steps=30)
        hdrs, recs = [], []
        _chunk(e, hdrs, recs)
        e.set_weights(weights_ckpt, temperature=0.7, version=2)
        _chunk(e, hdrs, recs)
        e.sync()
        e.close()
        runs.append(_by_episode(hdrs, recs))
    _same_runs(*runs)
    assert len(runs[0]) >= 2 * lanes
