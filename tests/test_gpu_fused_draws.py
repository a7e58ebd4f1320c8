"""The fused 1-ply step draws a step's Philox numbers once per workgroup: the
last item of every step queue (the draw item, csrc/bgx_fused.hip) fills a
slot per lane with the next step's two draws, and the choice items read the
slots and evaluate Philox themselves only past them (SlotRng,
csrc/bgx_engine.h). These tests run the new code at the smallest shapes where
it can go wrong. Seed-0 weights, T = 1.5; a shape is lanes / BGX_FUSED_LANES /
steps; every comparison is bit for bit against the phased engine (or, where
said, against the fused engine's plain lockstep run); every harvest and the
final sync report no error flag (BGX_ERRF_WAIT_BOUND in particular: they
raise on any), and env_steps has the expected count.
"""
import numpy as np
import pytest

from test_gpu_engine import _by_episode, _same_runs

pytestmark = pytest.mark.gpu

_RUNS = {}


def _make(weights, fused, lanes, seed=17, temperature=1.5, **kw):
    from bgx import Engine
    e = Engine(lanes=lanes, seed=seed, ply=1, fused=fused, **kw)
    assert bool(e.fused) == fused
    e.set_weights(weights, temperature=temperature, version=1)
    return e


def _play(e, launches):
    """The launches (steps each) with a harvest behind each, then sync, stats
    and close: ({(lane, episode): (header, records)}, stats)."""
    from bgx.episodes import decode_records
    hdrs, recs = [], []
    for n in launches:
        e.step(n)
        h = e.harvest()           # raises on any error flag of the launch
        hdr = h.headers.cpu().numpy().view(np.uint32)
        hdrs.append(hdr)
        recs.append(decode_records(hdr, h.records))
    e.sync()                      # raises on any error flag left
    st = e.stats()
    e.close()
    return _by_episode(hdrs, recs), st


def _shared(weights, monkeypatch, fused, lanes, fl, launches=(40, 40, 40), **kw):
    """A lockstep run with no test hook set, made once per shape, shared and
    left unchanged: the phased engine's (fl None) or the fused engine's."""
    key = (fused, lanes, fl, tuple(launches), tuple(sorted(kw.items())))
    if key not in _RUNS:
        monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
        if fl:
            monkeypatch.setenv("BGX_FUSED_LANES", fl)
        _RUNS[key] = _play(_make(weights, fused, lanes, **kw), launches)
    return _RUNS[key]


@pytest.mark.parametrize("lanes,fl", [(37, "32"), (48, "16")])
def test_short_episodes(weights_seed0, lanes, fl, monkeypatch):
    """max_steps = 6: every lane is truncated and restarts every six steps, so
    the roll behind the truncation and new_game's loops (the draws past the
    slot) run all the time, and every restart leaves the counter somewhere
    else for the next draw item."""
    ref, st_ref = _shared(weights_seed0, monkeypatch, False, lanes, None, max_steps=6)
    run, st = _shared(weights_seed0, monkeypatch, True, lanes, fl, max_steps=6)
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * 120 == st_ref["env_steps"]
    assert st["episodes"] == st_ref["episodes"] >= lanes * 120 // 6
    assert len(run) >= lanes * 120 // 6


def test_single_step_launches(weights_seed0, monkeypatch):
    """37 lanes / 32: thirty launches of 1 step, then launches of 2, 7, 40 and
    41 steps (120 in all). Every launch's first step takes its draws from the
    draw item of step -1: in the first launch beside the first positions'
    expansion, in every later one alone in its queue (the expansion is carried
    over from the launch before). Equal to one phased run of 120 steps."""
    lanes = 37
    ref, _ = _shared(weights_seed0, monkeypatch, False, lanes, None)
    monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
    monkeypatch.setenv("BGX_FUSED_LANES", "32")
    run, st = _play(_make(weights_seed0, True, lanes), [1] * 30 + [2, 7, 40, 41])
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * 120


def test_passes_happen(weights_seed0, monkeypatch):
    """96 lanes / 32 / 120 steps (three workgroups), seed 17: some lanes pass
    (a pass rolls from the slot's first pair and takes no uniform), fused ==
    phased."""
    lanes = 96
    ref, _ = _shared(weights_seed0, monkeypatch, False, lanes, None)
    run, st = _shared(weights_seed0, monkeypatch, True, lanes, "32")
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * 120
    assert st["env_steps"] > st["decisions"] > 0


@pytest.mark.parametrize("fl", ["32", "16"])
def test_scripted_dice_and_greedy_play(weights_seed0, fl, monkeypatch):
    """Engine(greedy=True) with set_dice on 37 lanes: the counter is the table
    cursor and the slots are unused. Fused == phased while the table lasts; a
    table that ends reports BGX_ERRF_DICE_EXHAUSTED (0x20) alone, on both."""
    from bgx import BgxError
    lanes, steps = 37, 120
    monkeypatch.delenv("BGX_MG_TEST_TIER", raising=False)
    monkeypatch.setenv("BGX_FUSED_LANES", fl)
    rng = np.random.default_rng(5)
    dice = rng.integers(1, 7, (lanes, 2 * steps + 400), dtype=np.uint8)   # new_game's re-rolls included
    runs = []
    for fused in (False, True):
        e = _make(weights_seed0, fused, lanes, greedy=True)
        e.set_dice(dice)
        run, st = _play(e, [40, 40, 40])
        assert st["env_steps"] == lanes * steps
        runs.append(run)
    _same_runs(*runs)
    for fused in (False, True):
        e = _make(weights_seed0, fused, lanes, greedy=True)
        e.set_dice(np.tile(np.array([3, 1, 4, 2], np.uint8), (lanes, 2)))   # reset + 2 rolls per lane
        with pytest.raises(BgxError, match=r"flags 0x20\b"):
            e.step(5)
            e.harvest()
            e.sync()
        e.close()


@pytest.mark.parametrize("tier", ["2", "3"])
def test_forced_tiers(weights_seed0, tier, monkeypatch):
    """BGX_MG_TEST_TIER=2 / 3 at 37 lanes / 32: every job is redone by the
    workgroup tiers, which reuse the scratch and put their barriers between
    the draw item and the choices: the records of the unforced run."""
    lanes = 37
    ref, st_ref = _shared(weights_seed0, monkeypatch, True, lanes, "32")
    monkeypatch.setenv("BGX_FUSED_LANES", "32")
    monkeypatch.setenv("BGX_MG_TEST_TIER", tier)
    run, st = _play(_make(weights_seed0, True, lanes), [40, 40, 40])
    _same_runs(ref, run)
    assert st["env_steps"] == lanes * 120
    assert st["fallback_jobs"] > st_ref["fallback_jobs"]


def test_balanced_launch(weights_seed0, monkeypatch):
    """96 lanes / 32, balance=True (a refused ticket ends the launch behind a
    draw item whose slots the next launch's step -1 draws again): every (lane,
    episode) that this run and the lockstep one both finished is identical."""
    lanes = 96
    ref, _ = _shared(weights_seed0, monkeypatch, True, lanes, "32")
    monkeypatch.setenv("BGX_FUSED_LANES", "32")
    run, st = _play(_make(weights_seed0, True, lanes, balance=True), [40, 40, 40])
    assert st["env_steps"] >= lanes * 120
    common = ref.keys() & run.keys()
    assert len(common) >= 0.8 * min(len(ref), len(run)) and len(common) > 30
    for key in common:
        np.testing.assert_array_equal(ref[key][0], run[key][0], err_msg=str(key))
        for f in ref[key][1]:
            np.testing.assert_array_equal(ref[key][1][f], run[key][1][f], err_msg=f"{key} {f}")
