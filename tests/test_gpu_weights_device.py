"""bgx_set_weights_device on the GPU: the device-built network equals the host
path's byte for byte (Engine.peek("net_frag"): fragments, feature scale, b2)
on fused and phased engines, plays the same games, rejects what the host path
rejects with its message and leaves the previous network, and orders itself
behind a queued step from another stream."""
import numpy as np
import pytest
import torch

import value_cases as vc
from test_cpuwave_pack import B1, B2, N_W1, W2, accepted_sets

pytestmark = pytest.mark.gpu

PEEK_SETS = ("seed0", "ckpt", "all_zero", "clamp_hi", "clamp_lo", "lo_subnormal", "cols_193_195", "under_193", "tiny")
ENGINES = {"fused16": dict(lanes=64, ply=1, fused=True, _fl="16"), "fused32": dict(lanes=64, ply=1, fused=True, _fl="32"),
           "phased": dict(lanes=64, ply=1, fused=False)}


def _dict(flat):
    flat = np.asarray(flat, np.float32)
    return {"W1": flat[:N_W1].reshape(128, 198).copy(), "b1": flat[B1:W2].copy(), "w2": flat[W2:B2].copy(),
            "b2": flat[B2:].copy()}


def _flat(w):
    return np.concatenate([np.asarray(w[k], np.float32).ravel() for k in ("W1", "b1", "w2", "b2")])


def _make(monkeypatch, kw):
    from bgx import Engine
    kw = dict(kw)
    fl = kw.pop("_fl", None)
    if fl is not None:
        monkeypatch.setenv("BGX_FUSED_LANES", fl)   # read when the engine is created
    else:
        monkeypatch.delenv("BGX_FUSED_LANES", raising=False)
    return Engine(seed=3, **kw)


@pytest.mark.parametrize("kind", list(ENGINES))
def test_device_packed_network_equals_host_packed(monkeypatch, kind):
    sets = accepted_sets()
    host, dev = _make(monkeypatch, ENGINES[kind]), _make(monkeypatch, ENGINES[kind])
    try:
        for k, name in enumerate(PEEK_SETS):
            flat, e = sets[name]
            host.set_weights(_dict(flat), temperature=1.5, version=k + 1)
            # (the first hand-off also creates the engine's network)
            dev.set_weights_device(torch.from_numpy(flat).cuda(), temperature=1.5, version=k + 1)
            a, b = host.peek("net_frag"), dev.peek("net_frag")
            assert a.shape == b.shape == (6656 * 16 + 8,)
            assert np.array_equal(a, b), (kind, name)
            scale, b2 = b[-8:].view(np.float32)
            assert scale == np.float32(2.0 ** -e) and b2 == np.float32(flat[B2]), (kind, name)
    finally:
        host.close()
        dev.close()


def _keyed(harvest):
    """{(lane, episode): (header bytes, record bytes)}"""
    hdr = harvest.headers.cpu().numpy().view(np.uint32)
    rec = harvest.records.cpu().numpy().view(np.uint32)
    offs = np.concatenate([[0], np.cumsum(hdr[:, 3].astype(np.int64))])
    return {(int(h[0]), int(h[1])): (h.tobytes(), rec[offs[i]:offs[i + 1]].tobytes()) for i, h in enumerate(hdr)}


def _play(e, first, second, device_path, side_stream=False):
    """Two launches of 6 steps, the weights changed in between; the games end at
    max_steps = 10, so every lane finishes one game that saw both networks."""
    lanes = e.lanes
    rng = np.random.default_rng(5)
    e.set_weights(_dict(first), temperature=1.5, version=1)
    e.set_dice(rng.integers(1, 7, size=(lanes, 160), dtype=np.uint8))
    s = torch.cuda.current_stream()
    p = torch.from_numpy(second).cuda() if device_path else None   # (uploaded before anything is queued)
    torch.cuda.synchronize()
    e.step(6, stream=s)
    if device_path:
        if side_stream:   # the step above is still queued or running on s
            side = torch.cuda.Stream()
            e.set_weights_device(p, temperature=0.9, version=2, stream=side)
        else:
            e.set_weights_device(p, temperature=0.9, version=2, stream=s)
    else:
        e.set_weights(_dict(second), temperature=0.9, version=2)
    e.step(6, stream=s)
    out = _keyed(e.harvest(stream=s))
    e.sync()
    return out


PLAY = {"fused 1-ply": dict(ply=1, fused=True), "phased 1-ply": dict(ply=1, fused=False), "ply 2": dict(ply=2, k_top=4)}


@pytest.mark.parametrize("kind", list(PLAY))
def test_same_records_through_host_and_device_path(kind):
    from bgx import Engine
    w = vc.weight_sets()
    first, second = _flat(w["seed0"]), _flat(w["ckpt"])   # e, the feature scale and b2 all change
    got = []
    for device_path in (False, True):
        e = Engine(lanes=64, seed=9, greedy=True, max_steps=10, **PLAY[kind])
        try:
            got.append(_play(e, first, second, device_path))
        finally:
            e.close()
    assert len(got[0]) >= 64 and set(k[0] for k in got[0]) == set(range(64))
    assert got[0].keys() == got[1].keys()
    for k in got[0]:
        assert got[0][k] == got[1][k], (kind, k)
    # the change mattered: the same games on the first network alone differ
    e = Engine(lanes=64, seed=9, greedy=True, max_steps=10, **PLAY[kind])
    try:
        same = _play(e, first, first, False)
    finally:
        e.close()
    assert any(same.get(k) != got[0][k] for k in got[0])


@pytest.mark.parametrize("fused", [True, False])
def test_side_stream_handoff_waits_for_the_queued_step(fused):
    from bgx import Engine
    w = vc.weight_sets()
    first, second = _flat(w["seed0"]), _flat(w["ckpt"])
    got = []
    for side in (False, True):
        e = Engine(lanes=64, seed=9, greedy=True, max_steps=10, ply=1, fused=fused)
        try:
            got.append(_play(e, first, second, True, side_stream=side))
        finally:
            e.close()
    assert len(got[0]) >= 64 and got[0] == got[1]


@pytest.mark.parametrize("where", [("W1", 77 * 198 + 12, "W1[15258]"), ("b1", B1 + 5, "b1[5]"), ("w2", W2 + 127, "w2[127]"),
                                   ("b2", B2, "b2[0]")])
def test_nan_is_rejected_by_name_and_the_network_stays(where):
    from bgx import BgxError, Engine
    _, index, text = where
    flat = _flat(vc.weight_sets()["ckpt"])
    e = Engine(lanes=64, seed=1, ply=1)
    try:
        e.set_weights_device(torch.from_numpy(flat).cuda(), temperature=1.5, version=1)
        before = e.peek("net_frag")
        bad = flat.copy()
        bad[index] = np.nan
        bad[index + 1:index + 2] = np.inf   # a later one is not the one named
        with pytest.raises(BgxError, match=r"\(-1\).*" + text.replace("[", r"\[").replace("]", r"\]") + " is not finite"):
            e.set_weights_device(torch.from_numpy(bad).cuda(), temperature=0.7, version=2)
        assert np.array_equal(e.peek("net_frag"), before)
        assert e.version == 1 and e.temperature == 1.5
        big = flat.copy()
        big[B1 + 3] = -1e9
        with pytest.raises(BgxError, match=r"b1\[3\] = -1e\+09: max\|log2\(e\) w\| must stay below 2\^26"):
            e.set_weights_device(torch.from_numpy(big).cuda(), temperature=0.7, version=2)
        assert np.array_equal(e.peek("net_frag"), before)
        e.step(4)   # and the engine still plays
        e.sync()
        assert e.stats()["env_steps"] == 64 * 4
    finally:
        e.close()


def test_rejected_first_handoff_leaves_no_network():
    from bgx import BgxError, Engine
    flat = _flat(vc.weight_sets()["ckpt"])
    flat[100] = np.inf
    e = Engine(lanes=64, seed=1, ply=1)
    try:
        with pytest.raises(BgxError, match=r"W1\[100\] is not finite"):
            e.set_weights_device(torch.from_numpy(flat).cuda())
        with pytest.raises(BgxError, match="no network"):
            e.peek("net_frag")
        with pytest.raises(BgxError, match="bgx_set_weights first"):
            e.step(1)
    finally:
        e.close()
