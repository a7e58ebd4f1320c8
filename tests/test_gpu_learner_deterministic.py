"""Learner(deterministic=True) on the GPU, at the lanes and chunk size of
test_gpu_learner.py: two runs of one seed agree in the trainer's digest after
every update; every ticket the trainer reads is in strictly ascending (lane,
episode) order; a second trainer fed the raw ticket sorted on the host with
numpy matches the learner bit for bit after every update (the learner trains on
exactly the canonical order); the errors; the command line."""
import json

import numpy as np
import pytest

from test_cpuwave_canon import canonical

pytestmark = pytest.mark.gpu

MODES = {"plain": {}, "lam_zero_sum_afterstates": dict(lam=0.7, zero_sum=True, afterstates=True)}


def _keys(headers):
    h = headers.cpu().numpy().view(np.uint32)
    return (h[:, 0].astype(np.int64) << 32) | h[:, 1].astype(np.int64)


def _run(mode):
    from bgx.learner import Learner
    digests, tickets = [], []
    state = {}

    def on_update(info):
        digests.append(state["ln"].digest())
        tickets.append((info["ticket"], _keys(info["headers"]), int(info["records"].shape[0])))

    ln = Learner(256, 64, seed=0, deterministic=True, on_update=on_update, **MODES[mode])
    try:
        state["ln"] = ln
        ln.run(chunks=8)
        ln.sync()
        assert ln.gpu_ms["canon"] > 0 and ln.gpu_ms["update"] > 0
        return digests, tickets, ln.digest()
    finally:
        ln.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_two_runs_of_one_seed_agree_after_every_update(mode):
    d1, t1, end1 = _run(mode)
    d2, t2, end2 = _run(mode)
    print(mode, d1)
    assert len(d1) >= 2 and len(d1) == len(d2)
    for k, (a, b) in enumerate(zip(d1, d2)):
        assert a == b, k
    assert end1 == end2 == d1[-1]
    assert len(set(d1)) == len(d1)   # every update moved the parameters
    for (ta, ka, ma), (tb, kb, mb) in zip(t1, t2):
        assert ta == tb and ma == mb and np.array_equal(ka, kb)
        assert len(ka) >= 1 and (np.diff(ka) > 0).all(), ta   # strictly ascending (lane, episode)


@pytest.mark.parametrize("mode", list(MODES))
def test_learner_trains_on_the_host_sorted_ticket(mode):
    import torch
    from bgx.learner import Learner
    from bgx.trainer import DeviceTrainer
    state, seen = {}, []

    def on_update(info):
        ref = state["ref"]
        hdr = info["raw_headers"].clone().cpu().numpy().view(np.uint32)
        rec = info["raw_records"].clone().cpu().numpy().view(np.uint32)
        h, r, _ = canonical(hdr, rec)
        # what the learner handed its trainer is that order ...
        assert info["headers"].cpu().numpy().tobytes() == h.tobytes()
        assert info["records"].cpu().numpy().tobytes() == r.tobytes()
        # ... and the replay through the host on it leaves the same bits
        ref.update_records(torch.from_numpy(h.view(np.int32)), torch.from_numpy(r.view(np.int32)))
        mine, theirs = state["ln"].trainer._flat, ref._flat
        for key in ("p", "m", "v", "step"):
            assert mine[key].cpu().numpy().tobytes() == theirs[key].cpu().numpy().tobytes(), (info["update"], key)
        seen.append(info["update"])

    ln = Learner(256, 64, seed=0, deterministic=True, on_update=on_update, **MODES[mode])
    try:
        state["ln"] = ln
        state["ref"] = DeviceTrainer(ln.params, device="cuda", batched=True, backend="hip", **MODES[mode])
        ln.run(chunks=8)
        ln.sync()
        assert len(seen) >= 2 and ln.updates == len(seen)
    finally:
        ln.close()


def test_balance_is_refused_and_a_healthy_run_syncs():
    from bgx.learner import Learner
    with pytest.raises(ValueError, match="balance"):
        Learner(256, 64, seed=0, deterministic=True, balance=True)
    ln = Learner(256, 64, seed=0, deterministic=True)
    try:
        ln.run(chunks=8)
        ln.sync()   # the status word is zero: nothing raised
        assert ln.updates >= 1
        ln.sync()
    finally:
        ln.close()


def test_the_command_line_repeats_its_digest(capsys):
    from bgx import learn
    args = ["--lanes", "256", "--steps-per-chunk", "64", "--updates", "3", "--deterministic"]
    a = learn.main(args)
    b = learn.main(args)
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 2
    for out, line in zip((a, b), lines):
        assert out["deterministic"] is True and line["deterministic"] is True and out["updates"] == 3
        assert len(out["params_sha256"]) == 64 and line["params_sha256"] == out["params_sha256"]
        assert out["canon_s"] > 0
    assert a["params_sha256"] == b["params_sha256"]
