"""bgx.learner.Learner on the GPU: 256 lanes, 64 steps per chunk, 8 chunks. A
second trainer replays every on_update ticket through update_records and must
match the learner's parameters bit for bit after every update; empty tickets
make no update; versions and temperatures follow the reference schedule; the
engine ends on the host pack of the final parameters; a hand-off of
non-finite weights raises and the engine still steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {"plain": {}, "lam_zero_sum_afterstates": dict(lam=0.7, zero_sum=True, afterstates=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_learner_matches_a_replaying_trainer_after_every_update(mode):
    from bgx import Engine
    from bgx.learner import Learner, reference_temperature
    from bgx.trainer import DeviceTrainer
    seen = []
    state = {}

    def on_update(info):
        ref = state["ref"]
        # the ticket's arrays are valid here; the replay goes through the host as update_records does
        ref.update_records(info["headers"].clone(), info["records"].clone())
        mine, theirs = state["ln"].trainer._flat, ref._flat
        for key in ("p", "m", "v", "step"):
            assert mine[key].cpu().numpy().tobytes() == theirs[key].cpu().numpy().tobytes(), (info["update"], key)
        seen.append({k: info[k] for k in ("update", "version", "temperature", "chunk", "ticket")} |
                    {"episodes": int(info["headers"].shape[0]), "records": int(info["records"].shape[0])})

    ln = Learner(256, 64, seed=0, on_update=on_update, **MODES[mode])
    try:
        state["ln"] = ln
        state["ref"] = DeviceTrainer(ln.params, device="cuda", batched=True, backend="hip", **MODES[mode])
        ln.run(chunks=8)
        ln.sync()
        print(mode, ln.log, seen)
        # tickets 0 .. 6 were looked at, in order; an update exactly where episodes had finished
        assert [t for t, _, _ in ln.log] == list(range(7)) and ln.chunks == 8
        assert all(updated == (n > 0) for _, n, updated in ln.log)
        assert [s["ticket"] for s in seen] == [t for t, n, _ in ln.log if n > 0]
        assert [s["episodes"] for s in seen] == [n for _, n, _ in ln.log if n > 0]
        assert all(s["chunk"] == s["ticket"] + 1 for s in seen)   # ticket c - 1 is trained during chunk c
        # (at least two updates, so that the second starts from the first one's Adam moments)
        assert len(seen) >= 2 and ln.updates == len(seen) and ln.episodes == sum(s["episodes"] for s in seen)
        # the reference schedule: version 1 is the initial network, every update is one version
        assert [s["update"] for s in seen] == list(range(1, len(seen) + 1))
        assert [s["version"] for s in seen] == list(range(2, len(seen) + 2))
        assert [s["temperature"] for s in seen] == [reference_temperature(v) for v in range(2, len(seen) + 2)]
        assert ln.version == ln.engine.version == len(seen) + 1
        assert ln.engine.temperature == reference_temperature(ln.version)
        # the engine plays on the host pack of the final parameters
        w = ln.weights()
        host = Engine(lanes=64, seed=1, ply=1, fused=False)
        try:
            host.set_weights(w, temperature=1.0)
            assert np.array_equal(ln.engine.peek("net_frag"), host.peek("net_frag"))
        finally:
            host.close()
        m = ln.metrics()
        assert m["updates"] == len(seen) and m["episodes"] == ln.episodes and np.isfinite(m["loss"])
        assert ln.gpu_ms["step"] > 0 and ln.gpu_ms["update"] > 0
    finally:
        ln.close()


def test_an_empty_ticket_makes_no_update():
    """No game ends within 8 steps (13 at the least): ticket 0 is empty by rule."""
    from bgx.learner import Learner
    calls = []
    ln = Learner(64, 8, seed=0, on_update=calls.append)
    try:
        ln.run(chunks=2)
        ln.sync()
        assert ln.log == [(0, 0, False)]
        assert ln.updates == 0 and ln.version == 1 and ln.engine.version == 1 and not calls
        assert ln.metrics() is None
    finally:
        ln.close()


def test_nonfinite_weights_raise_and_the_engine_still_steps():
    from bgx import BgxError
    from bgx.learner import Learner
    ln = Learner(256, 64, seed=0, lr=float("inf"))
    try:
        before = None
        with pytest.raises(BgxError, match="is not finite"):
            for _ in range(12):
                before = ln.engine.peek("net_frag") if ln.chunks >= 2 else before
                ln.run_chunk()
        assert ln.updates == 0 and ln.version == 1 and ln.engine.version == 1
        assert not torch.isfinite(ln.trainer.params).all()
        if before is not None:
            assert np.array_equal(ln.engine.peek("net_frag"), before)   # the previous network is in force
        steps = ln.engine.stats()["env_steps"]
        ln.engine.step(4, stream=ln.stream)
        ln.sync()
        assert ln.engine.stats()["env_steps"] == steps + 4 * 256
    finally:
        ln.close()
