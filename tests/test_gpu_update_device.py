"""DeviceTrainer.update_device against update_records on the same harvest: the
flat parameters, both Adam moments, the step count and the metrics come out
bit-identical for the plain, lambda, zero-sum and afterstate updates, from a
clone and from a tensor that aliases the ticket's own arrays; the host views
(state_dict, publish) follow on demand; the wrong backend raises."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {"plain": {}, "lam": dict(lam=0.7), "zero_sum": dict(zero_sum=True, lam=0.3),
         "afterstates": dict(afterstates=True, lam=0.7, zero_sum=True)}
METRIC_KEYS = ("loss", "grad_norm", "td_error", "predicted_value", "reward", "episode_length", "episodes")


class PM:
    def __init__(self, sd):
        self.sd, self.version = {k: v.detach().cpu().clone() for k, v in sd.items()}, 1

    def get_parameters(self, device=None):
        return self.sd

    def set_parameters(self, sd):
        self.sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
        self.version += 1


def _trainer(**kw):
    from bgx.net import BackgammonPolicyNetwork
    from bgx.trainer import DeviceTrainer
    torch.manual_seed(3)
    pm = PM(BackgammonPolicyNetwork().state_dict())
    kw = {"batched": True, "backend": "hip", **kw}
    return DeviceTrainer(pm, device="cuda", **kw), pm


@pytest.fixture(scope="module")
def engine_and_tickets(weights_seed0):
    """One engine, two harvests of about 150 episodes each: the first as clones,
    the second left aliasing the ticket's arrays. Read-only for the tests."""
    from bgx import Engine
    e = Engine(lanes=128, seed=6, ply=1)
    e.set_weights(weights_seed0, temperature=1.5)
    e.step(200)
    first = e.harvest(clone=True)
    e.step(120)
    t = e.harvest_enqueue()
    alias = e.harvest_fetch(t, clone=False)
    assert first.n_episodes >= 60 and alias.n_episodes >= 40
    yield first, alias
    e.close()


def _state(tr):
    f = tr._flat
    return {k: f[k].cpu().numpy().copy() for k in ("p", "m", "v", "step")}


@pytest.mark.parametrize("mode", list(MODES))
def test_update_device_equals_update_records_bit_for_bit(engine_and_tickets, mode):
    first, alias = engine_and_tickets
    ref, _ = _trainer(**MODES[mode])
    dev, pm = _trainer(**MODES[mode])
    for k, h in enumerate((first, alias, first)):   # Adam state carried across updates; the alias is used in place
        want = ref.update_records(h.headers.clone(), h.records.clone())
        assert dev.update_device(h.headers, h.records) is None
        got = dev.metrics(reset=True)
        a, b = _state(ref), _state(dev)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (mode, k, key)
        assert int(b["step"][0]) == k + 1
        for key in METRIC_KEYS:
            assert got[key] == want[key], (mode, k, key, got[key], want[key])
        assert got["updates"] == 1
    assert dev.metrics() is None   # reset: nothing since
    assert np.isfinite(a["p"]).all() and np.abs(a["m"]).max() > 0
    # the host follows on demand only
    assert pm.version == 1
    sd = dev.state_dict()
    flat = torch.cat([sd[k].reshape(-1) for k in dev._KEYS]).cpu().numpy()
    assert flat.tobytes() == b["p"].tobytes()
    dev.publish()
    assert pm.version == 2
    assert torch.equal(pm.sd["fc1.weight"], sd["fc1.weight"].cpu())
    assert dev.total_episodes == ref.total_episodes


def test_metrics_accumulate_until_read(engine_and_tickets):
    first, alias = engine_and_tickets
    ref, _ = _trainer()
    dev, _ = _trainer()
    want = [ref.update_records(h.headers.clone(), h.records.clone()) for h in (first, alias)]
    for h in (first, alias):
        dev.update_device(h.headers, h.records)
    got = dev.metrics(reset=False)
    n = [w["episodes"] for w in want]
    assert got["updates"] == 2 and got["episodes"] == sum(n)
    for key in ("loss", "grad_norm", "td_error", "predicted_value", "reward", "episode_length"):
        mean = (want[0][key] * n[0] + want[1][key] * n[1]) / sum(n)
        assert got[key] == pytest.approx(mean, rel=1e-12), key
    assert dev.metrics(reset=True) == got and dev.metrics() is None


def test_update_device_needs_the_batched_hip_backend(engine_and_tickets):
    first, _ = engine_and_tickets
    for kw in (dict(batched=True, backend="torch"), dict(batched=False, backend="hip"), dict(batched=False, backend="torch")):
        tr, _ = _trainer(**kw)
        with pytest.raises(ValueError, match="batched=True and backend='hip'"):
            tr.update_device(first.headers, first.records)
    tr, _ = _trainer()
    with pytest.raises(ValueError):
        tr.update_device(first.headers.cpu(), first.records)           # host tensor
    with pytest.raises(ValueError):
        tr.update_device(first.headers, first.records.to(torch.int64))  # wrong dtype
    with pytest.raises(ValueError):
        tr.update_device(first.headers[:0], first.records)             # no episodes
