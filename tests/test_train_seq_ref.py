"""CPU checks behind the sequential TD(0) kernel's piecewise tests
(test_gpu_train_seq.py): the rule that reads the kernel's gradient back from
its first moment, the inputs' own claims (the feature-edge episode's coverage,
which cases clip), the float64 chain against the reference loop restated in
test_gpu_trainer.py, and DeviceTrainer's record-count check, which comes
before libbgx.so is touched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_batch_cases as tc
import train_seq_cases as sc


def test_gradient_read_back_is_one_rounding():
    """m = fl32(fl32(0.1) g) from zero moments (g - 0 and 0 + x are exact), so
    m / fl32(0.1) in float64 is g to one fp32 rounding: 2^-24 relative."""
    rng = np.random.default_rng(1)
    g = (rng.standard_normal(200000) * 10.0 ** rng.uniform(-30, 3, 200000)).astype(np.float32)
    g = g[g != 0]
    assert sc.W1M == np.float32(0.1)
    m = np.float32(0.0) + sc.W1M * (g - np.float32(0.0))
    assert m.dtype == np.float32
    back = sc.grad_from_m(m)
    rel = np.abs(back - g.astype(np.float64)) / np.abs(g.astype(np.float64))
    assert rel.max() <= 2.0 ** -24
    assert rel.max() > 2.0 ** -26          # the rounding is there: the bound is not slack by construction


def test_feature_edge_episode_covers_every_count():
    """Every count 0..15 on points 0, 7, 8, 15, 16, 23 of both players and on
    bar and off of both, under either mover; encode_records on these records
    equals the C oracle's encoder (which the env_traj boards, rarely above 5
    checkers on a point, do not take to 15)."""
    import oracle
    from bgx.train_ref import encode_records
    rec = sc.edge_records()
    assert rec.shape == (40, 12) and rec.dtype == np.uint32
    sh = (np.arange(8, dtype=np.uint32) * 4)[None, None, :]
    n = ((rec[:, :6, None] >> sh) & 15).reshape(len(rec), 48)
    s6 = rec[:, 6]
    mover = (s6 >> 16) & 1
    assert np.array_equal(mover, (rec[:, 11] >> 9) & 1)
    fields = [n[:, 24 * pl + pt] for pl in (0, 1) for pt in sc.EDGE_POINTS] + [(s6 >> k) & 15 for k in (0, 4, 8, 12)]
    for f in fields:
        for mv in (0, 1):
            assert set(f[mover == mv].tolist()) == set(range(16))
    boards = np.concatenate([n, np.stack([s6 & 15, (s6 >> 4) & 15, (s6 >> 8) & 15, (s6 >> 12) & 15], 1)], 1)
    got = encode_records(rec)
    assert np.array_equal(got, oracle.encode_many(boards.astype(np.uint8), mover.astype(np.uint8)))
    assert got[:, 3:192:4].max() == 6.0 and got[:, 192].max() == 7.5 and got[:, 195].max() == 1.0


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_clip_table_from_float64_norms(wname):
    """The clip cases are the lengths whose float64 gradient norm is outside
    [0.95, 1.05], each on the side its table says, and both sides occur for
    either weight set: at grad_clip = 1 the GPU test then knows which branch
    of the clip a case takes."""
    for case in sc.CASES:
        norm = float(np.sqrt((sc.ref64(case, wname)["grad"] ** 2).sum()))
        print(f"{wname} T={case}: float64 norm {norm:.4g}")
        assert (norm > 1.05) == (case in sc.CLIP_ACTIVE[wname]), (case, norm)
        assert (norm < 0.95) == (case in sc.CLIP_INACTIVE[wname]), (case, norm)
    assert sc.CLIP_ACTIVE[wname] and sc.CLIP_INACTIVE[wname]


def test_float64_chain_equals_the_reference_loop_in_float64():
    """chain64 (per episode: batched_td0_reference with one episode, clip,
    Adam) against test_gpu_trainer._reference_update, the restated reference
    loop (torch autograd, clip_grad_norm_, torch.optim.Adam), run in float64
    on two short episodes, one of them a single record."""
    from bgx.train_ref import encode_records
    from test_gpu_trainer import _reference_update
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    _, rec, offs = tc.synth([5, 1], seed=9)
    obs = encode_records(rec).astype(np.float64)
    rew = np.ascontiguousarray(rec[:, 9]).view(np.float32).astype(np.float64)
    eps = [SimpleNamespace(experiences=[SimpleNamespace(observation=obs[k], reward=rew[k])
                                        for k in range(int(offs[e]), int(offs[e + 1]))]) for e in range(2)]
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        sd = _reference_update({k: v.double() for k, v in tc.state_dict(flat).items()}, eps,
                               lr=sc.LR, gamma=sc.GAMMA, clip=1.0)
    finally:
        torch.set_default_dtype(prev)
    want = np.concatenate([sd[k].numpy().reshape(-1) for k in ("fc1.weight", "fc1.bias", "value_head.weight",
                                                               "value_head.bias")])
    assert want.dtype == np.float64
    got, step = sc.chain64(flat, rec, offs)
    assert step == 2
    moved = np.abs(got - flat.astype(np.float64)).max()
    assert moved > 1e-4                                   # two Adam steps of lr 1e-3 happened
    assert np.abs(got - want).max() <= 1e-12


class _PM:
    def get_parameters(self, device=None):
        return tc.state_dict(tc.flat_params(tc.WEIGHTS["seed0"]))

    def set_parameters(self, sd):
        raise AssertionError("no update may complete")


def test_sequential_hip_update_counts_the_records_before_the_library(monkeypatch):
    """DeviceTrainer(batched=False, backend="hip").update_records raises
    ValueError when the headers count more or fewer records than it was given,
    and does so before libbgx.so is asked for (the kernel would read
    offs[-1] records whatever the tensor holds)."""
    import bgx._lib
    from bgx.trainer import DeviceTrainer

    def no_lib():
        raise AssertionError("the library was touched before the record count was checked")

    monkeypatch.setattr(bgx._lib, "lib", no_lib)
    hdr, rec, _ = tc.synth([3, 1, 5], seed=3)
    t = DeviceTrainer(_PM(), device="cpu", batch_episode_size=3)
    assert t.backend == "hip" and not t.batched
    with pytest.raises(ValueError, match="count 9 records, got 8"):
        t.update_records(hdr, rec[:-1])
    with pytest.raises(ValueError, match="count 9 records, got 10"):
        t.update_records(hdr, np.concatenate([rec, rec[:1]]))
    short = hdr.copy()
    short[2, 3] = 4
    with pytest.raises(ValueError, match="count 8 records, got 9"):
        t.update_records(short, rec)
    with pytest.raises(ValueError, match="more than 2048"):
        t.update_records(sc.headers_for([2049]), np.zeros((2049, 12), np.uint32))
