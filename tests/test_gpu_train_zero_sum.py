"""bgx_td_update_batched (the zero-sum instance of csrc/bgx_train_lambda.hip
between the forward and backward launches of csrc/bgx_train_batch.hip) on the
GPU: its targets, V and gradient against the float64 restatement
(bgx/train_ref.py, zero_sum=True), flags = 0 bit-identical to
bgx_tdlambda_update_batched, one mover everywhere bit-identical to it with the
flag set, the flag reaching the update, reproducibility,
DeviceTrainer(batched=True, backend="hip", zero_sum=True) against the torch
backend, and the existing entry points left as they were.

The shapes are train_gpu_runner.py's. The records carry the movers they
were drawn with (about every second pair of neighbours changes the mover); two
more cases rewrite them (word 11 bit 9 and word 6 bit 16): alternating, and a
single change 64 records before each episode's end, the edge between the target
stage's last two chunks."""
import numpy as np
import pytest
import torch

import train_batch_cases as tc
import train_lambda_cases as lc
import train_zero_sum_cases as zc
from train_gpu_runner import CASES as SHAPES, LAMBDA, TD, TD0, _PM, _adam64, _inputs as _shape_inputs, _state, run

pytestmark = pytest.mark.gpu

GAMMA, LR = lc.GAMMA, 1e-3
F32_FACTOR = lc.F32_FACTOR
ZS = zc.TDF_ZERO_SUM
_CACHE = {}
CASES = [(s, "drawn") for s in SHAPES] + [("edges", "alternating"), ("edges", "flip64")]


def _inputs(shape, pattern="drawn"):
    if ("in", shape, pattern) not in _CACHE:
        hdr, rec, offs = _shape_inputs(shape)
        _CACHE["in", shape, pattern] = (hdr, zc.with_pattern(rec, offs, pattern), offs)
    return _CACHE["in", shape, pattern]


ALL = ("p", "m", "v", "grad", "metrics", "Y", "target")


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("lam", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0] if c[1] == "drawn" else f"{c[0]}-{c[1]}")
def test_targets_value_and_gradient_against_float64(case, lam, wname):
    """Against batched_td0_reference(lam, zero_sum=True) in float64, each error as
    max|x - x64| / max|x64|. The fp32 comparison is torch's fp32 autograd of the
    same loss on the GPU (one forward per episode) whose targets are the serial
    fp32 lambda_returns(movers=) on its own Y, detached.
    Targets (d_target_out): at most max(2 fp32 ulps of max|G64|, 4 x the serial
    fp32 recurrence's). Gradient: at most 4 x torch's. V: at most max(2 fp32
    ulps of max|Y64|, 4 x torch's). The five metrics: within rel 1e-4, abs 1e-5.

    The tightest case is tile_edge_boot (one episode of 129 records) at lam = 1,
    where the serial chain happens to be at 1.32e-7: the stage is at 2.93e-7
    (6.14e-7, over the bound, with the plain instance's fp32-squared powers
    throughout: DESIGN.md 8a, "Zero-sum targets")."""
    from bgx.train_ref import batched_td0_reference
    shape, pattern = case
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = _inputs(shape, pattern)
    r64 = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=True)
    z = np.zeros_like(flat)
    hip = run(TD, flat, z, z, 0, rec, offs, lam, ZS, lr=0.0)
    g32, loss32, y32, t32 = zc.torch_zero_sum_grad(flat, rec, offs, GAMMA, lam, torch.float32, device="cuda")
    err_hip, err_t32 = lc.rel_err(hip["grad"], r64["grad"]), lc.rel_err(g32, r64["grad"])
    ey_hip, ey_t32 = lc.rel_err(hip["Y"], r64["Y"]), lc.rel_err(y32, r64["Y"])
    et_hip, et_t32 = lc.rel_err(hip["target"], r64["target"]), lc.rel_err(t32, r64["target"])
    E = len(offs) - 1
    print(f"{shape}/{pattern}/{wname}/lam {lam}: records {len(rec)} episodes {E} target err hip {et_hip:.3e} serial32 "
          f"{et_t32:.3e} | grad err hip {err_hip:.3e} torch32 {err_t32:.3e} | V err hip {ey_hip:.3e} torch32 {ey_t32:.3e}")
    assert np.isfinite(hip["grad"]).all() and np.isfinite(hip["target"]).all() and hip["step"] == 1
    assert np.array_equal(hip["p"], flat)          # lr = 0: the parameters stay
    assert et_hip <= max(lc.floor_rel(r64["target"]), F32_FACTOR * et_t32)
    assert err_hip <= F32_FACTOR * err_t32
    assert ey_hip <= max(lc.floor_rel(r64["Y"]), F32_FACTOR * ey_t32)
    # metrics: E loss, E post-clip norm, sum_e mean |Y - G|, sum_e mean V, reward sum
    met = hip["metrics"]
    norm = float(np.sqrt((r64["grad"] ** 2).sum()))
    want = [E * r64["loss"], E * min(norm, norm / (norm + 1e-6)), r64["td_error"], r64["predicted_value"],
            r64["reward"]]
    for k in range(5):
        assert met[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("shape", ["ragged_tile", "two_tiles_each"])
def test_flags_zero_is_bit_identical_to_the_lambda_call(shape, lam):
    """flags = 0, lr = 1e-3 and non-zero moments: parameters, moments, step,
    gradient, metrics, V and d_target_out equal bgx_tdlambda_update_batched's bit
    for bit (the records' movers do change: they are not read)."""
    flat = tc.flat_params(tc.WEIGHTS["ckpt"])
    _, rec, offs = _inputs(shape)
    mv = zc.movers_of(rec)
    assert (mv[1:] != mv[:-1]).any()
    m0, v0 = _state(len(flat), 4)
    a = run(LAMBDA, flat, m0, v0, 7, rec, offs, lam)
    b = run(TD, flat, m0, v0, 7, rec, offs, lam, 0)
    for k in ALL:
        assert np.array_equal(a[k], b[k]), k
    assert a["step"] == b["step"] == 8 and not np.array_equal(a["p"], flat)


@pytest.mark.parametrize("lam", [0.0, 0.7, 1.0])
def test_one_mover_everywhere_is_the_lambda_call(lam):
    """BGX_TDF_ZERO_SUM on records that all have one mover: for lam in {0.7, 1}
    everything equals bgx_tdlambda_update_batched's bit for bit (the products by
    +1 are exact); for lam = 0, where the lambda call keeps the TD(0) backward
    launch, d_target_out and V do."""
    flat = tc.flat_params(tc.WEIGHTS["ckpt"])
    m0, v0 = _state(len(flat), 5)
    for shape in ("edges", "two_tiles_each"):
        _, rec, offs = _inputs(shape, "equal")
        assert not zc.movers_of(rec).any()
        a = run(LAMBDA, flat, m0, v0, 7, rec, offs, lam)
        b = run(TD, flat, m0, v0, 7, rec, offs, lam, ZS)
        for k in (ALL if lam != 0.0 else ("Y", "target")):
            assert np.array_equal(a[k], b[k]), (shape, k)
        assert a["step"] == b["step"] == 8


def test_alternating_movers_reach_the_update_and_the_call_is_reproducible():
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    m0, v0 = _state(len(flat), 8)
    for lam in (0.0, 0.7):
        _, rec, offs = _inputs("two_tiles_each", "alternating")
        plain = run(LAMBDA, flat, m0, v0, 3, rec, offs, lam)
        a = run(TD, flat, m0, v0, 3, rec, offs, lam, ZS)
        b = run(TD, flat, m0, v0, 3, rec, offs, lam, ZS)
        for k in ALL:
            assert np.array_equal(a[k], b[k]), (lam, k)
        assert a["step"] == b["step"] == 4 and not np.array_equal(a["p"], flat)
        assert not np.array_equal(a["p"], plain["p"]) and not np.array_equal(a["target"], plain["target"])
        assert np.array_equal(a["Y"], plain["Y"])


def test_trainer_hip_against_torch_backend_and_backend_swaps():
    """DeviceTrainer(batched=True, zero_sum=True, lam=0.7): 5 updates of 40
    episodes on backend "hip" and on "torch" from the same weights. The
    parameters differ by at most 4 x what torch's differ from a float64 run of
    the same updates (batched_td0_reference(lam=0.7, zero_sum=True) and Adam in
    float64); loss and grad_norm agree to 1e-4. Then one trainer goes hip ->
    torch -> hip: the state carries over, under the same bound. A zero_sum=False
    trainer's first loss on the same batch is another: by more than 1e-3 of it,
    ten times what the zero-sum paths agree to."""
    from bgx.train_ref import batched_td0_reference
    from bgx.trainer import DeviceTrainer
    lam = 0.7
    flat0 = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat0)
    batches = [tc.synth(np.random.default_rng(300 + k).integers(5, 86, 40), seed=200 + k) for k in range(5)]
    pm_h, pm_t, pm_s, pm_0 = _PM(sd0), _PM(sd0), _PM(sd0), _PM(sd0)
    kw = dict(device="cuda", batch_episode_size=40, batched=True, lam=lam)
    th = DeviceTrainer(pm_h, backend="hip", zero_sum=True, **kw)
    tt = DeviceTrainer(pm_t, backend="torch", zero_sum=True, **kw)
    ts = DeviceTrainer(pm_s, backend="hip", zero_sum=True, **kw)
    t0 = DeviceTrainer(pm_0, backend="hip", **kw)
    assert th.backend == "hip" and tt.backend == "torch" and th.zero_sum and tt.zero_sum and not t0.zero_sum
    p64, m64, v64, s64 = flat0.astype(np.float64), np.zeros(len(flat0)), np.zeros(len(flat0)), 0
    swap = ("hip", "torch", "hip", "torch", "hip")
    for k, (hdr, rec, offs) in enumerate(batches):
        mh = th.update_records(hdr, rec)
        mt = tt.update_records(hdr, rec)
        ts.backend = swap[k]
        ts.update_records(hdr, rec)
        m0 = t0.update_records(hdr, rec)
        if k == 0:
            assert abs(m0["loss"] - mh["loss"]) > 1e-3 * mh["loss"]
        r = batched_td0_reference(p64, rec, offs, GAMMA, lam=lam, zero_sum=True)
        p64, m64, v64, s64 = _adam64(p64, m64, v64, s64, r["grad"], LR, 1.0)
        dev_t = np.abs(pm_t.flat() - p64).max()
        dev_h = np.abs(pm_h.flat().astype(np.float64) - pm_t.flat()).max()
        dev_s = np.abs(pm_s.flat().astype(np.float64) - pm_t.flat()).max()
        print(f"update {k + 1}: torch vs fp64 {dev_t:.3e}, hip vs torch {dev_h:.3e}, swapping vs torch {dev_s:.3e}; "
              f"loss hip {mh['loss']:.6g} torch {mt['loss']:.6g} fp64 {r['loss']:.6g} | zero_sum=False {m0['loss']:.6g}")
        assert dev_h <= F32_FACTOR * dev_t
        assert dev_s <= F32_FACTOR * dev_t
        assert mh["loss"] == pytest.approx(mt["loss"], rel=1e-4)
        assert mh["loss"] == pytest.approx(r["loss"], rel=1e-4)
        assert mh["grad_norm"] == pytest.approx(mt["grad_norm"], rel=1e-4)
        assert mh["td_error"] == pytest.approx(mt["td_error"], rel=1e-4)
        assert set(mh) == set(mt) and mh["episodes"] == 40 and mh["win_counts"] == mt["win_counts"]
        assert mh["episode_length"] == mt["episode_length"]


def test_existing_entry_points_are_unchanged_by_a_zero_sum_call():
    """bgx_td0_update_batched, bgx_tdlambda_update_batched and the sequential
    bgx_td0_update (DeviceTrainer(batched=False)) on the same inputs before and
    after a zero-sum call: bit-identical results (no state beyond the arguments)."""
    from bgx.trainer import DeviceTrainer
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat)
    _, rec, offs = _inputs("ragged_tile")
    m0, v0 = _state(len(flat), 9)
    hdr, srec, _ = tc.synth(tc.ragged_lens(1500, 21, 1, 90), seed=22)
    batched, lam, seq = [], [], []
    for k in range(2):
        batched.append(run(TD0, flat, m0, v0, 2, rec, offs))
        lam.append(run(LAMBDA, flat, m0, v0, 2, rec, offs, 0.7))
        pm = _PM(sd0)
        t = DeviceTrainer(pm, device="cuda", batch_episode_size=len(hdr))
        assert t.backend == "hip" and not t.batched and t.lam == 0.0 and not t.zero_sum
        met = t.update_records(hdr, srec)
        seq.append((pm.flat(), met))
        if k == 0:
            zs = run(TD, flat, m0, v0, 2, rec, offs, 0.7, ZS)
            assert not np.array_equal(zs["p"], lam[0]["p"])
            pb = _PM(sd0)
            DeviceTrainer(pb, device="cuda", batched=True, backend="hip", lam=0.7, zero_sum=True).update_records(hdr, srec)
            assert not np.array_equal(pb.flat(), pm.flat())
    for k in ("p", "m", "v", "grad", "metrics", "Y"):
        assert np.array_equal(batched[0][k], batched[1][k]), k
    for k in ALL:
        assert np.array_equal(lam[0][k], lam[1][k]), k
    assert batched[0]["step"] == batched[1]["step"] == lam[0]["step"] == lam[1]["step"] == 3
    assert np.array_equal(seq[0][0], seq[1][0])
    assert seq[0][1] == seq[1][1]
