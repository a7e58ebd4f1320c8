"""bgx_tdlambda_update_batched (csrc/bgx_train_lambda.hip between the forward and
backward launches of csrc/bgx_train_batch.hip) on the GPU: its targets, V and
gradient against the float64 restatement (bgx/train_ref.py), lambda = 0
bit-identical to bgx_td0_update_batched, lambda = 1 independent of the weights,
reproducibility, DeviceTrainer(batched=True, backend="hip", lam=0.7) against
the torch backend, and the TD(0) entry points left as they were.

The shapes are train_gpu_runner.py's (one record; a bootstrap across a tile
edge; an episode edge on a tile edge; a ragged tile; 2 G TILE + 7 records; an
episode of 2,100 records; and one harvest whose episode lengths put every width
of the target stage's 64-record chunks up to 256 at length - 1, equal and + 1)."""
import numpy as np
import pytest
import torch

import train_batch_cases as tc
import train_lambda_cases as lc
from train_gpu_runner import CASES, LAMBDA, TD0, _PM, _adam64, _inputs, _state, run

pytestmark = pytest.mark.gpu

GAMMA, LR = lc.GAMMA, 1e-3
F32_FACTOR = lc.F32_FACTOR
_CACHE = {}
def _ref64(case, wname, lam):
    if ("r64", case, wname, lam) not in _CACHE:
        from bgx.train_ref import batched_td0_reference
        _, rec, offs = _inputs(case)
        _CACHE["r64", case, wname, lam] = batched_td0_reference(tc.flat_params(tc.WEIGHTS[wname]), rec, offs, GAMMA,
                                                                 lam=lam)
    return _CACHE["r64", case, wname, lam]


def _hip_lr0(case, wname, lam):
    """The kernels' gradient and targets of a case: lr = 0, zero moments (cached)."""
    if ("hip", case, wname, lam) not in _CACHE:
        flat = tc.flat_params(tc.WEIGHTS[wname])
        _, rec, offs = _inputs(case)
        z = np.zeros_like(flat)
        _CACHE["hip", case, wname, lam] = run(LAMBDA, flat, z, z, 0, rec, offs, lam, lr=0.0)
    return _CACHE["hip", case, wname, lam]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("lam", [0.7, 1.0])
@pytest.mark.parametrize("case", CASES)
def test_targets_value_and_gradient_against_float64(case, lam, wname):
    """Against batched_td0_reference(lam) in float64, each error as max|x - x64| /
    max|x64|. The fp32 comparison is torch's fp32 autograd of the same loss on
    the GPU (one forward per episode) whose targets are the serial fp32
    lambda_returns on its own Y, detached.
    Targets (d_target_out): at most max(2 fp32 ulps of max|G64|, 4 x the serial
    fp32 recurrence's). Gradient: at most 4 x torch's. V: at most max(2 fp32
    ulps of max|Y64|, 4 x torch's). The five metrics: within rel 1e-4, abs 1e-5."""
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = _inputs(case)
    r64 = _ref64(case, wname, lam)
    hip = _hip_lr0(case, wname, lam)
    g32, loss32, y32, t32 = lc.torch_lambda_grad(flat, rec, offs, GAMMA, lam, torch.float32, device="cuda")
    err_hip, err_t32 = lc.rel_err(hip["grad"], r64["grad"]), lc.rel_err(g32, r64["grad"])
    ey_hip, ey_t32 = lc.rel_err(hip["Y"], r64["Y"]), lc.rel_err(y32, r64["Y"])
    et_hip, et_t32 = lc.rel_err(hip["target"], r64["target"]), lc.rel_err(t32, r64["target"])
    E = len(offs) - 1
    print(f"{case}/{wname}/lam {lam}: records {len(rec)} episodes {E} target err hip {et_hip:.3e} serial32 {et_t32:.3e} "
          f"| grad err hip {err_hip:.3e} torch32 {err_t32:.3e} | V err hip {ey_hip:.3e} torch32 {ey_t32:.3e}")
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


@pytest.mark.parametrize("case", ["ragged_tile", "two_tiles_each"])
def test_lambda_zero_is_bit_identical_to_the_td0_call(case):
    """lambda = 0 through the new entry point, lr = 1e-3 and non-zero moments:
    parameters, moments, step, gradient, metrics and V equal
    bgx_td0_update_batched's bit for bit, with and without d_target_out; the
    targets it returns are the TD(0) ones, r + gamma Y[s + 1] in one fma."""
    flat = tc.flat_params(tc.WEIGHTS["ckpt"])
    _, rec, offs = _inputs(case)
    m0, v0 = _state(len(flat), 4)
    a = run(TD0, flat, m0, v0, 7, rec, offs)
    for want_target in (True, False):
        b = run(LAMBDA, flat, m0, v0, 7, rec, offs, 0.0, want_target=want_target)
        for k in ("p", "m", "v", "grad", "metrics", "Y"):
            assert np.array_equal(a[k], b[k]), (k, want_target)
        assert a["step"] == b["step"] == 8 and not np.array_equal(a["p"], flat)
        if want_target:
            y = a["Y"].astype(np.float64)
            last = np.zeros(len(rec), bool)
            last[offs[1:] - 1] = True
            tg = lc.rewards(rec).astype(np.float64) + np.where(last, 0.0, float(np.float32(GAMMA)) * np.append(y[1:], 0.0))
            assert np.array_equal(b["target"], tg.astype(np.float32))   # the double sum rounds once, as the fma does


def test_lambda_one_targets_do_not_depend_on_the_weights():
    """lambda = 1: the discounted Monte-Carlo return, bit-identical under the
    seed0 and ckpt weights (whose V differ), and not the TD(0) target."""
    out = {}
    for case in ("edges", "ragged_tile"):
        _, rec, offs = _inputs(case)
        for w in tc.WEIGHTS:
            out[w] = _hip_lr0(case, w, 1.0)
        assert not np.array_equal(out["seed0"]["Y"], out["ckpt"]["Y"])
        assert np.array_equal(out["seed0"]["target"], out["ckpt"]["target"]), case
        assert not np.array_equal(out["seed0"]["target"], lc.rewards(rec))


def test_same_call_twice_is_bit_identical():
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    _, rec, offs = _inputs("two_tiles_each")
    m0, v0 = _state(len(flat), 8)
    a = run(LAMBDA, flat, m0, v0, 3, rec, offs, 0.7)
    b = run(LAMBDA, flat, m0, v0, 3, rec, offs, 0.7)
    for k in ("p", "m", "v", "grad", "metrics", "Y", "target"):
        assert np.array_equal(a[k], b[k]), k
    assert a["step"] == b["step"] == 4 and not np.array_equal(a["p"], flat)


def test_trainer_hip_against_torch_backend_and_backend_swaps():
    """DeviceTrainer(batched=True, lam=0.7): 5 updates of 40 episodes on backend
    "hip" and on "torch" from the same weights. The parameters differ by at most
    4 x what torch's differ from a float64 run of the same updates
    (batched_td0_reference(lam=0.7) and Adam in float64); loss and grad_norm
    agree to 1e-4. Then one trainer goes hip -> torch -> hip: the state carries
    over, under the same bound. A lam = 0 trainer's first loss on the same
    batch is another (lam does reach the update)."""
    from bgx.train_ref import batched_td0_reference
    from bgx.trainer import DeviceTrainer
    lam = 0.7
    flat0 = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat0)
    batches = [tc.synth(np.random.default_rng(300 + k).integers(5, 86, 40), seed=200 + k) for k in range(5)]
    pm_h, pm_t, pm_s, pm_0 = _PM(sd0), _PM(sd0), _PM(sd0), _PM(sd0)
    kw = dict(device="cuda", batch_episode_size=40, batched=True)
    th = DeviceTrainer(pm_h, backend="hip", lam=lam, **kw)
    tt = DeviceTrainer(pm_t, backend="torch", lam=lam, **kw)
    ts = DeviceTrainer(pm_s, backend="hip", lam=lam, **kw)
    t0 = DeviceTrainer(pm_0, backend="hip", **kw)
    assert th.backend == "hip" and tt.backend == "torch" and th.lam == tt.lam == lam and t0.lam == 0.0
    p64, m64, v64, s64 = flat0.astype(np.float64), np.zeros(len(flat0)), np.zeros(len(flat0)), 0
    swap = ("hip", "torch", "hip", "torch", "hip")
    for k, (hdr, rec, offs) in enumerate(batches):
        mh = th.update_records(hdr, rec)
        mt = tt.update_records(hdr, rec)
        ts.backend = swap[k]
        ts.update_records(hdr, rec)
        m0 = t0.update_records(hdr, rec)
        if k == 0:   # the same weights, another target: far outside the 1e-4 the lam = 0.7 paths agree to
            assert abs(m0["loss"] - mh["loss"]) > 1e-2 * mh["loss"]
        r = batched_td0_reference(p64, rec, offs, GAMMA, lam=lam)
        p64, m64, v64, s64 = _adam64(p64, m64, v64, s64, r["grad"], LR, 1.0)
        dev_t = np.abs(pm_t.flat() - p64).max()
        dev_h = np.abs(pm_h.flat().astype(np.float64) - pm_t.flat()).max()
        dev_s = np.abs(pm_s.flat().astype(np.float64) - pm_t.flat()).max()
        print(f"update {k + 1}: torch vs fp64 {dev_t:.3e}, hip vs torch {dev_h:.3e}, swapping vs torch {dev_s:.3e}; "
              f"loss hip {mh['loss']:.6g} torch {mt['loss']:.6g} fp64 {r['loss']:.6g}")
        assert dev_h <= F32_FACTOR * dev_t
        assert dev_s <= F32_FACTOR * dev_t
        assert mh["loss"] == pytest.approx(mt["loss"], rel=1e-4)
        assert mh["loss"] == pytest.approx(r["loss"], rel=1e-4)
        assert mh["grad_norm"] == pytest.approx(mt["grad_norm"], rel=1e-4)
        assert mh["td_error"] == pytest.approx(mt["td_error"], rel=1e-4)
        assert set(mh) == set(mt) and mh["episodes"] == 40 and mh["win_counts"] == mt["win_counts"]
        assert mh["episode_length"] == mt["episode_length"]


def test_td0_entry_points_are_unchanged_by_a_lambda_call():
    """bgx_td0_update_batched and the sequential bgx_td0_update
    (DeviceTrainer(batched=False)) on the same inputs before and after a
    lambda call: bit-identical results (no state beyond the arguments)."""
    from bgx.trainer import DeviceTrainer
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat)
    _, rec, offs = _inputs("ragged_tile")
    m0, v0 = _state(len(flat), 9)
    hdr, srec, _ = tc.synth(tc.ragged_lens(1500, 21, 1, 90), seed=22)
    batched, seq = [], []
    for k in range(2):
        batched.append(run(TD0, flat, m0, v0, 2, rec, offs))
        pm = _PM(sd0)
        t = DeviceTrainer(pm, device="cuda", batch_episode_size=len(hdr))
        assert t.backend == "hip" and not t.batched and t.lam == 0.0
        met = t.update_records(hdr, srec)
        seq.append((pm.flat(), met))
        if k == 0:
            lam_out = run(LAMBDA, flat, m0, v0, 2, rec, offs, 0.7)
            assert not np.array_equal(lam_out["p"], batched[0]["p"])
            pb = _PM(sd0)
            DeviceTrainer(pb, device="cuda", batched=True, backend="hip", lam=0.7).update_records(hdr, srec)
            assert not np.array_equal(pb.flat(), pm.flat())
    for k in ("p", "m", "v", "grad", "metrics", "Y"):
        assert np.array_equal(batched[0][k], batched[1][k]), k
    assert batched[0]["step"] == batched[1]["step"] == 3
    assert np.array_equal(seq[0][0], seq[1][0])
    assert seq[0][1] == seq[1][1]
