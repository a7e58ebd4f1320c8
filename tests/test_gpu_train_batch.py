"""bgx_td0_update_batched (csrc/bgx_train_batch.hip) on the GPU: its gradient
and V against the float64 restatement, its Adam stage against the fp32 one
(bgx/train_ref.py), DeviceTrainer(batched=True, backend="hip") against the
torch backend, reproducibility, and the sequential kernel left as it was.
Inputs are synthetic harvests built on the host (train_batch_cases.py), in the
shapes of train_gpu_runner.py (all but its last, which is the target stage's)."""
import numpy as np
import pytest
import torch

import train_batch_cases as tc
from train_gpu_runner import CASES as SHAPES, TD0, _PM, _adam64, _inputs, run

pytestmark = pytest.mark.gpu

GAMMA, LR = 0.99, 1e-3
F32_FACTOR = 4.0   # what DESIGN section 4 "Numerics" grants an fp32 chain in another summation order
Y_FLOOR_ULPS = 2    # fp32 ulps of max|Y64|: torch's own error can be 0 by chance (one record), a rounded fp32 V's cannot
_CACHE = {}
CASES = SHAPES[:6]


def _ref64(case, wname):
    if ("r64", case, wname) not in _CACHE:
        from bgx.train_ref import batched_td0_reference
        _, rec, offs = _inputs(case)
        _CACHE["r64", case, wname] = batched_td0_reference(tc.flat_params(tc.WEIGHTS[wname]), rec, offs, GAMMA)
    return _CACHE["r64", case, wname]


def _hip_lr0(case, wname):
    """The kernel's gradient of a case: lr = 0, zero moments (cached)."""
    if ("hip", case, wname) not in _CACHE:
        flat = tc.flat_params(tc.WEIGHTS[wname])
        _, rec, offs = _inputs(case)
        z = np.zeros_like(flat)
        _CACHE["hip", case, wname] = run(TD0, flat, z, z, 0, rec, offs, lr=0.0)
    return _CACHE["hip", case, wname]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("case", CASES)
def test_gradient_and_value_against_float64(case, wname):
    """err = max|g - g64| / max|g64| of the kernel's pre-clip gradient is at most
    4 x the same measure of torch's fp32 autograd of the batched loss (one
    forward per episode, as DeviceTrainer's torch path runs it) on the GPU; V
    the same way, max|Y - Y64| / max|Y64| (never asked to be below 2 fp32 ulps of
    max|Y64|, which a correctly rounded fp32 V may already miss while torch's
    error on a single record can be 0)."""
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = _inputs(case)
    r64 = _ref64(case, wname)
    hip = _hip_lr0(case, wname)
    g32, loss32, y32 = tc.torch_batched_grad(flat, rec, offs, GAMMA, torch.float32, device="cuda")
    gmax = np.abs(r64["grad"]).max()
    err_hip = np.abs(hip["grad"].astype(np.float64) - r64["grad"]).max() / gmax
    err_t32 = np.abs(g32 - r64["grad"]).max() / gmax
    ymax = np.abs(r64["Y"]).max()
    ey_hip = np.abs(hip["Y"].astype(np.float64) - r64["Y"]).max() / ymax
    ey_t32 = np.abs(y32 - r64["Y"]).max() / ymax
    y_floor = Y_FLOOR_ULPS * float(np.spacing(np.float32(ymax))) / ymax
    E = len(offs) - 1
    print(f"{case}/{wname}: records {len(rec)} episodes {E} grad err hip {err_hip:.3e} torch32 {err_t32:.3e} "
          f"| V err hip {ey_hip:.3e} torch32 {ey_t32:.3e}")
    assert np.isfinite(hip["grad"]).all() and hip["step"] == 1
    assert np.array_equal(hip["p"], flat)          # lr = 0: the parameters stay
    assert err_hip <= F32_FACTOR * err_t32
    assert ey_hip <= max(y_floor, F32_FACTOR * ey_t32)
    # metrics: E loss, E post-clip norm, sum_e mean |td|, sum_e mean V, reward sum
    met = hip["metrics"]
    norm = float(np.sqrt((r64["grad"] ** 2).sum()))
    want = [E * r64["loss"], E * min(norm, norm / (norm + 1e-6)), r64["td_error"], r64["predicted_value"],
            r64["reward"]]
    for k in range(5):
        assert met[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


def _adam_bound_ok(name, got, ref, delta):
    """|got - ref| <= 2^-20 |delta| + ulp(value): v_sqrt and v_rcp at most 1 ulp
    each and fewer than 6 more fp32 roundings in the step, under 8 ulp
    (2^-20) of it together, and one rounding of the final add."""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32)).astype(np.float64)
    excess = np.abs(got - ref) - (2.0 ** -20 * np.abs(delta.astype(np.float64)) + ulp)
    print(f"  {name}: max |diff| {np.abs(got - ref).max():.3e}, worst excess over the bound {excess.max():.3e}")
    return excess.max() <= 0.0


def _check_adam(label, before, after, clip):
    from bgx.train_ref import adam_reference
    p0, m0, v0, s0 = before
    r = adam_reference(p0, m0, v0, s0, after["grad"], LR, clip)
    print(f"{label}: norm {float(r['norm']):.6g} scale {float(r['scale']):.6g} step {r['step']}")
    assert after["step"] == r["step"] == s0 + 1
    assert _adam_bound_ok("params", after["p"], r["params"], r["u"])
    assert _adam_bound_ok("m", after["m"], r["m"], r["m"] - m0)
    assert _adam_bound_ok("v", after["v"], r["v"], r["v"] - v0)
    return r


def test_adam_stage_against_fp32_restatement():
    """The clip and the Adam step alone: adam_reference on the kernel's own
    pre-clip gradient. Clip active, clip off, a second call (step 2, moments
    carried) and a start from a non-zero Adam state."""
    flat = tc.flat_params(tc.WEIGHTS["ckpt"])
    _, rec, offs = _inputs("ragged_tile")
    z = np.zeros_like(flat)
    a1 = run(TD0, flat, z, z, 0, rec, offs, clip=1.0)
    r1 = _check_adam("clip 1.0", (flat, z, z, 0), a1, 1.0)
    assert float(r1["scale"]) < 1.0                # the clip was active
    assert a1["metrics"][1] == pytest.approx((len(offs) - 1) * float(r1["norm"] * r1["scale"]), rel=1e-6)
    a0 = run(TD0, flat, z, z, 0, rec, offs, clip=0.0)
    r0 = _check_adam("clip off", (flat, z, z, 0), a0, 0.0)
    assert float(r0["scale"]) == 1.0
    a2 = run(TD0, a1["p"], a1["m"], a1["v"], a1["step"], rec, offs, clip=1.0)
    _check_adam("second call", (a1["p"], a1["m"], a1["v"], 1), a2, 1.0)
    rng = np.random.default_rng(4)
    m0 = (rng.standard_normal(len(flat)) * 1e-3).astype(np.float32)
    v0 = (rng.random(len(flat)) * 1e-5).astype(np.float32)
    a3 = run(TD0, flat, m0, v0, 7, rec, offs, clip=1.0)
    _check_adam("non-zero state", (flat, m0, v0, 7), a3, 1.0)


def test_trainer_hip_against_torch_backend_and_backend_swaps():
    """DeviceTrainer(batched=True): 5 updates of 40 episodes on backend "hip" and
    on "torch" from the same weights. The parameters differ by at most 4 x what
    torch's differ from a float64 run of the same updates; loss and grad_norm
    agree to 1e-4. Then one trainer goes hip -> torch -> hip: the state carries
    over, under the same bound."""
    from bgx.train_ref import batched_td0_reference
    from bgx.trainer import DeviceTrainer
    flat0 = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat0)
    batches = [tc.synth(np.random.default_rng(300 + k).integers(5, 86, 40), seed=200 + k) for k in range(5)]
    pm_h, pm_t, pm_s = _PM(sd0), _PM(sd0), _PM(sd0)
    th = DeviceTrainer(pm_h, device="cuda", batch_episode_size=40, batched=True, backend="hip")
    tt = DeviceTrainer(pm_t, device="cuda", batch_episode_size=40, batched=True, backend="torch")
    ts = DeviceTrainer(pm_s, device="cuda", batch_episode_size=40, batched=True, backend="hip")
    assert th.backend == "hip" and tt.backend == "torch"
    p64, m64, v64, s64 = flat0.astype(np.float64), np.zeros(len(flat0)), np.zeros(len(flat0)), 0
    swap = ("hip", "torch", "hip", "torch", "hip")
    for k, (hdr, rec, offs) in enumerate(batches):
        mh = th.update_records(hdr, rec)
        mt = tt.update_records(hdr, rec)
        ts.backend = swap[k]
        ts.update_records(hdr, rec)
        r = batched_td0_reference(p64, rec, offs, GAMMA)
        p64, m64, v64, s64 = _adam64(p64, m64, v64, s64, r["grad"], LR, 1.0)
        dev_t = np.abs(pm_t.flat() - p64).max()
        dev_h = np.abs(pm_h.flat().astype(np.float64) - pm_t.flat()).max()
        dev_s = np.abs(pm_s.flat().astype(np.float64) - pm_t.flat()).max()
        print(f"update {k + 1}: torch vs fp64 {dev_t:.3e}, hip vs torch {dev_h:.3e}, swapping vs torch {dev_s:.3e}; "
              f"loss hip {mh['loss']:.6g} torch {mt['loss']:.6g} fp64 {r['loss']:.6g}")
        assert dev_h <= F32_FACTOR * dev_t
        assert dev_s <= F32_FACTOR * dev_t
        assert mh["loss"] == pytest.approx(mt["loss"], rel=1e-4)
        assert mh["grad_norm"] == pytest.approx(mt["grad_norm"], rel=1e-4)
        assert set(mh) == set(mt) and mh["episodes"] == 40 and mh["win_counts"] == mt["win_counts"]
        assert mh["episode_length"] == mt["episode_length"]
    with pytest.raises(ValueError):
        bad = batches[0][0].copy()
        bad[0, 3] = 0
        th.update_records(bad, batches[0][1])
    with pytest.raises(ValueError):
        th.update_records(batches[0][0], batches[0][1][:-1])   # offs[-1] != records


def test_same_call_twice_is_bit_identical():
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    _, rec, offs = _inputs("two_tiles_each")
    rng = np.random.default_rng(8)
    m0 = (rng.standard_normal(len(flat)) * 1e-3).astype(np.float32)
    v0 = (rng.random(len(flat)) * 1e-5).astype(np.float32)
    a = run(TD0, flat, m0, v0, 3, rec, offs)
    b = run(TD0, flat, m0, v0, 3, rec, offs)
    for k in ("p", "m", "v", "grad", "metrics", "Y"):
        assert np.array_equal(a[k], b[k]), k
    assert a["step"] == b["step"] == 4 and not np.array_equal(a["p"], flat)


def test_sequential_update_is_unchanged_by_a_batched_call():
    """DeviceTrainer(batched=False) on the same records before and after a
    batched update on another trainer: bit-identical weights and metrics."""
    from bgx.trainer import DeviceTrainer
    sd0 = tc.state_dict(tc.flat_params(tc.WEIGHTS["seed0"]))
    hdr, rec, _ = tc.synth(tc.ragged_lens(1500, 21, 1, 90), seed=22)
    out = []
    for k in range(2):
        pm = _PM(sd0)
        t = DeviceTrainer(pm, device="cuda", batch_episode_size=len(hdr))
        assert t.backend == "hip" and not t.batched
        met = t.update_records(hdr, rec)
        out.append((pm.flat(), met))
        if k == 0:
            pb = _PM(sd0)
            DeviceTrainer(pb, device="cuda", batched=True, backend="hip").update_records(hdr, rec)
            assert not np.array_equal(pb.flat(), pm.flat())
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
