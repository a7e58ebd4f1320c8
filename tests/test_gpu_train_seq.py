"""bgx_td0_update (csrc/bgx_train.hip, the sequential TD(0) kernel: one
workgroup, one Adam step per episode) piece by piece on the GPU: its gradient,
V and metrics against the float64 restatement (bgx/train_ref.py; with one
episode the batched loss is the sequential kernel's), its own norm, the clip
and the Adam step against the fp32 restatement, several episodes in one launch
against one launch each, and DeviceTrainer's checks in front of it.

The gradient is read through the first moment (train_seq_cases.py): a call
with lr = 0, grad_clip = 0, zero moments and step = 0 leaves m = fl32(0.1 g).
The episode lengths sit on the kernel's own edges: its chunk of 64 records
(TR_TC), whose last one bootstraps from the next chunk's first, the reverse
reload of pass 2, and TRAIN_TMAX = 2,048; one episode is hand-packed to take
every field of the feature decoder (live_feature) through 0..15."""
import numpy as np
import pytest
import torch

import train_batch_cases as tc
import train_seq_cases as sc
from train_gpu_runner import _PM

pytestmark = pytest.mark.gpu

GAMMA, LR = sc.GAMMA, sc.LR
U = 2.0 ** -24          # one correctly rounded fp32 operation, relative
F32_FACTOR = 4.0        # what DESIGN 8a "Numerics" grants an fp32 chain in another summation order
GRAD_FLOOR = 2.0 ** -22  # 4 fp32 ulps of max|g64|: the read-back's own rounding, and torch exact by chance on one record
Y_FLOOR_ULPS = 2        # as test_gpu_train_batch.py: a rounded fp32 V cannot be asked for less
# Roundings of the kernel's squared norm, each at most U of a partial sum that
# never exceeds the total: gS * gS (1), 52 fma per thread, 6 shuffle levels, 7
# adds of wave partials (the first, to 0, is exact), and the correctly rounded
# square root, which counts twice on the square: 68. The float64 side sums g'^2,
# and g' carries the read-back's one rounding, twice on the square: 70.
NORM_ROUNDINGS = 70
# Roundings between the kernel's Adam step and adam_reference's, relative to the
# quantity's change, in units of U (v_sqrt and v_rcp: 1 ulp = 2 U each, as the
# kernel's comment says; every other operation correctly rounded: 1):
#   g:  the reference's carries the read-back (1) and its cast to fp32 (1), and
#       each side multiplies by the clip factor (1 + 1)                       4
#   m:  g's 4; g - m and w1m * (.) on each side (the final add's rounding on
#       each side is the bound's ulp(value) term)                             8
#   v:  g enters squared (8); w2v * g and (.) * g on each side (4)            12
#   p:  the change is the step -step_size m / den.
#       m, relative to itself: its 8 and the final add of each side          10
#       den: v's 12, the rounding of v * beta2 (the kernel may fuse it) and
#       the final add of each side (3), halved by the square root: 7.5;
#       v_sqrt 2 and the reference's sqrt 1; fl32(1 / sqrt(bc2)) and a
#       multiply against fl32(sqrt(bc2)) and a division (4); + eps on each
#       side (2)                                                             16.5
#       v_rcp 2, m * rcp 1, * step_size 1 (0 where it is fused into the add)
#       against -step_size * m and / den (2)                                 6
#       10 + 16.5 + 6 = 32.5                                                 33
# (test_gpu_train_batch.py has 16 U = 2^-20 for all three: there the gradient is
# the kernel's own output to the bit, here each side rounds g on its own and
# that reaches m once and v twice.)
C_M, C_V, C_P = 8 * U, 12 * U, 33 * U
_CACHE = {}


def _flat(wname):
    return tc.flat_params(tc.WEIGHTS[wname])


def _hip_lr0(case, wname):
    """The kernel's zero-state call at lr = 0, grad_clip = 0 of a case (cached): g', its norm, the metrics."""
    if ("hip", case, wname) not in _CACHE:
        flat = _flat(wname)
        _, rec, offs = sc.case_inputs(case)
        z = np.zeros_like(flat)
        out = sc.run_seq(flat, z, z, 0, rec, offs, lr=0.0, clip=0.0)
        out["grad"] = sc.grad_from_m(out["m"])
        _CACHE["hip", case, wname] = out
    return _CACHE["hip", case, wname]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("case", sc.CASES)
def test_gradient_value_and_norm_against_float64(case, wname):
    """One episode per call. err = max|g' - g64| / max|g64| of the kernel's
    pre-clip gradient is at most 4 x the same measure of torch's fp32 autograd on
    the GPU, never asked to be below 2^-22. Loss, mean |td|, mean V and the
    reward sum match float64 to 1e-4; on one record the V metric is that
    record's V, bounded as the batched test bounds V. The kernel's own norm
    against sqrt(sum g'^2) in float64: at most NORM_ROUNDINGS x 2^-24 on the
    squared sum. The call leaves the parameters bit for bit and step = 1."""
    flat = _flat(wname)
    _, rec, offs = sc.case_inputs(case)
    T = len(rec)
    r64 = sc.ref64(case, wname)
    hip = _hip_lr0(case, wname)
    g32, _, y32 = tc.torch_batched_grad(flat, rec, offs, GAMMA, torch.float32, device="cuda")
    gmax = np.abs(r64["grad"]).max()
    err_hip = np.abs(hip["grad"] - r64["grad"]).max() / gmax
    err_t32 = np.abs(g32 - r64["grad"]).max() / gmax
    met = hip["metrics"]
    sq64 = float((hip["grad"] ** 2).sum())
    err_norm = abs(float(met[1]) ** 2 - sq64) / sq64
    print(f"T={case}/{wname}: grad err hip {err_hip:.3e} torch32 {err_t32:.3e} | norm {met[1]:.6g} "
          f"(float64 {np.sqrt((r64['grad'] ** 2).sum()):.6g}) err on the square {err_norm / U:.2f} x 2^-24")
    assert np.isfinite(hip["m"]).all() and np.isfinite(hip["v"]).all() and hip["step"] == 1
    assert np.array_equal(hip["p"].view(np.uint32), flat.view(np.uint32))   # lr = 0: the parameters stay
    assert err_hip <= max(F32_FACTOR * err_t32, GRAD_FLOOR)
    assert err_norm <= NORM_ROUNDINGS * U
    want = {0: r64["loss"], 2: r64["td_error"], 3: r64["predicted_value"], 4: r64["reward"]}
    for k, w in want.items():
        assert met[k] == pytest.approx(w, rel=1e-4, abs=1e-5), k
    if T == 1:
        ymax = abs(r64["Y"][0])
        ey_hip = abs(met[3] - r64["Y"][0]) / ymax
        ey_t32 = abs(y32[0] - r64["Y"][0]) / ymax
        y_floor = Y_FLOOR_ULPS * float(np.spacing(np.float32(ymax))) / ymax
        print(f"  one record: V err hip {ey_hip:.3e} torch32 {ey_t32:.3e}")
        assert ey_hip <= max(y_floor, F32_FACTOR * ey_t32)


def _adam_bound_ok(name, got, ref, delta, c):
    """|got - ref| <= c |delta| + ulp(value); returns the worst |got - ref| / bound (<= 1: inside)."""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32)).astype(np.float64)
    bound = c * np.abs(delta.astype(np.float64)) + ulp
    diff = np.abs(got - ref)
    k = int(np.argmax(diff / bound))
    print(f"  {name}: max |diff| {diff.max():.3e}, differing {np.count_nonzero(diff)}, worst |diff| / bound "
          f"{diff[k] / bound[k]:.3f} (bound there {bound[k]:.3e})")
    assert (diff - bound).max() <= 0.0, (name, float((diff - bound).max()))
    return float(diff[k] / bound[k])


def _check_adam(label, case, wname, m0, v0, step0, clip):
    """A second run of a case at lr = 1e-3 against adam_reference on the
    kernel's own g' and norm (from the lr = 0 run): p, m, v inside their bounds."""
    from bgx.train_ref import adam_reference
    flat = _flat(wname)
    _, rec, offs = sc.case_inputs(case)
    lr0 = _hip_lr0(case, wname)
    got = sc.run_seq(flat, m0, v0, step0, rec, offs, lr=LR, clip=clip)
    r = adam_reference(flat, m0, v0, step0, lr0["grad"], LR, clip, norm=lr0["metrics"][1])
    print(f"{label} T={case}/{wname}: kernel norm {float(r['norm']):.6g} scale {float(r['scale']):.6g} "
          f"step {r['step']}")
    assert got["step"] == r["step"] == step0 + 1
    ex = [_adam_bound_ok("params", got["p"], r["params"], r["u"], C_P),
          _adam_bound_ok("m", got["m"], r["m"], r["m"] - np.asarray(m0, np.float32), C_M),
          _adam_bound_ok("v", got["v"], r["v"], r["v"] - np.asarray(v0, np.float32), C_V)]
    print(f"  row {label} T={case}/{wname}: worst |diff| / bound p {ex[0]:.2f} m {ex[1]:.2f} v {ex[2]:.2f}")
    assert max(ex) <= 1.0, ex
    assert not np.array_equal(got["p"], flat)
    for k in (0, 2, 3, 4):                            # the forward pass does not depend on lr or the clip
        assert got["metrics"][k] == lr0["metrics"][k], k
    return got, r


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("case", sc.CASES)
def test_clip_and_adam_step_against_fp32_restatement(case, wname):
    """grad_clip = 1 from zero moments, every case. A clip case (float64 norm
    outside [0.95, 1.05]) must take its branch: the factor below 1 and the norm
    metric norm * factor, or the factor exactly 1 and the norm metric the norm."""
    z = np.zeros_like(_flat(wname))
    got, r = _check_adam("clip 1", case, wname, z, z, 0, 1.0)
    norm64 = float(np.sqrt((sc.ref64(case, wname)["grad"] ** 2).sum()))
    if case in sc.CLIP_ACTIVE[wname]:
        assert norm64 > 1.05 and float(r["scale"]) < 1.0
        assert got["metrics"][1] == pytest.approx(float(r["norm"]) * float(r["scale"]), rel=1e-6)
        assert got["metrics"][1] == pytest.approx(1.0, rel=1e-5)
    elif case in sc.CLIP_INACTIVE[wname]:
        assert norm64 < 0.95 and float(r["scale"]) == 1.0
        assert got["metrics"][1] == float(r["norm"])
    else:
        assert (case, wname) == (64, "seed0")         # the one case inside the band


@pytest.mark.parametrize("case,wname", [(129, "seed0"), (1, "ckpt")])
def test_clip_off_leaves_a_large_gradient_unscaled(case, wname):
    """grad_clip = 0 on a case whose norm exceeds 1: the factor is 1."""
    assert case in sc.CLIP_ACTIVE[wname]
    z = np.zeros_like(_flat(wname))
    got, r = _check_adam("clip off", case, wname, z, z, 0, 0.0)
    assert float(r["norm"]) > 1.05 and float(r["scale"]) == 1.0
    assert got["metrics"][1] == float(r["norm"])      # the norm metric is the unscaled norm, to the bit


@pytest.mark.parametrize("step0", [7, 100000])
@pytest.mark.parametrize("case,wname", [(129, "seed0"), (129, "ckpt")])
def test_adam_step_from_a_non_zero_state(case, wname, step0):
    """Moments drawn as in the batched test, step 7 and step 100,000 (both bias
    corrections near 1), one clipping case and one not."""
    flat = _flat(wname)
    rng = np.random.default_rng(4)
    m0 = (rng.standard_normal(len(flat)) * 1e-3).astype(np.float32)
    v0 = (rng.random(len(flat)) * 1e-5).astype(np.float32)
    _, r = _check_adam(f"step {step0}", case, wname, m0, v0, step0, 1.0)
    assert (float(r["scale"]) < 1.0) == (case in sc.CLIP_ACTIVE[wname])


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_several_episodes_in_one_launch(wname):
    """Lengths 1, 65, 64, 3, 130 at lr = 1e-3, clip 1. One call over the five
    equals five calls of one episode each that carry p, m, v and step, bit for
    bit (the small parameters and their moments stay in registers across the
    episodes of a launch; a launch of one writes them back), the metrics to
    1e-12. The same call twice is bit-identical. Against the torch backend's
    sequential update on the GPU: within 4 x what torch's parameters differ
    from a float64 chain of the same five updates."""
    from bgx.trainer import DeviceTrainer
    flat = _flat(wname)
    hdr, rec, offs = tc.synth(list(sc.MULTI_LENS), seed=sc.MULTI_SEED)
    z = np.zeros_like(flat)
    one = sc.run_seq(flat, z, z, 0, rec, offs)
    again = sc.run_seq(flat, z, z, 0, rec, offs)
    for k in ("p", "m", "v", "metrics"):
        assert np.array_equal(one[k], again[k]), k
    assert one["step"] == again["step"] == 5
    p, m, v, step, met = flat, z, z, 0, np.zeros(5)
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        o = sc.run_seq(p, m, v, step, rec[a:b], [0, b - a])
        p, m, v, step, met = o["p"], o["m"], o["v"], o["step"], met + o["metrics"]
    assert step == 5
    for name, x, y in (("p", one["p"], p), ("m", one["m"], m), ("v", one["v"], v)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    assert one["metrics"] == pytest.approx(met, rel=1e-12)
    p64, step64 = sc.chain64(flat, rec, offs)
    assert step64 == 5
    pm_t = _PM(tc.state_dict(flat))
    tt = DeviceTrainer(pm_t, device="cuda", batch_episode_size=5, backend="torch")
    assert not tt.batched
    tt.update_records(hdr, rec)
    p_t = pm_t.flat().astype(np.float64)
    dev_t = np.abs(p_t - p64).max()
    dev_h = np.abs(one["p"].astype(np.float64) - p_t).max()
    print(f"{wname}: torch vs fp64 {dev_t:.3e}, hip vs torch {dev_h:.3e}, hip vs fp64 "
          f"{np.abs(one['p'] - p64).max():.3e}, moved {np.abs(p64 - flat).max():.3e}")
    assert dev_h <= F32_FACTOR * dev_t


def test_update_records_checks_in_front_of_the_kernel():
    """DeviceTrainer(batched=False, backend="hip").update_records raises
    ValueError when the headers count more or fewer records than were passed
    (here a leading slice of a device tensor that holds them all) and for an
    episode of 2,049 records; one of 2,048 trains and advances the step."""
    from bgx.trainer import DeviceTrainer
    sd0 = tc.state_dict(_flat("seed0"))
    hdr, rec, _ = tc.synth(list(sc.MULTI_LENS), seed=sc.MULTI_SEED)
    rec_dev = torch.from_numpy(rec.view(np.int32)).to("cuda")
    pm = _PM(sd0)
    t = DeviceTrainer(pm, device="cuda", batch_episode_size=5, batched=False, backend="hip")
    with pytest.raises(ValueError, match="count 263 records, got 262"):
        t.update_records(hdr, rec_dev[:-1])
    fewer = hdr.copy()
    fewer[4, 3] -= 1
    with pytest.raises(ValueError, match="count 262 records, got 263"):
        t.update_records(fewer, rec_dev)
    hdr9, rec9, _ = tc.synth([2049], seed=31)
    with pytest.raises(ValueError, match="more than 2048"):
        t.update_records(hdr9, rec9)
    assert np.array_equal(pm.flat(), _flat("seed0")) and t._flat is None   # nothing ran
    hdr8, rec8, _ = sc.case_inputs(2048)
    met = t.update_records(hdr8, rec8)
    assert int(t._flat["step"].item()) == 1 and met["episodes"] == 1 and met["episode_length"] == 2048.0
    assert met["loss"] == pytest.approx(sc.ref64(2048, "seed0")["loss"], rel=1e-4)
    assert not np.array_equal(pm.flat(), _flat("seed0"))
