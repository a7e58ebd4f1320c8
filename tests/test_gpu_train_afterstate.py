"""bgx_td_afterstate_update_batched (the afterstate instances of the index,
forward and backward kernels of csrc/bgx_train_batch.hip, loader in
csrc/bgx_train_tile.h) on the GPU.

The main check needs no tolerance: the call on (records, headers) leaves the
bits that bgx_td_update_batched leaves on records whose words 0..6 were
replaced on the host by their afterstate rows (bgx.records.packed_afterstates):
parameters, both moments, step, the five metrics, gradient, targets and V, after
one call and after a second one on the updated state. Then reproducibility,
argument errors, V of the afterstate rows against the engine's own V(a) (record
word 8) on harvested self-play, and DeviceTrainer(afterstates=True) end to end
with the bounds of test_gpu_train_lambda.py.

The inputs (train_afterstate_cases.py) carry random indicator bits in the
headers and in every record's word 6: a loader that trusted them would show."""
import numpy as np
import pytest
import torch

import train_afterstate_cases as ac
import train_batch_cases as tc
import train_lambda_cases as lc
from train_gpu_runner import AFTER, TD, _PM, _adam64, _state, device_args, run
from train_zero_sum_cases import TDF_ZERO_SUM as ZS

pytestmark = pytest.mark.gpu

GAMMA, LR = lc.GAMMA, 1e-3
F32_FACTOR = lc.F32_FACTOR
E_ARG = -1      # BGX_E_ARG
_CACHE = {}
CASES = list(ac.EMU_LENS) + ["two_tiles_each", "trailing"]
ALL = ("p", "m", "v", "grad", "metrics", "Y", "target")


def _inputs(case):
    """(headers, records, offs, records rewritten on the host) of a case, built once."""
    if case not in _CACHE:
        if case == "two_tiles_each":   # every workgroup of the largest grid takes two tiles, ragged episodes
            from bgx.trainer import DeviceTrainer
            tile, grid = DeviceTrainer.batch_shape()
            assert tile == ac.TILE
            hdr, rec, offs = ac.synth_after(tc.ragged_lens(2 * grid * tile + 7, 11), seed=61)
        elif case == "trailing":
            hdr, rec, offs = ac.synth_after(ac.EMU_LENS[ac.TRAILING[0]], seed=62, trailing=ac.TRAILING[1])
        else:
            hdr, rec, offs = ac.synth_after(ac.EMU_LENS[case], seed=50 + CASES.index(case))
        _CACHE[case] = (hdr, rec, offs, ac.rewritten(hdr, rec, offs))
    return _CACHE[case]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("flags", [0, ZS], ids=["plain", "zero_sum"])
@pytest.mark.parametrize("lam", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_the_existing_call_on_rewritten_records(case, lam, flags, wname):
    """From equal non-zero parameters and moments, lr = 1e-3: one call, then a
    second one on the updated state. Records in no episode (the trailing case)
    keep their own words in both calls' inputs; V and the targets are compared on
    the covered records."""
    flat = tc.flat_params(tc.WEIGHTS[wname])
    hdr, rec, offs, rec2 = _inputs(case)
    covered = int(offs[-1])
    m0, v0 = _state(len(flat), 4)
    a = {"p": flat, "m": m0, "v": v0, "step": 7}
    b = dict(a)
    for call in range(2):
        a = run(AFTER, a["p"], a["m"], a["v"], a["step"], rec, offs, lam, flags, hdr=hdr)
        b = run(TD, b["p"], b["m"], b["v"], b["step"], rec2, offs, lam, flags)
        for k in ALL:
            x, y = (a[k][:covered], b[k][:covered]) if k in ("Y", "target") else (a[k], b[k])
            assert np.isfinite(x).all(), (call, k)
            np.testing.assert_array_equal(x, y, err_msg=f"call {call + 1}: {k}")
        assert a["step"] == b["step"] == 8 + call
    assert not np.array_equal(a["p"], flat)
    if case == "trailing":   # a record in no episode: target 0, as the existing call leaves it
        assert not a["target"][covered:].any() and not b["target"][covered:].any()


def test_same_call_twice_is_bit_identical():
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    hdr, rec, offs, _ = _inputs("two_tiles_each")
    m0, v0 = _state(len(flat), 8)
    a = run(AFTER, flat, m0, v0, 3, rec, offs, 0.7, ZS, hdr=hdr)
    b = run(AFTER, flat, m0, v0, 3, rec, offs, 0.7, ZS, hdr=hdr)
    for k in ALL:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["step"] == b["step"] == 4 and not np.array_equal(a["p"], flat)
    # the rows are not the records' own: the existing call on the records as they are gives another V
    plain = run(TD, flat, m0, v0, 3, rec, offs, 0.7, ZS)
    assert not np.array_equal(plain["Y"], a["Y"]) and not np.array_equal(plain["p"], a["p"])


def test_argument_errors_leave_the_state_untouched():
    """A null d_headers, flags = 2, lambda outside [0, 1] (and NaN) and work_bytes
    one short are BGX_E_ARG, before the device is touched."""
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    hdr, rec, offs, _ = _inputs("ragged_tile")
    m0, v0 = _state(len(flat), 6)
    from bgx import ops
    d = device_args(AFTER, flat, m0, v0, 5, rec, offs, hdr=hdr)
    p, m, v, step = d["state"]

    def call(**kw):   # the return code
        return ops.td_batched_call(AFTER, **{**d, "lr": LR, "gamma": GAMMA, "clip": 1.0, **kw})

    bad = [dict(lam=0.7, flags=0, headers=None), dict(lam=0.7, flags=2), dict(lam=0.7, flags=ZS | 2),
           dict(lam=-0.01, flags=0), dict(lam=1.01, flags=ZS), dict(lam=float("nan"), flags=0),
           dict(lam=0.7, flags=ZS, work_bytes=d["work"].numel() - 1)]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    np.testing.assert_array_equal(p.cpu().numpy(), flat)
    np.testing.assert_array_equal(m.cpu().numpy(), m0)
    np.testing.assert_array_equal(v.cpu().numpy(), v0)
    assert int(step.item()) == 5 and not d["metrics"].cpu().numpy().any()
    assert np.isnan(d["grad_out"].cpu().numpy()).all() and np.isnan(d["target_out"].cpu().numpy()).all()
    # the same tensors with valid arguments are accepted
    assert call(lam=0.7, flags=ZS) == 0
    torch.cuda.synchronize()
    assert int(step.item()) == 6


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_afterstate_values_are_the_engines_own(wname):
    """A 64-lane 1-ply engine, sampled play, fixed weights, stepped until at least
    20 episodes are harvested. With those weights as d_params, V of the afterstate
    call equals record word 8, the engine's V(a), within 1e-5 on EVERY record (the
    project's bound for the split-fp16 forward against fp32 on these two weight
    sets); as the control, V of bgx_td_update_batched equals word 7, V(s), within
    the same bound. Last records take the header's final board; a pass between
    two records of one mover leaves the next record's board as the afterstate."""
    from bgx import Engine
    w = tc._load(tc.WEIGHTS[wname])
    e = Engine(lanes=64, seed=3, ply=1)
    e.set_weights({k: w[k] for k in ("W1", "b1", "w2", "b2")}, temperature=1.5, version=1)
    hdrs, recs = [], []
    for _ in range(40):
        e.step(100)
        h = e.harvest()
        hdrs.append(h.headers.cpu().numpy().view(np.uint32).reshape(-1, 16))
        recs.append(h.records.cpu().numpy().view(np.uint32).reshape(-1, 12))
        if sum(len(x) for x in hdrs) >= 20:
            break
    e.sync()
    e.close()
    hdr, rec = np.concatenate(hdrs), np.concatenate(recs)
    lens = hdr[:, 3].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    assert len(hdr) >= 20 and offs[-1] == len(rec) and (lens >= 1).all()
    flat = tc.flat_params(tc.WEIGHTS[wname])
    z = np.zeros_like(flat)
    after = run(AFTER, flat, z, z, 0, rec, offs, 0.7, ZS, lr=0.0, hdr=hdr)
    before = run(TD, flat, z, z, 0, rec, offs, 0.7, ZS, lr=0.0)
    f = rec[:, 7:9].copy().view(np.float32)
    err_a, err_s = np.abs(after["Y"] - f[:, 1]), np.abs(before["Y"] - f[:, 0])
    mv = ac.movers_of(rec)
    same_mover = int((mv[1:] == mv[:-1])[np.setdiff1d(np.arange(len(rec) - 1), offs[1:] - 1)].sum())
    print(f"{wname}: {len(hdr)} episodes, {len(rec)} records, {same_mover} after a pass; max |V(A) - word 8| "
          f"{err_a.max():.3e}, max |V(s) - word 7| {err_s.max():.3e}, max |word 8 - word 7| {np.abs(f[:, 1] - f[:, 0]).max():.3e}")
    assert err_a.max() <= 1e-5
    assert err_s.max() <= 1e-5
    assert np.abs(f[:, 1] - f[:, 0]).max() > 1e-3   # the two columns are different numbers


def test_trainer_hip_against_torch_backend_and_backend_swaps():
    """DeviceTrainer(batched=True, afterstates=True, zero_sum=True, lam=0.7): 5
    updates of 40 episodes on backend "hip" and on "torch" from the same weights,
    with the bounds and measures of test_gpu_train_lambda.py: the parameters
    differ by at most 4 x what torch's differ from a float64 run of the same
    updates (batched_td0_reference(afterstates=True) and Adam in float64); loss,
    grad_norm and td_error agree to 1e-4. A trainer that swaps backends every
    update stays under the same bound. An afterstates=False trainer's first loss
    on the same batch is another."""
    from bgx.train_ref import batched_td0_reference
    from bgx.trainer import DeviceTrainer
    lam = 0.7
    flat0 = tc.flat_params(tc.WEIGHTS["seed0"])
    sd0 = tc.state_dict(flat0)
    batches = [ac.synth_after(np.random.default_rng(300 + k).integers(5, 86, 40), seed=200 + k) for k in range(5)]
    pm_h, pm_t, pm_s, pm_0 = _PM(sd0), _PM(sd0), _PM(sd0), _PM(sd0)
    kw = dict(device="cuda", batch_episode_size=40, batched=True, lam=lam, zero_sum=True)
    th = DeviceTrainer(pm_h, backend="hip", afterstates=True, **kw)
    tt = DeviceTrainer(pm_t, backend="torch", afterstates=True, **kw)
    ts = DeviceTrainer(pm_s, backend="hip", afterstates=True, **kw)
    t0 = DeviceTrainer(pm_0, backend="hip", **kw)
    assert th.backend == "hip" and tt.backend == "torch" and th.afterstates and tt.afterstates and not t0.afterstates
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
        r = batched_td0_reference(p64, rec, offs, GAMMA, lam=lam, zero_sum=True, afterstates=True, headers=hdr)
        p64, m64, v64, s64 = _adam64(p64, m64, v64, s64, r["grad"], LR, 1.0)
        dev_t = np.abs(pm_t.flat() - p64).max()
        dev_h = np.abs(pm_h.flat().astype(np.float64) - pm_t.flat()).max()
        dev_s = np.abs(pm_s.flat().astype(np.float64) - pm_t.flat()).max()
        print(f"update {k + 1}: torch vs fp64 {dev_t:.3e}, hip vs torch {dev_h:.3e}, swapping vs torch {dev_s:.3e}; "
              f"loss hip {mh['loss']:.6g} torch {mt['loss']:.6g} fp64 {r['loss']:.6g} | afterstates=False {m0['loss']:.6g}")
        assert dev_h <= F32_FACTOR * dev_t
        assert dev_s <= F32_FACTOR * dev_t
        assert mh["loss"] == pytest.approx(mt["loss"], rel=1e-4)
        assert mh["loss"] == pytest.approx(r["loss"], rel=1e-4)
        assert mh["grad_norm"] == pytest.approx(mt["grad_norm"], rel=1e-4)
        assert mh["td_error"] == pytest.approx(mt["td_error"], rel=1e-4)
        assert set(mh) == set(mt) and mh["episodes"] == 40 and mh["win_counts"] == mt["win_counts"]
        assert mh["episode_length"] == mt["episode_length"]


def test_trainer_option_checks_and_the_episode_path():
    """A non-bool afterstates and the sequential HIP backend are ValueErrors. With
    the torch backend, update(episodes) equals update_records bit for bit,
    batched and sequential: the Episodes come from the same records through
    bgx.episodes.episodes_from_arrays (their indicator is the mover's, as in
    engine records: the Episode path reads the mover from feature 197)."""
    from bgx.episodes import episodes_from_arrays
    from bgx.trainer import DeviceTrainer
    from environments import Episode, Experience, Player
    flat0 = tc.flat_params(tc.WEIGHTS["ckpt"])
    sd0 = tc.state_dict(flat0)
    with pytest.raises(ValueError, match="afterstates must be a bool"):
        DeviceTrainer(_PM(sd0), device="cuda", afterstates=1)
    hdr, rec, offs = ac.synth_after(np.random.default_rng(7).integers(1, 30, 12), seed=70, random_indicator=False)
    seq = DeviceTrainer(_PM(sd0), device="cuda", batch_episode_size=12, afterstates=True)
    assert seq.backend == "hip" and not seq.batched
    with pytest.raises(ValueError, match="afterstates=True"):
        seq.update_records(hdr, rec)
    assert seq.total_episodes == 0
    eps = episodes_from_arrays(hdr, torch.from_numpy(rec.view(np.int32)).cuda(), Episode, Experience, Player)
    for batched in (True, False):
        for zero_sum, lam in ((True, 0.7), (False, 0.0)):
            kw = dict(device="cuda", batch_episode_size=12, batched=batched, backend="torch", lam=lam,
                      zero_sum=zero_sum, afterstates=True)
            pm_r, pm_e, pm_b = _PM(sd0), _PM(sd0), _PM(sd0)
            mr = DeviceTrainer(pm_r, **kw).update_records(hdr, rec)
            me = DeviceTrainer(pm_e, **kw).update(eps)
            DeviceTrainer(pm_b, **{**kw, "afterstates": False}).update_records(hdr, rec)
            np.testing.assert_array_equal(pm_r.flat(), pm_e.flat())
            # (the synthetic records carry no win type, which the Episode path counts; the headers do)
            assert {k: v for k, v in mr.items() if k != "win_counts"} == \
                   {k: v for k, v in me.items() if k != "win_counts"}, (batched, zero_sum)
            assert not np.array_equal(pm_r.flat(), pm_b.flat())
