"""CPU checks of the batched TD(lambda) update: the numpy checkers
(bgx/train_ref.py: lambda_returns, batched_td0_reference(lam)), the argument
rules of bgx_tdlambda_batch_workspace / bgx_tdlambda_update_batched (every
rejection comes before the device is touched) and of DeviceTrainer(lam=), and
the target stage itself (csrc/bgx_train_lambda.hip) on the host emulation
(tests/cpuwave/lambda_emu.cpp) under AddressSanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG

import train_batch_cases as tc
import train_lambda_cases as lc
from test_cpuwave import CLANG, HERE, REPO, _emu_sources

LIB = os.path.join(PKG, "bgx", "libbgx.so")
GAMMA = lc.GAMMA
ENV = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    import bgx
    return bgx.lib()


def _plain_returns(Y, rew, offs, gamma, lam):
    """The recurrence as a plain Python double loop."""
    out = [0.0] * len(Y)
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        out[b - 1] = float(rew[b - 1])
        for s in range(b - 2, a - 1, -1):
            out[s] = float(rew[s]) + gamma * ((1.0 - lam) * float(Y[s + 1]) + lam * out[s + 1])
    return np.array(out)


def test_lambda_returns_float64():
    """lambda_returns in float64 on lengths 1, 2, 7 and 30: equal to a plain
    Python double loop (to the last bits: the same operations in the same
    order); at lam = 0 exactly batched_td0_reference's TD(0) target; at lam = 1
    the same under two weight sets (the return does not depend on Y)."""
    from bgx.train_ref import batched_td0_reference, lambda_returns
    _, rec, offs = tc.synth([1, 2, 7, 30], seed=6)
    rew = lc.rewards(rec).astype(np.float64)
    refs = {w: batched_td0_reference(tc.flat_params(tc.WEIGHTS[w]), rec, offs, GAMMA) for w in tc.WEIGHTS}
    for w, r in refs.items():
        for lam in (0.0, 0.3, 0.7, 1.0):
            got = lambda_returns(r["Y"], rew, offs, GAMMA, lam)
            assert got.dtype == np.float64
            assert np.abs(got - _plain_returns(r["Y"], rew, offs, GAMMA, lam)).max() <= 1e-15 * np.abs(got).max()
        assert np.array_equal(lambda_returns(r["Y"], rew, offs, GAMMA, 0.0), r["target"])
        assert lambda_returns(r["Y"].astype(np.float32), rew, offs, GAMMA, 0.7).dtype == np.float32
    g1 = [lambda_returns(refs[w]["Y"], rew, offs, GAMMA, 1.0) for w in tc.WEIGHTS]
    assert not np.array_equal(refs["seed0"]["Y"], refs["ckpt"]["Y"])
    assert np.array_equal(g1[0], g1[1])
    # the Monte-Carlo return by hand on the episode of length 2
    assert g1[0][1] == rew[1] + GAMMA * rew[2] and g1[0][2] == rew[2]
    # the default leaves batched_td0_reference as it was, and lam reaches its target
    r7 = batched_td0_reference(tc.flat_params(tc.WEIGHTS["seed0"]), rec, offs, GAMMA, lam=0.7)
    assert np.array_equal(r7["target"], lambda_returns(refs["seed0"]["Y"], rew, offs, GAMMA, 0.7))
    assert not np.array_equal(r7["grad"], refs["seed0"]["grad"])
    r0 = batched_td0_reference(tc.flat_params(tc.WEIGHTS["seed0"]), rec, offs, GAMMA, lam=0.0)
    assert np.array_equal(r0["grad"], refs["seed0"]["grad"]) and r0["loss"] == refs["seed0"]["loss"]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_reference_gradient_equals_float64_autograd(wname):
    """batched_td0_reference(lam=0.7) against torch CPU float64 autograd of the
    same loss with the targets fed in detached: E = 3, lengths 1, 2 and 7."""
    from bgx.train_ref import batched_td0_reference
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = tc.synth([1, 2, 7], seed=5)
    ref = batched_td0_reference(flat, rec, offs, GAMMA, lam=0.7)
    grad, loss, y, tgt = lc.torch_lambda_grad(flat, rec, offs, GAMMA, 0.7, torch.float64)
    assert ref["grad"].shape == (25601,) and ref["grad"].dtype == np.float64
    assert np.abs(ref["grad"] - grad).max() <= 1e-12 * np.abs(grad).max()
    assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ref["Y"] - y).max() <= 1e-12
    assert np.abs(ref["target"] - tgt).max() <= 1e-12


def test_workspace_query(L):
    b, old = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.bgx_tdlambda_batch_workspace(0, ctypes.byref(b)) == -1
    assert L.bgx_tdlambda_batch_workspace(-5, ctypes.byref(b)) == -1
    assert L.bgx_tdlambda_batch_workspace(1, None) == -1
    prev = 0
    for n in (1, 2, 127, 128, 129, 1000, 65543, 10 ** 6, 2 ** 31 - 1):
        assert L.bgx_tdlambda_batch_workspace(n, ctypes.byref(b)) == 0
        assert L.bgx_td0_batch_workspace(n, ctypes.byref(old)) == 0
        assert b.value >= prev and b.value % 16 == 0, n
        assert b.value >= old.value + 4 * n, n   # the TD(0) workspace and G of every record
        prev = b.value


def test_update_rejects_bad_arguments_before_the_device(L):
    """Each rule of include/bgx.h on its own; the other arguments are non-null
    (never dereferenced: the rejection comes first)."""
    need, old = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.bgx_tdlambda_batch_workspace(10, ctypes.byref(need)) == 0
    assert L.bgx_td0_batch_workspace(10, ctypes.byref(old)) == 0
    P = 0x10000   # a non-null, 16-byte aligned stand-in
    good = dict(rec=P, offs=P, n_eps=2, n_rec=10, params=P, m=P, v=P, step=P, lam=0.7, metrics=P, grad=None,
                target=None, work=P, bytes=need.value)

    def call(**kw):
        a = dict(good, **kw)
        return L.bgx_tdlambda_update_batched(a["rec"], a["offs"], a["n_eps"], a["n_rec"], a["params"], a["m"],
                                             a["v"], a["step"], 1e-3, 0.99, a["lam"], 1.0, a["metrics"], a["grad"],
                                             a["target"], a["work"], a["bytes"], None)

    for k in ("rec", "offs", "params", "m", "v", "step", "metrics", "work"):
        assert call(**{k: None}) == -1, k
        assert b"null" in L.bgx_last_error()
    for lam in (-0.1, 1.5, float("nan")):
        assert call(lam=lam) == -1, lam
        assert b"lambda" in L.bgx_last_error()
    assert call(n_eps=0) == -1
    assert call(n_eps=-3) == -1
    assert call(n_eps=11) == -1          # n_records < n_eps
    assert call(bytes=need.value - 1) == -1
    assert b"work_bytes" in L.bgx_last_error()
    assert call(bytes=old.value) == -1   # the TD(0) call's workspace is too small
    assert call(bytes=0) == -1
    assert call(work=P + 8) == -1
    assert b"aligned" in L.bgx_last_error()


def test_abi_version_unchanged(L):
    assert L.bgx_abi_version() == 10


def test_device_trainer_lam_rules():
    """lam outside [0, 1] (or NaN) is rejected at construction; lam != 0 on the
    sequential HIP backend when the update is called, with both ways out named;
    lam = 0 constructs on every backend and is the default."""
    import inspect
    from bgx.net import BackgammonPolicyNetwork
    from bgx.trainer import DeviceTrainer
    assert inspect.signature(DeviceTrainer.__init__).parameters["lam"].default == 0.0

    class PM:
        def get_parameters(self, device=None):
            return BackgammonPolicyNetwork().state_dict()

        def set_parameters(self, sd):
            pass

    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            DeviceTrainer(PM(), device="cpu", lam=bad)
    assert DeviceTrainer(PM(), device="cpu").lam == 0.0
    assert DeviceTrainer(PM(), device="cpu", batched=True, backend="hip", lam=1.0).lam == 1.0
    hdr, rec, _ = tc.synth([2, 3], seed=1)
    t = DeviceTrainer(PM(), device="cpu", lam=0.7)
    assert t.backend == "hip" and not t.batched
    with pytest.raises(ValueError, match="batched=True.*backend='torch'"):
        t.update_records(hdr, rec)


def test_torch_backend_honours_lam_on_the_cpu():
    """_episode_terms: the target of an episode is lambda_returns on the detached
    y (fp32), the last record's its reward; lam = 0 keeps the TD(0) target."""
    from bgx.train_ref import encode_records, lambda_returns
    from bgx.trainer import DeviceTrainer

    class PM:
        def get_parameters(self, device=None):
            return tc.state_dict(tc.flat_params(tc.WEIGHTS["seed0"]))

        def set_parameters(self, sd):
            pass

    _, rec, offs = tc.synth([1, 7], seed=2)
    obs = torch.from_numpy(encode_records(rec))
    rew = torch.from_numpy(lc.rewards(rec))
    for lam in (0.0, 0.7, 1.0):
        t = DeviceTrainer(PM(), device="cpu", backend="torch", batched=True, lam=lam)
        for e in range(2):
            a, b = int(offs[e]), int(offs[e + 1])
            y, tgt = t._episode_terms(obs, rew, a, b)
            assert y.requires_grad and not tgt.requires_grad and tgt.dtype == torch.float32
            want = lambda_returns(y.detach().reshape(-1).numpy(), rew[a:b].numpy(), [0, b - a], GAMMA, lam)
            assert np.array_equal(tgt.reshape(-1).numpy(), want), (lam, e)


# ---------------------------------------------------------------- the target stage, emulated
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    tmp = tmp_path_factory.mktemp("lambda_emu")
    src = _emu_sources(tmp)
    exe = tmp / "lambda_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address", "-fno-omit-frame-pointer",
                    "-I" + str(src), "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "include"),
                    "-x", "c++", os.path.join(HERE, "cpuwave", "lambda_emu.cpp"), "-o", str(exe), "-pthread"],
                   check=True, capture_output=True, text=True)
    return tmp, exe


N_PAST = 5   # records after the last episode: in no episode, their target stays 0
_HARVEST = {}


def _harvest(name):
    """(records with N_PAST more at the end, offs) of the two emulated harvests."""
    if name not in _HARVEST:
        lens = lc.EDGE_LENS if name == "edges" else tc.ragged_lens(20000, 31)[:300]
        _, rec, offs = tc.synth(lens, seed=40 + len(lens))
        extra = tc.base_records()[:N_PAST].copy()
        extra[:, 9] = np.float32([1.5] * N_PAST).view(np.uint32)
        _HARVEST[name] = (np.concatenate([rec, extra]), offs)
    return _HARVEST[name]


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("name", ["edges", "ragged300"])
def test_target_stage_emulated_against_float64(emu, name, wname):
    """tl_target_kernel through its launcher on the emulated grid (16 workgroups
    of 4 waves: the 300-episode harvest gives every wave several episodes), lam
    in {0, 0.7, 1}. Y is the fp32 rounding of the float64 forward pass; G64 is
    the float64 recurrence on that Y. err = max|tgt - G64| / max|G64| is at most
    max(2 fp32 ulps of max|G64|, 4 x the err of the serial fp32 lambda_returns on
    the same Y). target_out equals tgt; the records past the last episode keep
    0 (both buffers start as 7); AddressSanitizer reports nothing."""
    from bgx.train_ref import batched_td0_reference, lambda_returns
    tmp, exe = emu
    rec, offs = _harvest(name)
    n, n_in = len(rec), int(offs[-1])
    assert n == n_in + N_PAST and (name != "ragged300" or len(offs) - 1 == 300)
    y32 = batched_td0_reference(tc.flat_params(tc.WEIGHTS[wname]), rec[:n_in], offs, GAMMA)["Y"].astype(np.float32)
    y32 = np.concatenate([y32, np.float32([0.25] * N_PAST)])
    rew = lc.rewards(rec)
    tag = f"{name}_{wname}"
    rec.tofile(tmp / f"rec_{tag}.bin")
    offs.astype(np.int32).tofile(tmp / f"offs_{tag}.bin")
    y32.tofile(tmp / f"y_{tag}.bin")
    for lam in (0.0, 0.7, 1.0):
        out = tmp / f"out_{tag}_{lam}.bin"
        r = subprocess.run([str(exe), str(tmp / f"rec_{tag}.bin"), str(tmp / f"offs_{tag}.bin"),
                            str(tmp / f"y_{tag}.bin"), repr(GAMMA), repr(lam), str(out)],
                           capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode == 0 and not r.stderr, (lam, r.returncode, r.stderr[-3000:])
        got = np.fromfile(out, np.float32).reshape(2, n)
        g64 = lambda_returns(y32.astype(np.float64), rew.astype(np.float64), offs, GAMMA, lam)
        g32 = lambda_returns(y32, rew, offs, GAMMA, lam)
        err, err32 = lc.rel_err(got[0][:n_in], g64[:n_in]), lc.rel_err(g32[:n_in], g64[:n_in])
        print(f"{tag} lam {lam}: records {n_in} episodes {len(offs) - 1} target err emulated {err:.3e} "
              f"serial fp32 {err32:.3e}")
        assert np.array_equal(got[0], got[1])
        assert not got[0][n_in:].any()
        assert np.isfinite(got[0]).all()
        assert err <= max(lc.floor_rel(g64[:n_in]), lc.F32_FACTOR * err32)
        if lam == 0.0:   # c = 0: the chain is fma(gamma, Y[s + 1], r)
            assert err <= lc.floor_rel(g64[:n_in])
