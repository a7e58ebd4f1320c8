"""CPU checks of the zero-sum targets of the batched trainer: the numpy checkers
(bgx/train_ref.py: lambda_returns(movers=), batched_td0_reference(zero_sum=)),
the argument rules of bgx_td_update_batched (every rejection comes before the
device is touched) and of DeviceTrainer(zero_sum=), and both instances of the
target stage (csrc/bgx_train_lambda.hip) on the host emulation
(tests/cpuwave/zs_emu.cpp) under AddressSanitizer."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import PKG

import train_batch_cases as tc
import train_lambda_cases as lc
import train_zero_sum_cases as zc
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


def _plain_zero_sum_returns(Y, rew, offs, gamma, lam, movers):
    """The definition as a plain Python double loop."""
    out = [0.0] * len(Y)
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        out[b - 1] = float(rew[b - 1])
        for s in range(b - 2, a - 1, -1):
            y, g = float(Y[s + 1]), out[s + 1]
            if int(movers[s]) != int(movers[s + 1]):
                y, g = 1.0 - y, 1.0 - g
            out[s] = float(rew[s]) + gamma * ((1.0 - lam) * y + lam * g)
    return np.array(out)


def test_lambda_returns_movers_float64():
    """lambda_returns(movers=) in float64 on lengths 1, 2, 7 and 30: equal to a
    plain Python double loop of the definition under every mover pattern;
    movers=None and one mover everywhere give today's result bit for bit; the
    episode of length 2 with movers (0, 1) by hand."""
    from bgx.train_ref import batched_td0_reference, lambda_returns, record_movers
    _, rec, offs = tc.synth([1, 2, 7, 30], seed=6)
    rew = lc.rewards(rec).astype(np.float64)
    assert np.array_equal(record_movers(rec), zc.movers_of(rec))
    Y = batched_td0_reference(tc.flat_params(tc.WEIGHTS["seed0"]), rec, offs, GAMMA)["Y"]
    flips = 0
    for pattern in ("drawn", "alternating", "equal", "runs3"):
        mv = zc.pattern_movers(rec, offs, pattern)
        flips += int((mv[1:] != mv[:-1]).sum())
        for lam in (0.0, 0.3, 0.7, 1.0):
            got = lambda_returns(Y, rew, offs, GAMMA, lam, movers=mv)
            want = _plain_zero_sum_returns(Y, rew, offs, GAMMA, lam, mv)
            assert got.dtype == np.float64
            assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max(), (pattern, lam)
            plain = lambda_returns(Y, rew, offs, GAMMA, lam)
            if pattern == "equal":
                assert np.array_equal(got, plain)
                assert np.array_equal(lambda_returns(Y, rew, offs, GAMMA, lam, movers=None), plain)
                assert np.array_equal(lambda_returns(Y, rew, offs, GAMMA, lam, movers=1 - mv), plain)
            elif pattern == "alternating":
                assert not np.array_equal(got, plain)
    assert flips > 20
    assert lambda_returns(Y.astype(np.float32), rew, offs, GAMMA, 0.7, movers=mv).dtype == np.float32
    with pytest.raises(ValueError, match="movers"):
        lambda_returns(Y, rew, offs, GAMMA, 0.7, movers=mv[:-1])
    # the episode of length 2 (records 1, 2) with movers (0, 1)
    mv = np.zeros(len(rec), np.int64)
    mv[2] = 1
    for lam in (0.0, 0.3, 0.7, 1.0):
        g = lambda_returns(Y, rew, offs, GAMMA, lam, movers=mv)
        assert g[2] == rew[2]
        assert g[1] == rew[1] + GAMMA * ((1.0 - lam) * (1.0 - Y[2]) + lam * (1.0 - rew[2]))


def test_reference_defaults_are_unchanged_and_zero_sum_reaches_the_target():
    """batched_td0_reference: zero_sum=False is the result as it was (lam = 0 and
    0.7), zero_sum=True takes the movers from word 11 at every lam, also 0."""
    from bgx.train_ref import batched_td0_reference, lambda_returns
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    _, rec, offs = tc.synth([1, 2, 7, 30], seed=6)
    rew = lc.rewards(rec).astype(np.float64)
    for lam in (0.0, 0.7):
        a = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam)
        b = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=False)
        z = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=True)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(z["Y"], a["Y"])
        assert np.array_equal(z["target"], lambda_returns(a["Y"], rew, offs, GAMMA, lam, movers=zc.movers_of(rec)))
        assert not np.array_equal(z["target"], a["target"]) and not np.array_equal(z["grad"], a["grad"])
        # only word 11 is read: with one mover there, the plain target
        eq = rec.copy()
        eq[:, 11] &= ~np.uint32(1 << 9)
        zeq = batched_td0_reference(flat, eq, offs, GAMMA, lam=lam, zero_sum=True)
        assert np.array_equal(zeq["target"], a["target"]) and np.array_equal(zeq["grad"], a["grad"])


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_reference_gradient_equals_float64_autograd(wname):
    """batched_td0_reference(lam=0.7, zero_sum=True) against torch CPU float64
    autograd of the same loss with the targets fed in detached: E = 3, lengths
    1, 2 and 7."""
    from bgx.train_ref import batched_td0_reference
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = tc.synth([1, 2, 7], seed=5)
    mv = zc.movers_of(rec)
    assert (mv[2:] != mv[1:-1]).any()   # the drawn movers do change inside an episode
    ref = batched_td0_reference(flat, rec, offs, GAMMA, lam=0.7, zero_sum=True)
    grad, loss, y, tgt = zc.torch_zero_sum_grad(flat, rec, offs, GAMMA, 0.7, torch.float64)
    assert ref["grad"].shape == (25601,) and ref["grad"].dtype == np.float64
    assert np.abs(ref["grad"] - grad).max() <= 1e-12 * np.abs(grad).max()
    assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ref["Y"] - y).max() <= 1e-12
    assert np.abs(ref["target"] - tgt).max() <= 1e-12


def test_update_rejects_bad_arguments_before_the_device(L):
    """Each rule of include/bgx.h on its own; the other arguments are non-null
    (never dereferenced: the rejection comes first)."""
    need, old = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.bgx_tdlambda_batch_workspace(10, ctypes.byref(need)) == 0
    assert L.bgx_td0_batch_workspace(10, ctypes.byref(old)) == 0
    P = 0x10000   # a non-null, 16-byte aligned stand-in
    good = dict(rec=P, offs=P, n_eps=2, n_rec=10, params=P, m=P, v=P, step=P, lam=0.7, flags=zc.TDF_ZERO_SUM,
                metrics=P, grad=None, target=None, work=P, bytes=need.value)

    def call(**kw):
        a = dict(good, **kw)
        return L.bgx_td_update_batched(a["rec"], a["offs"], a["n_eps"], a["n_rec"], a["params"], a["m"], a["v"],
                                       a["step"], 1e-3, 0.99, a["lam"], a["flags"], 1.0, a["metrics"], a["grad"],
                                       a["target"], a["work"], a["bytes"], None)

    for flags in (0, zc.TDF_ZERO_SUM):
        for k in ("rec", "offs", "params", "m", "v", "step", "metrics", "work"):
            assert call(flags=flags, **{k: None}) == -1, k
            assert b"null" in L.bgx_last_error()
        for lam in (-0.1, 1.5, float("nan")):
            assert call(flags=flags, lam=lam) == -1, lam
            assert b"lambda" in L.bgx_last_error()
        assert call(flags=flags, bytes=need.value - 1) == -1
        assert b"work_bytes" in L.bgx_last_error()
        assert call(flags=flags, work=P + 8) == -1
        assert b"aligned" in L.bgx_last_error()
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
        assert call(flags=flags) == -1, flags
        assert b"flags" in L.bgx_last_error() and b"bgx_td_update_batched" in L.bgx_last_error()
    assert call(n_eps=0) == -1
    assert call(n_eps=-3) == -1
    assert call(n_eps=11) == -1          # n_records < n_eps
    assert call(bytes=old.value) == -1   # the TD(0) call's workspace is too small
    assert call(bytes=0) == -1


def test_abi_version_unchanged(L):
    assert L.bgx_abi_version() == 10


class _PM:
    def get_parameters(self, device=None):
        return tc.state_dict(tc.flat_params(tc.WEIGHTS["seed0"]))

    def set_parameters(self, sd):
        pass


def test_device_trainer_zero_sum_rules():
    """zero_sum defaults to False; a non-bool is rejected at construction;
    zero_sum=True on the sequential HIP backend is rejected when the update is
    called, with both ways out named."""
    import inspect
    from bgx.trainer import DeviceTrainer
    assert inspect.signature(DeviceTrainer.__init__).parameters["zero_sum"].default is False
    assert DeviceTrainer(_PM(), device="cpu").zero_sum is False
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="zero_sum"):
            DeviceTrainer(_PM(), device="cpu", zero_sum=bad)
    t = DeviceTrainer(_PM(), device="cpu", batched=True, backend="hip", lam=0.7, zero_sum=True)
    assert t.zero_sum is True and t.lam == 0.7
    hdr, rec, _ = tc.synth([2, 3], seed=1)
    t = DeviceTrainer(_PM(), device="cpu", zero_sum=True)
    assert t.backend == "hip" and not t.batched and t.lam == 0.0
    with pytest.raises(ValueError, match="batched=True.*backend='torch'"):
        t.update_records(hdr, rec)


def test_torch_backend_honours_zero_sum_on_the_cpu():
    """_episode_terms with the episode's movers: the target is fp32
    lambda_returns(movers=) on the detached y, bit for bit, at every lam (also
    0); without zero_sum the movers are not read."""
    from bgx.train_ref import encode_records, lambda_returns
    from bgx.trainer import DeviceTrainer
    _, rec, offs = tc.synth([1, 7, 30], seed=2)
    obs = torch.from_numpy(encode_records(rec))
    rew = torch.from_numpy(lc.rewards(rec))
    mv = DeviceTrainer._record_movers(torch.from_numpy(rec.view(np.int32)))
    assert np.array_equal(mv.numpy(), zc.movers_of(rec))
    for lam in (0.0, 0.7, 1.0):
        t = DeviceTrainer(_PM(), device="cpu", backend="torch", batched=True, lam=lam, zero_sum=True)
        p = DeviceTrainer(_PM(), device="cpu", backend="torch", batched=True, lam=lam)
        differs = False
        for e in range(3):
            a, b = int(offs[e]), int(offs[e + 1])
            y, tgt = t._episode_terms(obs, rew, a, b, mv)
            assert y.requires_grad and not tgt.requires_grad and tgt.dtype == torch.float32
            yh = y.detach().reshape(-1).numpy()
            want = lambda_returns(yh, rew[a:b].numpy(), [0, b - a], GAMMA, lam, movers=zc.movers_of(rec)[a:b])
            assert np.array_equal(tgt.reshape(-1).numpy(), want), (lam, e)
            _, tgt_p = p._episode_terms(obs, rew, a, b, mv)
            assert np.array_equal(tgt_p.reshape(-1).numpy(), p._episode_terms(obs, rew, a, b)[1].reshape(-1).numpy())
            differs |= not np.array_equal(tgt_p.reshape(-1).numpy(), want)
        assert differs
        with pytest.raises(ValueError, match="movers"):
            t._episode_terms(obs, rew, 0, 1)


def test_episode_path_and_records_path_see_the_same_movers():
    """update(episodes) reads feature 197 of each observation, update_records
    word 11 bit 9: the same movers for engine records (whose indicator is the
    mover), and so the same update on the torch backend."""
    from bgx.train_ref import encode_records
    from bgx.trainer import DeviceTrainer
    hdr, rec, offs = tc.synth([1, 7, 30], seed=2)
    assert np.array_equal((rec[:, 6] >> 16) & 1, (rec[:, 11] >> 9) & 1)
    obs = encode_records(rec)
    rew = lc.rewards(rec)
    episodes = [types.SimpleNamespace(win_type="regular",
                                      experiences=[types.SimpleNamespace(observation=obs[s], reward=rew[s])
                                                   for s in range(int(offs[e]), int(offs[e + 1]))])
                for e in range(3)]
    t = DeviceTrainer(_PM(), device="cpu", backend="torch", batched=True, lam=0.7, zero_sum=True,
                      batch_episode_size=3)
    o, r, lens, _, mv_e = t._from_episodes(episodes)
    mv_r = DeviceTrainer._record_movers(torch.from_numpy(rec.view(np.int32)))
    assert lens == [1, 7, 30] and np.array_equal(o.numpy(), obs) and np.array_equal(r.numpy(), rew)
    assert np.array_equal(mv_e.numpy(), mv_r.numpy()) and 0 < int(mv_e.sum()) < len(rec)
    m_e = t.update(episodes)
    t2 = DeviceTrainer(_PM(), device="cpu", backend="torch", batched=True, lam=0.7, zero_sum=True)
    m_r = t2._update(torch.from_numpy(obs), torch.from_numpy(rew), [1, 7, 30], ["regular"] * 3, mv_r)
    assert m_e == m_r
    t3 = DeviceTrainer(_PM(), device="cpu", backend="torch", batched=True, lam=0.7, batch_episode_size=3)
    assert t3.update(episodes)["loss"] != m_e["loss"]


# ---------------------------------------------------------------- the target stage, emulated
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    tmp = tmp_path_factory.mktemp("zs_emu")
    src = _emu_sources(tmp)
    exe = tmp / "zs_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address", "-fno-omit-frame-pointer",
                    "-I" + str(src), "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "include"),
                    "-x", "c++", os.path.join(HERE, "cpuwave", "zs_emu.cpp"), "-o", str(exe), "-pthread"],
                   check=True, capture_output=True, text=True)
    return tmp, exe


N_PAST = 5   # records after the last episode: in no episode, their target stays 0
_HARVEST = {}


def _harvest(name):
    """(records with N_PAST more at the end, offs) of the two emulated harvests
    (test_train_lambda_ref.py's)."""
    if name not in _HARVEST:
        lens = lc.EDGE_LENS if name == "edges" else tc.ragged_lens(20000, 31)[:300]
        _, rec, offs = tc.synth(lens, seed=40 + len(lens))
        extra = tc.base_records()[:N_PAST].copy()
        extra[:, 9] = np.float32([1.5] * N_PAST).view(np.uint32)
        _HARVEST[name] = (np.concatenate([rec, extra]), offs)
    return _HARVEST[name]


def _run(exe, tmp, tag, gamma, lam, zs, n):
    out = tmp / f"out_{tag}_{lam}_{zs}.bin"
    r = subprocess.run([str(exe), str(tmp / f"rec_{tag}.bin"), str(tmp / f"offs_{tag}.bin"), str(tmp / f"y_{tag}.bin"),
                        repr(gamma), repr(lam), str(zs), str(out)], capture_output=True, text=True, timeout=600,
                       env=ENV)
    assert r.returncode == 0 and not r.stderr, (tag, lam, zs, r.returncode, r.stderr[-3000:])
    return np.fromfile(out, np.float32).reshape(2, n)


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
@pytest.mark.parametrize("name", ["edges", "ragged300"])
def test_target_stage_emulated_against_float64(emu, name, wname):
    """tl_target_kernel<true> through its launcher on the emulated grid, every
    mover pattern of train_zero_sum_cases.PATTERNS (each written into word 11
    bit 9 and word 6 bit 16), lam in {0, 0.7, 1}. Y is the fp32 rounding of the
    float64 forward pass of the rewritten records; G64 is the float64
    recurrence on that Y. err = max|tgt - G64| / max|G64| is at most max(2 fp32
    ulps of max|G64|, 4 x the err of the serial fp32 lambda_returns(movers=) on
    the same Y). With one mover everywhere the output equals the plain
    instance's bit for bit. target_out equals tgt; the records past the last
    episode keep 0 (both buffers start as 7); AddressSanitizer reports nothing."""
    from bgx.train_ref import batched_td0_reference, lambda_returns
    tmp, exe = emu
    rec0, offs = _harvest(name)
    n, n_in = len(rec0), int(offs[-1])
    assert n == n_in + N_PAST and (name != "ragged300" or len(offs) - 1 == 300)
    worst = 0.0
    for pattern in zc.PATTERNS:
        rec = zc.with_pattern(rec0, offs, pattern)
        mv = zc.movers_of(rec)
        assert np.array_equal((rec[:, 6] >> 16) & 1, mv) and np.array_equal(mv, zc.pattern_movers(rec0, offs, pattern))
        n_flips = sum(int((mv[int(offs[e]) + 1:int(offs[e + 1])] != mv[int(offs[e]):int(offs[e + 1]) - 1]).sum())
                      for e in range(len(offs) - 1))
        if pattern == "equal":
            assert n_flips == 0
        elif pattern.startswith("flip"):
            assert n_flips == int((np.diff(offs) > int(pattern[4:])).sum()) > 0
        else:
            assert n_flips > (n_in - len(offs)) // 4
        y32 = batched_td0_reference(tc.flat_params(tc.WEIGHTS[wname]), rec[:n_in], offs, GAMMA)["Y"].astype(np.float32)
        y32 = np.concatenate([y32, np.float32([0.25] * N_PAST)])
        rew = lc.rewards(rec)
        tag = f"{name}_{wname}_{pattern}"
        rec.tofile(tmp / f"rec_{tag}.bin")
        offs.astype(np.int32).tofile(tmp / f"offs_{tag}.bin")
        y32.tofile(tmp / f"y_{tag}.bin")
        for lam in (0.0, 0.7, 1.0):
            got = _run(exe, tmp, tag, GAMMA, lam, 1, n)
            g64 = lambda_returns(y32.astype(np.float64), rew.astype(np.float64), offs, GAMMA, lam, movers=mv)
            g32 = lambda_returns(y32, rew, offs, GAMMA, lam, movers=mv)
            err, err32 = lc.rel_err(got[0][:n_in], g64[:n_in]), lc.rel_err(g32[:n_in], g64[:n_in])
            bound = max(lc.floor_rel(g64[:n_in]), lc.F32_FACTOR * err32)
            worst = max(worst, err / bound)
            print(f"{tag} lam {lam}: records {n_in} episodes {len(offs) - 1} flips {n_flips} target err emulated "
                  f"{err:.3e} serial fp32 {err32:.3e} bound {bound:.3e}")
            assert np.array_equal(got[0], got[1])
            assert not got[0][n_in:].any()
            assert np.isfinite(got[0]).all()
            assert err <= bound
            if pattern == "equal":
                plain = _run(exe, tmp, tag, GAMMA, lam, 0, n)
                assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), lam
                assert np.array_equal(plain[0], plain[1]) and not plain[0][n_in:].any()
            elif pattern == "alternating" and lam == 0.7:
                plain = _run(exe, tmp, tag, GAMMA, lam, 0, n)   # the flag does reach the stage
                assert not np.array_equal(got[0], plain[0])
    print(f"{name}_{wname}: worst err / bound {worst:.3f}")
