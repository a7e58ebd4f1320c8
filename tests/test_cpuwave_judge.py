"""judge() (bgx_engine.h) on the host against the reference's labels.

tests/cpuwave/judge_emu.cpp compiles the header as the kernels do (g++,
AddressSanitizer, its own main) and runs judge() on every row of
predicates.npz and outcomes.npz (the enumerated boundary boards of
tests/outcome_cases.py), each under all 16 values of the incoming shaping
bits 0-3, with the "moved" bits 4-5 both clear and both set. Everything is
compared exactly: flags, win types and the rewards' fp32 bits."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import golden
from test_cpuwave import _build, _pack

F32 = np.float32


def expected(p, flags_in):
    """What judge() must return on the fixture's rows for the incoming flag
    words: (reward bits, done, win_type, close, prime, flags out), from the
    reference's five booleans alone (backgammon_env.py:167-213)."""
    pl = p["player"].astype(np.uint32)
    over = p["game_over"]
    wt = np.where(p["backgammon"], 3, np.where(p["gammon"], 2, 1))
    win = np.array([0.0, 1.0, 2.0, 2.5], F32)[wt]
    close = ~over & p["closed_out"] & ((flags_in >> pl) & 1 == 0)
    prime = ~over & p["prime"] & ((flags_in >> (2 + pl)) & 1 == 0)
    # the kernel's order: 0.0f, + 0.30f, + 0.20f
    r = np.zeros(len(pl), F32)
    r = np.where(close, r + F32(0.30), r).astype(F32)
    r = np.where(prime, r + F32(0.20), r).astype(F32)
    r = np.where(over, win, r).astype(F32)
    out = flags_in | (close.astype(np.uint32) << pl) | (prime.astype(np.uint32) << (2 + pl))
    return np.stack([r.view(np.uint32), over.astype(np.uint32), np.where(over, wt, 0).astype(np.uint32),
                     close.astype(np.uint32), prime.astype(np.uint32), out.astype(np.uint32)], axis=1)


@pytest.fixture(scope="module")
def judge_emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    return _build(tmp_path_factory.mktemp("judge_emu"), "judge_emu.cpp", "judge_emu")


@pytest.mark.parametrize("fixture", ["predicates.npz", "outcomes.npz"])
def test_judge_emulated_equals_reference_labels(tmp_path, judge_emu, fixture):
    p = golden(fixture)
    n = len(p["boards"])
    rows = _pack(p["boards"], p["player"])   # word 6's indicator: as the engine's candidate rows carry the mover
    ins, want = [], []
    for hi in (0, 48):
        for lo in range(16):
            fl = np.full(n, hi | lo, np.uint32)
            ins.append(np.concatenate([rows, p["player"].astype(np.uint32)[:, None], fl[:, None]], axis=1))
            want.append(expected(p, fl))
    ins, want = np.concatenate(ins).astype(np.uint32), np.concatenate(want)
    ins.tofile(tmp_path / "in.bin")
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([str(judge_emu), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(-1, 6)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), ins[bad[0]], got[bad[0]], want[bad[0]], p["boards"][bad[0] % n])
    # what the comparison above pinned, stated on the outputs themselves
    fl_in = ins[:, 9]
    pl = ins[:, 8]
    term = got[:, 1] == 1
    assert set(np.unique(got[term, 0]).tolist()) <= {int(np.array(v, F32).view(np.uint32)) for v in (1.0, 2.0, 2.5)}
    assert (got[term, 5] == fl_in[term]).all() and not got[term, 3:5].any()
    other = (2 >> pl) | (8 >> pl) | 48   # the other player's bits and the moved bits
    assert ((got[:, 5] ^ fl_in) & other == 0).all()
    assert (got[:, 5] & fl_in == fl_in).all()
    if fixture == "outcomes.npz":
        assert term.any() and got[:, 3].any() and got[:, 4].any()
        assert {int(v) for v in np.unique(got[term, 2])} == {1, 2, 3}
