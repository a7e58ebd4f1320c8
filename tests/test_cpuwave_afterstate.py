"""The afterstate rows of the batched update on the host
(tests/cpuwave/after_emu.cpp, built with AddressSanitizer and UBSan, run as a
child process): the index launch's afterstate form, the staging of a tile's
source indices and the afterstate tile loader (csrc/bgx_train_tile.h), in the
kernels' order, on emulated workgroups with exact-size rec, hdr,
offs and workspace buffers. Every tile's 7 row words equal
bgx.records.packed_afterstates, the reward sits in slot 7, the slots past the
last record are zero, and the source index is s + 1, ~e on an episode's last
record and 0 on a record in no episode. A read at or past rec + 12 n_rec or
hdr + 16 n_eps is a sanitizer report (the last record of the last episode takes
its row from the header; a non-last record in a tile's last slot takes it from
the next tile). Only index + loader are emulated (see the program's header)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import train_afterstate_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = [(name, 0) for name in ac.EMU_LENS] + [ac.TRAILING]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("after_emu") / "after_emu"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-attributes", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "cpuwave", "after_emu.cpp"),
                    "-o", str(exe), "-pthread"], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0] + (f"+{c[1]}" if c[1] else ""))
def test_index_and_loader_rows_equal_packed_afterstates(emu, case, tmp_path):
    from bgx.records import packed_afterstates
    name, trailing = case
    hdr, rec, offs = ac.synth_after(ac.EMU_LENS[name], seed=40 + len(name), trailing=trailing)
    m, n_rec, n_eps = int(offs[-1]), len(rec), len(hdr)
    assert n_rec == m + trailing
    rec.astype(np.uint32).tofile(tmp_path / "rec.bin")
    hdr.astype(np.uint32).tofile(tmp_path / "hdr.bin")
    offs.astype(np.int32).tofile(tmp_path / "offs.bin")
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([emu, str(tmp_path / "rec.bin"), str(tmp_path / "hdr.bin"), str(tmp_path / "offs.bin"),
                        str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]   # a read out of bounds ends the program
    n_tiles = (n_rec + ac.TILE - 1) // ac.TILE
    out = np.fromfile(tmp_path / "out.bin", np.uint32)
    assert out.size == n_rec + n_tiles * ac.TILE * 8
    srcidx = out[:n_rec].view(np.int32)
    rows = out[n_rec:].reshape(n_tiles * ac.TILE, 8)
    # the source index: the next record, the header on an episode's last record, 0 in no episode
    want_src = np.arange(1, n_rec + 1, dtype=np.int64)
    want_src[offs[1:] - 1] = ~np.arange(n_eps, dtype=np.int64)
    want_src[m:] = 0
    assert np.array_equal(srcidx, want_src)
    # the covered rows, the rewards, the zero slots past the last record
    assert np.array_equal(rows[:m, :7], packed_afterstates(hdr, rec[:m])[:, :7])
    assert np.array_equal(rows[:m, :7], ac.rows_by_hand(hdr, rec, offs))
    assert np.array_equal(rows[:n_rec, 7], rec[:, 9])
    assert not rows[n_rec:].any()
    # the indicator is the mover's everywhere, also where the source's own bit differs
    assert np.array_equal((rows[:n_rec, 6] >> 16) & 1, ac.movers_of(rec))
    if m >= ac.TILE:   # most sources are the next record: its own bit is random
        assert (((rec[1:m, 6] >> 16) & 1) != ac.movers_of(rec[:m - 1])).any()
