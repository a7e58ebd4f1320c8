"""The batched trainer's live-feature rule on the host (tests/cpuwave/feature_emu.cpp,
built with AddressSanitizer and UBSan, run as a child process): the field
locator and the value table that the backward kernel reads (tb_field,
tb_lut_entry; csrc/bgx_train_tile.h) and their composition per feature agree on
every feature slot (checked in the program) and their 198 features equal
bgx.train_ref.encode_records bit for bit.

The 16 x 2 constructed rows put field j (48 points, then bar1, bar2, off1, off2)
at (v + j) % 16 for v = 0..15 under both indicator values: every field takes
every nibble value, and neighbouring fields always differ, so a locator that
reads the wrong field shows. One train_batch_cases.synth draw adds real boards."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import train_batch_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("feature_emu") / "feature_emu"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-attributes", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "cpuwave", "feature_emu.cpp"),
                    "-o", str(exe), "-pthread"], check=True, capture_output=True, text=True)
    return str(exe)


def constructed_rows():
    """uint32 [32, 7]: row 2 v + b has field j at (v + j) % 16 and indicator b."""
    rows = np.zeros((32, 7), np.uint32)
    for v in range(16):
        for b in range(2):
            w = rows[2 * v + b]
            for j in range(48):
                w[j // 8] |= np.uint32((v + j) % 16) << np.uint32(4 * (j % 8))
            bar1, bar2, off1, off2 = ((v + j) % 16 for j in range(48, 52))
            w[6] = bar1 | bar2 << 4 | off1 << 8 | off2 << 12 | b << 16
    return rows


def test_shared_feature_functions_equal_encode_records(emu, tmp_path):
    from bgx.train_ref import encode_records
    _, rec, _ = tc.synth([40, 1, 23], seed=77)
    rows = np.concatenate([constructed_rows(), rec[:, :7]]).astype(np.uint32)
    for j in range(52):   # every nibble value in every point, bar and off field
        word, nib = (j // 8, j % 8) if j < 48 else (6, j - 48)
        assert set(((rows[:32, word] >> np.uint32(4 * nib)) & 15).tolist()) == set(range(16)), j
    assert set(((rows[:32, 6] >> 16) & 1).tolist()) == {0, 1}
    rows.tofile(tmp_path / "rows.bin")
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([emu, str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]   # 3: the composition and locator + table disagree
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(len(rows), 198)
    full = np.zeros((len(rows), 12), np.uint32)
    full[:, :7] = rows
    want = encode_records(full).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(got[:32, 193])) == 16 and len(np.unique(got[:32, 195])) == 16   # n / 15, every n
