"""Two rule-mode non-doubles jobs in one wave (job_records_pair,
csrc/bgx_movegen.h) on the emulated wave (tests/cpuwave/pair_check.cpp, built
with AddressSanitizer): for each pair (A, B) the pair's emit writes, per job,
byte-identical boards in the same order and with the same count as
job_records + emit_records of the job alone; nothing is written outside each
job's `cap` slots; the 64-word parent map is zero on return; and both equal
the oracle's movegen list (checked here from the program's dump).

Inputs: the rule-mode non-doubles positions of tests/golden/env_traj.npz
paired (i, i + 1), plus the edge pairs the program picks among them (player 0
with player 1, equal dice, the two largest jobs together, nH == 1, 16 first
moves in a pass when one exists, a reduced list that forces "not pairable")
and one built position without two-move plays beside a normal one.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import golden

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
INC = ["-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
       "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(HERE, "cpuwave", "pair_check.cpp")


def _pack(boards, flag):
    """uint8 [n, 52] boards -> packed rows uint32 [n, 8] (bgx_device.h u8_to_packed)"""
    rows = np.zeros((len(boards), 8), np.uint32)
    for k in range(6):
        for q in range(8):
            rows[:, k] |= boards[:, 8 * k + q].astype(np.uint32) << np.uint32(4 * q)
    rows[:, 6] = (boards[:, 48].astype(np.uint32) | boards[:, 49].astype(np.uint32) << 4 |
                  boards[:, 50].astype(np.uint32) << 8 | boards[:, 51].astype(np.uint32) << 12 |
                  flag.astype(np.uint32) << 16)
    return rows


def _unpack(w):
    n = w.shape[0]
    out = np.zeros((n, 52), np.uint8)
    for k in range(6):
        for q in range(8):
            out[:, 8 * k + q] = (w[:, k] >> (4 * q)) & 15
    for i in range(4):
        out[:, 48 + i] = (w[:, 6] >> (4 * i)) & 15
    return out


def _no_two_move_position():
    """Player 0 to move 6-5 in rule mode (nothing on the bar, three checkers
    outside home) with one legal play, 0 -> 5: 0 + 6 and 5 + 6 are blocked and
    the twelve checkers on 23 cannot move while others are outside home."""
    b = np.zeros(52, np.uint8)
    b[0], b[23] = 3, 12
    b[24 + 6], b[24 + 11], b[24 + 12] = 2, 2, 11
    return b, 0, (6, 5)


def _positions():
    t = golden("env_traj.npz")
    nd = t["roll"][:, 0] != t["roll"][:, 1]
    boards = [b for b in t["board"][nd]]
    player = [int(p) for p in t["player"][nd]]
    dice = [(int(a), int(b)) for a, b in t["roll"][nd]]
    b, p, d = _no_two_move_position()
    boards.append(b)
    player.append(p)
    dice.append(d)
    return np.stack(boards), np.array(player, np.int64), np.array(dice, np.int64)


def _write(path, boards, player, dice):
    rows = np.zeros((len(boards), 11), np.uint32)
    rows[:, :8] = _pack(boards, player)
    rows[:, 8] = player
    rows[:, 9:11] = dice
    rows.tofile(path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_pair_equals_each_job_alone_and_the_oracle(tmp_path):
    orc = pytest.importorskip("oracle")
    boards, player, dice = _positions()
    pfile, dump = tmp_path / "pos.bin", tmp_path / "dump.bin"
    _write(pfile, boards, player, dice)
    exe = tmp_path / "pair_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address", "-fno-omit-frame-pointer", *INC,
                    "-x", "c++", SRC, "-o", str(exe), "-pthread"], check=True, capture_output=True, text=True)
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([str(exe), str(pfile), str(dump)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(r.stdout[-600:])
    assert res["mismatches"] == 0
    assert res["expanded_as_pairs"] > 0 and res["not_pairable"] >= 3   # the built position twice, the reduced list
    assert res["positions"] > 1500
    assert "no two-move play found" in r.stdout and "players found" in r.stdout
    # each job alone (which every pair equalled) is the oracle's list
    d = np.frombuffer(dump.read_bytes(), np.int32)
    at, seen = 0, 0
    while at < len(d):
        i, c, n = (int(x) for x in d[at:at + 3])
        at += 3
        got = _unpack(d[at:at + 8 * n].view(np.uint32).reshape(-1, 8))
        at += 8 * n
        cnt, want, _ = orc.movegen(boards[i], int(player[i]), int(dice[i][0]), int(dice[i][1]), cap=4096)
        assert c == cnt, (i, c, cnt)
        np.testing.assert_array_equal(got, want[:n], err_msg=f"position {i}")
        seen += 1
    assert seen == res["positions"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_pair_cross_lane_ops_are_uniform(tmp_path):
    """Every cross-lane operation of job_records_pair (ballots, shuffles,
    readlane, DPP scans) is reached by all 64 lanes from the same call chain
    (EMU_SITES build, -O0 -fno-inline), on the edge pairs and the last
    consecutive ones."""
    boards, player, dice = _positions()
    pfile = tmp_path / "pos.bin"
    _write(pfile, boards, player, dice)
    exe = tmp_path / "pair_site"
    subprocess.run(["g++", "-std=c++20", "-O0", "-fno-inline", "-g", "-w", "-DEMU_SITES", *INC, "-x", "c++", SRC,
                    "-o", str(exe), "-pthread"], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(pfile), str(tmp_path / "dump.bin"), "60"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '"mismatches": 0' in r.stdout
