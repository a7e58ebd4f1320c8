"""Host-emulated checks of the rollout mode's device code (tests/cpuwave/rollout_emu.cpp).

bgx_rollout.hip and bgx_engine.hip are compiled for the host against
tests/cpuwave/hip/hip_runtime.h as a stand-alone program under
AddressSanitizer, as test_cpuwave_match builds match_emu.cpp: the tally kernel
through its launcher (the LDS histogram while n_pos * 8 bins fit 2,048 words,
direct global atomics beyond) with exact-size buffers, and the reset kernel
with a start table (start_game: fixed dice, stratified and rolled first rolls).
"""
import os
import subprocess

import numpy as np
import pytest

from bgx.rollout import tally_counts
from test_cpuwave import CLANG, HERE, REPO, _emu_sources, _pack
from test_rollout_tally import POS_A, POS_C, POS_D, random_headers

ENV = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    tmp = tmp_path_factory.mktemp("rollout_emu")
    src = _emu_sources(tmp)
    exe = tmp / "rollout_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address", "-fno-omit-frame-pointer",
                    "-I" + str(src), "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "include"),
                    "-x", "c++", os.path.join(HERE, "cpuwave", "rollout_emu.cpp"), "-o", str(exe), "-pthread"],
                   check=True, capture_output=True, text=True)
    return tmp, exe


@pytest.mark.parametrize("n_pos", [1, 3, 600])
def test_tally_kernel_emulated_equals_tally_counts(emu, n_pos):
    """n_headers in {0 (the launcher alone), 1, 63, 64, 65, 1000} (one thread,
    a wave less / exactly / plus one, four workgroups with a partial last one)
    for n_pos = 1 and 3 (LDS histogram) and 600 (4,800 bins > 2,048: direct
    global atomics). Two accumulating calls over the same headers, the first
    with max_episode 2 and the second with 4 of the 5 episode numbers present:
    the counts equal tally_counts(.., 2) + tally_counts(.., 4) exactly."""
    tmp, exe = emu
    rng = np.random.default_rng(100 + n_pos)
    sp = rng.integers(0, 2, n_pos).astype(np.uint8)
    sp.tofile(tmp / f"sp{n_pos}.bin")
    for n in (0, 1, 63, 64, 65, 1000):
        h = random_headers(rng, n, lanes=5000, episodes=5)
        h.tofile(tmp / f"h{n_pos}_{n}.bin")
        out = tmp / f"c{n_pos}_{n}.bin"
        r = subprocess.run([str(exe), "tally", str(tmp / f"h{n_pos}_{n}.bin"), str(tmp / f"sp{n_pos}.bin"), str(n_pos),
                            "2", "4", str(out)], capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode == 0, (n, r.returncode, r.stderr[-3000:])
        got = np.fromfile(out, np.uint64).reshape(n_pos, 8)
        want = tally_counts(h, sp, n_pos, 2) + tally_counts(h, sp, n_pos, 4)
        np.testing.assert_array_equal(got, want, err_msg=f"n_headers={n}")
        if n >= 63:
            assert got[:, :7].sum() > 0 and got[:, :7].sum() < 2 * n   # some counted, some filtered


def _table(boards, player, dice):
    tab = _pack(boards, player)
    tab[:, 7] = player.astype(np.uint32) | dice[:, 0].astype(np.uint32) << 8 | dice[:, 1].astype(np.uint32) << 16
    return tab


def _reset(emu, tab, L, lane_base, stride, tag):
    tmp, exe = emu
    tab.tofile(tmp / f"tab_{tag}.bin")
    out = tmp / f"reset_{tag}.bin"
    r = subprocess.run([str(exe), "reset", str(tmp / f"tab_{tag}.bin"), str(L), str(lane_base), str(stride), "3",
                        str(out)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = out.read_bytes()
    rows = np.frombuffer(raw[:L * 32], np.uint32).reshape(L, 8)
    pd = np.frombuffer(raw[L * 32:L * 36], np.uint8).reshape(L, 4)
    ctr = np.frombuffer(raw[L * 36:], np.uint64)
    assert ctr.shape == (L,)
    return rows, pd[:, 0], pd[:, 1:3], ctr


def test_reset_kernel_emulated_starts_from_the_table(emu):
    """L = 70, lane_base = 5, three positions (players 0, 1, 0), fixed dice 6-5
    on position 1 and strat_stride = 4 on the others: lane i holds the row and
    the player of position g % 3 (g = 5 + i; word 7 back to 0), position 1's
    lanes carry 6-5, the others the stratified roll of trial t = 0 * 4 + g // 3
    of episode 0, and no lane drew from its stream. Without a stride the
    rolled lanes draw exactly one roll (dice in 1..6), the fixed ones none."""
    boards = np.stack([POS_C, POS_D, POS_A])
    player = np.array([0, 1, 0], np.uint8)
    dice = np.array([[0, 0], [6, 5], [0, 0]], np.uint8)
    tab = _table(boards, player, dice)
    L, base = 70, 5
    g = base + np.arange(L)
    pos = g % 3
    want_rows = tab[pos].copy()
    want_rows[:, 7] = 0
    rows, pl, dd, ctr = _reset(emu, tab, L, base, 4, "strat")
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(pl, player[pos])
    r = (g // 3) % 36
    want_d = np.where((pos == 1)[:, None], np.array([6, 5]), np.stack([r // 6 + 1, r % 6 + 1], 1))
    np.testing.assert_array_equal(dd, want_d)
    assert not ctr.any()
    assert len({tuple(x) for x in dd[pos != 1]}) >= 20   # the stratified rolls do run over the 36
    rows, pl, dd, ctr = _reset(emu, tab, L, base, 0, "rolled")
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(pl, player[pos])
    np.testing.assert_array_equal(dd[pos == 1], np.tile([6, 5], (int((pos == 1).sum()), 1)))
    assert dd.min() >= 1 and dd.max() <= 6
    np.testing.assert_array_equal(ctr, np.where(pos == 1, 0, 1))
    assert len({tuple(x) for x in dd[pos != 1]}) >= 10   # per-lane streams, not one roll for all
