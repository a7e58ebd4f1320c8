"""Host-emulated check of the match mode's routed MLP launch (tests/cpuwave/match_emu.cpp).

bgx_match.hip is compiled for the host against tests/cpuwave/hip/hip_runtime.h
(each lane a thread, v_mfma_f32_32x32x16_f16 with the operand layout the
fragments are built for) as a stand-alone program under AddressSanitizer, as
test_cpuwave.test_mlp_kernels_emulated_equal_oracle_value builds mlp_emu.cpp:
the id routing (route_ids_kernel) and mlp_kernel_routed, on 2 emulated CUs so
that both starting networks and the reload of the other network's fragments
run.
"""
import os
import subprocess

import numpy as np
import pytest

from test_cpuwave import CLANG, HERE, REPO, _emu_sources, _pack

N = 150


def _weights(name):
    w = np.load(os.path.join(HERE, "golden", name))
    return {k: w[k].astype(np.float32) for k in ("W1", "b1", "w2", "b2")}


def _patterns(n):
    rng = np.random.default_rng(5)
    return {"all0": np.zeros(n, np.uint8), "all1": np.ones(n, np.uint8),
            "alternating": (np.arange(n) & 1).astype(np.uint8),
            "random": rng.integers(0, 2, n).astype(np.uint8)}


def _setup(tmp_path, seed, n):
    """n random placements, both networks' oracle values [2, n], the harness built
    under AddressSanitizer, and run(rows_file, ids, nt, tag) -> V."""
    orc = pytest.importorskip("oracle")
    from test_gpu_parity import _random_positions
    pos = _random_positions(seed, n)
    boards = np.stack([p[0] for p in pos])
    pl = np.array([p[1] for p in pos])
    W = [_weights("weights_ckpt2100000.npz"), _weights("weights_seed0.npz")]
    x = orc.encode_many(boards, pl)
    ref = np.stack([orc.value(W[0], x), orc.value(W[1], x)])
    for k in (0, 1):
        np.concatenate([W[k][q].ravel() for q in ("W1", "b1", "w2", "b2")]).astype(np.float32).tofile(
            tmp_path / f"w{k}.bin")
    rows = _pack(boards, pl)
    rows.tofile(tmp_path / "rows.bin")
    rows[:1].tofile(tmp_path / "row1.bin")
    src = _emu_sources(tmp_path)
    exe = tmp_path / "match_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address", "-fno-omit-frame-pointer",
                    "-I" + str(src), "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "include"),
                    "-x", "c++", os.path.join(HERE, "cpuwave", "match_emu.cpp"), "-o", str(exe), "-pthread"],
                   check=True, capture_output=True, text=True)
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0", "EMU_N_CU": "2"}

    def run(rows_file, ids, nt, tag):
        ids.tofile(tmp_path / f"ids_{tag}.bin")
        out = tmp_path / f"v_{tag}_{nt}.bin"
        r = subprocess.run([str(exe), str(rows_file), str(tmp_path / "w0.bin"), str(tmp_path / "w1.bin"),
                            str(tmp_path / f"ids_{tag}.bin"), nt, str(out)], capture_output=True, text=True,
                           timeout=600, env=env)
        assert r.returncode == 0, (tag, nt, r.returncode, r.stderr[-3000:])
        return np.fromfile(out, np.float32)

    return ref, run


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang")
def test_routed_mlp_emulated_equals_oracle_value_per_network(tmp_path):
    """150 random placements (bar, borne-off checkers), the trained checkpoint
    as network 0 and the untrained weights as network 1, five id patterns (all
    0, all 1, alternating, random, a single row), both tile forms (NT = 1: root
    launch / stateless call; NT = 2: reply launch): every V within 1e-6 of the
    oracle's fp64 value (policy_network.py:53-70) under the row's own network,
    every row stored. In the random pattern at least half the rows lie more
    than 1e-4 from the other network's value, which an unrouted kernel would
    fail; the oracle alone meets that share here (checked first: 150 of the
    150 rows differ by more than 1e-4 between the two networks)."""
    ref, run = _setup(tmp_path, 3, N)
    # the discrimination condition on the oracle alone, before relying on it
    assert np.mean(np.abs(ref[0] - ref[1]) > 1e-4) >= 0.5
    for nt in ("1", "2"):
        for tag, ids in _patterns(N).items():
            v = run(tmp_path / "rows.bin", ids, nt, tag)
            assert v.shape == (N,)
            own = ref[ids, np.arange(N)]
            err = np.abs(v - own)
            print(f"nt={nt} {tag}: max |V - oracle| = {err.max():.3g}")
            assert err.max() < 1e-6, (nt, tag, err.max(), int(err.argmax()))
            if tag == "random":
                other = ref[1 - ids, np.arange(N)]
                assert np.mean(np.abs(v - other) > 1e-4) >= 0.5
        for net in (0, 1):   # a single row: one list empty, the other one partial tile
            v = run(tmp_path / "row1.bin", np.array([net], np.uint8), nt, f"single{net}")
            assert v.shape == (1,) and abs(v[0] - ref[net, 0]) < 1e-6, (nt, net, v)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang")
def test_routed_mlp_emulated_several_chunks_per_list(tmp_path):
    """1,100 rows, random ids: each list spans several of the workgroup claims
    (chunks of 16 single tiles, or of 8 tile pairs), so the claim-ahead slots
    rotate and a chunk's tail runs past the list's end; the second emulated
    workgroup finds both lists taken. Every V within 1e-6 of the oracle under
    the row's own network."""
    n = 1100
    ref, run = _setup(tmp_path, 4, n)
    ids = np.random.default_rng(6).integers(0, 2, n).astype(np.uint8)
    own = ref[ids, np.arange(n)]
    for nt in ("1", "2"):
        v = run(tmp_path / "rows.bin", ids, nt, "many")
        assert v.shape == (n,)
        assert np.abs(v - own).max() < 1e-6, (nt, float(np.abs(v - own).max()))
