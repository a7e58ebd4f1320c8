"""The learner's device-side hand-offs (csrc/bgx_pack.h) on the host
(tests/cpuwave/pack_emu.cpp under the wave emulation, built with
AddressSanitizer and UBSan).

Weights: the check and pack kernels against bgx_frag.h's unrepresentable /
build_fragments, byte for byte (fragments, e, the fp32 copies, the bits of b2)
for every weight set of tests/value_cases.py, all zeros, sets scaled so that e
hits both clamps, a set whose lo halves are fp16 subnormals, and values in
columns 193 / 195; rejections (NaN and Inf in each of the four tensors, the
first index when there are several, a W1 and a b1 entry at the 2^26 limit, the
193 / 195 columns at their own limit) report the host's rule and index and
leave every output byte as it was; an entry just under the limit is accepted.

Offsets: the offsets kernel against numpy.cumsum for n in 0 .. 5,000 across
the wave, workgroup-chunk and multi-chunk edges, lengths 0 .. 300.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import value_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
N_W1 = 128 * 198
B1, W2, B2 = N_W1, N_W1 + 128, N_W1 + 256
LIMIT = 2.0 ** 26
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OFFS_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(CLANG):   # _Float16 conversions: the ROCm clang, as for the MLP emulation
        pytest.skip("no ROCm clang")
    out = tmp_path_factory.mktemp("pack_emu") / "pack_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), "-x", "c++", os.path.join(HERE, "cpuwave", "pack_emu.cpp"),
                    "-o", str(out), "-pthread"], check=True, capture_output=True, text=True)
    return str(out)


def _run(exe, args):
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _flat(w):
    return np.concatenate([np.asarray(w[k], np.float32).ravel() for k in ("W1", "b1", "w2", "b2")])


def _f32_below(x):
    return np.nextafter(np.float32(x), np.float32(0.0))


def accepted_sets():
    """{name: (flat float32 [25601], expected e)}"""
    sets = {name: (_flat(w), vc.INTENDED_E[name]) for name, w in vc.weight_sets().items()}
    ckpt = vc.weight_sets()["ckpt"]
    sets["all_zero"] = (np.zeros(B2 + 1, np.float32), 0)
    sets["clamp_hi"] = (_flat(vc.scaled(ckpt, -30)), 13)          # unclamped e far above 13
    # (the low clamp: mx < 2^26 gives e >= -11 by itself; value_cases' clamp_lo and the under_* sets
    # below sit at e = -11, the largest weights the scheme takes)
    # lo halves that are fp16 subnormals: every |w| < 2^-8, so e clamps to 13 and x = -log2(e) w 2^13;
    # w is the fp32 nearest to an integer x = H in 1 .. 16, moved k fp32 ulps: hi = H exactly and the
    # rest, about k H 2^-24 < 2^-14, is below the smallest normal fp16
    rng = np.random.default_rng(7)
    H = rng.integers(1, 17, size=N_W1).astype(np.float64) * np.where(rng.integers(0, 2, N_W1) == 1, 1.0, -1.0)
    w = (H / (vc.LOG2E * 8192.0)).astype(np.float32)
    w = (w.view(np.int32) + rng.integers(1, 41, size=N_W1).astype(np.int32)).view(np.float32)
    s = np.zeros(B2 + 1, np.float32)
    s[:N_W1] = w
    s[W2:B2] = vc.weight_sets()["seed0"]["w2"]
    sets["lo_subnormal"] = (s, 13)
    # the borne-off columns carry the maximum: 15 x what any other column could hold
    c = {k: v.copy() for k, v in ckpt.items()}
    c["W1"][5, 193] = 7000.0
    c["W1"][77, 195] = -9000.0
    sets["cols_193_195"] = (_flat(c), None)
    # a hair under the limit, in W1, in b1 and (15 x) in column 193
    for name, idx, scale in (("under_W1", 17 * 198 + 3, 1.0), ("under_b1", B1 + 9, 1.0), ("under_193", 4 * 198 + 193, 15.0)):
        u = _flat(ckpt)
        v = np.float32(LIMIT / vc.LOG2E * scale)
        while vc.LOG2E * float(v) / scale >= LIMIT:
            v = _f32_below(v)
        u[idx] = -v
        sets[name] = (u, -11)
    out = {}
    for name, (flat, e) in sets.items():
        if e is None:
            e = vc.expected_e({"W1": flat[:N_W1].reshape(128, 198), "b1": flat[B1:W2]})
        out[name] = (flat, e)
    # the clamp cases hit the clamps
    assert out["clamp_hi"][1] == 13 and out["clamp_lo"][1] == -11
    return out


def rejected_sets():
    """{name: (flat, rule, flat index)}: rule 1 = not finite, 2 = the 2^26 limit"""
    base = _flat(vc.weight_sets()["ckpt"])
    out = {}
    for tname, lo, n in (("W1", 0, N_W1), ("b1", B1, 128), ("w2", W2, 128), ("b2", B2, 1)):
        for vname, val in (("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf)):
            f = base.copy()
            f[lo + (n * 2) // 3] = val
            out[f"{vname}_{tname}"] = (f, 1, lo + (n * 2) // 3)
    f = base.copy()   # several: the lowest flat index wins, also over a limit breach in front of it
    f[[B2, W2 + 3, B1 + 100, 20000, 1234]] = [np.nan, np.inf, np.nan, -np.inf, np.nan]
    f[7] = 1e30
    out["several_nonfinite"] = (f, 1, 1234)
    at_limit = np.float32(LIMIT / vc.LOG2E)
    while vc.LOG2E * float(at_limit) < LIMIT:
        at_limit = np.nextafter(at_limit, np.float32(np.inf))
    f = base.copy()
    f[100 * 198 + 50] = at_limit
    out["limit_W1"] = (f, 2, 100 * 198 + 50)
    f = base.copy()
    f[B1 + 64] = -at_limit
    out["limit_b1"] = (f, 2, B1 + 64)
    f = base.copy()   # W1 before b1, the lower W1 index first
    f[B1 + 1] = 1e20
    f[9000] = -1e20
    f[300] = 3e38
    out["limit_several"] = (f, 2, 300)
    f = base.copy()   # column 193: 15 x the limit breaks it, 14 x does not (then column 195 further on does)
    f[2 * 198 + 193] = np.float32(14.0) * at_limit
    f[3 * 198 + 195] = np.float32(15.5) * at_limit
    out["limit_195"] = (f, 2, 3 * 198 + 195)
    return out


@pytest.fixture(scope="module")
def pack_results(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("pack_cases")
    names, paths = [], []
    for name, case in {**accepted_sets(), **rejected_sets()}.items():
        p = d / f"{len(names)}.bin"
        np.asarray(case[0], np.float32).tofile(p)
        names.append(name)
        paths.append(str(p))
    lines = [json.loads(x) for x in _run(exe, ["pack", *paths]).strip().splitlines()]
    assert len(lines) == len(names)
    return dict(zip(names, lines))


def test_pack_equals_build_fragments_on_accepted_sets(pack_results):
    acc = accepted_sets()
    assert len(acc) >= len(vc.weight_sets()) + 7
    for name, (_, e) in acc.items():
        r = pack_results[name]
        print(name, r)
        assert r["host_rule"] == 0 and r["rule"] == 0, name
        assert r["e"] == r["host_e"] == e, name
        assert r["frag_equal"] and r["copies_equal"] and r["b2_ok"] and not r["untouched"], name
    # the cases are what they claim to be
    assert pack_results["lo_subnormal"]["lo_subnormal"] > 10000
    assert pack_results["tiny"]["e"] == 13 and pack_results["under_b1"]["e"] == -11


def test_rejections_report_the_hosts_rule_and_index_and_write_nothing(pack_results):
    rej = rejected_sets()
    assert len(rej) >= 17
    for name, (_, rule, index) in rej.items():
        r = pack_results[name]
        print(name, r)
        assert r["host_rule"] == rule and r["host_index"] == index, name   # the case is what it claims
        assert r["rule"] == rule and r["index"] == index, name
        assert r["untouched"] and not r["frag_equal"], name


def test_episode_offsets_equal_cumsum(exe, tmp_path):
    rng = np.random.default_rng(11)
    args, want = [], []
    for k, n in enumerate(OFFS_SIZES):
        hdr = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
        lens = rng.integers(0, 301, size=n)
        if n >= 2:
            lens[0], lens[-1] = 300, 0
        hdr[:, 3] = lens
        hdr.tofile(tmp_path / f"h{k}.bin")
        args += [str(tmp_path / f"h{k}.bin"), str(n), str(tmp_path / f"o{k}.bin")]
        want.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    _run(exe, ["offs", *args])
    for k, n in enumerate(OFFS_SIZES):
        got = np.fromfile(tmp_path / f"o{k}.bin", dtype=np.int32)
        assert got.shape == (n + 1,), n
        assert np.array_equal(got, want[k]), n
