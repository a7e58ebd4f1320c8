"""The canonical harvest order (csrc/bgx_canon.h) on the host
(tests/cpuwave/canon_emu.cpp under the wave emulation, built with
AddressSanitizer and UBSan; a stand-alone program run as a subprocess).

Well-formed harvests: headers, records and offsets against
numpy.lexsort((episode, lane)) plus a host gather, byte for byte, at every
shape of CASES (the wave, workgroup-chunk and multi-chunk edges of the episode
count; one lane, few lanes, the LDS form's last lane count and the workspace
form beyond it), in a random, the sorted and the reversed arrival order; a
heavy lane of 200 episodes; episode numbers above 2^31; lane_base 0 and 8192.

Malformed headers (a lane below / above the range, a duplicated key, word 3
summing above / below the record count): the status bit, and no access outside
the arrays (every buffer is allocated at exactly its size).
"""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LANE_RANGE, DUPLICATE, RECORDS = 1, 2, 4   # BGX_CANON_* (include/bgx.h)

# (n_eps, lanes) of the well-formed cases; 5,000 lanes is past CN_LDS_LANES (the workspace form of the index launch)
SHAPES = [(n, lanes) for n in (0, 1, 2, 63, 64, 65) for lanes in (1, 64, 300)] + \
         [(n, lanes) for n in (1023, 1024, 1025, 2049, 5000) for lanes in (300, 4096)] + [(65, 5000), (2049, 5000)]
HEAVY = (2049, 300)      # the shape whose lane 7 holds 200 episodes
HIGH = (1025, 300)       # the shape whose episode numbers straddle 2^31 within a lane


def make_case(n, lanes, seed, lane_base=0, heavy=0, high=False):
    """A well-formed harvest in key order: (headers uint32 [n, 16], records uint32
    [m, 12]). Episode numbers per lane are distinct, not consecutive and do not
    start at 0; lengths run 0 .. 300, the first 300 and the last 0."""
    rng = np.random.default_rng(seed)
    lane = rng.integers(0, lanes, size=n)
    if heavy:
        lane[rng.choice(n, size=heavy, replace=False)] = min(7, lanes - 1)
    lane = np.sort(lane)
    ep = np.zeros(n, np.uint64)
    for l in np.unique(lane):
        k = int((lane == l).sum())
        first = 2 ** 31 - 6 + int(rng.integers(0, 4)) if high else 3 + int(rng.integers(0, 50))
        ep[lane == l] = first + np.cumsum(rng.integers(1, 5, size=k))
    hdr = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
    hdr[:, 0] = lane + lane_base
    hdr[:, 1] = ep.astype(np.uint32)
    lens = rng.integers(0, 301, size=n)
    if n >= 2:
        lens[0], lens[-1] = 300, 0
    hdr[:, 3] = lens
    rec = rng.integers(0, 2 ** 32, size=(int(lens.sum()), 12), dtype=np.uint64).astype(np.uint32)
    return hdr, rec


def relaid(hdr, rec, order):
    """The same episodes arriving in `order` (a permutation of the headers)."""
    offs = np.concatenate([[0], np.cumsum(hdr[:, 3].astype(np.int64))])
    rows = [np.arange(offs[i], offs[i + 1]) for i in order]
    idx = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    return np.ascontiguousarray(hdr[order]), np.ascontiguousarray(rec[idx])


def canonical(hdr, rec):
    """numpy's statement of bgx_harvest_canonical: (headers, records, offs int32)."""
    order = np.lexsort((hdr[:, 1], hdr[:, 0]))   # by lane, then by episode number, unsigned
    h, r = relaid(hdr, rec, order)
    return h, r, np.concatenate([[0], np.cumsum(h[:, 3].astype(np.int64))]).astype(np.int32)


def arrival_orders(n, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.permutation(n), "sorted": np.arange(n), "reversed": np.arange(n)[::-1]}


def well_formed_cases():
    """[(name, lane_base, lanes, headers as they arrive, records, canonical triple)]"""
    out = []
    for k, (n, lanes) in enumerate(SHAPES):
        lane_base = 8192 if k % 2 else 0
        hdr, rec = make_case(n, lanes, seed=100 + k, lane_base=lane_base, heavy=200 if (n, lanes) == HEAVY else 0,
                             high=(n, lanes) == HIGH)
        want = canonical(hdr, rec)
        assert np.array_equal(want[0], hdr)   # make_case builds in key order
        for oname, order in arrival_orders(n, seed=k).items():
            h, r = relaid(hdr, rec, order)
            out.append((f"n{n}_l{lanes}_{oname}", lane_base, lanes, h, r, want))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    out = tmp_path_factory.mktemp("canon_emu") / "canon_emu"
    subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), "-x", "c++", os.path.join(HERE, "cpuwave", "canon_emu.cpp"),
                    "-o", str(out), "-pthread"], check=True, capture_output=True, text=True)
    return str(out)


def run_cases(exe, d, cases):
    """cases: [(lane_base, lanes, hdr, rec)] -> [(status, headers, records, offs)]"""
    args = []
    for k, (lane_base, lanes, hdr, rec) in enumerate(cases):
        hdr.astype(np.uint32).tofile(d / f"h{k}.bin")
        rec.astype(np.uint32).tofile(d / f"r{k}.bin")
        args += [str(d / f"h{k}.bin"), str(d / f"r{k}.bin"), str(len(hdr)), str(len(rec)), str(lane_base), str(lanes),
                 str(d / f"o{k}")]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0"}
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]   # a sanitizer report ends the program
    lines = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert len(lines) == len(cases)
    out = []
    for k, line in enumerate(lines):
        out.append((line["status"], np.fromfile(d / f"o{k}.hdr", dtype=np.uint32).reshape(-1, 16),
                    np.fromfile(d / f"o{k}.rec", dtype=np.uint32).reshape(-1, 12),
                    np.fromfile(d / f"o{k}.offs", dtype=np.int32)))
    return out


def test_the_cases_are_what_they_claim():
    hdr, _ = make_case(*HEAVY, seed=1, heavy=200)
    assert np.bincount(hdr[:, 0]).max() >= 200
    hdr, _ = make_case(*HIGH, seed=2, high=True)
    straddles = [l for l in np.unique(hdr[:, 0])
                 if (hdr[hdr[:, 0] == l, 1] >= 2 ** 31).any() and (hdr[hdr[:, 0] == l, 1] < 2 ** 31).any()]
    assert len(straddles) >= 10
    for n, lanes in ((65, 64), (1025, 300)):
        hdr, rec = make_case(n, lanes, seed=3)
        key = (hdr[:, 0].astype(np.int64) << 32) | hdr[:, 1].astype(np.int64)
        assert len(np.unique(key)) == n and (np.diff(key) > 0).all()
        per_lane = [hdr[hdr[:, 0] == l, 1] for l in np.unique(hdr[:, 0])]
        assert all(e[0] > 0 for e in per_lane) and any((np.diff(e.astype(np.int64)) > 1).any() for e in per_lane)
        assert hdr[0, 3] == 300 and hdr[-1, 3] == 0 and len(rec) == hdr[:, 3].sum()


def test_canonical_order_equals_lexsort_and_gather(exe, tmp_path):
    cases = well_formed_cases()
    assert len(cases) == 3 * len(SHAPES)
    got = run_cases(exe, tmp_path, [(b, l, h, r) for _, b, l, h, r, _ in cases])
    for (name, _, _, h, r, want), (status, gh, gr, go) in zip(cases, got):
        assert status == 0, name
        assert go.shape == want[2].shape and np.array_equal(go, want[2]), name
        assert gh.tobytes() == want[0].tobytes(), name
        assert gr.tobytes() == want[1].tobytes(), name


def malformed_cases():
    """{name: (lane_base, lanes, hdr, rec, expected status bit)}"""
    out = {}
    hdr, rec = make_case(130, 64, seed=7, lane_base=8192)
    h = hdr.copy()
    h[17, 0] = 8191
    out["lane_below"] = (8192, 64, h, rec, LANE_RANGE)
    h = hdr.copy()
    h[101, 0] = 8192 + 64
    out["lane_above"] = (8192, 64, h, rec, LANE_RANGE)
    h = hdr.copy()
    h[88, 0] = 3   # far below a non-zero base: wraps as unsigned
    out["lane_far_below"] = (8192, 64, h, rec, LANE_RANGE)
    h = hdr.copy()
    h[40, :2] = h[9, :2]
    out["duplicate_key"] = (8192, 64, h, rec, DUPLICATE)
    h = hdr.copy()
    h[60, 3] += 55   # word 3 sums above the records given: nothing may be read past them
    out["records_above"] = (8192, 64, h, rec, RECORDS)
    h = hdr.copy()
    h[0, 3] -= 100
    out["records_below"] = (8192, 64, h, rec, RECORDS)
    h = hdr.copy()
    h[5, 3] = 0xFFFFFF00   # one word 3 past every bound (the sum wraps)
    out["records_huge"] = (8192, 64, h, rec, RECORDS)
    hdr2, rec2 = make_case(1500, 5000, seed=8)   # the workspace form
    h = hdr2.copy()
    h[700, 0] = 5000
    h[20, :2] = h[1400, :2]
    out["workspace_form"] = (0, 5000, h, rec2, LANE_RANGE | DUPLICATE)
    return out


def test_malformed_headers_set_their_status_bit_and_stay_in_bounds(exe, tmp_path):
    cases = malformed_cases()
    rng = np.random.default_rng(5)
    names, runs = [], []
    for name, (b, l, h, r, _) in cases.items():
        if not name.startswith("records"):   # (relaid gathers by word 3, which those cases break)
            h, r = relaid(h, r, rng.permutation(len(h)))
        names.append(name)
        runs.append((b, l, h, r))
    got = run_cases(exe, tmp_path, runs)
    for name, (status, gh, gr, go) in zip(names, got):
        bit = cases[name][4]
        assert status & bit == bit, (name, status)
        assert gh.shape == runs[names.index(name)][2].shape and go.shape == (len(gh) + 1,), name
