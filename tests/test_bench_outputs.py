"""bench.py --dump-outputs: the decoder on a synthetic harvest (no GPU), and
on the GPU a plain run's line and two dumping runs that write the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from bgx.records import EP_WORDS, pack_record  # noqa: E402


def _packed(board, flag):
    w = np.zeros(7, np.uint32)
    for i in range(48):
        w[i // 8] |= np.uint32(board[i]) << np.uint32(4 * (i % 8))
    w[6] = board[48] | board[49] << 4 | board[50] << 8 | board[51] << 12 | flag << 16
    return w


def test_dump_outputs_decodes_a_harvest(tmp_path):
    """Three episodes in harvest order (lanes 5, 2, 5; the later episode of lane
    5 first): the files list them by (lane, episode no.) with each episode's own
    records, every field decoded, and nothing of a lane outside the sample."""
    rng = np.random.default_rng(3)
    lanes = 8   # < DUMP_LANES: every lane is in the sample
    eps = [(5, 7, 3), (2, 0, 2), (5, 6, 4)]   # lane, episode no., records
    headers, records, want = [], [], {}
    for lane, no, n in eps:
        final = rng.integers(0, 16, 52).astype(np.uint32)
        h = np.zeros(EP_WORDS, np.uint32)
        h[:6] = lane, no, len(records), n, 10 * n + lane, 2 | 1 << 8 | 3 << 16
        h[6:13] = _packed(final, 1)
        headers.append(h)
        rows = []
        for k in range(n):
            b = rng.integers(0, 16, 52).astype(np.uint32)
            f = dict(mover=k % 2, v_s=float(rng.random()), v_a=float(rng.random()), reward=float(k == n - 1),
                     action=int(rng.integers(0, 2048)), n_moves=int(rng.integers(1, 4096)), step=3 * k + 1,
                     dice=(int(rng.integers(1, 7)), int(rng.integers(1, 7))), done=k == n - 1, close_out=k % 2 == 0,
                     prime=k % 3 == 0, win_type=2 if k == n - 1 else 0)
            records.append(pack_record(_packed(b, f["mover"]), **f))
            rows.append(np.concatenate([[lane, no], b, [f["mover"]], np.float32([f["v_s"], f["v_a"], f["reward"]]),
                                        [f["action"], f["n_moves"], f["step"], *f["dice"], f["done"], f["close_out"],
                                         f["prime"], f["mover"], f["win_type"]]]).astype(np.float32))
        want[(lane, no)] = (np.concatenate([[lane, no, n, 10 * n + lane, 2, 1, 3], final, [1]]).astype(np.float32),
                            np.stack(rows))
    counters = dict(env_steps=100, decisions=9, episodes=3, value_rows=1234, movegen_jobs=77, gap_rows=0)
    bench.dump_outputs(str(tmp_path), np.stack(headers).view(np.int32), np.stack(records).view(np.int32), 0, lanes,
                       counters)
    e, r, s = (np.load(tmp_path / f"{n}.npy") for n in ("episodes", "records", "stats"))
    assert e.dtype == np.float32 and r.dtype == np.float32 and s.dtype == np.float64
    order = sorted(want)
    np.testing.assert_array_equal(e, np.stack([want[k][0] for k in order]))
    np.testing.assert_array_equal(r, np.concatenate([want[k][1] for k in order]))
    np.testing.assert_array_equal(s, [100, 9, 3, 1234, 77])
    # a lane base that puts every episode outside the sample: empty files of the same widths
    bench.dump_outputs(str(tmp_path / "none"), np.stack(headers).view(np.int32), np.stack(records).view(np.int32),
                       1000, lanes, counters)
    assert np.load(tmp_path / "none" / "episodes.npy").shape == (0, e.shape[1])
    assert np.load(tmp_path / "none" / "records.npy").shape == (0, r.shape[1])


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--lanes", "1024", "--steps",
                        "90", "--warmup", "10", "--desync-steps", "300", "--harvest-every", "30", *args],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1   # the JSON line is stdout's only line
    return json.loads(out[0])


@pytest.mark.gpu
def test_dump_outputs_is_reproducible_and_plain_run_is_lean(tmp_path):
    """Two runs with the same arguments write identical files that hold finished
    episodes of the 90 timed steps' last harvest; the line times exactly --steps
    steps and, without --full, carries none of the side measurements."""
    lines = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 90 and line["ms_per_step"] > 0 and line["env_steps_per_rank"] == [1024 * 90]
        assert abs(line["value"] - 1024 * 90 / (90 * line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        assert line["roofline"] is None and line["kernels"] is None and line["cpu_baseline"] is None
        assert not any(k in line for k in ("two_ply_k4", "two_ply_kall", "configs1_4096_lanes", "configs2_4096_lanes"))
        assert {"metric", "unit", "higher_is_better", "dtype"} <= set(line)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) == ["episodes.npy", "records.npy", "stats.npy"]
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b, err_msg=f)
        total += a.nbytes
    assert total <= 64 << 20
    e, r, s = (np.load(tmp_path / "a" / f) for f in files)
    assert len(e) > 0 and len(r) == e[:, 2].sum() and len(np.unique(e[:, 0])) <= bench.DUMP_LANES
    assert np.all(np.diff(e[:, 0] * 1e6 + e[:, 1]) > 0)   # by (lane, episode no.), each once
    assert s[0] == 1024 * 90
