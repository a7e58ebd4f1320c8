#!/usr/bin/env python3
"""What match mode costs: the MLP slot of a phased engine step in match mode
against the same engine out of match mode, with the same network on both sides
so that both engines play identical games (tests/test_gpu_match.py checks the
records are bit-identical).

Out of match mode the MLP slot of bgx_get_timing is the root launch (and at
ply 2 the reply launch) of bgx_launch_mlp; in match mode it is, per phase, the
routing kernel plus mlp_kernel_routed (csrc/bgx_match.hip). Running the
unrouted kernel once per network over all rows would cost exactly 2x; the
routed path has to come in under that to have a reason to exist.

  python tools/match_bench.py [--lanes 8192] [--steps 200] [--desync 150] [--reps 3]

prints one JSON line: per configuration the MLP slot's ms per step in both
modes (median of --reps timed windows of --steps steps), their ratio, and the
wall-clock ms per step.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mlp-ppo-2ply-multi_amd"))


def measure(weights, match, lanes, steps, desync, reps, **kw):
    from bgx import Engine
    e = Engine(lanes=lanes, seed=0, fused=False, **kw)
    e.set_weights(weights, temperature=1.5)
    if match:
        e.set_opponent(weights)
    chunk = min(100, e.max_steps_per_call)

    def run(n):
        left = n
        while left > 0:
            k = min(chunk, left)
            e.step(k)
            e.harvest(clone=False)
            left -= k

    run(desync)   # the lanes spread over their games
    mlp, wall, rows = [], [], []
    for _ in range(reps):
        s0 = e.stats()
        e.set_timing(True)   # events between the kernels
        run(steps)
        t = e.timing()
        e.set_timing(False)
        s1 = e.stats()
        mlp.append(t["mlp_ms"] / steps)
        rows.append((s1["value_rows"] - s0["value_rows"]) / steps)
        e.sync()
        t0 = time.perf_counter()   # the same number of steps untimed: wall clock, harvests included
        run(steps)
        e.sync()
        wall.append((time.perf_counter() - t0) * 1e3 / steps)
    e.close()
    return {"mlp_ms_per_step": statistics.median(mlp), "wall_ms_per_step": statistics.median(wall),
            "value_rows_per_step": statistics.median(rows), "mlp_ms_windows": mlp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--desync", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    d = np.load(os.path.join(REPO, "tests", "golden", "weights_seed0.npz"))
    w = {k: d[k] for k in ("W1", "b1", "w2", "b2")}
    out = {"lanes": args.lanes, "steps": args.steps}
    for name, kw in (("1ply_phased", dict(ply=1)), ("2ply_k4", dict(ply=2, k_top=4))):
        base = measure(w, False, args.lanes, args.steps, args.desync, args.reps, **kw)
        match = measure(w, True, args.lanes, args.steps, args.desync, args.reps, **kw)
        out[name] = {"self_play": base, "match": match,
                     "mlp_ratio": match["mlp_ms_per_step"] / base["mlp_ms_per_step"],
                     "wall_ratio": match["wall_ms_per_step"] / base["wall_ms_per_step"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
