"""python -m bgx.learn: self-play + batched TD updates through bgx.learner.Learner.

Prints one JSON line with the keys of tools/train_loop.py (the loop that goes
through the host at every step, kept as the comparison) plus env_steps_per_s
and gpu_busy_share, the event-timed step and update time over the wall time.
The learner updates on whatever a chunk's harvest holds, so episodes_per_update
is the run's mean: choose --steps-per-chunk for the batch size wanted (4,096
lanes finish about 41 episodes per env step once the games have spread out: a
chunk of 48 steps some 2,000 episodes, one of 5 steps some 200).
--deterministic trains on every harvest in canonical order (Learner
deterministic=True), so that a run repeats to the bit; the line then also has
deterministic, params_sha256 (Learner.digest()) and canon_s, the event-timed
seconds the reordering took.
"""
import argparse
import json
import time

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m bgx.learn", description=__doc__.split("\n\n")[0])
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps-per-chunk", type=int, default=48, metavar="S",
                    help="env steps of every lane between two harvests (one update per non-empty harvest)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lam", type=float, default=0.0, help="lambda of the lambda-return targets (0: TD(0))")
    ap.add_argument("--zero-sum", action="store_true", help="zero-sum targets (DeviceTrainer zero_sum=True)")
    ap.add_argument("--afterstates", action="store_true", help="fit V on afterstates (DeviceTrainer afterstates=True)")
    ap.add_argument("--deterministic", action="store_true",
                    help="train on every harvest in canonical order (Learner deterministic=True): a run repeats to the "
                         "bit; the line then carries params_sha256 and canon_s")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the final weights (W1 b1 w2 b2) to this .npz")
    ap.add_argument("--eval-games", type=int, default=0, metavar="G",
                    help="after the last update: G games of the final weights against the initial ones, 1-ply greedy")
    args = ap.parse_args(argv)
    import torch

    from .learner import Learner
    kw = {"deterministic": True} if args.deterministic else {}
    ln = Learner(args.lanes, args.steps_per_chunk, seed=args.seed, lam=args.lam, zero_sum=args.zero_sum,
                 afterstates=args.afterstates, **kw)
    w_init = ln.weights()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.updates > 1:
        ln.run(updates=args.updates - 1)
        ln.metrics(reset=True)   # so that the last read below covers the last update alone
    ln.run(updates=1)
    ln.sync()
    el = time.perf_counter() - t0
    m = ln.metrics(reset=True)
    w = ln.weights()
    env_steps = ln.chunks * ln.steps_per_chunk * ln.lanes
    train_s = ln.gpu_ms["update"] / 1e3
    out = {"updates": ln.updates, "episodes_trained": ln.episodes, "env_steps": env_steps, "wall_s": el,
           "train_s": train_s, "updates_per_s": ln.updates / el, "train_episodes_per_s": ln.episodes / train_s,
           "train_share": train_s / el, "last_loss": m["loss"], "version": ln.version,
           "temperature": float(ln.temperature(ln.version)), "batched": True, "backend": "hip",
           "episodes_per_update": ln.episodes / max(1, ln.updates), "lam": ln.trainer.lam,
           "zero_sum": ln.trainer.zero_sum, "afterstates": ln.trainer.afterstates,
           "env_steps_per_s": env_steps / el, "trained_episodes_per_s": ln.episodes / el,
           "gpu_busy_share": (ln.gpu_ms["step"] + ln.gpu_ms["update"] + ln.gpu_ms["canon"]) / 1e3 / el,
           "lanes": ln.lanes, "steps_per_chunk": ln.steps_per_chunk, "chunks": ln.chunks}
    if args.deterministic:
        out.update({"deterministic": True, "params_sha256": ln.digest(), "canon_s": ln.gpu_ms["canon"] / 1e3})
    ln.close()
    if args.save:
        np.savez(args.save, **{k: np.asarray(v) for k, v in w.items()})
    if args.eval_games > 0:
        from .match import play
        res = play(w, w_init, games=args.eval_games, ply=1, greedy=True)
        out.update({"games": res["games"], "ppg": res["ppg"], "ppg_se": res["ppg_se"]})
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
