#!/usr/bin/env python3
"""Self-play + training on one GPU without Python Episode objects (SURVEY §8f
rows 1-3 together): the engine plays, every finished episode's compact
records feed DeviceTrainer.update_records in the reference's batches of 200
(--episodes-per-update N for others; --batched --backend hip for the multi-CU update;
--lam L for TD(lambda) targets and --zero-sum for targets that take the next
record from the opponent's side where the mover changes, --afterstates to fit V
on the board after each move under the mover's indicator, the positions the
engine rates; all three with --batched --backend hip or --backend torch), and each update's weights go straight back
into the engine with the reference temperature schedule
(ParameterManager.get_temperature). --eval-games G then plays the final weights
against the initial ones (bgx.match.play, 1-ply greedy) and adds games, ppg and
its standard error to the JSON line; --save PATH writes the final weights as an
.npz that `python -m bgx.match` reads."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mlp-ppo-2ply-multi_amd")]
from bgx import Engine  # noqa: E402
from bgx.net import BackgammonPolicyNetwork  # noqa: E402
from bgx.ops import weights_from  # noqa: E402
from bgx.trainer import DeviceTrainer  # noqa: E402


class LocalPM:
    """Versioned weights + temperature schedule (parameter_manager.py:79-111), single process."""

    def __init__(self, sd):
        self.sd, self.version = {k: v.detach().cpu() for k, v in sd.items()}, 1

    def get_parameters(self, device=None):
        return {k: v.to(device) if device else v for k, v in self.sd.items()}

    def set_parameters(self, sd):
        self.sd = {k: v.detach().cpu() for k, v in sd.items()}
        self.version += 1

    def get_temperature(self):
        v = self.version
        return 1.5 if v <= 1 else (0.5 if v >= 4001 else 1.5 - (v - 1) / 4000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--backend", default=None, choices=("hip", "torch"),
                    help="unset: hip for the sequential update, torch for --batched (DeviceTrainer's rule)")
    ap.add_argument("--episodes-per-update", type=int, default=200, metavar="N",
                    help="episodes per trainer update (the reference's batch is 200)")
    ap.add_argument("--lam", type=float, default=0.0,
                    help="lambda of the lambda-return targets (0: TD(0), the reference's)")
    ap.add_argument("--zero-sum", action="store_true",
                    help="zero-sum targets (DeviceTrainer zero_sum=True): 1 - x of the next record where the mover changes")
    ap.add_argument("--afterstates", action="store_true",
                    help="fit V on afterstates (DeviceTrainer afterstates=True): the board after each move, the mover's indicator")
    ap.add_argument("--eval-games", type=int, default=0, metavar="G",
                    help="after the last update: G games of the final weights against the initial ones, 1-ply greedy")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the final weights (W1 b1 w2 b2) to this .npz")
    args = ap.parse_args()
    per = args.episodes_per_update
    torch.manual_seed(0)
    pm = LocalPM(BackgammonPolicyNetwork().state_dict())
    trainer = DeviceTrainer(pm, device="cuda", batch_episode_size=per, batched=args.batched, backend=args.backend,
                            lam=args.lam, zero_sum=args.zero_sum, afterstates=args.afterstates)
    eng = Engine(lanes=args.lanes, seed=0)
    w = dict(zip(("W1", "b1", "w2", "b2"), weights_from(pm.get_parameters())))
    w_init = {k: np.array(v, copy=True) for k, v in w.items()}
    eng.set_weights(w, pm.get_temperature(), pm.version)
    hdr_buf, rec_buf = [], []
    done, steps, t0, t_train = 0, 0, time.perf_counter(), 0.0
    while done < args.updates:
        eng.step(50)
        steps += 50
        h = eng.harvest()
        if h.n_episodes:
            hdr_buf.append(h.headers.cpu())
            rec_buf.append(h.records)
        n = sum(x.shape[0] for x in hdr_buf)
        while n >= per and done < args.updates:
            hdr, rec = torch.cat(hdr_buf), torch.cat(rec_buf)
            k = int(hdr[:per, 3].sum())
            t1 = time.perf_counter()
            m = trainer.update_records(hdr[:per], rec[:k])
            torch.cuda.synchronize()
            t_train += time.perf_counter() - t1
            hdr_buf, rec_buf = [hdr[per:]], [rec[k:]]
            n -= per
            done += 1
            w = dict(zip(("W1", "b1", "w2", "b2"), weights_from(pm.get_parameters())))
            eng.set_weights(w, pm.get_temperature(), pm.version)
    el = time.perf_counter() - t0
    eng.close()
    out = {}
    if args.save:
        np.savez(args.save, **{k: np.asarray(v) for k, v in w.items()})
    if args.eval_games > 0:
        from bgx.match import play
        res = play(w, w_init, games=args.eval_games, ply=1, greedy=True)
        out = {"games": res["games"], "ppg": res["ppg"], "ppg_se": res["ppg_se"]}
    print(json.dumps({"updates": done, "episodes_trained": per * done, "env_steps": steps * args.lanes,
                      "wall_s": el, "train_s": t_train, "updates_per_s": done / el,
                      "train_episodes_per_s": per * done / t_train, "train_share": t_train / el, "last_loss": m["loss"],
                      "version": pm.version, "temperature": pm.get_temperature(), "batched": args.batched,
                      "backend": trainer.backend, "episodes_per_update": per, "lam": trainer.lam, "zero_sum": trainer.zero_sum,
                      "afterstates": trainer.afterstates,
                      **out}))


if __name__ == "__main__":
    main()
