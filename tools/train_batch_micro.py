#!/usr/bin/env python3
"""Batched-trainer micro-benchmark (tools only): one harvest of self-play
episodes (repeated to reach the larger sizes), then per size

  batched_hip   one bgx_td0_update_batched call, event-timed on the stream
  lambda_hip    (--lam L) one bgx_tdlambda_update_batched call on the same
                records in the same process, event-timed the same way
  zero_sum_hip  (--lam L --zero-sum) one bgx_td_update_batched call with
                BGX_TDF_ZERO_SUM, likewise
  afterstate_hip (--lam L --zero-sum --afterstates) one
                bgx_td_afterstate_update_batched call with BGX_TDF_ZERO_SUM on
                the same records and their headers, likewise
  sequential    one bgx_td0_update call on the same records, event-timed
  batched_torch DeviceTrainer(batched=True, backend="torch").update_records,
                wall clock around a synchronize (an eager path: its host work
                is the path)

as the median of --reps runs after a warm-up. Prints one JSON line with
episodes/s and records/s of each and the batched call's TFLOP/s, counting
3 x 2 x 198 x 128 FLOP per record (forward, recomputed forward, dW1) against
the 157.3 TF f32-MFMA peak. --only hip runs the batched call alone (for a
kernel trace, which gives the launches' shares)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mlp-ppo-2ply-multi_amd"), os.path.join(REPO, "tools")]
from bgx import Engine  # noqa: E402
from bgx._lib import check, lib, ptr, stream_handle  # noqa: E402
from bgx.net import BackgammonPolicyNetwork  # noqa: E402
from bgx import ops  # noqa: E402
from bgx.ops import weights_from  # noqa: E402
from bgx.trainer import DeviceTrainer  # noqa: E402
from train_loop import LocalPM  # noqa: E402

FLOP_PER_RECORD = 3 * 2 * 198 * 128
PEAK_TF = 157.3


def harvest(n_eps):
    """headers (host) and records (device) of n_eps episodes: one harvest, repeated as needed."""
    pm = LocalPM(BackgammonPolicyNetwork().state_dict())
    eng = Engine(lanes=4096, seed=0)
    eng.set_weights(dict(zip(("W1", "b1", "w2", "b2"), weights_from(pm.get_parameters()))), 1.5, 1)
    eng.step(300)
    h = eng.harvest()
    hdr, rec = h.headers.cpu(), h.records.clone()
    eng.close()
    k = min(n_eps, hdr.shape[0])
    hdr = hdr[:k]
    rec = rec[:int(hdr[:, 3].sum())]
    reps = -(-n_eps // k)
    hdr = hdr.repeat(reps, 1)[:n_eps].clone()
    rec = rec.repeat(reps, 1)[:int(hdr[:, 3].sum())].contiguous()
    return pm, hdr, rec


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def flat_state(pm, dev):
    sd = pm.get_parameters()
    p = torch.cat([sd[k].reshape(-1) for k in DeviceTrainer._KEYS]).float().to(dev).contiguous()
    return p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 2000, 20000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("hip",), default=None)
    ap.add_argument("--torch-max-reps", type=int, default=5)
    ap.add_argument("--lam", type=float, default=None,
                    help="also time bgx_tdlambda_update_batched with this lambda beside the TD(0) call")
    ap.add_argument("--zero-sum", action="store_true",
                    help="with --lam: also time bgx_td_update_batched with BGX_TDF_ZERO_SUM beside the lambda call")
    ap.add_argument("--afterstates", action="store_true",
                    help="with --lam --zero-sum: also time bgx_td_afterstate_update_batched beside the zero-sum call")
    args = ap.parse_args()
    if args.zero_sum and args.lam is None:
        ap.error("--zero-sum needs --lam")
    if args.afterstates and not args.zero_sum:
        ap.error("--afterstates needs --lam and --zero-sum")
    dev =torch.device("cuda")
    torch.manual_seed(0)
    pm, hdr_all, rec_all = harvest(max(args.sizes))
    out = []
    for n_eps in args.sizes:
        hdr = hdr_all[:n_eps]
        lens = hdr[:, 3].numpy().astype(np.int64)
        n_rec = int(lens.sum())
        rec = rec_all[:n_rec].contiguous()
        offs = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
        row = {"episodes": n_eps, "records": n_rec}
        # ---- the batched HIP entries, each timed by name on the same records from a fresh state
        def batched_ms(entry, **kw):
            p, m, v, step = flat_state(pm, dev)
            work = torch.empty(ops.td_batched_workspace(entry, n_rec), dtype=torch.uint8, device=dev)
            return event_ms(lambda: ops.td_batched(entry, records=rec, offs=offs, n_eps=n_eps, n_rec=n_rec,
                                                   state=(p, m, v, step), lr=1e-3, gamma=0.99, clip=1.0, metrics=met,
                                                   work=work, stream=stream, **kw), args.reps)

        def rates(ms):
            return {"ms": ms, "episodes_per_s": n_eps / ms * 1e3, "records_per_s": n_rec / ms * 1e3}

        met = torch.zeros(5, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream()
        ms = batched_ms("bgx_td0_update_batched")
        row["batched_hip"] = {**rates(ms), "tflops": n_rec * FLOP_PER_RECORD / ms * 1e-9,
                              "of_f32_mfma_peak": n_rec * FLOP_PER_RECORD / ms * 1e-9 / PEAK_TF}
        if args.lam is not None:
            # the same launches and the target stage between forward and backward
            ms_l = batched_ms("bgx_tdlambda_update_batched", lam=args.lam)
            row["lambda_hip"] = {"lam": args.lam, **rates(ms_l), "over_td0": ms_l / ms}
        if args.zero_sum:
            # the lambda call's launches with the target stage's zero-sum instance
            ms_z = batched_ms("bgx_td_update_batched", lam=args.lam, flags=ops.TDF_ZERO_SUM)
            row["zero_sum_hip"] = {"lam": args.lam, **rates(ms_z), "over_lambda": ms_z / ms_l,
                                   "extra_us": (ms_z - ms_l) * 1e3}
        if args.afterstates:
            # the zero-sum call's launches on afterstate rows
            ms_a = batched_ms("bgx_td_afterstate_update_batched", headers=hdr.to(torch.int32).contiguous().to(dev),
                              lam=args.lam, flags=ops.TDF_ZERO_SUM)
            row["afterstate_hip"] = {"lam": args.lam, **rates(ms_a), "over_zero_sum": ms_a / ms_z,
                                     "extra_us": (ms_a - ms_z) * 1e3}
        if args.only is None:
            # ---- the sequential kernel (one Adam step per episode)
            p, m, v, step = flat_state(pm, dev)
            s = stream_handle(stream)

            def sequential():
                check(lib().bgx_td0_update(ptr(rec), ptr(offs), n_eps, ptr(p), ptr(m), ptr(v), ptr(step), 1e-3, 0.99,
                                           1.0, ptr(met), s))

            ms = event_ms(sequential, min(args.reps, 5))
            row["sequential"] = rates(ms)
            # ---- the eager torch batched path
            tr = DeviceTrainer(pm, device="cuda", batch_episode_size=n_eps, batched=True, backend="torch")
            reps = min(args.torch_max_reps, args.reps) if n_eps <= 2000 else 2
            tr.update_records(hdr, rec)
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                tr.update_records(hdr, rec)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ms = statistics.median(ts)
            row["batched_torch"] = {"ms": ms, "runs": reps, "episodes_per_s": n_eps / ms * 1e3,
                                    "records_per_s": n_rec / ms * 1e3}
        out.append(row)
    print(json.dumps({"sizes": out}))


if __name__ == "__main__":
    main()
