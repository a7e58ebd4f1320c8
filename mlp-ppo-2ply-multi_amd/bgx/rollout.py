"""Position rollouts: play given positions out and tally the results on the device.

What is this position worth under this checkpoint, and how often does the
player on roll win a gammon from it? `rollout(weights, boards, player)` plays
every position `trials` times to the end on the phased engine and counts the
results. In rollout mode (include/bgx.h, bgx_engine_set_start) global lane g
plays position g % n_pos in every one of its episodes, with the given player on
roll and no starter roll; the first roll of a trial is the position's fixed
dice, or the stratified roll of trial t (t % 36 runs over the 36 ordered rolls,
so every position sees each of them equally often), or a roll from the lane's
stream. Every harvest is tallied on the device (bgx_rollout_tally): only the
final counts [n_pos, 8] cross to the host.

  python -m bgx.rollout CKPT (--positions FILE.npz | --opening) --trials N
         [--ply 2 --k-top 4 --sample --no-stratify --seed S --lanes L]

prints one JSON line. FILE.npz holds boards [n, 52] (positions_0[24] |
positions_1[24] | bar[2] | off[2]), player [n] and optionally dice [n, 2];
--opening is the 15 non-double opening rolls on the initial board with player
0 to play: what the checkpoint thinks each opening roll is worth.
`check_positions`, `tally_counts` and `summarize` are pure numpy (no GPU, no
libbgx.so).
"""
from __future__ import annotations

import math

import numpy as np

from .records import EP_WORDS, REC_WORDS, WIN_TYPES, episode_bounds

# counts[pos] words (bgx_rollout_tally): 0..2 regular / gammon / backgammon wins of
# the player on roll, 3..5 of the other player, 6 unfinished, 7 env steps
COUNT_WORDS = 8
_POINTS = np.array([1, 2, 3, -1, -2, -3, 0], np.int64)

INITIAL_BOARD = np.array([2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 3, 0, 5, 0, 0, 0, 0, 0,
                          0, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0],
                         np.uint8)


def check_positions(boards, player, dice=None):
    """The rules of bgx_engine_set_start on the host: every board within the
    input domain (counts <= 15, no point held by both players, at most 15
    checkers a side), exactly 15 checkers per player (points + bar + off), not
    already over (15 off), player 0 / 1, dice 0, 0 (= roll) or two values in
    1..6. Returns (boards uint8 [n, 52], player uint8 [n], dice uint8 [n, 2]);
    raises ValueError naming the first bad index."""
    b = np.asarray(boards)
    if b.size == 0 or b.size % 52:
        raise ValueError("boards must be [n, 52] with n >= 1")
    b = b.reshape(-1, 52).astype(np.int64)
    n = b.shape[0]
    p = np.asarray(player).reshape(-1).astype(np.int64)
    if p.shape[0] != n:
        raise ValueError(f"{n} boards, {p.shape[0]} players")
    d = np.zeros((n, 2), np.int64) if dice is None else np.broadcast_to(np.asarray(dice), (n, 2)).astype(np.int64)
    for i in range(n):
        x = b[i]
        sums = (int(x[:24].sum() + x[48] + x[50]), int(x[24:48].sum() + x[49] + x[51]))
        if x.min() < 0 or x.max() > 15:
            raise ValueError(f"position {i}: a count outside 0..15")
        if np.any((x[:24] > 0) & (x[24:48] > 0)):
            raise ValueError(f"position {i}: a point holds checkers of both players")
        if sums != (15, 15):
            raise ValueError(f"position {i}: {sums[0]} and {sums[1]} checkers (15 each: points + bar + off)")
        if x[50] >= 15 or x[51] >= 15:
            raise ValueError(f"position {i}: already over (15 checkers off)")
        if p[i] not in (0, 1):
            raise ValueError(f"position {i}: player {p[i]} (0 or 1)")
        d0, d1 = int(d[i, 0]), int(d[i, 1])
        if not (d0 == 0 and d1 == 0) and not (1 <= d0 <= 6 and 1 <= d1 <= 6):
            raise ValueError(f"position {i}: dice {d0}, {d1} (0, 0 = roll, or two values in 1..6)")
    return b.astype(np.uint8), p.astype(np.uint8), d.astype(np.uint8)


def tally_counts(headers, start_player, n_pos, max_episode):
    """The numpy statement of rollout_tally_kernel: uint64 [n_pos, 8] from
    episode headers (uint32 / int32 [n, 16], host). Header h counts for position
    lane % n_pos, seen from start_player[pos]; headers with episode no. >=
    max_episode are skipped."""
    h = np.ascontiguousarray(headers).view(np.uint32).reshape(-1, EP_WORDS)
    sp = np.asarray(start_player).reshape(-1).astype(np.int64)
    n_pos = int(n_pos)
    h = h[h[:, 1].astype(np.int64) < int(max_episode)]
    pos = (h[:, 0].astype(np.int64) % n_pos)
    wt = (h[:, 5] & 0xFF).astype(np.int64)
    winner = ((h[:, 5] >> 8) & 1).astype(np.int64)
    slot = np.where(wt == 0, 6, np.where(winner == (sp[pos] & 1), 0, 3) + np.minimum(wt, 3) - 1)
    counts = np.zeros((n_pos, COUNT_WORDS), np.uint64)
    np.add.at(counts, (pos, slot), np.uint64(1))
    np.add.at(counts, (pos, np.full_like(pos, 7)), h[:, 4].astype(np.uint64))
    return counts


def summarize(counts) -> list:
    """Per position of counts [n_pos, 8]: games; wins {"on_roll", "other"} keyed
    by records.WIN_TYPES; unfinished games (win type 0, no points); `equity`,
    the points per game of the player on roll (1 / 2 / 3 per win type);
    `equity_se`, its standard error from the exact per-game point distribution
    the counts imply (sample standard deviation / sqrt(games); 0.0 below two
    games); `mean_steps`, env steps per game."""
    c = np.asarray(counts).astype(np.uint64).reshape(-1, COUNT_WORDS)
    out = []
    for row in c:
        k = [int(v) for v in row]
        n = sum(k[:7])
        s1 = sum(int(x) * v for x, v in zip(_POINTS, k[:7]))        # sum of points (exact integers)
        s2 = sum(int(x) * int(x) * v for x, v in zip(_POINTS, k[:7]))
        var_n = n * s2 - s1 * s1                                    # n^2 x the population variance
        se = math.sqrt(var_n / (n * (n - 1)) / n) if n > 1 else 0.0
        out.append({"games": n,
                    "wins": {"on_roll": {WIN_TYPES[t]: k[t - 1] for t in (1, 2, 3)},
                             "other": {WIN_TYPES[t]: k[2 + t] for t in (1, 2, 3)}},
                    "unfinished": k[6],
                    "equity": s1 / n if n else 0.0,
                    "equity_se": se,
                    "mean_steps": k[7] / n if n else 0.0})
    return out


def plan(n_pos, trials, lanes, stratify):
    """(J lanes per position, G games per lane, strat_stride): J = max(1,
    min(lanes // n_pos, trials)), G = ceil(trials / J), with `stratify` rounded
    up to the next G with J * G % 36 == 0 (J * G trials are played)."""
    n_pos, trials, lanes = int(n_pos), int(trials), int(lanes)
    if n_pos <= 0 or trials <= 0 or lanes <= 0:
        raise ValueError("positions, trials and lanes must be positive")
    J = max(1, min(lanes // n_pos, trials))
    G = -(-trials // J)
    if stratify:
        while (J * G) % 36:
            G += 1
    return J, G, (J if stratify else 0)


def rollout(weights, boards, player, dice=None, trials=1296, lanes=8192, ply=1, k_top=4, greedy=True,
            temperature=1.5, seed=0, stratify=True, max_steps=300, opponent=None, device=None,
            return_episodes=False, chunk=128) -> dict:
    """Play every position out `trials` times under `weights`: `positions` =
    summarize(counts) (one entry per position), `counts` (uint64 [n_pos, 8]), the
    run's parameters, env steps and wall time.

    The engine gets n_pos * J lanes (see `plan`): lane g plays position g %
    n_pos, and every lane plays exactly G games (only episodes with episode no.
    < G count, bgx/match.py's rule), so each position is played J * G times
    (`trials`, >= the trials asked for). With `stratify` the first rolls that
    are rolled are stratified: trial t = k * J + g // n_pos of a position (game
    k of lane g) starts with roll t % 36 of the 36 ordered rolls. The engine is
    stepped `chunk` env steps at a time and harvested after each; from a late
    position a game can be a single env step long, so the engine is created
    with ep_cap = lanes * chunk (+ slack): the episode list cannot overflow.
    The loop is bounded by G * max_steps steps (asserted). Each harvest is
    tallied on the device; only the final counts are copied to the host, and,
    once as many episodes have been harvested as games are needed (a number the
    harvest gives on the host), the 8-byte total of games counted so far after
    each harvest. `env_steps` = steps x lanes is everything the engine stepped,
    including the uncounted games (episode no. >= G) that lanes play while the
    slowest lane finishes; `tallied_steps` is the env steps of the counted games
    alone (the sum of counts[:, 7]), the useful work.

    `opponent`: a second network plays by match mode (Engine.set_opponent):
    `weights` are network 0, `opponent` network 1, and player p of game k on
    lane g is played by network (p ^ g ^ k) & 1, so the player on roll of a
    position is network 0 in half of its trials (`networks` in the result says
    so); return_episodes gives the headers to split the results by seat.

    return_episodes adds the counted games' `headers` and `records` (uint32
    host arrays, bgx/records.py; each episode's records contiguous, in header
    order with first-record offsets rewritten)."""
    b, p, d = check_positions(boards, player, dice)   # on the host, before any engine exists
    import time

    import torch

    from . import ops
    from .engine import Engine
    n_pos = int(b.shape[0])
    J, G, stride = plan(n_pos, trials, lanes, stratify)
    L = n_pos * J
    max_steps, chunk = int(max_steps), int(chunk)
    ring = 1024
    while ring < max_steps + 1:
        ring <<= 1
    chunk = max(1, min(chunk, ring - max_steps))
    e = Engine(lanes=L, seed=seed, ply=ply, k_top=k_top, device=device, greedy=greedy, fused=False, ring=ring,
               max_steps=max_steps, ep_cap=L * chunk + 1024)
    try:
        e.set_weights(weights, temperature=temperature)
        if opponent is not None:
            e.set_opponent(opponent)
        e.set_start(b, p, d if dice is not None else None, strat_stride=stride)
        with torch.cuda.device(e.device):
            counts = torch.zeros((n_pos, COUNT_WORDS), dtype=torch.int64, device=e.device)
            sp = torch.from_numpy(p).to(e.device)
            bound = G * max_steps
            need, got, steps, seen = L * G, 0, 0, 0
            hdrs, recs = [], []
            t0 = time.perf_counter()
            while got < need:
                assert steps < bound, f"{got} of {need} games after {steps} steps (bound {bound})"
                n = min(chunk, bound - steps)
                e.step(n)
                hv = e.harvest(clone=False)
                steps += n
                if hv.n_episodes:
                    ops.rollout_tally(hv.headers, sp, n_pos, G, counts)
                    if return_episodes:
                        h = hv.headers.cpu().numpy().view(np.uint32).reshape(-1, EP_WORDS)
                        r = hv.records.cpu().numpy().view(np.uint32).reshape(-1, REC_WORDS)
                        keep = h[:, 1] < G
                        offs, _ = episode_bounds(h)
                        hdrs.append(h[keep])
                        recs += [r[offs[i]:offs[i + 1]] for i in np.nonzero(keep)[0]]
                    # the counted games are among the harvested ones (a host number):
                    # the device total is read only once it can be complete
                    seen += hv.n_episodes
                    if seen >= need:
                        got = int(counts[:, :7].sum().item())
            e.sync()
            seconds = time.perf_counter() - t0
            assert got == need, (got, need)
            host = counts.cpu().numpy().view(np.uint64)
    finally:
        e.close()
    out = {"positions": summarize(host), "counts": host, "n_positions": n_pos, "trials": J * G,
           "trials_asked": int(trials), "lanes": L, "lanes_per_position": J, "games_per_lane": G,
           "strat_stride": stride, "stratify": bool(stratify), "ply": int(ply), "k_top": int(k_top),
           "greedy": bool(greedy), "temperature": float(temperature), "seed": int(seed), "max_steps": max_steps,
           "chunk": chunk, "env_steps": steps * L, "tallied_steps": int(host[:, 7].sum()), "seconds": seconds,
           "networks": ("player p of game k on lane g: network (p ^ g ^ k) & 1 (0 = weights, 1 = opponent)"
                        if opponent is not None else "weights on both sides")}
    if return_episodes:
        headers = np.concatenate(hdrs) if hdrs else np.zeros((0, EP_WORDS), np.uint32)
        headers = headers.copy()
        lens = headers[:, 3].astype(np.int64)
        headers[:, 2] = (np.cumsum(lens) - lens).astype(np.uint32)
        out["headers"] = headers
        out["records"] = np.concatenate(recs) if recs else np.zeros((0, REC_WORDS), np.uint32)
    return out


def opening_positions():
    """The 15 non-double opening rolls (d0 > d1) on the initial board, player 0
    to play: (boards [15, 52], player [15], dice [15, 2])."""
    rolls = [(a, c) for a in range(6, 0, -1) for c in range(a - 1, 0, -1)]
    return (np.stack([INITIAL_BOARD] * len(rolls)), np.zeros(len(rolls), np.uint8), np.array(rolls, np.uint8))


def main(argv=None):
    import argparse
    import json

    from .ops import load_pth
    ap = argparse.ArgumentParser(prog="python -m bgx.rollout", description="play positions out under a checkpoint")
    ap.add_argument("ckpt", help="checkpoint (.pth state_dict, or .npz with W1 b1 w2 b2)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--positions", help=".npz with boards [n, 52], player [n] and optionally dice [n, 2]")
    src.add_argument("--opening", action="store_true", help="the 15 non-double opening rolls, player 0 to play")
    ap.add_argument("--trials", type=int, required=True)
    ap.add_argument("--lanes", type=int, default=8192)
    ap.add_argument("--ply", type=int, default=1, choices=(1, 2))
    ap.add_argument("--k-top", type=int, default=4, choices=(0, 4))
    ap.add_argument("--sample", action="store_true", help="sample moves from softmax(score / T) instead of argmax")
    ap.add_argument("--temperature", type=float, default=1.5)
    ap.add_argument("--no-stratify", action="store_true", help="roll every first roll from the lane's stream")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    def load(path):
        if path.endswith(".npz"):
            w = np.load(path)
            return {k: w[k] for k in ("W1", "b1", "w2", "b2")}
        return load_pth(path)

    if args.opening:
        boards, player, dice = opening_positions()
    else:
        f = np.load(args.positions)
        boards, player, dice = f["boards"], f["player"], (f["dice"] if "dice" in f.files else None)
    res = rollout(load(args.ckpt), boards, player, dice, trials=args.trials, lanes=args.lanes, ply=args.ply,
                  k_top=args.k_top, greedy=not args.sample, temperature=args.temperature, seed=args.seed,
                  stratify=not args.no_stratify)
    del res["counts"]
    if dice is not None:
        for pos, dd in zip(res["positions"], np.asarray(dice).reshape(-1, 2)):
            pos["dice"] = [int(dd[0]), int(dd[1])]
    res.update(ckpt=args.ckpt, source="opening" if args.opening else args.positions)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
