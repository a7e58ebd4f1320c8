"""Match play: two networks head to head on the phased engine.

Does checkpoint B play better than checkpoint A? `play(a, b, games)` lets the
two networks play `games` games against each other on one device and counts
the results. In match mode (include/bgx.h, bgx_engine_set_opponent) network 0
is the one `Engine.set_weights` sets, network 1 the one `Engine.set_opponent`
sets, and player p of episode k on global lane g is played by network
(p ^ g ^ k) & 1: the seats swap from lane to lane and from game to game, so
each network plays PLAYER1 (who is decided by the starter roll to move first
or second) in half the games. Who played which side of a harvested game follows
from (lane, episode no.) in its header; `tally` turns headers into a result.

  python -m bgx.match A.pth B.pth --games 65536 [--ply 2 --k-top 4 --lanes L --sample]

prints one JSON line (index 0 of `wins` / `points` is A, index 1 is B; ppg > 0: A is ahead).
`tally` and `net_of_player0` are pure numpy (no GPU, no libbgx.so).
"""
from __future__ import annotations

import numpy as np

from .records import EP_WORDS, REC_WORDS, WIN_TYPES, episode_bounds


def net_of_player0(lane, episode):
    """The network (0 / 1) in PLAYER1's seat (player 0) in episode `episode` of
    global lane `lane` (numpy arrays or ints); player 1 has the other one."""
    return ((np.asarray(lane).astype(np.int64) ^ np.asarray(episode).astype(np.int64)) & 1).astype(np.int64)


def _per_game(headers):
    """(winning network or -1, points) per header."""
    h = np.ascontiguousarray(headers).view(np.uint32).reshape(-1, EP_WORDS)
    wt = (h[:, 5] & 0xFF).astype(np.int64)
    winner = ((h[:, 5] >> 8) & 0xFF).astype(np.int64)
    net = np.where(wt > 0, net_of_player0(h[:, 0], h[:, 1]) ^ (winner & 1), -1)
    pts = np.where(wt > 0, np.minimum(wt, 3), 0)
    return wt, net, pts


def tally(headers) -> dict:
    """The result of the match games in `headers` (uint32 / int32 [n, 16], host):
    games; per network the regular / gammon / backgammon wins (`wins`, keyed by
    records.WIN_TYPES) and points (1 / 2 / 3 per win type); `unfinished`, the
    games that hit max_steps with win type 0 (no points to either side); `ppg`
    = (points of network 0 - points of network 1) / games and `ppg_se`, the
    standard error of that mean from the per-game point differences (sample
    standard deviation / sqrt(games); 0.0 with fewer than two games)."""
    wt, net, pts = _per_game(headers)
    n = int(wt.shape[0])
    wins = [{WIN_TYPES[t]: int(np.sum((net == k) & (wt == t))) for t in (1, 2, 3)} for k in (0, 1)]
    points = [int(np.sum(pts[net == k])) for k in (0, 1)]
    diff = np.where(net == 0, pts, -pts).astype(np.float64)
    ppg = float(diff.mean()) if n else 0.0
    se = float(diff.std(ddof=1) / np.sqrt(n)) if n > 1 else 0.0
    return {"games": n, "wins": wins, "points": points, "unfinished": int(np.sum(wt == 0)), "ppg": ppg, "ppg_se": se}


def play(weights_a, weights_b, games, lanes=4096, ply=1, k_top=4, greedy=True, temperature=1.5, seed=0,
         device=None, ring=1024, max_steps=300, reply_sample=0, return_episodes=False) -> dict:
    """weights_a against weights_b: the `tally` of lanes * G games, G =
    ceil(games / lanes), with a as index 0 and b as index 1 of `wins` /
    `points` (`ppg` = (points of a - points of b) / games), plus the run's
    parameters, env steps and wall time.

    The result does not depend on the order of the arguments: play(b, a) is
    the exact mirror of play(a, b). The engine's seat rule names its networks
    (network 0 sits in PLAYER1's seat of game (lane, episode) when lane ^
    episode is even), so which of the two becomes the engine's network 0 is
    decided by the weights alone (the smaller SHA-256 of their fp32 bytes), not
    by the argument order, and the tally is turned to the caller's order
    afterwards; `engine_net_of_a` says which engine network a was.

    Every lane plays exactly G games: only episodes with episode number < G
    count, and the engine steps until all lanes * G of them have arrived.
    Counting whatever finishes inside a fixed step budget instead would
    over-weight short games (a lane that happens to play long games would
    contribute fewer of them), and gammons / backgammons and one-sided games
    are not equally long. An episode takes at most max_steps env steps, so the
    loop is bounded by G * max_steps steps (asserted).

    return_episodes adds the counted games' `headers` and `records` (uint32
    host arrays, bgx/records.py; each episode's records contiguous, in header
    order with first-record offsets rewritten) to the result; the seat rule in
    them is the engine's (net_of_player0 gives the engine network)."""
    import hashlib
    import time

    from .engine import Engine
    from .ops import weights_from
    nets = [dict(zip(("W1", "b1", "w2", "b2"), weights_from(w))) for w in (weights_a, weights_b)]
    digest = [hashlib.sha256(b"".join(w[k].tobytes() for k in ("W1", "b1", "w2", "b2"))).digest() for w in nets]
    swap = digest[1] < digest[0]   # b becomes the engine's network 0
    if swap:
        nets.reverse()
    games, lanes = int(games), int(lanes)
    if games <= 0 or lanes <= 0:
        raise ValueError("games and lanes must be positive")
    lanes = min(lanes, games)
    G = -(-games // lanes)
    e = Engine(lanes=lanes, seed=seed, ply=ply, k_top=k_top, device=device, greedy=greedy, fused=False, ring=ring,
               max_steps=max_steps, reply_sample=reply_sample)
    try:
        e.set_weights(nets[0], temperature=temperature)
        e.set_opponent(nets[1])
        chunk = e.max_steps_per_call
        bound = G * int(max_steps)
        need, got, steps = lanes * G, 0, 0
        hdrs, recs = [], []
        t0 = time.perf_counter()
        while got < need:
            assert steps < bound, f"{got} of {need} games after {steps} steps (bound {bound})"
            n = min(chunk, bound - steps)
            e.step(n)
            hv = e.harvest(clone=False)
            steps += n
            h = hv.headers.cpu().numpy().view(np.uint32).reshape(-1, EP_WORDS)
            keep = h[:, 1] < G
            got += int(keep.sum())
            hdrs.append(h[keep])
            if return_episodes and h.shape[0]:
                r = hv.records.cpu().numpy().view(np.uint32).reshape(-1, REC_WORDS)
                offs, _ = episode_bounds(h)
                recs += [r[offs[i]:offs[i + 1]] for i in np.nonzero(keep)[0]]
        e.sync()
        seconds = time.perf_counter() - t0
        assert got == need, (got, need)
    finally:
        e.close()
    headers = np.concatenate(hdrs) if hdrs else np.zeros((0, EP_WORDS), np.uint32)
    out = tally(headers)
    if swap:   # the caller's order: a first
        out.update(wins=out["wins"][::-1], points=out["points"][::-1], ppg=-out["ppg"])
    out.update(engine_net_of_a=1 if swap else 0, games_per_lane=G, lanes=lanes, ply=int(ply), k_top=int(k_top),
               greedy=bool(greedy), temperature=float(temperature), seed=int(seed), reply_sample=int(reply_sample),
               env_steps=steps * lanes, seconds=seconds)
    if return_episodes:
        headers = headers.copy()
        lens = headers[:, 3].astype(np.int64)
        headers[:, 2] = (np.cumsum(lens) - lens).astype(np.uint32)
        out["headers"] = headers
        out["records"] = np.concatenate(recs) if recs else np.zeros((0, REC_WORDS), np.uint32)
    return out


def main(argv=None):
    import argparse
    import json

    from .ops import load_pth
    ap = argparse.ArgumentParser(prog="python -m bgx.match", description="two checkpoints head to head")
    ap.add_argument("a", help="checkpoint of network 0 (.pth state_dict, or .npz with W1 b1 w2 b2)")
    ap.add_argument("b", help="checkpoint of network 1")
    ap.add_argument("--games", type=int, required=True)
    ap.add_argument("--lanes", type=int, default=8192)
    ap.add_argument("--ply", type=int, default=1, choices=(1, 2))
    ap.add_argument("--k-top", type=int, default=4, choices=(0, 4))
    ap.add_argument("--sample", action="store_true", help="sample moves from softmax(score / T) instead of argmax")
    ap.add_argument("--temperature", type=float, default=1.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    def load(path):
        if path.endswith(".npz"):
            d = np.load(path)
            return {k: d[k] for k in ("W1", "b1", "w2", "b2")}
        return load_pth(path)

    res = play(load(args.a), load(args.b), args.games, lanes=args.lanes, ply=args.ply, k_top=args.k_top,
               greedy=not args.sample, temperature=args.temperature, seed=args.seed)
    res.update(a=args.a, b=args.b)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
