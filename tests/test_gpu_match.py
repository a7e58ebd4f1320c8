"""Match mode on the GPU: two networks head to head on the phased engine.

Network 0 (Engine.set_weights) and network 1 (Engine.set_opponent); player p
of episode k on global lane g is played by network (p ^ g ^ k) & 1, and the
mover's network evaluates everything its step needs (include/bgx.h,
bgx_engine_set_opponent; csrc/bgx_match.hip). The trained checkpoint and the
untrained weights of tests/golden are the two networks: their values differ by
more than 1 on every test position, so a row evaluated under the wrong network
cannot pass a 1e-5 check.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
from test_gpu_parity import _random_positions
from test_gpu_scale import _check_headers, _check_lane_w, _kall_scores, _peek_step

pytestmark = pytest.mark.gpu
V_TOL = 1e-5


def _engine(w0, w1, **kw):
    from bgx import Engine
    e = Engine(**kw)
    e.set_weights(w0, temperature=1.5, version=1)
    if w1 is not None:
        e.set_opponent(w1)
    return e


def _raw(h):
    return h.headers.cpu().numpy().view(np.uint32).copy(), h.records.cpu().numpy().view(np.uint32).copy()


# ---------------------------------------------------------------- 1. the routed kernel alone
@pytest.fixture(scope="module")
def value_ref(weights_ckpt, weights_seed0):
    """1,000 random placements: V under each network from bgx_value_boards (the
    bits the routed launch must reproduce) and from the oracle, computed once."""
    import torch
    from bgx import ops
    pos = _random_positions(31, 1000)
    boards = np.stack([p[0] for p in pos])
    pl = np.array([p[1] for p in pos], np.uint8)
    W = [weights_ckpt, weights_seed0]
    nets = [ops.Net(w) for w in W]
    bt, pt = torch.from_numpy(boards).cuda(), torch.from_numpy(pl).cuda()
    own = np.stack([n.value_boards(bt, pt).cpu().numpy() for n in nets])
    x = orc.encode_many(boards, pl)
    ref = np.stack([orc.value(w, x) for w in W])
    return dict(nets=nets, boards=bt, player=pt, own=own, ref=ref)


@pytest.mark.parametrize("n", [1, 31, 33, 65, 1000])
def test_value_boards_routed_is_value_boards_of_each_rows_network(value_ref, n):
    """bgx_value_boards_routed (route_ids_kernel + mlp_kernel_routed, NT = 1) at
    a single row, one tile minus / plus one row, two tiles plus one and many
    tiles on many workgroups, ids all 0, all 1, alternating and random: every
    V bit-equal to bgx_value_boards of the row's own network and within 1e-5 of
    the oracle under that network."""
    import torch
    from bgx import ops
    r = value_ref
    rng = np.random.default_rng(n)
    pats = {"all0": np.zeros(n, np.uint8), "all1": np.ones(n, np.uint8), "alternating": (np.arange(n) & 1).astype(np.uint8),
            "random": rng.integers(0, 2, n).astype(np.uint8)}
    for tag, ids in pats.items():
        v = ops.value_boards_routed(r["nets"][0], r["nets"][1], r["boards"][:n], r["player"][:n],
                                    torch.from_numpy(ids).cuda()).cpu().numpy()
        own = r["own"][ids, np.arange(n)]
        assert np.array_equal(v.view(np.uint32), own.view(np.uint32)), (tag, int(np.sum(v != own)))
        err = np.abs(v - r["ref"][ids, np.arange(n)])
        assert err.max() < V_TOL, (tag, float(err.max()))


# ---------------------------------------------------------------- 2. one network on both sides
def _episodes_raw(e, steps, chunk):
    """{(lane, episode no.): (header words 3.., its records)} over `steps` steps."""
    out, done = {}, 0
    while done < steps:
        k = min(chunk, steps - done)
        e.step(k)
        hdr, rec = _raw(e.harvest())
        o = 0
        for row in hdr:
            m = int(row[3])
            out[(int(row[0]), int(row[1]))] = (row[3:].copy(), rec[o:o + m].copy())
            o += m
        done += k
    e.sync()
    return out


@pytest.mark.parametrize("ply,k_top,lanes,steps", [(1, 4, 96, 400), (2, 4, 64, 40), (2, 0, 64, 40)])
def test_same_network_on_both_sides_equals_self_play(weights_seed0, ply, k_top, lanes, steps):
    """set_opponent(the same weights) against the same engine out of match
    mode (sampling, seed 3): headers and records bit-identical. Routing neither
    loses, duplicates nor perturbs a row: every V the step kernel reads has the
    bits of the unrouted launches, whichever list, tile and column it took."""
    runs = []
    for match in (True, False):
        e = _engine(weights_seed0, weights_seed0 if match else None, lanes=lanes, seed=3, ply=ply, k_top=k_top,
                    fused=False)
        eps = _episodes_raw(e, steps, chunk=200)
        # (40 steps finish few games: the lanes' positions, movers and rolls after them, too)
        runs.append((eps, [e.peek(k).copy() for k in ("lane_rows", "player", "dice")]))
        e.close()
    (a, sa), (b, sb) = runs
    assert a.keys() == b.keys() and (ply == 2 or len(a) > 50)
    for key in a:
        np.testing.assert_array_equal(a[key][0], b[key][0], err_msg=str(key))
        np.testing.assert_array_equal(a[key][1], b[key][1], err_msg=str(key))
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------- 3. / 4. two networks, 1-ply
def _decode(hdr, rec):
    """Record fields plus, per record, the mover's network from its header."""
    import torch
    from bgx.episodes import decode_records
    d = decode_records(hdr, torch.from_numpy(rec.view(np.int32)).cuda())
    lens = hdr[:, 3].astype(np.int64)
    lane = np.repeat(hdr[:, 0].astype(np.int64), lens)
    ep = np.repeat(hdr[:, 1].astype(np.int64), lens)
    d["net"] = (d["mover"].astype(np.int64) ^ lane ^ ep) & 1
    return d


def _check_decision(W, d, k):
    """Decision k under its mover's network W[net]: greedy = the oracle's
    argmax within 2e-5, V(s) and V(a) within 1e-5. Returns whether the other
    network's best candidate scores more than 1e-3 above the move played."""
    net, mover = int(d["net"][k]), int(d["mover"][k])
    b, dice = d["before"][k], d["dice"][k]
    cnt, res, _ = orc.movegen(b, mover, int(dice[0]), int(dice[1]))
    m = min(cnt, 500)
    a = int(d["action"][k])
    assert 0 <= a < m
    x = orc.encode_many(res[:m], [mover] * m)
    v = orc.value(W[net], x)
    assert v[a] >= v.max() - 2 * V_TOL, (k, net, a, float(v[a]), float(v.max()))
    vs = orc.value(W[net], orc.encode_many(b[None], [mover]))[0]
    assert abs(vs - d["v_s"][k]) < V_TOL and abs(v[a] - d["v_a"][k]) < V_TOL, (k, net, vs, d["v_s"][k], v[a], d["v_a"][k])
    vo = orc.value(W[1 - net], x)
    return bool(vo.max() - vo[a] > 1e-3)


def test_two_networks_1ply_each_mover_plays_its_own_argmax(weights_ckpt, weights_seed0):
    """ckpt (network 0) against seed0 (network 1), greedy 1-ply, 96 lanes, 600
    steps: the episode bookkeeping of test_gpu_scale._check_headers, and for a
    seeded sample of 3,000 decisions the move played is the oracle's argmax
    under the mover's network (from the header's lane and episode no.), with
    the record's V(s) / V(a) within 1e-5 of that network's values. In at least
    25 % of them the other network would have played a move it values more than
    1e-3 higher (the CPU oracle alone: 74 % of 3,430 decisions), so the check
    tells the networks apart."""
    W = [weights_ckpt, weights_seed0]
    e = _engine(W[0], W[1], lanes=96, seed=3, ply=1, greedy=True, fused=False)
    harvests = []
    for _ in range(3):
        e.step(200)
        harvests.append(_raw(e.harvest()))
    e.sync()
    e.close()
    assert _check_headers(harvests, 96) > 100
    hdr = np.concatenate([h for h, _ in harvests])
    rec = np.concatenate([r for _, r in harvests])
    d = _decode(hdr, rec)
    m = d["action"].shape[0]
    assert m >= 3000, m
    assert 0.3 < d["net"].mean() < 0.7
    ks = np.random.default_rng(2026).choice(m, 3000, replace=False)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:   # ctypes drops the GIL
        other = list(ex.map(lambda k: _check_decision(W, d, int(k)), ks))
    share = float(np.mean(other))
    print(f"decisions {m}, checked {len(other)}, other network prefers another move in {share:.3f}")
    assert share >= 0.25, share


@pytest.mark.parametrize("lanes", [1, 2])
def test_two_networks_degenerate_lane_counts(weights_ckpt, weights_seed0, lanes):
    """1 and 2 lanes, 300 steps: at most steps one of the two row lists is
    empty (1 lane: always), the other a single partial tile. Every decision of
    the finished games is checked as above; no error flags at sync()."""
    W = [weights_ckpt, weights_seed0]
    e = _engine(W[0], W[1], lanes=lanes, seed=5, ply=1, greedy=True, fused=False)
    harvests = []
    for _ in range(2):
        e.step(150)
        harvests.append(_raw(e.harvest()))
    e.sync()
    s = e.stats()
    e.close()
    assert s["env_steps"] == 300 * lanes
    assert _check_headers(harvests, lanes) >= 1
    d = _decode(np.concatenate([h for h, _ in harvests]), np.concatenate([r for _, r in harvests]))
    m = d["action"].shape[0]
    assert m > 20 and len(set(d["net"].tolist())) == 2
    for k in range(m):
        _check_decision(W, d, k)


# ---------------------------------------------------------------- 5. two networks, 2-ply
@pytest.mark.parametrize("k_top", [4, 0])
def test_two_networks_2ply_values_and_argmax(weights_ckpt, weights_seed0, k_top):
    """2-ply greedy, 48 lanes, ckpt against seed0. One peeked step: every
    lane's candidates, their V and the W of every scored candidate (from
    job_val) within 1e-5 of orc.value / orc.two_ply_response under the mover's
    network (test_gpu_scale._check_lane_w with that network's weights). Then
    ~300 sampled decisions equal the oracle's argmax of 1.0 V - 0.9 W under the
    mover's network within 2e-5 (K = 4: over the top 4 by V; fewer than 4
    moves: the 1-ply argmax)."""
    from test_gpu_replay import _two_ply_scores
    W = [weights_ckpt, weights_seed0]
    lanes = 48
    e = _engine(W[0], W[1], lanes=lanes, seed=7, ply=2, k_top=k_top, greedy=True)
    e.step(30)
    hdr0, _ = _raw(e.harvest())
    epi = np.bincount(hdr0[:, 0].astype(np.int64), minlength=lanes)   # each lane's current episode no.
    before, after = _peek_step(e)
    net = (before["player"].astype(np.int64) ^ np.arange(lanes) ^ epi) & 1
    assert len(set(net.tolist())) == 2
    e.step(70)
    hdr, rec = _raw(e.harvest())
    e.sync()
    e.close()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        nw = list(ex.map(lambda i: _check_lane_w(W[int(net[i])], lanes, before, after, i), range(lanes)))
    assert sum(nw) >= (100 if k_top == 4 else 300), sum(nw)

    d = _decode(hdr, rec)
    m = d["action"].shape[0]
    assert m >= 300, m
    ks = np.random.default_rng(11).choice(m, 300, replace=False)

    def one(k):
        w = W[int(d["net"][k])]
        a = int(d["action"][k])
        board, mover, dice = d["before"][k], int(d["mover"][k]), d["dice"][k]
        if k_top == 0:
            s = _kall_scores(w, board, mover, *dice)
            return "2ply", s[a] >= s.max() - 2 * V_TOL, (a, float(s[a]), float(s.max()))
        r = _two_ply_scores(w, board, mover, *dice, 4)
        if r[0] is None:
            v = r[1]
            return "1ply", v[a] >= v.max() - V_TOL, (a, float(v[a]), float(v.max()))
        cand, score, v = r
        if a not in set(cand.tolist()):   # only a V tie at the top-4 boundary moves a candidate in or out
            return "tie", abs(v[a] - v[cand[-1]]) < V_TOL, (a, float(v[a]), float(v[cand[-1]]))
        return "2ply", score[list(cand).index(a)] >= score.max() - 2 * V_TOL, (a, score.tolist())

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(one, ks))
    for k, (kind, ok, info) in zip(ks, res):
        assert ok, (int(k), kind, int(d["net"][k]), info)
    assert sum(kind == "2ply" for kind, _, _ in res) >= 150


# ---------------------------------------------------------------- 6. / 7. bgx.match.play
def test_play_tally_equals_recount_from_records(weights_ckpt, weights_seed0):
    """play() at 64 lanes x 2 games: exactly two counted games per lane
    (episodes 0 and 1), and its tally equals an independent recount from the
    decoded records (the winner is the mover of the record that ends the game,
    its engine network (mover ^ lane ^ episode) & 1, the points its win type)."""
    from bgx.match import play
    from bgx.records import fields
    r = play(weights_ckpt, weights_seed0, games=128, lanes=64, seed=9, return_episodes=True)
    hdr, rec = r["headers"], r["records"]
    assert r["games"] == 128 and r["games_per_lane"] == 2
    assert sorted(zip(hdr[:, 0].tolist(), hdr[:, 1].tolist())) == [(g, k) for g in range(64) for k in (0, 1)]
    f = fields(rec)
    last = np.cumsum(hdr[:, 3].astype(np.int64)) - 1
    done, wt, mover = f["done"][last], f["win_type"][last], f["mover"][last]
    assert np.array_equal(done, wt > 0)
    net = (mover.astype(np.int64) ^ hdr[:, 0].astype(np.int64) ^ hdr[:, 1].astype(np.int64)) & 1   # engine network
    net = net ^ r["engine_net_of_a"]   # 0: play's first argument
    pts = [int(wt[done & (net == k)].sum()) for k in (0, 1)]
    names = {1: "regular", 2: "gammon", 3: "backgammon"}
    wins = [{names[t]: int(np.sum(done & (net == k) & (wt == t))) for t in (1, 2, 3)} for k in (0, 1)]
    assert r["points"] == pts and r["wins"] == wins and r["unfinished"] == int(np.sum(~done))
    assert r["ppg"] == pytest.approx((pts[0] - pts[1]) / 128)


def test_play_swap_symmetry(weights_ckpt, weights_seed0):
    """play(a, b) and play(b, a) with the same seed, 64 lanes x 2 games: the two
    tallies are each other's mirror.

    The engine's seat rule names its networks, so play() decides which of the
    two becomes the engine's network 0 from the weights alone, not from the
    argument order: both calls play the same games and report them from their
    own first argument's side."""
    from bgx.match import play
    ab = play(weights_ckpt, weights_seed0, games=128, lanes=64, seed=9)
    ba = play(weights_seed0, weights_ckpt, games=128, lanes=64, seed=9)
    print("a vs b:", ab["wins"], ab["points"], ab["unfinished"], "b vs a:", ba["wins"], ba["points"], ba["unfinished"])
    assert ab["games"] == ba["games"] == 128
    assert ab["wins"] == ba["wins"][::-1] and ab["points"] == ba["points"][::-1]
    assert ab["unfinished"] == ba["unfinished"] and ab["ppg"] == -ba["ppg"] and ab["ppg_se"] == ba["ppg_se"]
    assert ab["engine_net_of_a"] == 1 - ba["engine_net_of_a"]
    assert sum(ab["wins"][0].values()) + sum(ab["wins"][1].values()) + ab["unfinished"] == 128


def test_each_network_wins_a_game_of_512(weights_ckpt, weights_seed0):
    """ckpt against seed0, 512 greedy 1-ply games: each network wins at least
    one (nothing is asserted about which one is stronger)."""
    from bgx.match import play
    r = play(weights_ckpt, weights_seed0, games=512, lanes=256, seed=1)
    print({k: r[k] for k in ("wins", "points", "unfinished", "ppg", "ppg_se", "seconds")})
    assert r["games"] == 512
    assert sum(r["wins"][0].values()) >= 1 and sum(r["wins"][1].values()) >= 1


# ---------------------------------------------------------------- entering, leaving, refusing
def test_set_opponent_states(weights_ckpt, weights_seed0, monkeypatch):
    """Match mode needs the phased engine and the full reply evaluation
    (BGX_E_STATE = -4 on a fused engine and with BGX_REPLY_DELTA=1); entering
    and leaving restart every lane, so a left engine replays self-play from the
    reset; replacing network 1 while in match mode does not restart; with
    BGX_GRAPH=1 a match engine launches directly and plays the same games."""
    from bgx import BgxError, Engine
    e = Engine(lanes=64, seed=3, ply=1)   # fused
    e.set_weights(weights_seed0)
    with pytest.raises(BgxError, match=r"\(-4\).*phased"):
        e.set_opponent(weights_ckpt)
    e.close()
    monkeypatch.setenv("BGX_REPLY_DELTA", "1")
    e = Engine(lanes=64, seed=3, ply=2, k_top=4)
    monkeypatch.delenv("BGX_REPLY_DELTA")
    e.set_weights(weights_seed0)
    with pytest.raises(BgxError, match=r"\(-4\).*BGX_REPLY_DELTA"):
        e.set_opponent(weights_ckpt)
    e.close()

    ref = _engine(weights_seed0, None, lanes=64, seed=3, ply=1, fused=False)
    want = _episodes_raw(ref, 200, chunk=100)
    ref.close()
    e = _engine(weights_seed0, weights_ckpt, lanes=64, seed=3, ply=1, fused=False)
    e.set_opponent(None)           # out again before any step, and back in
    e.set_opponent(weights_ckpt)
    e.step(50)
    e.harvest()
    before = e.stats()["episodes"]
    e.set_opponent(weights_seed0)  # replaces network 1 only: the lanes keep their games
    assert e.stats()["episodes"] == before
    e.step(10)
    e.set_opponent(None)           # leaves match mode: every lane back at the reset
    assert e.stats()["episodes"] == 0
    got = _episodes_raw(e, 200, chunk=100)
    e.close()
    assert len(want) > 20 and want.keys() == got.keys()
    for key in want:
        np.testing.assert_array_equal(want[key][0], got[key][0], err_msg=str(key))
        np.testing.assert_array_equal(want[key][1], got[key][1], err_msg=str(key))

    runs = []
    for g in ("1", "0"):
        monkeypatch.setenv("BGX_GRAPH", g)
        e = _engine(weights_ckpt, weights_seed0, lanes=64, seed=3, ply=1, greedy=True, fused=False)
        runs.append(_episodes_raw(e, 120, chunk=60))
        e.close()
    assert len(runs[0]) > 10 and runs[0].keys() == runs[1].keys()
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key][1], runs[1][key][1], err_msg=str(key))
