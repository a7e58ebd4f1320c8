"""GPU: the value-network kernels across weight ranges and batch edges.

The split-fp16 MFMA network (bgx_mlp.hip) scales W1 / b1 by 2^e and the
features by 2^-e, e chosen from the largest weight (bgx_frag.h); the two
shipped weight sets reach e = 13 and e = 11 only. These tests run every MLP
entry point under the weight sets of tests/value_cases.py (e from 13 down to
the -11 clamp, the all-zero branch, saturated and cancelling nets) on boards
that reach every entry of the feature LUT, at the batch sizes where the tile,
the block and the persistent loop turn over, and across a weight swap on a
live engine.

Tolerance rule (value_cases.tolerance): V is finite and
max|V - V64| <= max(1e-5, 4 max|V32 - V64|), V64 the oracle's fp64 value and
V32 a numpy fp32 forward; 1e-6 where V has a closed form. Each check prints
its measured error and fp32's (the table in DESIGN.md comes from these lines).
"""
import numpy as np
import pytest
import torch

import oracle as orc
import value_cases as vc

pytestmark = pytest.mark.gpu

SETS = list(vc.INTENDED_E)
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]


@pytest.fixture(scope="module")
def bgx_ops():
    from bgx import ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return ops


@pytest.fixture(scope="module")
def pool():
    """Edge boards + 500 random placements, their oracle features and the
    device copies; shared, read-only."""
    from test_gpu_parity import _random_positions
    eb, ep = vc.edge_boards()
    pos = _random_positions(77, 500)
    boards = np.ascontiguousarray(np.concatenate([eb, np.stack([p[0] for p in pos])]))
    player = np.ascontiguousarray(np.concatenate([ep, np.array([p[1] for p in pos], np.uint8)]))
    x = orc.encode_many(boards, player)
    for a in (boards, player, x):
        a.setflags(write=False)
    return {"boards": boards, "player": player, "x": x, "d_boards": torch.from_numpy(boards.copy()).cuda(),
            "d_player": torch.from_numpy(player.copy()).cuda(), "ref": {}}


def _ref(pool, name):
    """(V64, V32) of the pool under a weight set, computed once."""
    if name not in pool["ref"]:
        w = vc.weight_sets()[name]
        v64 = orc.value(w, pool["x"])
        if name in vc.CLOSED_FORM:
            assert np.abs(v64 - vc.closed_form(name, w)).max() < 1e-12
        pool["ref"][name] = (v64, vc.value_f32(w, pool["x"]))
    return pool["ref"][name]


def _assert_rule(name, what, v, v64, v32):
    v = np.asarray(v, np.float64)
    assert v.shape == v64.shape and np.isfinite(v).all(), (name, what)
    tol, e32 = vc.tolerance(name, v32, v64)
    err = float(np.abs(v - v64).max())
    ratio = err / e32 if e32 > 0 else float("nan")
    print(f"RATIO {name} | {what} | e={vc.INTENDED_E[name]} | err {err:.3g} | fp32 {e32:.3g} | ratio {ratio:.3g} | "
          f"bound {tol:.3g}")
    assert err <= tol, (name, what, err, e32, tol, int(np.abs(v - v64).argmax()))


@pytest.mark.parametrize("name", SETS)
def test_value_paths_across_weight_ranges(bgx_ops, pool, name):
    """Net.value_boards (the MFMA path) and Net.value (the fp32 path on the
    oracle's features) under every weight set, on every LUT-edge board and 500
    random placements."""
    w = vc.weight_sets()[name]
    v64, v32 = _ref(pool, name)
    net = bgx_ops.Net(w)
    got = net.value_boards(pool["d_boards"], pool["d_player"]).cpu().numpy()
    _assert_rule(name, "value_boards", got, v64, v32)
    got = net.value(torch.from_numpy(pool["x"].copy()).cuda()).cpu().numpy()
    _assert_rule(name, "value (fp32)", got, v64, v32)


def _value_boards_canary(net, d_boards, d_player, n):
    """bgx_value_boards into a buffer with 64 canary floats past out[n - 1]."""
    from bgx._lib import check, lib, ptr, stream_handle
    canary = np.float32(-12345.678)
    out = torch.full((n + 64,), float(canary), dtype=torch.float32, device="cuda")
    check(lib().bgx_value_boards(net._h, ptr(d_boards), ptr(d_player), n, ptr(out), stream_handle(None)),
          "bgx_value_boards")
    out = out.cpu().numpy()
    assert (out[n:] == canary).all(), "a write past out[n - 1]"
    assert (out[:n] != canary).all(), "a row left unwritten"
    return out[:n]


@pytest.mark.parametrize("name", ["dense_unit", "ckpt_x2^6"])
def test_value_boards_batch_edges(bgx_ops, pool, name):
    """Batch sizes around the 32-row tile, the 16-wave block (512 rows) and the
    persistent loop's second pass (32 x 16 x CUs + 33 rows): every row by the
    tolerance rule, nothing written past out[n - 1]."""
    w = vc.weight_sets()[name]
    v64, v32 = _ref(pool, name)
    net = bgx_ops.Net(w)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(314)
    m = len(pool["boards"])
    for n in (1, 31, 32, 33, 63, 65, 511, 512, 513, 1025, 32 * 16 * n_cu + 33):
        idx = rng.integers(0, m, n)
        idx[-1] = int(rng.integers(0, 3264))   # a LUT-edge row in the tail
        t = torch.from_numpy(idx).cuda()
        got = _value_boards_canary(net, pool["d_boards"][t].contiguous(), pool["d_player"][t].contiguous(), n)
        _assert_rule(name, f"value_boards n={n}", got, v64[idx], v32[idx])


def _bearoff_board():
    b = np.zeros(52, np.uint8)
    b[18:24] = (3, 2, 2, 0, 3, 1)         # PLAYER1 home, 4 borne off
    b[50] = 4
    b[24 + 0:24 + 6] = (2, 3, 0, 2, 2, 1)  # PLAYER2 home, 5 borne off
    b[51] = 5
    return b


def test_rows_do_not_depend_on_their_tile(bgx_ops, pool):
    """A row's V has the same bits whichever rows share its tile (the header
    claim of mlp_kernel_delta, for the kernels value_boards and
    value_boards_routed launch): a 1,025-row mixed batch with one whole tile of
    identical bear-off boards (which skips k-steps) equals, bit for bit, the
    same rows under a fixed permutation, 16 sampled rows each evaluated alone,
    and, routed over two nets of different e, value_boards under each row's
    own net."""
    sets = vc.weight_sets()
    rng = np.random.default_rng(2718)
    idx = rng.integers(0, len(pool["boards"]), 1025)
    boards = pool["boards"][idx].copy()
    player = pool["player"][idx].copy()
    boards[64:96] = _bearoff_board()
    player[64:96] = 1
    from test_abi import _host_check
    assert _host_check(boards, player) == (0, -1)
    perm = rng.permutation(1025)
    db, dp = torch.from_numpy(boards).cuda(), torch.from_numpy(player).cuda()
    dperm = torch.from_numpy(perm).cuda()
    single = rng.choice(1025, 14, replace=False).tolist() + [64, 1024]
    nets = {}
    for name in ("ckpt_x2^6", "seed0"):
        net = nets[name] = bgx_ops.Net(sets[name])
        v = net.value_boards(db, dp).cpu().numpy()
        x = orc.encode_many(boards, player)
        _assert_rule(name, "value_boards mixed batch", v, orc.value(sets[name], x), vc.value_f32(sets[name], x))
        assert len(np.unique(v[64:96].view(np.uint32))) == 1
        vp = net.value_boards(db[dperm].contiguous(), dp[dperm].contiguous()).cpu().numpy()
        np.testing.assert_array_equal(vp.view(np.uint32), v[perm].view(np.uint32))
        for i in single:
            v1 = net.value_boards(db[i:i + 1], dp[i:i + 1]).cpu().numpy()
            assert v1.view(np.uint32)[0] == v.view(np.uint32)[i], (name, i, v1[0], v[i])
        nets[name + "/v"] = v
    net_id = rng.integers(0, 2, 1025).astype(np.uint8)
    net_id[64:80] = 0
    net_id[80:96] = 1
    vr = bgx_ops.value_boards_routed(nets["ckpt_x2^6"], nets["seed0"], db, dp,
                                     torch.from_numpy(net_id).cuda()).cpu().numpy()
    want = np.where(net_id == 0, nets["ckpt_x2^6/v"], nets["seed0/v"])
    np.testing.assert_array_equal(vr.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def roots():
    """40 random afterstates and, from the oracle's movegen, the union of the
    opponent's reply boards to each prefix of 1, 3 and 40 of them."""
    from test_gpu_parity import _random_positions
    pos = _random_positions(41, 40)
    boards = np.stack([p[0] for p in pos])
    opp = np.array([p[1] for p in pos], np.uint8)
    reps, owner = [], []
    mass = np.zeros(40)   # the probability of the rolls the opponent can move on (the others add nothing to W)
    for i in range(40):
        for a, b in ROLLS21:
            n, res, _ = orc.movegen(boards[i], int(opp[i]), a, b)
            reps.append(res[:n])
            owner += [i] * n
            mass[i] += ((1 if a == b else 2) / 36.0) * (n > 0)
    reps = np.concatenate(reps)
    owner = np.array(owner)
    x = orc.encode_many(reps, opp[owner])
    return {"boards": boards, "opp": opp, "x": x, "owner": owner, "mass": mass, "W": {}}


@pytest.mark.parametrize("delta", ["0", "1"])
@pytest.mark.parametrize("name", ["ckpt_x2^6", "ckpt_x2^14", "bias_dominates", "zero_hidden"])
def test_two_ply_across_weight_ranges(bgx_ops, roots, name, delta, monkeypatch):
    """Net.two_ply (the reply launch's mlp_kernel_il, or with BGX_REPLY_DELTA=1
    the root launch and mlp_kernel_delta) for 1, 3 and 40 roots against the
    oracle's two_ply_response. W is a probability-weighted mean of top-5 reply
    values, so its error is bounded by the largest reply-value error: the
    tolerance rule with V32 / V64 on the union of the reply boards. With
    zero_hidden every reply value is equal and W is the closed form, V times
    the probability of the rolls that have a reply (ties in the top-5
    included)."""
    monkeypatch.setenv("BGX_REPLY_DELTA", delta)
    w = vc.weight_sets()[name]
    if name not in roots["W"]:
        roots["W"][name] = (np.array([orc.two_ply_response(w, roots["boards"][i], int(roots["opp"][i]))
                                      for i in range(40)]), orc.value(w, roots["x"]), vc.value_f32(w, roots["x"]))
    want, v64, v32 = roots["W"][name]
    if name == "zero_hidden":
        assert np.abs(want - vc.closed_form(name, w) * roots["mass"]).max() < 1e-12
        assert roots["mass"].min() < 1.0 <= roots["mass"].max() + 1e-12   # both kinds of root
    net = bgx_ops.Net(w)
    for n in (1, 3, 40):
        got = net.two_ply(torch.from_numpy(roots["boards"][:n]).cuda(),
                          torch.from_numpy(roots["opp"][:n]).cuda()).cpu().numpy()
        assert got.shape == (n,) and np.isfinite(got).all()
        sel = roots["owner"] < n
        tol, e32 = vc.tolerance(name, v32[sel], v64[sel])
        err = float(np.abs(got - want[:n]).max())
        print(f"RATIO {name} | two_ply delta={delta} n={n} | e={vc.INTENDED_E[name]} | err {err:.3g} | "
              f"fp32 {e32:.3g} | ratio {err / e32 if e32 > 0 else float('nan'):.3g} | bound {tol:.3g}")
        assert err <= tol, (name, delta, n, err, e32, tol)


# ---------------------------------------------------------------- engines

MAX_STEPS = 30   # episodes are cut every 30 steps, so 120 steps harvest four per lane


def _harvest(e):
    from bgx.episodes import decode_records
    h = e.harvest()
    hdr = h.headers.cpu().numpy().view(np.uint32)
    d = decode_records(hdr, h.records)
    e.sync()
    return hdr, d


def _record_values(d, w):
    """(V64, V32) of every record's V(s) and V(a) under a weight set."""
    mover = d["mover"].astype(np.uint8)
    xs, xa = orc.encode_many(d["before"], mover), orc.encode_many(d["after"], mover)
    np.testing.assert_array_equal(d["obs"].view(np.uint32), xs.view(np.uint32))
    return (orc.value(w, xs), vc.value_f32(w, xs)), (orc.value(w, xa), vc.value_f32(w, xa))


ENGINES = [dict(lanes=64, ply=1, fused=False), dict(lanes=64, ply=1, fused=True), dict(lanes=32, ply=2, k_top=4)]


@pytest.mark.parametrize("kw", ENGINES, ids=["phased-1ply", "fused-1ply", "phased-2ply-k4"])
def test_engine_weight_swap_across_exponents(kw):
    """set_weights(seed0, e = 13), 40 steps, set_weights(ckpt_x2^6, e = 5), 80
    steps: every record's V(s) matches the oracle under exactly one of the two
    nets (records where the two oracle values differ by less than 1e-4 are
    ambiguous and left out, at most 1 %), within an episode the matches run
    seed0 ... seed0 then scaled ... scaled with one switch, at least 1,000
    records match the scaled net, and V(a) (the afterstate's value, as
    test_gpu_engine._check_transitions checks it at either ply) matches under
    the same net: the new feature scale reaches the kernel arguments and the
    per-launch LUT of every engine."""
    from bgx import Engine
    sets = vc.weight_sets()
    names = ("seed0", "ckpt_x2^6")
    e = Engine(seed=17, max_steps=MAX_STEPS, **kw)
    e.set_weights(sets["seed0"], temperature=1.5, version=1)
    e.step(40)
    e.set_weights(sets["ckpt_x2^6"], temperature=1.5, version=2)
    e.step(80)
    hdr, d = _harvest(e)
    e.close()
    m = len(d["v_s"])
    assert m > 1000 and int(hdr[:, 3].sum()) == m
    ref = [_record_values(d, sets[n]) for n in names]
    tol = [vc.tolerance(n, r[0][1], r[0][0])[0] for n, r in zip(names, ref)]
    tol_a = [vc.tolerance(n, r[1][1], r[1][0])[0] for n, r in zip(names, ref)]
    err = [np.abs(d["v_s"].astype(np.float64) - r[0][0]) for r in ref]
    err_a = [np.abs(d["v_a"].astype(np.float64) - r[1][0]) for r in ref]
    clear = np.abs(ref[0][0][0] - ref[1][0][0]) >= 1e-4
    assert (~clear).sum() <= 0.01 * m, int((~clear).sum())
    match = [err[k] <= tol[k] for k in (0, 1)]
    print(f"RATIO engine {kw} | records {m} | seed0 {int(match[0].sum())} | scaled {int(match[1].sum())} | "
          f"worst err {float(np.minimum(err[0], err[1]).max()):.3g} | tol {tol}")
    assert np.isfinite(d["v_s"]).all() and np.isfinite(d["v_a"]).all()
    assert (match[0][clear] ^ match[1][clear]).all(), np.nonzero(clear & ~(match[0] ^ match[1]))[0][:10]
    assert int((match[1] & clear).sum()) >= 1000
    o = 0
    mixed = 0
    for row in hdr:
        n = int(row[3])
        k = np.arange(o, o + n)[clear[o:o + n]]
        which = match[1][k].astype(int)          # 0 = seed0, 1 = scaled
        assert (np.diff(which) >= 0).all(), (int(row[0]), int(row[1]), which)
        mixed += int(which.min(initial=1) == 0 and which.max(initial=0) == 1)
        # V(a) under the net of the record's V(s)
        for j, wn in zip(k, which):
            assert err_a[wn][j] <= tol_a[wn], (int(row[0]), int(row[1]), int(j), names[wn], err_a[wn][j])
        o += n
    assert mixed >= kw["lanes"] // 2, mixed     # the swap fell inside an episode on (nearly) every lane


def _bad_weights():
    sets = vc.weight_sets()
    out = []
    for t, idx in (("W1", (64, 100)), ("b1", (9,)), ("w2", (0,)), ("b2", (0,))):
        w = {k: a.copy() for k, a in sets["ckpt"].items()}
        w[t][idx] = np.nan
        out.append((t + " nan", t, w))
    for t, idx, v in (("W1", (127, 197), np.inf), ("b1", (127,), -np.inf), ("w2", (5,), np.inf), ("b2", (0,), -np.inf)):
        w = {k: a.copy() for k, a in sets["ckpt"].items()}
        w[t][idx] = v
        out.append((t + " inf", t, w))
    w = {k: a.copy() for k, a in sets["seed0"].items()}
    w["W1"][:] = 5e7
    out.append(("W1 = 5e7", "W1", w))
    out.append(("ckpt x 2^24", "W1", vc.scaled(sets["ckpt"], 24)))
    return out


def test_unrepresentable_weights_are_rejected(bgx_ops):
    """bgx_net_create: a NaN or an inf in any tensor, and W1 = 5e7
    (max|log2(e) w| >= 2^26: the e = -11 clamp would overflow fp16 and V would
    be NaN), are BGX_E_ARG with the tensor named; the largest accepted scale
    still evaluates."""
    from bgx import BgxError
    for what, t, w in _bad_weights():
        with pytest.raises(BgxError, match=r"\(-1\).*" + t) as ei:
            bgx_ops.Net(w)
        assert "bgx_net_create" in str(ei.value), what


@pytest.mark.parametrize("kw", ENGINES, ids=["phased-1ply", "fused-1ply", "phased-2ply-k4"])
def test_engine_keeps_its_network_after_a_rejected_upload(kw):
    """Engine.set_weights (and set_opponent on the phased engines) with
    unrepresentable weights raises BGX_E_ARG and leaves the previous network
    in force: the engine steps on, and every record before and after the
    rejected uploads carries V(s) / V(a) of the old weights."""
    from bgx import BgxError, Engine
    w = vc.weight_sets()["ckpt_x2^3"]
    e = Engine(seed=23, max_steps=MAX_STEPS, **kw)
    e.set_weights(w, temperature=1.5, version=1)
    e.step(MAX_STEPS)
    for what, t, bad in _bad_weights():
        with pytest.raises(BgxError, match=r"\(-1\).*" + t):
            e.set_weights(bad, temperature=1.5, version=2)
        if not e.fused:
            with pytest.raises(BgxError, match=r"\(-1\).*" + t):
                e.set_opponent(bad)
    e.step(MAX_STEPS)
    hdr, d = _harvest(e)
    e.close()
    assert len(hdr) >= 2 * kw["lanes"] - 2 and len(d["v_s"]) > 20 * kw["lanes"]
    (s64, s32), (a64, a32) = _record_values(d, w)
    _assert_rule("ckpt_x2^3", f"engine {kw} V(s)", d["v_s"], s64, s32)
    _assert_rule("ckpt_x2^3", f"engine {kw} V(a)", d["v_a"], a64, a32)
