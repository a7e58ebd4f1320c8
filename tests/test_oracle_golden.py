"""Pin the CPU oracle (oracle/bgref.c) against the reference's golden vectors.

The fixtures were produced by tools/gen_golden.py importing the reference in
the build container; see that script's header for what was imported.
"""
import hashlib

import numpy as np
import pytest

from conftest import golden
import oracle as orc


def test_movegen_cases_ordered_with_submoves():
    d = golden("movegen_cases.npz")
    for i in range(len(d["boards"])):
        o0, o1 = d["offsets"][i], d["offsets"][i + 1]
        n, res, nsub, sub = orc.movegen(d["boards"][i], d["player"][i], *d["dice"][i],
                                        with_sub=True)
        assert n == o1 - o0, i
        np.testing.assert_array_equal(res, d["results"][o0:o1], err_msg=str(i))
        np.testing.assert_array_equal(nsub, d["nsub"][o0:o1])
        np.testing.assert_array_equal(sub, d["subs"][o0:o1])


def test_movegen_opening_counts():
    # P1 at the start: 3-1 -> 16, 6-6 -> 11, 1-1 -> 42, 6-5 -> 7, 2-1 -> 15
    init = golden("movegen_cases.npz")["boards"][0]
    for dice, cnt in (((3, 1), 16), ((6, 6), 11), ((1, 1), 42), ((6, 5), 7), ((2, 1), 15)):
        assert orc.movegen(init, 0, *dice)[0] == cnt


def test_movegen_digests():
    g = golden("movegen_digests.npz")
    for i in range(len(g["boards"])):
        n, res, _ = orc.movegen(g["boards"][i], g["player"][i], *g["dice"][i])
        assert n == g["count"][i], i
        assert hashlib.sha256(res.tobytes()).digest() == g["sha256"][i].tobytes(), i


def test_movegen_heavy_digests():
    """The heaviest legal positions (tests/heavy_cases.py, lists up to 2,140
    plays), all 36 rolls: the reference's count and ordered boards, and for the
    three largest lists the plays' sub-move counts."""
    import heavy_cases as hc
    g = golden("movegen_heavy.npz")
    cs = hc.cases()
    assert len(g["boards"]) == 36 * len(cs) and g["count"].max() == 2140
    for i in range(len(g["boards"])):
        name, b, pl = cs[i // 36]
        assert g["name"][i] == name and g["player"][i] == pl and tuple(g["dice"][i]) == hc.ROLLS36[i % 36]
        np.testing.assert_array_equal(g["boards"][i], b)
        n, res, nsub = orc.movegen(b, pl, *g["dice"][i])
        assert n == g["count"][i], (name, i)
        assert hashlib.sha256(res.tobytes()).digest() == g["sha256"][i].tobytes(), (name, i)
        for k, j in enumerate(g["nsub_job"]):
            if j == i:
                np.testing.assert_array_equal(nsub, g["nsub"][g["nsub_offsets"][k]:g["nsub_offsets"][k + 1]])
    assert len(g["nsub_job"]) == 3 and (g["count"][g["nsub_job"]] >= 2140).all()


def test_encode_live_and_interleaved_bit_exact():
    e = golden("encode.npz")
    live = orc.encode_many(e["boards"], e["player"], 0)
    np.testing.assert_array_equal(live.view(np.uint32), e["live"].view(np.uint32))
    n = len(e["interleaved"])
    inter = orc.encode_many(e["boards"][:n], e["player"][:n], 1)
    np.testing.assert_array_equal(inter.view(np.uint32), e["interleaved"].view(np.uint32))


@pytest.mark.parametrize("which", ["seed0", "ckpt"])
def test_value_within_1e5(which, weights_seed0, weights_ckpt):
    v = golden("value.npz")
    w = weights_seed0 if which == "seed0" else weights_ckpt
    ref = v["v_seed0"] if which == "seed0" else v["v_ckpt"]
    got = orc.value(w, v["x"])
    assert np.max(np.abs(got - ref)) < 1e-5


def _outcome_cells(o):
    """Every named cell of the outcome rules occurs in outcomes.npz with the
    reference's label, read off the fixture's arrays alone (the boards are
    parsed by outcome_cases.features, in the mover's view: the mover runs
    towards point 23, home 18..23, "behind a run" = on a higher point)."""
    import outcome_cases as oc
    boards, player = o["boards"], o["player"]
    # each board twice: with the player who moved, then with the other one
    np.testing.assert_array_equal(boards[0::2], boards[1::2])
    assert (player[0::2] != player[1::2]).all()
    assert not o["prime"][1::2].any() and not o["closed_out"][1::2].any()
    assert not (o["game_over"][1::2] & (boards[1::2, 50:52].max(axis=1) < 15)).any()
    for pl in (0, 1):
        idx = [i for i in range(0, len(boards), 2) if player[i] == pl]
        F = {i: oc.features(boards[i], pl) for i in idx}

        def cell(cond, key, want, what):
            hit = [i for i in idx if cond(F[i])]
            assert hit, (pl, what)
            bad = [i for i in hit if bool(o[key][i]) != want]
            assert not bad, (pl, what, boards[bad[0]])
            return hit

        one = lambda f: f["n_theirs"] == 1 and f["bar_o"] == 0 and f["max_stack"] == 2  # noqa: E731
        for n in (5, 6, 7):
            run = lambda f: f["run_len"] == n and f["n_made"] == n  # noqa: E731
            assert {F[i]["run_start"] for i in idx if run(F[i])} == set(range(25 - n)), (pl, n)
            cell(lambda f: run(f) and one(f) and f["first_behind"], "prime", True, f"run {n}, first point behind")
            cell(lambda f: run(f) and one(f) and f["theirs"][23] and f["run_end"] < 22, "prime", True,
                 f"run {n}, farthest point behind")
            cell(lambda f: run(f) and one(f) and f["ahead"], "prime", False, f"run {n}, only ahead")
            cell(lambda f: run(f) and one(f) and f["theirs"][max(f["run_start"] - 1, 0)] and f["run_start"] > 0,
                 "prime", False, f"run {n}, first point ahead")
            cell(lambda f: run(f) and f["n_theirs"] == 0 and f["bar_o"] == 1, "prime", False, f"run {n}, only the bar")
            cell(lambda f: run(f) and f["n_theirs"] == 0 and f["off_o"] == 15, "prime", False, f"run {n}, all off")
            edge = cell(lambda f: run(f) and f["run_end"] == 23, "prime", False, f"run {n} against the edge")
            assert len(edge) >= 19 - n                       # every free point, the bar, all off
            for s in range(25 - n):                          # one checker on every free point in turn
                pts = {int(np.flatnonzero(F[i]["theirs"])[0]) for i in idx
                       if run(F[i]) and one(F[i]) and F[i]["run_start"] == s and F[i]["mine"].sum() == 2 * n}
                assert pts == set(range(24)) - set(range(s, s + n)), (pl, n, s)
            cell(lambda f: run(f) and f["max_stack"] == 3 and f["first_behind"], "prime", True, f"run {n}, spare on it")
            cell(lambda f: run(f) and one(f) and f["mine"].sum() == 2 * n + 1 and f["first_behind"], "prime", True,
                 f"run {n}, spare elsewhere")
        cell(lambda f: f["run_len"] == 5 and f["max_stack"] == 7 and f["first_behind"], "prime", True, "stack of 7")
        behind = lambda f: f["first_behind"] or f["far_behind"]  # noqa: E731
        cell(lambda f: f["run_len"] == 4 and f["n_made"] == 4 and f["first_behind"], "prime", False, "run of 4")
        cell(lambda f: f["run_len"] == 4 and f["n_made"] == 4 and f["far_behind"], "prime", False, "run of 4")
        single = cell(lambda f: f["n_made"] == 4 and (f["mine"] == 1).sum() == 1 and f["run_len"] < 5 and (
            lambda occ: any(occ[s:s + 5].all() for s in range(20)))(f["mine"] > 0) and behind(f), "prime", False,
            "run of 5 with a single checker")
        assert {F[i]["run_len"] for i in single} == {2, 3, 4}   # the single checker at the ends and inside
        cell(lambda f: f["n_made"] == 7 and f["run_len"] == 4 and behind(f), "prime", False, "4 + gap + 3")
        for k in range(8, 16):
            cell(lambda f: f["max_stack"] == k, "prime", False, f"stack of {k}")
        for base in (18, 17):
            for h in range(base, base + 6):
                for v in (0, 1, 2, 5):
                    for bar in (0, 1, 2, 15):
                        cell(lambda f: f["mine"][h] == v and f["bar_o"] == bar and f["mine"].sum() == 10 + v
                             and (np.delete(f["mine"][base:base + 6], h - base) == 2).all(),
                             "closed_out", base == 18 and v >= 2 and bar > 0, f"close-out {base} {h} {v} {bar}")
        for off in (0, 1, 14):
            for bar in (0, 1):
                for pt in [None] + list(range(24)):
                    if off + bar + (pt is not None) > 15:
                        continue
                    hit = cell(lambda f: f["off_m"] == 15 and f["off_o"] == off and f["bar_o"] == bar and f["n_theirs"] == (
                        pt is not None) and (pt is None or f["theirs"][pt] == 1), "game_over", True, f"over {off} {bar} {pt}")
                    for i in hit:
                        assert bool(o["gammon"][i]) == (off == 0)
                        assert bool(o["backgammon"][i]) == (off == 0 and (bar > 0 or (pt is not None and pt >= 18)))


def test_reward_predicates():
    names = {"game_over": "check_game_over", "gammon": "check_for_gammon",
             "backgammon": "check_for_backgammon", "prime": "made_at_least_five_prime",
             "closed_out": "is_closed_out"}
    for fixture in ("predicates.npz", "outcomes.npz"):
        p = golden(fixture)
        for key, fn in names.items():
            got = np.array([orc.predicate(fn, b, pl) for b, pl in zip(p["boards"], p["player"])])
            np.testing.assert_array_equal(got, p[key], err_msg=fixture + " " + key)
        assert p["prime"].any() and p["closed_out"].any() and p["backgammon"].any()
    # outcomes.npz: the enumerated boards of tests/outcome_cases.py, and every
    # named cell of the rules with the reference's label
    import outcome_cases as oc
    o = golden("outcomes.npz")
    boards, player, _ = oc.fixture_rows()
    np.testing.assert_array_equal(o["boards"], boards)
    np.testing.assert_array_equal(o["player"], player)
    _outcome_cells(o)


def test_env_greedy_trajectories():
    t = golden("env_traj.npz")
    for (d0, dn, s0, sn) in t["episodes"]:
        env = orc.OracleEnv(t["dice"][d0:d0 + dn])
        env.reset()
        for s in range(s0, s0 + sn):
            np.testing.assert_array_equal(env.board, t["board"][s])
            assert env.env.current_player == t["player"][s]
            assert env.env.num_moves == t["num_moves"][s]
            assert env.env.full_moves == t["full_moves"][s]
            assert tuple(env.env.roll) == tuple(t["roll"][s])
            r = env.step(t["action"][s] if t["kind"][s] == 0 else 0)
            assert r.kind == t["kind"][s]
            assert np.float32(r.reward) == t["reward"][s]
            assert bool(r.done) == bool(t["done"][s])
            assert r.win_type == t["win_type"][s]
            assert bool(r.close_out_reward) == bool(t["close_out"][s])
            assert bool(r.prime_reward) == bool(t["prime"][s])
            if t["kind"][s] == 0:
                np.testing.assert_array_equal(env.board, t["after"][s])
                if not t["done"][s]:
                    mover = int(t["player"][s])
                    assert orc.predicate("is_closed_out", env.board, mover) == bool(t["closed_pred"][s])
                    assert orc.predicate("made_at_least_five_prime", env.board, mover) == bool(t["prime_pred"][s])


def _env_events(t):
    """Event counts of env_traj.npz (tools/gen_golden.py episode_events)."""
    k, rew = t["kind"], t["reward"]
    prev_pass = np.concatenate([[False], k[:-1] == 1])
    first = np.zeros(len(k), bool)
    first[t["episodes"][:, 2]] = True
    return dict(close_out=int(t["close_out"].sum()), prime=int(t["prime"].sum()),
                close_repeat=int((t["closed_pred"] & ~t["close_out"]).sum()),
                prime_repeat=int((t["prime_pred"] & ~t["prime"]).sum()),
                backgammon=int((t["win_type"] == 3).sum()), gammon=int((t["win_type"] == 2).sum()),
                pass_run=int(((k == 1) & prev_pass & ~first).sum()),
                shaping_rewards=sorted(set(rew[(rew > 0) & (rew < 1)].tolist())))


def test_env_fixture_covers_shaping_and_terminal_events():
    """The reference-generated trajectories hold every reward path of
    backgammon_env.py:167-213: close-outs (+0.30) and primes (+0.20), either
    predicate holding again after the player's reward was given (no second
    reward: once per player per game), gammons, backgammons, consecutive
    passes; under both weight sets (the seed-0 net and the 2.1M checkpoint)."""
    t = golden("env_traj.npz")
    ev = _env_events(t)
    assert ev["close_out"] >= 10 and ev["prime"] >= 10, ev
    assert ev["close_repeat"] >= 1 and ev["prime_repeat"] >= 1, ev
    assert ev["backgammon"] >= 3 and ev["gammon"] >= 3 and ev["pass_run"] >= 1, ev
    # the rewards are torch fp32 (backgammon_env.py:165-213): 0.2f and 0.3f exactly
    assert ev["shaping_rewards"] == [float(np.float32(0.2)), float(np.float32(0.3))], ev
    assert set(np.unique(t["weight_set"]).tolist()) == {0, 1}
    # the once-per-player rule: at most one close-out and one prime reward per player per game
    for (d0, dn, s0, sn) in t["episodes"]:
        rows = slice(s0, s0 + sn)
        for pl in (0, 1):
            mine = t["player"][rows] == pl
            assert t["close_out"][rows][mine].sum() <= 1 and t["prime"][rows][mine].sum() <= 1


def test_close_out_and_prime_never_coincide():
    """A step cannot earn both shaping rewards (0.30 + 0.20): a close-out needs
    the mover's six home points made (12 checkers), and a counted 5-prime needs
    an opponent checker past the prime's end (env_helper.py:167-242), i.e. on
    one of those home points, or 10 more checkers for a prime outside home.
    Checked exhaustively over the predicate fixture's boards and 20,000 random
    closed-out boards on the oracle."""
    p = golden("predicates.npz")
    assert not np.any(p["closed_out"] & p["prime"])
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(20000):
        b = np.zeros(52, np.uint8)
        mover = int(rng.integers(2))
        home = np.arange(18, 24) if mover == 0 else np.arange(0, 6)
        b[24 * mover + home] = 2
        rest = 3
        while rest:
            i = int(rng.integers(24))
            if i in home or b[24 * (1 - mover) + i] == 0:
                k = int(rng.integers(1, rest + 1))
                b[24 * mover + i] += k
                rest -= k
        b[48 + (1 - mover)] = int(rng.integers(1, 4))
        left = 15 - b[48 + (1 - mover)]
        free = [i for i in range(24) if b[24 * mover + i] == 0]
        for i in rng.choice(free, size=min(len(free), 6), replace=False):
            k = int(min(left, rng.integers(1, 4)))
            b[24 * (1 - mover) + i] += k
            left -= k
        b[50 + (1 - mover)] = left
        if orc.predicate("is_closed_out", b, mover):
            n += 1
            assert not orc.predicate("made_at_least_five_prime", b, mover), b
    assert n == 20000


def test_two_ply_exact_mode(weights_seed0, weights_ckpt):
    t = golden("two_ply.npz")
    for i in range(len(t["boards"])):
        w0 = orc.two_ply_response(weights_seed0, t["boards"][i], t["opponent"][i])
        wc = orc.two_ply_response(weights_ckpt, t["boards"][i], t["opponent"][i])
        assert abs(w0 - t["w_seed0"][i]) < 1e-5
        assert abs(wc - t["w_ckpt"][i]) < 1e-5
