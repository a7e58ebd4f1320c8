"""GPU move generation at the heaviest legal positions (tests/heavy_cases.py),
tier by tier, bit for bit and in order against the CPU oracle and the
reference's digests (tests/golden/movegen_heavy.npz).

Where a job ends (bgx_movegen.h, bgx_movegen.hip):
  * table-free doubles (doubles_by_path: >= 5 mover checkers outside home)
    stay in tier 1 while their level-1..3 lists fit 480 entries (the depth-4
    leaves are streamed), whatever the final count; the block kernel
    (coop_doubles_path) then takes levels of up to K_F = 2,048 entries, and a
    longer list runs on a global workspace slice (run_global, tier 3);
  * through the hash table (other roots, or BGX_MG_TEST_TABLE=1) tier 1 ends at
    224-entry frontiers and tier 2 at 2,016.
So of the spread board's doubles 1-1 (levels 15 / 112 / 561 / 2,140) takes the
tier-1 -> tier-2 -> tier-3 path, 2-2 (15 / 111 / 546 / 2,027) ends in tier 2, and
3-3 (1,225 plays, level 3 = 389) never leaves tier 1; `_levels` recomputes
these figures.
"""
import hashlib
import time

import numpy as np
import pytest
import torch

from conftest import golden
import heavy_cases as hc
import oracle as orc

pytestmark = pytest.mark.gpu

V_TOL = 1e-5
CANARY = 0xA5
GUARD_ROWS = 4096   # canary rows past the output: above any list (hc.RECORD_CLAMP), so even an
                    # emission without its capacity test would stay inside the allocation


@pytest.fixture(scope="module")
def heavy():
    """Every member x 36 rolls with the oracle's ordered lists, computed once."""
    jobs = []
    for name, b, pl in hc.cases():
        for a, c in hc.ROLLS36:
            n, res, _ = orc.movegen(b, pl, a, c)
            jobs.append({"name": name, "board": b, "player": pl, "dice": (a, c), "n": n, "res": res})
    g = golden("movegen_heavy.npz")
    assert len(jobs) == len(g["count"])
    for j, job in enumerate(jobs):
        job["sha256"] = g["sha256"][j].tobytes()
        assert job["n"] == g["count"][j]
    return jobs


def _levels(board, d):
    """Distinct boards after 1..4 moves of d pips for player 0 with nothing on
    the bar and the opponent on point 23 only (a checker on i moves iff
    i + d <= 22): the sizes of the path expansion's level lists."""
    cur, out = {tuple(int(x) for x in board[:24])}, []
    for _ in range(4):
        nxt = set()
        for s in cur:
            for i in range(23 - d):
                if s[i]:
                    t = list(s)
                    t[i] -= 1
                    t[i + d] += 1
                    nxt.add(tuple(t))
        out.append(len(nxt))
        cur = nxt
    return out


def _movegen(boards, player, dice, cap):
    from bgx import ops
    out, cnt = ops.movegen(torch.from_numpy(np.ascontiguousarray(boards)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(player)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(dice)).cuda(), cap=cap)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.fixture(scope="module")
def mixed(heavy):
    """One batch for all three tiers: 2,000 light jobs of movegen_cases.npz with
    the 396 heavy jobs spread through them, 300 more copies of the heaviest job
    (more than the 256 workspace slices) spread as well, and two further copies
    of it next to each other. Returns (boards, player, dice, expected lists,
    digest or None)."""
    d = golden("movegen_cases.npz")
    light = [(d["boards"][i], int(d["player"][i]), tuple(d["dice"][i]),
              d["results"][d["offsets"][i]:d["offsets"][i + 1]], None) for i in range(2000)]
    hv = [(j["board"], j["player"], j["dice"], j["res"], j["sha256"]) for j in heavy]
    top = max(hv, key=lambda t: len(t[3]))
    assert len(top[3]) == 2140 and _levels(top[0], top[2][0]) == [15, 112, 561, 2140]
    extra = hv + [top] * 300
    order = np.random.default_rng(7).permutation(len(extra))
    at = np.linspace(0, len(light), len(extra), endpoint=False).astype(int)
    batch, k = [], 0
    for i, job in enumerate(light):
        while k < len(extra) and at[k] <= i:
            batch.append(extra[order[k]])
            k += 1
        if i == 1000:
            batch += [top, top]
        batch.append(job)
    batch += [extra[order[q]] for q in range(k, len(extra))]
    assert len(batch) == 2000 + 396 + 302
    return (np.stack([t[0] for t in batch]), np.array([t[1] for t in batch], np.uint8),
            np.array([t[2] for t in batch], np.uint8), [t[3] for t in batch], [t[4] for t in batch])


@pytest.mark.parametrize("few,table,tier", [("0", "0", ""), ("1", "0", ""), ("0", "1", ""), ("1", "1", ""),
                                            ("0", "0", "3")])
def test_all_three_tiers_in_one_launch(mixed, few, table, tier, monkeypatch):
    """Tiers 1, 2 and 3 in one launch, sharing the overflow list and the
    workspace slices: both tier-1 kernels (BGX_MG_FEW), the table-free rules and
    the hash table for every job (BGX_MG_TEST_TABLE: there the 2,038-play list
    outgrows tier 2's 2,016-entry frontier), and every job through tier 3
    (BGX_MG_TEST_TIER=3). cap = the largest count rounded up to 256."""
    monkeypatch.setenv("BGX_MG_FEW", few)
    monkeypatch.setenv("BGX_MG_TEST_TABLE", table)
    if tier:
        monkeypatch.setenv("BGX_MG_TEST_TIER", tier)
    boards, player, dice, want, sha = mixed
    cap = (max(len(w) for w in want) + 255) // 256 * 256
    assert cap == 2304
    out, cnt = _movegen(boards, player, dice, cap)
    for i, w in enumerate(want):
        assert cnt[i] == len(w), (i, dice[i], cnt[i], len(w))
        np.testing.assert_array_equal(out[i, :len(w)], w, err_msg=f"job {i} dice {dice[i]}")
        if sha[i] is not None:
            assert hashlib.sha256(out[i, :len(w)].tobytes()).digest() == sha[i], i


def _movegen_canary(boards, player, dice, cap):
    """bgx_movegen into buffers with canary rows past out[n - 1, cap - 1] and
    canary counts past count[n - 1]; returns (rows [n, cap, 52], count [n])."""
    from bgx._lib import check, lib, ptr, stream_handle
    n = len(boards)
    db, dp, dd = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (boards, player, dice))
    out = torch.full((n * cap + GUARD_ROWS, 52), CANARY, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
    check(lib().bgx_movegen(ptr(db), ptr(dp), ptr(dd), n, ptr(out), ptr(cnt), cap, stream_handle(None)),
          "bgx_movegen")
    torch.cuda.synchronize()
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    assert (cnt[n:] == -7).all(), "a write past count[n - 1]"
    return out, cnt[:n]


@pytest.mark.parametrize("cap", [64, 1])
def test_truncated_output_keeps_inside_its_rows(heavy, cap):
    """cap far below the lists: count is the full count, the first
    min(count, cap) rows are exact and no row past out[n - 1, cap - 1] is
    touched."""
    boards = np.stack([j["board"] for j in heavy])
    player = np.array([j["player"] for j in heavy], np.uint8)
    dice = np.array([j["dice"] for j in heavy], np.uint8)
    out, cnt = _movegen_canary(boards, player, dice, cap)
    n = len(heavy)
    assert (out[n * cap:] == CANARY).all(), "a write past out[n - 1, cap - 1]"
    rows = out[:n * cap].reshape(n, cap, 52)
    for i, j in enumerate(heavy):
        k = min(j["n"], cap)
        assert cnt[i] == j["n"], (i, j["name"], j["dice"], cnt[i], j["n"])
        np.testing.assert_array_equal(rows[i, :k], j["res"][:k], err_msg=f"{j['name']} {j['dice']}")


def test_more_overflowing_jobs_than_the_overflow_list_holds(heavy):
    """65,536 + 64 copies of a job that leaves tier 1 and ends in tier 2, at
    cap = 1, then 64 light jobs: every count and first row equals the oracle's.
    The job is the spread board's 2-2: its three-move list (546 entries) outgrows
    tier 1's 480 and its 2,027 plays fit the block kernel's 2,048 (a final count
    just above 480 would not do: such a list can stay in tier 1, see the module
    docstring). The overflow list holds 65,536 jobs; push_ovf drops the rest,
    whose counts nothing would write, so bgx_movegen runs the call as launches
    of at most 65,536 jobs."""
    job = next(j for j in heavy if j["name"] == "spread_p0" and j["dice"] == (2, 2))
    lv = _levels(job["board"], 2)
    assert lv == [15, 111, 546, 2027] and lv[2] > hc.T1_LIST and max(lv) <= hc.T2_PARENTS and job["n"] == lv[3]
    d = golden("movegen_cases.npz")
    n_big, n_light = (1 << 16) + 64, 64
    boards = np.concatenate([np.repeat(job["board"][None], n_big, 0), d["boards"][:n_light]])
    player = np.concatenate([np.full(n_big, job["player"], np.uint8), d["player"][:n_light]])
    dice = np.concatenate([np.repeat(np.array([job["dice"]], np.uint8), n_big, 0), d["dice"][:n_light]])
    _movegen_canary(boards[:64], player[:64], dice[:64], 1)   # first-call setup kept out of the timing
    t0 = time.perf_counter()
    out, cnt = _movegen_canary(boards, player, dice, 1)
    print(f"{n_big} tier-2 jobs + {n_light} light: {time.perf_counter() - t0:.3f} s (with the copies to the host)")
    n = n_big + n_light
    assert (out[n:] == CANARY).all(), "a write past out[n - 1, 0]"
    bad = np.flatnonzero(cnt[:n_big] != job["n"])
    assert bad.size == 0, (bad.size, bad[:8], cnt[bad[:8]])
    assert (out[:n_big] == job["res"][0]).all()
    for i in range(n_light):
        o0, o1 = d["offsets"][i], d["offsets"][i + 1]
        assert cnt[n_big + i] == o1 - o0, i
        if o1 > o0:
            np.testing.assert_array_equal(out[n_big + i], d["results"][o0])


def _roots():
    cs = hc.cases()
    return np.stack([c[1] for c in cs]), np.array([c[2] for c in cs], np.uint8)


@pytest.mark.parametrize("bm,dbl,tail", [("0", "1", "4"), ("1", "0", "4"), ("1", "1", "0"), ("1", "1", "32")])
def test_reply_expansion_on_heavy_roots(heavy, bm, dbl, tail, monkeypatch):
    """bgx_reply_moves with the heavy positions as roots and their mover as the
    opponent who replies: the per-roll kernel (BGX_REPLY_BM=0), per-roll doubles
    items (BGX_REPLY_DBL=0) and the board-major doubles item with no and half
    the rows in per-roll items (BGX_REPLY_DBL_TAIL 0 / 32)."""
    from bgx import ops
    monkeypatch.setenv("BGX_REPLY_BM", bm)
    monkeypatch.setenv("BGX_REPLY_DBL", dbl)
    monkeypatch.setenv("BGX_REPLY_DBL_TAIL", tail)
    monkeypatch.setenv("BGX_MG_FEW", "0")
    boards, opp = _roots()
    by = {(j["name"], j["dice"]): j for j in heavy}
    names = [c[0] for c in hc.cases()]
    total = sum(by[(nm, r)]["n"] for nm in names for r in hc.ROLLS21)
    # the records; as ops.reply_moves reserves, two 2,048-row chunks for each of the launch's
    # ceil(7 x 11 / 16) = 5 workgroups; and for the per-roll kernel two partly used 256-row
    # chunks per job (its waves reserve rows on their own)
    rows, off, cnt = ops.reply_moves(torch.from_numpy(boards).cuda(), torch.from_numpy(opp).cuda(),
                                     cap=total + 5 * 2 * 2048 + len(names) * 21 * 2 * 256 + 4096)
    torch.cuda.synchronize()
    u8, off, cnt = ops.unpack(rows).cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()
    for i, nm in enumerate(names):
        for r, roll in enumerate(hc.ROLLS21):
            j, w = i * 21 + r, by[(nm, roll)]
            assert cnt[j] == w["n"], (nm, roll, cnt[j], w["n"])
            np.testing.assert_array_equal(u8[off[j]:off[j] + w["n"]], w["res"], err_msg=f"{nm} {roll}")


@pytest.mark.parametrize("which", ["seed0", "ckpt"])
def test_two_ply_on_heavy_roots(which, weights_seed0, weights_ckpt):
    """Net.two_ply on the heavy roots (up to 10,839 replies a root, inside the
    21 x 768 rows it allocates per root) against the oracle's
    compute_weighted_opponent_response, within the bound of
    test_two_ply_exact_mode_vs_reference."""
    from bgx import ops
    w = weights_seed0 if which == "seed0" else weights_ckpt
    boards, opp = _roots()
    got = ops.Net(w).two_ply(torch.from_numpy(boards).cuda(), torch.from_numpy(opp).cuda()).cpu().numpy()
    want = np.array([orc.two_ply_response(w, b, int(o)) for b, o in zip(boards, opp)])
    np.testing.assert_allclose(got, want, atol=V_TOL, rtol=0)


# (member, first roll) of the engine's start table; the first five have the
# opponent's fifteen checkers on one point, so every candidate has few replies
START = [("spread_p0", (1, 1)), ("spread_p1", (1, 1)), ("edge_t2", (1, 1)), ("spread_p0", (3, 3)),
         ("spread_p0", (2, 1)), ("blots_over_t2", (1, 1)), ("blocked_t2", (1, 1)), ("tier2_mid", (2, 2)),
         ("hits_t2", (1, 1)), ("tier2_low", (2, 2)), ("nd_max", (2, 1)), ("bar", (1, 1)), ("bearoff", (1, 1))]


@pytest.mark.parametrize("ply,k_top,greedy,n_start,steps", [(1, 4, False, 13, 4), (1, 4, True, 13, 4),
                                                            (2, 4, False, 13, 3), (2, 0, False, 5, 2)])
def test_phased_engine_from_heavy_starts(heavy, weights_ckpt, ply, k_top, greedy, n_start, steps):
    """Engine(fused=False, lanes=64) started on the heavy positions with fixed
    first rolls: every record against the oracle (_check_transitions: n_moves =
    min(count, 4095), action < min(count, 500)), greedy actions the argmax over
    the first 500 candidates only, and the heavy first steps really ran: one
    above 2,048 plays and one in (500, 2,016]. K = all runs the five starts
    whose candidates have few replies, so that the reply rows stay small."""
    from bgx import Engine
    from test_gpu_engine import _check_transitions, _collect
    by = {(j["name"], j["dice"]): j for j in heavy}
    table = [by[s] for s in START[:n_start]]
    lanes = 64
    first_total = sum(table[g % n_start]["n"] for g in range(lanes))
    # the first step's candidates of all lanes, plus a 256-row chunk a wave may leave unused per job
    cand_per_lane = (first_total + 256 * lanes) // lanes + 1
    # max_steps = steps: every lane's game is cut there, so its records are harvested
    e = Engine(fused=False, lanes=lanes, seed=5, ply=ply, k_top=k_top, greedy=greedy, cand_per_lane=cand_per_lane,
               reply_per_lane=262144 if k_top == 0 else 0, max_steps=steps)
    e.set_weights(weights_ckpt, temperature=1.5, version=1)
    e.set_start(np.stack([t["board"] for t in table]), [t["player"] for t in table],
                dice=np.array([t["dice"] for t in table], np.uint8))
    hdrs, recs = _collect(e, steps, chunk=steps)
    e.close()
    assert _check_transitions(weights_ckpt, hdrs, recs, ply, max_steps=steps) >= lanes
    firsts = []
    for d in recs:
        for k in range(len(d["action"])):
            b, mover, dice = d["before"][k], int(d["mover"][k]), d["dice"][k]
            cnt, res, _ = orc.movegen(b, mover, int(dice[0]), int(dice[1]))
            if d["step"][k] == 0:
                firsts.append(cnt)
            if greedy:
                m = min(cnt, 500)
                v = orc.value(weights_ckpt, orc.encode_many(res[:m], [mover] * m))
                a = int(d["action"][k])
                assert v[a] >= v.max() - V_TOL, (k, a, v[a], v.max())
    assert any(c > hc.T2_PARENTS for c in firsts), firsts
    assert any(500 < c <= hc.T2_FRONTIER for c in firsts), firsts
