"""Shared cases for the value-network tests: weight sets across the split-fp16
scaling exponent e (bgx_frag.h build_fragments) and boards at the edges of the
feature LUT (bgx_mlp.h lut_entry / feat_frag). Seeded numpy only; a plain
module (imported by test_value_cases.py, test_cpuwave.py and
test_gpu_value_range.py), not a conftest.

The tolerance rule of those tests lives here too (`tolerance`): a kernel's V
passes when max|V - V64| <= max(1e-5, 4 max|V32 - V64|), V64 the oracle's fp64
value and V32 a numpy fp32 forward of the same network (`value_f32`) -- the
precision the reference runs at. 1e-5 is the project's V tolerance; the factor
4 covers the kernels' summation order and the hardware exp2 / rcp against
numpy's.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOG2E = 1.4426950408889634
V_FLOOR = 1e-5          # the project's V tolerance (BASELINE.json north_star)
F32_FACTOR = 4.0
CLOSED_TOL = 1e-6       # weight sets whose V has a closed form
MAX_SCALED = 2.0 ** 26  # max|-log2(e) w| the split-fp16 scheme accepts (include/bgx.h)

_CACHE = {}


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k].astype(np.float32).copy() for k in ("W1", "b1", "w2", "b2")}


def scaled(w, k):
    out = {n: v.copy() for n, v in w.items()}
    out["W1"] = np.ldexp(out["W1"], k).astype(np.float32)
    out["b1"] = np.ldexp(out["b1"], k).astype(np.float32)
    return out


# the e build_fragments must pick for each set (recomputed by expected_e in
# test_value_cases.py; frag_check and the GPU tests rely on it)
INTENDED_E = {
    "seed0": 13, "ckpt": 11,
    "ckpt_x2^-12": 13, "ckpt_x2^-6": 13, "ckpt_x2^3": 8, "ckpt_x2^6": 5, "ckpt_x2^10": 1, "ckpt_x2^14": -3,
    "ckpt_x2^20": -9, "clamp_lo": -11, "zero_hidden": 0, "bias_dominates": 8, "one_big": 2, "dense_unit": 12,
    "saturated": 3, "tiny": 13, "w2_cancel": 11,
}
CKPT_K = (-12, -6, 3, 6, 10, 14, 20)
CLOSED_FORM = ("zero_hidden", "saturated")


def weight_sets():
    """{name: dict W1 [128, 198], b1 [128], w2 [128], b2 [1] (fp32)}; every set
    has sum|w2| <= 13 (seed0's), so the 1e-5 floor keeps its meaning. The two
    shipped sets come first."""
    if "w" in _CACHE:
        return _CACHE["w"]
    seed0, ckpt = _load("weights_seed0.npz"), _load("weights_ckpt2100000.npz")
    rng = np.random.default_rng(20240)
    sets = {"seed0": seed0, "ckpt": ckpt}
    for k in CKPT_K:
        sets[f"ckpt_x2^{k}"] = scaled(ckpt, k)
    # e = -11 unclamped is also the clamp's value: mx in [2^25, 2^26), every scaled weight below 2^15
    sets["clamp_lo"] = scaled(ckpt, 22)
    z = {n: v.copy() for n, v in seed0.items()}
    z["W1"][:] = 0.0
    z["b1"][:] = 0.0
    sets["zero_hidden"] = z                      # mx == 0: V = 0.5 sum(w2) + b2
    b = {n: v.copy() for n, v in seed0.items()}
    b["b1"][37] = 60.0
    sets["bias_dominates"] = b                   # the bias column sets e; the weights live mostly in lo
    o = {n: v.copy() for n, v in seed0.items()}
    o["W1"][91, 58] = 3000.0
    sets["one_big"] = o
    d = {n: v.copy() for n, v in seed0.items()}
    d["W1"] = rng.standard_normal((128, 198)).astype(np.float32)
    d["b1"] = rng.standard_normal(128).astype(np.float32)
    sets["dense_unit"] = d                       # pre-activations in the tens, many units half saturated
    s = {n: v.copy() for n, v in seed0.items()}
    sign = np.where(rng.integers(0, 2, 128) == 1, 1.0, -1.0).astype(np.float32)
    s["W1"] = np.repeat(sign[:, None] * np.float32(2000.0), 198, axis=1).astype(np.float32)
    s["b1"][:] = 0.0
    sets["saturated"] = s                        # sigmoids exactly 0 / 1: V = sum(w2[sign > 0]) + b2
    t = {n: v.copy() for n, v in seed0.items()}
    t["W1"] = (np.where(rng.integers(0, 2, (128, 198)) == 1, 1.0, -1.0) * 1e-30).astype(np.float32)
    t["b1"] = (np.where(rng.integers(0, 2, 128) == 1, 1.0, -1.0) * 1e-30).astype(np.float32)
    t["W1"][3, 5:9] = np.array([1e-40, -3e-42, 1.4e-45, -1e-39], np.float32)   # fp32 subnormals
    t["W1"][4, 0:3] = np.float32(-0.0)
    t["b1"][7] = np.float32(-0.0)
    t["b1"][8] = np.float32(2e-41)
    sets["tiny"] = t
    c = {n: v.copy() for n, v in ckpt.items()}
    c["w2"] = (np.float32(0.1) * np.where(np.arange(128) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    c["b2"] = np.array([5.0], np.float32)
    sets["w2_cancel"] = c
    for w in sets.values():
        assert float(np.abs(w["w2"].astype(np.float64)).sum()) <= 13.0
    _CACHE["w"] = sets
    return sets


def scaled_max(w):
    """max|-log2(e) w| over W1 (columns 193 / 195 divided by 15: their feature
    is the integer borne-off count) and b1, as build_fragments takes it."""
    W = w["W1"].astype(np.float64).copy()
    W[:, 193] /= 15.0
    W[:, 195] /= 15.0
    return max(float(np.abs(-LOG2E * W).max()), float(np.abs(-LOG2E * w["b1"].astype(np.float64)).max()))


def expected_e(w):
    mx = scaled_max(w)
    if mx == 0.0:
        return 0
    return int(min(13, max(-11, 14 - int(np.floor(np.log2(mx))))))


def closed_form(name, w):
    """The exact V of the sets whose hidden units do not depend on the board."""
    w2, b2 = w["w2"].astype(np.float64), float(w["b2"][0])
    if name == "zero_hidden":
        return 0.5 * w2.sum() + b2
    if name == "saturated":   # every board has a feature >= 1 (the side to move), so |h| >= 2000
        return w2[w["W1"][:, 0] > 0].sum() + b2
    raise KeyError(name)


def value_f32(w, x):
    """A plain fp32 forward (numpy): the precision of the reference's network."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 198)
    with np.errstate(over="ignore"):
        h = (x @ w["W1"].astype(np.float32).T + w["b1"].astype(np.float32)).astype(np.float32)
        s = (np.float32(1.0) / (np.float32(1.0) + np.exp(-h, dtype=np.float32))).astype(np.float32)
        return (s @ w["w2"].astype(np.float32) + w["b2"].astype(np.float32)[0]).astype(np.float32)


def tolerance(name, v32, v64):
    """(bound, fp32's own error) for a weight set on the rows v32 / v64 cover."""
    e32 = float(np.abs(np.asarray(v32, np.float64) - np.asarray(v64, np.float64)).max()) if len(v64) else 0.0
    if name in CLOSED_FORM:
        return CLOSED_TOL, e32
    return max(V_FLOOR, F32_FACTOR * e32), e32


def features_numpy(boards, player):
    """get_board_features (immutable_board.py:86-128) stated directly."""
    b = np.asarray(boards, np.uint8).reshape(-1, 52)
    p = np.broadcast_to(np.asarray(player), (len(b),))
    n = b[:, :48].astype(np.float32)
    f = np.zeros((len(b), 198), np.float32)
    pts = f[:, :192].reshape(len(b), 48, 4)
    pts[:, :, 0] = n >= 1
    pts[:, :, 1] = n >= 2
    pts[:, :, 2] = n >= 3
    pts[:, :, 3] = np.maximum(n - 3.0, 0.0) / 2.0
    f[:, 192] = b[:, 48] / 2.0
    f[:, 193] = (b[:, 50] / 15.0).astype(np.float32)
    f[:, 194] = b[:, 49] / 2.0
    f[:, 195] = (b[:, 51] / 15.0).astype(np.float32)
    f[:, 196] = p == 0
    f[:, 197] = p == 1
    return f


def _place_other(b, side, rng):
    """15 checkers of `side` on points the other side does not hold; now and
    then a few on the bar or borne off."""
    free = [i for i in range(24) if b[24 * (1 - side) + i] == 0]
    pts = rng.choice(free, size=int(rng.integers(1, min(6, len(free)) + 1)), replace=False)
    left = 15
    if rng.integers(0, 4) == 0:
        k = int(rng.integers(0, 8))
        b[48 + side] = k
        left -= k
    if rng.integers(0, 4) == 0:
        k = int(rng.integers(0, left + 1))
        b[50 + side] = k
        left -= k
    cnt = rng.multinomial(left, np.ones(len(pts)) / len(pts))
    for i, c in zip(pts, cnt):
        b[24 * side + int(i)] += c


def edge_boards():
    """(boards uint8 [n, 52], player uint8 [n]): every LUT byte reachable on a
    legal board, in every packed byte. For each side and each of its 12 pairs
    of adjacent point slots that share a packed byte, every count pair (a, b)
    with a + b <= 15, the rest of the 15 on the bar (even cases) or borne off
    (odd cases); bar = 0..15 and off = 0..15 for each side; all 15 on each point
    of each side. The other side sits on points that do not collide. Every
    board appears with both values of player."""
    if "b" in _CACHE:
        return _CACHE["b"]
    rng = np.random.default_rng(1507)
    out = []
    case = 0
    for side in (0, 1):
        for j in range(12):
            for a in range(16):
                for c in range(16 - a):
                    b = np.zeros(52, np.uint8)
                    b[24 * side + 2 * j], b[24 * side + 2 * j + 1] = a, c
                    b[(48 if case % 2 == 0 else 50) + side] = 15 - a - c
                    _place_other(b, 1 - side, rng)
                    out.append(b)
                    case += 1
    for side in (0, 1):
        for field in (48, 50):
            for k in range(16):
                b = np.zeros(52, np.uint8)
                b[field + side] = k
                pts = rng.choice(24, size=3, replace=False)
                for i, c in zip(pts, rng.multinomial(15 - k, np.ones(3) / 3)):
                    b[24 * side + int(i)] = c
                _place_other(b, 1 - side, rng)
                out.append(b)
        for i in range(24):
            b = np.zeros(52, np.uint8)
            b[24 * side + i] = 15
            _place_other(b, 1 - side, rng)
            out.append(b)
    boards = np.stack(out)
    boards = np.concatenate([boards, boards])
    player = np.concatenate([np.zeros(len(out), np.uint8), np.ones(len(out), np.uint8)])
    boards.setflags(write=False)
    player.setflags(write=False)
    _CACHE["b"] = (boards, player)
    return _CACHE["b"]


def edge_sample(n):
    """n rows of edge_boards() at an even stride (both players, both sides)."""
    boards, player = edge_boards()
    idx = (np.arange(n) * (len(boards) - 1)) // max(n - 1, 1)
    return boards[idx].copy(), player[idx].copy()


def write_weights(w, path):
    """The w.bin the host tools of tests/cpuwave/ read: W1, b1, w2, b2 (fp32)."""
    np.concatenate([np.asarray(w[k], np.float32).ravel() for k in ("W1", "b1", "w2", "b2")]).tofile(path)
