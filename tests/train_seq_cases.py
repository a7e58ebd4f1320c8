"""Shared inputs and helpers of the sequential TD(0) kernel's piecewise tests
(test_train_seq_ref.py on the CPU, test_gpu_train_seq.py on the GPU):
bgx_td0_update, csrc/bgx_train.hip. A plain module, not a conftest; nothing
here touches the GPU or libbgx.so until run_seq is called.

The ABI has no gradient output, but one call with n_eps = 1, lr = 0,
grad_clip = 0, zero moments and step = 0 leaves m = fl32(fl32(0.1) g) in the
first moment, so g' = m / fl32(0.1) (grad_from_m, in float64) is the kernel's
pre-clip gradient to one fp32 rounding, d_metrics[1] is its own fp32 norm
(the clip factor is 1) and the parameters stay as they were.
"""
import numpy as np

import train_batch_cases as tc

GAMMA, LR = 0.99, 1e-3
W1M = np.float32(1.0 - 0.9)   # the kernel's (float)(1.0 - 0.9), Adam's 1 - beta1

# One episode per call: one record (no bootstrap); two; one short of a chunk
# (TR_TC = 64), a full chunk, a bootstrap across the chunk edge; two full
# chunks, the reverse reload behind a one-record last chunk; a ragged third
# chunk; one short of TRAIN_TMAX and TRAIN_TMAX = 2,048, the longest accepted.
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200, 2047, 2048)
EDGE = "edge"                  # the hand-packed feature-edge episode
CASES = LENGTHS + (EDGE,)

# The clip cases at grad_clip = 1, picked from the float64 gradient norm
# (test_train_seq_ref.py recomputes it): above 1.05 the clip is active, below
# 0.95 it is not. seed0 at T = 64 (0.961) is inside that band and so is no clip
# case; its Adam step is checked like every other.
CLIP_ACTIVE = {"seed0": (1, 2, 63, 128, 129, 200, 2047, 2048, EDGE), "ckpt": (1, 2)}
CLIP_INACTIVE = {"seed0": (65,), "ckpt": (63, 64, 65, 128, 129, 200, 2047, 2048, EDGE)}

MULTI_LENS = (1, 65, 64, 3, 130)   # several episodes in one launch
MULTI_SEED = 600

EDGE_POINTS = (0, 7, 8, 15, 16, 23)   # first and last point of each packed word
_CACHE = {}


def edge_records():
    """uint32 [40, 12]: hand-packed records, not reachable positions. Records
    2 n and 2 n + 1 (n = 0..15; mover 0, then mover 1) put rotating counts on
    the first and last point of each packed word of both players and on bar
    and off of both, so that over the 32 of them every one of those 28 fields
    takes every value 0..15 under either mover; the other points hold small
    counts. 8 more records repeat fields at 15 next to fields at 0."""
    if "edge" in _CACHE:
        return _CACHE["edge"]
    from bgx.records import pack_record
    rng = np.random.default_rng(77)
    rows = []

    def pack(counts, bars, mover, k):
        w = np.zeros(7, np.uint32)
        for i in range(48):
            w[i // 8] |= np.uint32(int(counts[i]) << (4 * (i % 8)))
        w[6] = np.uint32(bars[0] | bars[1] << 4 | bars[2] << 8 | bars[3] << 12)   # bar1, bar2, off1, off2
        return pack_record(w, mover, 0.5, 0.5, 0.0, k, 1 + k, k, (1 + k % 6, 1 + (k // 6) % 6), 0, 0, 0, 0)

    for n in range(16):
        for mover in (0, 1):
            counts = rng.integers(0, 4, 48)
            for pl in (0, 1):
                for i, pt in enumerate(EDGE_POINTS):
                    counts[24 * pl + pt] = (n + 3 * i + 7 * pl + 5 * mover) % 16
            bars = ((n + 5 * mover) % 16, (n + 9 + 5 * mover) % 16, (n + 5 + 5 * mover) % 16, (15 - n + 5 * mover) % 16)
            rows.append(pack(counts, bars, mover, len(rows)))
    for k in range(8):
        counts = np.where(rng.integers(0, 2, 48) == 1, 15, 0)
        bars = tuple(15 if (k >> b) & 1 else 0 for b in range(4))
        rows.append(pack(counts, bars, k % 2, len(rows)))
    rec = np.stack(rows)
    rew = rng.choice(np.float32([0.0, 0.0, 0.2, 0.3]), len(rec))
    rew[-1] = np.float32(-2.0)
    rec[:, 9] = rew.astype(np.float32).view(np.uint32)
    rec[-1, 11] |= np.uint32(1 << 6)   # done
    rec.setflags(write=False)
    _CACHE["edge"] = rec
    return rec


def headers_for(lens):
    """Episode headers uint32 [E, 16] of contiguous episodes of these lengths."""
    lens = np.asarray(lens, np.int64)
    hdr = np.zeros((len(lens), 16), np.uint32)
    hdr[:, 0] = np.arange(len(lens))
    hdr[:, 2] = np.concatenate([[0], np.cumsum(lens)])[:-1]
    hdr[:, 3] = lens
    hdr[:, 4] = lens
    hdr[:, 5] = 1
    return hdr


def case_inputs(case):
    """(headers, records, offs) of one single-episode case, built once."""
    if ("in", case) not in _CACHE:
        if case == EDGE:
            rec = edge_records()
            out = (headers_for([len(rec)]), rec, np.array([0, len(rec)], np.int64))
        else:
            out = tc.synth([case], seed=500 + LENGTHS.index(case))
        _CACHE["in", case] = out
    return _CACHE["in", case]


def ref64(case, wname):
    """batched_td0_reference of a case (one episode: the sequential kernel's loss), computed once."""
    if ("r64", case, wname) not in _CACHE:
        from bgx.train_ref import batched_td0_reference
        _, rec, offs = case_inputs(case)
        _CACHE["r64", case, wname] = batched_td0_reference(tc.flat_params(tc.WEIGHTS[wname]), rec, offs, GAMMA)
    return _CACHE["r64", case, wname]


def grad_from_m(m):
    """g' (float64) from the first moment a zero-state step left: m = fl32(W1M g)."""
    return np.asarray(m, np.float32).astype(np.float64) / np.float64(W1M)


def run_seq(flat, m, v, step, rec, offs, lr=LR, clip=1.0, gamma=GAMMA):
    """One bgx_td0_update call from host arrays; everything it writes, as numpy."""
    import torch
    from bgx._lib import check, lib, ptr, stream_handle
    offs = np.asarray(offs, np.int64)
    rec = np.array(rec, dtype=np.uint32, order="C")   # a writable copy (torch.from_numpy)
    if offs[0] != 0 or offs[-1] != len(rec) or (np.diff(offs) < 1).any() or np.diff(offs).max() > 2048:
        raise ValueError("run_seq: offs must tile the records in episodes of 1 .. 2048")   # the kernel's reads
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)   # noqa: E731
    d_rec = torch.from_numpy(rec.view(np.int32)).to(dev)
    d_offs = t(offs, np.int32)
    d_p, d_m, d_v = t(flat, np.float32), t(m, np.float32), t(v, np.float32)
    if not d_p.numel() == d_m.numel() == d_v.numel() == tc.N_W1 + 257:
        raise ValueError("run_seq: 25,601 parameters and moments each")
    d_step = torch.tensor([int(step)], dtype=torch.int32, device=dev)
    d_met = torch.zeros(5, dtype=torch.float64, device=dev)
    check(lib().bgx_td0_update(ptr(d_rec), ptr(d_offs), len(offs) - 1, ptr(d_p), ptr(d_m), ptr(d_v), ptr(d_step),
                               lr, gamma, clip, ptr(d_met), stream_handle()), "bgx_td0_update")
    torch.cuda.synchronize()
    return {"p": d_p.cpu().numpy(), "m": d_m.cpu().numpy(), "v": d_v.cpu().numpy(), "step": int(d_step.item()),
            "metrics": d_met.cpu().numpy()}


def adam64(p, m, v, step, g, lr, clip):
    """clip_grad_norm_ and Adam in float64."""
    norm = np.sqrt((g * g).sum())
    if clip > 0:
        g = g * min(1.0, clip / (norm + 1e-6))
    step += 1
    m = m + (1.0 - 0.9) * (g - m)
    v = v * 0.999 + (1.0 - 0.999) * g * g
    den = np.sqrt(v) / np.sqrt(1.0 - 0.999 ** step) + 1e-8
    return p - (lr / (1.0 - 0.9 ** step)) * m / den, m, v, step


def chain64(flat, rec, offs, gamma=GAMMA, lr=LR, clip=1.0):
    """The sequential update in float64 from zero moments: per episode the
    gradient of its own loss (batched_td0_reference with one episode), the
    clip and an Adam step. Returns (params float64 [25601], step)."""
    from bgx.train_ref import batched_td0_reference
    p = np.asarray(flat, np.float64).copy()
    m, v, step = np.zeros_like(p), np.zeros_like(p), 0
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        g = batched_td0_reference(p, rec[a:b], [0, b - a], gamma)["grad"]
        p, m, v, step = adam64(p, m, v, step, g, lr, clip)
    return p, step
