"""Numpy restatements of the batched TD(0) update (bgx_td0_update_batched,
csrc/bgx_train_batch.hip; DeviceTrainer batched=True), the checkers its tests
use. No torch, no GPU, no libbgx.so.

    loss = (1/E) sum_e (1/T_e) sum_s (Y_s - tgt_s)^2,
    tgt_s = r_s + gamma Y_{s+1} (detached; r_s alone on an episode's last record)

and of its TD(lambda) form (bgx_tdlambda_update_batched), whose target is the
lambda-return of lambda_returns, with the zero-sum targets of
bgx_td_update_batched (BGX_TDF_ZERO_SUM) as lambda_returns(movers=) /
batched_td0_reference(zero_sum=True), and of bgx_td_afterstate_update_batched
(the same update on afterstate rows) as batched_td0_reference(afterstates=True,
headers=). batched_td0_reference states the forward pass and the gradient in float64;
adam_reference states clip_grad_norm_ and the Adam step in float32, in the
kernel's operation order, which is torch's (sqrt(v) / sqrt(bc2) + eps, then
p + (-step_size m) / den, every operation correctly rounded).
"""
from __future__ import annotations

import numpy as np

N_W1 = 128 * 198
N_PARAMS = N_W1 + 128 + 128 + 1   # fc1.weight | fc1.bias | value_head.weight | value_head.bias


def encode_records(records) -> np.ndarray:
    """The live 198-feature encoding (float32 [m, 198]) of each record's packed
    before-board, words 0..6 with indicator = the mover (bgx/records.py)."""
    r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
    m = r.shape[0]
    sh = (np.arange(8, dtype=np.uint32) * 4)[None, None, :]
    n = ((r[:, :6, None] >> sh) & 15).reshape(m, 48).astype(np.float32)   # P1 points 0..23, P2 points 0..23
    f = np.zeros((m, 198), np.float32)
    pts = f[:, :192].reshape(m, 48, 4)
    pts[:, :, 0] = n >= 1
    pts[:, :, 1] = n >= 2
    pts[:, :, 2] = n >= 3
    pts[:, :, 3] = np.maximum(n - 3.0, 0.0) * 0.5
    s6 = r[:, 6]
    f[:, 192] = (s6 & 15).astype(np.float32) * 0.5                          # bar1
    f[:, 193] = (((s6 >> 8) & 15).astype(np.float64) / 15.0).astype(np.float32)    # off1
    f[:, 194] = ((s6 >> 4) & 15).astype(np.float32) * 0.5                   # bar2
    f[:, 195] = (((s6 >> 12) & 15).astype(np.float64) / 15.0).astype(np.float32)   # off2
    ind = (s6 >> 16) & 1
    f[:, 196] = ind == 0
    f[:, 197] = ind == 1
    return f


def encode_afterstates(headers, records) -> np.ndarray:
    """The same encoding (float32 [m, 198]) of each record's afterstate row: the
    board after its move under its own mover's indicator
    (bgx.records.packed_afterstates; bgx_td_afterstate_update_batched)."""
    from .records import packed_afterstates
    r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12).copy()
    r[:, :7] = packed_afterstates(headers, r)[:, :7]
    return encode_records(r)


def split_params(params):
    p = np.asarray(params).reshape(-1)
    if p.shape[0] != N_PARAMS:
        raise ValueError(f"expected {N_PARAMS} parameters, got {p.shape[0]}")
    return p[:N_W1].reshape(128, 198), p[N_W1:N_W1 + 128], p[N_W1 + 128:N_W1 + 256], p[N_W1 + 256]


def record_movers(records) -> np.ndarray:
    """int64 [m]: the mover of each record (word 11 bit 9, bgx/records.py)."""
    r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
    return ((r[:, 11] >> 9) & 1).astype(np.int64)


def lambda_returns(Y, rewards, offs, gamma, lam, movers=None):
    """The lambda-return of every record, the serial recurrence from each
    episode's end in the dtype of Y (float64: the checker; float32: the fp32
    comparison, every operation rounded to float32):
        G_{b-1} = r_{b-1},  G_s = r_s + gamma ((1 - lam) Y_{s+1} + lam G_{s+1}).
    A record in no episode keeps 0. lam = 0 is the TD(0) target, lam = 1 the
    discounted Monte-Carlo return (Y then enters with weight 0).
    movers ([m], the mover of each record): the zero-sum target
    (bgx_td_update_batched, BGX_TDF_ZERO_SUM). Where the mover changes from
    record s to s + 1 both Y_{s+1} and G_{s+1} enter from the opponent's side,
    as 1 - x:
        G_s = r_s + gamma ((1 - lam) (1 - Y_{s+1}) + lam (1 - G_{s+1})).
    None, or one mover everywhere: the plain return, bit for bit."""
    Y = np.asarray(Y)
    dt = Y.dtype.type
    r = np.asarray(rewards).astype(dt)
    g, lam = dt(gamma), dt(lam)
    one_m, one = dt(1.0) - lam, dt(1.0)
    G = np.zeros(len(Y), dt)
    offs = np.asarray(offs, np.int64)
    mv = None if movers is None else np.asarray(movers).astype(np.int64)
    if mv is not None and len(mv) != len(Y):
        raise ValueError(f"movers: expected {len(Y)} values, got {len(mv)}")
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        if b <= a:
            continue
        G[b - 1] = r[b - 1]
        for s in range(b - 2, a - 1, -1):
            if mv is not None and mv[s] != mv[s + 1]:
                G[s] = r[s] + g * (one_m * (one - Y[s + 1]) + lam * (one - G[s + 1]))
            else:
                G[s] = r[s] + g * (one_m * Y[s + 1] + lam * G[s + 1])
    return G


def batched_td0_reference(params, records, offs, gamma, lam=0.0, zero_sum=False, afterstates=False, headers=None):
    """float64 forward and gradient of the batched loss. params: 25,601 values in
    state_dict order; records [m, 12]; offs [E + 1] (episode e = records
    [offs[e], offs[e + 1]), each at least 1 long). lam != 0: the target is the
    lambda-return (lambda_returns on the detached Y). zero_sum: the zero-sum
    target at every lam (lambda_returns with the movers of word 11). afterstates:
    V is taken on each record's afterstate row (encode_afterstates; headers
    [E, 16] is then required), the targets' recurrence is unchanged. Returns dict(grad float64
    [25601], loss, Y float64 [m], target, td_error, predicted_value, reward: the
    last three summed over episodes as the kernel's metrics are)."""
    W1, b1, w2, b2 = (np.asarray(x, np.float64) for x in split_params(params))
    r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
    offs = np.asarray(offs, np.int64)
    E = len(offs) - 1
    lens = np.diff(offs)
    if E < 1 or offs[0] != 0 or offs[-1] != r.shape[0] or (lens < 1).any():
        raise ValueError("offs: episodes must tile the records, each at least 1 long")
    if afterstates and headers is None:
        raise ValueError("afterstates=True needs the episode headers (the final boards)")
    X = (encode_afterstates(headers, r) if afterstates else encode_records(r)).astype(np.float64)
    rew = r[:, 9].copy().view(np.float32).astype(np.float64)
    S = 1.0 / (1.0 + np.exp(-(X @ W1.T + b1)))
    Y = S @ w2 + b2
    last = np.zeros(r.shape[0], bool)
    last[offs[1:] - 1] = True
    nxt = np.append(Y[1:], 0.0)
    tgt = np.where(last, rew, rew + float(gamma) * nxt)
    if zero_sum:
        tgt = lambda_returns(Y, rew, offs, gamma, lam, movers=record_movers(r))
    elif lam != 0.0:
        tgt = lambda_returns(Y, rew, offs, gamma, lam)
    T =np.repeat(lens, lens).astype(np.float64)
    diff = Y - tgt
    loss = float((diff * diff / T).sum() / E)
    d = 2.0 * diff / (E * T)
    dh = (d[:, None] * w2[None, :]) * (1.0 - S) * S
    grad = np.concatenate([(dh.T @ X).reshape(-1), dh.sum(0), S.T @ d, [d.sum()]])
    return {"grad": grad, "loss": loss, "Y": Y, "target": tgt, "td_error": float((np.abs(diff) / T).sum()),
            "predicted_value": float((Y / T).sum()), "reward": float(rew.sum())}


def adam_reference(params, m, v, step, grad, lr, grad_clip, norm=None):
    """clip_grad_norm_(grad_clip) and one Adam step (betas 0.9 / 0.999, eps 1e-8)
    in float32, as tb_adam_kernel orders them. step: the count before this update.
    norm: the gradient's 2-norm where the caller has one already (the kernel's
    comes from double partial sums, as the default here does).
    Returns dict(params, m, v float32 [n], step, norm, scale (the clip factor
    applied, 1 when none), u (the step added to params))."""
    f = np.float32
    p, m, v, g = (np.asarray(x, f).reshape(-1).copy() for x in (params, m, v, grad))
    norm = f(np.sqrt((g.astype(np.float64) ** 2).sum())) if norm is None else f(norm)
    scale = f(1.0)
    if grad_clip is not None and grad_clip > 0:
        coef = f(grad_clip) / (norm + f(1e-6))
        scale = coef if coef < f(1.0) else f(1.0)
        g = g * scale
    step = int(step) + 1
    bc1 = 1.0 - 0.9 ** step                      # bias corrections in double, as torch's
    bc2 = 1.0 - 0.999 ** step
    step_size = f(float(f(lr)) / bc1)
    bc2s = f(np.sqrt(bc2))
    w1m, w2v = f(1.0 - 0.9), f(1.0 - 0.999)
    m = m + w1m * (g - m)                        # lerp(m, g, 1 - beta1)
    v = v * f(0.999) + (w2v * g) * g             # mul(beta2).addcmul(g, g, 1 - beta2)
    den = np.sqrt(v) / bc2s + f(1e-8)
    u = ((-step_size) * m) / den                 # addcdiv(m, den, -step_size)
    p = p + u
    assert p.dtype == f and m.dtype == f and v.dtype == f
    return {"params": p, "m": m, "v": v, "step": step, "norm": norm, "scale": scale, "u": u}
