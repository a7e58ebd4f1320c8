"""Shared helpers of the zero-sum target tests (test_train_zero_sum_ref.py,
test_gpu_train_zero_sum.py), on top of train_batch_cases.py and
train_lambda_cases.py. A plain module, not a conftest.
"""
import numpy as np

import train_batch_cases as tc
import train_lambda_cases as lc
from bgx.ops import TDF_ZERO_SUM  # noqa: F401  (BGX_TDF_ZERO_SUM, for the tests that pass flags)

# a single mover change this many records before an episode's end: the edge between the target
# stage's last two 64-record chunks (the flip of lane 63) and its two neighbours
FLIP_AT = (63, 64, 65)
PATTERNS = ("drawn", "alternating", "equal", "runs3") + tuple(f"flip{k}" for k in FLIP_AT)


def movers_of(rec):
    """int64 [m]: word 11 bit 9."""
    return ((np.asarray(rec)[:, 11] >> 9) & 1).astype(np.int64)


def set_movers(rec, movers):
    """A copy of rec with the mover of every record rewritten, in both places
    that carry it: word 11 bit 9 and the indicator, word 6 bit 16."""
    out = np.array(rec, dtype=np.uint32, copy=True)
    m = np.asarray(movers).astype(np.uint32)
    out[:, 11] = (out[:, 11] & ~np.uint32(1 << 9)) | (m << np.uint32(9))
    out[:, 6] = (out[:, 6] & ~np.uint32(1 << 16)) | (m << np.uint32(16))
    return out


def pattern_movers(rec, offs, pattern):
    """The movers of a pattern for the n = offs[-1] records in episodes (records
    past them keep theirs). drawn: as the records have them; alternating: every
    record another mover; equal: one mover everywhere; runs3: runs of three;
    flipK: one change per episode, between the records K + 1 and K from its end
    (none in an episode of K records or fewer)."""
    mv = movers_of(rec)
    if pattern == "drawn":
        return mv
    offs = np.asarray(offs, np.int64)
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        pos = np.arange(b - a)
        if pattern == "alternating":
            mv[a:b] = pos & 1
        elif pattern == "equal":
            mv[a:b] = 0
        elif pattern == "runs3":
            mv[a:b] = (pos // 3) & 1
        elif pattern.startswith("flip"):
            mv[a:b] = pos >= (b - a) - int(pattern[4:])
        else:
            raise ValueError(pattern)
    return mv


def with_pattern(rec, offs, pattern):
    """rec with the pattern's movers written into word 11 and word 6."""
    return set_movers(rec, pattern_movers(rec, offs, pattern))


def torch_zero_sum_grad(flat, rec, offs, gamma, lam, dtype, device="cpu"):
    """lc.torch_lambda_grad with the zero-sum targets: autograd of the batched
    loss (one forward per episode, the mean of the per-episode MSE losses) with
    the targets fed in detached, the serial lambda_returns(movers=) in `dtype`
    on the detached Y. Returns (grad [25601], loss, Y, targets) as numpy float64."""
    import torch
    import torch.nn.functional as F
    from bgx.net import BackgammonPolicyNetwork
    from bgx.train_ref import encode_records, lambda_returns
    net = BackgammonPolicyNetwork()
    net.load_state_dict(tc.state_dict(flat))
    net = net.to(dtype).to(device)
    obs = torch.from_numpy(encode_records(rec)).to(dtype).to(device)
    offs = [int(o) for o in offs]
    ys = [net(obs[offs[e]:offs[e + 1]]).reshape(-1) for e in range(len(offs) - 1)]
    y_host = torch.cat([y.detach() for y in ys]).cpu().numpy()
    tgt_host = lambda_returns(y_host, lc.rewards(rec).astype(y_host.dtype), offs, gamma, lam, movers=movers_of(rec))
    tgt = torch.from_numpy(tgt_host).to(device)
    loss = torch.stack([F.mse_loss(ys[e], tgt[offs[e]:offs[e + 1]]) for e in range(len(ys))]).mean()
    loss.backward()
    p = dict(net.named_parameters())
    grad = torch.cat([p[k].grad.reshape(-1) for k in ("fc1.weight", "fc1.bias", "value_head.weight",
                                                      "value_head.bias")])
    return (grad.double().cpu().numpy(), float(loss.detach().double().cpu()), y_host.astype(np.float64),
            tgt_host.astype(np.float64))
