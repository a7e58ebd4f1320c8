"""Shared inputs of the batched TD(0) trainer tests (test_train_batch_ref.py,
test_gpu_train_batch.py): synthetic harvests built on the host. A plain module,
not a conftest.

Boards are the 4,534 positions of tests/golden/env_traj.npz, each made a record
once through bgx.records.pack_record; a case draws its records from them by
index and sets the reward word: 0 or a shaping value (0.2 / 0.3) inside an
episode, +/- a terminal value (1, 2, 2.5) on its last record.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_W1 = 128 * 198
_CACHE = {}


def _load(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
            _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def base_records():
    """uint32 [4534, 12]: one record per env_traj position (reward 0)."""
    if "base" not in _CACHE:
        from bgx.records import pack_record
        t = _load("env_traj.npz")
        b = t["board"].astype(np.uint32)
        w = np.zeros((len(b), 7), np.uint32)
        for i in range(48):
            w[:, i // 8] |= b[:, i] << np.uint32(4 * (i % 8))
        w[:, 6] = b[:, 48] | b[:, 49] << 4 | b[:, 50] << 8 | b[:, 51] << 12
        mover = (t["player"] % 2).astype(np.int64)
        out = np.stack([pack_record(w[k], int(mover[k]), float(t["v_obs"][k]), float(t["v_act"][k]), 0.0,
                                    int(t["action"][k]), int(t["num_moves"][k]), k % 300, t["roll"][k], 0, 0, 0, 0)
                        for k in range(len(b))])
        out.setflags(write=False)
        _CACHE["base"] = out
    return _CACHE["base"]


def synth(lens, seed):
    """(headers uint32 [E, 16], records uint32 [sum lens, 12], offs int64 [E + 1])."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    n, E = int(lens.sum()), len(lens)
    base = base_records()
    rec = base[rng.integers(0, len(base), n)].copy()
    offs = np.concatenate([[0], np.cumsum(lens)])
    rew = rng.choice(np.float32([0.0, 0.0, 0.0, 0.2, 0.3]), n)
    last = offs[1:] - 1
    rew[last] = rng.choice(np.float32([1.0, 2.0, 2.5]), E) * rng.choice(np.float32([1.0, -1.0]), E)
    rec[:, 9] = rew.astype(np.float32).view(np.uint32)
    rec[last, 11] |= np.uint32(1 << 6)   # done
    hdr = np.zeros((E, 16), np.uint32)
    hdr[:, 0] = np.arange(E)
    hdr[:, 2] = offs[:-1]
    hdr[:, 3] = lens
    hdr[:, 4] = lens
    hdr[:, 5] = rng.integers(1, 4, E).astype(np.uint32) | (rng.integers(0, 2, E).astype(np.uint32) << 8)
    return hdr, rec, offs


def ragged_lens(total, seed, lo=1, hi=90):
    """Episode lengths in [lo, hi] adding up to exactly `total`."""
    rng = np.random.default_rng(seed)
    out, left = [], int(total)
    while left > 0:
        k = min(int(rng.integers(lo, hi + 1)), left)
        out.append(k)
        left -= k
    return out


def flat_params(name):
    """float32 [25601] in state_dict order from a golden weight file."""
    w = _load(name)
    return np.concatenate([w[k].astype(np.float32).reshape(-1) for k in ("W1", "b1", "w2", "b2")])


def state_dict(flat):
    """The torch state_dict of flat parameters."""
    import torch
    f = np.asarray(flat, np.float32)
    return {"fc1.weight": torch.from_numpy(f[:N_W1].reshape(128, 198).copy()),
            "fc1.bias": torch.from_numpy(f[N_W1:N_W1 + 128].copy()),
            "value_head.weight": torch.from_numpy(f[N_W1 + 128:N_W1 + 256].reshape(1, 128).copy()),
            "value_head.bias": torch.from_numpy(f[N_W1 + 256:].copy())}


WEIGHTS = {"seed0": "weights_seed0.npz", "ckpt": "weights_ckpt2100000.npz"}


def torch_batched_grad(flat, rec, offs, gamma, dtype, device="cpu"):
    """Autograd of the batched loss (one forward per episode, targets detached,
    mean of the per-episode MSE losses): (grad [25601], loss, Y) as numpy float64."""
    import torch
    import torch.nn.functional as F
    from bgx.net import BackgammonPolicyNetwork
    from bgx.train_ref import encode_records
    net = BackgammonPolicyNetwork()
    net.load_state_dict(state_dict(flat))
    net = net.to(dtype).to(device)
    obs = torch.from_numpy(encode_records(rec)).to(dtype).to(device)
    rew = torch.from_numpy(np.ascontiguousarray(rec[:, 9]).view(np.float32).copy()).to(dtype).to(device)
    g = torch.tensor(gamma, dtype=dtype, device=device)
    losses, ys = [], []
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        y = net(obs[a:b]).reshape(-1)
        tgt = rew[a:b].clone()
        if b - a > 1:
            tgt[:-1] += g * y[1:].detach()
        losses.append(F.mse_loss(y, tgt))
        ys.append(y.detach())
    loss = torch.stack(losses).mean()
    loss.backward()
    p = dict(net.named_parameters())
    grad = torch.cat([p[k].grad.reshape(-1) for k in ("fc1.weight", "fc1.bias", "value_head.weight",
                                                      "value_head.bias")])
    return (grad.double().cpu().numpy(), float(loss.detach().double().cpu()),
            torch.cat(ys).double().cpu().numpy())
