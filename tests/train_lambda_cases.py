"""Shared helpers of the batched TD(lambda) trainer tests (test_train_lambda_ref.py,
test_gpu_train_lambda.py), on top of train_batch_cases.py. A plain module, not a
conftest.
"""
import numpy as np

import train_batch_cases as tc

GAMMA = 0.99
F32_FACTOR = 4.0    # what DESIGN section 4 "Numerics" grants an fp32 chain in another summation order
FLOOR_ULPS = 2      # fp32 ulps of the largest reference value: a serial fp32 chain's own error can be 0 by chance
# every chunk width of the target stage (64 records) up to 256 at length - 1, equal and + 1
EDGE_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def rewards(rec):
    """float32 [m]: the reward word (word 9) of each record."""
    return np.ascontiguousarray(np.asarray(rec)[:, 9]).view(np.float32).copy()


def rel_err(got, want64):
    """max|got - want| / max|want| in float64."""
    want64 = np.asarray(want64, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want64).max() / np.abs(want64).max())


def floor_rel(want64):
    """FLOOR_ULPS fp32 ulps of max|want|, relative to it."""
    m = float(np.abs(np.asarray(want64, np.float64)).max())
    return FLOOR_ULPS * float(np.spacing(np.float32(m))) / m


def torch_lambda_grad(flat, rec, offs, gamma, lam, dtype, device="cpu"):
    """Autograd of the batched TD(lambda) loss (one forward per episode, the mean
    of the per-episode MSE losses) with the targets fed in detached: the serial
    lambda_returns in `dtype` on the detached Y. Returns (grad [25601], loss, Y,
    targets) as numpy float64."""
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
    tgt_host = lambda_returns(y_host, rewards(rec).astype(y_host.dtype), offs, gamma, lam)
    tgt = torch.from_numpy(tgt_host).to(device)
    loss = torch.stack([F.mse_loss(ys[e], tgt[offs[e]:offs[e + 1]]) for e in range(len(ys))]).mean()
    loss.backward()
    p = dict(net.named_parameters())
    grad = torch.cat([p[k].grad.reshape(-1) for k in ("fc1.weight", "fc1.bias", "value_head.weight",
                                                      "value_head.bias")])
    return (grad.double().cpu().numpy(), float(loss.detach().double().cpu()), y_host.astype(np.float64),
            tgt_host.astype(np.float64))
