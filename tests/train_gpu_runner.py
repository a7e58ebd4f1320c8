"""What the batched trainer's GPU tests share (test_gpu_train_batch.py, _lambda,
_zero_sum, _afterstate; _PM also test_gpu_train_seq.py): one runner for the four
update entry points, the shape table and its cached inputs, and the small
helpers of the DeviceTrainer tests. A plain module, not a conftest.

The shapes are the smallest that reach each way the kernels can go wrong, in
units of TILE (the backward launch's records per tile) and G (its largest
grid): one record; a bootstrap across a tile edge; an episode edge on a tile
edge; a ragged last tile with fewer tiles than workgroups; 2 G TILE + 7 records
(every workgroup sums over two tiles or more, the last one ragged); an episode
of 2,100 records (longer than the sequential kernel's 2,048); and one harvest
whose episode lengths put every width of the target stage's 64-record chunks up
to 256 at length - 1, equal and + 1."""
import numpy as np
import torch

import train_batch_cases as tc
import train_lambda_cases as lc

GAMMA, LR = lc.GAMMA, 1e-3
TD0, LAMBDA, TD, AFTER = ("bgx_td0_update_batched", "bgx_tdlambda_update_batched", "bgx_td_update_batched",
                          "bgx_td_afterstate_update_batched")   # the four entry points (include/bgx.h)
CASES = ("one", "tile_edge_boot", "tile_edge_episode_edge", "ragged_tile", "two_tiles_each", "long_episode", "edges")
_CACHE = {}


def batch_shape():
    if "shape" not in _CACHE:
        from bgx.trainer import DeviceTrainer
        _CACHE["shape"] = DeviceTrainer.batch_shape()
    return _CACHE["shape"]


def _lens(case):
    tile, grid = batch_shape()
    return {"one": [1], "tile_edge_boot": [tile + 1], "tile_edge_episode_edge": [tile, 1],
            "ragged_tile": [1, tile - 1, 2, 1, 3], "two_tiles_each": tc.ragged_lens(2 * grid * tile + 7, 11),
            "long_episode": [2100], "edges": lc.EDGE_LENS}[case]


def _inputs(case):
    """(headers, records, offs) of a shape, built once."""
    if case not in _CACHE:
        _CACHE[case] = tc.synth(_lens(case), seed=100 + CASES.index(case))
    return _CACHE[case]


def device_args(entry, flat, m, v, step, rec, offs, hdr=None, want_target=True):
    """The named arguments of one ops.td_batched_call(entry, ...) from host arrays,
    lr / gamma / lam / flags / clip apart: device copies of the inputs and the
    state, zero metrics, NaN-filled grad_out and (where the entry has one and it
    is wanted) target_out, and a workspace of exactly the size the entry asks for."""
    from bgx import ops
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)   # noqa: E731
    n_rec, n_eps = len(rec), len(offs) - 1
    need = ops.td_batched_workspace(entry, n_rec)
    if entry == AFTER:   # the source index behind the lambda layout
        assert need == ops.td_batched_workspace(LAMBDA, n_rec) + 4 * ((n_rec + 3) // 4 * 4)
    has = ops.TD_BATCHED[entry][1]
    return {"records": torch.from_numpy(np.ascontiguousarray(rec).view(np.int32)).to(dev),
            "headers": torch.from_numpy(np.ascontiguousarray(hdr).view(np.int32)).to(dev) if "headers" in has else None,
            "offs": t(offs, np.int32), "n_eps": n_eps, "n_rec": n_rec,
            "state": (t(flat, np.float32), t(m, np.float32), t(v, np.float32),
                      torch.tensor([int(step)], dtype=torch.int32, device=dev)),
            "metrics": torch.zeros(5, dtype=torch.float64, device=dev),
            "grad_out": torch.full((len(flat),), float("nan"), dtype=torch.float32, device=dev),
            "target_out": torch.full((n_rec,), float("nan"), dtype=torch.float32, device=dev)
            if "target_out" in has and want_target else None,
            "work": torch.empty(need, dtype=torch.uint8, device=dev)}


def run(entry, flat, m, v, step, rec, offs, lam=0.0, flags=0, *, hdr=None, lr=LR, clip=1.0, gamma=GAMMA, want_target=True):
    """One call of a batched-update entry point (lam and flags go to the entries
    that have them, hdr to AFTER) from host arrays; everything it writes, as
    numpy ("target" only for the entries that have d_target_out; None when it
    was not asked for)."""
    from bgx import ops
    d = device_args(entry, flat, m, v, step, rec, offs, hdr=hdr, want_target=want_target)
    ops.td_batched(entry, lr=lr, gamma=gamma, lam=lam, flags=flags, clip=clip, **d)
    torch.cuda.synchronize()
    p, m, v, step = d["state"]
    y = d["work"][:4 * d["n_rec"]].view(torch.float32).cpu().numpy().copy()   # the workspace starts with V of every record
    out = {"p": p.cpu().numpy(), "m": m.cpu().numpy(), "v": v.cpu().numpy(), "step": int(step.item()),
           "grad": d["grad_out"].cpu().numpy(), "metrics": d["metrics"].cpu().numpy(), "Y": y}
    if "target_out" in ops.TD_BATCHED[entry][1]:
        out["target"] = d["target_out"].cpu().numpy() if want_target else None
    return out


def _state(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.random(n) * 1e-5).astype(np.float32)


class _PM:
    def __init__(self, sd):
        self.sd = {k: v.clone() for k, v in sd.items()}

    def get_parameters(self, device=None):
        return {k: v.to(device) if device else v for k, v in self.sd.items()}

    def set_parameters(self, sd):
        self.sd = {k: v.detach().cpu().clone() for k, v in sd.items()}

    def flat(self):
        return np.concatenate([self.sd[k].numpy().reshape(-1) for k in ("fc1.weight", "fc1.bias",
                                                                        "value_head.weight", "value_head.bias")])


def _adam64(p, m, v, step, g, lr, clip):
    """clip_grad_norm_ and Adam in float64."""
    norm = np.sqrt((g * g).sum())
    if clip > 0:
        g = g * min(1.0, clip / (norm + 1e-6))
    step += 1
    m = m + (1.0 - 0.9) * (g - m)
    v = v * 0.999 + (1.0 - 0.999) * g * g
    den = np.sqrt(v) / np.sqrt(1.0 - 0.999 ** step) + 1e-8
    return p - (lr / (1.0 - 0.9 ** step)) * m / den, m, v, step
