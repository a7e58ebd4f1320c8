"""CPU checks of the batched TD(0) update's checkers and boundary: the numpy
restatements (bgx/train_ref.py) against torch autograd / torch.optim.Adam, and
the argument rules of bgx_td0_batch_workspace / bgx_td0_update_batched (no GPU
needed: every rejection comes before the device is touched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG

import train_batch_cases as tc

LIB = os.path.join(PKG, "bgx", "libbgx.so")
GAMMA = 0.99


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    import bgx
    return bgx.lib()


def test_encode_records_matches_the_oracle_encoder():
    """The numpy encoder of packed record words equals the C oracle's encoding
    of the same boards (the mover's indicator)."""
    import oracle
    from bgx.train_ref import encode_records
    t = tc._load("env_traj.npz")
    idx = np.arange(0, len(t["board"]), 7)
    got = encode_records(tc.base_records()[idx])
    want = oracle.encode_many(t["board"][idx], (t["player"][idx] % 2))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("wname", list(tc.WEIGHTS))
def test_reference_gradient_equals_float64_autograd(wname):
    """batched_td0_reference against torch CPU float64 autograd of the batched
    loss: E = 3, lengths 1, 2 and 7."""
    from bgx.train_ref import batched_td0_reference
    flat = tc.flat_params(tc.WEIGHTS[wname])
    _, rec, offs = tc.synth([1, 2, 7], seed=5)
    ref = batched_td0_reference(flat, rec, offs, GAMMA)
    grad, loss, y = tc.torch_batched_grad(flat, rec, offs, GAMMA, torch.float64)
    assert ref["grad"].shape == (25601,) and ref["grad"].dtype == np.float64
    assert np.abs(ref["grad"] - grad).max() <= 1e-12 * np.abs(grad).max()
    assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ref["Y"] - y).max() <= 1e-12


def _ulps(got, want, *operands):
    """|got - want| in units of the fp32 spacing at the largest magnitude among
    the result and the operands of the sum that made it: a sum that cancels
    (an update as large as the parameter) keeps its operands' absolute error, so
    the spacing of the small result is not the unit of that error."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    mag = np.maximum(np.abs(got), np.abs(want))
    for o in operands:
        mag = np.maximum(mag, np.abs(np.asarray(o, np.float32)))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(mag, np.float32(1e-30)))


@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_adam_reference_equals_torch_adam(clip):
    """adam_reference against clip_grad_norm_ + one torch.optim.Adam step on CPU
    fp32 tensors, within 2 ulp per parameter (and per moment); the ulp is the
    spacing at the larger of the parameter and the step added to it (_ulps).
    The gradient is the batched loss's own; its norm, about 12, is above the
    clip of 1. With the clip active the reference gets torch's own norm, so that
    the run compares the clip and the Adam arithmetic: torch's fp32 norm of
    per-tensor norms and the reference's (a float64 sum, as the kernel's) differ
    in the last bits, checked here to 8 ulp, and that relative difference would
    otherwise reach every clipped gradient and twice over every second moment."""
    from bgx.net import BackgammonPolicyNetwork
    from bgx.train_ref import adam_reference, batched_td0_reference
    flat = tc.flat_params(tc.WEIGHTS["seed0"])
    _, rec, offs = tc.synth([1, 2, 7, 30], seed=6)
    net = BackgammonPolicyNetwork()
    net.load_state_dict(tc.state_dict(flat))
    params = [dict(net.named_parameters())[k] for k in ("fc1.weight", "fc1.bias", "value_head.weight",
                                                        "value_head.bias")]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    zero = np.zeros_like(flat)
    g = batched_td0_reference(flat, rec, offs, GAMMA)["grad"].astype(np.float32)
    own = adam_reference(flat, zero, zero, 0, g, 1e-3, clip)
    assert float(own["norm"]) > 1.0 and (own["scale"] < 1.0) == (clip > 0)
    o = 0
    for q in params:
        q.grad = torch.from_numpy(g[o:o + q.numel()].reshape(q.shape).copy())
        o += q.numel()
    norm = None
    if clip > 0:
        norm = float(torch.nn.utils.clip_grad_norm_(params, clip))
        assert abs(norm - float(own["norm"])) <= 8 * np.spacing(np.float32(norm))
    opt.step()
    r = adam_reference(flat, zero, zero, 0, g, 1e-3, clip, norm=norm)
    assert r["step"] == 1
    want = torch.cat([q.detach().reshape(-1) for q in params]).numpy()
    want_m = torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]).numpy()
    want_v = torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params]).numpy()
    for name, u in (("params", _ulps(r["params"], want, flat, r["u"])), ("m", _ulps(r["m"], want_m)),
                    ("v", _ulps(r["v"], want_v))):
        print(f"clip={clip} {name}: max {u.max():.2f} ulp")
        assert u.max() <= 2.0, (name, float(u.max()))
    # The default norm path (the reference's own float64 norm, checked against
    # torch's above): the parameters alone. The step -step_size m / (sqrt(v) /
    # sqrt(bc2) + eps) does not move with the gradient's scale, but a clip
    # coefficient that differs in its last bits gives each side its own rounded
    # gradient, so the step's fp32 roundings no longer cancel between the two:
    # w1m g; (w2v g) g and the square root (half of the two before it), / sqrt(bc2),
    # + eps; -step_size m; the quotient: at most 0.5 + (0.5 + 0.5) / 2 + 0.5 + 0.5 +
    # 0.5 + 0.5 + 0.5 = 3.5 ulp of the step on each side, and the final add's 0.5
    # each: 8 ulp between them, in the unit of _ulps.
    u = _ulps(own["params"], want, flat, own["u"])
    print(f"clip={clip} params, the reference's own norm: max {u.max():.2f} ulp")
    assert u.max() <= 8.0, float(u.max())


def test_workspace_query(L):
    b = ctypes.c_uint64(0)
    assert L.bgx_td0_batch_workspace(0, ctypes.byref(b)) == -1
    assert L.bgx_td0_batch_workspace(-5, ctypes.byref(b)) == -1
    assert L.bgx_td0_batch_workspace(1, None) == -1
    prev = 0
    for n in (1, 2, 127, 128, 129, 1000, 65543, 10 ** 6, 2 ** 31 - 1):
        assert L.bgx_td0_batch_workspace(n, ctypes.byref(b)) == 0
        assert b.value > 0 and b.value >= prev and b.value % 16 == 0, n
        assert b.value >= 8 * n + 256 * 25601 * 4   # Y, the episode info, one partial gradient per workgroup
        prev = b.value
    tile, grid = ctypes.c_int(0), ctypes.c_int(0)
    assert L.bgx_td0_batch_shape(ctypes.byref(tile), ctypes.byref(grid)) == 0
    assert tile.value > 0 and tile.value % 32 == 0 and 0 < grid.value <= 256


def test_update_batched_rejects_bad_arguments_before_the_device(L):
    """Each rule of include/bgx.h on its own; the other arguments are non-null
    (never dereferenced: the rejection comes first)."""
    need = ctypes.c_uint64(0)
    assert L.bgx_td0_batch_workspace(10, ctypes.byref(need)) == 0
    P = 0x10000   # a non-null, 16-byte aligned stand-in
    good = dict(rec=P, offs=P, n_eps=2, n_rec=10, params=P, m=P, v=P, step=P, metrics=P, grad=None, work=P,
                bytes=need.value)

    def call(**kw):
        a = dict(good, **kw)
        return L.bgx_td0_update_batched(a["rec"], a["offs"], a["n_eps"], a["n_rec"], a["params"], a["m"], a["v"],
                                        a["step"], 1e-3, 0.99, 1.0, a["metrics"], a["grad"], a["work"], a["bytes"],
                                        None)

    for k in ("rec", "offs", "params", "m", "v", "step", "metrics", "work"):
        assert call(**{k: None}) == -1, k
        assert b"null" in L.bgx_last_error()
    assert call(n_eps=0) == -1
    assert call(n_eps=-3) == -1
    assert call(n_eps=11) == -1          # n_records < n_eps
    assert call(bytes=need.value - 1) == -1
    assert b"work_bytes" in L.bgx_last_error()
    assert call(bytes=0) == -1
    assert call(work=P + 8) == -1
    assert b"aligned" in L.bgx_last_error()


def test_abi_version_unchanged(L):
    assert L.bgx_abi_version() == 10


def test_device_trainer_backend_default():
    """backend unset: "hip" for the sequential update, "torch" for the batched
    one (as before); an explicit "hip" with batched=True is kept."""
    import inspect
    from bgx.trainer import DeviceTrainer
    assert inspect.signature(DeviceTrainer.__init__).parameters["backend"].default is None

    class PM:
        def get_parameters(self, device=None):
            from bgx.net import BackgammonPolicyNetwork
            return BackgammonPolicyNetwork().state_dict()

        def set_parameters(self, sd):
            pass

    mk = lambda **kw: DeviceTrainer(PM(), device="cpu", **kw).backend   # noqa: E731
    assert mk() == "hip" and mk(batched=True) == "torch"
    assert mk(batched=True, backend="hip") == "hip" and mk(batched=False, backend="torch") == "torch"
    with pytest.raises(ValueError):
        mk(backend="cuda")
