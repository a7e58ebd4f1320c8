"""bgx_episode_offsets on the GPU: the CPU harness's size list against
numpy.cumsum, and one real harvest."""
import numpy as np
import pytest
import torch

from test_cpuwave_pack import OFFS_SIZES

pytestmark = pytest.mark.gpu


def test_offsets_equal_cumsum_at_every_edge_size():
    from bgx import ops
    rng = np.random.default_rng(11)
    big = torch.full((max(OFFS_SIZES) + 9,), -7, dtype=torch.int32, device="cuda")
    for n in OFFS_SIZES:
        hdr = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
        lens = rng.integers(0, 301, size=n)
        if n >= 2:
            lens[0], lens[-1] = 300, 0
        hdr[:, 3] = lens
        want = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        d_hdr = torch.from_numpy(hdr.view(np.int32)).cuda().reshape(n, 16)
        got = ops.episode_offsets(d_hdr)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n + 1,)
        assert np.array_equal(got.cpu().numpy(), want), n
        # into a caller's buffer: the first n + 1 elements, nothing behind them
        big.fill_(-7)
        view = ops.episode_offsets(d_hdr, out=big)
        assert view.data_ptr() == big.data_ptr()
        host = big.cpu().numpy()
        assert np.array_equal(host[:n + 1], want) and (host[n + 1:] == -7).all(), n


def test_offsets_of_a_real_harvest(weights_seed0):
    from bgx import Engine, ops
    e = Engine(lanes=256, seed=4, ply=1)
    try:
        e.set_weights(weights_seed0, temperature=1.5)
        e.step(300)
        h = e.harvest(clone=False)
        assert h.n_episodes >= 100
        offs = ops.episode_offsets(h.headers).cpu().numpy()
        lens = h.headers.cpu().numpy().view(np.uint32)[:, 3].astype(np.int64)
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]))
        assert int(offs[-1]) == h.n_records
    finally:
        e.close()


def test_offsets_argument_checks():
    from bgx import ops
    with pytest.raises(ValueError):
        ops.episode_offsets(torch.zeros((3, 12), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.episode_offsets(torch.zeros((3, 16), dtype=torch.int32, device="cuda"),
                            out=torch.zeros(3, dtype=torch.int32, device="cuda"))
