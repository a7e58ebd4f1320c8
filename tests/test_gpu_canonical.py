"""ops.canonical_harvest (bgx_harvest_canonical) on the GPU: the CPU harness's
well-formed cases against numpy.lexsort plus a host gather, byte for byte,
into caller buffers with guard rows; a real harvest of the fused and of the
phased engine, re-laid on the host in two more arrival orders; the argument
checks. (Malformed headers are the CPU harness's: tests/test_cpuwave_canon.py.)"""
import numpy as np
import pytest
import torch

from test_cpuwave_canon import arrival_orders, canonical, relaid, well_formed_cases

pytestmark = pytest.mark.gpu

GUARD = 9   # rows behind the outputs that must keep their fill


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _bytes(t):
    return t.cpu().numpy().tobytes()


def test_canonical_harvest_equals_lexsort_at_every_edge_shape():
    from bgx import ops
    cases = well_formed_cases()
    n_max = max(len(c[3]) for c in cases)
    m_max = max(len(c[4]) for c in cases)
    out = (torch.empty((n_max + GUARD, 16), dtype=torch.int32, device="cuda"),
           torch.empty((m_max + GUARD, 12), dtype=torch.int32, device="cuda"),
           torch.empty((n_max + 1 + GUARD,), dtype=torch.int32, device="cuda"))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for name, lane_base, lanes, hdr, rec, want in cases:
        n, m = len(hdr), len(rec)
        d_hdr, d_rec = _dev(hdr).reshape(n, 16), _dev(rec).reshape(m, 12)
        for t in out:
            t.fill_(-7)
        gh, gr, go = ops.canonical_harvest(d_hdr, d_rec, lane_base=lane_base, lanes=lanes, out=out, status=status)
        # views of the caller's buffers (an empty view has no address)
        assert go.data_ptr() == out[2].data_ptr(), name
        assert (n == 0 or gh.data_ptr() == out[0].data_ptr()) and (m == 0 or gr.data_ptr() == out[1].data_ptr()), name
        assert tuple(gh.shape) == (n, 16) and tuple(gr.shape) == (m, 12) and tuple(go.shape) == (n + 1,), name
        first = (_bytes(gh), _bytes(gr), _bytes(go))
        assert first[0] == want[0].tobytes(), name
        assert first[1] == want[1].tobytes(), name
        assert first[2] == want[2].tobytes(), name
        # nothing behind the results, nothing in the inputs
        assert (out[0][n:] == -7).all() and (out[1][m:] == -7).all() and (out[2][n + 1:] == -7).all(), name
        assert _bytes(d_hdr) == hdr.tobytes() and _bytes(d_rec) == rec.tobytes(), name
        # the same call again, into fresh tensors (and the lane range read from the headers)
        again = ops.canonical_harvest(d_hdr, d_rec, lane_base=lane_base, status=status)
        assert tuple(_bytes(t) for t in again) == first, name
    assert int(status.item()) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_a_real_harvest_in_three_arrival_orders(weights_seed0, fused):
    from bgx import Engine, ops
    e = Engine(lanes=256, seed=4, ply=1, fused=fused)
    try:
        e.set_weights(weights_seed0, temperature=1.5)
        e.step(300)
        h = e.harvest(clone=False)
        assert h.n_episodes >= 100
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ops.canonical_harvest(h.headers, h.records, lanes=256, status=status)
        hdr = h.headers.cpu().numpy().view(np.uint32)
        rec = h.records.cpu().numpy().view(np.uint32)
        want = canonical(hdr, rec)
        first = tuple(_bytes(t) for t in got)
        assert first == tuple(w.tobytes() for w in want)
        key = (want[0][:, 0].astype(np.int64) << 32) | want[0][:, 1].astype(np.int64)
        assert (np.diff(key) > 0).all() and int(want[2][-1]) == h.n_records
        orders = arrival_orders(h.n_episodes, seed=9)
        for oname in ("reversed", "random"):
            oh, orr = relaid(hdr, rec, orders[oname])
            again = ops.canonical_harvest(_dev(oh).reshape(-1, 16), _dev(orr).reshape(-1, 12), lanes=256, status=status)
            assert tuple(_bytes(t) for t in again) == first, oname
        assert int(status.item()) == 0
    finally:
        e.close()


def test_canonical_harvest_argument_checks():
    from bgx import ops
    hdr = torch.zeros((3, 16), dtype=torch.int32, device="cuda")
    rec = torch.zeros((0, 12), dtype=torch.int32, device="cuda")
    ops.canonical_harvest(hdr[:0], rec, lanes=4)   # an empty harvest is fine
    for bad_h, bad_r in ((hdr.to(torch.int64), rec), (hdr, rec.to(torch.float32)),          # dtype
                         (torch.zeros((3, 12), dtype=torch.int32, device="cuda"), rec),     # width
                         (hdr, torch.zeros((0, 16), dtype=torch.int32, device="cuda")),
                         (hdr.cpu(), rec), (hdr, rec.cpu())):                               # device
        with pytest.raises(ValueError):
            ops.canonical_harvest(bad_h, bad_r, lanes=4)
    with pytest.raises(ValueError):   # out too small
        ops.canonical_harvest(hdr, rec, lanes=4, out=(hdr.clone()[:2], rec.clone(), torch.zeros(4, dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):
        ops.canonical_harvest(hdr, rec, lanes=4, status=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.canonical_harvest(hdr, rec, lanes=0)
