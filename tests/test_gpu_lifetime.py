"""Engine lifetime on the GPU: every device buffer, event, stream and mapped
host block an engine takes (create, match mode, a start table, stepping,
harvest) goes back at destroy. The engine's members own their allocations
(csrc/bgx_host.h DevBuf / Handle), so there is no list of pointers to keep in
step with the struct; this test is the check that nothing is left behind.
"""
import numpy as np
import pytest

from test_gpu_engine import _engine
from test_gpu_rollout import _table

pytestmark = pytest.mark.gpu

# The allowed drift of torch.cuda.mem_get_info()'s free bytes, taken from the
# engine with the hand-written free lists (the commit before the owners): the
# same cycle as below on an MI355X / ROCm 7 gave 308,365,230,080 B free after
# each of cycles 1..8, a difference of 0 B between any two cycles. So the
# granule that run shows is none at all, and the bound is equality.
GRANULE = 0


def _cycle(weights, other):
    boards, player = _table()
    e = _engine(weights, lanes=64, seed=1, ply=2, k_top=4)
    e.set_opponent(other)
    e.set_start(boards, player)
    e.step(4)
    h = e.harvest()
    e.sync()
    assert e.stats()["env_steps"] == 64 * 4
    del h
    e.set_start(None)
    e.set_opponent(None)
    e.close()


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_eight_engine_lifetimes_return_their_memory(weights_seed0, weights_ckpt):
    """64 lanes, 2-ply K = 4, 8 times in one process: create, enter match
    mode, set a 3-position start table, step 4, harvest, leave both modes,
    destroy. Free device memory after the 8th cycle is within one allocator
    granule of its value after the first (the first cycle's one-time costs --
    code objects, the stateless scratch pool, torch's own cache -- are in
    both)."""
    _cycle(weights_seed0, weights_ckpt)
    first = _free()
    for _ in range(7):
        _cycle(weights_seed0, weights_ckpt)
    last = _free()
    print(f"free after cycle 1: {first}, after cycle 8: {last}, difference {first - last} B")
    assert abs(first - last) <= GRANULE, (first, last)
