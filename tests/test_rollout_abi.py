"""The rollout entry points at the C boundary, without a GPU: both symbols are
exported and bound, and argument errors come back as codes before any device
is touched."""
import ctypes
import subprocess

import pytest

from test_abi import built  # noqa: F401  (module fixture: builds libbgx.so when missing)


def test_rollout_symbols_are_exported_and_bound(built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    for name in ("bgx_engine_set_start", "bgx_rollout_tally"):
        assert f" T {name}\n" in out, name
    from bgx._lib import SIGNATURES
    import bgx
    L = bgx.lib()
    for name in ("bgx_engine_set_start", "bgx_rollout_tally"):
        assert name in SIGNATURES and getattr(L, name).restype is ctypes.c_int
    assert L.bgx_abi_version() == 10   # entry points were only added


def test_rollout_argument_errors_cross_abi_as_codes(built):  # noqa: F811
    import bgx
    L = bgx.lib()
    assert L.bgx_engine_set_start(None, None, None, None, 0, 0) == -1
    assert b"bgx_engine_set_start" in L.bgx_last_error()
    boards = (ctypes.c_uint8 * 52)()
    player = (ctypes.c_uint8 * 1)()
    assert L.bgx_engine_set_start(None, boards, player, None, 1, 0) == -1   # null engine, whatever the table
    counts = (ctypes.c_uint64 * 8)()
    assert L.bgx_rollout_tally(None, 1, None, 1, 1, None, None) == -1       # null pointers with a header to read
    assert b"bgx_rollout_tally" in L.bgx_last_error()
    assert L.bgx_rollout_tally(None, -1, None, 1, 1, counts, None) == -1    # n_headers < 0
    assert L.bgx_rollout_tally(None, 0, None, 0, 1, counts, None) == -1     # n_pos = 0
    assert L.bgx_rollout_tally(None, 1, None, 0, 1, counts, None) == -1
    assert L.bgx_rollout_tally(None, 0, None, 3, 1, None, None) == 0        # nothing to tally: no launch, no device
    assert list(counts) == [0] * 8


def test_rollout_python_surface_is_exported():
    import bgx
    from bgx import rollout
    assert bgx.rollout is rollout
    for name in ("rollout", "summarize", "tally_counts", "check_positions", "main"):
        assert callable(getattr(rollout, name))
    with pytest.raises(ValueError, match="position 0"):
        rollout.rollout({}, [[0] * 52], [0])   # rejected on the host before any engine exists
