"""bgx_harvest_canonical at the C boundary, without a GPU: both entry points
are exported and bound, the workspace size is host arithmetic, and every bad
argument comes back as BGX_E_ARG before any device is touched (the buffers here
are host memory: a launch would fail differently)."""
import ctypes
import subprocess

import pytest

from test_abi import built  # noqa: F401  (module fixture: builds libbgx.so when missing)

NAMES = ("bgx_harvest_canonical", "bgx_harvest_canonical_workspace")


def test_canonical_symbols_are_exported_and_bound(built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out, name
    from bgx._lib import SIGNATURES
    import bgx
    L = bgx.lib()
    for name in NAMES:
        assert name in SIGNATURES and getattr(L, name).restype is ctypes.c_int
    assert L.bgx_abi_version() == 10   # entry points were only added


def test_workspace_size(built):  # noqa: F811
    import bgx
    L = bgx.lib()
    b = ctypes.c_uint64(0)
    assert L.bgx_harvest_canonical_workspace(2000, 4096, ctypes.byref(b)) == 0
    # start [lanes + 1], cur [lanes], three index arrays [n] and in_offs [n + 1], int32, rounded up to 16 bytes
    assert b.value == (4 * (2 * 4096 + 1 + 4 * 2000 + 1) + 15) // 16 * 16
    assert L.bgx_harvest_canonical_workspace(0, 1, ctypes.byref(b)) == 0 and b.value == 16
    for n, lanes in ((-1, 4), (4, 0), (4, -3)):
        assert L.bgx_harvest_canonical_workspace(n, lanes, ctypes.byref(b)) == -1
        assert b"bgx_harvest_canonical_workspace" in L.bgx_last_error()
    assert L.bgx_harvest_canonical_workspace(4, 4, None) == -1


class _Bufs:
    """Host buffers, 64-byte aligned, for 4 episodes / 10 records / 8 lanes."""

    def __init__(self):
        self.raw = (ctypes.c_uint8 * 8192)(*([0x5A] * 8192))
        base = (ctypes.addressof(self.raw) + 63) // 64 * 64
        self.hdr, self.rec, self.ohdr, self.orec = base, base + 512, base + 1024, base + 1536
        self.offs, self.status, self.work = base + 2048, base + 2112, base + 2176
        self.work_bytes = 4096

    def call(self, L, **kw):
        a = dict(hdr=self.hdr, rec=self.rec, n=4, m=10, lane_base=0, lanes=8, ohdr=self.ohdr, orec=self.orec,
                 offs=self.offs, status=self.status, work=self.work, work_bytes=self.work_bytes)
        a.update(kw)
        return L.bgx_harvest_canonical(a["hdr"], a["rec"], a["n"], a["m"], a["lane_base"], a["lanes"], a["ohdr"],
                                       a["orec"], a["offs"], a["status"], a["work"], a["work_bytes"], None)


BAD = {
    "n_eps": dict(n=-1), "n_records": dict(m=-1), "lane_base": dict(lane_base=-1), "lanes_0": dict(lanes=0),
    "lanes_neg": dict(lanes=-5),
    "null_headers": dict(hdr=None), "null_records": dict(rec=None), "null_out_headers": dict(ohdr=None),
    "null_out_records": dict(orec=None), "null_out_offs": dict(offs=None), "null_status": dict(status=None),
    "null_work": dict(work=None), "null_out_offs_empty": dict(n=0, m=0, offs=None),
    "work_small": dict(work_bytes=4 * (2 * 8 + 1 + 4 * 4 + 1) - 1),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_are_refused_before_the_device(built, name):  # noqa: F811
    import bgx
    L = bgx.lib()
    b = _Bufs()
    assert b.call(L, **BAD[name]) == -1, name
    assert b"bgx_harvest_canonical" in L.bgx_last_error()
    assert bytes(b.raw) == bytes([0x5A] * 8192)


def test_misaligned_and_overlapping_pointers_are_refused(built):  # noqa: F811
    import bgx
    L = bgx.lib()
    b = _Bufs()
    for key in ("hdr", "rec", "ohdr", "orec", "work"):
        for off in (4, 8):
            assert b.call(L, **{key: getattr(b, key) + off}) == -1, key
            assert b"aligned" in L.bgx_last_error()
    for key in ("offs", "status"):
        for off in (1, 2, 3):
            assert b.call(L, **{key: getattr(b, key) + off}) == -1, key
            assert b"aligned" in L.bgx_last_error()
    # an output on top of an input (whole or in part), and outputs on top of each other
    for kw in (dict(ohdr=b.hdr), dict(orec=b.rec), dict(orec=b.rec + 48 * 9), dict(ohdr=b.hdr + 64 * 3),
               dict(offs=b.hdr + 16), dict(status=b.rec + 4), dict(work=b.hdr), dict(work=b.rec - 64),
               dict(orec=b.ohdr), dict(offs=b.work + 16)):
        assert b.call(L, **kw) == -1, kw
        assert b"overlaps" in L.bgx_last_error(), kw
    assert bytes(b.raw) == bytes([0x5A] * 8192)
