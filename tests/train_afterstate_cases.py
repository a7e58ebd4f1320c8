"""Shared inputs of the afterstate trainer tests (test_train_afterstate_ref.py,
test_cpuwave_afterstate.py, test_gpu_train_afterstate.py). A plain module, not
a conftest.

train_batch_cases.synth leaves the headers' final-board words zero. synth_after
fills them (header words 6..12) from base_records() boards drawn by index, and
sets the indicator bit (bit 16 of the packed word 6) AT RANDOM in the headers
and in every record's word 6, so that a loader that trusts the bit it finds
shows; word 11's mover stays as drawn. `trailing` appends records that no
episode covers (n_records = offs[-1] + trailing).
"""
import numpy as np

import train_batch_cases as tc

TILE = 128   # records per tile of the batched update (DeviceTrainer.batch_shape()[0])
IND = np.uint32(1 << 16)
# the tile loader's edges: a full tile, one record past it, an episode edge one
# record before the tile edge, one-record episodes, a ragged tile, two full
# tiles and one record
EMU_LENS = {"tile": [TILE], "tile_plus_1": [TILE + 1], "edge_before_tile_edge": [TILE - 1, 2], "ones": [1, 1, 1],
            "ragged_tile": [1, TILE - 1, 2, 1, 3], "two_tiles_and_one": [2 * TILE, 1]}
TRAILING = ("ragged_tile", 5)   # that case again with 5 records in no episode behind it


def synth_after(lens, seed, trailing=0, random_indicator=True):
    """(headers uint32 [E, 16], records uint32 [sum lens + trailing, 12], offs int64 [E + 1])."""
    hdr, rec, offs = tc.synth(lens, seed)
    rng = np.random.default_rng(seed + 7919)
    base = tc.base_records()
    E = len(hdr)
    hdr[:, 6:13] = base[rng.integers(0, len(base), E), :7]
    if trailing:
        rec = np.concatenate([rec, base[rng.integers(0, len(base), trailing)]])
    if random_indicator:
        hdr[:, 12] = (hdr[:, 12] & ~IND) | (rng.integers(0, 2, E).astype(np.uint32) << 16)
        rec[:, 6] = (rec[:, 6] & ~IND) | (rng.integers(0, 2, len(rec)).astype(np.uint32) << 16)
    return hdr, rec, offs


def movers_of(rec):
    return ((np.asarray(rec)[:, 11] >> 9) & 1).astype(np.uint32)


def rewritten(hdr, rec, offs):
    """rec with words 0..6 of every covered record replaced by its afterstate row
    (bgx.records.packed_afterstates); records past offs[-1] keep their words."""
    from bgx.records import packed_afterstates
    m = int(offs[-1])
    out = np.array(rec, np.uint32, copy=True)
    out[:m, :7] = packed_afterstates(hdr, out[:m])[:, :7]
    return out


def rows_by_hand(hdr, rec, offs):
    """The rows of the definition, one record at a time (uint32 [offs[-1], 7])."""
    out = np.zeros((int(offs[-1]), 7), np.uint32)
    for e in range(len(offs) - 1):
        a, b = int(offs[e]), int(offs[e + 1])
        for s in range(a, b):
            src = rec[s + 1, 0:7] if s < b - 1 else hdr[e, 6:13]
            out[s, :6] = src[:6]
            out[s, 6] = (int(src[6]) & 0xFFFF) | (((int(rec[s, 11]) >> 9) & 1) << 16)
    return out
