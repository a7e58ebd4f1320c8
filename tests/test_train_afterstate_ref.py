"""The afterstate rows on the host (bgx.records.packed_afterstates) and the
float64 restatement on them (bgx.train_ref.batched_td0_reference(afterstates=True)):
the row of record s is the board after its move, the next record's before-board
or the header's final board on an episode's last record, under the indicator of
record s's own mover (word 11 bit 9), whatever indicator the source carries.
No GPU, no libbgx.so."""
import numpy as np
import pytest

import train_afterstate_cases as ac
import train_batch_cases as tc

GAMMA = 0.99


@pytest.mark.parametrize("lens", [[1], [1, 1, 1], [3, 1, 2], ac.EMU_LENS["ragged_tile"]], ids=str)
def test_rows_differ_from_next_observation_in_the_indicator_only(lens):
    from bgx.records import packed_afterstates, packed_before_after
    hdr, rec, offs = ac.synth_after(lens, seed=5)
    rows = packed_afterstates(hdr, rec)
    after = packed_before_after(hdr, rec)[1]
    assert rows.dtype == np.uint32 and rows.shape == (len(rec), 8)
    keep = np.full(8, 0xFFFFFFFF, np.uint32)
    keep[6] = 0xFFFFFFFF ^ (1 << 16)
    assert np.array_equal(rows & keep, after & keep)
    assert np.array_equal((rows[:, 6] >> 16) & 1, ac.movers_of(rec))
    assert not rows[:, 7].any() and not (rows[:, 6] >> 17).any()


def test_rows_spelled_out_by_hand():
    from bgx.records import packed_afterstates
    mv = lambda r: ((int(r[11]) >> 9) & 1) << 16   # noqa: E731
    lo = lambda w: int(w) & 0xFFFF                 # noqa: E731
    # one episode of one record: the header's board
    hdr, rec, offs = ac.synth_after([1], seed=1)
    rows = packed_afterstates(hdr, rec)
    assert rows[0, :6].tolist() == hdr[0, 6:12].tolist()
    assert int(rows[0, 6]) == lo(hdr[0, 12]) | mv(rec[0])
    # three episodes of one record: each its own header, never the next record
    hdr, rec, offs = ac.synth_after([1, 1, 1], seed=2)
    rows = packed_afterstates(hdr, rec)
    for e in range(3):
        assert rows[e, :6].tolist() == hdr[e, 6:12].tolist()
        assert int(rows[e, 6]) == lo(hdr[e, 12]) | mv(rec[e])
    # lengths 3, 1, 2: records 0, 1 and 4 take the next record, 2, 3 and 5 headers 0, 1 and 2
    hdr, rec, offs = ac.synth_after([3, 1, 2], seed=3)
    rows = packed_afterstates(hdr, rec)
    for s, nxt in ((0, 1), (1, 2), (4, 5)):
        assert rows[s, :6].tolist() == rec[nxt, :6].tolist()
        assert int(rows[s, 6]) == lo(rec[nxt, 6]) | mv(rec[s])
    for s, e in ((2, 0), (3, 1), (5, 2)):
        assert rows[s, :6].tolist() == hdr[e, 6:12].tolist()
        assert int(rows[s, 6]) == lo(hdr[e, 12]) | mv(rec[s])
    assert np.array_equal(rows[:, :7], ac.rows_by_hand(hdr, rec, offs))
    # the indicator bits the sources carry are random: some disagree with the mover, and the rows ignore them
    carried = [(int(w) >> 16) & 1 for w in (rec[1, 6], rec[2, 6], hdr[0, 12], hdr[1, 12], rec[5, 6], hdr[2, 12])]
    assert (np.array(carried) != ac.movers_of(rec)).any()


def test_headers_must_count_the_records():
    from bgx.records import packed_afterstates
    hdr, rec, _ = ac.synth_after([3, 1, 2], seed=3)
    with pytest.raises(ValueError):
        packed_afterstates(hdr, rec[:-1])


@pytest.mark.parametrize("zero_sum", [False, True])
@pytest.mark.parametrize("lam", [0.0, 0.7, 1.0])
def test_reference_on_afterstates_is_the_reference_on_rewritten_records(lam, zero_sum):
    from bgx.train_ref import batched_td0_reference, encode_afterstates, encode_records
    flat = tc.flat_params(tc.WEIGHTS["ckpt"])
    hdr, rec, offs = ac.synth_after([3, 1, 2, 40, 1, 17], seed=9)
    rec2 = ac.rewritten(hdr, rec, offs)
    assert not np.array_equal(rec2[:, :7], rec[:, :7]) and np.array_equal(rec2[:, 7:], rec[:, 7:])
    assert np.array_equal(encode_afterstates(hdr, rec), encode_records(rec2))
    a = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=zero_sum, afterstates=True, headers=hdr)
    b = batched_td0_reference(flat, rec2, offs, GAMMA, lam=lam, zero_sum=zero_sum)
    plain = batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=zero_sum)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["Y"], plain["Y"])
    with pytest.raises(ValueError):
        batched_td0_reference(flat, rec, offs, GAMMA, lam=lam, zero_sum=zero_sum, afterstates=True)
