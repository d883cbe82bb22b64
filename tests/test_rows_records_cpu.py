"""Oracle-only side of the receivers' record tests (tests/rows_records_util.py; the GPU side: tests/test_gpu_rows_records.py).

  * the sweep layout covers what the GPU test relies on: for every case and word type, every (side, bin) of both search windows
    decides a record as a clear winner at EACH of the 8 FIFO offsets;
  * the definition of a unit is the FIFO's: the m = 8 unit of a block is the block itself, a busy mask removes blocks, and main()'s
    switch run over the helper's records gives the trace of the oracle's own receiver, snr_up / snr_down included;
  * uc_debug_rx_records refuses a NULL context without a GPU."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import uco
import rows_records_util as rru
from rows_records_util import N, PER_BLOCK, STEP


@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("name", rru.SWEEP_CASES)
def test_every_window_bin_decides_a_record_at_every_fifo_offset(name, dtype):
    sw = rru.sweep(name, dtype)
    o, nf = sw.o, sw.n_frames
    whole = sw.whole()
    assert len(whole) == 2 * o.bandwidth2 and (o.bandwidth2 > 191) == ("wide" in name)
    assert sw.want.shape == (rru.ROWS, PER_BLOCK * sw.nb, 2) and sw.unit.max() < PER_BLOCK * sw.nb
    # every tone frame lies whole on its designed unit, on every offset once
    _, own = o.process(sw.frames)
    for r in range(rru.ROWS):
        buf = np.concatenate([np.zeros(N, sw.x.dtype), sw.x[r]])
        for q in range(nf):
            k = int(sw.unit[r, q]) + 1
            assert k % PER_BLOCK == sw.m[r, q] % PER_BLOCK
            assert np.array_equal(buf[STEP * k: STEP * k + N], sw.frames[q]), (r, q)
        for h in range(2):      # ... so its record is the frame's own
            assert np.array_equal(sw.want[r, sw.unit[r], h], own[:, h]["mag_max"].astype(np.float64)), (r, h)
    assert all(sorted(sw.m[:, q]) == list(range(1, 9)) for q in range(nf))
    counts = []
    for m in range(1, 9):
        cov = sw.coverage(m)
        counts.append(len(cov))
        assert cov == whole, "%s %s offset %d: %d of %d (side, bin) decide a record" % (name, dtype, m, len(cov), len(whole))
    designed = sw.designed()
    assert len(designed) >= 8 * len(whole)
    assert not np.isnan(sw.want).any() and (sw.want[[d[0] for d in designed], [d[1] for d in designed], [d[2] for d in designed]] > 0).all()
    print("%-20s %-8s %5d frames in %d rows of %4d blocks: %d of %d (side, bin) at each of 8 offsets, %d designed records"
          % (name, dtype, nf, rru.ROWS, sw.nb, min(counts), len(whole), len(designed)))


def _transmitted(dtype):
    from test_gpu_receive_many import _transmissions
    x, busy, msgs = _transmissions(6, seed=77, blocks=110)
    busy[1] = np.random.default_rng(3).random(busy.shape[1]) < 0.1
    if dtype == "int32":
        x = (np.round(x).astype(np.int64) * 256).astype(np.int32)
    return x, busy, msgs


@pytest.mark.parametrize("variant", [uco.RX_REAL, uco.SYNC_CPLX])
def test_the_last_unit_of_a_block_is_the_block_and_a_busy_mask_removes_blocks(variant):
    x, busy, _ = _transmitted("float32")
    x, busy = x[:3, :20 * N], busy[:3, :20].copy()
    busy[0, [0, 3, 4, 19]] = 1
    busy[2, :] = 1
    o = uco.Oracle(variant)
    want = rru.expected(o, x)
    assert want.shape == (3, PER_BLOCK * 20, 2)
    for s in range(3):
        _, st = o.process(x[s])
        for h in range(2):
            assert np.array_equal(want[s, PER_BLOCK - 1::PER_BLOCK, h], st[:, h]["mag_max"].astype(np.float64))
    masked = rru.expected(o, x, busy=busy)
    for s in range(3):
        keep = np.nonzero(busy[s] == 0)[0]
        assert masked[s].shape == (PER_BLOCK * keep.size, 2)
        if keep.size:
            packed = np.concatenate([x[s, b * N:(b + 1) * N] for b in keep])
            assert np.array_equal(masked[s], rru.expected_row(o, packed))
    # a block in front other than zeros: the units of block 5 onwards, with block 4 in front, are the whole stream's
    assert np.array_equal(rru.expected(o, x[:, 5 * N:], prev=x[:, 4 * N:5 * N]), want[:, PER_BLOCK * 5:])
    assert np.array_equal(rru.last_accepted(x, None, busy)[0], x[0, 18 * N:19 * N])
    assert not rru.last_accepted(x, None, busy)[2].any()


@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("variant", [uco.RX_REAL, uco.SYNC_CPLX])
def test_the_switch_over_the_records_is_the_oracles_receiver(variant, dtype):
    """main()'s switch (include/uchirp_mainloop.hpp, restated in rows_records_util.replay) looking its frames up in the helper's
    records gives the oracle receiver's trace: the discrete fields exactly, snr_up / snr_down of the tracking blocks to float32
    rounding.  This ties unit (jb, m) to FIFO position 256 (m + 8) of block jb -- the state machine the records feed."""
    x, busy, msgs = _transmitted(dtype)
    o = uco.Oracle(variant)
    tracking = decoded = 0
    for s in range(x.shape[0]):
        bz = busy[s] if busy[s].any() else None
        text, tr = o.receive(x[s], busy=bz)
        rec = rru.expected(o, x[s:s + 1], busy=None if bz is None else busy[s:s + 1])[0]
        blocks = np.arange(busy.shape[1]) if bz is None else np.nonzero(bz == 0)[0]
        mine = rru.replay(rec.astype(np.float32), blocks, thr=float(o.cfg.snr_threshold))
        assert len(mine) == len(tr)
        for f in ("block", "state_before", "state_after", "bit", "sync_position"):
            assert np.array_equal(mine[f], tr[f]), (s, f)
        act = tr["state_before"] >= 2
        for f in ("snr_up", "snr_down"):
            assert np.allclose(mine[f][act], tr[f][act], rtol=1e-6, atol=0.0), (s, f)
            assert not mine[f][~act].any() and not tr[f][~act].any()
        tracking += int(act.sum())
        decoded += int(msgs[s] in text)
    assert tracking >= 100 and decoded >= 3


def test_the_bar_knows_zeros_and_nans():
    want = np.array([[1000.0, 0.0], [np.nan, 2.0]])
    ok = np.array([[1000.0 * (1 + 1e-5), 0.0], [np.nan, 2.0]], np.float32)
    assert rru.worst_of(ok, want) <= 1.0
    for i, j, v in ((0, 0, 1000.05), (0, 1, -0.0), (0, 1, 1e-38), (1, 0, 3.0), (1, 1, np.nan), (0, 0, np.inf)):
        bad = ok.copy()
        bad[i, j] = v
        assert rru.worst_of(bad, want) > 1.0, (i, j, v)
    assert rru.passed_over(np.float32([0.0, -0.0, 1e15])).tolist() == [True, False, False]
    assert rru.passed_over(np.float32([0.0, 1e15]), poison=True).tolist() == [False, True]


def test_the_read_back_refuses_a_null_context():
    import uchirp
    uchirp.build()
    L = uchirp.lib()
    buf = np.zeros(16, np.float32)
    ns, units = C.c_size_t(5), C.c_size_t(5)
    assert L.uc_debug_rx_records(None, None, buf.ctypes.data_as(C.c_void_p), 8, C.byref(ns), C.byref(units)) == -errno.EINVAL
    assert (ns.value, units.value) == (0, 0) and not buf.any()
    assert L.uc_debug_rx_records(None, None, None, 0, None, None) == -errno.EINVAL
    assert b"uc_debug_rx_records" in L.uc_last_error()
