"""The receivers' band kernel (the ROWS build) by its own statistics, against the float64 oracle.

uc_receive_streams and uc_receive_streams_next run instantiations of band_kernel that nothing else runs (FRAMES ==
kFramesRows: RX_REAL and SYNC_CPLX, default and WIDE, float32 and int32 words): two buffer resources per frame, the split
chosen per FIFO offset m = 1 .. 8; unit -> (row, block, m) through a magic divisor; the ring slot of a unit is its index in
the group; live states add the need-word walk, the two halves, kept chunks; and a finaliser of their own writes only
(up, down) mag_max.  The receiver tests judge texts and traces of the modem's own chirps: the maximum sits on the same few
bins, everything else only has to stay below it.  Here uc_debug_rx_records reads the records back and every one of them is
compared with the oracle (tests/rows_records_util.py: the definition, the bar, the sweep; tests/test_rows_records_cpu.py
proves the helpers on the oracle alone):

  a. a tone through every window bin at every FIFO offset, through every ROWS instantiation;
  b. stream counts, block counts and strides that exercise the divisor, ragged groups and unaligned rows, host and device memory;
  c. live states: chunks of any sizes, kept chunks, a busy-masked call, the need-word walk, forced need words, stepped calls;
  d. all-zero and all-NaN blocks;
  e. the contract of the read-back itself.

Every test prints its worst |gpu - oracle| / (MAG_TOL x scale) before it asserts (`pytest -s`)."""
import ctypes as C
import errno

import numpy as np
import pytest

from oracle import uco
import rows_records_util as rru
from rows_records_util import N, PER_BLOCK
import tone_sweep_util as tsu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


def _engine(uchirp, monkeypatch, case, dtype, env=None):
    variant, cfg = tsu.config(case)
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = uchirp.Engine(variant, mag_mean=1000.0 * (256 if dtype == "int32" else 1), **cfg)
    for k in env:
        monkeypatch.delenv(k)
    return e


def _geometry(e, o, case):
    """The numbers the dispatcher selects default or WIDE by (tests/test_gpu_tone_sweep.py: _assert_geometry)."""
    assert (e.n, e.bandwidth, e.bandwidth2, e.idx_left_zero) == (o.n, o.bandwidth, o.bandwidth2, o.idx_left_zero)
    assert e.n == N and e.bandwidth2 == tsu.CASES[case][3]["bw2"] and (e.bandwidth2 > 191) == ("wide" in case)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- a. the tone sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("case", rru.SWEEP_CASES)
def test_tone_sweep_through_every_fifo_offset(uchirp, monkeypatch, uc_tuning, case, dtype):
    import torch
    sw = rru.sweep(case, dtype)
    e = _engine(uchirp, monkeypatch, case, dtype)
    _geometry(e, sw.o, case)
    xd = torch.tensor(sw.x, device="cuda:0")
    e.receive_many(xd, want_trace=False)                   # 8 streams: one launch, below the stepping thresholds
    g = e.rx_records()
    assert g.shape == (rru.ROWS, PER_BLOCK * sw.nb, 2)      # units == 8 nb
    r = rru.ratios(g, sw.want)
    designed = sw.designed()
    ix = tuple(np.array(designed).T)
    whole = sw.whole()
    reached = [len(sw.coverage(m) & whole) for m in range(1, 9)]
    print("%-20s %-8s %7d records  worst |gpu - oracle| / (MAG_TOL x scale) %.3f  designed records %6d, worst %.3f, (side, bin) "
          "reached per offset %d .. %d of %d" % (case, dtype, r.size, r.max(), len(designed), r[ix].max(), min(reached), max(reached),
                                                 len(whole)))
    assert r.max() <= 1.0, "first misses (row, unit, up/down): %r" % (np.argwhere(r > 1.0)[:8].tolist(),)
    assert min(reached) == len(whole) and (sw.want[ix] > 0).all() and r[ix].max() <= 1.0
    assert sorted(set(sw.m[:, 0])) == list(range(1, 9))
    # one workgroup, groups of 2 (whole rows no longer: every ring slot, the hand-out over many groups): the same bits
    e1 = _engine(uchirp, monkeypatch, case, dtype, {"UC_GRID": "1", "UC_BAND_GROUP": "2"})
    e1.receive_many(xd, want_trace=False)
    assert np.array_equal(_bits(e1.rx_records()), _bits(g)), "UC_GRID=1 UC_BAND_GROUP=2"
    # the same rows in a fixed permutation: the same bits, row by row
    perm = np.random.default_rng(tsu.PERM_SEED).permutation(rru.ROWS)
    assert (perm != np.arange(rru.ROWS)).sum() >= 6
    e.receive_many(xd[torch.from_numpy(perm).to("cuda:0")].contiguous(), want_trace=False)
    assert np.array_equal(_bits(e.rx_records()), _bits(g[perm])), "permuted rows"
    e.close()
    e1.close()


# ---- b. geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("geometry", list(rru.GEOMETRIES))
def test_stream_counts_block_counts_and_strides(uchirp, monkeypatch, geometry, dtype):
    """n_streams x blocks x stride x (host | device memory): the non-powers of two exercise the magic divisor, the stream counts
    give ragged groups, the strides rows that are only 4-byte aligned; what lies between the rows is NaN (int32: INT32_MIN)
    and must reach no record."""
    import torch
    x, o = rru.noisy_streams(geometry, dtype)
    want = rru.noisy_expected(geometry, dtype)
    e = _engine(uchirp, monkeypatch, rru.GEOMETRIES[geometry], dtype)
    _geometry(e, o, rru.GEOMETRIES[geometry])
    worst, calls, records = 0.0, 0, 0
    for ns in (1, 3, 4, 5, 37):
        for nb in (1, 2, 3, 5, 7, 9, 31):
            nsmp = nb * N
            w = want[:ns, :PER_BLOCK * nb]
            for stride in (nsmp, nsmp + 1, nsmp + 256, nsmp + 2049):
                host = np.full((ns, stride), rru.NAN_WORD[dtype])
                host[:, :nsmp] = x[:ns, :nsmp]
                for arg in (host[:, :nsmp], torch.from_numpy(host).to("cuda:0")[:, :nsmp]):
                    e.receive_many(arg, want_trace=False)
                    g = e.rx_records()
                    assert g.shape == w.shape, (ns, nb, stride)
                    assert not np.isnan(g).any(), (ns, nb, stride)
                    r = rru.ratios(g, w)
                    worst, calls, records = max(worst, float(r.max())), calls + 1, records + r.size
                    assert r.max() <= 1.0, "%d streams, %d blocks, stride %d, %s memory: %.3f at (stream, unit, up/down) %r" \
                        % (ns, nb, stride, "host" if isinstance(arg, np.ndarray) else "device", r.max(), np.argwhere(r > 1.0)[:4].tolist())
    print("%-20s %-8s %4d calls, %7d records  worst |gpu - oracle| / (MAG_TOL x scale) %.3f" % (geometry, dtype, calls, records, worst))
    assert (want > 0).all() and calls == 5 * 7 * 4 * 2
    e.close()


# ---- c. live states ------------------------------------------------------------------------------------------------
def _need_rule(g, w, poison, label):
    """A one-block call of a live state evaluates what the need word says: every component is within the bar, or passed over
    (exactly +0; exactly 1e15f under UC_RX_POISON=1).  No true record is 0 (noise in every sample), and every stream keeps at least
    3 of its 8 UP components (include/uchirp.h: 3 to 5 of 8 for an idle stream, 5 to 6 while tracking) -- a kernel that wrote zeros
    everywhere does not pass.  -> (worst ratio over the evaluated components, number of evaluated components)."""
    r = rru.ratios(g, w)
    over = rru.passed_over(g, poison)
    assert (w > 0).all()
    assert ((r <= 1.0) | over).all(), "%s: %r" % (label, np.argwhere(~((r <= 1.0) | over))[:6].tolist())
    kept_up = (~over[:, :, 0]).sum(axis=1)
    assert (kept_up >= 3).all(), "%s: UP components evaluated per stream %r" % (label, kept_up.tolist())
    return float(r[~over].max()), int((~over).sum())


SIZES = [1, 1, 3, 1, 2, 5, 1, 1, 7, 1, 8]         # 31 blocks


@pytest.mark.parametrize("kept,poison,masked", [(False, False, False), (True, False, False), (False, True, False),
                                                (False, False, True), (True, False, True)],
                         ids=["plain", "kept", "poison", "masked", "kept-masked"])
@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("geometry", ["rx_real", "sync_cplx"])
def test_live_states_chunk_after_chunk(uchirp, monkeypatch, uc_tuning, geometry, dtype, kept, poison, masked):
    """After every call on a live state its records equal the oracle on the stream so far: the block in front of the call comes
    from the state's halves, from the kept chunk (a ring of two buffers), or -- behind a busy-masked call -- is every stream's
    newest ACCEPTED block."""
    import torch
    x, o = rru.noisy_streams(geometry, dtype)
    ns = 5
    x = x[:ns]
    e = _engine(uchirp, monkeypatch, rru.GEOMETRIES[geometry], dtype, {"UC_RX_POISON": "1"} if poison else None)
    live = e.live(ns)
    live.keep_previous(kept)
    ring = [torch.full((ns, max(SIZES) * N + 64), 7, dtype=getattr(torch, dtype), device="cuda:0") for _ in range(2)]
    prev, b0 = None, 0
    worst = walked = 0.0
    evaluated = total = 0
    assert sum(SIZES) * N == x.shape[1]
    for k, nb in enumerate(SIZES):
        chunk = np.ascontiguousarray(x[:, b0 * N:(b0 + nb) * N])
        busy = None
        if masked and nb == 5:
            busy = np.zeros((ns, nb), np.uint8)
            busy[0, [0, 4]] = 1
            busy[1, :] = 1
            busy[2, [1, 2, 3]] = 1
            busy[3, 4] = 1
        if kept or k % 3 != 2:
            arg = ring[k % 2][:, :nb * N]
            arg.copy_(torch.from_numpy(chunk))
        else:
            arg = chunk                                   # host memory: staged by the library
        live.next(arg, busy=busy, want_trace=False)
        g = e.rx_records(live)
        assert g.shape == (ns, PER_BLOCK * nb, 2)
        w = rru.expected(o, chunk, prev=prev, busy=busy)
        label = "call %d (%d blocks)" % (k, nb)
        if busy is not None:                              # accepted rows only: what lies beyond them is stale
            for s in range(ns):
                if len(w[s]):
                    worst = max(worst, rru.worst_of(g[s, :len(w[s])], w[s]))
                    total += w[s].size
        elif nb == 1:
            wk, n_eval = _need_rule(g, w, poison, label)
            walked, evaluated, total = max(walked, wk), evaluated + n_eval, total + w.size
        else:
            worst, total = max(worst, rru.worst_of(g, w)), total + w.size
        assert max(worst, walked) <= 1.0, label
        prev = rru.last_accepted(chunk, prev, busy)
        b0 += nb
    print("%-10s %-8s %-12s %5d components  worst |gpu - oracle| / (MAG_TOL x scale) %.3f (whole calls) %.3f (one-block calls: "
          "%d components evaluated)" % (geometry, dtype, "kept" * kept + " poison" * poison + " masked" * masked, total, worst, walked,
                                       evaluated))
    assert evaluated >= 3 * ns * SIZES.count(1) and worst > 0 and walked > 0
    live.close()
    e.close()


@pytest.mark.parametrize("geometry", ["rx_real", "sync_cplx", "sync_cplx-wide294"])
def test_forced_need_words_evaluate_everything(uchirp, monkeypatch, uc_tuning, geometry):
    """UC_RX_NEED_FORCE=0x1ff: every replay leaves the need word "all 8 offsets and the DOWN statistics", so from the second
    one-block step on every component is evaluated, through the walk's own addressing."""
    x, o = rru.noisy_streams(geometry, "float32")
    want = rru.noisy_expected(geometry, "float32")
    ns, steps = 5, 6
    e = _engine(uchirp, monkeypatch, rru.GEOMETRIES[geometry], "float32", {"UC_RX_NEED_FORCE": "0x1ff", "UC_RX_POISON": "1"})
    live = e.live(ns)
    worst = 0.0
    for b in range(steps):
        live.next(np.ascontiguousarray(x[:ns, b * N:(b + 1) * N]), want_trace=False)
        g = e.rx_records(live)
        w = want[:ns, PER_BLOCK * b:PER_BLOCK * (b + 1)]
        assert g.shape == w.shape
        if b == 0:
            _need_rule(g, w, True, "step 0")
        else:
            worst = max(worst, rru.worst_of(g, w))
    print("%-20s forced need words, %d steps  worst |gpu - oracle| / (MAG_TOL x scale) %.3f" % (geometry, steps - 1, worst))
    assert worst <= 1.0
    live.close()
    e.close()


@pytest.mark.parametrize("dtype", rru.DTYPES)
@pytest.mark.parametrize("geometry", ["rx_real", "sync_cplx"])
def test_a_call_served_block_by_block_leaves_its_last_step(uchirp, monkeypatch, uc_tuning, geometry, dtype):
    x, o = rru.noisy_streams(geometry, dtype)
    want = rru.noisy_expected(geometry, dtype)
    ns, nb = 5, 3
    e = _engine(uchirp, monkeypatch, rru.GEOMETRIES[geometry], dtype, {"UC_RX_STEP_MIN": "1"})
    e.receive_many(np.ascontiguousarray(x[:ns, :nb * N]), want_trace=False)
    g = e.rx_records()
    assert g.shape == (ns, PER_BLOCK, 2)                 # units == 8: the last step's
    wk, n_eval = _need_rule(g, want[:ns, PER_BLOCK * (nb - 1):PER_BLOCK * nb], False, "last step")
    print("%-10s %-8s block by block: %d of %d components evaluated, worst |gpu - oracle| / (MAG_TOL x scale) %.3f"
          % (geometry, dtype, n_eval, g.size, wk))
    assert wk <= 1.0
    e.close()


# ---- d. edge frames ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", list(rru.GEOMETRIES))
def test_all_zero_and_all_nan_blocks(uchirp, monkeypatch, geometry):
    """Stream 0 holds an all-zero and an all-NaN block between ordinary ones: an exact +0 where the oracle has 0 (the m = 8 unit
    of the zero block), NaN in both components of the 15 units that touch the NaN block (include/uchirp.h) and nothing else;
    the stream next to it is what it is without stream 0, bit for bit."""
    x, o = rru.noisy_streams(geometry, "float32")
    x = np.array(x[:2, :7 * N])
    x[0, 2 * N:3 * N] = 0.0
    x[0, 4 * N:5 * N] = np.nan
    w = rru.expected(o, x)
    assert np.isnan(w[0]).all(axis=1).sum() == 15 and np.isnan(w[0]).any(axis=1).sum() == 15 and not np.isnan(w[1]).any()
    assert (w[0] == 0).all(axis=1).sum() == 1 and (w[0, PER_BLOCK * 2 + 7] == 0).all() and (w[1] > 0).all()
    e = _engine(uchirp, monkeypatch, rru.GEOMETRIES[geometry], "float32")
    e.receive_many(x, want_trace=False)
    g = e.rx_records()
    r = rru.ratios(g, w)
    print("%-20s zero and NaN blocks  worst |gpu - oracle| / (MAG_TOL x scale) %.3f, NaN units %d, zero units %d"
          % (geometry, r.max(), int(np.isnan(g[0]).all(axis=1).sum()), int((_bits(g[0]) == 0).all(axis=1).sum())))
    assert r.max() <= 1.0, np.argwhere(r > 1.0)[:8].tolist()
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(_bits(g) == 0, w == 0)
    e.receive_many(x[1:2], want_trace=False)
    assert np.array_equal(_bits(e.rx_records()[0]), _bits(g[1]))
    e.close()


# ---- e. the read-back's contract ------------------------------------------------------------------------------------
def test_the_read_back_refuses_what_it_must_and_changes_nothing(uchirp):
    import torch
    x, _ = rru.noisy_streams("rx_real", "float32")
    x = x[:4, :3 * N]
    L = uchirp.lib()
    e, other = uchirp.Engine(uchirp.RX_REAL), uchirp.Engine(uchirp.RX_REAL)
    live, foreign = e.live(4), other.live(4)
    buf = np.zeros(4 * 24 * 2, np.float32)
    ns, units = C.c_size_t(9), C.c_size_t(9)

    def call(ctx, st, cap, out=buf):
        return L.uc_debug_rx_records(ctx, st, out.ctypes.data_as(C.c_void_p) if out is not None else None, cap, C.byref(ns), C.byref(units))

    # before any call: nothing to read, on the context and on a state
    assert call(e._h, None, 96) == -errno.ENODATA and (ns.value, units.value) == (0, 0)
    assert call(e._h, live._h, 96) == -errno.ENODATA
    with pytest.raises(uchirp.UchirpError):
        e.rx_records()
    assert call(None, None, 96) == -errno.EINVAL
    assert call(e._h, foreign._h, 96) == -errno.EINVAL                      # a state of another context
    e.receive_many(x[:, :0], want_trace=False)                               # no whole block: still nothing
    assert call(e._h, None, 96) == -errno.ENODATA
    t0, tr0 = e.receive_many(x)
    assert call(e._h, None, 95) == -errno.EINVAL and (ns.value, units.value) == (4, 24)     # too small: the shape is reported
    assert call(e._h, None, 96, out=None) == -errno.EINVAL
    assert not buf.any()
    assert call(e._h, None, 96) == 96 and (ns.value, units.value) == (4, 24) and (buf > 0).all()
    assert call(e._h, live._h, 96) == -errno.ENODATA                        # the state has still seen nothing
    assert np.array_equal(e.rx_records().reshape(-1), buf)
    # a stream that is being captured
    xd = torch.from_numpy(np.ascontiguousarray(x[:, :N])).to("cuda:0")
    text = torch.zeros((4, 64), dtype=torch.uint8, device="cuda:0")
    ntext = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    live.next_into(xd, text, ntext)                                          # (an eager step sizes the state's scratch)
    assert call(e._h, live._h, 96) == 32 and (ns.value, units.value) == (4, 8)
    eager = buf[:64].copy()
    live.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    seen = []
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            live.next_into(xd, text, ntext, stream=side.cuda_stream)
            seen.append(call(e._h, live._h, 96))
    assert seen == [-errno.ENOTSUP]
    graph.replay()                                                           # the captured step, replayed: the same records
    torch.cuda.synchronize()
    assert call(e._h, live._h, 96) == 32 and np.array_equal(_bits(buf[:64]), _bits(eager))
    del graph
    # a receiver call after a read-back gives what it gives without one
    a, b = e.live(4), e.live(4)
    ta, tra = a.next(np.ascontiguousarray(x[:, :2 * N]))
    assert e.rx_records(a).shape == (4, 16, 2)
    ta2, tra2 = a.next(np.ascontiguousarray(x[:, 2 * N:]))
    tb, trb = b.next(np.ascontiguousarray(x[:, :2 * N]))
    tb2, trb2 = b.next(np.ascontiguousarray(x[:, 2 * N:]))
    assert ta == tb and ta2 == tb2
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(tra + tra2, trb + trb2))
    t1, tr1 = e.receive_many(x)
    assert t1 == t0 and all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(tr1, tr0))
    assert e.busy_counters() == 0
    for st in (a, b, live, foreign):
        st.close()
    e.close()
    other.close()
