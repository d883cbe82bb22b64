"""GPU tests of the pulse compressor (include/uchirp_mf.h, libuchirp_mf.so, uchirp/mf.py): every output against the float64
model inside the header's bound and the four formats consistent bit for bit; exact zeros and the indexing at the seams;
the records against uc_mf_select over the GPU's own powers; the same bits whatever the grid, the jobs' order, the staging
slot or the cut of a range into calls; the notebook's case and the chain scene -> down-converter -> compressor -> arrivals
on the device; the contract; the C host; the code object."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

import mf_util as u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mf():
    import os
    from uchirp import mf as m
    if not os.path.exists(m.LIB_PATH):   # a library that is there is taken as it is
        m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def dev_rows():
    import torch
    return {k: torch.from_numpy(np.array(u.rows(k))).to("cuda:0") for k in u.DTYPES}


def _bits(t):
    import torch
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _seams_apart(mf, rec, e, hop, k0, pos0, first, n, tol, n_in):
    """rec [n_segments] of one job against uc_mf_select over e: e[i] the power of the output first - 1 + i of the call (the
    GPU's own, from a call one output wider on each side; 0 where the row has none).  Everything is compared bit for bit
    but the sum (the kernel's own order; the caller checks it) and ONE kind of field: the neighbour of a candidate on a
    segment's first or last output lies in the next segment, and the record holds this segment's own transform's value of
    it, the stored output the other's.  Likewise the neighbours in front of the row's first output and behind its last one
    are no stored outputs: e holds the model's there.  Those fields are compared within `tol` (absolute)."""
    q0 = pos0 + first
    for k in range(len(rec)):
        lo, hi = max((k0 + k) * hop, q0), min((k0 + k + 1) * hop, q0 + n)        # the segment's outputs in range
        seg = np.zeros(hop + 2, np.float32)
        a = lo - 1 - (k0 + k) * hop + 1                                          # index in seg of the output lo - 1
        seg[a:a + hi - lo + 2] = e[lo - 1 - (q0 - 1):hi + 1 - (q0 - 1)]
        want = mf.select(seg, lo - (k0 + k) * hop, hi - (k0 + k) * hop)
        got = rec[k]
        assert got["count"] == want["count"] == hi - lo and got["n_cand"] == want["n_cand"] and got["reserved"] == 0, (k, got, want)
        for g, w in zip(got["cand"], want["cand"]):
            assert g["offset"] == w["offset"] and g["peak"].tobytes() == w["peak"].tobytes(), (k, got, want)
            q = (k0 + k) * hop + int(w["offset"]) - pos0                       # the candidate's element of the row
            for side, edge, end in (("left", 0, 0), ("right", hop - 1, n_in - 1)):
                if w["peak"] > 0 and (w["offset"] == edge or q == end):
                    assert abs(float(g[side]) - float(w[side])) <= tol, (k, side, got, want)
                else:
                    assert g[side].tobytes() == w[side].tobytes(), (k, side, got, want)


@pytest.mark.parametrize("n_taps", u.TAPS)
@pytest.mark.parametrize("kind", u.DTYPES)
def test_outputs_against_the_model_inside_the_bound(mf, dev_rows, kind, n_taps):
    """Rows of 3 * 2048 + 37 samples through two templates; pos0 0, S - 1 and 2^40 + 5; first 0 and 37; n = 1, up to the
    segment's end, one more, the rest of the row.  Every complex output within UC_MF_ERROR_C 2^-24 ||a_k|| ||h|| of the
    float64 model; REAL, POWER and MAG are the complex output's own values bit for bit; outputs with a stride leave the
    gaps untouched; the records are uc_mf_select's over the GPU's own powers."""
    import torch
    x = dev_rows[kind]
    want_rows = u.model_rows(kind, n_taps)
    m = mf.Mf(u.templates(n_taps))
    nj = len(u.JOBS)
    worst = 0.0
    for pos0 in u.positions(n_taps):
        B = mf.bound(u.rows(kind), u.templates(n_taps), u.JOBS, pos0)
        for first, n in u.ranges(n_taps, pos0):
            guard = torch.full((nj, n + 5), complex(7.0, -7.0), dtype=torch.complex64, device="cuda:0")
            y, rec = m.run(x, u.JOBS, pos0=pos0, first=first, n=n, y=guard[:, :n])
            got = y.cpu().numpy()
            assert (guard[:, n:] == complex(7.0, -7.0)).all()
            err = np.abs(got.astype(np.complex128) - want_rows[:, first:first + n])
            ratio = float((err / (2.0 ** -24 * B[:, first:first + n])).max())
            worst = max(worst, ratio)
            assert ratio <= mf.ERROR_C, (pos0, first, n, ratio)
            if n == 1 or n == u.NS - first:
                fguard = torch.full((nj, n + 3), -3.0, dtype=torch.float32, device="cuda:0")
                re, _ = m.run(x, u.JOBS, pos0=pos0, first=first, n=n, out="real", records=False, y=fguard[:, :n])
                assert re.cpu().numpy().tobytes() == got.real.tobytes() and (fguard[:, n:] == -3.0).all()
                pw, _ = m.run(x, u.JOBS, pos0=pos0, first=first, n=n, out="power", records=False)
                e = mf.power32(got)
                assert pw.cpu().numpy().tobytes() == e.tobytes()
                mg, rec2 = m.run(x, u.JOBS, pos0=pos0, first=first, n=n, out="mag")
                assert mg.cpu().numpy().tobytes() == np.sqrt(e).tobytes()
                assert _same(rec, rec2)                                         # the records do not depend on the format
                none, rec3 = m.run(x, u.JOBS, pos0=pos0, first=first, n=n, out=None)
                assert none is None and _same(rec, rec3)                        # nor on whether anything is stored
            # ---- the records: from a call one output wider on each side
            lo, hi = max(first - 1, 0), min(first + n + 1, u.NS)
            wide, _ = m.run(x, u.JOBS, pos0=pos0, first=lo, n=hi - lo, out="power", records=False)
            e = np.zeros((nj, n + 2), np.float32)
            e[:, lo - (first - 1):hi - (first - 1)] = wide.cpu().numpy()
            # what lies outside the row has no stored output: in front of it the exact value is 0, behind it the filter's tail
            if first + n == u.NS:
                e[:, n + 1] = (np.abs(u.model_tail(kind, n_taps)) ** 2).astype(np.float32)
            hop, k0, ns = mf.plan(n_taps, pos0, first, n)
            r = mf.records_of(rec)
            assert r.shape == (nj, ns)
            for i in range(nj):
                amp = np.sqrt(e[i].astype(np.float64).max())
                d = 2.0 * mf.ERROR_C * 2.0 ** -24 * float(B[i].max())
                _seams_apart(mf, r[i], e[i], hop, k0, pos0, first, n, 2.0 * amp * d + d * d, u.NS)
                # the sum: any order of float additions
                for k in range(ns):
                    a = max((k0 + k) * hop, pos0 + first) - (pos0 + first)
                    part = float(e[i, 1 + a:1 + a + int(r[i, k]["count"])].astype(np.float64).sum())
                    assert abs(float(r[i, k]["sum"]) - part) <= int(r[i, k]["count"]) * 2.0 ** -24 * part + 1e-30, (pos0, first, n, i, k)
    print("%s, %d taps: worst |gpu - model| / (2^-24 ||a_k|| ||h||) %.3f (bound %d)" % (kind, n_taps, worst, mf.ERROR_C))
    m.close()


def test_a_crest_on_the_rows_last_output_is_found(mf):
    """The neighbour behind a row's last output is the transform's own value: with a one-tap template that is 0 to the bound,
    and a row that ends on its greatest sample has its crest there."""
    import torch
    x = torch.zeros((1, 500), dtype=torch.float32, device="cuda:0")
    x[0, 498] = 1.0
    x[0, 499] = 2.0
    m = mf.Mf(np.array([1.0], np.complex64))
    y, rec = m.run(x, out="real")
    tol = mf.ERROR_C * 2.0 ** -24 * np.sqrt(5.0)
    r = mf.records_of(rec)[0, 0]
    top = r["cand"][0]
    assert np.abs(y.cpu().numpy() - x.cpu().numpy()).max() <= tol
    assert int(top["offset"]) == 499 and abs(float(top["peak"]) - 4.0) <= 5 * tol and abs(float(top["left"]) - 1.0) <= 3 * tol and float(top["right"]) <= tol * tol
    assert r["count"] == 500 and abs(float(r["sum"]) - 5.0) <= 10 * tol
    m.close()


def test_zeros_give_zeros_and_no_candidate(mf):
    import torch
    m = mf.Mf(u.templates(255))
    for dt in (torch.float32, torch.int32, torch.complex64):
        x = torch.zeros((2, 4500), dtype=dt, device="cuda:0")
        y, rec = m.run(x, [(0, 0), (1, 1)], pos0=2 ** 40 + 5)
        assert not _bits(m.run(x, [(0, 0), (1, 1)], out="power", records=False)[0]).any()
        assert (y == 0).all()
        r = mf.records_of(rec)
        assert r.shape[1] == mf.plan(255, 2 ** 40 + 5, 0, 4500)[2]
        assert not r["n_cand"].any() and not r["sum"].view(np.uint32).any() and not r["cand"]["peak"].any() and not r["cand"]["offset"].any()
        assert r["count"].sum() == 2 * 4500
    m.close()


@pytest.mark.parametrize("pos0", [0, 2 ** 40 + 5])
def test_unit_pulses_around_the_seams(mf, pos0):
    """A unit pulse at every position within +-2 of two segment seams, against one-tap templates at k = 0 and k = T - 1:
    the output is the pulse moved by k, to the bound, and nothing else: the indexing at the seams."""
    import torch
    T = 255
    hop = 2048 - T - 1
    n_in = 2 * hop + 700
    seams = [s for s in ((pos0 // hop + 1) * hop - pos0, (pos0 // hop + 2) * hop - pos0)]      # elements on a segment's first output
    taps = np.zeros((2, T), np.complex64)
    taps[0, 0] = 1.0
    taps[1, T - 1] = 1.0
    spots = [s + d for s in seams for d in (-2, -1, 0, 1, 2)]
    x = torch.zeros((2 * len(spots), n_in), dtype=torch.float32, device="cuda:0")
    jobs, where = [], []
    for i, q in enumerate(spots):
        for s, k in ((0, 0), (1, T - 1)):
            x[2 * i + s, q - k] = 1.0                                           # its output lands on q
            jobs.append((2 * i + s, s))
            where.append(q)
    m = mf.Mf(taps)
    y, rec = m.run(x, jobs, pos0=pos0)
    got = y.cpu().numpy()
    tol = mf.ERROR_C * 2.0 ** -24                                               # ||a_k|| = ||h|| = 1
    r = mf.records_of(rec)
    h, k0, ns = mf.plan(T, pos0, 0, n_in)
    for i, q in enumerate(where):
        want = np.zeros(n_in)
        want[q] = 1.0
        assert np.abs(got[i] - want).max() <= tol, (i, q)
        top = r[i, (pos0 + q) // hop - k0]["cand"][0]
        assert int(top["offset"]) == (pos0 + q) % hop and abs(float(top["peak"]) - 1.0) <= 3 * tol, (i, q, top)
    m.close()


def test_grids_orders_slots_and_cuts_give_the_same_bits(mf, dev_rows, uc_tuning, monkeypatch):
    import torch
    T = 1023
    hop = 2048 - T - 1                                                          # 1024: six segments and a part
    x = dev_rows["c32"]
    kw = dict(pos0=hop - 1, first=3, n=u.NS - 3, out="mag")
    monkeypatch.delenv("UC_MF_GRID", raising=False)
    m = mf.Mf(u.templates(T))
    whole, rec = m.run(x, u.JOBS, **kw)
    # ---- two calls in a row (the other staging slot), four unsynchronised ones on one stream
    again, rec_again = m.run(x, u.JOBS, **kw)
    assert _same(again, whole) and _same(rec_again, rec)
    outs = [m.run(x, u.JOBS, **kw) for _ in range(4)]
    torch.cuda.synchronize()
    assert all(_same(o, whole) and _same(r, rec) for o, r in outs)
    # ---- the jobs reordered, one job alone
    order = [2, 0, 3, 1]
    o, r = m.run(x, [u.JOBS[i] for i in order], **kw)
    assert _same(o, whole[order]) and _same(r, rec[order])
    o, r = m.run(x, u.JOBS[3:4], **kw)
    assert _same(o, whole[3:4]) and _same(r, rec[3:4])
    # ---- grids of 1 .. 5 workgroups: chunks of 28, 14, 10, 7 and 6 units
    for grid in (1, 2, 3, 4, 5):
        monkeypatch.setenv("UC_MF_GRID", str(grid))
        mg = mf.Mf(u.templates(T))
        o, r = mg.run(x, u.JOBS, **kw)
        assert _same(o, whole) and _same(r, rec), grid
        mg.close()
    monkeypatch.delenv("UC_MF_GRID")
    # ---- the range cut into calls at segment borders: the same outputs, and every segment's record
    pos0, first, n = kw["pos0"], kw["first"], kw["n"]
    h, k0, ns = mf.plan(T, pos0, first, n)
    cut = torch.empty_like(whole)
    recs = []
    at = first
    while at < first + n:
        end = min(((pos0 + at) // hop + 2) * hop - pos0, first + n)             # two segments a call (the first: what is left of two)
        o, r = m.run(x, u.JOBS, pos0=pos0, first=at, n=end - at, out="mag", y=cut[:, at - first:end - first])
        recs.append(r)
        at = end
    assert _same(cut, whole) and _same(torch.cat(recs, dim=1), rec)
    # ---- a live caller who keeps T samples of history: the tail of the row alone, its window inside both rows
    start = ((pos0 + 2 * hop) // hop) * hop - pos0                              # the element on a segment's first output
    tail = x[:, start - T:].contiguous()
    o, r = m.run(tail, u.JOBS, pos0=pos0 + start - T, first=T, n=u.NS - start, out="mag")
    k_start = (pos0 + start) // hop - k0
    assert _same(o, whole[:, start - first:]) and _same(r, rec[:, k_start:])
    m.close()


def test_notebook_case_on_the_device(mf):
    """'Compress chirp in time domain' on the GPU: the crest at index 881, every output inside the bound of lfilter's."""
    import scipy.signal
    import torch
    buf, down = u.notebook_case()
    x = torch.from_numpy(buf.astype(np.float32)[None]).to("cuda:0")
    m = mf.Mf(down)
    y, rec = m.run(x)
    got = y.cpu().numpy()[0]
    want = scipy.signal.lfilter(down.astype(np.float32).astype(np.float64), 1, buf.astype(np.float32).astype(np.float64))
    B = mf.bound(buf.astype(np.float32), down)[0]
    ratio = float((np.abs(got - want) / (2.0 ** -24 * B)).max())
    print("notebook on the device: worst |gpu - lfilter| / (2^-24 ||a_k|| ||h||) %.3f (the emulation: 1.56)" % ratio)
    assert ratio <= mf.ERROR_C and int(np.argmax(np.abs(got))) == 881
    found = mf.arrivals(mf.records_of(rec), m.plan(0, 0, buf.size), min_ratio=8.0)[0]
    best = max(found, key=lambda a: a[1])
    assert abs(best[0] - 881.0) <= 0.01 and abs(best[1] / np.abs(want).max() - 1.0) <= 1e-3
    m.close()


def test_chain_on_the_device(mf):
    """Scene.render, two microphones with two paths each -> Ddc.run -> Mf.run -> arrivals, against the same chain in float64
    (scene.model | ddc.model | mf.model | the candidates' parabolas): positions within 1e-3 decimated samples; against the
    truth, and for the spacing of a microphone's two paths, within twice what the CPU suite records (mf_util.CHAIN_RECORDED)."""
    import torch
    from uchirp import ddc, scene
    x = scene.Scene(0, **u.CHAIN_FMT).render([""], u.CHAIN_MICS, n_samples=u.CHAIN_SAMPLES, seed=u.CHAIN_SEED)
    z, _ = ddc.Ddc(chain_lpf32(), u.DECIM, 0).run(x, steps=[ddc.step_of(u.CARRIER, u.FS)] * len(u.CHAIN_MICS))
    m = mf.Mf(u.chain_template())
    y, rec = m.run(z, out=None)
    assert y is None
    plan = m.plan(0, 0, int(z.shape[1]))
    got = mf.arrivals(mf.records_of(rec), plan, min_ratio=20.0)
    _, _, cand = u.chain64(x.cpu().numpy())
    worst = spacing = 0.0
    for i, (_, paths) in enumerate(u.CHAIN_MICS):
        truth = sorted(u.chain_truth(ld) for (_, _, ld, _) in paths)
        assert len(got[i]) == 2, got[i]                                         # the two paths and nothing else above 20 x the mean
        want = sorted(p for (p, _, _) in cand[i][0][:2])
        for (p, hgt), w, t in zip(got[i], want, truth):
            print("microphone %d: arrival at %.4f (float64 chain %.4f, truth %.4f), height %.1f" % (i, p, w, t, hgt))
            assert abs(p - w) <= 1e-3 and abs(p - t) <= 2.0 * u.CHAIN_RECORDED
            worst = max(worst, abs(p - w))
        spacing = max(spacing, abs((got[i][1][0] - got[i][0][0]) - (truth[1] - truth[0])))
    print("chain: worst |gpu - float64 chain| %.2e decimated samples; worst spacing error %.4f (bar %.2f)" % (worst, spacing, 2.0 * u.CHAIN_RECORDED))
    assert spacing <= 2.0 * u.CHAIN_RECORDED
    m.close()


def chain_lpf32():
    return u.chain_lpf().astype(np.float32)


@pytest.fixture
def other_device():
    """The calling thread's current device while the object lives on device 0: device 1 where the machine has one, so that
    an entry point that left the object's device current would be seen.  With a single GPU device 0 is always current and
    the assertions on the current device cannot fail: the restore is then not tested."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_refused_calls_leave_the_object_usable(mf, dev_rows, other_device):
    import torch
    L = mf.lib()
    x = dev_rows["f32"]
    ns, T = u.NS, 256
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    m = mf.Mf()
    assert torch.cuda.current_device() == dev0
    jobs = np.zeros(3, mf.JOB_DTYPE)
    jobs["row"], jobs["set"] = [0, 2, 1], [1, 0, 1]
    first, n = 10, ns - 20
    hop, k0, nseg = mf.plan(T, 5, first, n)
    out = torch.full((3, n), 7.0, dtype=torch.float32, device="cuda:0")
    rec = torch.full((3, nseg, 20), 7, dtype=torch.int32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=mf.DTYPE_F32, n_rows=3, n_in=ns, in_stride=0, jobs=jobs, n_jobs=3, pos0=5, first=first, n=n,
             out_ptr=out.data_ptr(), fmt=mf.OUT_REAL, out_stride=0, rec_ptr=rec.data_ptr()):
        rc = L.uc_mf_run(m._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_rows, n_in, in_stride,
                         jobs.ctypes.data_as(C.c_void_p) if jobs is not None else None, n_jobs, pos0, first, n, C.c_void_p(out_ptr), fmt, out_stride,
                         C.c_void_p(rec_ptr), stream)
        assert torch.cuda.current_device() == dev0
        return rc

    def changed(field, i, v):
        b = jobs.copy()
        b[field][i] = v
        return b

    assert call() == -errno.EINVAL and b"no templates" in L.uc_mf_last_error()      # nothing set yet
    h = u.templates(T)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = np.array(h)
    bad[1, 7] = np.nan
    for name, args in (("taps NULL", (None, 2, T)), ("no sets", (vp(h), 0, T)), ("257 sets", (vp(h), 257, 1)), ("no taps", (vp(h), 2, 0)),
                       ("1665 taps", (vp(h), 1, 1665)), ("a tap that is no number", (vp(bad), 2, T))):
        assert L.uc_mf_set_templates(m._h, *args) == -errno.EINVAL, name
        assert L.uc_mf_last_error(), name
    assert call() == -errno.EINVAL                                                  # a refused set leaves none
    m.set_templates(h)
    assert L.uc_mf_set_templates(m._h, vp(bad), 2, T) == -errno.EINVAL               # ... and a later one the former in place

    host = np.zeros(3 * ns, np.float32)
    refusals = [("row >= n_rows", dict(jobs=changed("row", 1, 3))), ("set >= n_sets", dict(jobs=changed("set", 2, 2))),
                ("row >= n_rows (fewer rows)", dict(n_rows=2)),
                ("first + n > n_in", dict(first=21)), ("first + n > n_in (n alone)", dict(first=0, n=ns + 1)),
                ("first beyond the row", dict(first=ns + 1, n=1)), ("first + n wraps", dict(first=2 ** 64 - 1, n=2)),
                ("pos0 + n_in beyond 2^64 - 1", dict(pos0=2 ** 64 - ns + 1)),
                ("out_stride < n", dict(out_stride=n - 1)), ("in_stride < n_in", dict(in_stride=ns - 1)),
                ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)), ("format 4", dict(fmt=4)), ("format -1", dict(fmt=-1)),
                ("no rows", dict(n_rows=0)), ("no input samples", dict(n_in=0)), ("no jobs", dict(n_jobs=0)), ("n = 0", dict(n=0)),
                ("jobs NULL", dict(jobs=None)), ("in NULL", dict(in_ptr=None)), ("out and records NULL", dict(out_ptr=None, rec_ptr=None)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("records: host memory", dict(rec_ptr=host.ctypes.data)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * ns)),
                ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (3 * ns - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (3 * n - 1))),
                ("records overlap in", dict(rec_ptr=x.data_ptr() + 4 * (3 * ns - 1))),
                ("records overlap out", dict(rec_ptr=out.data_ptr() + 4 * (3 * n - 1)))]
    if two:
        far_in = torch.zeros((3, ns), dtype=torch.float32, device="cuda:1")
        far_out = torch.zeros((3, n), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far_in.data_ptr())), ("out: memory of another device", dict(out_ptr=far_out.data_ptr())),
                     ("records: memory of another device", dict(rec_ptr=far_out.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_mf_last_error(), name
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max()) and int(rec.min()) == 7 == int(rec.max())    # nothing was enqueued
    assert call() == 0                                                              # and the object is as usable as before
    torch.cuda.synchronize()
    jl = list(zip(jobs["row"].tolist(), jobs["set"].tolist()))
    ref = mf.Mf(h)
    want, want_rec = ref.run(x, jl, pos0=5, first=first, n=n, out="real")
    assert _same(out, want) and _same(rec, want_rec)
    model = mf.model(u.rows("f32"), h, jl, first, n).real
    assert (np.abs(out.cpu().numpy() - model) <= mf.ERROR_C * 2.0 ** -24 * mf.bound(u.rows("f32"), h, jl, 5, first, n)).all()
    # only the records, only the outputs
    out.fill_(7.0)
    assert call(out_ptr=None) == 0 and call(rec_ptr=None) == 0
    torch.cuda.synchronize()
    assert _same(out, want) and _same(rec, want_rec)
    # four calls in a row that reuse (and overwrite) the same host array: the library has copied it when a call returns
    outs = [torch.empty((3, n), dtype=torch.float32, device="cuda:0") for _ in range(4)]
    sets = []
    for i in range(4):
        sets.append([(i % 3, i % 2), (2 - i % 3, 1), ((i + 1) % 3, 0)])
        jobs["row"], jobs["set"] = [q[0] for q in sets[i]], [q[1] for q in sets[i]]
        assert call(out_ptr=outs[i].data_ptr(), rec_ptr=None) == 0
    jobs["row"] = jobs["set"] = 0
    torch.cuda.synchronize()
    for i in range(4):
        assert _same(outs[i], ref.run(x, sets[i], pos0=5, first=first, n=n, out="real", records=False)[0]), i
    # new templates take effect, synchronously, behind the calls in flight
    m.set_templates(u.templates(255))
    assert _same(m.run(x, jl, out="power", records=False)[0], mf.Mf(u.templates(255)).run(x, jl, out="power", records=False)[0])
    h2 = C.c_void_p()
    assert L.uc_mf_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_mf_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    m.close()
    ref.close()
    assert torch.cuda.current_device() == dev0


def test_plain_c_host_finds_the_pulses(mf, tmp_path):
    from test_mf_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_mf_abi_version 1 (header 1)"
    assert any(ln.startswith("10000 outputs, worst error") and ln.endswith("4 of 4 arrivals in the records") for ln in lines), lines


def test_a_row_shorter_than_a_window(mf):
    """64 samples: one unit, a grid of one workgroup."""
    import torch
    m = mf.Mf(u.templates(2))
    x = torch.zeros((1, 64), dtype=torch.float32, device="cuda:0")
    y, rec = m.run(x)
    torch.cuda.synchronize()
    assert m.plan(0, 0, 64) == (2045, 0, 1) and tuple(rec.shape) == (1, 1, 20)
    m.close()
