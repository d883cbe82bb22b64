"""One non-finite sample among clean rows, on the GPU: the zones the headers' "Non-finite samples" paragraphs state
(include/uchirp_xcorr.h, uchirp_align.h, uchirp_mf.h, uchirp_spec.h, uchirp_rate.h, uchirp_array.h,
uchirp_retime.h, uchirp_track.h, uchirp_wcorr.h), with the masks of tests/poison_util.py that tests/test_poison_cpu.py
proves against the float64 models.

Every case puts copies of one clean row set, each with ONE poisoned sample (NaN, +Inf, -Inf at every position of the
case), between clean copies into ONE call and compares with the clean call of the same shape:
  MUST      not finite;
  MAY       bit-identical to the clean call's, or not finite;
  MUST NOT  bit-identical, guard words behind every output row included.
No tolerance anywhere.  Each call runs at the default grid, at a grid of 1 (one workgroup or wave walks poisoned and clean
units back to back through the same LDS tiles and registers: where a carry-over would show) and at a grid of 2.
"""
import numpy as np
import pytest

import poison_util as pu

pytestmark = pytest.mark.gpu

CASES = pu.all_cases()
GUARD = 3                       # words behind every output row that no call may touch


def _ids(cases):
    return [c.name for c in cases]


def _copies(case):
    """[(pos or None, label, rows)]: a clean copy, every position x every poison value, a clean copy"""
    out = [(None, "clean", case.rows)]
    for pos in case.positions:
        for vname, v in pu.POISONS:
            out.append((pos, "%s %s %s" % (pos.label, pos.part or "", vname), pu.poisoned(case.rows, pos, v)))
    out.append((None, "clean", case.rows))
    assert len(out) == 2 + 3 * len(case.positions)          # nothing filtered out
    return out


def _zones(case, copies, name):
    must = np.stack([case.reads(p)[name] if p else np.zeros_like(case.reads(case.positions[0])[name]) for p, _, _ in copies])
    may = np.stack([case.may(p)[name] if p else np.zeros_like(must[0]) for p, _, _ in copies])
    return must, may


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _compare(what, got, ref, must, may):
    """got, ref: [copies, ..., width + GUARD]; must, may: [copies, ..., width]"""
    pad = [(0, 0)] * (must.ndim - 1) + [(0, GUARD)]
    must, may = np.pad(must, pad), np.pad(may, pad)
    assert got.shape == ref.shape == must.shape, what
    width = must.shape[-1] - GUARD
    assert np.isfinite(ref[..., :width]).all(), what
    bad = ~np.isfinite(got)
    same = _bits(got) == _bits(ref)
    assert bad[must].all(), (what, "a MUST output is finite", np.argwhere(must & ~bad)[:8])
    assert (same | bad)[may].all(), (what, "a MAY output is another finite number", np.argwhere(may & ~(same | bad))[:8])
    rest = ~(must | may)
    assert same[rest].all(), (what, "a MUST NOT word changed", np.argwhere(rest & ~same)[:8])
    print("%s: MUST %d not finite; MAY %d, %d of them not finite; MUST NOT %d bit-identical"
          % (what, must.sum(), may.sum(), (may & bad).sum(), rest.sum()))


def _grid(monkeypatch, lib, grid):
    var = "UC_%s_GRID" % lib.upper()
    if grid is None:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, str(grid))


# ------------------------------------------------------------------------------------------------- xcorr and align

CORR = [c for c in CASES if c.lib in ("xcorr", "align")]


@pytest.mark.parametrize("case", CORR, ids=_ids(CORR))
def test_correlators(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import align, xcorr
    mod, cls = (xcorr, xcorr.Xcorr) if case.lib == "xcorr" else (align, align.Aligner)
    copies = _copies(case)
    R, lags = case.rows.shape[0], 2 * case.L + 1
    pairs = [(c * R + ref, c * R + mic) for c in range(len(copies)) for ref, mic in case.PAIRS]
    must, may = _zones(case, copies, "corr")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()

    def run(obj, x):
        out = torch.full((len(pairs), lags + GUARD), 12345.678, dtype=torch.float64, device="cuda")
        obj.correlate(x, pairs, first=case.first, n=case.n, max_lag=case.L, out=out[:, :lags])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(len(copies), len(case.PAIRS), lags + GUARD)

    for grid in pu.GRIDS:
        _grid(monkeypatch, case.lib, grid)
        obj = cls()
        try:
            ref, got = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        _compare("%s grid %s" % (case.name, grid), got, ref, must, may)
        # the host's detector: the peak rule refuses a correlation with a value that is not finite
        hit = np.argwhere(must.any(axis=2))
        assert len(hit)
        for c, p in hit[:: max(1, len(hit) // 6)]:
            with pytest.raises(mod.XcorrError if case.lib == "xcorr" else mod.AlignError):
                mod.peak(got[c, p, :lags])
        assert mod.peak(got[0, 0, :lags])["flags"] is not None          # a clean pair of the same call is read as usual


# ------------------------------------------------------------------------------------------------------------ mf

MF = [c for c in CASES if c.lib == "mf"]


def _record_zones(what, rec, ref, must, may):
    """rec, ref: RECORD_DTYPE [copies, jobs, segments].  The record of a segment with a non-finite power: n_cand = 0, four
    zero slots, count as usual, reserved 0 and a sum that is not finite -- the caller's test."""
    assert rec.shape == ref.shape == must.shape, what
    raw, raw_ref = rec.view(np.int32).reshape(rec.shape + (20,)), ref.view(np.int32).reshape(ref.shape + (20,))
    same = (raw == raw_ref).all(axis=-1)
    dead = ((rec["n_cand"] == 0) & (raw[..., :16] == 0).all(axis=-1) & (rec["count"] == ref["count"]) & (rec["reserved"] == 0) &
            ~np.isfinite(rec["sum"]))
    assert np.isfinite(ref["sum"]).all() and (ref["n_cand"] > 0).all(), what
    assert dead[must].all(), (what, "a record of a non-finite segment", np.argwhere(must & ~dead)[:8])
    assert (same | dead)[may].all(), (what, "a MAY record", np.argwhere(may & ~(same | dead))[:8])
    rest = ~(must | may)
    assert same[rest].all(), (what, "a MUST NOT record changed", np.argwhere(rest & ~same)[:8])


@pytest.mark.parametrize("case", MF, ids=_ids(MF))
def test_mf(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import mf
    copies = _copies(case)
    jobs = [(c + row, s) for c in range(len(copies)) for row, s in case.JOBS]        # (one row a copy)
    assert case.rows.shape[0] == 1
    must, may = _zones(case, copies, "y")
    rmust, rmay = _zones(case, copies, "rec")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()
    shape = (len(copies), len(case.JOBS))

    def run(obj, x, fmt, records=True):
        y = None
        if fmt is not None:
            y = torch.full((len(jobs), case.n + GUARD), 12345.678, dtype=torch.complex64 if fmt == "complex" else torch.float32,
                           device="cuda")
        _, rec = obj.run(x, jobs, pos0=case.pos0, first=case.first, n=case.n, out=fmt, records=records,
                         y=None if y is None else y[:, :case.n])
        torch.cuda.synchronize()
        return (None if y is None else y.cpu().numpy().reshape(shape + (case.n + GUARD,)),
                None if rec is None else mf.records_of(rec).reshape(shape + (case.ns,)))

    for grid in pu.GRIDS:
        _grid(monkeypatch, "mf", grid)
        obj = mf.Mf(case.taps)
        try:
            for fmt in ("complex", "real", "power", "mag", None):
                what = "%s grid %s out %s" % (case.name, grid, fmt)
                (y0, r0), (y1, r1) = run(obj, x_clean, fmt), run(obj, x_bad, fmt)
                if fmt is not None:
                    _compare(what, y1, y0, must, may)
                _record_zones(what, r1, r0, rmust, rmay)
            y0, r0 = run(obj, x_clean, "power", records=False)
            y1, r1 = run(obj, x_bad, "power", records=False)
            assert r0 is None and r1 is None
            _compare("%s grid %s no records" % (case.name, grid), y1, y0, must, may)
        finally:
            obj.close()


# ---------------------------------------------------------------------------------------------------------- spec

SPEC = [c for c in CASES if c.lib == "spec"]


def _peak_rule(values, bin_first):
    """include/uchirp_spec.h: the largest stored value and its bin, the lowest bin on a tie; a NaN is never the largest; a
    frame whose stored values are all NaN has { NaN, bin_first }.  values: [..., bins] -> (value bits, bin)"""
    v = np.where(np.isnan(values), -np.inf, values.astype(np.float64))
    k = v.argmax(axis=-1)                                     # (the first maximum)
    best = np.take_along_axis(values, k[..., None], axis=-1)[..., 0]
    dead = np.isnan(values).all(axis=-1)
    return np.where(dead, np.float32(np.nan), best), np.where(dead, bin_first, bin_first + k)


@pytest.mark.parametrize("case", SPEC, ids=_ids(SPEC))
def test_spec(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import spec
    copies = _copies(case)
    zeros = np.zeros_like(case.rows)                          # a last copy of zeros: what the floor level of UC_SPEC_DB is
    must, may = _zones(case, copies, "out")
    pmust, _ = _zones(case, copies, "peak")
    grow = lambda m: np.concatenate([m, np.zeros_like(m[:1])])
    must, may, pmust = grow(must), grow(may), grow(pmust)
    n_rows = len(copies) + 1
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies) + [zeros])).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies] + [zeros])).cuda()
    nf, nb = case.n_frames, case.n_bins
    nan_copy = np.array([lab.endswith(" nan") for _, lab, _ in copies] + [False])

    def run(obj, x, kind):
        out = torch.full((n_rows, nf, nb + GUARD), 12345.678, dtype=torch.float32, device="cuda")
        _, rec = obj.spectra(x, out=out[:, :, :nb], peaks=True, floor=1e-3, **case.kw(kind))
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(n_rows, 1, nf, nb + GUARD), spec.peaks_of(rec)

    for grid in pu.GRIDS:
        _grid(monkeypatch, "spec", grid)
        obj = spec.Analyser()
        try:
            obj.set_window(None, case.FRAME_LEN)
            for kind in (spec.MAG, spec.POWER, spec.DB):
                what = "%s grid %s kind %d" % (case.name, grid, kind)
                (o0, p0), (o1, p1) = run(obj, x_clean, kind), run(obj, x_bad, kind)
                ac = case.bin_first + np.arange(nb) < case.ac_bins
                if kind != spec.DB:
                    _compare(what, o1, o0, must, may)
                else:
                    # UC_SPEC_DB: a NaN magnitude stores the floor level (a dead microphone reads as silence), a magnitude of
                    # +Inf stores +Inf; the floor level is what the row of zeros stores in every bin above the AC coupling
                    level = o0[-1, 0, 0, nb - 1]
                    assert np.isfinite(level) and (_bits(o0[-1, 0][:, :nb][:, ~ac]) == _bits(level)).all(), what
                    at_floor = _bits(o1) == _bits(level)
                    pad = np.pad(must, [(0, 0)] * 3 + [(0, GUARD)])
                    assert (at_floor | (o1 == np.inf))[pad].all(), (what, "a DB value of a poisoned frame")
                    assert at_floor[pad & nan_copy[:, None, None, None]].all(), (what, "a NaN sample stores the floor level")
                    assert (_bits(o1) == _bits(o0))[~pad].all(), (what, "a MUST NOT word changed")
                    print("%s: MUST %d, %d of them at the floor level, the others +Inf" % (what, pad.sum(), (pad & at_floor).sum()))
                # bins under the AC coupling store their constant in a poisoned frame too (they are MUST NOT words above)
                # ---- peaks: every record is the rule over the stored values; clean frames keep theirs bit for bit
                val, k = _peak_rule(o1[:, 0, :, :nb], case.bin_first)
                assert (_bits(p1["value"]) == _bits(val.astype(np.float32)))[~np.isnan(val)].all(), (what, "peak value")
                assert np.isnan(p1["value"][np.isnan(val)]).all() and (p1["bin"] == k).all(), (what, "peak bin")
                assert (p1.view(np.int64) == p0.view(np.int64))[~pmust[:, 0]].all(), (what, "a clean frame's peak changed")
                dead = pmust[:, 0] & nan_copy[:, None]        # the frames a NaN sample lies in
                assert dead.any()
                if kind != spec.DB and case.ac_bins <= case.bin_first:
                    assert np.isnan(p1["value"][dead]).all() and (p1["bin"][dead] == case.bin_first).all(), (what, "{ NaN, bin_first }")
                elif kind != spec.DB:
                    assert (p1["value"][dead] == 1.0).all() and (p1["bin"][dead] == case.bin_first).all(), (what, "the AC constant")
                else:
                    # { the larger of the AC constant and the floor level, bin_first }: the zeros' row stores the AC constant
                    # in its bin 0 and the floor level above the AC coupling
                    stated = max(o0[-1, 0, 0, 0], level) if case.bin_first < case.ac_bins else level
                    assert (_bits(p1["value"][dead]) == _bits(np.float32(stated))).all(), (what, "DB peak value")
                    assert (p1["bin"][dead] == case.bin_first).all(), (what, "DB peak bin")
        finally:
            obj.close()


# ---------------------------------------------------------------------------------------------------------- rate

RATE = [c for c in CASES if c.lib == "rate"]


@pytest.mark.parametrize("case", RATE, ids=_ids(RATE))
def test_rate(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import rate
    copies = _copies(case)
    must, may = _zones(case, copies, "out")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()
    assert len(copies) > 16                                   # more than one block of 16 rows

    def run(obj, x):
        out = torch.full((len(copies), case.n_out + GUARD), 12345.678, dtype=torch.float32, device="cuda")
        obj.convert(x, out=out[:, :case.n_out])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(len(copies), 1, case.n_out + GUARD)

    for grid in pu.GRIDS:
        _grid(monkeypatch, "rate", grid)
        obj = rate.Converter(0, case.up, case.down, case.HALF)
        try:
            ref, got = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        _compare("%s grid %s" % (case.name, grid), got, ref, must, may)


# --------------------------------------------------------------------------------------------------------- array

ARRAY = [c for c in CASES if c.lib == "array"]


@pytest.mark.parametrize("case", ARRAY, ids=_ids(ARRAY))
def test_array(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import array
    copies = _copies(case)
    R = case.rows.shape[0]
    beams = [[(c * R + mic, w, d) for mic, w, d in taps] for c in range(len(copies)) for taps in case.BEAMS]
    must, may = _zones(case, copies, "out")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()

    def run(obj, x):
        out = torch.full((len(beams), case.N_OUT + GUARD), 12345.678, dtype=torch.float32, device="cuda")
        obj.combine(x, beams, out_first=case.OUT_FIRST, n_out=case.N_OUT, out=out[:, :case.N_OUT])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(len(copies), len(case.BEAMS), case.N_OUT + GUARD)

    for grid in pu.GRIDS:
        _grid(monkeypatch, "array", grid)
        obj = array.Array()
        try:
            ref, got = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        _compare("%s grid %s" % (case.name, grid), got, ref, must, may)


# -------------------------------------------------------------------------------------------------------- retime

RETIME = [c for c in CASES if c.lib == "retime"]


@pytest.mark.parametrize("case", RETIME, ids=_ids(RETIME))
def test_retime(case, uc_tuning, monkeypatch):
    import torch
    from uchirp import retime
    copies = _copies(case)
    R = case.rows.shape[0]
    lines = [(c * R + mic, d, s) for c in range(len(copies)) for mic, d, s in case.LINES]
    must, may = _zones(case, copies, "out")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()

    def run(obj, x):
        out = torch.full((len(lines), case.N_OUT + GUARD), 12345.678, dtype=torch.float32, device="cuda")
        obj.rows(x, lines, out_first=case.OUT_FIRST, n_out=case.N_OUT, out=out[:, :case.N_OUT])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(len(copies), len(case.LINES), case.N_OUT + GUARD)

    for grid in pu.GRIDS:
        _grid(monkeypatch, "retime", grid)
        obj = retime.Retimer()
        try:
            ref, got = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        _compare("%s grid %s" % (case.name, grid), got, ref, must, may)


# --------------------------------------------------------------------------------------------------------- track

TRACK = [c for c in CASES if c.lib == "track"]


@pytest.mark.parametrize("case", TRACK, ids=_ids(TRACK))
def test_track(case, uc_tuning, monkeypatch):
    """from samples through uc_track_windows: the correlations' zones, and the crest records -- UC_TRACK_NOT_FINITE alone and
    every other byte zero for a (pair, window) with a MUST lag, bit-identical records elsewhere; uc_track_finish refuses"""
    import torch
    from uchirp import track
    copies = _copies(case)
    R, lags, W = case.rows.shape[0], 2 * case.L + 1, case.N_WINDOWS
    pairs = [(c * R + ref, c * R + mic) for c in range(len(copies)) for ref, mic in case.PAIRS]
    must, may = _zones(case, copies, "corr")
    cmust, _ = _zones(case, copies, "crest")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()
    shape = (len(copies), len(case.PAIRS), W)

    def run(obj, x):
        out = torch.full((len(pairs), W, lags + GUARD), 12345.678, dtype=torch.float64, device="cuda")
        cr, _ = obj.windows(x, pairs, case.FIRST, case.WINDOW, case.hop, W, case.L, corr=out[:, :, :lags])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(shape + (lags + GUARD,)), track.crests(cr).reshape(shape)

    for grid in pu.GRIDS:
        _grid(monkeypatch, "track", grid)
        obj = track.Tracker()
        try:
            (ref, c0), (got, c1) = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        what = "%s grid %s" % (case.name, grid)
        _compare(what, got, ref, must, may)
        raw0 = c0.view(np.uint8).reshape(shape + (track.CREST_BYTES,))
        raw1 = c1.view(np.uint8).reshape(shape + (track.CREST_BYTES,))
        assert (c0["flags"] & track.NOT_FINITE == 0).all(), what
        dead = (c1["flags"] == track.NOT_FINITE) & (raw1[..., 4:] == 0).all(axis=-1)
        assert dead[cmust].all(), (what, "a crest record without the flag alone", np.argwhere(cmust & ~dead)[:8])
        assert (raw1 == raw0).all(axis=-1)[~cmust].all(), (what, "a clean window's crest record changed")
        hit = np.argwhere(cmust)
        assert len(hit)
        with pytest.raises(track.TrackError):
            track.finish(c1[tuple(hit[0])], case.L)
        assert track.finish(c1[0, 0], case.L).shape == (W,)     # the clean copy's records finish as usual


# --------------------------------------------------------------------------------------------------------- wcorr

WCORR = [c for c in CASES if c.lib == "wcorr"]


@pytest.mark.parametrize("case", WCORR, ids=_ids(WCORR))
def test_wcorr(case, uc_tuning, monkeypatch):
    """guard 64 on the L' = 512 segments, with weights of ones, band weights and weights of zero: every stored lag of a
    (pair, window) one of whose segments holds the sample is not finite -- the lags of the guard are not stored, but what
    they read counts --, every other (pair, window) is bit-identical; uc_wcorr_peak refuses"""
    import torch
    from uchirp import wcorr
    copies = _copies(case)
    R, lags, W = case.rows.shape[0], 2 * case.L + 1, case.N_WINDOWS
    pairs = [(c * R + ref, c * R + mic) for c in range(len(copies)) for ref, mic in case.PAIRS]
    must, may = _zones(case, copies, "corr")
    x_clean = torch.from_numpy(np.concatenate([case.rows] * len(copies))).cuda()
    x_bad = torch.from_numpy(np.concatenate([r for _, _, r in copies])).cuda()
    shape = (len(copies), len(case.PAIRS), W)

    def run(obj, x):
        out = torch.full((len(pairs), W, lags + GUARD), 12345.678, dtype=torch.float64, device="cuda")
        obj.windows(x, pairs, case.FIRST, case.WINDOW, case.hop, W, case.L, case.GUARD, case.weights, out=out[:, :, :lags])
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(shape + (lags + GUARD,))

    for grid in pu.GRIDS:
        _grid(monkeypatch, "wcorr", grid)
        obj = wcorr.Wcorr()
        try:
            ref, got = run(obj, x_clean), run(obj, x_bad)
        finally:
            obj.close()
        what = "%s grid %s" % (case.name, grid)
        _compare(what, got, ref, must, may)
        if case.kind == "zero":       # "Weights of zero give 0.0" holds for finite inputs
            assert (ref[..., :lags] == 0.0).all(), what
        hit = np.argwhere(must.any(axis=3))
        assert len(hit)
        with pytest.raises(wcorr.WcorrError):
            wcorr.peak(got[tuple(hit[0])][:lags])
        assert wcorr.peak(got[0, 0, 0, :lags])["flags"] is not None     # a clean window of the same call is read as usual
