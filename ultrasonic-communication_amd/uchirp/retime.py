"""uchirp.retime -- the retimer: binding of libuchirp_retime.so (include/uchirp_retime.h), its float64 model, and the
host-side estimator of the lines it takes.

`Array.combine` (uchirp.array) shifts every microphone by a constant fractional delay: an array there shares one clock.
Microphones with clocks of their own drift against each other by tens of ppm, many carrier periods over a message.
`Retimer.rows` reads every row along a LINE, position(j) = j + delay + slope * j, through a 16-coefficient Kaiser-windowed
sinc whose coefficients follow the position from sample to sample, in one pass on the GPU, into a device tensor that
`Array.combine`, `Aligner.correlate`, `Xcorr.correlate` and the receivers read in place.  There is no CPU path behind
`Retimer`; `fixed`, `table` (the library's host functions) and the models need no GPU.

Lines are written as
    lines = [(mic, delay_samples, slope), ...]          one per output row
where the microphone hears the sound `delay_samples + slope * j` later than the output's time axis at output sample j.
`undo` gives the line of a row rendered by the link's law; `drift` estimates lines from a recording.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
COEFS = 16
TABLE_ROWS = 257
DELAY_MAX = 2.0 ** 30
SLOPE_MAX = 2.0 ** -9
SAMPLE_END_MAX = 2 ** 38
EXPORTS = ["uc_retime_abi_version", "uc_retime_last_error", "uc_retime_create", "uc_retime_destroy", "uc_retime_fixed",
           "uc_retime_table", "uc_retime_rows"]


class RetimeLine(C.Structure):
    """struct uc_retime_line (include/uchirp_retime.h)."""
    _fields_ = [("delay_samples", C.c_double), ("slope", C.c_double), ("mic", C.c_uint32), ("reserved", C.c_uint32)]


LINE_DTYPE = np.dtype([("delay_samples", "<f8"), ("slope", "<f8"), ("mic", "<u4"), ("reserved", "<u4")])


class RetimeError(RuntimeError):
    pass


def _declare(L):
    L.uc_retime_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_retime_fixed.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.uc_retime_table.argtypes = [C.POINTER(C.c_float)]
    L.uc_retime_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p]


_so = Binding("retime", RetimeError, _declare, env="UCHIRP_RETIME_LIB")  # UCHIRP_RETIME_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def fixed(delay, slope=0.0):
    """uc_retime_fixed: (lead_fx, drift_fx), the two integers the device works from, computed by the library (no GPU)."""
    lead, drift = C.c_int64(), C.c_int64()
    _check(lib().uc_retime_fixed(float(delay), float(slope), C.byref(lead), C.byref(drift)), "uc_retime_fixed")
    return int(lead.value), int(drift.value)


def fixed_model(delay, slope=0.0):
    """The fixed-point step of include/uchirp_retime.h in Python integers: the exact products rounded to the nearest
    integer, ties to even (llrint in the default rounding mode)."""
    delay, slope = float(delay), float(slope)
    if not (np.isfinite(delay) and np.isfinite(slope) and abs(delay) <= DELAY_MAX and abs(slope) <= SLOPE_MAX):
        raise ValueError("delay and slope must be finite, |delay| <= 2^30, |slope| <= 2^-9")
    return int(round(Fraction(delay) * 2 ** 32)), int(round(Fraction(slope) * 2 ** 32))


_table = None


def table():
    """uc_retime_table: T as float32 [257, 16], computed by the library on the host (no GPU); computed once and shared:
    do not write to it."""
    global _table
    if _table is None:
        t = (C.c_float * (TABLE_ROWS * COEFS))()
        _check(lib().uc_retime_table(t), "uc_retime_table")
        _table = np.frombuffer(t, np.float32).reshape(TABLE_ROWS, COEFS).copy()
        _table.setflags(write=False)
    return _table


def table_model():
    """The table of include/uchirp_retime.h in numpy: float32 [257, 16] (numpy's sine and Bessel function: it may differ
    from the library's in the last bit of an entry)."""
    t = np.zeros((TABLE_ROWS, COEFS), np.float32)
    t[0, 7] = 1.0
    t[256, 8] = 1.0
    f = np.arange(1, 256, dtype=np.float64)[:, None] / 256.0
    u = np.arange(COEFS, dtype=np.float64)[None, :] - 7.0 - f
    t[1:256] = (np.sin(np.pi * u) / (np.pi * u)) * np.i0(8.0 * np.sqrt(1.0 - (u / 8.0) ** 2)) / np.i0(8.0)
    return t


def pack(lines):
    """The host array of uc_retime_rows: LINE_DTYPE [n_lines] from (mic, delay_samples, slope) tuples."""
    out = np.zeros(len(lines), LINE_DTYPE)
    for i, (mic, delay, slope) in enumerate(lines):
        if int(mic) < 0:
            raise ValueError("line %d: microphone %d" % (i, int(mic)))
        out[i] = (float(delay), float(slope), int(mic), 0)
    return out


def undo(lead, ppm, ref_lead=0.0, ref_ppm=0.0):
    """(delay_samples, slope) of the line that puts a row rendered by the link's law at (lead, ppm) onto the sample axis of
    a reference rendered at (ref_lead, ref_ppm).

    The link's law (uchirp.link.signal) gives sample j of a stream the transmitter's time tt = j (1 + e) - lead (in output
    samples), e = ppm * 1e-6.  The reference's sample j holds the transmitter's time j (1 + e0) - ref_lead.  The row holds
    that same instant at the position p with p (1 + e) - lead = j (1 + e0) - ref_lead, so
        p = (j (1 + e0) - ref_lead + lead) / (1 + e) = j + (lead - ref_lead) / (1 + e) + j (e0 - e) / (1 + e):
    delay = (lead - ref_lead) / (1 + e) and slope = (e0 - e) / (1 + e)."""
    e, e0 = float(ppm) * 1e-6, float(ref_ppm) * 1e-6
    return (float(lead) - float(ref_lead)) / (1.0 + e), (e0 - e) / (1.0 + e)


class Retimer:
    """One uc_retime: the retimer on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_retime_create(int(device), C.byref(h)), "uc_retime_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_retime_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows_packed(self, x, lines, in_first=0, out_first=None, n_out=None, out=None, stream=None):
        """uc_retime_rows on an array as `pack` makes it (a loop of calls packs once)."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nm, n_in = int(x.shape[0]), int(x.shape[1])
        lines = np.ascontiguousarray(lines, LINE_DTYPE)
        nl = len(lines)
        if out_first is None:
            out_first = in_first
        if out is None:
            out = torch.empty((nl, n_in if n_out is None else int(n_out)), dtype=torch.float32, device=dev)
        else:
            if (out.dim() != 2 or out.dtype != torch.float32 or out.device != dev or out.shape[0] != nl or
                    (out.shape[1] > 1 and out.stride(1) != 1) or (nl > 1 and out.stride(0) < out.shape[1])):
                raise ValueError("out must be a [%d, n_out] float32 tensor on %s with contiguous rows" % (nl, dev))
            if n_out is not None and int(n_out) != out.shape[1]:
                raise ValueError("n_out does not match out")
        no = int(out.shape[1])
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_retime_rows(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm,
                                    int(in_first), n_in, int(x.stride(0)) if nm > 1 else n_in, lines.ctypes.data_as(C.c_void_p), nl,
                                    C.c_void_p(out.data_ptr()), int(out_first), no, int(out.stride(0)) if nl > 1 else no,
                                    C.c_void_p(stream) if stream else None), "uc_retime_rows")
        return out

    def rows(self, x, lines, in_first=0, out_first=None, n_out=None, out=None, stream=None):
        """uc_retime_rows: samples [out_first, out_first + n_out) of len(lines) rows -> a float32 torch tensor
        [n_lines, n_out] on the object's device (or into `out`: a 2-d device tensor with contiguous rows).  `x`: a 2-d
        float32 / int32 device tensor with contiguous rows holding the samples from `in_first` on.  out_first defaults to
        in_first and n_out to the length of x's rows.  Asynchronous on `stream` / torch's current stream."""
        return self.rows_packed(x, pack(lines), in_first=in_first, out_first=out_first, n_out=n_out, out=out, stream=stream)


def positions(delay, slope, out_first, n_out, fix=fixed_model):
    """The integer side of the definition for output samples [out_first, out_first + n_out): (I int64, q int64, mu float64)."""
    lead_fx, drift_fx = fix(delay, slope)
    j = np.arange(int(out_first), int(out_first) + int(n_out), dtype=np.int64)
    if len(j) and int(j[-1]) >= SAMPLE_END_MAX:
        raise ValueError("out_first + n_out > 2^38")
    off = np.int64(lead_fx) + j * np.int64(drift_fx)
    frac = off & np.int64(0xFFFFFFFF)
    return j + (off >> np.int64(32)), frac >> np.int64(24), (frac & np.int64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24


def model(x, lines, in_first=0, out_first=None, n_out=None, table=table_model, magnitude=False):
    """What Retimer.rows writes, with the blend and the sums in float64: [n_lines, n_out].  The inputs are rounded to float32
    first (the (float) cast of integer words); the table is the float32 array `table()` gives (`table_model`, or
    `retime.table` for the library's); D is the float32 difference of its rows; c = T[q] + mu * D[q] is not rounded.  Samples
    outside the rows are 0.  With `magnitude` the sum of |c[t] x| instead: what the rounding errors of a float evaluation
    scale with."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be 2-d")
    xf = x.astype(np.float32).astype(np.float64)
    T = np.asarray(table() if callable(table) else table, np.float32)
    D = (T[1:] - T[:-1]).astype(np.float64)            # float32 subtraction, then widened
    T = T.astype(np.float64)
    if magnitude:
        xf = np.abs(xf)
    n_in = x.shape[1]
    in_first = int(in_first)
    out_first = in_first if out_first is None else int(out_first)
    n_out = n_in if n_out is None else int(n_out)
    out = np.zeros((len(lines), n_out), np.float64)
    Tt, Dt = np.ascontiguousarray(T[:256].T), np.ascontiguousarray(D.T)      # [16, 256]: one coefficient of every row
    padded = np.zeros(n_in + 2 * COEFS, np.float64)                          # 16 zeros on either side of the row
    for r, (mic, delay, slope) in enumerate(lines):
        I, q, mu = positions(delay, slope, out_first, n_out)
        padded[COEFS:COEFS + n_in] = xf[int(mic)]
        # element of `padded` under c[0]; a window that lies wholly outside is moved onto the zeros next to the row
        base = np.clip(I - 7 - in_first + COEFS, 0, n_in + COEFS)
        for t in range(COEFS):
            c = np.take(Tt[t], q) + mu * np.take(Dt[t], q)
            out[r] += (np.abs(c) if magnitude else c) * np.take(padded, base + t)
    return out


# ---- estimating the lines of a recording: windows of the correlators, one straight line per microphone

NO_PEAK, AT_EDGE = 1, 2                                 # the flags of uchirp_align.h and uchirp_xcorr.h
WINDOW = 4 * 2048
HEIGHT_FLOOR = 0.5                                      # a window whose peak is below this part of the pair's best is mostly silent
RESIDUAL_MAX = 1.0                                      # samples: a whole carrier cycle is 4.46


def fit_line(centres, delays, usable):
    """The fit of `drift`: (D, s, kept) with delay(c) = D + s c over the usable windows.
    1. Theil-Sen: s0 = the median of (d_b - d_a) / (c_b - c_a) over all pairs a < b of usable windows, D0 = the median of
       d - s0 c.  Up to 29 % of the windows may lie anywhere (a neighbouring crest of the carrier, 4.46 samples off)
       without moving it far.
    2. Windows whose residual against (D0, s0) exceeds RESIDUAL_MAX = 1 sample are dropped.
    3. One least-squares line through the windows kept (centred abscissae, float64).
    Deterministic: medians and sums in the order of the windows.  ValueError with fewer than two windows kept."""
    c = np.asarray(centres, np.float64)
    d = np.asarray(delays, np.float64)
    use = np.asarray(usable, bool)
    idx = np.nonzero(use)[0]
    if len(idx) < 2:
        raise ValueError("fewer than two windows with a signal")
    a, b = np.triu_indices(len(idx), 1)
    s0 = float(np.median((d[idx[b]] - d[idx[a]]) / (c[idx[b]] - c[idx[a]])))
    d0 = float(np.median(d[idx] - s0 * c[idx]))
    kept = use & (np.abs(d - (d0 + s0 * c)) <= RESIDUAL_MAX)
    if kept.sum() < 2:
        raise ValueError("fewer than two windows agree with one line")
    cm = float(c[kept].mean())
    u = c[kept] - cm
    s = float(np.dot(u, d[kept]) / np.dot(u, u))
    return float(d[kept].mean()) - s * cm, s, kept


def _estimate(delays_of, arrays, first, count, window, max_lag):
    """one pass: [(D, s, fit)] per microphone of every array in turn (None for a reference)"""
    centres = first + window * np.arange(count, dtype=np.float64) + 0.5 * window
    per = [delays_of(first + w * window, window, max_lag) for w in range(count)]      # (delays, peaks) per window
    out = []
    for ai, a in enumerate(arrays):
        out.append(None)
        for mi in range(1, len(a)):
            d = np.array([per[w][0][ai][mi] for w in range(count)], np.float64)
            recs = [per[w][1][ai][mi] for w in range(count)]
            height = np.array([r["height"] for r in recs], np.float64)
            flags = np.array([r["flags"] for r in recs], np.int64)
            usable = ((flags & (NO_PEAK | AT_EDGE)) == 0) & (height >= HEIGHT_FLOOR * height.max()) & (height > 0.0)
            D, s, kept = fit_line(centres, d, usable)
            out.append((D, s, {"windows": count, "usable": int(usable.sum()), "kept": int(kept.sum()),
                               "residual": float(np.abs(d[kept] - (D + s * centres[kept])).max())}))
    return out


def _drift(delays_of, retimed, n_in, arrays, first, n, window, max_lag):
    arrays = [[int(m) for m in a] for a in arrays]
    if not arrays or any(len(a) < 2 for a in arrays):
        raise ValueError("every array needs a reference and at least one more microphone")
    first, window = int(first), int(window)
    n = n_in - first if n is None else int(n)
    count = n // window
    if count < 2:
        raise ValueError("drift needs at least two whole windows of %d samples" % window)
    rows = [m for a in arrays for m in a]
    coarse = _estimate(lambda f, w, L: delays_of(None, arrays, f, w, L), arrays, first, count, window, max_lag)
    lines = [(m, 0.0, 0.0) if c is None else (m, c[0], c[1]) for m, c in zip(rows, coarse)]
    # second pass on the rows retimed by the first one: row i of the retimed buffer is rows[i]
    again, at = [], 0
    for a in arrays:
        again.append(list(range(at, at + len(a))))
        at += len(a)
    y = retimed(lines)
    fine = _estimate(lambda f, w, L: delays_of(y, again, f, w, L), again, first, count, window, max_lag)
    out, fits = [], []
    for (m, d1, s1), f in zip(lines, fine):
        if f is None:
            out.append((m, 0.0, 0.0))
            fits.append(None)
        else:
            d2, s2, fit = f
            out.append((m, d1 + d2 * (1.0 + s1), s1 + s2 * (1.0 + s1)))
            fits.append(dict(fit, correction=(d2, s2)))
    return out, fits


def drift(x, arrays, estimator, first=0, n=None, window=WINDOW, max_lag=64, retimer=None, stream=None):
    """Lines for `Retimer.rows` from a recording: every array's microphones onto the clock of its reference (the array's
    first row).  `estimator` is an `Aligner` (uchirp.align, max_lag <= 64) or an `Xcorr` (uchirp.xcorr, <= 512); `retimer`
    a `Retimer` (one is made and closed if None).

    One pass: `estimator.delays` is called once per whole window of `window` samples in [first, first + n) (a rest shorter
    than a window is left out; the default is 4 blocks of 2048), which gives every microphone's delay against the reference
    at the window's centre c = start + window / 2.  Per microphone the windows without a signal are set aside -- those whose
    peak record carries NO_PEAK or AT_EDGE, and those whose height is below HEIGHT_FLOOR = 0.5 of the tallest window of that
    pair: silent ones, and ones the message fills less than about half -- and `fit_line` puts one straight line
    delay(c) = D + s c through the rest: a Theil-Sen line first, windows more than 1 sample off it dropped (a neighbouring
    crest of the carrier is 4.46 samples off), then one least-squares line.

    Two passes.  A window's correlation gives the delay at the centre of the SIGNAL in it, and over a window the delay
    moves (0.8 samples at 100 ppm between two microphones).  Where the message fills a window the two centres agree and the
    smear is symmetric; in the windows where the message starts and ends they do not, by up to a quarter of a window, which
    pulls the ends of the line together: a few per cent of the slope (4 ppm of 100 in a message of 13 windows; with windows
    of 16 blocks, which such a message fills only two or three of, 6 ppm were measured).  So the rows are retimed by the first
    pass's lines (D1, s1) and estimated once more, in the same windows: what is left, (D2, s2), is a fraction of a sample
    and a few ppm, the same few per cent of THAT is below 0.2 ppm, and the two lines compose exactly: the row is read at
    p = j' + D1 + s1 j' with j' = j + D2 + s2 j, so
        D = D1 + D2 (1 + s1),  s = s1 + s2 (1 + s1).
    max_lag must cover the largest |D + s j| over the record.

    Returns (lines, fits): `lines` in the order of the arrays' rows, [(row, D, s)] with (row, 0.0, 0.0) for a reference;
    `fits` the matching list of the second pass's {windows, usable, kept, residual, correction} (None for a reference).  A row
    retimed by its line lies on the reference's sample axis; it has not been steered further."""
    own = retimer is None
    if own:
        retimer = Retimer(x.device.index or 0)
    try:
        return _drift(lambda y, arr, f, w, L: estimator.delays(x if y is None else y, arr, first=f, n=w, max_lag=L, stream=stream),
                      lambda lines: retimer.rows(x, lines, stream=stream), int(x.shape[1]), arrays, first, n, window, max_lag)
    finally:
        if own:
            retimer.close()


def drift_model(x, arrays, first=0, n=None, window=WINDOW, max_lag=64, table=table_model, threads=8):
    """`drift` over `align.delays_model` and `model`: float64 on the host (the retimed rows are rounded to float32, as the
    device holds them; they are computed row by row on `threads` threads)."""
    from concurrent.futures import ThreadPoolExecutor
    from . import align
    x = np.asarray(x)
    tab = table() if callable(table) else table

    def retimed(lines):
        def one(ln):
            return x[ln[0]].astype(np.float32) if ln[1] == 0.0 and ln[2] == 0.0 else model(x, [ln], table=tab)[0].astype(np.float32)
        with ThreadPoolExecutor(int(threads)) as ex:
            return np.stack(list(ex.map(one, lines)))

    return _drift(lambda y, arr, f, w, L: align.delays_model(x if y is None else y, arr, first=f, n=w, max_lag=L), retimed,
                  int(x.shape[1]), arrays, first, n, window, max_lag)
