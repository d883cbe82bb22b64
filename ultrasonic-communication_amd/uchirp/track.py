"""uchirp.track -- the delay tracker: binding of libuchirp_track.so (include/uchirp_track.h), the float64 models of its
windows, its crest selection and its finishing rule, and `drift`, which estimates the lines of `retime.drift` with one
tracker call per pass.

`Xcorr.delays` gives one delay per pair and call.  `Tracker.windows` computes the same correlations for a series of windows
of one recording in ONE call and leaves a crest record of 136 bytes per (pair, window) on the device: the four candidates
of greatest selection height with their three samples each.  `finish` (the library's host function: the loop body of
uc_xcorr_peak over those candidates) turns a record into the peak record `xcorr.peak` gives for the whole correlation.
There is no CPU path behind `Tracker`; `finish`, `finish_model`, `select_model` and `windows_model` need no GPU.

Arrays are written as in uchirp.xcorr: [[row, row, ...], ...], the first row of an array its reference.
"""
import ctypes as C

import numpy as np

from . import retime, xcorr
from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_LAG = 512
POINTS = 2048
GROUP = 4
SLOTS = 4
ERROR_C = xcorr.ERROR_C                      # the arithmetic is that of uc_xcorr_correlate
NO_PEAK, AT_EDGE, NOT_FINITE = 1, 2, 4
EXPORTS = ["uc_track_abi_version", "uc_track_last_error", "uc_track_create", "uc_track_destroy", "uc_track_windows",
           "uc_track_finish"]


class TrackPair(C.Structure):
    """struct uc_track_pair (include/uchirp_track.h)."""
    _fields_ = [("ref", C.c_uint32), ("mic", C.c_uint32)]


class TrackSlot(C.Structure):
    """struct uc_track_slot (include/uchirp_track.h)."""
    _fields_ = [("k", C.c_int32), ("reserved", C.c_int32), ("r", C.c_double * 3)]


class TrackCrest(C.Structure):
    """struct uc_track_crest (include/uchirp_track.h)."""
    _fields_ = [("flags", C.c_uint32), ("n_candidates", C.c_uint32), ("slot", TrackSlot * SLOTS)]


class TrackPeak(C.Structure):
    """struct uc_track_peak_t (include/uchirp_track.h)."""
    _fields_ = [("delay_samples", C.c_double), ("height", C.c_double), ("runner_up", C.c_double), ("lag", C.c_int32),
                ("flags", C.c_uint32)]


PAIR_DTYPE = np.dtype([("ref", "<u4"), ("mic", "<u4")])
SLOT_DTYPE = np.dtype([("k", "<i4"), ("reserved", "<i4"), ("r", "<f8", (3,))])
CREST_DTYPE = np.dtype([("flags", "<u4"), ("n_candidates", "<u4"), ("slot", SLOT_DTYPE, (SLOTS,))])
PEAK_DTYPE = np.dtype([("delay_samples", "<f8"), ("height", "<f8"), ("runner_up", "<f8"), ("lag", "<i4"), ("flags", "<u4")])
CREST_BYTES = CREST_DTYPE.itemsize           # 136


class TrackError(RuntimeError):
    pass


def _declare(L):
    L.uc_track_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_track_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.c_void_p]
    L.uc_track_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]


_so = Binding("track", TrackError, _declare, env="UCHIRP_TRACK_LIB")  # UCHIRP_TRACK_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def _record(p):
    return xcorr._record(p["delay_samples"], p["height"], p["runner_up"], p["lag"], p["flags"])


def finish(crest, max_lag):
    """uc_track_finish over an array of crest records (CREST_DTYPE, any shape), computed by the library on the host (no
    GPU): PEAK_DTYPE records of the same shape."""
    c = np.ascontiguousarray(crest, CREST_DTYPE)
    out = np.zeros(c.shape, PEAK_DTYPE)
    fn, L = lib().uc_track_finish, int(max_lag)
    src, dst = c.ctypes.data, out.ctypes.data
    for i in range(c.size):
        rc = fn(src + i * CREST_BYTES, L, dst + i * PEAK_DTYPE.itemsize)
        if rc < 0:
            _check(rc, "uc_track_finish")
    return out


def _fit(lo, mid, hi):
    """(height, d) of one candidate: the loop body of uc_xcorr_peak as `xcorr.peak_model` writes it"""
    c = (lo + hi) / (2.0 * mid)
    if -1.0 < c < 1.0:
        w = np.arccos(c)
        q = (hi - lo) / (2.0 * np.sin(w))
        return float(np.hypot(mid, q)), float(np.arctan2(q, mid) / w)
    return float(mid), 0.0


def finish_model(crest, max_lag):
    """The finishing rule of include/uchirp_track.h in numpy / float64: the same records as `finish`."""
    c = np.ascontiguousarray(crest, CREST_DTYPE)
    L = int(max_lag)
    if not 1 <= L <= MAX_LAG:
        raise ValueError("L must be 1 .. %d" % MAX_LAG)
    out = np.zeros(c.shape, PEAK_DTYPE)
    flat, oflat = c.reshape(-1), out.reshape(-1)
    for i, rec in enumerate(flat):
        if rec["flags"] & NOT_FINITE:
            raise ValueError("the correlation held a value that is not finite")
        flags = int(rec["flags"]) & AT_EDGE
        best = None
        second = 0.0
        for s in rec["slot"]:
            k = int(s["k"])
            if k < 0:
                continue
            if not 1 <= k < 2 * L:
                raise ValueError("slot k %d not in 1 .. %d" % (k, 2 * L - 1))
            h, d = _fit(*[np.float64(v) for v in s["r"]])
            if best is None or h > best[0]:
                if best is not None:
                    second = best[0]
                best = (h, k, d)
            elif h > second:
                second = h
        if best is None:
            oflat[i] = (0.0, 0.0, 0.0, 0, flags | NO_PEAK)
        else:
            h, k, d = best
            oflat[i] = (k - L + d, h, second / h, k - L, flags)
    return out


def _candidates(r):
    """(ks, lo, mid, hi) of the candidates of a finite row"""
    lo, mid, hi = r[:-2], r[1:-1], r[2:]
    at = np.nonzero((mid > 0.0) & (mid >= lo) & (mid > hi))[0]
    return at + 1, lo[at], mid[at], hi[at]


def select_model(row):
    """The crest record of include/uchirp_track.h of one correlation row of 2 L + 1 doubles, in numpy float64 operation for
    operation (every numpy operation below is one correctly rounded IEEE operation per element): a CREST_DTYPE scalar."""
    r = np.asarray(row, np.float64)
    if r.ndim != 1 or len(r) < 3 or len(r) % 2 == 0:
        raise ValueError("a correlation row has 2 L + 1 values")
    last = len(r) - 1
    out = np.zeros((), CREST_DTYPE)
    if not np.isfinite(r).all():
        out["flags"] = NOT_FINITE
        return out
    out["slot"]["k"] = -1
    flags = AT_EDGE if int(np.argmax(r)) in (0, last) else 0
    ks, lo, mid, hi = _candidates(r)
    with np.errstate(all="ignore"):
        c = (lo + hi) / (2.0 * mid)
        inside = (c > -1.0) & (c < 1.0)
        s = np.sqrt((1.0 - c) * (1.0 + c))
        q = (hi - lo) / (2.0 * s)
        h2 = np.where(inside, mid * mid + q * q, mid * mid)
    keep = np.sort(ks[np.lexsort((ks, -h2))[:SLOTS]])           # the greater h2, the smaller k on equal h2; then ascending k
    for i, k in enumerate(keep):
        out["slot"][i]["k"] = k
        out["slot"][i]["r"] = r[k - 1:k + 2]
    out["flags"] = flags | (0 if len(ks) else NO_PEAK)
    out["n_candidates"] = len(ks)
    return out


def excluded(row, crest):
    """The stated exception of the header: True if fewer than two of uc_xcorr_peak's top two candidates of `row` (its best,
    and the best of the others; one if there is only one) are among the record's slots."""
    r = np.asarray(row, np.float64)
    ks, lo, mid, hi = _candidates(r)
    if not len(ks):
        return False
    with np.errstate(all="ignore"):
        c = (lo + hi) / (2.0 * mid)
        w = np.arccos(np.clip(c, -1.0, 1.0))
        height = np.where((c > -1.0) & (c < 1.0), np.hypot(mid, (hi - lo) / (2.0 * np.sin(w))), mid)
    top = ks[np.lexsort((ks, -height))[:2]]
    kept = set(int(k) for k in np.asarray(crest)["slot"]["k"] if k >= 0)
    return not set(int(k) for k in top) <= kept


def _windows(n_in, first, window_len, hop, n_windows):
    first, window_len = int(first), int(window_len)
    hop = window_len if hop is None else int(hop)
    if first < 0 or window_len < 1 or hop < 1 or first + window_len > n_in:
        raise ValueError("first, window_len or hop out of range")
    n_windows = (n_in - first - window_len) // hop + 1 if n_windows is None else int(n_windows)
    if n_windows < 1 or first + (n_windows - 1) * hop + window_len > n_in:
        raise ValueError("a window past the rows")
    return first, window_len, hop, n_windows


def windows_model(x, pairs, first=0, window_len=None, hop=None, n_windows=None, max_lag=512, magnitude=False):
    """What Tracker.windows stores as correlations, in float64: `xcorr.model` per window, [n_pairs, n_windows, 2 L + 1]
    (with `magnitude` E_p per window instead, [n_pairs, n_windows])."""
    x = np.asarray(x)
    first, window_len, hop, n_windows = _windows(x.shape[1], first, x.shape[1] - int(first) if window_len is None else window_len, hop, n_windows)
    per = [xcorr.model(x, pairs, first + w * hop, window_len, max_lag, magnitude=magnitude) for w in range(n_windows)]
    return np.stack(per, axis=1)


def _split(arrays, peaks):
    """(delays[array][mic][window], peaks[array][mic][window]) of PEAK_DTYPE records [pair][window]; the reference of an
    array has delays of 0.0 and None for its records"""
    nw = peaks.shape[1]
    delays, recs, at = [], [], 0
    for a in arrays:
        rows = peaks[at:at + len(a) - 1]
        at += len(a) - 1
        delays.append([[0.0] * nw] + [[float(v) for v in row["delay_samples"]] for row in rows])
        recs.append([None] + [[_record(p) for p in row] for row in rows])
    return delays, recs


class Tracker:
    """One uc_track: the delay tracker on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_track_create(int(device), C.byref(h)), "uc_track_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_track_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def windows(self, x, pairs, first=0, window_len=None, hop=None, n_windows=None, max_lag=512, corr=False, crest=True,
                stream=None):
        """uc_track_windows: the crest records of every (pair, window) as a uint8 torch tensor [n_pairs, n_windows, 136] on
        the object's device (`crests` reads it as CREST_DTYPE), and with `corr` the correlations too, as a float64 tensor
        [n_pairs, n_windows, 2 L + 1]: returns crest, or (crest, corr).  `corr` may be True or a float64 device tensor of
        that shape with contiguous rows to write into; with crest=False only the correlations are produced and returned.
        `x`: a 2-d float32 / int32 device tensor with contiguous rows; `pairs`: (ref, mic) rows, a list or a PAIR_DTYPE
        array.  window_len defaults to the rest of the row, hop to window_len, n_windows to as many as fit.  Asynchronous
        on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nm, n_in = int(x.shape[0]), int(x.shape[1])
        p = pairs if isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE else xcorr._pairs(pairs)
        p = np.ascontiguousarray(p)
        L = int(max_lag)
        if L < 0:
            raise ValueError("max_lag must not be negative")
        first, window_len, hop, n_windows = _windows(n_in, first, n_in - int(first) if window_len is None else window_len, hop, n_windows)
        lags = 2 * L + 1
        rows = len(p) * n_windows
        out = None
        if corr is True:
            out = torch.empty((len(p), n_windows, lags), dtype=torch.float64, device=dev)
        elif corr is not False and corr is not None:
            out = corr
            if (out.dim() != 3 or out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (len(p), n_windows, lags) or
                    out.stride(2) != 1 or (n_windows > 1 and out.stride(1) < lags) or
                    (len(p) > 1 and (out.stride(0) != n_windows * out.stride(1) if n_windows > 1 else out.stride(0) < lags))):
                raise ValueError("corr must be a [%d, %d, %d] float64 tensor on %s with evenly spaced contiguous rows" % (len(p), n_windows, lags, dev))
        if out is None and not crest:
            raise ValueError("nothing to produce: neither crests nor correlations")
        cr = torch.empty((len(p), n_windows, CREST_BYTES), dtype=torch.uint8, device=dev) if crest else None
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        cstride = lags if out is None or rows == 1 else int(out.stride(1) if n_windows > 1 else out.stride(0))
        _check(lib().uc_track_windows(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm, n_in,
                                      int(x.stride(0)) if nm > 1 else n_in, p.ctypes.data_as(C.c_void_p), len(p), first, window_len, hop,
                                      n_windows, L, C.c_void_p(out.data_ptr()) if out is not None else None, cstride,
                                      C.c_void_p(cr.data_ptr()) if cr is not None else None, C.c_void_p(stream) if stream else None),
               "uc_track_windows")
        if out is None:
            return cr
        return (cr, out) if crest else out

    def peaks(self, x, pairs, first=0, window_len=None, hop=None, n_windows=None, max_lag=512, stream=None):
        """One `windows` call, one copy of the crest records to the host, `finish`: PEAK_DTYPE records [pair][window]."""
        return finish(crests(self.windows(x, pairs, first, window_len, hop, n_windows, max_lag, stream=stream)), max_lag)

    def delays(self, x, arrays, first=0, window_len=None, hop=None, n_windows=None, max_lag=512, stream=None):
        """The delays of every array's microphones against its reference (the array's first row) in every window: one
        `peaks` call over all pairs.  Returns (delays, peaks): delays[array][mic][window] in samples (0.0 for the
        reference) and peaks[array][mic][window], the records `xcorr.peak` gives (None in place of a reference's list)."""
        arrays, pairs = xcorr._arrays(arrays)
        return _split(arrays, self.peaks(x, pairs, first, window_len, hop, n_windows, max_lag, stream=stream))


def crests(t):
    """The crest tensor of `Tracker.windows` on the host: CREST_DTYPE [n_pairs, n_windows] (synchronises)."""
    a = t.cpu().numpy()
    return np.ascontiguousarray(a).view(CREST_DTYPE).reshape(a.shape[:-1])


class _Served:
    """What `retime._drift` calls once per window, answered from ONE `delays` call per recording: the windows of a pass
    are asked in turn for the same buffer, so the first question of a pass computes them all."""

    def __init__(self, x, tracker, first, count, window, stream):
        self.x, self.tracker, self.first, self.count, self.window, self.stream = x, tracker, first, count, window, stream
        self.key = self.held = None

    def __call__(self, y, arrays, f, w, L):
        key = (id(y), L, tuple(tuple(int(m) for m in a) for a in arrays))
        if self.held is None or self.key != key:
            self.held = self.tracker.delays(self.x if y is None else y, arrays, first=self.first, window_len=self.window,
                                            hop=self.window, n_windows=self.count, max_lag=L, stream=self.stream)
            self.key, self.y = key, y          # (y is kept so that its id stays its own)
        if w != self.window or (f - self.first) % self.window:
            raise ValueError("a window that the call did not cover")
        i = (f - self.first) // self.window
        delays, peaks = self.held
        return ([[d[i] for d in a] for a in delays], [[None if r is None else r[i] for r in a] for a in peaks])


def drift(x, arrays, tracker, first=0, n=None, window=retime.WINDOW, max_lag=64, retimer=None, stream=None):
    """`retime.drift` -- its windows, its two passes, its fit -- with ONE `Tracker.delays` call per pass in place of one
    estimator call per window: `retime._drift` is handed an adapter that serves window after window from that call's
    result.  The peak records are the bits `Xcorr.delays` gives and `retime.fit_line` is the same code, so the lines
    returned equal those of `retime.drift(x, arrays, Xcorr(...), ...)` exactly.  Returns (lines, fits) as that function."""
    n_in = int(x.shape[1])
    first, window = int(first), int(window)
    count = ((n_in - first) if n is None else int(n)) // window
    if count < 2:
        raise ValueError("drift needs at least two whole windows of %d samples" % window)
    own = retimer is None
    if own:
        retimer = retime.Retimer(x.device.index or 0)
    try:
        return retime._drift(_Served(x, tracker, first, count, window, stream), lambda lines: retimer.rows(x, lines, stream=stream),
                             n_in, arrays, first, n, window, max_lag)
    finally:
        if own:
            retimer.close()
