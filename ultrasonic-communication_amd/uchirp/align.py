"""uchirp.align -- the delay estimator: binding of libuchirp_align.so (include/uchirp_align.h) and its float64 model.

`Array.combine` (uchirp.array) needs every microphone's fractional delay.  For a buffer `Scene.render` made they come from
the scene; a recording has none.  `Aligner.correlate` cross-correlates pairs of rows over the lags -L .. L in one pass on
the GPU, `peak` (the library's host function) reads the fractional delay off one correlation, `Aligner.delays` does both
for a list of arrays and `steer` turns the result into the beams `Array.combine` takes.  There is no CPU path behind
`Aligner`; `peak`, `peak_model` and `model` need no GPU.

Arrays are written as
    arrays = [[row, row, ...], ...]          the rows of x that make one array, the first one the reference
and a delay is the number of samples by which a microphone hears the sound LATER than its array's reference.
"""
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_LAG = 64
SEGMENT = 4096
ROUNDINGS = 70
NO_PEAK, AT_EDGE = 1, 2
EXPORTS = ["uc_align_abi_version", "uc_align_last_error", "uc_align_create", "uc_align_destroy", "uc_align_correlate",
           "uc_align_peak"]


class AlignPair(C.Structure):
    """struct uc_align_pair (include/uchirp_align.h)."""
    _fields_ = [("ref", C.c_uint32), ("mic", C.c_uint32)]


class AlignPeak(C.Structure):
    """struct uc_align_peak_t (include/uchirp_align.h)."""
    _fields_ = [("delay_samples", C.c_double), ("height", C.c_double), ("runner_up", C.c_double), ("lag", C.c_int32),
                ("flags", C.c_uint32)]


PAIR_DTYPE = np.dtype([("ref", "<u4"), ("mic", "<u4")])


class AlignError(RuntimeError):
    pass


def _declare(L):
    L.uc_align_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_align_correlate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.uc_align_peak.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(AlignPeak)]


_so = Binding("align", AlignError, _declare, env="UCHIRP_ALIGN_LIB")  # UCHIRP_ALIGN_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def _record(delay, height, runner_up, lag, flags):
    return {"delay_samples": float(delay), "height": float(height), "runner_up": float(runner_up), "lag": int(lag), "flags": int(flags)}


def peak(row):
    """uc_align_peak: the record {delay_samples, height, runner_up, lag, flags} of one correlation row of 2 L + 1 values,
    computed by the library on the host (no GPU)."""
    r = np.ascontiguousarray(row, np.float64)
    if r.ndim != 1 or len(r) < 3 or len(r) % 2 == 0:
        raise ValueError("a correlation row has 2 L + 1 values")
    out = AlignPeak()
    _check(lib().uc_align_peak(r.ctypes.data_as(C.c_void_p), (len(r) - 1) // 2, C.byref(out)), "uc_align_peak")
    return _record(out.delay_samples, out.height, out.runner_up, out.lag, out.flags)


def peak_model(row, lag_limit=MAX_LAG):
    """The peak rule of include/uchirp_align.h in numpy / float64: the same record as `peak` (`lag_limit`: the greatest L
    the library behind `peak` takes; uchirp.xcorr's is 512)."""
    r = np.asarray(row, np.float64)
    if r.ndim != 1 or len(r) < 3 or len(r) % 2 == 0:
        raise ValueError("a correlation row has 2 L + 1 values")
    L = (len(r) - 1) // 2
    if not 1 <= L <= lag_limit or not np.isfinite(r).all():
        raise ValueError("L must be 1 .. %d and every value finite" % lag_limit)
    flags = AT_EDGE if int(np.argmax(r)) in (0, 2 * L) else 0
    heights = []
    for k in range(1, 2 * L):
        if r[k] > 0.0 and r[k] >= r[k - 1] and r[k] > r[k + 1]:
            c = (r[k - 1] + r[k + 1]) / (2.0 * r[k])
            if -1.0 < c < 1.0:
                w = np.arccos(c)
                q = (r[k + 1] - r[k - 1]) / (2.0 * np.sin(w))
                heights.append((float(np.hypot(r[k], q)), k, float(np.arctan2(q, r[k]) / w)))
            else:
                heights.append((float(r[k]), k, 0.0))
    if not heights:
        return _record(0.0, 0.0, 0.0, 0, flags | NO_PEAK)
    best = max(range(len(heights)), key=lambda i: (heights[i][0], -i))        # the first one on a tie
    h, k, d = heights[best]
    others = [heights[i][0] for i in range(len(heights)) if i != best]
    return _record(k - L + d, h, max(others) / h if others else 0.0, k - L, flags)


def _pairs(pairs):
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(p) == 0 or p.min() < 0 or p.max() > 0xFFFFFFFF:
        raise ValueError("pairs: a non-empty list of (ref, mic) rows")
    out = np.zeros(len(p), PAIR_DTYPE)
    out["ref"], out["mic"] = p[:, 0], p[:, 1]
    return out


def model(x, pairs, first=0, n=None, max_lag=48, magnitude=False):
    """What Aligner.correlate writes, with every sum in float64: [n_pairs, 2 L + 1].  The inputs are rounded to float32
    first (the (float) cast of integer words); samples of the microphone row outside it are 0.  With `magnitude` the sum
    of |x_ref[j] x_mic[j + l]| instead: what the rounding errors of a float evaluation scale with."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be 2-d")
    xf = x.astype(np.float32).astype(np.float64)
    if magnitude:
        xf = np.abs(xf)
    n_in = x.shape[1]
    first = int(first)
    n = n_in - first if n is None else int(n)
    L = int(max_lag)
    if not (1 <= L <= MAX_LAG and n >= 1 and first >= 0 and first + n <= n_in):
        raise ValueError("first, n or max_lag out of range")
    p = _pairs(pairs)
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    padded = np.zeros(n + 2 * L, np.float64)
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        padded[:] = 0.0
        lo, hi = max(first - L, 0), min(first + n + L, n_in)
        padded[lo - (first - L):hi - (first - L)] = xf[mic, lo:hi]
        a = xf[ref, first:first + n]
        for k in range(2 * L + 1):
            out[i, k] = np.dot(a, padded[k:k + n])
    return out


def _arrays(arrays):
    arrays = [[int(m) for m in a] for a in arrays]
    if not arrays or any(len(a) < 2 for a in arrays):
        raise ValueError("every array needs a reference and at least one more microphone")
    return arrays, [(a[0], m) for a in arrays for m in a[1:]]


class Aligner:
    """One uc_align: the correlator on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_align_create(int(device), C.byref(h)), "uc_align_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_align_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def correlate(self, x, pairs, first=0, n=None, max_lag=48, out=None, stream=None):
        """uc_align_correlate: r[p, l + L] = sum over j in [first, first + n) of x[ref_p, j] x[mic_p, j + l] -> a float64
        torch tensor [n_pairs, 2 L + 1] on the object's device (or into `out`: a 2-d device tensor with contiguous rows).
        `x`: a 2-d float32 / int32 device tensor with contiguous rows; `pairs`: (ref, mic) rows, a list or a PAIR_DTYPE
        array; n defaults to the rest of the row.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nm, n_in = int(x.shape[0]), int(x.shape[1])
        p = pairs if isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE else _pairs(pairs)
        p = np.ascontiguousarray(p)
        first, L = int(first), int(max_lag)
        n = n_in - first if n is None else int(n)
        if first < 0 or n < 0 or L < 0:
            raise ValueError("first, n and max_lag must not be negative")
        lags = 2 * L + 1
        if out is None:
            out = torch.empty((len(p), lags), dtype=torch.float64, device=dev)
        elif (out.dim() != 2 or out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (len(p), lags) or
              out.stride(1) != 1 or (len(p) > 1 and out.stride(0) < lags)):
            raise ValueError("out must be a [%d, %d] float64 tensor on %s with contiguous rows" % (len(p), lags, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_align_correlate(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm, n_in,
                                        int(x.stride(0)) if nm > 1 else n_in, p.ctypes.data_as(C.c_void_p), len(p), first, n, L,
                                        C.c_void_p(out.data_ptr()), int(out.stride(0)) if len(p) > 1 else lags,
                                        C.c_void_p(stream) if stream else None), "uc_align_correlate")
        return out

    def delays(self, x, arrays, first=0, n=None, max_lag=48, stream=None):
        """The delays of every array's microphones against its reference (the array's first row): one `correlate` call
        over all pairs, one copy to the host, one `peak` call per pair.  Returns (delays, peaks): per array the list of
        delays in samples (0.0 for the reference) and the list of peak records (None for the reference)."""
        arrays, pairs = _arrays(arrays)
        rows = self.correlate(x, pairs, first=first, n=n, max_lag=max_lag, stream=stream).cpu().numpy()
        return _split(arrays, [peak(r) for r in rows])


def _split(arrays, records):
    delays, peaks, at = [], [], 0
    for a in arrays:
        recs = records[at:at + len(a) - 1]
        at += len(a) - 1
        delays.append([0.0] + [r["delay_samples"] for r in recs])
        peaks.append([None] + recs)
    return delays, peaks


def delays_model(x, arrays, first=0, n=None, max_lag=48, model=model, peak_model=peak_model):
    """`Aligner.delays` through `model` and `peak_model`: float64 on the host."""
    arrays, pairs = _arrays(arrays)
    return _split(arrays, [peak_model(r) for r in model(x, pairs, first, n, max_lag)])


def steer(x, arrays, aligner=None, first=0, n=None, max_lag=48, stream=None):
    """Delay-and-sum beams for `Array.combine`, one per array, steered by the ESTIMATED delays: `array.steer` of every
    array's delays (its reference is the smallest delay, so that none is negative), with the array's rows of x as the
    microphones.  Returns (beams, delays, peaks)."""
    from . import array
    own = aligner is None
    if own:
        aligner = Aligner(x.device.index or 0)
    try:
        delays, peaks = aligner.delays(x, arrays, first=first, n=n, max_lag=max_lag, stream=stream)
    finally:
        if own:
            aligner.close()
    beams = [[(int(a[m]), w, d) for (m, w, d) in array.steer(dl)] for a, dl in zip(arrays, delays)]
    return beams, delays, peaks
