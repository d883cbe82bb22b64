"""uchirp.xcorr -- the wide-lag correlator: binding of libuchirp_xcorr.so (include/uchirp_xcorr.h), its float64 model and an
independent float32 evaluation of the same definition.

`align.Aligner` evaluates lags directly and stops at +-64 samples.  `Xcorr.correlate` computes the same sums
r[p, l + L] = sum_j x[ref_p, j] x[mic_p, j + l] out to L = 512 by overlap-save on 2048-point transforms on the GPU; `peak`
(the library's host function: the crest rule of uchirp_align.h) reads the fractional delay off one correlation,
`Xcorr.delays` does both for a list of arrays and `steer` turns the result into the beams `Array.combine` takes.  There is
no CPU path behind `Xcorr`; `peak`, `peak_model`, `model` and `emulate32` need no GPU.

Arrays are written as
    arrays = [[row, row, ...], ...]          the rows of x that make one array, the first one the reference
and a delay is the number of samples by which a microphone hears the sound LATER than its array's reference.
"""
import ctypes as C

import numpy as np

from . import align
from ._binding import Binding
from .align import PAIR_DTYPE, _arrays, _pairs, _record, _split  # noqa: F401  (one layout of pairs, one shape of records)

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_LAG = 512
POINTS = 2048
GROUP = 4
ERROR_C = 11
NO_PEAK, AT_EDGE = 1, 2
EXPORTS = ["uc_xcorr_abi_version", "uc_xcorr_last_error", "uc_xcorr_create", "uc_xcorr_destroy", "uc_xcorr_correlate",
           "uc_xcorr_peak"]


class XcorrPair(C.Structure):
    """struct uc_xcorr_pair (include/uchirp_xcorr.h)."""
    _fields_ = [("ref", C.c_uint32), ("mic", C.c_uint32)]


class XcorrPeak(C.Structure):
    """struct uc_xcorr_peak_t (include/uchirp_xcorr.h)."""
    _fields_ = [("delay_samples", C.c_double), ("height", C.c_double), ("runner_up", C.c_double), ("lag", C.c_int32),
                ("flags", C.c_uint32)]


class XcorrError(RuntimeError):
    pass


def _declare(L):
    L.uc_xcorr_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_xcorr_correlate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.uc_xcorr_peak.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(XcorrPeak)]


_so = Binding("xcorr", XcorrError, _declare, env="UCHIRP_XCORR_LIB")  # UCHIRP_XCORR_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def peak(row):
    """uc_xcorr_peak: the record {delay_samples, height, runner_up, lag, flags} of one correlation row of 2 L + 1 values,
    computed by the library on the host (no GPU)."""
    r = np.ascontiguousarray(row, np.float64)
    if r.ndim != 1 or len(r) < 3 or len(r) % 2 == 0:
        raise ValueError("a correlation row has 2 L + 1 values")
    out = XcorrPeak()
    _check(lib().uc_xcorr_peak(r.ctypes.data_as(C.c_void_p), (len(r) - 1) // 2, C.byref(out)), "uc_xcorr_peak")
    return _record(out.delay_samples, out.height, out.runner_up, out.lag, out.flags)


def peak_model(row):
    """The peak rule of include/uchirp_xcorr.h (that of uchirp_align.h) in numpy / float64: the same record as `peak`."""
    return align.peak_model(row, MAX_LAG)


def _rows(x, first, n, max_lag):
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be 2-d")
    n_in = x.shape[1]
    first = int(first)
    n = n_in - first if n is None else int(n)
    L = int(max_lag)
    if not (1 <= L <= MAX_LAG and n >= 1 and first >= 0 and first + n <= n_in):
        raise ValueError("first, n or max_lag out of range")
    return x.astype(np.float32), n_in, first, n, L


def _window(row, start, count):
    """row[start : start + count] with zeros where the row has no sample"""
    out = np.zeros(count, row.dtype)
    lo, hi = max(start, 0), min(start + count, len(row))
    if hi > lo:
        out[lo - start:hi - start] = row[lo:hi]
    return out


def segments(first, n, max_lag):
    """The segments of the definition: [(s S, cnt)], S = POINTS - 2 L."""
    S = POINTS - 2 * int(max_lag)
    return [(i0, min(S, n - i0)) for i0 in range(0, n, S)]


def model(x, pairs, first=0, n=None, max_lag=512, magnitude=False):
    """What Xcorr.correlate writes, with every sum in float64 and by plain dot products: [n_pairs, 2 L + 1].  The inputs
    are rounded to float32 first (the (float) cast of integer words); samples of the microphone row outside it are 0.
    With `magnitude` E_p = sum over the segments of ||a_s|| ||b_s|| instead, [n_pairs]: what the header's error form
    scales with."""
    x32, n_in, first, n, L = _rows(x, first, n, max_lag)
    xf = x32.astype(np.float64)
    p = _pairs(pairs)
    if magnitude:
        E = np.zeros(len(p), np.float64)
        for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
            for i0, cnt in segments(first, n, L):
                a = xf[ref, first + i0:first + i0 + cnt]
                b = _window(xf[mic], first + i0 - L, cnt + 2 * L)
                E[i] += np.sqrt(np.dot(a, a)) * np.sqrt(np.dot(b, b))
        return E
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        padded = _window(xf[mic], first - L, n + 2 * L)
        a = xf[ref, first:first + n]
        for k in range(2 * L + 1):
            out[i, k] = np.dot(a, padded[k:k + n])
    return out


def emulate32(x, pairs, first=0, n=None, max_lag=512):
    """The definition's structure -- segments of S = P - 2 L samples, groups of G cross-spectra added in float, one inverse
    transform per group, the unit sums added in double -- with scipy.fft (pocketfft) in single precision: an independent
    float32 evaluation, there only so that tests have a yardstick for what float32 can do."""
    import scipy.fft
    x32, n_in, first, n, L = _rows(x, first, n, max_lag)
    p = _pairs(pairs)
    segs = segments(first, n, L)
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        for g0 in range(0, len(segs), GROUP):
            acc = np.zeros(POINTS // 2 + 1, np.complex64)
            for i0, cnt in segs[g0:g0 + GROUP]:
                a = _window(x32[ref, first + i0:first + i0 + cnt], 0, POINTS)
                b = _window(_window(x32[mic], first + i0 - L, cnt + 2 * L), 0, POINTS)
                A, B = scipy.fft.rfft(a), scipy.fft.rfft(b)
                assert A.dtype == np.complex64
                acc = acc + np.conj(A) * B
            unit = scipy.fft.irfft(acc, POINTS)
            assert unit.dtype == np.float32
            out[i] += unit[:2 * L + 1].astype(np.float64)
    return out


class Xcorr:
    """One uc_xcorr: the wide-lag correlator on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_xcorr_create(int(device), C.byref(h)), "uc_xcorr_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_xcorr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def correlate(self, x, pairs, first=0, n=None, max_lag=512, out=None, stream=None):
        """uc_xcorr_correlate: r[p, l + L] = sum over j in [first, first + n) of x[ref_p, j] x[mic_p, j + l] -> a float64
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
        _check(lib().uc_xcorr_correlate(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm, n_in,
                                        int(x.stride(0)) if nm > 1 else n_in, p.ctypes.data_as(C.c_void_p), len(p), first, n, L,
                                        C.c_void_p(out.data_ptr()), int(out.stride(0)) if len(p) > 1 else lags,
                                        C.c_void_p(stream) if stream else None), "uc_xcorr_correlate")
        return out

    def delays(self, x, arrays, first=0, n=None, max_lag=512, stream=None):
        """The delays of every array's microphones against its reference (the array's first row): one `correlate` call
        over all pairs, one copy to the host, one `peak` call per pair.  Returns (delays, peaks): per array the list of
        delays in samples (0.0 for the reference) and the list of peak records (None for the reference)."""
        arrays, pairs = _arrays(arrays)
        rows = self.correlate(x, pairs, first=first, n=n, max_lag=max_lag, stream=stream).cpu().numpy()
        return _split(arrays, [peak(r) for r in rows])


def delays_model(x, arrays, first=0, n=None, max_lag=512):
    """`Xcorr.delays` through `model` and `peak_model`: float64 on the host."""
    return align.delays_model(x, arrays, first, n, max_lag, model, peak_model)


def steer(x, arrays, xcorr=None, first=0, n=None, max_lag=512, stream=None):
    """Delay-and-sum beams for `Array.combine`, one per array, steered by the ESTIMATED delays: `array.steer` of every
    array's delays (its reference is the smallest delay, so that none is negative), with the array's rows of x as the
    microphones.  Returns (beams, delays, peaks)."""
    from . import array
    own = xcorr is None
    if own:
        xcorr = Xcorr(x.device.index or 0)
    try:
        delays, peaks = xcorr.delays(x, arrays, first=first, n=n, max_lag=max_lag, stream=stream)
    finally:
        if own:
            xcorr.close()
    beams = [[(int(a[m]), w, d) for (m, w, d) in array.steer(dl)] for a, dl in zip(arrays, delays)]
    return beams, delays, peaks
