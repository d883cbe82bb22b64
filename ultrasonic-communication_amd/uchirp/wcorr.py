"""uchirp.wcorr -- the band-weighted correlator: binding of libuchirp_wcorr.so (include/uchirp_wcorr.h), its float64 model,
the ideal it approximates and an independent float32 evaluation of the same definition.

`Xcorr.correlate` and `Tracker.windows` correlate the rows over the whole band; `Wcorr.windows` computes the same windowed
correlations with a real weight on every bin of the 2048-point cross-spectrum (`band_weights`: 1 on the chirps' band, cos^2
edges), with `guard` extra lags that are computed and not stored, so that at low SNR the crest rule (`peak`, the library's
host function: the bits of `xcorr.peak`) stays on the right carrier cycle.  `Wcorr.estimator(weights, guard)` has
`Xcorr.delays`' signature, so `retime.drift` and `steer` work on top of it.  There is no CPU path behind `Wcorr`;
`band_weights`, `peak`, `peak_model`, `model`, `ideal_model` and `emulate32` need no GPU.

Arrays are written as in uchirp.xcorr: [[row, row, ...], ...], the first row of an array its reference.
"""
import ctypes as C

import numpy as np

from . import align, xcorr
from ._binding import Binding
from .align import PAIR_DTYPE, _arrays, _pairs, _record, _split  # noqa: F401  (one layout of pairs, one shape of records)
from .track import _windows
from .xcorr import _rows, _window, segments

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_LAG = 512
POINTS = 2048
GROUP = 4
BINS = POINTS // 2 + 1
ERROR_C = 9                                   # four times the worst ratio of emulate32 (2.22), rounded up
GUARD = 128                                   # the header's recommendation
NO_PEAK, AT_EDGE = 1, 2
EXPORTS = ["uc_wcorr_abi_version", "uc_wcorr_last_error", "uc_wcorr_create", "uc_wcorr_destroy", "uc_wcorr_windows",
           "uc_wcorr_band_weights", "uc_wcorr_peak"]


class WcorrPair(C.Structure):
    """struct uc_wcorr_pair (include/uchirp_wcorr.h)."""
    _fields_ = [("ref", C.c_uint32), ("mic", C.c_uint32)]


class WcorrPeak(C.Structure):
    """struct uc_wcorr_peak_t (include/uchirp_wcorr.h)."""
    _fields_ = [("delay_samples", C.c_double), ("height", C.c_double), ("runner_up", C.c_double), ("lag", C.c_int32),
                ("flags", C.c_uint32)]


class WcorrError(RuntimeError):
    pass


def _declare(L):
    L.uc_wcorr_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_wcorr_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]
    L.uc_wcorr_band_weights.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p]
    L.uc_wcorr_peak.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(WcorrPeak)]


_so = Binding("wcorr", WcorrError, _declare, env="UCHIRP_WCORR_LIB")  # UCHIRP_WCORR_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def band_weights(fs, f_lo, f_hi, taper_hz=0.0, guard=GUARD):
    """uc_wcorr_band_weights: (w, tail) -- the BINS float32 weights of the band [f_lo, f_hi] with cos^2 edges `taper_hz`
    wide at the sample rate fs, and the share of their impulse response's energy at circular distance > guard; computed
    by the library on the host (no GPU)."""
    w = np.zeros(BINS, np.float32)
    tail = C.c_double()
    _check(lib().uc_wcorr_band_weights(float(fs), float(f_lo), float(f_hi), float(taper_hz), int(guard), w.ctypes.data_as(C.c_void_p),
                                       C.byref(tail)), "uc_wcorr_band_weights")
    return w, tail.value


def peak(row):
    """uc_wcorr_peak: the record {delay_samples, height, runner_up, lag, flags} of one correlation row of 2 L + 1 values,
    computed by the library on the host (no GPU)."""
    r = np.ascontiguousarray(row, np.float64)
    if r.ndim != 1 or len(r) < 3 or len(r) % 2 == 0:
        raise ValueError("a correlation row has 2 L + 1 values")
    out = WcorrPeak()
    _check(lib().uc_wcorr_peak(r.ctypes.data_as(C.c_void_p), (len(r) - 1) // 2, C.byref(out)), "uc_wcorr_peak")
    return _record(out.delay_samples, out.height, out.runner_up, out.lag, out.flags)


def peak_model(row):
    """The peak rule of include/uchirp_wcorr.h (that of uchirp_align.h) in numpy / float64: the same record as `peak`."""
    return align.peak_model(row, MAX_LAG)


def _weights(weights):
    """the table of a call: BINS finite float32 values (None: ones)"""
    if weights is None:
        return np.ones(BINS, np.float32)
    w = np.ascontiguousarray(weights, np.float32)
    if w.shape != (BINS,) or not np.isfinite(w).all():
        raise ValueError("weights: %d finite values" % BINS)
    return w


def _lags(max_lag, guard):
    L, g = int(max_lag), int(guard)
    if not (1 <= L and 0 <= g and L + g <= MAX_LAG):
        raise ValueError("max_lag >= 1, guard >= 0 and max_lag + guard <= %d" % MAX_LAG)
    return L, g


def impulse_response(weights):
    """h[t] = (1 / 2048) sum over k of W[k] cos(2 pi k t / 2048), t = 0 .. 2047, in float64"""
    return np.fft.irfft(_weights(weights).astype(np.float64), POINTS)


def model(x, pairs, first=0, n=None, max_lag=64, guard=GUARD, weights=None, magnitude=False):
    """What one window of Wcorr.windows writes, in float64, segment by segment as the header defines it: every segment's
    2048-point circular correlation at L' = max_lag + guard, its spectrum times W, the values guard .. guard + 2 L, summed
    over the segments: [n_pairs, 2 L + 1].  The transforms are numpy's in double precision (their error is some 1e-15 of
    E_p).  With `magnitude` E_p at L' instead, [n_pairs]: what the header's error form scales with (`xcorr.model`'s)."""
    L, g = _lags(max_lag, guard)
    Lp = L + g
    if magnitude:
        return xcorr.model(x, pairs, first, n, Lp, magnitude=True)
    x32, n_in, first, n, _ = _rows(x, first, n, Lp)
    xf = x32.astype(np.float64)
    W = _weights(weights).astype(np.float64)
    p = _pairs(pairs)
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        for i0, cnt in segments(first, n, Lp):
            a = _window(xf[ref, first + i0:first + i0 + cnt], 0, POINTS)
            b = _window(_window(xf[mic], first + i0 - Lp, cnt + 2 * Lp), 0, POINTS)
            c = np.fft.irfft(np.conj(np.fft.rfft(a)) * np.fft.rfft(b) * W, POINTS)
            out[i] += c[g:g + 2 * L + 1]
    return out


def windows_model(x, pairs, first=0, window_len=None, hop=None, n_windows=None, max_lag=64, guard=GUARD, weights=None, magnitude=False):
    """What Wcorr.windows writes, in float64: `model` per window, [n_pairs, n_windows, 2 L + 1] (with `magnitude` E_p per
    window instead, [n_pairs, n_windows])."""
    x = np.asarray(x)
    first, window_len, hop, n_windows = _windows(x.shape[1], first, x.shape[1] - int(first) if window_len is None else window_len, hop, n_windows)
    per = [model(x, pairs, first + w * hop, window_len, max_lag, guard, weights, magnitude=magnitude) for w in range(n_windows)]
    return np.stack(per, axis=1)


def ideal_model(x, pairs, first=0, n=None, max_lag=64, weights=None):
    """The linearly filtered correlation that `model` approximates, by one long transform: the whole window's linear
    correlation r[l] = sum over j in [first, first + n) of x[ref, j] x[mic, j + l] at every lag |l| <= L + 1024 (samples
    of the microphone row outside it are 0), convolved LINEARLY with the impulse response h[t], t = -1023 .. 1024:
    [n_pairs, 2 L + 1].  `model` differs from it by what its segments' wrapped lags carry: h's tail beyond the guard."""
    L, _ = _lags(max_lag, 0)
    x32, n_in, first, n, _ = _rows(x, first, n, L)
    xf = x32.astype(np.float64)
    h = impulse_response(weights)
    reach = POINTS // 2
    M = L + reach                                                # lags of r that a stored lag draws on
    size = 1 << int(np.ceil(np.log2(2 * n + 2 * M + 1)))
    p = _pairs(pairs)
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    hc = np.concatenate([h[reach + 1:], h[:reach + 1]])         # h[t], t = -1023 .. 1024
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        a = np.zeros(size)
        a[:n] = xf[ref, first:first + n]
        b = np.zeros(size)
        b[:n + 2 * M] = _window(xf[mic], first - M, n + 2 * M)
        r = np.fft.irfft(np.conj(np.fft.rfft(a)) * np.fft.rfft(b), size)[:2 * M + 1]      # r[l], l = -M .. M
        # out[l] = sum over t of h[t] r[l - t]
        full = np.convolve(r, hc)                                # index (l + M) + (t + 1023)
        out[i] = full[reach - 1 + reach:reach - 1 + reach + 2 * L + 1]
    return out


def emulate32(x, pairs, first=0, n=None, max_lag=64, guard=GUARD, weights=None):
    """The definition's structure -- segments of S = P - 2 L' samples, groups of G cross-spectra added in float, every bin
    times its weight in float, one inverse transform per group, the unit sums guard .. guard + 2 L added in double -- with
    scipy.fft (pocketfft) in single precision: an independent float32 evaluation, there only so that tests have a
    yardstick for what float32 can do."""
    import scipy.fft
    L, g = _lags(max_lag, guard)
    Lp = L + g
    x32, n_in, first, n, _ = _rows(x, first, n, Lp)
    W = _weights(weights)
    p = _pairs(pairs)
    segs = segments(first, n, Lp)
    out = np.zeros((len(p), 2 * L + 1), np.float64)
    for i, (ref, mic) in enumerate(zip(p["ref"], p["mic"])):
        for g0 in range(0, len(segs), GROUP):
            acc = np.zeros(BINS, np.complex64)
            for i0, cnt in segs[g0:g0 + GROUP]:
                a = _window(x32[ref, first + i0:first + i0 + cnt], 0, POINTS)
                b = _window(_window(x32[mic], first + i0 - Lp, cnt + 2 * Lp), 0, POINTS)
                A, B = scipy.fft.rfft(a), scipy.fft.rfft(b)
                assert A.dtype == np.complex64
                acc = acc + np.conj(A) * B
            acc = (acc.real * W + 1j * (acc.imag * W)).astype(np.complex64)
            unit = scipy.fft.irfft(acc, POINTS)
            assert unit.dtype == np.float32
            out[i] += unit[g:g + 2 * L + 1].astype(np.float64)
    return out


class Wcorr:
    """One uc_wcorr: the band-weighted correlator on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_wcorr_create(int(device), C.byref(h)), "uc_wcorr_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_wcorr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def windows(self, x, pairs, first=0, window_len=None, hop=None, n_windows=None, max_lag=64, guard=GUARD, weights=None,
                out=None, stream=None):
        """uc_wcorr_windows: the weighted correlations of every (pair, window) as a float64 torch tensor
        [n_pairs, n_windows, 2 L + 1] on the object's device (or into `out`: such a tensor with evenly spaced contiguous
        rows).  `x`: a 2-d float32 / int32 device tensor with contiguous rows; `pairs`: (ref, mic) rows, a list or a
        PAIR_DTYPE array; `weights`: BINS floats or None (ones).  window_len defaults to the rest of the row, hop to
        window_len, n_windows to as many as fit.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nm, n_in = int(x.shape[0]), int(x.shape[1])
        p = pairs if isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE else _pairs(pairs)
        p = np.ascontiguousarray(p)
        L, g = int(max_lag), int(guard)
        if L < 0 or g < 0:
            raise ValueError("max_lag and guard must not be negative")
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        if w is not None and w.shape != (BINS,):
            raise ValueError("weights: %d values" % BINS)
        first, window_len, hop, n_windows = _windows(n_in, first, n_in - int(first) if window_len is None else window_len, hop, n_windows)
        lags = 2 * L + 1
        rows = len(p) * n_windows
        if out is None:
            out = torch.empty((len(p), n_windows, lags), dtype=torch.float64, device=dev)
        elif (out.dim() != 3 or out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (len(p), n_windows, lags) or
              out.stride(2) != 1 or (n_windows > 1 and out.stride(1) < lags) or
              (len(p) > 1 and (out.stride(0) != n_windows * out.stride(1) if n_windows > 1 else out.stride(0) < lags))):
            raise ValueError("out must be a [%d, %d, %d] float64 tensor on %s with evenly spaced contiguous rows" % (len(p), n_windows, lags, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        cstride = lags if rows == 1 else int(out.stride(1) if n_windows > 1 else out.stride(0))
        _check(lib().uc_wcorr_windows(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm, n_in,
                                      int(x.stride(0)) if nm > 1 else n_in, p.ctypes.data_as(C.c_void_p), len(p), first, window_len, hop,
                                      n_windows, L, g, w.ctypes.data_as(C.c_void_p) if w is not None else None, C.c_void_p(out.data_ptr()),
                                      cstride, C.c_void_p(stream) if stream else None), "uc_wcorr_windows")
        return out

    def correlate(self, x, pairs, first=0, n=None, max_lag=64, guard=GUARD, weights=None, stream=None):
        """One window: the weighted counterpart of `Xcorr.correlate`, [n_pairs, 2 L + 1]; n defaults to the rest of the row."""
        n = int(x.shape[1]) - int(first) if n is None else int(n)
        return self.windows(x, pairs, first, n, n, 1, max_lag, guard, weights, stream=stream)[:, 0]

    def estimator(self, weights=None, guard=GUARD):
        """An object whose `.delays(x, arrays, first, n, max_lag, stream)` is `Xcorr.delays` over the weighted correlation:
        what `retime.drift` and `steer` take as their estimator."""
        return Estimator(self, weights, guard)


class Estimator:
    """`Xcorr.delays` over `Wcorr.correlate` with fixed weights and guard."""

    def __init__(self, wcorr, weights=None, guard=GUARD):
        self.wcorr, self.weights, self.guard = wcorr, None if weights is None else _weights(weights), int(guard)

    def delays(self, x, arrays, first=0, n=None, max_lag=64, stream=None):
        """The delays of every array's microphones against its reference (the array's first row): one `correlate` call
        over all pairs, one copy to the host, one `peak` call per pair.  Returns (delays, peaks) as `Xcorr.delays`."""
        arrays, pairs = _arrays(arrays)
        rows = self.wcorr.correlate(x, pairs, first, n, max_lag, self.guard, self.weights, stream=stream).cpu().numpy()
        return _split(arrays, [peak(r) for r in rows])


def delays_model(x, arrays, first=0, n=None, max_lag=64, guard=GUARD, weights=None):
    """`Estimator.delays` through `model` and `peak_model`: float64 on the host."""
    return align.delays_model(x, arrays, first, n, max_lag, lambda y, p, f, m, L: model(y, p, f, m, L, guard, weights), peak_model)


def steer(x, arrays, estimator, first=0, n=None, max_lag=64, stream=None):
    """`xcorr.steer` over an `Estimator`: delay-and-sum beams for `Array.combine`, one per array, steered by the delays
    estimated from the weighted correlation.  Returns (beams, delays, peaks)."""
    return xcorr.steer(x, arrays, estimator, first=first, n=n, max_lag=max_lag, stream=stream)
