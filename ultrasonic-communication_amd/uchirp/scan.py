"""uchirp.scan -- the beam scanner: binding of libuchirp_scan.so (include/uchirp_scan.h), its float64 model, and the candidate
delay vectors of an array's geometry.

The estimators (uchirp.align, .xcorr, .track, .wcorr) find delays pair by pair, and at low SNR a pair lands whole carrier
cycles off.  `Scanner.power` forms the delay-and-sum beam of EVERY candidate delay vector (`direction_delays`,
`point_delays`) over many identical arrays in one pass on the GPU and writes one power per (array, window, beam) and the
strongest beam per (array, window); `beams_of` turns the chosen candidates into the tap lists `Array.combine` takes.  There
is no CPU path behind `Scanner`; `quantise`, `table`, `power_row` (the library's host functions: the definition in plain C)
and `model` need no GPU.
"""
import ctypes as C

import numpy as np

from . import array
from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_TAPS = 32
COEFS = 16
FRACTIONS = 256
MAX_BEAMS = 1 << 20
SEGMENT = 4096
DELAY_MAX = 2.0 ** 20
NOT_FINITE = 1
EXPORTS = ["uc_scan_abi_version", "uc_scan_last_error", "uc_scan_create", "uc_scan_destroy", "uc_scan_quantise", "uc_scan_table",
           "uc_scan_power_row", "uc_scan_set_beams", "uc_scan_direct_beams", "uc_scan_power"]

BEST_DTYPE = np.dtype([("beam", "<u4"), ("flags", "<u4"), ("power", "<f8")])     # struct uc_scan_best


class ScanError(RuntimeError):
    pass


def _declare(L):
    u32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    L.uc_scan_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_scan_quantise.argtypes = [C.c_double, C.POINTER(C.c_int32)]
    L.uc_scan_table.argtypes = [C.c_float, f32]
    L.uc_scan_power_row.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, u32, f32, C.POINTER(C.c_int32),
                                    C.c_size_t, C.c_uint64, C.c_size_t, C.POINTER(C.c_double)]
    L.uc_scan_set_beams.argtypes = [C.c_void_p, u32, f32, C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.c_size_t]
    L.uc_scan_direct_beams.argtypes = [C.c_void_p, u32]
    L.uc_scan_power.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]


_so = Binding("scan", ScanError, _declare, env="UCHIRP_SCAN_LIB")  # UCHIRP_SCAN_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


# ------------------------------------------------------------------------------------------------------ the host functions

def quantise(delay):
    """uc_scan_quantise: llrint(delay * 256), by the library (no GPU)."""
    q = C.c_int32()
    _check(lib().uc_scan_quantise(float(delay), C.byref(q)), "uc_scan_quantise")
    return int(q.value)


def quantise_model(delays):
    """The same in numpy: int64, the shape of `delays` (np.rint rounds ties to even, as llrint does)."""
    d = np.asarray(delays, np.float64)
    if not np.isfinite(d).all() or (np.abs(d) > DELAY_MAX).any():
        raise ValueError("delays must be finite, |delay| <= 2^20")
    return np.rint(d * 256.0).astype(np.int64)


def table(weight=1.0):
    """uc_scan_table: float32 [256, 16], the coefficient rows of a tap of this weight, by the library (no GPU)."""
    t = np.zeros((FRACTIONS, COEFS), np.float32)
    _check(lib().uc_scan_table(float(weight), t.ctypes.data_as(C.POINTER(C.c_float))), "uc_scan_table")
    return t


def _taps(mics, weights):
    m = np.ascontiguousarray(np.asarray(mics, np.int64).reshape(-1))
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if m.size != w.size or not 1 <= m.size <= MAX_TAPS or (m < 0).any() or (m > 0xFFFFFFFF).any():
        raise ValueError("mics and weights must hold the same 1 .. %d taps" % MAX_TAPS)
    return m.astype(np.uint32), w


def _rows(x):
    a = np.asarray(x)
    a = np.ascontiguousarray(a, np.int32 if a.dtype == np.int32 else np.float32)
    if a.ndim != 2:
        raise ValueError("x must be 2-d")
    return a


def power_row(x, mics, weights, q, first, window_len, in_first=0):
    """uc_scan_power_row: the definition in plain C for ONE beam and ONE window (no GPU).  x: host rows [n_rows, n_in]
    (float32, or int32 words) holding the samples from `in_first` on; mics[k] names tap k's row, q[k] its quantised delay."""
    a = _rows(x)
    m, w = _taps(mics, weights)
    qq = np.ascontiguousarray(np.asarray(q, np.int64).reshape(-1).astype(np.int32))
    if qq.size != m.size:
        raise ValueError("q must hold one quantised delay per tap")
    out = C.c_double()
    _check(lib().uc_scan_power_row(a.ctypes.data_as(C.c_void_p), DTYPE_I32 if a.dtype == np.int32 else DTYPE_F32, a.shape[0], int(in_first),
                                   a.shape[1], a.shape[1], m.ctypes.data_as(C.POINTER(C.c_uint32)), w.ctypes.data_as(C.POINTER(C.c_float)),
                                   qq.ctypes.data_as(C.POINTER(C.c_int32)), m.size, int(first), int(window_len), C.byref(out)), "uc_scan_power_row")
    return float(out.value)


def definition(x, mics, weights, delays, first, window_len, hop=None, n_windows=1, n_arrays=1, array_rows=None, in_first=0):
    """What Scanner.power writes, through `power_row` beam by beam and window by window: float64 [n_arrays, n_windows,
    n_beams].  Slow; the tests' reference."""
    a = _rows(x)
    m, w = _taps(mics, weights)
    q = quantise_model(np.asarray(delays, np.float64).reshape(-1, m.size))
    hop = int(window_len) if hop is None else int(hop)
    array_rows = a.shape[0] // int(n_arrays) if array_rows is None else int(array_rows)
    out = np.zeros((int(n_arrays), int(n_windows), q.shape[0]), np.float64)
    for ar in range(int(n_arrays)):
        sub = a[ar * array_rows:(ar + 1) * array_rows]
        for wi in range(int(n_windows)):
            for b in range(q.shape[0]):
                out[ar, wi, b] = power_row(sub, m, w, q[b], int(first) + wi * hop, window_len, in_first)
    return out


def best_model(power):
    """The best records of powers [..., n_beams]: BEST_DTYPE [...] (the lowest index on a tie; a row with a power that is
    not finite is flagged, beam 0, power 0)."""
    p = np.asarray(power, np.float64)
    out = np.zeros(p.shape[:-1], BEST_DTYPE)
    bad = ~np.isfinite(p).all(axis=-1)
    at = np.argmax(np.where(np.isfinite(p), p, -1.0), axis=-1)
    out["beam"] = np.where(bad, 0, at)
    out["flags"] = np.where(bad, NOT_FINITE, 0)
    out["power"] = np.where(bad, 0.0, np.take_along_axis(np.where(np.isfinite(p), p, 0.0), at[..., None], axis=-1)[..., 0])
    return out


# ------------------------------------------------------------------------------------------------------------- the model

def model(x, mics, weights, delays, first, window_len, hop=None, n_windows=1, n_arrays=1, array_rows=None, in_first=0,
          coef=array.coefficients_model, samples=False):
    """The powers in float64 on the float32 coefficients and samples: [n_arrays, n_windows, n_beams].  The beam samples are
    `array.model`'s for the taps (mics[k] + a * array_rows, weights[k], q_bk / 256) with `coef(delay, weight)` as there
    (`array.coefficients` for the library's); they are computed row by row here, one matrix product per (array, tap) for all
    the fractions the beams use, so that thousands of beams cost little.  `samples`: return the beam samples over
    [first, first + (n_windows - 1) hop + window_len) instead: [n_arrays, n_beams, span]."""
    a = np.asarray(x)
    if a.ndim != 2:
        raise ValueError("x must be 2-d")
    xf = a.astype(np.float32).astype(np.float64)
    m, w = _taps(mics, weights)
    q = quantise_model(np.asarray(delays, np.float64).reshape(-1, m.size))
    nb = q.shape[0]
    hop = int(window_len) if hop is None else int(hop)
    n_windows, n_arrays, window_len, first, in_first = int(n_windows), int(n_arrays), int(window_len), int(first), int(in_first)
    array_rows = a.shape[0] // n_arrays if array_rows is None else int(array_rows)
    span = (n_windows - 1) * hop + window_len
    shift, frac = (q >> 8) - 7, q & 255
    taps = []
    for k in range(m.size):
        fr = np.unique(frac[:, k])
        cf = np.stack([np.asarray(coef(f / 256.0, w[k])[0], np.float32).astype(np.float64) for f in fr], axis=1)    # [16, fractions]
        taps.append((cf, np.searchsorted(fr, frac[:, k]), int(shift[:, k].min()), int(shift[:, k].max())))
    out = np.zeros((n_arrays, n_windows, nb), np.float64)
    kept = []
    for ar in range(n_arrays):
        y = np.zeros((nb, span), np.float64)
        for k, (cf, col, lo, hi) in enumerate(taps):
            row = xf[ar * array_rows + int(m[k])]
            seg = np.zeros(span + hi - lo + COEFS - 1, np.float64)                    # the row from first + lo on
            start = first + lo - in_first
            s0, s1 = max(start, 0), min(start + seg.size, row.size)
            if s1 > s0:
                seg[s0 - start:s1 - start] = row[s0:s1]
            filt = np.lib.stride_tricks.sliding_window_view(seg, COEFS) @ cf          # [span + hi - lo, fractions]
            for b in range(nb):
                o = int(shift[b, k]) - lo
                y[b] += filt[o:o + span, col[b]]
        if samples:
            kept.append(y)
        for wi in range(n_windows):
            out[ar, wi, :] = (y[:, wi * hop:wi * hop + window_len] ** 2).sum(axis=1)
    return np.stack(kept) if samples else out


# -------------------------------------------------------------------------------------------------- candidate delay vectors

def _rebase(d):
    return d - d.min(axis=1, keepdims=True)


def direction_delays(mic_xyz, unit_vectors, fs=78125.0, c=343.0):
    """Far field: the delays [n_directions, n_mics] (samples) of a plane wave that ARRIVES FROM the directions
    `unit_vectors` [n, 3] at microphones `mic_xyz` [m, 3] (metres): -(m . u) / c * fs minus the row's minimum, so that no
    delay is negative (`array.steer`'s convention: the beam hears the sound when the first microphone does)."""
    mic = np.asarray(mic_xyz, np.float64).reshape(-1, 3)
    u = np.asarray(unit_vectors, np.float64).reshape(-1, 3)
    return _rebase(-(u @ mic.T) / float(c) * float(fs))


def point_delays(mic_xyz, points, fs=78125.0, c=343.0):
    """Near field: |p - m| / c * fs minus the row's minimum, [n_points, n_mics]."""
    mic = np.asarray(mic_xyz, np.float64).reshape(-1, 3)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return _rebase(np.linalg.norm(p[:, None, :] - mic[None, :, :], axis=2) / float(c) * float(fs))


def best_of(records):
    """The best records a call returned (a device tensor [n_arrays, n_windows, 4] of int32) as BEST_DTYPE
    [n_arrays, n_windows] on the host; synchronises."""
    t = records.cpu().numpy()
    return np.ascontiguousarray(t).view(BEST_DTYPE)[..., 0]


def beams_of(best, delays, mics, weights, array_rows=None):
    """The tap lists `Array.combine` takes for the chosen candidates: one beam per record of `best` (BEST_DTYPE, any shape,
    flattened; or plain beam indices), its delays at their quantised values.  With `array_rows`, pass one record per array:
    record a's taps name the rows mics[k] + a * array_rows of the whole buffer."""
    m, w = _taps(mics, weights)
    q = quantise_model(np.asarray(delays, np.float64).reshape(-1, m.size))
    idx = np.asarray(best["beam"] if getattr(best, "dtype", None) == BEST_DTYPE else best, np.int64).reshape(-1)
    return [[(int(m[k]) + (a * int(array_rows) if array_rows else 0), float(w[k]), float(q[b, k]) / 256.0) for k in range(m.size)]
            for a, b in enumerate(idx)]


# -------------------------------------------------------------------------------------------------------------- the object

class Scanner:
    """One uc_scan: the beam scanner on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_scan_create(int(device), C.byref(h)), "uc_scan_create")
        self._h = h
        self.device = int(device)
        self.n_taps = self.n_beams = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_beams(self, mics, weights, delays):
        """uc_scan_set_beams: mics and weights of n_taps microphones, delays [n_beams, n_taps] (samples); they replace the
        object's steering set.  Synchronous."""
        m, w = _taps(mics, weights)
        d = np.ascontiguousarray(np.asarray(delays, np.float64).reshape(-1, m.size))
        _check(lib().uc_scan_set_beams(self._h, m.ctypes.data_as(C.POINTER(C.c_uint32)), w.ctypes.data_as(C.POINTER(C.c_float)), m.size,
                                       d.ctypes.data_as(C.POINTER(C.c_double)), d.shape[0], m.size), "uc_scan_set_beams")
        self.n_taps, self.n_beams = int(m.size), int(d.shape[0])

    def direct_beams(self):
        """uc_scan_direct_beams: how many beams of the set take the kernel's direct path."""
        n = C.c_uint32()
        _check(lib().uc_scan_direct_beams(self._h, C.byref(n)), "uc_scan_direct_beams")
        return int(n.value)

    def power(self, x, first, window_len, hop=None, n_windows=1, n_arrays=1, array_rows=None, power=None, best=True, stream=None, in_first=0):
        """uc_scan_power: x [n_rows, n_in] (a 2-d float32 / int32 device tensor with contiguous rows holding the samples from
        `in_first` on) -> (powers, best): float64 [n_arrays, n_windows, n_beams] and the best records, int32
        [n_arrays, n_windows, 4] (`best_of` reads them), both on the object's device.  hop defaults to window_len and
        array_rows to n_rows // n_arrays.  `power`: a float64 device tensor [n_arrays, n_windows, n_beams] to write into
        (rows may lie apart: stride(2) == 1, stride(0) == n_windows * stride(1)), or False: no powers are returned (they
        stay in the object's scratch).  `best` False: no records.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nr, n_in = int(x.shape[0]), int(x.shape[1])
        n_arrays, n_windows = int(n_arrays), int(n_windows)
        if array_rows is None:
            array_rows = nr // max(n_arrays, 1)
        shape = (n_arrays, n_windows, self.n_beams)
        pstride = 0
        if power is None:
            power = torch.empty(shape, dtype=torch.float64, device=dev)
        elif power is False:
            power = None
            if not best:
                raise ValueError("neither powers nor best records are asked for")
        else:
            if (power.dim() != 3 or power.dtype != torch.float64 or power.device != dev or tuple(power.shape) != shape or
                    (shape[2] > 1 and power.stride(2) != 1)):
                raise ValueError("power must be a %r float64 tensor on %s with contiguous rows" % (shape, dev))
            pstride = int(power.stride(1)) if n_windows > 1 else int(power.stride(0)) if n_arrays > 1 else shape[2]
            if pstride < shape[2] or (n_arrays > 1 and n_windows > 1 and power.stride(0) != n_windows * pstride):
                raise ValueError("power's rows must lie one stride apart")
        rec = torch.zeros((n_arrays, n_windows, 4), dtype=torch.int32, device=dev) if best else None
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_scan_power(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nr, int(in_first), n_in,
                                   int(x.stride(0)) if nr > 1 else n_in, n_arrays, int(array_rows), int(first), int(window_len),
                                   int(window_len if hop is None else hop), n_windows, C.c_void_p(power.data_ptr()) if power is not None else None,
                                   pstride, C.c_void_p(rec.data_ptr()) if best else None, C.c_void_p(stream) if stream else None), "uc_scan_power")
        return power, rec
