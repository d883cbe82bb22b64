"""uchirp.array -- the array combiner: binding of libuchirp_array.so (include/uchirp_array.h) and its float64 model.

`Scene.render` (uchirp.scene) gives every microphone of an array the same transmission at its own fractional lead.
`Array.combine` turns rows of such a buffer into BEAMS: every beam is a weighted sum of microphones, each delayed by its
own fractional number of samples through a 16-coefficient Kaiser-windowed sinc, in one pass on the GPU, into a device
tensor that `Engine.receive_many` / `LiveStreams.next` / `Engine.process` read in place.  There is no CPU path behind
`Array`; `coefficients` (the library's host function) and the model need no GPU.

Beams are written as
    beams = [[(mic, weight, delay_samples), ...], ...]          one list of taps per beam
where the microphone hears the wanted sound `delay_samples` later than the beam's time axis.  `steer` makes the taps of a
delay-and-sum beam from the microphones' leads.  `model` is the same definition in numpy / float64.
"""
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_TAPS = 32
COEFS = 16
DELAY_MAX = 2.0 ** 30
EXPORTS = ["uc_array_abi_version", "uc_array_last_error", "uc_array_create", "uc_array_destroy", "uc_array_tap_coefficients",
           "uc_array_combine"]


class ArrayTap(C.Structure):
    """struct uc_array_tap (include/uchirp_array.h)."""
    _fields_ = [("delay_samples", C.c_double), ("weight", C.c_float), ("mic", C.c_uint32)]


class ArrayBeam(C.Structure):
    """struct uc_array_beam (include/uchirp_array.h)."""
    _fields_ = [("first_tap", C.c_uint32), ("n_taps", C.c_uint32)]


TAP_DTYPE = np.dtype([("delay_samples", "<f8"), ("weight", "<f4"), ("mic", "<u4")])
BEAM_DTYPE = np.dtype([("first_tap", "<u4"), ("n_taps", "<u4")])


class ArrayError(RuntimeError):
    pass


def _declare(L):
    L.uc_array_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_array_tap_coefficients.argtypes = [C.c_double, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    L.uc_array_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p]


_so = Binding("array", ArrayError, _declare, env="UCHIRP_ARRAY_LIB")  # UCHIRP_ARRAY_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def coefficients(delay, weight=1.0):
    """uc_array_tap_coefficients: (float32 [16], shift) of one tap, computed by the library on the host (no GPU)."""
    c = (C.c_float * COEFS)()
    shift = C.c_int64()
    _check(lib().uc_array_tap_coefficients(float(delay), float(weight), C.byref(shift), c), "uc_array_tap_coefficients")
    return np.frombuffer(c, np.float32).copy(), int(shift.value)


def coefficients_model(delay, weight=1.0):
    """The coefficients of include/uchirp_array.h in numpy: (float32 [16], shift)."""
    delay, weight = float(delay), float(np.float32(weight))
    if not (np.isfinite(delay) and np.isfinite(weight) and abs(delay) <= DELAY_MAX):
        raise ValueError("delay and weight must be finite, |delay| <= 2^30")
    whole = np.floor(delay)
    f = delay - whole
    if f >= 1.0:
        whole, f = whole + 1.0, 0.0
    c = np.zeros(COEFS, np.float32)
    if f == 0.0:
        c[7] = weight
    else:
        u = np.arange(COEFS, dtype=np.float64) - 7.0 - f
        c[:] = weight * (np.sin(np.pi * u) / (np.pi * u)) * np.i0(8.0 * np.sqrt(1.0 - (u / 8.0) ** 2)) / np.i0(8.0)
    return c, int(whole) - 7


def pack(beams):
    """The host arrays of uc_array_combine: (taps TAP_DTYPE [n_taps], beams BEAM_DTYPE [n_beams]); every beam's taps are
    laid out one after the other in the order given.  ValueError for a beam without taps or with more than MAX_TAPS."""
    rows = []
    b = np.zeros(len(beams), BEAM_DTYPE)
    for i, taps in enumerate(beams):
        taps = list(taps)
        if not 1 <= len(taps) <= MAX_TAPS:
            raise ValueError("beam %d has %d taps (1 .. %d)" % (i, len(taps), MAX_TAPS))
        b[i] = (len(rows), len(taps))
        for (mic, weight, delay) in taps:
            if int(mic) < 0:
                raise ValueError("beam %d: microphone %d" % (i, int(mic)))
            rows.append((delay, weight, int(mic)))
    return np.array(rows, TAP_DTYPE), b


def steer(leads, ref=None):
    """The taps of one delay-and-sum beam over microphones 0 .. M - 1 whose copies of the wanted sound have the leads
    `leads` (samples): [(m, 1 / M, lead_m - ref)].  `ref`, the beam's own lead, defaults to the smallest lead, so that no
    delay is negative and the beam hears the sound when the first microphone does."""
    leads = [float(v) for v in leads]
    if ref is None:
        ref = min(leads)
    return [(m, 1.0 / len(leads), ld - float(ref)) for m, ld in enumerate(leads)]


class Array:
    """One uc_array: the combiner on one MI355X."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_array_create(int(device), C.byref(h)), "uc_array_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_array_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def combine_packed(self, x, taps, beams, in_first=0, out_first=None, n_out=None, out=None, stream=None):
        """uc_array_combine on arrays as `pack` makes them (a loop of calls packs once)."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nm, n_in = int(x.shape[0]), int(x.shape[1])
        nb = len(beams)
        if out_first is None:
            out_first = in_first
        if out is None:
            out = torch.empty((nb, n_in if n_out is None else int(n_out)), dtype=torch.float32, device=dev)
        else:
            if (out.dim() != 2 or out.dtype != torch.float32 or out.device != dev or out.shape[0] != nb or
                    (out.shape[1] > 1 and out.stride(1) != 1) or (nb > 1 and out.stride(0) < out.shape[1])):
                raise ValueError("out must be a [%d, n_out] float32 tensor on %s with contiguous rows" % (nb, dev))
            if n_out is not None and int(n_out) != out.shape[1]:
                raise ValueError("n_out does not match out")
        no = int(out.shape[1])
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_array_combine(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nm,
                                      int(in_first), n_in, int(x.stride(0)) if nm > 1 else n_in, taps.ctypes.data_as(C.c_void_p), len(taps),
                                      beams.ctypes.data_as(C.c_void_p), nb, C.c_void_p(out.data_ptr()), int(out_first), no,
                                      int(out.stride(0)) if nb > 1 else no, C.c_void_p(stream) if stream else None), "uc_array_combine")
        return out

    def combine(self, x, beams, in_first=0, out_first=None, n_out=None, out=None, stream=None):
        """uc_array_combine: samples [out_first, out_first + n_out) of len(beams) beams -> a float32 torch tensor
        [n_beams, n_out] on the object's device (or into `out`: a 2-d device tensor with contiguous rows).  `x`: a 2-d
        float32 / int32 device tensor with contiguous rows holding the samples from `in_first` on.  out_first defaults to
        in_first and n_out to the length of x's rows.  Asynchronous on `stream` / torch's current stream."""
        return self.combine_packed(x, *pack(beams), in_first=in_first, out_first=out_first, n_out=n_out, out=out, stream=stream)


def model(x, beams, in_first=0, out_first=None, n_out=None, coef=coefficients_model):
    """What Array.combine writes, with the sums in float64: [n_beams, n_out].  The inputs are rounded to float32 first (the
    (float) cast of integer words), the coefficients are the float32 values `coef(delay, weight)` gives
    (`coefficients_model`, or `coefficients` for the library's), the weights float32 as struct uc_array_tap holds them.
    Samples outside the rows are 0.  (Products with a coefficient that is exactly 0 are left out: inputs are taken as
    finite.)"""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be 2-d")
    xf = x.astype(np.float32).astype(np.float64)
    n_in = x.shape[1]
    in_first = int(in_first)
    out_first = in_first if out_first is None else int(out_first)
    n_out = n_in if n_out is None else int(n_out)
    out = np.zeros((len(beams), n_out), np.float64)
    for b, taps in enumerate(beams):
        for (mic, weight, delay) in taps:
            c, shift = coef(delay, np.float32(weight))
            c = np.asarray(c, np.float32).astype(np.float64)
            start = out_first + shift - in_first                # row element under c[0] for the first output
            seg = np.zeros(n_out + COEFS - 1, np.float64)
            lo, hi = max(start, 0), min(start + len(seg), n_in)
            if hi > lo:
                seg[lo - start:hi - start] = xf[int(mic), lo:hi]
            for t in np.nonzero(c)[0]:
                out[b] += c[t] * seg[t:t + n_out]
    return out


def magnitude(x, beams, in_first=0, out_first=None, n_out=None, coef=coefficients_model):
    """Sum over the taps and coefficients of |c_k[t] x_k[j + shift_k + t]|, per output sample (float64, the shape of
    `model`): what the rounding errors of a float evaluation scale with."""
    def absolute(delay, weight):
        c, shift = coef(delay, weight)
        return np.abs(c), shift

    return model(np.abs(np.asarray(x).astype(np.float32)), beams, in_first, out_first, n_out, coef=absolute)
