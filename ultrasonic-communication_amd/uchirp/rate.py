"""uchirp.rate -- the rate converter: binding of libuchirp_rate.so (include/uchirp_rate.h) and its float64 model.

Every receiver here reads samples at 78 125 Hz; a sound card delivers 44.1, 48 or 96 kHz, and the transmitter the project
pins itself to is a 44.1 kHz WAV.  `Converter.convert` takes many rows at one rate to up / down times that rate through one
polyphase Kaiser-windowed sinc, in one pass on the GPU, into a device tensor that the retimer, the correlators, the combiner
and the receivers read in place.  It is `uchirp.resample.resample` (float64 numpy, one row) for thousands of microphones:
on whole rows from sample 0 `model` agrees with it to 1e-9 of the peak.  There is no CPU path behind `Converter`; `plan`,
`table`, `step`, `span`, `count` (the library's host functions) and the models need no GPU.
"""
import ctypes as C
from math import gcd

import numpy as np

from . import resample as _resample
from ._binding import Binding

ABI_VERSION = 1
DTYPE_I16, DTYPE_F32 = 0, 1
RATIO_MAX = 4096
HALF_MIN, HALF_MAX = 4, 32
TAPS_MAX = 128
TABLE_MAX = 2 ** 19
BETA_MAX = 100.0
SAMPLE_END_MAX = 2 ** 38
FS_OUT = 78125
TILE_LANES, WINDOW = 256, 504                         # of the kernel (csrc/uc_rate.hpp): what `tile_outputs` mirrors
EXPORTS = ["uc_rate_abi_version", "uc_rate_last_error", "uc_rate_plan", "uc_rate_table", "uc_rate_step", "uc_rate_span",
           "uc_rate_count", "uc_rate_create", "uc_rate_destroy", "uc_rate_convert"]


class RateInfo(C.Structure):
    """struct uc_rate_info (include/uchirp_rate.h)."""
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32), ("half", C.c_uint32), ("taps", C.c_uint32), ("centre", C.c_uint32),
                ("table_len", C.c_uint32)]

    def __repr__(self):
        return "RateInfo(up=%d, down=%d, half=%d, taps=%d, centre=%d, table_len=%d)" % (
            self.up, self.down, self.half, self.taps, self.centre, self.table_len)


class RateError(RuntimeError):
    pass


def _declare(L):
    L.uc_rate_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(RateInfo)]
    L.uc_rate_table.argtypes = [C.POINTER(RateInfo), C.c_double, C.POINTER(C.c_float), C.c_size_t]
    L.uc_rate_step.argtypes = [C.POINTER(RateInfo), C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]
    L.uc_rate_span.argtypes = [C.POINTER(RateInfo), C.c_uint64, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.uc_rate_count.argtypes = [C.POINTER(RateInfo), C.c_uint64]
    L.uc_rate_count.restype = C.c_int64
    L.uc_rate_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_void_p)]
    L.uc_rate_convert.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p,
                                  C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p]


_so = Binding("rate", RateError, _declare, env="UCHIRP_RATE_LIB")  # UCHIRP_RATE_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def plan(up, down, half=24, beta=9.0):
    """uc_rate_plan: the RateInfo of a ratio (reduced up and down, half, taps, centre, table_len), by the library (no GPU)."""
    info = RateInfo()
    _check(lib().uc_rate_plan(int(up), int(down), int(half), float(beta), C.byref(info)), "uc_rate_plan")
    return info


def plan_model(up, down, half=24, beta=9.0):
    """The plan of include/uchirp_rate.h in Python integers: (up, down, half, taps, centre, table_len); ValueError where the
    library refuses."""
    up, down, half, beta = int(up), int(down), int(half), float(beta)
    if up < 1 or down < 1:
        raise ValueError("up or down below 1")
    g = gcd(up, down)
    up, down = up // g, down // g
    q = max(up, down)
    taps = 2 * half * q // up + 1
    if (up == down or q > RATIO_MAX or not HALF_MIN <= half <= HALF_MAX or not (np.isfinite(beta) and 0.0 <= beta <= BETA_MAX)
            or taps > TAPS_MAX or up * taps > TABLE_MAX):
        raise ValueError("a ratio, half or beta that include/uchirp_rate.h refuses")
    return up, down, half, taps, half * q, up * taps


def table(info, beta=9.0):
    """uc_rate_table: C as float32 [up, taps], computed by the library on the host (no GPU)."""
    t = (C.c_float * info.table_len)()
    _check(lib().uc_rate_table(C.byref(info), float(beta), t, info.table_len), "uc_rate_table")
    return np.frombuffer(t, np.float32).reshape(info.up, info.taps).copy()


def prototype(info, beta=9.0):
    """h of the definition in float64 (resample.design: numpy's sinc, Kaiser window and sum)."""
    return _resample.design(info.up, info.down, info.half, float(beta))


def table_model(info, beta=9.0):
    """The table of include/uchirp_rate.h in numpy: float32 [up, taps] (numpy's sine, Bessel function and pairwise sum: it
    may differ from the library's in the last bit of an entry)."""
    h = prototype(info, beta)
    hp = np.zeros(info.up * info.taps)                 # up * taps > 2 half q: h and the zeros behind it
    hp[:h.size] = h
    return np.ascontiguousarray(hp.reshape(info.taps, info.up).T).astype(np.float32)


def step(info, m):
    """uc_rate_step: (k, p) of output sample m, by the library (no GPU)."""
    k, p = C.c_int64(), C.c_uint32()
    _check(lib().uc_rate_step(C.byref(info), int(m), C.byref(k), C.byref(p)), "uc_rate_step")
    return int(k.value), int(p.value)


def span(info, out_first, n_out):
    """uc_rate_span: (in_lo, in_hi), the input samples [in_lo, in_hi) that the outputs [out_first, out_first + n_out) read
    (in_lo < 0 near sample 0: those read as 0), by the library (no GPU)."""
    lo, hi = C.c_int64(), C.c_int64()
    _check(lib().uc_rate_span(C.byref(info), int(out_first), int(n_out), C.byref(lo), C.byref(hi)), "uc_rate_span")
    return int(lo.value), int(hi.value)


def count(info, n_in):
    """uc_rate_count: ceil(n_in * up / down), by the library (no GPU)."""
    return int(_check(lib().uc_rate_count(C.byref(info), int(n_in)), "uc_rate_count"))


def tile_outputs(info):
    """Outputs of one tile of the kernel for this ratio (csrc/uc_rate.hpp: tile_outputs); the tests cut calls around it."""
    return min(TILE_LANES, 1 + (WINDOW - info.taps) * info.up // info.down)


def model(x, up, down, half=24, beta=9.0, in_first=0, out_first=0, n_out=None, magnitude=False):
    """What Converter.convert writes, with the coefficients and the sums in float64: [n_rows, n_out] (1-d in, 1-d out).  The
    inputs are rounded to float32 first (the (float) cast); h is not rounded.  Samples outside [in_first, in_first + n_in)
    are 0.  n_out defaults to the outputs up to the row's end, ceil((in_first + n_in) up / down) - out_first.  With
    `magnitude` the sum of |h x| instead: what the rounding errors of a float evaluation scale with."""
    x = np.asarray(x)
    one = x.ndim == 1
    if x.ndim not in (1, 2):
        raise ValueError("x must be 1-d or 2-d")
    xf = np.atleast_2d(x).astype(np.float32).astype(np.float64)
    up, down, half, taps, centre, _ = plan_model(up, down, half, beta)
    h = _resample.design(up, down, half, float(beta))
    n_in = xf.shape[1]
    in_first, out_first = int(in_first), int(out_first)
    if n_out is None:
        n_out = -(-(in_first + n_in) * up // down) - out_first
    n_out = int(n_out)
    if n_out < 0 or out_first < 0 or out_first + n_out > SAMPLE_END_MAX:
        raise ValueError("out_first + n_out > 2^38")
    if magnitude:
        xf, h = np.abs(xf), np.abs(h)
    hp = np.concatenate([h, np.zeros(taps * up)])
    xp = np.concatenate([xf, np.zeros((xf.shape[0], 1))], axis=1)          # element n_in: the zero outside
    m = np.arange(out_first, out_first + n_out, dtype=np.int64)
    pos = m * down + centre
    k = pos // up
    p = pos - k * up
    y = np.zeros((xf.shape[0], n_out))
    for j in range(taps):
        i = k - j - in_first
        y += hp[p + j * up][None, :] * xp[:, np.where((i >= 0) & (i < n_in), i, n_in)]
    return y[0] if one else y


class Converter:
    """One uc_rate: the rate converter for one ratio on one MI355X."""

    def __init__(self, device, up, down, half=24, beta=9.0):
        h = C.c_void_p()
        _check(lib().uc_rate_create(int(device), int(up), int(down), int(half), float(beta), C.byref(h)), "uc_rate_create")
        self._h = h
        self.device = int(device)
        self.beta = float(beta)
        self.info = plan(up, down, half, beta)

    @classmethod
    def for_rates(cls, fs_in, fs_out=FS_OUT, device=0, half=24, beta=9.0):
        """The converter from fs_in to fs_out (both in whole Hz): 44 100 -> 78 125 is 3125 / 1764."""
        return cls(device, int(fs_out), int(fs_in), half, beta)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_rate_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def convert(self, x, in_first=0, out_first=0, n_out=None, out=None, stream=None):
        """uc_rate_convert: samples [out_first, out_first + n_out) of every row of x -> a float32 torch tensor [n_rows, n_out]
        on the object's device (or into `out`: a 2-d device tensor with contiguous rows).  `x`: a 2-d int16 / float32 device
        tensor with contiguous rows holding the samples from `in_first` on.  n_out defaults to the outputs up to the rows'
        end, ceil((in_first + n_in) up / down) - out_first.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int16) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int16 tensor on %s with contiguous rows" % dev)
        nr, n_in = int(x.shape[0]), int(x.shape[1])
        if out is None:
            if n_out is None:
                n_out = -(-(int(in_first) + n_in) * self.info.up // self.info.down) - int(out_first)
            out = torch.empty((nr, int(n_out)), dtype=torch.float32, device=dev)
        else:
            if (out.dim() != 2 or out.dtype != torch.float32 or out.device != dev or out.shape[0] != nr or
                    (out.shape[1] > 1 and out.stride(1) != 1) or (nr > 1 and out.stride(0) < out.shape[1])):
                raise ValueError("out must be a [%d, n_out] float32 tensor on %s with contiguous rows" % (nr, dev))
            if n_out is not None and int(n_out) != out.shape[1]:
                raise ValueError("n_out does not match out")
        no = int(out.shape[1])
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_rate_convert(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I16, nr,
                                     int(in_first), n_in, int(x.stride(0)) if nr > 1 else n_in, C.c_void_p(out.data_ptr()),
                                     int(out_first), no, int(out.stride(0)) if nr > 1 else no,
                                     C.c_void_p(stream) if stream else None), "uc_rate_convert")
        return out
