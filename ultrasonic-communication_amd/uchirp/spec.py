"""uchirp.spec -- the spectrum analyser: binding of libuchirp_spec.so (include/uchirp_spec.h), its float64 model and an
independent float32 evaluation.

The firmware's first look at a recording is `fft()` (experiments/basic/Src/main.c:107-175): Hann window, 2048-point
transform, magnitude / sqrt(N), the bins below 1 kHz forced to 1, 10 log10, the frequency of the maximum; the notebooks draw
spectrograms.  `Analyser.spectra` is that for many rows at once on the GPU: every frame of every row -> its windowed
2048-point magnitude, power or level spectrum, any sub-range of the bins, and each frame's largest stored value with its
bin.  There is no CPU path behind `Analyser`; `frames`, `plan` (the library's host functions), `model`, `emulate32`, `freqs`
and `times` need no GPU.
"""
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAG, POWER, DB = 0, 1, 2
POINTS, BINS = 2048, 1025
ERROR_C = 200                     # UC_SPEC_ERROR_C
LOG10_ERROR = 5.0e-6              # UC_SPEC_LOG10_ERROR
EXPORTS = ["uc_spec_abi_version", "uc_spec_last_error", "uc_spec_frames", "uc_spec_plan", "uc_spec_create", "uc_spec_destroy",
           "uc_spec_set_window", "uc_spec_run"]
KINDS = {"mag": MAG, "power": POWER, "db": DB, MAG: MAG, POWER: POWER, DB: DB}


class SpecParams(C.Structure):
    """struct uc_spec_params (include/uchirp_spec.h)."""
    _fields_ = [("first", C.c_int64), ("n_frames", C.c_uint64), ("frame_len", C.c_uint32), ("hop", C.c_uint32),
                ("bin_first", C.c_uint32), ("n_bins", C.c_uint32), ("ac_bins", C.c_uint32), ("kind", C.c_int32),
                ("scale", C.c_float), ("floor", C.c_float), ("db_mul", C.c_float), ("reserved", C.c_uint32)]


class SpecInfo(C.Structure):
    """struct uc_spec_info (include/uchirp_spec.h)."""
    _fields_ = [("n_frames", C.c_uint64), ("out_stride", C.c_uint64), ("out_elems", C.c_uint64), ("bin_first", C.c_uint32),
                ("n_bins", C.c_uint32)]

    def __repr__(self):
        return "SpecInfo(n_frames=%d, out_stride=%d, out_elems=%d, bin_first=%d, n_bins=%d)" % (
            self.n_frames, self.out_stride, self.out_elems, self.bin_first, self.n_bins)


PEAK_DTYPE = np.dtype([("value", np.float32), ("bin", np.uint32)])     # struct uc_spec_peak


class SpecError(RuntimeError):
    pass


def _declare(L):
    L.uc_spec_frames.argtypes = [C.c_uint64, C.c_int64, C.c_uint32, C.c_uint32]
    L.uc_spec_frames.restype = C.c_int64
    L.uc_spec_plan.argtypes = [C.POINTER(SpecParams), C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(SpecInfo)]
    L.uc_spec_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_spec_set_window.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]
    L.uc_spec_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(SpecParams), C.c_void_p,
                              C.c_size_t, C.c_void_p, C.c_void_p]


_so = Binding("spec", SpecError, _declare, env="UCHIRP_SPEC_LIB")  # UCHIRP_SPEC_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def params(frame_len=POINTS, hop=None, first=0, n_frames=0, bin_first=0, n_bins=None, ac_bins=0, kind=MAG, scale=1.0, floor=1e-20,
           db_mul=10.0):
    """A SpecParams; hop defaults to frame_len, n_bins to the bins from bin_first up to 1024, n_frames 0 means all."""
    return SpecParams(int(first), int(n_frames), int(frame_len), int(frame_len if hop is None else hop), int(bin_first),
                      int(BINS - bin_first if n_bins is None else n_bins), int(ac_bins), int(KINDS[kind]), float(scale), float(floor),
                      float(db_mul), 0)


def frames(n_in, first=0, frame_len=POINTS, hop=None):
    """uc_spec_frames: the frames f >= 0 whose first sample first + f hop lies below n_in, by the library (no GPU)."""
    return int(_check(lib().uc_spec_frames(int(n_in), int(first), int(frame_len), int(frame_len if hop is None else hop)), "uc_spec_frames"))


def plan(p, n_rows, n_in, out_stride=0):
    """uc_spec_plan: the SpecInfo of a SpecParams (frames, bins, output elements), by the library (no GPU)."""
    info = SpecInfo()
    _check(lib().uc_spec_plan(C.byref(p), int(n_rows), int(n_in), int(out_stride), C.byref(info)), "uc_spec_plan")
    return info


def hann(frame_len=POINTS):
    """The default window: the periodic Hann, (float)(0.5 - 0.5 cos(2 pi i / frame_len)) evaluated in double."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(frame_len), dtype=np.float64) / int(frame_len))).astype(np.float32)


def freqs(fs, bin_first=0, n_bins=None):
    """The bins' frequencies in Hz: k fs / 2048."""
    n_bins = BINS - bin_first if n_bins is None else n_bins
    return np.arange(bin_first, bin_first + n_bins, dtype=np.float64) * (float(fs) / POINTS)


def times(fs, n_frames, first=0, hop=POINTS):
    """The frames' first samples in seconds: (first + f hop) / fs."""
    return (int(first) + np.arange(int(n_frames), dtype=np.float64) * int(hop)) / float(fs)


def _frames_of(x, window, frame_len, hop, first, n_frames, dtype):
    """u[row, frame, i] = w[i] x[first + f hop + i], zero outside the row and from frame_len on; x cast to float32 first."""
    x = np.asarray(x)
    if x.ndim not in (1, 2):
        raise ValueError("x must be 1-d or 2-d")
    xf = np.atleast_2d(x).astype(np.float32)
    n_in = xf.shape[1]
    frame_len = int(frame_len)
    hop = frame_len if hop is None else int(hop)
    first = int(first)
    w = hann(frame_len) if window is None else np.asarray(window, dtype=np.float32)
    if not 1 <= frame_len <= POINTS or w.shape != (frame_len,) or hop < 1 or not -frame_len < first < n_in:
        raise ValueError("a frame_len, window, hop or first that include/uchirp_spec.h refuses")
    count = -(-(n_in - first) // hop)
    n_frames = count if not n_frames else int(n_frames)
    if n_frames > count:
        raise ValueError("n_frames above the frames of the row")
    idx = first + hop * np.arange(n_frames)[:, None] + np.arange(frame_len)[None, :]
    inside = (idx >= 0) & (idx < n_in)
    xp = np.concatenate([xf, np.zeros((xf.shape[0], 1), np.float32)], axis=1)        # element n_in: the zero outside
    u = np.zeros((xf.shape[0], n_frames, POINTS), dtype)
    u[:, :, :frame_len] = xp[:, np.where(inside, idx, n_in)].astype(dtype) * w.astype(dtype)[None, None, :]
    return u, x.ndim == 1


def _values(v, kind, ac_bins, floor, db_mul, bin_first, n_bins, dtype):
    v = v.astype(dtype)
    v[..., :min(int(ac_bins), BINS)] = 1.0
    kind = KINDS[kind]
    if kind == POWER:
        v = v * v
    elif kind == DB:
        v = (dtype(db_mul) * np.log10(np.maximum(v, dtype(np.float32(floor))))).astype(dtype)
    n_bins = BINS - bin_first if n_bins is None else n_bins
    if n_bins < 1 or bin_first < 0 or bin_first + n_bins > BINS:
        raise ValueError("a bin range outside 0 .. 1024")
    return v[..., bin_first:bin_first + n_bins]


def model(x, window=None, frame_len=POINTS, hop=None, first=0, n_frames=0, bin_first=0, n_bins=None, ac_bins=0, kind=MAG, scale=1.0,
          floor=1e-20, db_mul=10.0, norm=False):
    """What Analyser.spectra writes, in float64: [rows, frames, bins] (1-d in: [frames, bins]).  The inputs, the window and
    the scale are rounded to float32 first; the product, the transform and the values are float64.  With `norm` the frames'
    ||u||_2 instead, [rows, frames]: what the error form scales with."""
    u, one = _frames_of(x, window, frame_len, hop, first, n_frames, np.float64)
    if norm:
        r = np.sqrt((u * u).sum(axis=2))
        return r[0] if one else r
    v = float(np.float32(scale)) * np.abs(np.fft.rfft(u, axis=2))
    v = _values(v, kind, ac_bins, floor, float(np.float32(db_mul)), bin_first, n_bins, np.float64)
    return v[0] if one else v


def emulate32(x, window=None, frame_len=POINTS, hop=None, first=0, n_frames=0, bin_first=0, n_bins=None, ac_bins=0, kind=MAG, scale=1.0,
              floor=1e-20, db_mul=10.0):
    """An independent float32 evaluation of the same definition: numpy's float32 rfft of the float32 product, float32
    values.  The error constant of include/uchirp_spec.h is four times the worst ratio it reaches against `model`."""
    u, one = _frames_of(x, window, frame_len, hop, first, n_frames, np.float32)
    X = np.fft.rfft(u, axis=2)
    if X.dtype != np.complex64:
        raise RuntimeError("numpy's rfft did not stay in float32")
    v = np.float32(scale) * np.sqrt(X.imag * X.imag + X.real * X.real)
    v = _values(v, kind, ac_bins, floor, db_mul, bin_first, n_bins, np.float32)
    return v[0] if one else v


def error_ratio(got, x, window=None, frame_len=POINTS, hop=None, first=0, n_frames=0, scale=1.0, bin_first=0, n_bins=None):
    """The error form's ratio of a MAG result: max |got - model| / (2^-24 |scale| ||u||_2) per frame, [rows, frames]; a frame of
    zeros has ratio 0 if it is zeros and inf if not."""
    kw = dict(window=window, frame_len=frame_len, hop=hop, first=first, n_frames=n_frames)
    x = np.atleast_2d(np.asarray(x))
    want = model(x, scale=scale, bin_first=bin_first, n_bins=n_bins, **kw)
    unit = 2.0 ** -24 * abs(float(np.float32(scale))) * model(x, norm=True, **kw)
    err = np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))


class Analyser:
    """One uc_spec: the spectrum analyser on one MI355X.  Its window starts as the periodic Hann of 2048 values."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().uc_spec_create(int(device), C.byref(h)), "uc_spec_create")
        self._h = h
        self.device = int(device)
        self._window = ("hann", POINTS)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_spec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_window(self, window=None, frame_len=None):
        """uc_spec_set_window: a float array (its length is the frame length from now on), or -- window None -- the periodic
        Hann of frame_len values."""
        if window is None:
            n = POINTS if frame_len is None else int(frame_len)
            _check(lib().uc_spec_set_window(self._h, None, n), "uc_spec_set_window")
            self._window = ("hann", n)
        else:
            w = np.ascontiguousarray(window, dtype=np.float32)
            if w.ndim != 1 or (frame_len is not None and int(frame_len) != w.size):
                raise ValueError("window must be 1-d and frame_len values long")
            _check(lib().uc_spec_set_window(self._h, w.ctypes.data_as(C.POINTER(C.c_float)), w.size), "uc_spec_set_window")
            self._window = ("own", w.size)

    @property
    def frame_len(self):
        return self._window[1]

    def spectra(self, x, hop=None, first=0, n_frames=0, bin_first=0, n_bins=None, ac_bins=0, kind=MAG, scale=1.0, floor=1e-20,
                db_mul=10.0, out=None, peaks=False, stream=None):
        """uc_spec_run: the spectra of every frame of every row of x -> a float32 torch tensor [rows, frames, bins] on the
        object's device (or into `out`: such a tensor whose last dimension is contiguous and whose rows and frames are
        evenly spaced, out.stride(0) == frames * out.stride(1)).  `x`: a 2-d int32 / float32 device tensor with contiguous
        rows.  The frame length is that of the object's window (set_window).  With `peaks` the pair (spectra, records): a
        numpy-viewable uint8 tensor [rows, frames, 8] of struct uc_spec_peak (see `peaks_of`).  Asynchronous on `stream` /
        torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nr, n_in = int(x.shape[0]), int(x.shape[1])
        p = params(self.frame_len, hop, first, n_frames, bin_first, n_bins, ac_bins, kind, scale, floor, db_mul)
        info = plan(p, nr, n_in)
        nf, nb = int(info.n_frames), int(info.n_bins)
        if out is None:
            out = torch.empty((nr, nf, nb), dtype=torch.float32, device=dev)
        elif (out.dim() != 3 or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (nr, nf, nb) or
              (nb > 1 and out.stride(2) != 1) or (nf > 1 and out.stride(1) < nb) or (nr > 1 and out.stride(0) != nf * out.stride(1))):
            raise ValueError("out must be a [%d, %d, %d] float32 tensor on %s with evenly spaced frames" % (nr, nf, nb, dev))
        ostride = int(out.stride(1)) if nf > 1 else (int(out.stride(0)) if nr > 1 else nb)
        rec = torch.empty((nr, nf, 8), dtype=torch.uint8, device=dev) if peaks else None
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_spec_run(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nr, n_in,
                                 int(x.stride(0)) if nr > 1 else n_in, C.byref(p), C.c_void_p(out.data_ptr()), ostride,
                                 C.c_void_p(rec.data_ptr()) if peaks else None, C.c_void_p(stream) if stream else None), "uc_spec_run")
        return (out, rec) if peaks else out

    def spectrogram(self, x, fs, hop=None, first=0, **kw):
        """(freqs [bins], times [frames], spectra [rows, frames, bins]) of `spectra`: what a plot needs."""
        s = self.spectra(x, hop=hop, first=first, **kw)
        hop = self.frame_len if hop is None else hop
        return freqs(fs, kw.get("bin_first", 0), s.shape[2]), times(fs, s.shape[1], first, hop), s


def peaks_of(rec):
    """The records of `Analyser.spectra(..., peaks=True)` as a numpy structured array [rows, frames] with `value`, `bin`."""
    a = rec.cpu().numpy()
    return a.reshape(a.shape[0], a.shape[1] * 8).view(PEAK_DTYPE).reshape(a.shape[0], a.shape[1])
