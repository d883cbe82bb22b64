"""uchirp.mf -- the pulse compressor: binding of libuchirp_mf.so (include/uchirp_mf.h), its float64 model and an independent
float32 evaluation of the same definition.

`Mf.run` filters many rows -- float32, int32 DFSDM words or complex64 (what `Ddc.run` writes) -- with known pulses:
y[q] = sum_k h[k] x[q - k], `scipy.signal.lfilter(h, 1, x)`, by overlap-save on 2048-point transforms on the GPU, several
templates per row in one call (a job is a (row, set) pair).  Beside the outputs, or instead of them, it leaves one small
record per (job, segment of S = 2047 - T outputs): the four greatest local maxima of the power, each with its two
neighbours, the segment's summed power and counts.  `arrivals` turns records into fractional positions and heights.  A
matched filter is `matched(pulse)`: the reversed conjugate.  There is no CPU path behind `Mf`; `plan`, `spectrum`,
`select`, `arrival`, `model`, `emulate32`, `select_model` and `arrivals` need no GPU.

Positions are absolute: element j of a row is sample pos0 + j, and segment k covers the outputs k S .. k S + S - 1.
"""
import ctypes as C

import numpy as np

from ._binding import Binding
from .ddc import fma32

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32, DTYPE_C32 = 0, 1, 2
OUT_COMPLEX, OUT_REAL, OUT_POWER, OUT_MAG = 0, 1, 2, 3
FORMATS = {"complex": OUT_COMPLEX, "real": OUT_REAL, "power": OUT_POWER, "mag": OUT_MAG}
POINTS = 2048
MAX_TAPS = 1664
MAX_SETS = 256
CANDIDATES = 4
ERROR_C = 9
EXPORTS = ["uc_mf_abi_version", "uc_mf_last_error", "uc_mf_create", "uc_mf_destroy", "uc_mf_set_templates", "uc_mf_run",
           "uc_mf_plan", "uc_mf_spectrum", "uc_mf_select", "uc_mf_arrival"]

JOB_DTYPE = np.dtype([("row", np.uint32), ("set", np.uint32)])
CANDIDATE_DTYPE = np.dtype([("offset", np.uint32), ("left", np.float32), ("peak", np.float32), ("right", np.float32)])
RECORD_DTYPE = np.dtype([("cand", CANDIDATE_DTYPE, (CANDIDATES,)), ("sum", np.float32), ("count", np.uint32), ("n_cand", np.uint32),
                         ("reserved", np.uint32)])


class MfJob(C.Structure):
    """struct uc_mf_job (include/uchirp_mf.h)."""
    _fields_ = [("row", C.c_uint32), ("set", C.c_uint32)]


class MfCandidate(C.Structure):
    """struct uc_mf_candidate (include/uchirp_mf.h)."""
    _fields_ = [("offset", C.c_uint32), ("left", C.c_float), ("peak", C.c_float), ("right", C.c_float)]


class MfRecord(C.Structure):
    """struct uc_mf_record (include/uchirp_mf.h)."""
    _fields_ = [("cand", MfCandidate * CANDIDATES), ("sum", C.c_float), ("count", C.c_uint32), ("n_cand", C.c_uint32),
                ("reserved", C.c_uint32)]


class MfError(RuntimeError):
    pass


def _declare(L):
    L.uc_mf_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_mf_set_templates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.uc_mf_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64,
                            C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    L.uc_mf_plan.argtypes = [C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                             C.POINTER(C.c_uint64)]
    L.uc_mf_spectrum.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.uc_mf_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.uc_mf_arrival.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]


_so = Binding("mf", MfError, _declare, env="UCHIRP_MF_LIB")  # UCHIRP_MF_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


# ---------------------------------------------------------------------------------------------------------- templates

def matched(pulse):
    """The matched filter of a pulse: its reversed conjugate, complex128 [T]."""
    return np.conj(np.asarray(pulse, np.complex128).reshape(-1)[::-1])


def chirp(f0, f1, fs, duration, amplitude=1.0, phase=0.0, inclusive=False):
    """A linear chirp: amplitude * exp(i (2 pi (f0 + (f1 - f0) t / (2 duration)) t + phase)) at n = int(duration fs) instants,
    complex128; f0 > f1 is a down chirp.  The instants are t = m / fs; with `inclusive` they are the notebook's, n points
    from 0 to `duration` itself (ChirpSimulation.ipynb: its time axis ends on the last sample)."""
    n = int(float(duration) * float(fs))
    t = np.linspace(0.0, float(duration), n) if inclusive else np.arange(n, dtype=np.float64) / float(fs)
    k = (float(f1) - float(f0)) / float(duration)
    return float(amplitude) * np.exp(1j * (2.0 * np.pi * (float(f0) + 0.5 * k * t) * t + float(phase)))


def chirp_template(f0, f1, fs, duration, carrier=None, window=None, pad_to=None):
    """The matched filter of a chirp f0 -> f1 Hz of `duration` seconds at the rate fs: real (float64, as complex128 with a
    zero imaginary part) without a carrier; with `carrier` the base-band pulse exp(i ...) with the carrier taken out, as
    `Ddc.run` leaves it.  window: None or "hann"; pad_to: zero taps behind the template up to this length (denser records)."""
    if carrier is None:
        p = chirp(f0, f1, fs, duration).real.astype(np.complex128)
    else:
        p = chirp(float(f0) - float(carrier), float(f1) - float(carrier), fs, duration)
    if window == "hann":
        p = p * (0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(p.size) + 0.5) / p.size))
    elif window is not None:
        raise ValueError("window must be None or 'hann'")
    h = matched(p)
    if pad_to is not None:
        if int(pad_to) < h.size:
            raise ValueError("pad_to below the template's length")
        h = np.concatenate([h, np.zeros(int(pad_to) - h.size, np.complex128)])
    return h


def _taps(taps):
    """[n_sets, T] complex64 from one set [T] or several"""
    t = np.asarray(taps)
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2 or not (1 <= t.shape[0] <= MAX_SETS and 1 <= t.shape[1] <= MAX_TAPS):
        raise ValueError("taps must be [T] or [n_sets, T], n_sets 1 .. %d, T 1 .. %d" % (MAX_SETS, MAX_TAPS))
    return np.ascontiguousarray(t.astype(np.complex64))


# ----------------------------------------------------------------------------------------------------- host functions

def plan(n_taps, pos0, first, n):
    """uc_mf_plan: (hop S, first_segment, n_segments) of a call."""
    hop, k0, ns = C.c_uint32(), C.c_uint64(), C.c_uint64()
    _check(lib().uc_mf_plan(int(n_taps), int(pos0), int(first), int(n), C.byref(hop), C.byref(k0), C.byref(ns)), "uc_mf_plan")
    return int(hop.value), int(k0.value), int(ns.value)


def spectrum(taps):
    """uc_mf_spectrum: H of the definition for one set, complex64 [2048], by the library (no GPU)."""
    t = _taps(taps)
    if t.shape[0] != 1:
        raise ValueError("one set")
    out = np.zeros(POINTS, np.complex64)
    _check(lib().uc_mf_spectrum(t.ctypes.data_as(C.c_void_p), t.shape[1], out.ctypes.data_as(C.c_void_p)), "uc_mf_spectrum")
    return out


def select(e, lo=0, hi=None):
    """uc_mf_select: the record of one segment from e [S + 2] (float32: the powers of the outputs -1 .. S), the outputs
    lo .. hi - 1 in range: a RECORD_DTYPE scalar, by the library (no GPU)."""
    a = np.ascontiguousarray(e, np.float32).reshape(-1)
    hop = a.size - 2
    hi = hop if hi is None else int(hi)
    out = np.zeros(1, RECORD_DTYPE)
    _check(lib().uc_mf_select(a.ctypes.data_as(C.c_void_p), max(hop, 0), int(lo), hi, out.ctypes.data_as(C.c_void_p)), "uc_mf_select")
    return out[0]


def select_model(e, lo=0, hi=None):
    """The selection rule of include/uchirp_mf.h in numpy: the same record as `select` (its sum in ascending order)."""
    a = np.asarray(e, np.float32).reshape(-1)
    hop = a.size - 2
    hi = hop if hi is None else int(hi)
    lo = int(lo)
    if not (hop >= 1 and 0 <= lo < hi <= hop):
        raise ValueError("outputs out of range")
    u = np.arange(lo, hi)
    l, v, r = a[u], a[u + 1], a[u + 2]
    is_c = (v >= l) & (v > r)
    cu = u[is_c]
    order = np.lexsort((cu, -a[cu + 1].astype(np.float64)))[:CANDIDATES]        # by falling e, then by rising q
    out = np.zeros(1, RECORD_DTYPE)[0]
    for m, i in enumerate(cu[order]):
        out["cand"][m] = (i, a[i], a[i + 1], a[i + 2])
    s = np.float32(0.0)
    for x in v:
        s = np.float32(s + x)
    out["sum"], out["count"], out["n_cand"] = s, hi - lo, int(is_c.sum())
    return out


def arrival(cand):
    """uc_mf_arrival: (offset, height) of one candidate (a CANDIDATE_DTYPE scalar or an (offset, left, peak, right) tuple)."""
    c = MfCandidate(int(cand[0]), float(cand[1]), float(cand[2]), float(cand[3]))
    off, top = C.c_double(), C.c_double()
    _check(lib().uc_mf_arrival(C.byref(c), C.byref(off), C.byref(top)), "uc_mf_arrival")
    return off.value, top.value


def arrival_model(cand):
    """The arrival of include/uchirp_mf.h in Python floats."""
    a, b, c = (float(np.sqrt(np.float64(v))) for v in (cand[1], cand[2], cand[3]))
    d = a - 2.0 * b + c
    if d < 0.0:
        delta = (a - c) / (2.0 * d)
        return float(cand[0]) + delta, b - (a - c) * delta / 4.0
    return float(cand[0]), b


def arrivals(records, plan_, min_ratio=0.0):
    """Records [n_jobs, n_segments] (RECORD_DTYPE) and the call's plan (hop, first_segment, n_segments) -> per job a list of
    (position, height): every kept candidate with peak >= min_ratio * sum / count of its segment, the position absolute
    (first_segment + segment) * hop + fitted offset, the height that of the fitted amplitude; by rising position."""
    rec = np.asarray(records)
    if rec.dtype != RECORD_DTYPE or rec.ndim != 2:
        raise ValueError("records must be [n_jobs, n_segments] of RECORD_DTYPE")
    hop, k0, ns = plan_
    if rec.shape[1] != ns:
        raise ValueError("records of %d segments, the plan has %d" % (rec.shape[1], ns))
    out = []
    for row in rec:
        found = []
        for s, r in enumerate(row):
            floor = float(min_ratio) * float(r["sum"]) / max(int(r["count"]), 1)
            for m in range(min(int(r["n_cand"]), CANDIDATES)):
                c = r["cand"][m]
                if float(c["peak"]) >= floor:
                    off, top = arrival_model((c["offset"], c["left"], c["peak"], c["right"]))
                    found.append(((k0 + s) * hop + off, top))
        out.append(sorted(found))
    return out


# ------------------------------------------------------------------------------------------------------ the definition

def samples(x):
    """The input rule: int32 are DFSDM words cast with (float); complex input is rounded to complex64, anything else to
    float32.  Returns complex64 / float32 [n_rows, n_in]."""
    a = np.asarray(x)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2:
        raise ValueError("x must be 1-d or 2-d")
    return a.astype(np.complex64) if np.iscomplexobj(a) else a.astype(np.float32)


def _jobs(jobs, n_rows=None):
    if isinstance(jobs, np.ndarray) and jobs.dtype == JOB_DTYPE:
        return np.ascontiguousarray(jobs)
    j = np.zeros(len(jobs), JOB_DTYPE)
    for i, (r, s) in enumerate(jobs):
        j[i] = (int(r), int(s))
    return j


def _range(n_in, first, n):
    first = int(first)
    n = n_in - first if n is None else int(n)
    if not (first >= 0 and n >= 1 and first + n <= n_in):
        raise ValueError("first or n out of range")
    return first, n


def model(x, taps, jobs=None, first=0, n=None, exact=False):
    """What Mf.run writes as complex, in float64 by np.convolve: complex128 [n_jobs, n].  The inputs and the taps are rounded
    to float32 first, as the library reads them; with `exact` they are taken as they are (float64: the notebook's own
    lfilter).  jobs defaults to every row through set 0.  (pos0 does not enter: y of element j is what it is.)"""
    if exact:
        u, h = np.atleast_2d(np.asarray(x)).astype(np.complex128), np.atleast_2d(np.asarray(taps)).astype(np.complex128)
    else:
        u, h = samples(x).astype(np.complex128), _taps(taps).astype(np.complex128)
    jb = _jobs([(r, 0) for r in range(u.shape[0])] if jobs is None else jobs)
    first, n = _range(u.shape[1], first, n)
    return np.stack([np.convolve(u[int(r)], h[int(s)])[first:first + n] for r, s in zip(jb["row"], jb["set"])])


def windows(x_row, hop, n_taps, pos0, segment):
    """a_k of the definition for one row (1-d), as it is: elements k S - T - pos0 .. + 2047 of the row, zeros outside."""
    start = int(segment) * int(hop) - int(n_taps) - int(pos0)
    out = np.zeros(POINTS, x_row.dtype)
    lo, hi = max(start, 0), min(start + POINTS, x_row.size)
    if hi > lo:
        out[lo - start:hi - start] = x_row[lo:hi]
    return out


def bound(x, taps, jobs=None, pos0=0, first=0, n=None):
    """||a_k||_2 ||h||_2 for every output of a call: what the header's error form scales with, float64 [n_jobs, n]."""
    u = samples(x).astype(np.complex128)
    h = _taps(taps).astype(np.complex128)
    jb = _jobs([(r, 0) for r in range(u.shape[0])] if jobs is None else jobs)
    first, n = _range(u.shape[1], first, n)
    hop = POINTS - h.shape[1] - 1
    k0 = (int(pos0) + first) // hop
    q = int(pos0) + first + np.arange(n)
    seg = q // hop
    out = np.zeros((len(jb), n))
    for i, (r, s) in enumerate(zip(jb["row"], jb["set"])):
        hn = np.linalg.norm(h[int(s)])
        for k in range(k0, int(seg[-1]) + 1):
            out[i, seg == k] = np.linalg.norm(windows(u[int(r)], hop, h.shape[1], pos0, k)) * hn
    return out


def power32(y):
    """e of the definition from complex64 y: fmaf(re, re, im * im), the product rounded first."""
    y = np.asarray(y, np.complex64)
    return fma32(y.real, y.real, y.imag * y.imag)


def emulate32(x, taps, jobs=None, pos0=0, first=0, n=None, spectra=None):
    """The definition's structure -- windows of 2048 elements every S outputs, transform, times H, inverse transform -- with
    scipy.fft (pocketfft) in single precision: an independent float32 evaluation, there only so that tests have a
    yardstick for what float32 can do.  Returns (y complex64 [n_jobs, n], e float32 [n_jobs, n_segments, S + 2]): e holds
    every segment's powers of the outputs -1 .. S, what `select_model` reads."""
    import scipy.fft
    u = samples(x)
    t = _taps(taps)
    jb = _jobs([(r, 0) for r in range(u.shape[0])] if jobs is None else jobs)
    first, n = _range(u.shape[1], first, n)
    T = t.shape[1]
    hop = POINTS - T - 1
    q0 = int(pos0) + first
    k0, k1 = q0 // hop, (q0 + n - 1) // hop
    H = [spectrum(t[s]) for s in range(t.shape[0])] if spectra is None else spectra
    y = np.zeros((len(jb), n), np.complex64)
    e = np.zeros((len(jb), k1 - k0 + 1, hop + 2), np.float32)
    for i, (r, s) in enumerate(zip(jb["row"], jb["set"])):
        for k in range(k0, k1 + 1):
            a = windows(u[int(r)], hop, T, pos0, k).astype(np.complex64)
            A = scipy.fft.fft(a)
            assert A.dtype == np.complex64
            z = scipy.fft.ifft(A * H[int(s)], norm="forward")               # not normalised: H holds the 1 / P
            assert z.dtype == np.complex64
            e[i, k - k0] = power32(z[T - 1:])
            lo, hi = max(k * hop, q0), min(k * hop + hop, q0 + n)
            y[i, lo - q0:hi - q0] = z[T + lo - k * hop:T + hi - k * hop]
    return y, e


# -------------------------------------------------------------------------------------------------------------- the object

class Mf:
    """One uc_mf: the pulse compressor on one MI355X."""

    def __init__(self, taps=None, device=0):
        h = C.c_void_p()
        _check(lib().uc_mf_create(int(device), C.byref(h)), "uc_mf_create")
        self._h = h
        self.device = int(device)
        self.n_sets = self.n_taps = 0
        if taps is not None:
            self.set_templates(taps)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_mf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_templates(self, taps):
        """uc_mf_set_templates: one set [T] or several [n_sets, T] (rounded to complex64); they replace the object's.
        Synchronous."""
        t = _taps(taps)
        _check(lib().uc_mf_set_templates(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1]), "uc_mf_set_templates")
        self.n_sets, self.n_taps = int(t.shape[0]), int(t.shape[1])

    def plan(self, pos0=0, first=0, n=1):
        return plan(self.n_taps, pos0, first, n)

    def run(self, x, jobs=None, pos0=0, first=0, n=None, out="complex", records=True, y=None, stream=None):
        """uc_mf_run: x [n_rows, n_in] (a 2-d float32 / int32 / complex64 device tensor with contiguous rows), element j the
        sample pos0 + j -> (y, records).  y: the outputs pos0 + first .. + n - 1 of every job, [n_jobs, n], complex64 for
        out="complex", float32 for "real", "power", "mag"; None for out=None.  records: an int32 device tensor
        [n_jobs, n_segments, 20] (`records_of` makes RECORD_DTYPE of its host copy), None for records=False.  jobs: (row, set)
        pairs or a JOB_DTYPE array; default: every row through set 0.  `y`: a 2-d device tensor of the format's type with
        contiguous rows to write into.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        kinds = {torch.float32: DTYPE_F32, torch.int32: DTYPE_I32, torch.complex64: DTYPE_C32}
        if (x.dim() != 2 or x.dtype not in kinds or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 / complex64 tensor on %s with contiguous rows" % dev)
        if out is not None and out not in FORMATS:
            raise ValueError("out must be one of %s or None" % sorted(FORMATS))
        if out is None and not records:
            raise ValueError("nothing to compute: out is None and records is False")
        nr, n_in = int(x.shape[0]), int(x.shape[1])
        jb = _jobs([(r, 0) for r in range(nr)] if jobs is None else jobs)
        nj = len(jb)
        first = int(first)
        n = n_in - first if n is None else int(n)
        if first < 0 or n < 0 or int(pos0) < 0:
            raise ValueError("pos0, first and n must not be negative")
        ydt = torch.complex64 if out == "complex" else torch.float32
        if out is None:
            y = None
        elif y is None:
            y = torch.empty((nj, n), dtype=ydt, device=dev)
        elif (y.dim() != 2 or y.dtype != ydt or y.device != dev or tuple(y.shape) != (nj, n) or (n > 1 and y.stride(1) != 1) or
              (nj > 1 and y.stride(0) < n)):
            raise ValueError("y must be a [%d, %d] %s tensor on %s with contiguous rows" % (nj, n, ydt, dev))
        rec = None
        if records:
            ns = plan(self.n_taps, pos0, first, n)[2] if self.n_taps and n >= 1 and first + n <= n_in else 1
            rec = torch.empty((nj, ns, RECORD_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_mf_run(self._h, C.c_void_p(x.data_ptr()), kinds[x.dtype], nr, n_in, int(x.stride(0)) if nr > 1 else n_in,
                               jb.ctypes.data_as(C.c_void_p), nj, int(pos0), first, n,
                               C.c_void_p(y.data_ptr()) if y is not None else None, FORMATS[out] if out is not None else OUT_COMPLEX,
                               int(y.stride(0)) if y is not None and nj > 1 else 0,
                               C.c_void_p(rec.data_ptr()) if rec is not None else None, C.c_void_p(stream) if stream else None), "uc_mf_run")
        return y, rec


def records_of(rec):
    """The host copy of Mf.run's record tensor as RECORD_DTYPE [n_jobs, n_segments]."""
    a = np.ascontiguousarray(rec.cpu().numpy() if hasattr(rec, "cpu") else rec)
    return a.view(RECORD_DTYPE).reshape(a.shape[0], a.shape[1])
