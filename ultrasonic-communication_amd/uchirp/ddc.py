"""uchirp.ddc -- the down-converter: binding of libuchirp_ddc.so (include/uchirp_ddc.h), its definition in numpy float32, a
float64 model, and the notebook's low-pass design.

`Ddc.run` multiplies many rows (float, or DFSDM words) by the carriers of 32-bit phase accumulators, runs the products through
a FIR of 1 .. 128 taps and decimates by 1 .. 64 on the GPU, to complex base-band rows or to the I chain alone; the history of
every input row is carried in a device tensor, so that a stream is converted block by block, and with `row_map`, `set_index`,
`steps` and `phases` one row is converted at several carriers in one call.  The carrier and the mixer are float32 with one
rounding per operation, the chains one fused multiply-add per tap, denormals kept: `emulate32` is the definition in numpy,
vectorised over rows, and the GPU's floats equal it bit for bit, as do those of `filter_row` (the library's plain-C row
function).  There is no CPU path behind `Ddc`; everything else here needs no GPU.

`lpf_taps` restates the reference's design (simulation/FIR LPF design.ipynb): fe = cutoff / fs, round(3.1 / (4 fe)) taps made
odd, 2 fe sinc(2 pi fe m) centred; the firmware's 27 taps are the unwindowed ones (the notebook prints b, not b w).
"""
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
OUT_IQ, OUT_I = 0, 1
MAX_TAPS = 128
MAX_DECIM = 64
MAX_SETS = 256
STATE_WORDS = 128
TABLE_WORDS = 2048
EXPORTS = ["uc_ddc_abi_version", "uc_ddc_last_error", "uc_ddc_carrier_tables", "uc_ddc_outputs", "uc_ddc_span", "uc_ddc_filter_row",
           "uc_ddc_create", "uc_ddc_destroy", "uc_ddc_set_taps", "uc_ddc_run"]
_MASK = 0xFFFFFFFF


class DdcError(RuntimeError):
    pass


def _declare(L):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.uc_ddc_carrier_tables.argtypes = [fp, fp]
    L.uc_ddc_outputs.argtypes = [C.c_uint64, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    L.uc_ddc_span.argtypes = [C.c_int]
    L.uc_ddc_filter_row.argtypes = [fp, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, fp, fp, C.c_int]
    L.uc_ddc_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_ddc_set_taps.argtypes = [C.c_void_p, fp, C.c_size_t, C.c_int, C.c_int]
    L.uc_ddc_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64, up, up, up, up,
                             C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]


_so = Binding("ddc", DdcError, _declare, env="UCHIRP_DDC_LIB")  # UCHIRP_DDC_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


# ----------------------------------------------------------------------------------------------------------------- design

def hanning_window(n):
    """The notebook's window: 0.5 - 0.5 cos(2 pi (m + 0.5) / n) for an odd n, 0.5 - 0.5 cos(2 pi m / n) for an even one,
    m = 0 .. n - 1."""
    m = np.arange(int(n)) + (0.5 if int(n) % 2 else 0.0)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * m / int(n))


def lpf_taps(fs, cutoff, n_taps=None, window=None):
    """The notebook's low-pass: float64 [n_taps].  n_taps: round(3.1 / (4 fe)) made odd unless given; window: None (what the
    firmware holds) or "hann"."""
    fe = float(cutoff) / float(fs)
    if not 0.0 < fe < 0.5:
        raise ValueError("cutoff must lie in (0, fs / 2)")
    if n_taps is None:
        n_taps = int(round(3.1 / (4.0 * fe)))
        n_taps += 1 - n_taps % 2
    n_taps = int(n_taps)
    if not 1 <= n_taps <= MAX_TAPS:
        raise ValueError("%d taps; a set holds 1 .. %d" % (n_taps, MAX_TAPS))
    m = np.arange(n_taps) - (n_taps - 1) / 2.0
    b = 2.0 * fe * np.sinc(2.0 * fe * m)                      # numpy's sinc(x) = sin(pi x) / (pi x)
    if window == "hann":
        b = b * hanning_window(n_taps)
    elif window is not None:
        raise ValueError("window must be None or 'hann'")
    return b


def step_of(freq, fs):
    """The phase step of `freq` Hz at the rate fs: round(freq / fs 2^32) mod 2^32 (a negative frequency: two's complement)."""
    return int(round(float(freq) / float(fs) * 2.0 ** 32)) & _MASK


def outputs(first, n, decim):
    """uc_ddc_outputs: (the first absolute output index, the number of outputs) of a call of n samples from `first` on."""
    p, c = C.c_uint64(), C.c_size_t()
    _check(lib().uc_ddc_outputs(int(first), int(n), int(decim), C.byref(p), C.byref(c)), "uc_ddc_outputs")
    return int(p.value), int(c.value)


def span(decim):
    """uc_ddc_span: the outputs of one unit of the kernel's work at this decimation."""
    return _check(lib().uc_ddc_span(int(decim)), "uc_ddc_span")


_tables = None


def tables():
    """uc_ddc_carrier_tables: (coarse, fine), float32 [1024, 2] each: cos, sin of 2 pi i / 2^10 and of 2 pi f / 2^20."""
    global _tables
    if _tables is None:
        c, f = np.zeros(TABLE_WORDS, np.float32), np.zeros(TABLE_WORDS, np.float32)
        fp = C.POINTER(C.c_float)
        _check(lib().uc_ddc_carrier_tables(c.ctypes.data_as(fp), f.ctypes.data_as(fp)), "uc_ddc_carrier_tables")
        c.setflags(write=False)
        f.setflags(write=False)
        _tables = (c.reshape(1024, 2), f.reshape(1024, 2))
    return _tables


# ------------------------------------------------------------------------------------------------------ the definition

def samples32(x):
    """The input rule of include/uchirp_ddc.h: int32 are DFSDM words, (float)(word >> 8); anything else is rounded to float32,
    and what is not finite reads as +0."""
    a = np.asarray(x)
    if a.dtype == np.int32:
        return (a >> 8).astype(np.float32)
    a = a.astype(np.float32)
    return np.where(np.isfinite(a), a, np.float32(0.0))


def phases32(first, count, step, phase0):
    """The phases of `count` samples from the absolute index `first` on (any integer; it counts modulo 2^32): uint32
    [rows, count] for step, phase0 [rows]."""
    n = (np.uint64(int(first) & _MASK) + np.arange(count, dtype=np.uint64)) & np.uint64(_MASK)
    st = np.asarray(step, np.uint64).reshape(-1, 1)
    p0 = np.asarray(phase0, np.uint64).reshape(-1, 1)
    return ((p0 + st * n) & np.uint64(_MASK)).astype(np.uint32)


def carrier32(phase):
    """The definition's (cos, sin) of uint32 phases: float32, every operation rounded once."""
    coarse, fine = tables()
    ph = np.asarray(phase, np.uint32)
    i, f = ph >> np.uint32(22), (ph >> np.uint32(12)) & np.uint32(1023)
    cc, sc, cf, sf = coarse[i, 0], coarse[i, 1], fine[f, 0], fine[f, 1]
    return (cc * cf) - (sc * sf), (sc * cf) + (cc * sf)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64; the sum is rounded to odd there (its error from the
    two-sum), so that the rounding to float32 behind it is the one rounding of the exact value."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        if fix.any():
            up = (e > 0.0) == (s > 0.0)                       # away from zero: the next larger magnitude
            s = (s.view(np.int64) + np.where(fix, np.where(up, 1, -1), 0)).view(np.float64)
        return s.astype(np.float32)


def _state_of(state, rows):
    if state is None:
        return np.zeros((rows, STATE_WORDS), np.float32)
    s = np.array(state, np.float32).reshape(-1, STATE_WORDS)
    if s.shape[0] != rows:
        raise ValueError("state must be [n_rows, %d]" % STATE_WORDS)
    return s


def _taps32(taps):
    h = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
    if not 1 <= h.size <= MAX_TAPS:
        raise ValueError("a set holds 1 .. %d taps" % MAX_TAPS)
    if not np.isfinite(h).all():
        raise ValueError("a tap is not finite")
    return h


def _per_row(v, rows, name):
    if v is None:
        return np.zeros(rows, np.uint64)
    a = np.asarray(v, np.int64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, rows)
    if a.size != rows or (a < 0).any() or (a > _MASK).any():
        raise ValueError("%s must hold %d uint32" % (name, rows))
    return a.astype(np.uint64)


def _span_of(first, n, decim):
    """(p_first, count, lead) in Python integers: the outputs of a call and the first one's sample, counted from in[0]."""
    first, n, decim = int(first), int(n), int(decim)
    if not 1 <= decim <= MAX_DECIM:
        raise ValueError("decim must lie in 1 .. %d" % MAX_DECIM)
    p_first = -(-first // decim)
    last = (first + n - 1) // decim
    return p_first, max(0, last - p_first + 1), p_first * decim - first


def emulate32(taps, x, decim=1, first=0, steps=None, phases=None, state=None, out="iq"):
    """The definition of include/uchirp_ddc.h in numpy float32, vectorised over rows: x float32 / int32 [n_rows, n] (1-d: one
    row), the first sample with the absolute index `first`, every row against its own carrier (steps, phases: uint32 per row,
    a scalar for all, None: 0) through one tap set -> (y, state): complex64 [n_rows, count] for out="iq" (real: I, imaginary:
    Q), float32 for out="i"; state float32 [n_rows, 128].  `state`: the carried state, zeros if None."""
    h = _taps32(taps)
    u = samples32(x)
    one = u.ndim == 1
    if u.ndim not in (1, 2) or out not in ("iq", "i"):
        raise ValueError("x must be a 1-d or 2-d array, out 'iq' or 'i'")
    u = np.atleast_2d(u)
    rows, n = u.shape
    if n == 0:
        raise ValueError("no samples")
    hist = np.concatenate([_state_of(state, rows), u], axis=1)
    ph = phases32(int(first) - STATE_WORDS, STATE_WORDS + n, _per_row(steps, rows, "steps"), _per_row(phases, rows, "phases"))
    c, s = carrier32(ph)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        mixed = [hist * c] + ([hist * s] if out == "iq" else [])
        _, count, lead = _span_of(first, n, decim)
        acc = [np.zeros((rows, count), np.float32) for _ in mixed]
        if count:
            for k in range(h.size):
                a = STATE_WORDS + lead - k
                for j, m in enumerate(mixed):
                    acc[j] = fma32(h[k], m[:, a:a + (count - 1) * decim + 1:decim], acc[j])
    if out == "iq":
        y = np.empty((rows, count), np.complex64)
        y.real, y.imag = acc[0], acc[1]
    else:
        y = acc[0]
    st = np.ascontiguousarray(hist[:, n:])
    return (y[0], st[0]) if one else (y, st)


def model(taps, x, decim=1, first=0, freq=None, fs=1.0, steps=None, phases=None, out="iq"):
    """The same in float64 from rest: the exact cosine and sine of the full 32-bit phase (or, with `freq`, of 2 pi freq n /
    fs: the unquantised carrier), a plain convolution with the float32 taps: complex128 / float64 [n_rows, count] (1-d: one
    row)."""
    h = _taps32(taps).astype(np.float64)
    u = samples32(x).astype(np.float64)
    one = u.ndim == 1
    u = np.atleast_2d(u)
    rows, n = u.shape
    if freq is not None:
        ang = 2.0 * np.pi * float(freq) / float(fs) * (int(first) + np.arange(n, dtype=np.float64))[None, :]
    else:
        ang = phases32(first, n, _per_row(steps, rows, "steps"), _per_row(phases, rows, "phases")).astype(np.float64) * (2.0 * np.pi / 2.0 ** 32)
    z = u * (np.cos(ang) + 1j * np.sin(ang))
    _, count, lead = _span_of(first, n, decim)
    full = np.stack([np.convolve(r, h)[:n] for r in z])
    y = full[:, lead:lead + (count - 1) * decim + 1:decim] if count else np.zeros((rows, 0), np.complex128)
    if out == "i":
        y = y.real
    return y[0] if one else y


def filter_row(taps, x, decim=1, first=0, step=0, phase=0, state=None, out="iq"):
    """uc_ddc_filter_row: the definition in plain C for one row (float32 or int32 DFSDM words) -> (y complex64 / float32
    [count], state float32 [128]), by the library (no GPU)."""
    h = _taps32(taps)
    a = np.asarray(x)
    a = np.ascontiguousarray(a, np.int32 if a.dtype == np.int32 else np.float32).reshape(-1)
    st = np.ascontiguousarray(_state_of(state, 1)[0])
    _, count, _ = _span_of(first, a.size, decim)
    y = np.zeros(count * (2 if out == "iq" else 1), np.float32)
    fp = C.POINTER(C.c_float)
    _check(lib().uc_ddc_filter_row(h.ctypes.data_as(fp), h.size, int(decim), a.ctypes.data_as(C.c_void_p),
                                   DTYPE_I32 if a.dtype == np.int32 else DTYPE_F32, a.size, int(first), int(step) & _MASK, int(phase) & _MASK,
                                   st.ctypes.data_as(fp), y.ctypes.data_as(fp), OUT_IQ if out == "iq" else OUT_I), "uc_ddc_filter_row")
    return (y.view(np.complex64) if out == "iq" else y), st


# -------------------------------------------------------------------------------------------------------------- the object

def _u32(v, n, name):
    if v is None:
        return None, None
    if isinstance(v, np.ndarray) and v.dtype == np.uint32 and v.ndim == 1 and v.flags.c_contiguous and v.size == n:
        return v, v.ctypes.data_as(C.POINTER(C.c_uint32))        # (as it is: a caller in a loop converts once)
    a = np.ascontiguousarray(np.asarray(v, np.int64).reshape(-1))
    if a.size != n or (a < 0).any() or (a > _MASK).any():
        raise ValueError("%s must hold %d uint32" % (name, n))
    a = a.astype(np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


class Ddc:
    """One uc_ddc: the down-converter on one MI355X."""

    def __init__(self, taps=None, decim=1, device=0):
        h = C.c_void_p()
        _check(lib().uc_ddc_create(int(device), C.byref(h)), "uc_ddc_create")
        self._h = h
        self.device = int(device)
        self.n_sets = self.n_taps = self.decim = 0
        if taps is not None:
            self.set_taps(taps, decim)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_ddc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_taps(self, taps, decim=1):
        """uc_ddc_set_taps: one set [n_taps] or several [n_sets, n_taps] (rounded to float32) and the decimation; they replace
        the object's.  Synchronous."""
        t = np.asarray(taps, np.float32)
        if t.ndim == 1:
            t = t[None]
        if t.ndim != 2:
            raise ValueError("taps must be [n_taps] or [n_sets, n_taps]")
        t = np.ascontiguousarray(t)
        _check(lib().uc_ddc_set_taps(self._h, t.ctypes.data_as(C.POINTER(C.c_float)), t.shape[0], t.shape[1], int(decim)), "uc_ddc_set_taps")
        self.n_sets, self.n_taps, self.decim = int(t.shape[0]), int(t.shape[1]), int(decim)

    def new_state(self, n_in_rows):
        """The state of n_in_rows input rows at rest: zeros, float32 [n_in_rows, 128] on the object's device."""
        import torch
        return torch.zeros((int(n_in_rows), STATE_WORDS), dtype=torch.float32, device=torch.device("cuda", self.device))

    def run(self, x, first=0, steps=None, phases=None, row_map=None, set_index=None, state=None, out="iq", y=None, stream=None):
        """uc_ddc_run: x [n_in_rows, n] (a 2-d float32 / int32 device tensor with contiguous rows; int32 are DFSDM words), its
        first sample with the absolute index `first` -> (y, state): the outputs that outputs(first, n, decim) names, complex64
        [n_rows, count] for out="iq" (a view of the I, Q pairs), float32 for out="i"; and the carried state of the INPUT rows,
        float32 [n_in_rows, 128], updated in place (zeros if None: filters at rest).  n_rows is the length of the first of
        row_map, set_index, steps, phases that is given, else n_in_rows.  `y`: a 2-d float32 device tensor with contiguous
        rows of count (or 2 count) floats to write into; the return value is then a view of it.  Asynchronous on `stream` /
        torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        if out not in ("iq", "i"):
            raise ValueError("out must be 'iq' or 'i'")
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        n_in, n = int(x.shape[0]), int(x.shape[1])
        given = [v for v in (row_map, set_index, steps, phases) if v is not None]
        nr = len(given[0]) if given else n_in
        rm, rm_p = _u32(row_map, nr, "row_map")
        si, si_p = _u32(set_index, nr, "set_index")
        sp, sp_p = _u32(steps, nr, "steps")
        pp, pp_p = _u32(phases, nr, "phases")
        if state is None:
            state = self.new_state(n_in)
        elif state.dtype != torch.float32 or state.device != dev or tuple(state.shape) != (n_in, STATE_WORDS) or not state.is_contiguous():
            raise ValueError("state must be a contiguous [%d, %d] float32 tensor on %s" % (n_in, STATE_WORDS, dev))
        _, count, _ = _span_of(first, n, self.decim or 1)
        words = count * (2 if out == "iq" else 1)
        if y is None:
            y = torch.empty((nr, max(words, 1)), dtype=torch.float32, device=dev)[:, :words]
        elif (y.dim() != 2 or y.dtype != torch.float32 or y.device != dev or tuple(y.shape) != (nr, words) or
              (words > 1 and y.stride(1) != 1) or (nr > 1 and y.stride(0) < words)):
            raise ValueError("y must be a [%d, %d] float32 tensor on %s with contiguous rows" % (nr, words, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        # (a call without outputs still names a buffer, and an empty tensor has no address)
        target = y if words else torch.empty(2, dtype=torch.float32, device=dev)
        _check(lib().uc_ddc_run(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, n_in,
                                int(x.stride(0)) if n_in > 1 else n, nr, n, int(first), rm_p, si_p, sp_p, pp_p, C.c_void_p(state.data_ptr()),
                                C.c_void_p(target.data_ptr()), OUT_IQ if out == "iq" else OUT_I, int(y.stride(0)) if nr > 1 and words else 0,
                                C.c_void_p(stream) if stream else None), "uc_ddc_run")
        if out == "iq":
            if count == 0:
                return torch.empty((nr, 0), dtype=torch.complex64, device=dev), state
            if y.is_contiguous() and y.data_ptr() % 8 == 0:
                return torch.view_as_complex(y.view(nr, count, 2)), state
            return torch.complex(y[:, 0::2], y[:, 1::2]), state      # (rows off 8 bytes: no complex view of them exists)
        return y, state
