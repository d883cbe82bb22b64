"""uchirp.iir -- the recursive filter bank: binding of libuchirp_iir.so (include/uchirp_iir.h), its definition in numpy float32,
a float64 model, and Butterworth designs as second-order sections (no scipy).

`Iir.run` sends many rows (float, or DFSDM words) through cascades of 1 .. 8 biquad sections on the GPU, the state of every
row carried in a device tensor, so that a stream is filtered block by block; with `row_map` and `set_index` one row goes
through several coefficient sets in one call (a filter bank).  The arithmetic is float32, one rounding per operation, nothing
fused, denormals kept: `emulate32` is the definition in numpy, vectorised over rows, and the GPU's floats equal it bit for
bit, as do those of `filter_row` (the library's plain-C row function).  There is no CPU path behind `Iir`; everything else
here needs no GPU.

`lpf_sections` restates the reference's lpf() design (simulation/dsp.py: buttord(wp, 1.3 wp, 2, 30), then butter) as
sections; `dc_block_sections` and `bandpass_sections` are Butterworth high-pass and band-pass designs by the same route:
the analogue prototype's poles through the bilinear transform, pole pairs to sections, every section scaled to unity gain
in its pass band, sections in ascending order of pole radius.  The designs return float64; the filters round to float32.
"""
import ctypes as C
import math

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
MAX_SECTIONS = 8
MAX_SETS = 256
SECTION_WORDS = 5
STATE_WORDS = 16
EXPORTS = ["uc_iir_abi_version", "uc_iir_last_error", "uc_iir_filter_row", "uc_iir_create", "uc_iir_destroy", "uc_iir_set_sections",
           "uc_iir_run"]


class IirError(RuntimeError):
    pass


def _declare(L):
    L.uc_iir_filter_row.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.uc_iir_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_iir_set_sections.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int]
    L.uc_iir_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32),
                             C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


_so = Binding("iir", IirError, _declare, env="UCHIRP_IIR_LIB")  # UCHIRP_IIR_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


# ---------------------------------------------------------------------------------------------------------------- designs

def _prototype(order):
    """The Butterworth analogue prototype's poles: on the unit circle, in the left half plane."""
    return np.array([-np.exp(1j * np.pi * m / (2.0 * order)) for m in range(-order + 1, order, 2)])


def _bilinear(s):
    """s (in units of 2 fs) -> z"""
    return (1.0 + s) / (1.0 - s)


def _sections(poles, numerator, gain_at):
    """Poles in z -> float64 [n, 5]: a conjugate pair, or a real pole, per section, in ascending order of pole radius.
    `numerator`: (second-order, first-order) numerators before scaling; `gain_at`: the z at which every section has gain 1."""
    poles = np.asarray(poles, np.complex128)
    scale = np.abs(poles).max()
    real = np.abs(poles.imag) <= 1e-13 * scale
    rows = [(abs(z), -2.0 * z.real, abs(z) ** 2, numerator[0]) for z in poles[~real & (poles.imag > 0)]]
    singles = sorted(poles[real].real)
    if len(rows) * 2 + len(singles) != poles.size:
        raise ValueError("the poles are not conjugate pairs")
    if len(singles) > 1:
        raise ValueError("more than one real pole: the band is too wide for this route")
    if singles and numerator[1] is None:
        raise ValueError("a real pole: the band is too wide for this route")
    rows += [(abs(z), -z, 0.0, numerator[1]) for z in singles]
    rows.sort(key=lambda r: r[0])
    if not 1 <= len(rows) <= MAX_SECTIONS:
        raise ValueError("%d sections; a cascade holds 1 .. %d" % (len(rows), MAX_SECTIONS))
    out = np.zeros((len(rows), 5))
    zi = 1.0 / complex(gain_at)
    for k, (_, a1, a2, num) in enumerate(rows):
        g = abs(1.0 + a1 * zi + a2 * zi * zi) / abs(num[0] + num[1] * zi + num[2] * zi * zi)
        out[k] = [g * num[0], g * num[1], g * num[2], a1, a2]
    return out


def lpf_order(fs, cutoff):
    """(order, natural frequency as tan(pi f / fs)) of the reference's lpf(): buttord(wp, 1.3 wp, gpass 2, gstop 30)."""
    wp = float(cutoff) / (float(fs) / 2.0)
    ws = 1.3 * wp
    if not 0.0 < wp < ws < 1.0:
        raise ValueError("cutoff must lie in (0, fs / 2.6)")
    passb, stopb = math.tan(math.pi * wp / 2.0), math.tan(math.pi * ws / 2.0)
    gstop, gpass = 10.0 ** (0.1 * 30.0), 10.0 ** (0.1 * 2.0)
    order = int(math.ceil(math.log10((gstop - 1.0) / (gpass - 1.0)) / (2.0 * math.log10(stopb / passb))))
    wn = (gpass - 1.0) ** (-1.0 / (2.0 * order)) * passb      # exactly gpass at the pass-band edge
    return order, wn


def lpf_sections(fs, cutoff):
    """The reference's lpf(fs, ., cutoff) as sections: float64 [order / 2 rounded up, 5], unity gain at DC in every section."""
    order, wn = lpf_order(fs, cutoff)
    return _sections(_bilinear(wn * _prototype(order)), ((1.0, 2.0, 1.0), (1.0, 1.0, 0.0)), 1.0)


def dc_block_sections(fs, corner, order=1):
    """A Butterworth high-pass of `order` with its -3 dB point at `corner` Hz: unity gain at fs / 2 in every section, a zero
    at DC per pole.  Order 1 is the usual DC blocker."""
    if not 0.0 < corner < fs / 2.0 or order < 1:
        raise ValueError("corner must lie in (0, fs / 2), order >= 1")
    wn = math.tan(math.pi * float(corner) / float(fs))
    return _sections(_bilinear(wn / _prototype(int(order))), ((1.0, -2.0, 1.0), (1.0, -1.0, 0.0)), -1.0)


def bandpass_sections(fs, f_lo, f_hi, order):
    """A Butterworth band-pass of `order` (2 order poles: `order` sections) with its -3 dB points at f_lo and f_hi Hz: unity
    gain at the centre of the band in every section, a zero at DC and one at fs / 2 per section."""
    if not 0.0 < f_lo < f_hi < fs / 2.0 or order < 1:
        raise ValueError("0 < f_lo < f_hi < fs / 2 and order >= 1")
    w1, w2 = math.tan(math.pi * float(f_lo) / float(fs)), math.tan(math.pi * float(f_hi) / float(fs))
    half = 0.5 * (w2 - w1) * _prototype(int(order))
    root = np.sqrt(half * half - w1 * w2 + 0j)
    centre = np.exp(2j * math.atan(math.sqrt(w1 * w2)))
    return _sections(_bilinear(np.concatenate([half + root, half - root])), ((1.0, 0.0, -1.0), None), centre)


def response(sections, f, fs):
    """The cascade's frequency response at f Hz (array-like): complex128, from the coefficients as given."""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    zi = np.exp(-2j * np.pi * np.asarray(f, np.float64) / float(fs))
    h = np.ones_like(zi)
    for b0, b1, b2, a1, a2 in s:
        h = h * (b0 + b1 * zi + b2 * zi * zi) / (1.0 + a1 * zi + a2 * zi * zi)
    return h


def polynomials(sections):
    """(b, a) of the cascade as one rational function: the products of the sections' polynomials, float64."""
    b, a = np.ones(1), np.ones(1)
    for b0, b1, b2, a1, a2 in np.asarray(sections, np.float64).reshape(-1, 5):
        b, a = np.convolve(b, [b0, b1, b2]), np.convolve(a, [1.0, a1, a2])
    return b, a


# ------------------------------------------------------------------------------------------------------ the definition

def _sections32(sections):
    s = np.ascontiguousarray(np.asarray(sections, np.float32).reshape(-1, 5))
    if not 1 <= s.shape[0] <= MAX_SECTIONS:
        raise ValueError("a cascade holds 1 .. %d sections" % MAX_SECTIONS)
    if not np.isfinite(s).all():
        raise ValueError("a coefficient is not finite")
    return s


def samples32(x):
    """The input rule of include/uchirp_iir.h: int32 are DFSDM words, (float)(word >> 8); anything else is rounded to float32,
    and what is not finite reads as +0."""
    a = np.asarray(x)
    if a.dtype == np.int32:
        return (a >> 8).astype(np.float32)
    a = a.astype(np.float32)
    return np.where(np.isfinite(a), a, np.float32(0.0))


def _state_of(state, rows):
    if state is None:
        return np.zeros((rows, STATE_WORDS), np.float32)
    s = np.array(state, np.float32).reshape(-1, STATE_WORDS)
    if s.shape[0] != rows:
        raise ValueError("state must be [n_rows, %d]" % STATE_WORDS)
    return s


def emulate32(sections, x, state=None, flush=False):
    """The definition of include/uchirp_iir.h in numpy float32 (every operation rounded once, nothing fused, denormals kept),
    vectorised over rows: x float32 / int32 [n_rows, n] (1-d: one row) -> (out float32 [n_rows, n], state float32
    [n_rows, 16]).  `state`: the carried state, zeros if None; the words of sections that do not exist pass through.
    `flush`: what the definition is NOT -- every denormal operand and result replaced by a zero of its sign, as a
    flush-to-zero device computes; tests use it to prove that their inputs tell the two apart."""
    c = _sections32(sections)
    u_all = samples32(x)
    one = u_all.ndim == 1
    if u_all.ndim not in (1, 2):
        raise ValueError("x must be a 1-d or 2-d array")
    u_all = np.atleast_2d(u_all)
    rows, n = u_all.shape
    st = _state_of(state, rows)
    tiny = np.finfo(np.float32).tiny

    def ftz(v):
        return np.where(np.abs(v) < tiny, np.copysign(np.float32(0.0), v), v) if flush else v

    z = [ftz(st[:, k].copy()) if k < 2 * c.shape[0] else st[:, k].copy() for k in range(STATE_WORDS)]
    out = np.zeros((rows, n), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(n):
            u = ftz(u_all[:, j])
            for s, (b0, b1, b2, a1, a2) in enumerate(c):
                o = ftz(ftz(b0 * u) + z[2 * s])
                z[2 * s] = ftz(ftz(ftz(b1 * u) - ftz(a1 * o)) + z[2 * s + 1])
                z[2 * s + 1] = ftz(ftz(b2 * u) - ftz(a2 * o))
                u = o
            out[:, j] = u
    st = np.stack(z, axis=1).astype(np.float32)
    return (out[0], st[0]) if one else (out, st)


def model(sections, x):
    """The same recurrence in float64 on the float32 coefficients and the samples of the input rule, from rest:
    float64 [n_rows, n] (1-d: one row)."""
    c = _sections32(sections).astype(np.float64)
    u_all = samples32(x).astype(np.float64)
    one = u_all.ndim == 1
    u_all = np.atleast_2d(u_all)
    rows, n = u_all.shape
    z = np.zeros((2 * c.shape[0], rows))
    out = np.zeros((rows, n))
    for j in range(n):
        u = u_all[:, j]
        for s, (b0, b1, b2, a1, a2) in enumerate(c):
            o = b0 * u + z[2 * s]
            z[2 * s] = (b1 * u - a1 * o) + z[2 * s + 1]
            z[2 * s + 1] = b2 * u - a2 * o
            u = o
        out[:, j] = u
    return out[0] if one else out


def filter_row(sections, x, state=None):
    """uc_iir_filter_row: the definition in plain C for one row (float32 or int32 DFSDM words) -> (out float32 [n], state
    float32 [16]), by the library (no GPU)."""
    c = np.ascontiguousarray(np.asarray(sections, np.float32).reshape(-1, 5))
    a = np.asarray(x)
    a = np.ascontiguousarray(a, np.int32 if a.dtype == np.int32 else np.float32).reshape(-1)
    st = np.ascontiguousarray(_state_of(state, 1)[0])
    out = np.zeros(a.size, np.float32)
    _check(lib().uc_iir_filter_row(c.ctypes.data_as(C.POINTER(C.c_float)), c.shape[0], a.ctypes.data_as(C.c_void_p),
                                   DTYPE_I32 if a.dtype == np.int32 else DTYPE_F32, a.size, st.ctypes.data_as(C.POINTER(C.c_float)),
                                   out.ctypes.data_as(C.POINTER(C.c_float))), "uc_iir_filter_row")
    return out, st


# -------------------------------------------------------------------------------------------------------------- the object

def _u32(v, n, name):
    if v is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(v, np.int64).reshape(-1))
    if a.size != n or (a < 0).any() or (a > 0xFFFFFFFF).any():
        raise ValueError("%s must hold %d row numbers" % (name, n))
    a = a.astype(np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


class Iir:
    """One uc_iir: the recursive filter bank on one MI355X."""

    def __init__(self, sections=None, device=0):
        h = C.c_void_p()
        _check(lib().uc_iir_create(int(device), C.byref(h)), "uc_iir_create")
        self._h = h
        self.device = int(device)
        self.n_sets = self.n_sections = 0
        if sections is not None:
            self.set_sections(sections)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_iir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sections(self, sections):
        """uc_iir_set_sections: one set [n_sections, 5] or several [n_sets, n_sections, 5] (rounded to float32); they replace
        the object's sets.  Synchronous."""
        s = np.asarray(sections, np.float32)
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or s.shape[2] != SECTION_WORDS:
            raise ValueError("sections must be [n_sections, 5] or [n_sets, n_sections, 5]")
        s = np.ascontiguousarray(s)
        _check(lib().uc_iir_set_sections(self._h, s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[0], s.shape[1]), "uc_iir_set_sections")
        self.n_sets, self.n_sections = int(s.shape[0]), int(s.shape[1])

    def new_state(self, n_rows):
        """The state of n_rows filters at rest: zeros, float32 [n_rows, 16] on the object's device."""
        import torch
        return torch.zeros((int(n_rows), STATE_WORDS), dtype=torch.float32, device=torch.device("cuda", self.device))

    def run(self, rows, state=None, out=None, row_map=None, set_index=None, stream=None):
        """uc_iir_run: rows [n_in_rows, n] (a 2-d float32 / int32 device tensor with contiguous rows; int32 are DFSDM words)
        -> (out, state): float32 [n_rows, n] and the carried state, float32 [n_rows, 16], updated in place (zeros if None:
        filters at rest).  n_rows is len(row_map) or len(set_index) where given, else n_in_rows; output row r reads input
        row row_map[r] through set set_index[r].  `out`: a 2-d float32 device tensor with contiguous rows to write into.
        Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        x = rows
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("rows must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        n_in, n = int(x.shape[0]), int(x.shape[1])
        nr = len(row_map) if row_map is not None else len(set_index) if set_index is not None else n_in
        rm, rm_p = _u32(row_map, nr, "row_map")
        si, si_p = _u32(set_index, nr, "set_index")
        if state is None:
            state = self.new_state(nr)
        elif state.dtype != torch.float32 or state.device != dev or tuple(state.shape) != (nr, STATE_WORDS) or not state.is_contiguous():
            raise ValueError("state must be a contiguous [%d, %d] float32 tensor on %s" % (nr, STATE_WORDS, dev))
        if out is None:
            out = torch.empty((nr, n), dtype=torch.float32, device=dev)
        elif (out.dim() != 2 or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (nr, n) or
              (n > 1 and out.stride(1) != 1) or (nr > 1 and out.stride(0) < n)):
            raise ValueError("out must be a [%d, %d] float32 tensor on %s with contiguous rows" % (nr, n, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_iir_run(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, n_in,
                                int(x.stride(0)) if n_in > 1 else n, nr, n, rm_p, si_p, C.c_void_p(state.data_ptr()),
                                C.c_void_p(out.data_ptr()), int(out.stride(0)) if nr > 1 else n, C.c_void_p(stream) if stream else None),
               "uc_iir_run")
        return out, state
