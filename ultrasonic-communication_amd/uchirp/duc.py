"""uchirp.duc -- the up-converter: binding of libuchirp_duc.so (include/uchirp_duc.h), its definition in numpy float32, a
float64 model, and a Kaiser-windowed interpolation prototype.

`Duc.run` puts many base-band rows (I, Q float pairs, or I alone) onto carriers on the GPU: every output row is the sum of
n_chan channels, each one input row interpolated by 1 .. 64 through a polyphase FIR of up to 128 taps per phase and multiplied
by the carrier of a 32-bit phase accumulator, as floats or as int16 PCM; the history of every input row is carried in a device
tensor, so that a stream is converted block by block, and with `row_map`, `set_index`, `steps` and `phases` one row goes onto
several carriers in one call.  It is the down-converter's (uchirp.ddc) other direction: y = I cos + Q sin, the sign that
`Ddc.run` undoes.  The carrier, the mixer and the sums are float32 with one rounding per operation, the chains one fused
multiply-add per tap, denormals kept: `emulate32` is the definition in numpy, and the GPU's values equal it bit for bit, as
do those of `filter_row` + `sum_row` (the library's plain-C functions).  There is no CPU path behind `Duc`; everything else
here needs no GPU.
"""
import ctypes as C

import numpy as np

from ._binding import Binding
from .ddc import fma32, step_of      # pure helpers: numpy alone, no library behind them

ABI_VERSION = 1
IN_IQ, IN_I = 0, 1
OUT_F32, OUT_I16 = 0, 1
MAX_PHASE_TAPS = 128
MAX_INTERP = 64
MAX_TAPS = 2048
MAX_SETS = 256
MAX_CHAN = 16
STATE_SAMPLES = 128
TABLE_WORDS = 2048
EXPORTS = ["uc_duc_abi_version", "uc_duc_last_error", "uc_duc_carrier_tables", "uc_duc_span", "uc_duc_filter_row", "uc_duc_sum_row",
           "uc_duc_create", "uc_duc_destroy", "uc_duc_set_taps", "uc_duc_run"]
_MASK = 0xFFFFFFFF


class DucError(RuntimeError):
    pass


def _declare(L):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.uc_duc_carrier_tables.argtypes = [fp, fp]
    L.uc_duc_span.argtypes = [C.c_int]
    L.uc_duc_filter_row.argtypes = [fp, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, fp, fp]
    L.uc_duc_sum_row.argtypes = [C.POINTER(fp), C.c_int, C.c_size_t, C.c_void_p, C.c_int, up]
    L.uc_duc_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.uc_duc_set_taps.argtypes = [C.c_void_p, fp, C.c_size_t, C.c_int, C.c_int]
    L.uc_duc_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_uint64, up, up, up, up,
                             C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]


_so = Binding("duc", DucError, _declare, env="UCHIRP_DUC_LIB")  # UCHIRP_DUC_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


# ----------------------------------------------------------------------------------------------------------------- design

def interp_taps(interp, k_taps, cutoff=0.45, beta=9.0):
    """A Kaiser-windowed sinc prototype at the output rate with gain L (so that the interpolated row keeps the input's
    level): float64 [k_taps * interp], the window uchirp.resample.design uses (np.kaiser with the same beta).  cutoff: the
    pass-band edge in cycles per INPUT sample, in (0, 0.5]."""
    L, K = int(interp), int(k_taps)
    if not (1 <= L <= MAX_INTERP and 1 <= K <= MAX_PHASE_TAPS and K * L <= MAX_TAPS):
        raise ValueError("interp 1 .. %d, k_taps 1 .. %d, k_taps * interp <= %d" % (MAX_INTERP, MAX_PHASE_TAPS, MAX_TAPS))
    if not 0.0 < float(cutoff) <= 0.5:
        raise ValueError("cutoff must lie in (0, 0.5] cycles per input sample")
    n = K * L
    m = np.arange(n) - (n - 1) / 2.0
    fe = float(cutoff) / L                                     # cycles per output sample
    return L * 2.0 * fe * np.sinc(2.0 * fe * m) * np.kaiser(n, float(beta))


def span(interp):
    """uc_duc_span: the outputs of one unit of the kernel's work at this interpolation."""
    return _check(lib().uc_duc_span(int(interp)), "uc_duc_span")


_tables = None


def tables():
    """uc_duc_carrier_tables: (coarse, fine), float32 [1024, 2] each: cos, sin of 2 pi i / 2^10 and of 2 pi f / 2^20."""
    global _tables
    if _tables is None:
        c, f = np.zeros(TABLE_WORDS, np.float32), np.zeros(TABLE_WORDS, np.float32)
        fp = C.POINTER(C.c_float)
        _check(lib().uc_duc_carrier_tables(c.ctypes.data_as(fp), f.ctypes.data_as(fp)), "uc_duc_carrier_tables")
        c.setflags(write=False)
        f.setflags(write=False)
        _tables = (c.reshape(1024, 2), f.reshape(1024, 2))
    return _tables


# ------------------------------------------------------------------------------------------------------ the definition

def samples32(x):
    """The input rule of include/uchirp_duc.h: float32 [rows, words] of the row's floats -- a complex array gives its
    interleaved I, Q pairs -- and what is not finite reads as +0."""
    a = np.asarray(x)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a.astype(np.complex64)).view(np.float32)
    else:
        a = a.astype(np.float32)
    return np.where(np.isfinite(a), a, np.float32(0.0))


def carrier32(phase):
    """The definition's (cos, sin) of uint32 phases: float32, every operation rounded once."""
    coarse, fine = tables()
    ph = np.asarray(phase, np.uint32)
    i, f = ph >> np.uint32(22), (ph >> np.uint32(12)) & np.uint32(1023)
    cc, sc, cf, sf = coarse[i, 0], coarse[i, 1], fine[f, 0], fine[f, 1]
    return (cc * cf) - (sc * sf), (sc * cf) + (cc * sf)


def phases32(first_out, count, step, phase0):
    """The phases of `count` outputs from the absolute OUTPUT index `first_out` on (it counts modulo 2^32): uint32
    [slots, count] for step, phase0 [slots]."""
    n = (np.uint64(int(first_out) & _MASK) + np.arange(count, dtype=np.uint64)) & np.uint64(_MASK)
    st = np.asarray(step, np.uint64).reshape(-1, 1)
    p0 = np.asarray(phase0, np.uint64).reshape(-1, 1)
    return ((p0 + st * n) & np.uint64(_MASK)).astype(np.uint32)


def to_int16(y):
    """The output stage UC_DUC_OUT_I16 in numpy: rint (ties to even), clamped to -32768 .. 32767, NaN -> 0 -> (int16 array,
    the number of values per row whose rounded value lay outside int16 or was NaN)."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(y)
        nan = np.isnan(y)
        clipped = nan | (r > 32767.0) | (r < -32768.0)
        out = np.clip(np.where(nan, np.float32(0.0), r), -32768.0, 32767.0).astype(np.int16)
    return out, clipped.sum(axis=-1).astype(np.uint32)


def _sets32(taps, interp):
    t = np.asarray(taps, np.float32)
    if t.ndim == 1:
        t = t[None]
    L = int(interp)
    if t.ndim != 2 or not 1 <= L <= MAX_INTERP or t.shape[1] % L or not 1 <= t.shape[1] // L <= MAX_PHASE_TAPS or t.shape[1] > MAX_TAPS \
            or not 1 <= t.shape[0] <= MAX_SETS:
        raise ValueError("taps must be [k_taps * interp] or [n_sets, k_taps * interp]: k_taps 1 .. %d, interp 1 .. %d, at most %d taps, %d sets"
                         % (MAX_PHASE_TAPS, MAX_INTERP, MAX_TAPS, MAX_SETS))
    if not np.isfinite(t).all():
        raise ValueError("a tap is not finite")
    return np.ascontiguousarray(t)


def _slots(v, n, name, default=0):
    if v is None:
        return np.full(n, default, np.uint64) if not isinstance(default, np.ndarray) else default
    a = np.asarray(v, np.int64).reshape(-1)
    if a.size == 1 and n != 1:
        a = np.repeat(a, n)
    if a.size != n or (a < 0).any() or (a > _MASK).any():
        raise ValueError("%s must hold %d uint32" % (name, n))
    return a.astype(np.uint64)


def _words(in_format):
    if in_format not in ("iq", "i"):
        raise ValueError("in_format must be 'iq' or 'i'")
    return 2 if in_format == "iq" else 1


def _rows32(x, in_format):
    """float32 [n_in_rows, n * words] and n"""
    w = _words(in_format)
    u = samples32(x)
    if u.ndim == 1:
        u = u[None]
    if u.ndim != 2 or u.shape[1] == 0 or u.shape[1] % w:
        raise ValueError("x must be [n_in_rows, n] complex, or float32 [n_in_rows, n * %d]" % w)
    return u, u.shape[1] // w


def _n_rows(n_in, n_chan, given):
    n_chan = int(n_chan)
    if not 1 <= n_chan <= MAX_CHAN:
        raise ValueError("n_chan must lie in 1 .. %d" % MAX_CHAN)
    slots = len(np.asarray(given[0]).reshape(-1)) if given else n_in
    if slots % n_chan or slots == 0:
        raise ValueError("%d channels do not fill rows of %d" % (slots, n_chan))
    return slots // n_chan, slots


def channels32(taps, x, interp, first=0, row_map=None, set_index=None, steps=None, phases=None, state=None, in_format="iq"):
    """One channel per entry of row_map / set_index / steps / phases (or per input row): the mixed rows y float32 [slots, n *
    interp] in front of the sum, and the new state float32 [n_in_rows, 128 * words]."""
    L = int(interp)
    h = _sets32(taps, L)
    K = h.shape[1] // L
    w = _words(in_format)
    u, n = _rows32(x, in_format)
    n_in = u.shape[0]
    if int(first) < 0 or (int(first) + n) * L > 2 ** 63:
        raise ValueError("(first + n) * interp > 2^63")
    given = [v for v in (row_map, set_index, steps, phases) if v is not None]
    slots = len(np.asarray(given[0]).reshape(-1)) if given else n_in
    rm = _slots(row_map, slots, "row_map", np.arange(slots, dtype=np.uint64)).astype(np.int64)
    si = _slots(set_index, slots, "set_index").astype(np.int64)
    if (rm >= n_in).any() or (si >= h.shape[0]).any():
        raise ValueError("row_map or set_index out of range")
    if state is None:
        st = np.zeros((n_in, STATE_SAMPLES * w), np.float32)
    else:
        st = np.array(state, np.float32).reshape(-1, STATE_SAMPLES * w)
        if st.shape[0] != n_in:
            raise ValueError("state must be [n_in_rows, %d]" % (STATE_SAMPLES * w))
    hist = np.concatenate([st, u], axis=1)                                       # [n_in, (128 + n) w]
    hk = h[si].reshape(slots, K, L)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        acc = []
        for part in range(w):
            z = hist[rm, part::w]                                                # [slots, 128 + n]
            a = np.zeros((slots, n, L), np.float32)
            for k in range(K):
                a = fma32(hk[:, None, k, :], z[:, STATE_SAMPLES - k:STATE_SAMPLES - k + n, None], a)
            acc.append(a.reshape(slots, n * L))
        c, s = carrier32(phases32(int(first) * L, n * L, _slots(steps, slots, "steps"), _slots(phases, slots, "phases")))
        y = (acc[0] * c) + (acc[1] * s) if w == 2 else acc[0] * c
    return y.astype(np.float32), np.ascontiguousarray(hist[:, n * w:])


def emulate32(taps, x, interp, first=0, n_chan=1, row_map=None, set_index=None, steps=None, phases=None, state=None, in_format="iq", out="f32"):
    """The definition of include/uchirp_duc.h in numpy float32, vectorised over channels: x complex64 [n_in_rows, n] (or float32
    [n_in_rows, 2 n] of I, Q pairs) for in_format="iq", float32 [n_in_rows, n] for "i" (1-d: one row), the first sample with
    the absolute input index `first`; taps [k_taps * interp] or [n_sets, k_taps * interp]; row_map, set_index, steps, phases:
    uint32 per channel, channel j of output row r at r * n_chan + j (None: input row r * n_chan + j, set 0, step 0, phase 0; a
    scalar: for all) -> (y, state, clipped): float32 [n_rows, n * interp] for out="f32", int16 for out="i16"; state float32
    [n_in_rows, 128 * words]; clipped uint32 [n_rows] (zeros for floats).  `state`: the carried state, zeros if None."""
    if out not in ("f32", "i16"):
        raise ValueError("out must be 'f32' or 'i16'")
    u, _ = _rows32(x, in_format)
    given = [v for v in (row_map, set_index, steps, phases) if v is not None and np.ndim(v) > 0]
    n_rows, slots = _n_rows(u.shape[0], n_chan, given)
    full = [None if v is None else _slots(v, slots, "a channel array") for v in (row_map, set_index, steps, phases)]
    if full[0] is None:
        full[0] = np.arange(slots, dtype=np.uint64)
    ych, st = channels32(taps, x, interp, first, full[0], full[1], full[2], full[3], state, in_format)
    ych = ych.reshape(n_rows, int(n_chan), -1)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = ych[:, 0]
        for j in range(1, int(n_chan)):
            y = y + ych[:, j]
    if out == "i16":
        y, clipped = to_int16(y)
    else:
        clipped = np.zeros(n_rows, np.uint32)
    return y, st, clipped


def model(taps, x, interp, first=0, freq=None, fs=1.0, step=0, phase=0, in_format="iq"):
    """One channel in float64 from rest: the row zero-stuffed by interp, a plain convolution with the float32 taps, times the
    exact cosine and sine of the full 32-bit phase at the output index (or, with `freq`, of 2 pi freq n / fs at the OUTPUT rate
    fs: the unquantised carrier): float64 [n_rows, n * interp] (1-d: one row)."""
    L = int(interp)
    h = _sets32(taps, L)[0].astype(np.float64)
    w = _words(in_format)
    one = np.asarray(x).ndim == 1
    u, n = _rows32(x, in_format)
    u = u.astype(np.float64)
    idx = int(first) * L + np.arange(n * L)
    if freq is not None:
        ang = 2.0 * np.pi * float(freq) / float(fs) * idx.astype(np.float64)
    else:
        ang = ((int(phase) + int(step) * idx.astype(object)) % 2 ** 32).astype(np.float64) * (2.0 * np.pi / 2.0 ** 32)
    out = np.zeros((u.shape[0], n * L))
    for part, trig in zip(range(w), (np.cos(ang), np.sin(ang))):
        for r in range(u.shape[0]):
            up = np.zeros(n * L)
            up[::L] = u[r, part::w]
            out[r] += np.convolve(up, h)[:n * L] * trig
    return out[0] if one else out


def filter_row(taps, x, interp, first=0, step=0, phase=0, state=None, in_format="iq"):
    """uc_duc_filter_row: one channel of the definition in plain C -> (y float32 [n * interp], state float32 [128 * words]),
    by the library (no GPU)."""
    L = int(interp)
    h = _sets32(taps, L)[0]
    w = _words(in_format)
    a = np.asarray(x)
    a = np.ascontiguousarray(a.astype(np.complex64)).view(np.float32) if np.iscomplexobj(a) else np.ascontiguousarray(a, np.float32)
    a = a.reshape(-1)
    n = a.size // w
    st = np.zeros(STATE_SAMPLES * w, np.float32) if state is None else np.ascontiguousarray(np.array(state, np.float32).reshape(STATE_SAMPLES * w))
    y = np.zeros(n * L, np.float32)
    fp = C.POINTER(C.c_float)
    _check(lib().uc_duc_filter_row(h.ctypes.data_as(fp), h.size // L, L, a.ctypes.data_as(C.c_void_p), IN_IQ if w == 2 else IN_I, n, int(first),
                                   int(step) & _MASK, int(phase) & _MASK, st.ctypes.data_as(fp), y.ctypes.data_as(fp)), "uc_duc_filter_row")
    return y, st


def sum_row(ys, out="f32"):
    """uc_duc_sum_row: the sum over channels and the output stage in plain C: ys float32 [n_chan, n] -> (float32 / int16 [n],
    the clipped count)."""
    ys = np.ascontiguousarray(np.asarray(ys, np.float32))
    if ys.ndim != 2:
        raise ValueError("ys must be [n_chan, n]")
    fp = C.POINTER(C.c_float)
    rows = (fp * ys.shape[0])(*[ys[j].ctypes.data_as(fp) for j in range(ys.shape[0])])
    res = np.zeros(ys.shape[1], np.int16 if out == "i16" else np.float32)
    clipped = C.c_uint32(0)
    _check(lib().uc_duc_sum_row(rows, ys.shape[0], ys.shape[1], res.ctypes.data_as(C.c_void_p), OUT_I16 if out == "i16" else OUT_F32, C.byref(clipped)),
           "uc_duc_sum_row")
    return res, int(clipped.value)


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


class Duc:
    """One uc_duc: the up-converter on one MI355X."""

    def __init__(self, taps=None, interp=1, device=0):
        h = C.c_void_p()
        _check(lib().uc_duc_create(int(device), C.byref(h)), "uc_duc_create")
        self._h = h
        self.device = int(device)
        self.n_sets = self.k_taps = self.interp = 0
        if taps is not None:
            self.set_taps(taps, interp)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_duc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_taps(self, taps, interp=1):
        """uc_duc_set_taps: one prototype [k_taps * interp] or several [n_sets, k_taps * interp] (rounded to float32) and the
        interpolation; they replace the object's.  Synchronous."""
        t = np.asarray(taps, np.float32)
        if t.ndim == 1:
            t = t[None]
        L = int(interp)
        if t.ndim != 2 or L < 1 or t.shape[1] % L:
            raise ValueError("taps must be [k_taps * interp] or [n_sets, k_taps * interp]")
        t = np.ascontiguousarray(t)
        _check(lib().uc_duc_set_taps(self._h, t.ctypes.data_as(C.POINTER(C.c_float)), t.shape[0], t.shape[1] // L, L), "uc_duc_set_taps")
        self.n_sets, self.k_taps, self.interp = int(t.shape[0]), int(t.shape[1] // L), L

    def new_state(self, n_in_rows, in_format="iq"):
        """The state of n_in_rows input rows at rest: zeros, float32 [n_in_rows, 128 * words] on the object's device."""
        import torch
        return torch.zeros((int(n_in_rows), STATE_SAMPLES * _words(in_format)), dtype=torch.float32, device=torch.device("cuda", self.device))

    def run(self, x, first=0, n_chan=1, steps=None, phases=None, row_map=None, set_index=None, state=None, in_format="iq", out="f32", y=None,
            clip=None, stream=None):
        """uc_duc_run: x [n_in_rows, n * words] (a 2-d float32 device tensor with contiguous rows: I, Q pairs for in_format="iq",
        I alone for "i"; or a 2-d complex64 tensor, which is its pairs), its first sample with the absolute input index `first`
        -> (y, state): the n * interp outputs of every output row, float32 for out="f32", int16 for out="i16"; and the carried
        state of the INPUT rows, float32 [n_in_rows, 128 * words], updated in place (zeros if None: filters at rest).  The
        channels are the entries of the first of row_map, set_index, steps, phases that is given (n_rows * n_chan of them), else
        the input rows.  `y`: a 2-d device tensor of the output's type with contiguous rows to write into; `clip`: an int32
        device tensor [n_rows] that gains the clipped counts of an int16 call.  Asynchronous on `stream` / torch's current
        stream."""
        import torch
        dev = torch.device("cuda", self.device)
        w = _words(in_format)
        if out not in ("f32", "i16"):
            raise ValueError("out must be 'f32' or 'i16'")
        if x.dim() == 2 and x.dtype == torch.complex64 and w == 2:
            x = torch.view_as_real(x).reshape(x.shape[0], -1) if x.is_contiguous() else torch.view_as_real(x.contiguous()).reshape(x.shape[0], -1)
        if (x.dim() != 2 or x.dtype != torch.float32 or x.device != dev or x.shape[1] == 0 or x.shape[1] % w or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("x must be a 2-d float32 (or complex64) tensor on %s with contiguous rows of n * %d floats" % (dev, w))
        n_in, n = int(x.shape[0]), int(x.shape[1]) // w
        given = [v for v in (row_map, set_index, steps, phases) if v is not None]
        nr, slots = _n_rows(n_in, n_chan, given)
        rm, rm_p = _u32(row_map, slots, "row_map")
        si, si_p = _u32(set_index, slots, "set_index")
        sp, sp_p = _u32(steps, slots, "steps")
        pp, pp_p = _u32(phases, slots, "phases")
        if state is None:
            state = self.new_state(n_in, in_format)
        elif state.dtype != torch.float32 or state.device != dev or tuple(state.shape) != (n_in, STATE_SAMPLES * w) or not state.is_contiguous():
            raise ValueError("state must be a contiguous [%d, %d] float32 tensor on %s" % (n_in, STATE_SAMPLES * w, dev))
        count = n * (self.interp or 1)
        dt = torch.float32 if out == "f32" else torch.int16
        if y is None:
            y = torch.empty((nr, count), dtype=dt, device=dev)
        elif (y.dim() != 2 or y.dtype != dt or y.device != dev or tuple(y.shape) != (nr, count) or (count > 1 and y.stride(1) != 1) or
              (nr > 1 and y.stride(0) < count)):
            raise ValueError("y must be a [%d, %d] %s tensor on %s with contiguous rows" % (nr, count, dt, dev))
        if clip is not None and (clip.dtype != torch.int32 or clip.device != dev or tuple(clip.shape) != (nr,) or not clip.is_contiguous()):
            raise ValueError("clip must be a contiguous [%d] int32 tensor on %s" % (nr, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_duc_run(self._h, C.c_void_p(x.data_ptr()), IN_IQ if w == 2 else IN_I, n_in, int(x.stride(0)) if n_in > 1 else 0, nr,
                                int(n_chan), n, int(first), rm_p, si_p, sp_p, pp_p, C.c_void_p(state.data_ptr()), C.c_void_p(y.data_ptr()),
                                OUT_F32 if out == "f32" else OUT_I16, int(y.stride(0)) if nr > 1 else 0,
                                C.c_void_p(clip.data_ptr()) if clip is not None else None, C.c_void_p(stream) if stream else None), "uc_duc_run")
        return y, state
