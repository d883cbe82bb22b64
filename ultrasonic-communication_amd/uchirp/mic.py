"""uchirp.mic -- the MEMS-microphone model: binding of libuchirp_mic.so (include/uchirp_mic.h) and its definition in numpy
integers.

The chain this project serves starts at the microphones' 1-bit PDM streams.  `Mic.modulate` turns many rows of samples at
78 125 Hz (float, or DFSDM words) into those streams on the GPU: one packed word of 32 bits per sample, through a second-order
delta-sigma modulator in int32 arithmetic, into a device tensor that `Engine.receive_many(..., pdm=True)`,
`LiveStreams.next(..., pdm=True)` and `Engine.dfsdm_streams` read in place.  The arithmetic is exact: `model` is the
definition in numpy int32, vectorised over rows, and the GPU's words equal it bit for bit.  There is no CPU path behind `Mic`;
`quantise`, `modulate_row` (the library's host functions), `model` and `linear` need no GPU.
"""
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
DTYPE_I32, DTYPE_F32 = 0, 1
Q_MAX = 2 ** 23 - 1
Y = 2 ** 25
OSR = 32
SILENCE = 0x99999999                                  # every word of a silent row from the zero state
EXPORTS = ["uc_mic_abi_version", "uc_mic_last_error", "uc_mic_quantise", "uc_mic_modulate_row", "uc_mic_create", "uc_mic_destroy",
           "uc_mic_modulate"]


class MicError(RuntimeError):
    pass


def _declare(L):
    L.uc_mic_quantise.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.POINTER(C.c_int32)]
    L.uc_mic_modulate_row.argtypes = [C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.uc_mic_create.argtypes = [C.c_int, C.c_float, C.POINTER(C.c_void_p)]
    L.uc_mic_modulate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]


_so = Binding("mic", MicError, _declare, env="UCHIRP_MIC_LIB")  # UCHIRP_MIC_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def quantise(x, scale=1.0):
    """uc_mic_quantise: float32 samples (times `scale`, to nearest even) or int32 DFSDM words (>> 8) -> int32 q,
    |q| <= 2^23 - 1, by the library (no GPU).  Any shape; other float types are rounded to float32 first."""
    a = np.asarray(x)
    a = np.ascontiguousarray(a, np.int32 if a.dtype == np.int32 else np.float32)
    q = np.zeros(a.shape, np.int32)
    if a.size:
        _check(lib().uc_mic_quantise(a.ctypes.data_as(C.c_void_p), DTYPE_I32 if a.dtype == np.int32 else DTYPE_F32, float(scale), a.size,
                                     q.ctypes.data_as(C.POINTER(C.c_int32))), "uc_mic_quantise")
    return q


def quantise_model(x, scale=1.0):
    """The quantiser of include/uchirp_mic.h restated in numpy."""
    a = np.asarray(x)
    if a.dtype == np.int32:
        return np.maximum(a >> 8, -Q_MAX).astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = a.astype(np.float32) * np.float32(scale)              # one float32 multiply
    v = np.where(np.isnan(v), np.float32(0.0), v)
    return np.rint(np.clip(v, -float(Q_MAX), float(Q_MAX))).astype(np.int32)


def _state_of(state, rows):
    if state is None:
        return np.zeros((rows, 4), np.int32)
    s = np.array(state, np.int32).reshape(-1, 4)
    if s.shape[0] != rows:
        raise ValueError("state must be [n_rows, 4]")
    return s


def modulate_row(q, state=None):
    """uc_mic_modulate_row: the definition in plain C for one row of quantised samples -> (words uint32 [n], state int32 [4]),
    by the library (no GPU)."""
    q = np.ascontiguousarray(q, np.int32).reshape(-1)
    st = np.ascontiguousarray(_state_of(state, 1)[0])
    w = np.zeros(q.size, np.uint32)
    if q.size:
        _check(lib().uc_mic_modulate_row(q.ctypes.data_as(C.POINTER(C.c_int32)), q.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                         w.ctypes.data_as(C.POINTER(C.c_uint32))), "uc_mic_modulate_row")
    return w, st


def model(q, state=None, track=None):
    """The definition of include/uchirp_mic.h in numpy int32 (every sum wraps), vectorised over rows: q int32 [n_rows, n]
    (1-d: one row) -> (words uint32 [n_rows, n], state int32 [n_rows, 4]).  `state`: the carried state, zeros if None.
    `track`: a dict that receives max |s1| and max |s2| per row as int64 arrays under "s1" and "s2"."""
    q = np.asarray(q)
    one = q.ndim == 1
    if q.ndim not in (1, 2) or q.dtype != np.int32:
        raise ValueError("q must be a 1-d or 2-d int32 array")
    q = np.atleast_2d(q)
    rows, n = q.shape
    st = _state_of(state, rows)
    prev, s1, s2 = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
    words = np.zeros((rows, n), np.uint32)
    plus, minus = np.int32(Y), np.int32(-Y)
    m1 = np.zeros(rows, np.int64)
    m2 = np.zeros(rows, np.int64)
    with np.errstate(over="ignore"):
        for j in range(n):
            qj = q[:, j]
            d = qj - prev
            base = prev + prev
            ramp = np.zeros(rows, np.int32)
            w = np.zeros(rows, np.uint32)
            for b in range(OSR):
                ramp = ramp + d                                   # d (b + 1)
                u = base + (ramp >> 4)
                up = s2 >= 0
                y = np.where(up, plus, minus)
                s1 = s1 + (u - y)
                s2 = s2 + (s1 - y)
                w |= up.astype(np.uint32) << np.uint32(b)
                if track is not None:
                    np.maximum(m1, np.abs(s1.astype(np.int64)), out=m1)
                    np.maximum(m2, np.abs(s2.astype(np.int64)), out=m2)
            words[:, j] = w
            prev = qj.copy()
    if track is not None:
        track["s1"], track["s2"] = m1, m2
    out = np.stack([prev, s1, s2, np.zeros(rows, np.int32)], axis=1).astype(np.int32)
    return (words[0], out[0]) if one else (words, out)


def sinc5_taps():
    """The 156 taps of the sinc^5 of 32 bits (their sum is 2^25), as uc_dfsdm_sinc5 applies them."""
    h = np.ones(1, np.int64)
    for _ in range(5):
        h = np.convolve(h, np.ones(OSR, np.int64))
    return h


def interpolated(q):
    """u of the definition from the zero state, in Python-sized integers (no wrap): int64 [n_rows, 32 n]."""
    q = np.atleast_2d(np.asarray(q)).astype(np.int64)
    prev = np.concatenate([np.zeros((q.shape[0], 1), np.int64), q[:, :-1]], axis=1)
    k = np.arange(1, OSR + 1, dtype=np.int64)
    u = 2 * prev[:, :, None] + (((q - prev)[:, :, None] * k) >> 4)
    return u.reshape(q.shape[0], -1)


def linear(q):
    """The linear path of the model from the zero state in float64: the same interpolation, one bit of delay, u / Y, the
    156-tap sinc^5 taken every 32 bits, then / 4: float64 [n_rows, n] in LSB of the 24-bit value, what
    uc_dfsdm_sinc5_streams gives (>> 8) of the model's words behind a silent history, without the quantisation error."""
    q = np.asarray(q)
    one = q.ndim == 1
    u = interpolated(q).astype(np.float64) / Y
    h = sinc5_taps().astype(np.float64)
    n = u.shape[1] // OSR
    out = np.zeros((u.shape[0], n))
    for r in range(u.shape[0]):
        delayed = np.concatenate([[0.0], u[r, :-1]])
        out[r] = np.convolve(delayed, h)[np.arange(n) * OSR + OSR - 1] / 4.0
    return out[0] if one else out


class Mic:
    """One uc_mic: the microphone model on one MI355X."""

    def __init__(self, scale=1.0, device=0):
        h = C.c_void_p()
        _check(lib().uc_mic_create(int(device), float(scale), C.byref(h)), "uc_mic_create")
        self._h = h
        self.device = int(device)
        self.scale = float(scale)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_mic_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_state(self, n_rows):
        """The state of n_rows microphones that start: zeros, int32 [n_rows, 4] on the object's device."""
        import torch
        return torch.zeros((int(n_rows), 4), dtype=torch.int32, device=torch.device("cuda", self.device))

    def modulate(self, rows, state=None, out=None, stream=None):
        """uc_mic_modulate: rows [n_rows, n] (a 2-d float32 / int32 device tensor with contiguous rows; int32 are DFSDM words)
        -> (words, state): the packed PDM words as an int32 tensor [n_rows, n] (the bit patterns of the uint32 words: the type
        the receivers' pdm=True path takes) and the carried state, int32 [n_rows, 4], updated in place (zeros if None: the
        microphones start).  `out`: a 2-d int32 device tensor with contiguous rows to write into.  Asynchronous on `stream` /
        torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        x = rows
        if (x.dim() != 2 or x.dtype not in (torch.float32, torch.int32) or x.device != dev or
                (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("rows must be a 2-d float32 / int32 tensor on %s with contiguous rows" % dev)
        nr, n = int(x.shape[0]), int(x.shape[1])
        if state is None:
            state = self.new_state(nr)
        elif state.dtype != torch.int32 or state.device != dev or tuple(state.shape) != (nr, 4) or not state.is_contiguous():
            raise ValueError("state must be a contiguous [%d, 4] int32 tensor on %s" % (nr, dev))
        if out is None:
            out = torch.empty((nr, n), dtype=torch.int32, device=dev)
        elif (out.dim() != 2 or out.dtype != torch.int32 or out.device != dev or tuple(out.shape) != (nr, n) or
              (n > 1 and out.stride(1) != 1) or (nr > 1 and out.stride(0) < n)):
            raise ValueError("out must be a [%d, %d] int32 tensor on %s with contiguous rows" % (nr, n, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_mic_modulate(self._h, C.c_void_p(x.data_ptr()), DTYPE_F32 if x.dtype == torch.float32 else DTYPE_I32, nr, n,
                                     int(x.stride(0)) if nr > 1 else n, C.c_void_p(state.data_ptr()), C.c_void_p(out.data_ptr()),
                                     int(out.stride(0)) if nr > 1 else n, C.c_void_p(stream) if stream else None), "uc_mic_modulate")
        return out, state
