"""uchirp.dfsdm -- the DFSDM filter in every configuration of the peripheral: binding of libuchirp_dfsdm.so
(include/uchirp_dfsdm.h) and its definition in numpy.

`uchirp.Engine.dfsdm` / `dfsdm_streams` (uc_dfsdm_sinc5*) are the peripheral in the receiver's one configuration and stay the
fast path for it.  `Dfsdm(cfg).run` turns many rows of packed PDM words into the filter's 24-bit words (in bits 31:8) on the
GPU for any order (FastSinc, Sinc1..5), ratio, integrator, right shift and offset, the state of every row carried in a device
tensor.  The arithmetic is exact: `model` is the definition in numpy (from a zero state the direct FIR in int64), and the
GPU's words equal it bit for bit.  There is no CPU path behind `Dfsdm`; `check`, `gain`, `plan`, `filter_row` (the library's
host functions), `taps`, `model` and `word_rate` need no GPU.
"""
import collections
import ctypes as C

import numpy as np

from ._binding import Binding

ABI_VERSION = 1
FASTSINC = 0
STATE_WORDS = 16
GAIN_MAX = 2 ** 31 - 1
EXPORTS = ["uc_dfsdm_abi_version", "uc_dfsdm_last_error", "uc_dfsdm_check", "uc_dfsdm_gain", "uc_dfsdm_plan", "uc_dfsdm_filter_row",
           "uc_dfsdm_create", "uc_dfsdm_destroy", "uc_dfsdm_run"]

Config = collections.namedtuple("Config", "order ratio integrator shift offset", defaults=(1, 0, 0))
Config.__doc__ = "order 0 (FastSinc) .. 5, ratio R 1 .. 1024, integrator I 1 .. 256, right shift 0 .. 31, offset -2^23 .. 2^23 - 1"

# What the reference's firmware projects write into the peripheral (*/Src/dfsdm.c): name -> (Config, clock divider of the
# 80 MHz system clock).  word_rate(divider, cfg) is the rate of the words each of them saw.
REFERENCE_CONFIGS = {
    "receiver": (Config(5, 32, 1, 2, 0), 32),                                   # receiver/Src/dfsdm.c:59-61, 69, 77-78
    "experiments/synchronization": (Config(5, 32, 1, 2, 0), 32),                # .../Src/dfsdm.c:62-64, 73, 81-82
    "experiments/iq_modulation": (Config(5, 32, 1, 2, 0), 25),                  # .../Src/dfsdm.c:62-64, 73, 81-82
    "experiments/basic": (Config(3, 32, 1, 2, 0), 52),                          # .../Src/dfsdm.c:68-70, 103, 111-112 (the 48.1 kHz captures)
    "experiments/basic _100kHz": (Config(3, 32, 1, 2, 0), 25),                  # .../Src/dfsdm.c:68-70, 103, 111-112
    "experiments/chirp": (Config(3, 32, 1, 2, 0), 25),                          # .../Src/dfsdm.c:68-70, 103, 111-112
    "experiments/ultracom": (Config(3, 32, 1, 2, 0), 25),                       # .../Src/dfsdm.c:65-67, 88, 96-97
    "experiments/chirp_compression_time_domain": (Config(3, 32, 1, 2, 0), 25),  # .../Src/dfsdm.c:62-64, 73, 81-82
    "experiments/chirp_compression_freq_domain": (Config(3, 32, 1, 2, 0), 25),  # .../Src/dfsdm.c:62-64, 73, 81-82
}
SYSTEM_CLOCK_HZ = 80e6


class DfsdmError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("order", C.c_int32), ("ratio", C.c_uint32), ("integrator", C.c_uint32), ("shift", C.c_int32), ("offset", C.c_int32)]


def _declare(L):
    cfg = C.POINTER(_Config)
    L.uc_dfsdm_check.argtypes = [cfg]
    L.uc_dfsdm_gain.argtypes, L.uc_dfsdm_gain.restype = [cfg], C.c_uint64
    L.uc_dfsdm_plan.argtypes = [cfg, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.uc_dfsdm_filter_row.argtypes = [cfg, C.POINTER(C.c_uint32), C.c_size_t, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.c_size_t, C.POINTER(C.c_size_t)]
    L.uc_dfsdm_create.argtypes = [C.c_int, cfg, C.POINTER(C.c_void_p)]
    L.uc_dfsdm_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p]


_so = Binding("dfsdm", DfsdmError, _declare, env="UCHIRP_DFSDM_LIB")  # UCHIRP_DFSDM_LIB: diagnostic builds
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def _c(cfg):
    """The C structure of a configuration; values outside the fields' C types (the library refuses what is left) raise
    DfsdmError here."""
    cfg = Config(*cfg)
    try:
        vals = [int(v) for v in cfg]
        if not (-2 ** 31 <= vals[0] < 2 ** 31 and 0 <= vals[1] < 2 ** 32 and 0 <= vals[2] < 2 ** 32 and -2 ** 31 <= vals[3] < 2 ** 31 and
                -2 ** 31 <= vals[4] < 2 ** 31):
            raise ValueError
    except (TypeError, ValueError):
        raise DfsdmError("configuration %r does not fit the fields of uc_dfsdm_config" % (cfg,))
    return _Config(*vals)


def check(cfg):
    """uc_dfsdm_check: raises DfsdmError with the library's reason unless the configuration is one of the definition's."""
    _check(lib().uc_dfsdm_check(C.byref(_c(cfg))), "uc_dfsdm_check")
    return Config(*cfg)


def stages(cfg):
    """N of the definition: the order, 2 for FastSinc."""
    return 2 if Config(*cfg).order == FASTSINC else int(Config(*cfg).order)


def gain(cfg):
    """uc_dfsdm_gain: G = R^N I, for FastSinc 2 R^2 I (no check of the limit 2^31 - 1)."""
    return int(lib().uc_dfsdm_gain(C.byref(_c(cfg))))


def plan(cfg, words_before, n_words):
    """uc_dfsdm_plan: the outputs of a call of n_words words behind words_before."""
    n = C.c_uint64()
    _check(lib().uc_dfsdm_plan(C.byref(_c(cfg)), int(words_before), int(n_words), C.byref(n)), "uc_dfsdm_plan")
    return int(n.value)


def taps(cfg):
    """The FIR that the configuration is from a zero state, before the integrator: int64, the N-fold convolution of R ones,
    for FastSinc two such boxcars and {1, 0 .. 0, 1} of length 2 R + 1.  Their sum is G / I."""
    cfg = Config(*cfg)
    box = np.ones(cfg.ratio, np.int64)
    h = np.ones(1, np.int64)
    for _ in range(stages(cfg)):
        h = np.convolve(h, box)
    if cfg.order == FASTSINC:
        two = np.zeros(2 * cfg.ratio + 1, np.int64)
        two[0] = two[-1] = 1
        h = np.convolve(h, two)
    return h


def word_rate(divider, cfg, clock_hz=SYSTEM_CLOCK_HZ):
    """Words per second of a configuration behind a bit clock of clock_hz / divider."""
    cfg = Config(*cfg)
    return clock_hz / divider / (cfg.ratio * cfg.integrator)


def bits_of(words):
    """The +-1 of packed words [..., n] -> int64 [..., 32 n]: bit t is bit t & 31 of word t >> 5."""
    w = np.asarray(words).view(np.uint32) if np.asarray(words).dtype == np.int32 else np.asarray(words, np.uint32)
    b = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(w.shape[:-1] + (-1,)).astype(np.int64) * 2 - 1


def _finish(y, cfg):
    return (np.clip((y >> cfg.shift) - cfg.offset, -2 ** 23, 2 ** 23 - 1) * 256).astype(np.int32)


def _wrap(v):
    """int64 values reduced to int32 in two's complement, still int64"""
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def zero_state(n_rows=None):
    return np.zeros(STATE_WORDS if n_rows is None else (int(n_rows), STATE_WORDS), np.int32)


def model(words, cfg, state=None, words_before=0):
    """The definition of include/uchirp_dfsdm.h in numpy int64: words uint32 [n_rows, n] (1-d: one row) -> (out int32
    [n_rows, n_out], state int32 [n_rows, 16]).  With state None and words_before 0 (the peripheral just enabled) the outputs
    are the DIRECT convolution of the bits with `taps`, summed over I values, with no recursion anywhere, and the state
    behind it comes from the recursion; with a state, the recursion of the header reduced to int32 after every sum."""
    cfg = check(cfg)
    w = np.asarray(words)
    one = w.ndim == 1
    w = np.atleast_2d(w)
    w = w.view(np.uint32) if w.dtype == np.int32 else w.astype(np.uint32)
    rows, n = w.shape
    N, R, I = stages(cfg), cfg.ratio, cfg.integrator
    fresh = state is None and words_before == 0
    st = zero_state(rows) if state is None else np.array(state, np.int32).reshape(-1, STATE_WORDS).copy()
    if st.shape[0] != rows:
        raise ValueError("state must be [n_rows, 16]")
    bits = bits_of(w)
    n_out = plan(cfg, words_before, n)
    out = np.zeros((rows, n_out), np.int32)
    # the recursion (always: it gives the state; from a fresh start the outputs come from the FIR below)
    integ = [st[:, k].astype(np.int64) for k in range(N)]
    comb = [st[:, 5 + k].astype(np.int64) for k in range(N)]
    fast = [st[:, 10].astype(np.int64), st[:, 11].astype(np.int64)]
    acc = st[:, 12].astype(np.int64)
    pr = (32 * words_before) % R
    pi = ((32 * words_before) // R) % I
    k_out = 0
    t = 0
    total = bits.shape[1]
    while t < total:
        # the integrators up to the next R-th bit: N running sums over the span, reduced to int32
        span = min(R - pr, total - t)
        s = bits[:, t:t + span]
        for k in range(N):
            c = np.cumsum(s, axis=1) + integ[k][:, None]
            integ[k] = _wrap(c[:, -1])
            s = _wrap(c)
        t += span
        pr += span
        if pr < R:
            break
        pr = 0
        v = integ[N - 1]
        for k in range(N):
            d = _wrap(v - comb[k])
            comb[k] = v
            v = d
        if cfg.order == FASTSINC:
            wsum = _wrap(v + fast[1])
            fast = [v, fast[0]]
            v = wsum
        acc = _wrap(acc + v)
        pi += 1
        if pi == I:
            pi = 0
            out[:, k_out] = _finish(acc, cfg)
            acc = np.zeros(rows, np.int64)
            k_out += 1
    assert k_out == n_out
    if fresh and n_out:
        h = taps(cfg)
        idx = (np.arange(n_out * I, dtype=np.int64) + 1) * R - 1          # the bits at which a value falls
        for r in range(rows):
            y = np.convolve(bits[r], h)[idx].reshape(n_out, I).sum(axis=1)    # exact in int64: |y| <= G
            out[r] = _finish(y, cfg)
    for k in range(N):
        st[:, k] = integ[k]
        st[:, 5 + k] = comb[k]
    if cfg.order == FASTSINC:
        st[:, 10], st[:, 11] = fast[0], fast[1]
    st[:, 12] = acc
    st[:, 13:] = 0
    return (out[0], st[0]) if one else (out, st)


def filter_row(words, cfg, state=None, words_before=0):
    """uc_dfsdm_filter_row: the definition in plain C for one row of words -> (out int32 [n_out], state int32 [16]), by the
    library (no GPU)."""
    w = np.asarray(words)
    w = np.ascontiguousarray(w.view(np.uint32) if w.dtype == np.int32 else w.astype(np.uint32)).reshape(-1)
    st = zero_state() if state is None else np.ascontiguousarray(np.array(state, np.int32).reshape(STATE_WORDS))
    c = _c(cfg)
    cap = 32 * w.size
    out = np.zeros(max(cap, 1), np.int32)
    n = C.c_size_t()
    _check(lib().uc_dfsdm_filter_row(C.byref(c), w.ctypes.data_as(C.POINTER(C.c_uint32)), w.size, int(words_before),
                                     st.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n)),
           "uc_dfsdm_filter_row")
    return out[:n.value].copy(), st


class Dfsdm:
    """One uc_dfsdm: the DFSDM filter in one configuration on one MI355X."""

    def __init__(self, cfg, device=0):
        self.cfg = Config(*cfg)
        h = C.c_void_p()
        _check(lib().uc_dfsdm_create(int(device), C.byref(_c(self.cfg)), C.byref(h)), "uc_dfsdm_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_dfsdm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_state(self, n_rows):
        """The state of n_rows filters just enabled: zeros, int32 [n_rows, 16] on the object's device."""
        import torch
        return torch.zeros((int(n_rows), STATE_WORDS), dtype=torch.int32, device=torch.device("cuda", self.device))

    def run(self, words, state=None, words_before=0, out=None, stream=None):
        """uc_dfsdm_run: words [n_rows, n] (a 2-d int32 device tensor with contiguous rows: the bit patterns of the packed PDM
        words, what Mic.modulate gives) -> (out, state): the filter's words as an int32 tensor [n_rows, n_out] (n_out =
        plan(cfg, words_before, n)) and the carried state, int32 [n_rows, 16], updated in place (zeros if None: the filters
        start, and then words_before must be what they have consumed: 0).  `out`: a 2-d int32 device tensor with contiguous
        rows to write into.  Asynchronous on `stream` / torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        x = words
        if (x.dim() != 2 or x.dtype != torch.int32 or x.device != dev or (x.shape[1] > 1 and x.stride(1) != 1) or
                (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError("words must be a 2-d int32 tensor on %s with contiguous rows" % dev)
        nr, n = int(x.shape[0]), int(x.shape[1])
        n_out = plan(self.cfg, words_before, n)
        if state is None:
            state = self.new_state(nr)
        elif state.dtype != torch.int32 or state.device != dev or tuple(state.shape) != (nr, STATE_WORDS) or not state.is_contiguous():
            raise ValueError("state must be a contiguous [%d, %d] int32 tensor on %s" % (nr, STATE_WORDS, dev))
        if out is None:
            out = torch.empty((nr, n_out), dtype=torch.int32, device=dev)
        elif (out.dim() != 2 or out.dtype != torch.int32 or out.device != dev or tuple(out.shape) != (nr, n_out) or
              (n_out > 1 and out.stride(1) != 1) or (nr > 1 and out.stride(0) < n_out)):
            raise ValueError("out must be a [%d, %d] int32 tensor on %s with contiguous rows" % (nr, n_out, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        # (a call without outputs still needs an address that is device memory: the state's own would overlap, so one word)
        target = out if n_out else torch.empty((nr, 1), dtype=torch.int32, device=dev)
        _check(lib().uc_dfsdm_run(self._h, C.c_void_p(x.data_ptr()), nr, n, int(x.stride(0)) if nr > 1 else n, int(words_before),
                                  C.c_void_p(state.data_ptr()), C.c_void_p(target.data_ptr()),
                                  int(target.stride(0)) if nr > 1 else max(n_out, 1), C.c_void_p(stream) if stream else None), "uc_dfsdm_run")
        return out, state
