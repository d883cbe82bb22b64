"""uchirp.link -- the link simulator: binding of libuchirp_link.so (include/uchirp_link.h) and its float64 model.

`Link.transmit` renders on the GPU, in one pass, what many microphones receive from as many independent transmissions
(own text, amplitude, fractional lead, clock offset in ppm and noise level each) into a device tensor that
`Engine.receive_many` / `LiveStreams.next` / `Engine.process` read in place.  There is no CPU path behind `Link`.

`model` is the same definition in numpy, in float64: `tx.render`'s law generalised by a clock offset and a
fractional lead, Philox4x32-10 and Box-Muller.  It is what the tests hold the kernel against, and what a user without
a GPU can call; it is slow (one stream at a time) and never used by `Link`.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import tx
from ._binding import Binding

ABI_VERSION = 2
DTYPE_I32, DTYPE_F32, DTYPE_I16 = 0, 1, 3
MAX_TEXT = 4096
MAX_FIRST_SAMPLE, MAX_SAMPLES = 1 << 52, 1 << 40
EXPORTS = ["uc_link_abi_version", "uc_link_last_error", "uc_link_default_config", "uc_link_create", "uc_link_destroy",
           "uc_link_transmit", "uc_link_noise_words", "uc_link_frame_origin"]


class LinkConfig(C.Structure):
    """struct uc_link_config (include/uchirp_link.h)."""
    _fields_ = [("fs_tx", C.c_double), ("t_symbol", C.c_double), ("f0", C.c_double), ("f1", C.c_double),
                ("n_preamble", C.c_uint32), ("n_guard", C.c_uint32)]


class LinkStream(C.Structure):
    """struct uc_link_stream (include/uchirp_link.h)."""
    _fields_ = [("lead_samples", C.c_double), ("amplitude", C.c_float), ("sigma", C.c_float), ("ppm", C.c_float),
                ("text_len", C.c_uint32)]


class LinkOrigin(C.Structure):
    """struct uc_link_origin (include/uchirp_link.h)."""
    _fields_ = [("origin", C.c_int64), ("t0", C.c_double), ("rate", C.c_double)]


STREAM_DTYPE = np.dtype([("lead_samples", "<f8"), ("amplitude", "<f4"), ("sigma", "<f4"), ("ppm", "<f4"), ("text_len", "<u4")])


class LinkError(RuntimeError):
    pass


def _declare(L):
    L.uc_link_default_config.argtypes = [C.POINTER(LinkConfig)]
    L.uc_link_create.argtypes = [C.c_int, C.POINTER(LinkConfig), C.POINTER(C.c_void_p)]
    L.uc_link_transmit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_double,
                                   C.c_uint64, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p]
    L.uc_link_noise_words.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p]
    L.uc_link_frame_origin.argtypes = [C.c_double, C.c_float, C.c_double, C.POINTER(LinkOrigin)]


_so = Binding("link", LinkError, _declare)
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def default_config(**over):
    cfg = LinkConfig()
    _check(lib().uc_link_default_config(C.byref(cfg)), "uc_link_default_config")
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def frame_origin(lead_samples, ppm=0.0, fs_out=78125.0):
    """uc_link_frame_origin: (origin, t0, rate) as the library derives them on the host; needs no GPU."""
    o = LinkOrigin()
    _check(lib().uc_link_frame_origin(float(lead_samples), float(ppm), float(fs_out), C.byref(o)), "uc_link_frame_origin")
    return int(o.origin), float(o.t0), float(o.rate)


def _as_bytes(t):
    return t.encode("latin-1") if isinstance(t, str) else bytes(t)


def pack(texts, lead_samples, amplitude, sigma, ppm=0.0):
    """The host arrays of uc_link_transmit: (text uint8 [n_streams, text_stride], params STREAM_DTYPE [n_streams]).
    Scalars are broadcast over the streams."""
    raw = [_as_bytes(t) for t in texts]
    ns = len(raw)
    stride = max(1, max((len(r) for r in raw), default=1))
    text = np.zeros((ns, stride), np.uint8)
    for i, r in enumerate(raw):
        text[i, :len(r)] = np.frombuffer(r, np.uint8)
    p = np.zeros(ns, STREAM_DTYPE)
    p["lead_samples"] = np.broadcast_to(np.asarray(lead_samples, np.float64), (ns,))
    p["amplitude"] = np.broadcast_to(np.asarray(amplitude, np.float32), (ns,))
    p["sigma"] = np.broadcast_to(np.asarray(sigma, np.float32), (ns,))
    p["ppm"] = np.broadcast_to(np.asarray(ppm, np.float32), (ns,))
    p["text_len"] = [len(r) for r in raw]
    return text, p


class Link:
    """One uc_link: the transmitter + channel of one frame format on one MI355X."""

    def __init__(self, device=0, **over):
        self.cfg = default_config(**over)
        h = C.c_void_p()
        _check(lib().uc_link_create(int(device), C.byref(self.cfg), C.byref(h)), "uc_link_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_link_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _dtype(dtype):
        import torch
        table = {DTYPE_F32: torch.float32, DTYPE_I32: torch.int32, DTYPE_I16: torch.int16}
        if dtype in table:
            return dtype, table[dtype]
        for code, t in table.items():
            if dtype is t or dtype == t:
                return code, t
        raise TypeError("dtype must be float32, int32 (DFSDM words) or int16")

    def transmit(self, texts, lead_samples, amplitude, sigma, ppm=0.0, n_samples=None, fs_out=78125.0, dtype=DTYPE_F32,
                 first_sample=0, seed=0, out=None, stream=None):
        """uc_link_transmit: samples [first_sample, first_sample + n_samples) of len(texts) streams -> a torch tensor
        [n_streams, n_samples] on the link's device (or into `out`: a 2-d device tensor with contiguous rows, e.g. a
        column slice of a ring buffer).  Asynchronous on `stream` / torch's current stream."""
        import torch
        text, p = pack(texts, lead_samples, amplitude, sigma, ppm)
        ns = len(p)
        code, tdt = self._dtype(dtype)
        dev = torch.device("cuda", self.device)
        if out is None:
            if n_samples is None:
                raise ValueError("n_samples or out must be given")
            out = torch.empty((ns, int(n_samples)), dtype=tdt, device=dev)
        else:
            if (out.dim() != 2 or out.dtype != tdt or out.device != dev or out.shape[0] != ns or
                    (out.shape[1] > 1 and out.stride(1) != 1) or (ns > 1 and out.stride(0) < out.shape[1])):
                raise ValueError("out must be a [%d, n_samples] %s tensor on %s with contiguous rows" % (ns, tdt, dev))
            if n_samples is not None and int(n_samples) != out.shape[1]:
                raise ValueError("n_samples does not match out")
        nsmp = int(out.shape[1])
        stride = int(out.stride(0)) if ns > 1 else nsmp
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_link_transmit(self._h, text.ctypes.data_as(C.c_void_p), text.shape[1], p.ctypes.data_as(C.c_void_p), ns,
                                      C.c_void_p(out.data_ptr()), code, float(fs_out), int(first_sample), nsmp, stride,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(stream) if stream else None),
               "uc_link_transmit")
        return out

    def noise_words(self, seed, stream_index, first_counter, n_counters, stream=None):
        """uc_link_noise_words -> int32 device tensor [n_counters, 4] (the bit patterns of the uint32 words)."""
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty((int(n_counters), 4), dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_link_noise_words(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_index), int(first_counter),
                                         int(n_counters), C.c_void_p(out.data_ptr()), C.c_void_p(stream) if stream else None),
               "uc_link_noise_words")
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the model: the same definition in numpy / float64

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11).  counter: uint32 [..., 4], key: two 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter).astype(np.uint64)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def noise_words(seed, stream_index, first_counter, n_counters):
    """The words uc_link_noise_words writes: uint32 [n_counters, 4]."""
    seed, s = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_index) & 0xFFFFFFFFFFFFFFFF
    c = (np.arange(int(n_counters), dtype=np.uint64) + np.uint64(int(first_counter) & 0xFFFFFFFFFFFFFFFF))
    ctr = np.empty((c.size, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = c & _MASK, c >> _S32, s & 0xFFFFFFFF, s >> 32
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(words):
    """u = ((w >> 8) + 1/2) 2^-24 in float64 (exact; never 0 or 1)."""
    return ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed, stream_index, first_sample, n_samples):
    """Standard normals of samples [first_sample, first_sample + n_samples) of one stream (float64), and the uniform under
    each sample's radius (the tests' tail criterion)."""
    first_sample, n_samples = int(first_sample), int(n_samples)
    c0, c1 = first_sample // 4, (first_sample + n_samples + 3) // 4
    u = uniforms(noise_words(seed, stream_index, c0, c1 - c0))
    z = np.empty_like(u)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        z[:, a], z[:, a + 1] = r * np.cos(2.0 * np.pi * u[:, a + 1]), r * np.sin(2.0 * np.pi * u[:, a + 1])
    ur = u[:, [0, 0, 2, 2]]
    lo = first_sample - 4 * c0
    return z.reshape(-1)[lo:lo + n_samples], ur.reshape(-1)[lo:lo + n_samples]


def origin_model(lead_samples, ppm=0.0, fs_out=78125.0):
    """What uc_link_frame_origin states, from fractions: (origin, t0, rate).  origin is the library's own choice (the double
    quotient lead / (1 + ppm / 1e6) to the nearest integer, ties to even, held to +-2^53); t0 is the rational
    (origin (1 + ppm 10^-6) - lead) / fs_out rounded once; rate is the library's double expression."""
    lead, ppm, fs_out = float(lead_samples), float(np.float32(ppm)), float(fs_out)
    den = 1.0 + ppm / 1e6
    q = lead / den if den != 0.0 else (0.0 if lead == 0.0 else float(np.copysign(np.inf, lead)))   # (Python raises where C gives inf)
    origin = int(round(min(max(q, -2.0 ** 53), 2.0 ** 53)))
    t0 = float((origin * (1 + Fraction(ppm) / 10 ** 6) - Fraction(lead)) / Fraction(fs_out))
    return origin, t0, (1.0 / fs_out) * (1.0 + ppm * 1e-6)


def signal(text, lead_samples=0.0, amplitude=tx.AMPLITUDE, ppm=0.0, n_samples=None, fs_out=78125.0, first_sample=0,
           fs_tx=tx.FS_TX, t_symbol=tx.T_SYMBOL, f0=tx.F0, f1=tx.F1, n_preamble=tx.N_PREAMBLE, n_guard=tx.N_GUARD):
    """tx.render's law, operation for operation, with a clock offset and a fractional lead (float64 [n_samples]).  The
    seconds since the frame began come from the integer distance of the sample to the frame's origin (origin_model), as
    in the library, so their error is that of a time inside the frame wherever in a recording the frame lies."""
    if n_samples is None:
        n_seq = 2 + n_preamble + 8 * len(_as_bytes(text)) + n_guard
        lead_s = float(lead_samples) / float(fs_out)
        n_samples = int(np.floor((lead_s + n_seq * (int(t_symbol * fs_tx) / float(fs_tx))) * fs_out)) - int(first_sample)
    origin, t0, rate = origin_model(lead_samples, ppm, fs_out)
    d = np.arange(int(first_sample) - origin, int(first_sample) - origin + int(n_samples), dtype=np.int64)
    tt = d.astype(np.float64) * rate + t0
    return law(text, tt, amplitude, fs_tx, t_symbol, f0, f1, n_preamble, n_guard)


def law(text, tt, amplitude=tx.AMPLITUDE, fs_tx=tx.FS_TX, t_symbol=tx.T_SYMBOL, f0=tx.F0, f1=tx.F1, n_preamble=tx.N_PREAMBLE,
        n_guard=tx.N_GUARD):
    """The frame at the times tt (float64 seconds since it began): what `signal` does with its times."""
    raw = _as_bytes(text)
    bits = np.unpackbits(np.frombuffer(raw, np.uint8)).astype(int) if raw else np.zeros(0, int)
    seq = np.concatenate([[-1], np.ones(n_preamble, int), [0], bits, -np.ones(n_guard, int)]).astype(int)
    n_sym = int(t_symbol * fs_tx)
    sym_dur = n_sym / float(fs_tx)
    tt = np.asarray(tt, np.float64)
    idx = np.floor((tt + 1e-10) / sym_dur).astype(np.int64)
    valid = (idx >= 0) & (idx < len(seq))
    tau = np.maximum(tt - idx * sym_dur, 0.0)
    t = tau * fs_tx * t_symbol / (n_sym - 1)
    k = float(f1 - f0) / t_symbol
    kind = np.where(valid, seq[np.clip(idx, 0, len(seq) - 1)], -1)
    f = np.where(kind == 1, f0 + k * t / 2.0, f1 - k * t / 2.0)
    arg = 2.0 * np.pi * f * t - np.pi / 2.0
    out = (np.cos(arg) + np.sin(arg)) * float(amplitude)
    return np.where(kind >= 0, out, 0.0)


def model(texts, lead_samples, amplitude, sigma, ppm=0.0, n_samples=None, fs_out=78125.0, first_sample=0, seed=0, **fmt):
    """What Link.transmit renders, in float64 before the output conversion: [n_streams, n_samples].  The parameters are
    rounded to the types of struct uc_link_stream first (float amplitude / sigma / ppm), as the library sees them."""
    if n_samples is None:
        raise ValueError("n_samples must be given")
    _, p = pack(texts, lead_samples, amplitude, sigma, ppm)
    out = np.empty((len(p), int(n_samples)), np.float64)
    for s, t in enumerate(texts):
        x = signal(t, float(p["lead_samples"][s]), float(p["amplitude"][s]), float(p["ppm"][s]), n_samples, fs_out, first_sample,
                   **fmt)
        sg = float(p["sigma"][s])
        if sg != 0.0:
            x = x + sg * normals(seed, s, first_sample, n_samples)[0]
        out[s] = x
    return out


def convert(x, dtype):
    """The output conversions of uc_link_transmit applied to model values."""
    x = np.asarray(x)
    if dtype == DTYPE_F32:
        return x.astype(np.float32)
    if dtype == DTYPE_I32:
        return (np.clip(np.round(x), -8388608, 8388607).astype(np.int64) * 256).astype(np.int32)
    if dtype == DTYPE_I16:
        return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16)
    raise TypeError("unknown dtype")
