"""uchirp.scene -- the acoustic scene renderer: binding of libuchirp_scene.so (include/uchirp_scene.h) and its float64 model.

`Link.transmit` (uchirp.link) gives every microphone one arrival of one transmission.  `Scene.render` gives every
microphone a list of paths -- arrivals of any of the scene's transmissions, each with its own gain (negative: inverted),
fractional lead and clock offset -- sums them in one pass on the GPU and adds noise once per microphone, into a device
tensor that `Engine.receive_many` / `LiveStreams.next` / `Engine.process` read in place.  There is no CPU path behind
`Scene`.

A scene is written as
    texts = ["Hello World!", "other"]                       the transmissions
    mics  = [(sigma, [(tx, gain, lead_samples, ppm), ...]), ...]   one entry per microphone, its paths in order
`model` is the same definition in numpy / float64, built from `link.signal` and `link.normals`.
"""
import ctypes as C

import numpy as np

from . import link
from .link import DTYPE_F32, DTYPE_I16, DTYPE_I32, MAX_TEXT, LinkConfig, convert  # noqa: F401  (one set of formats)
from ._binding import Binding

ABI_VERSION = 1
MAX_PATHS = 16
EXPORTS = ["uc_scene_abi_version", "uc_scene_last_error", "uc_scene_default_config", "uc_scene_create", "uc_scene_destroy",
           "uc_scene_render"]


class ScenePath(C.Structure):
    """struct uc_scene_path (include/uchirp_scene.h)."""
    _fields_ = [("lead_samples", C.c_double), ("gain", C.c_float), ("ppm", C.c_float), ("tx", C.c_uint32), ("reserved", C.c_uint32)]


class SceneMic(C.Structure):
    """struct uc_scene_mic (include/uchirp_scene.h)."""
    _fields_ = [("first_path", C.c_uint32), ("n_paths", C.c_uint32), ("sigma", C.c_float), ("reserved", C.c_uint32)]


PATH_DTYPE = np.dtype([("lead_samples", "<f8"), ("gain", "<f4"), ("ppm", "<f4"), ("tx", "<u4"), ("reserved", "<u4")])
MIC_DTYPE = np.dtype([("first_path", "<u4"), ("n_paths", "<u4"), ("sigma", "<f4"), ("reserved", "<u4")])


class SceneError(RuntimeError):
    pass


def _declare(L):
    L.uc_scene_default_config.argtypes = [C.POINTER(LinkConfig)]
    L.uc_scene_create.argtypes = [C.c_int, C.POINTER(LinkConfig), C.POINTER(C.c_void_p)]
    L.uc_scene_render.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_size_t, C.c_void_p, C.c_int, C.c_double, C.c_uint64, C.c_size_t, C.c_size_t, C.c_uint64,
                                  C.c_void_p]


_so = Binding("scene", SceneError, _declare)
LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check


def default_config(**over):
    cfg = LinkConfig()
    _check(lib().uc_scene_default_config(C.byref(cfg)), "uc_scene_default_config")
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def pack(texts, mics):
    """The host arrays of uc_scene_render: (text uint8 [n_tx, text_stride], text_len uint32 [n_tx], paths PATH_DTYPE
    [n_paths], mics MIC_DTYPE [n_mics]).  `mics`: a list of (sigma, [(tx, gain, lead_samples, ppm), ...]); every
    microphone's paths are laid out one after the other in the order given.  ValueError for a tx that names no text and
    for more than MAX_PATHS paths of one microphone."""
    raw = [link._as_bytes(t) for t in texts]
    stride = max(1, max((len(r) for r in raw), default=1))
    text = np.zeros((len(raw), stride), np.uint8)
    for i, r in enumerate(raw):
        text[i, :len(r)] = np.frombuffer(r, np.uint8)
    text_len = np.array([len(r) for r in raw], np.uint32)
    m = np.zeros(len(mics), MIC_DTYPE)
    rows = []
    for i, (sigma, plist) in enumerate(mics):
        plist = list(plist)
        if len(plist) > MAX_PATHS:
            raise ValueError("microphone %d has %d paths (at most %d)" % (i, len(plist), MAX_PATHS))
        m[i] = (len(rows), len(plist), sigma, 0)
        for (tx_i, gain, lead, ppm) in plist:
            if not 0 <= int(tx_i) < len(raw):
                raise ValueError("microphone %d: tx %d names none of the %d transmissions" % (i, int(tx_i), len(raw)))
            rows.append((lead, gain, ppm, int(tx_i), 0))
    p = np.array(rows, PATH_DTYPE) if rows else np.zeros(0, PATH_DTYPE)
    return text, text_len, p, m


class Scene:
    """One uc_scene: the renderer of one frame format on one MI355X."""

    def __init__(self, device=0, **over):
        self.cfg = default_config(**over)
        h = C.c_void_p()
        _check(lib().uc_scene_create(int(device), C.byref(self.cfg), C.byref(h)), "uc_scene_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().uc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_packed(self, text, text_len, paths, mics, n_samples=None, fs_out=78125.0, dtype=DTYPE_F32, first_sample=0, seed=0,
                      out=None, stream=None):
        """uc_scene_render on arrays as `pack` makes them (a loop of calls packs once)."""
        import torch
        nm = len(mics)
        code, tdt = link.Link._dtype(dtype)
        dev = torch.device("cuda", self.device)
        if out is None:
            if n_samples is None:
                raise ValueError("n_samples or out must be given")
            out = torch.empty((nm, int(n_samples)), dtype=tdt, device=dev)
        else:
            if (out.dim() != 2 or out.dtype != tdt or out.device != dev or out.shape[0] != nm or
                    (out.shape[1] > 1 and out.stride(1) != 1) or (nm > 1 and out.stride(0) < out.shape[1])):
                raise ValueError("out must be a [%d, n_samples] %s tensor on %s with contiguous rows" % (nm, tdt, dev))
            if n_samples is not None and int(n_samples) != out.shape[1]:
                raise ValueError("n_samples does not match out")
        nsmp = int(out.shape[1])
        stride = int(out.stride(0)) if nm > 1 else nsmp
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().uc_scene_render(self._h, text.ctypes.data_as(C.c_void_p), text.shape[1], text_len.ctypes.data_as(C.c_void_p),
                                     len(text_len), paths.ctypes.data_as(C.c_void_p) if len(paths) else None, len(paths),
                                     mics.ctypes.data_as(C.c_void_p), nm, C.c_void_p(out.data_ptr()), code, float(fs_out),
                                     int(first_sample), nsmp, stride, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     C.c_void_p(stream) if stream else None), "uc_scene_render")
        return out

    def render(self, texts, mics, n_samples=None, fs_out=78125.0, dtype=DTYPE_F32, first_sample=0, seed=0, out=None, stream=None):
        """uc_scene_render: samples [first_sample, first_sample + n_samples) of len(mics) microphones -> a torch tensor
        [n_mics, n_samples] on the scene's device (or into `out`: a 2-d device tensor with contiguous rows, e.g. a column
        slice of a ring buffer).  Asynchronous on `stream` / torch's current stream."""
        return self.render_packed(*pack(texts, mics), n_samples=n_samples, fs_out=fs_out, dtype=dtype, first_sample=first_sample,
                                  seed=seed, out=out, stream=stream)


def model(texts, mics, n_samples=None, fs_out=78125.0, first_sample=0, seed=0, **fmt):
    """What Scene.render renders, in float64 before the output conversion: [n_mics, n_samples].  The paths are summed in
    float64 and the noise is added once, keyed by the microphone's index.  The parameters are rounded to the types of
    struct uc_scene_path / uc_scene_mic first (float gain / ppm / sigma), as the library sees them."""
    if n_samples is None:
        raise ValueError("n_samples must be given")
    _, _, p, m = pack(texts, mics)
    out = np.empty((len(m), int(n_samples)), np.float64)
    for i in range(len(m)):
        x = None
        for q in p[int(m["first_path"][i]):int(m["first_path"][i]) + int(m["n_paths"][i])]:
            s = link.signal(texts[int(q["tx"])], float(q["lead_samples"]), float(q["gain"]), float(q["ppm"]), n_samples, fs_out,
                            first_sample, **fmt)
            x = s if x is None else x + s
        if x is None:
            x = np.zeros(int(n_samples), np.float64)
        sg = float(m["sigma"][i])
        if sg != 0.0:
            x = x + sg * link.normals(seed, i, first_sample, n_samples)[0]
        out[i] = x
    return out
