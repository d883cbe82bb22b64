"""What the CPU and the GPU tests of the pulse compressor share (uchirp/mf.py, include/uchirp_mf.h): the rows, templates, jobs
and call ranges of the GPU comparison -- so that the CPU suite fixes the error constant on exactly those inputs --, the
notebook's chirp case, and the chain scene -> down-converter -> compressor -> arrivals in float64."""
import functools

import numpy as np

NS = 3 * 2048 + 37                                     # samples of a row
TAPS = (1, 2, 255, 256, 1023, 1024, 1664)
DTYPES = ("f32", "i32", "c32")
JOBS = [(0, 0), (1, 1), (2, 0), (0, 1)]                # three rows, two templates; row 0 through both
P = 2048
FS = 78125.0


@functools.lru_cache(maxsize=None)
def rows(kind):
    """three rows of NS samples: floats, DFSDM words that are mostly no floats, complex pairs"""
    rng = np.random.default_rng({"f32": 31, "i32": 32, "c32": 33}[kind])
    if kind == "f32":
        x = (rng.standard_normal((3, NS)) * 1000.0).astype(np.float32)
    elif kind == "i32":
        x = rng.integers(-2 ** 27, 2 ** 27, size=(3, NS)).astype(np.int32)
    else:
        x = ((rng.standard_normal((3, NS)) + 1j * rng.standard_normal((3, NS))) * 700.0).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def templates(n_taps):
    """two sets of random complex taps"""
    rng = np.random.default_rng(1000 + n_taps)
    h = ((rng.standard_normal((2, n_taps)) + 1j * rng.standard_normal((2, n_taps))) / np.sqrt(2.0 * n_taps)).astype(np.complex64)
    h.setflags(write=False)
    return h


def positions(n_taps):
    """pos0 of the GPU comparison: 0, S - 1 (element 0 is a segment's last output), far out"""
    return (0, P - n_taps - 2, 2 ** 40 + 5)


def ranges(n_taps, pos0):
    """(first, n) of the GPU comparison: first 0 and an odd one; n = 1, up to the end of first's segment, one more, the
    rest of the row"""
    hop = P - n_taps - 1
    out = []
    for first in (0, 37):
        to_end = hop - (pos0 + first) % hop
        for n in (1, to_end, to_end + 1, NS - first):
            out.append((first, n))
    return out


@functools.lru_cache(maxsize=None)
def _model_full(kind, n_taps):
    from uchirp import mf
    x = mf.samples(rows(kind)).astype(np.complex128)
    h = np.asarray(templates(n_taps)).astype(np.complex128)
    y = np.stack([np.convolve(x[r], h[s]) for r, s in JOBS])                # NS + n_taps - 1 outputs: the row's and the tail
    y = np.concatenate([y, np.zeros((len(JOBS), 1))], axis=1)               # (one tap: no tail)
    y.setflags(write=False)
    return y


def model_rows(kind, n_taps):
    """mf.model of the whole rows for JOBS: complex128 [4, NS], shared and left unchanged"""
    return _model_full(kind, n_taps)[:, :NS]


def model_tail(kind, n_taps):
    """the output behind the row's last one (the filter's tail over the zeros behind the row): complex128 [4]"""
    return _model_full(kind, n_taps)[:, NS]


# ---------------------------------------------------------------------------------------------------- the notebook's case

def notebook_case():
    """'Compress chirp in time domain': fs 44 100, a chirp 440 -> 1760 Hz of 0.02 s and amplitude 1000 at the phase -pi/2 at
    the head of a buffer of 0.04 s; the filter is the down chirp at the phase +pi/2 (882 taps).  (receive_buf, matched_filter),
    float64."""
    from uchirp import mf
    fs = 44100
    up = mf.chirp(440.0, 1760.0, fs, 0.02, 1000.0, -np.pi / 2.0, inclusive=True).real
    down = mf.chirp(1760.0, 440.0, fs, 0.02, 1000.0, np.pi / 2.0, inclusive=True).real
    buf = np.zeros(int(fs * 0.04))
    buf[:up.size] = up
    return buf, down


# --------------------------------------------------------------------------------------------------------------- the chain

CARRIER = 17500.0
DECIM = 8
LPF_TAPS = 65
MF_TAPS = 256
CHAIN_SAMPLES = 16384
CHAIN_FMT = dict(n_preamble=1, n_guard=1)              # silence, ONE up chirp, one down chirp, silence
SNR_DB = 1.0
AMPLITUDE = 2000.0


def chain_sigma():
    return AMPLITUDE * 10.0 ** (-SNR_DB / 20.0)


# the closure's microphones: two paths each, 150.5 samples apart, the later one weaker; (sigma, [(tx, gain, lead, ppm)])
CHAIN_MICS = [(chain_sigma(), [(0, AMPLITUDE, 500.25, 0.0), (0, AMPLITUDE * 0.5, 650.75, 0.0)]),
              (chain_sigma(), [(0, AMPLITUDE, 700.5, 0.0), (0, AMPLITUDE * 0.7, 851.0, 0.0)])]
CHAIN_SEED = 21
# what the CPU suite's chain test records: the worst |position - truth| of an arrival, in decimated samples, in float64
# (the GPU closure's bar against the truth is twice this)
CHAIN_RECORDED = 0.13


def chain_lpf():
    from uchirp import ddc
    return ddc.lpf_taps(FS, 1800.0, LPF_TAPS, window="hann")


def chain_template():
    """the Hann-weighted base-band up chirp of 255 taps at FS / 8, as the down-converter leaves it (it mixes with
    exp(+i w n), so the low-pass keeps the conjugate of the analytic pulse), reversed and conjugated, padded to 256"""
    from uchirp import tx
    n_sym = int(tx.T_SYMBOL * tx.FS_TX)
    tau = np.arange(MF_TAPS - 1) * DECIM / FS
    t = tau * tx.FS_TX * tx.T_SYMBOL / (n_sym - 1)                                     # the transmitter's time axis
    k = float(tx.F1 - tx.F0) / tx.T_SYMBOL
    theta = 2.0 * np.pi * (tx.F0 + k * t / 2.0) * t - 2.0 * np.pi * CARRIER * tau
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(MF_TAPS - 1) + 0.5) / (MF_TAPS - 1))
    pulse = np.exp(-1j * theta) * w
    return np.concatenate([np.conj(pulse[::-1]), [0.0]])


def chain_truth(lead):
    """where the compressor's crest of an arrival with this lead (samples at FS) lies, in decimated samples: the up chirp is
    the frame's second symbol; the low-pass delays it by (65 - 1) / 2 samples, the template by its 254"""
    from uchirp import tx
    start = float(lead) + int(tx.T_SYMBOL * tx.FS_TX) / float(tx.FS_TX) * FS
    return (start + (LPF_TAPS - 1) / 2.0) / DECIM + (MF_TAPS - 2)


def chain64(x):
    """rows at FS (float32 values) -> (base-band rows complex128, compressed rows complex128, candidates per row) in float64:
    ddc.model | mf.model | candidates64, for a call over the whole row at pos0 = 0"""
    from uchirp import ddc, mf
    z = ddc.model(chain_lpf(), x, DECIM, 0, steps=ddc.step_of(CARRIER, FS))
    y = mf.model(z.astype(np.complex64), chain_template())
    return z, y, [candidates64(r, MF_TAPS) for r in y]


def candidates64(y, n_taps):
    """the definition's candidates of one row of float64 outputs (a call from output 0 at pos0 = 0), segment by segment:
    [[(position, height, e), ...] by falling e].  Position and height are the parabola's through the square roots, the
    header's rule in float64 throughout.  The neighbours outside the row are taken as 0 (no crest of the tests lies there)."""
    hop = P - n_taps - 1
    n = y.size
    e = np.concatenate([[0.0], np.abs(y) ** 2, [0.0]])
    out = []
    for k in range((n - 1) // hop + 1):
        seg = []
        for q in range(k * hop, min(k * hop + hop, n)):
            l, v, r = e[q], e[q + 1], e[q + 2]
            if v >= l and v > r:
                a, b, c = np.sqrt(l), np.sqrt(v), np.sqrt(r)
                d = a - 2.0 * b + c
                delta = (a - c) / (2.0 * d) if d < 0.0 else 0.0
                seg.append((q + delta, b - (a - c) * delta / 4.0, v))
        out.append(sorted(seg, key=lambda t: (-t[2], t[0])))
    return out
