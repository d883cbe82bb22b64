"""Far sample positions in the link simulator and the scene renderer: the exact reference and the cases that
tests/test_far_cpu.py and tests/test_gpu_far.py share.

`exact_signal` is the definition of include/uchirp_link.h (lines "signal tt = ..." to "x = ...") in rational arithmetic
on the arguments' exact binary values, 1e-6 and 1e-10 being the numbers 10^-6 and 10^-10: the time, the symbol index, the
law's t, the frequency and the phase in turns are fractions, the phase is reduced mod 1 exactly, and one float64 cosine and
sine of the reduced phase follow.  Its own error is about 1e-15 A: under 0.001 ulp of float at the peak.  It is slow and
meant for the few thousand samples per stream that `chosen` picks."""
from fractions import Fraction as F
import math

import numpy as np

from uchirp import tx

N = 2048
FS = 78125.0
N_SAMPLES = 24 * N
N_STREAMS = 16
BASES = [2 ** 31 - 2048, 2 ** 32, 2 ** 33, 2 ** 34, 2 ** 36, 2 ** 40, 2 ** 44, 2 ** 48, 2 ** 52 - 2 ** 20]
PPMS = [0.0, 35.0, -35.0, 200.0, -200.0]
AMPS = [500.0, 2000.0, 8000.0, 20000.0]
FMT = dict(fs_tx=tx.FS_TX, t_symbol=tx.T_SYMBOL, f0=tx.F0, f1=tx.F1, n_preamble=tx.N_PREAMBLE, n_guard=tx.N_GUARD)
GUARD = F(1, 10 ** 10)


def ulp_of_peak(amplitude):
    """one float ulp at the peak A sqrt 2"""
    return float(np.spacing(np.float32(abs(float(np.float32(amplitude))) * 2 ** 0.5)))


class Frame:
    """The constants of one stream's definition as fractions."""

    def __init__(self, text, lead_samples, ppm, fs_out=FS, **fmt):
        fmt = dict(FMT, **fmt)
        raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
        bits = [(b >> (7 - i)) & 1 for b in raw for i in range(8)]
        self.seq = [-1] + [1] * fmt["n_preamble"] + [0] + bits + [-1] * fmt["n_guard"]     # -1: G, 1: H, 0: L
        self.n_on = 2 + fmt["n_preamble"] + len(bits)                                     # symbols 1 .. n_on - 1 sound
        fs_tx, t_symbol = float(fmt["fs_tx"]), float(fmt["t_symbol"])
        n_sym = int(t_symbol * fs_tx)
        self.sym_dur = F(n_sym) / F(fs_tx)
        self.t_scale = F(fs_tx) * F(t_symbol) / (n_sym - 1)
        self.f0, self.f1 = F(float(fmt["f0"])), F(float(fmt["f1"]))
        self.k = (self.f1 - self.f0) / F(t_symbol)
        self.fs_out = F(float(fs_out))
        self.stretch = 1 + F(float(np.float32(ppm))) / 10 ** 6
        self.lead = F(float(lead_samples))
        self.a, self.b = self.stretch / self.fs_out, self.lead / self.fs_out

    def time(self, j):
        """exact seconds since the frame began at absolute sample j"""
        return int(j) * self.a - self.b

    def seam(self, k):
        """the first sample whose symbol index is >= k (the index is taken at tt + 1e-10)"""
        return math.ceil((self.lead + (k * self.sym_dur - GUARD) * self.fs_out) / self.stretch)


def exact_signal(text, lead_samples, amplitude, ppm, js, fs_out=FS, **fmt):
    """(x, sounding): the definition's signal at the absolute samples js (float64) and whether each lies in a sounding
    symbol (x is exactly 0.0 where it does not)."""
    fr = Frame(text, lead_samples, ppm, fs_out, **fmt)
    amp = float(np.float32(amplitude))
    x, on = np.zeros(len(js), np.float64), np.zeros(len(js), bool)
    quarter = F(1, 4)
    for i, j in enumerate(js):
        tt = fr.time(j)
        idx = math.floor((tt + GUARD) / fr.sym_dur)
        if not 0 <= idx < len(fr.seq) or fr.seq[idx] < 0:
            continue
        t = max(tt - idx * fr.sym_dur, 0) * fr.t_scale
        f = fr.f0 + fr.k * t / 2 if fr.seq[idx] == 1 else fr.f1 - fr.k * t / 2
        ph = f * t - quarter                       # a / 2 pi, in turns
        ph -= round(ph)                            # exact, to [-1/2, 1/2]
        a = 2.0 * math.pi * float(ph)
        x[i], on[i] = amp * (math.cos(a) + math.sin(a)), True
    return x, on


def chosen(text, lead_samples, ppm, first_sample, n_samples, fs_out=FS, **fmt):
    """The samples of a call that the exact reference is taken at: every 97th, the call's last, and the eight around every
    symbol seam of the frame (the frame's first and last sounding sample are at seams 1 and n_on).  Sorted, absolute."""
    fr = Frame(text, lead_samples, ppm, fs_out, **fmt)
    first_sample, end = int(first_sample), int(first_sample) + int(n_samples)
    js = set(range(first_sample, end, 97)) | {end - 1}
    for k in range(len(fr.seq) + 1):
        jk = fr.seam(k)
        js.update(j for j in range(jk - 4, jk + 4) if first_sample <= j < end)
    return sorted(js)


def seam_margin(text, lead_samples, ppm, fs_out=FS, **fmt):
    """min over the frame's seams k and the two samples next to each of |tt + 1e-10 - k sym_dur| in seconds: the time is
    monotone in j, so no other sample comes nearer to a symbol boundary."""
    fr = Frame(text, lead_samples, ppm, fs_out, **fmt)
    worst = None
    for k in range(len(fr.seq) + 1):
        jk = fr.seam(k)
        for j in (jk - 1, jk):
            d = abs(fr.time(j) + GUARD - k * fr.sym_dur)
            worst = d if worst is None or d < worst else worst
    return worst


def link_case(base, first_sample=None, seed=0):
    """One call of 16 streams whose frames begin 1 to 6 blocks into it: one-character texts, ppm from {0, +-35, +-200},
    amplitudes from {500, 2000, 8000, 20000}, lead = (first_sample + off) (1 + ppm 1e-6) with a fractional off, rounded to
    double once; that double is every side's input."""
    first_sample = base if first_sample is None else first_sample
    rng = np.random.default_rng([int(base) % (1 << 63), seed])
    texts = [chr(int(c)) for c in rng.integers(33, 127, size=N_STREAMS)]
    ppm = np.array([PPMS[i % len(PPMS)] for i in range(N_STREAMS)], np.float32)
    amp = np.array([AMPS[(i // 2) % len(AMPS)] for i in range(N_STREAMS)], np.float32)
    off = [F(int(v), 1024) for v in rng.integers(1 * N * 1024, 6 * N * 1024, size=N_STREAMS)]
    lead = np.array([float((first_sample + o) * (1 + F(float(q)) / 10 ** 6)) for o, q in zip(off, ppm)], np.float64)
    return dict(base=base, first_sample=first_sample, n_samples=N_SAMPLES, texts=texts, lead=lead, amp=amp, ppm=ppm)


def link_cases():
    """Every base at first_sample = base, and 2^40 once more at base + 3: rows that start off the 16-byte grid."""
    return [link_case(b) for b in BASES] + [link_case(2 ** 40, 2 ** 40 + 3, seed=1)]


def case_name(c):
    b, extra = c["base"], c["first_sample"] - c["base"]
    e = b.bit_length() - 1 if b & (b - 1) == 0 else b.bit_length()
    name = "2^%d" % e if b == 1 << e else "2^%d-%d" % (e, (1 << e) - b)
    return name + ("+%d" % extra if extra else "")


def old_time(lead_samples, ppm, js, fs_out=FS):
    """The time as the kernels took it before: ONE double fma of j * rate - lead_s on rate = (1 / fs_out) (1 + ppm 1e-6) and
    lead_s = lead / fs_out in double (each rounding here is a correctly rounded fraction -> float)."""
    ppm, fs_out = float(np.float32(ppm)), float(fs_out)
    rate, lead_s = (1.0 / fs_out) * (1.0 + ppm * 1e-6), float(lead_samples) / fs_out
    fr, fl = F(rate), F(lead_s)
    return np.array([float(int(j) * fr - fl) for j in js], np.float64)
