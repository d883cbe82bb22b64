"""Tone sweeps for the frame kernels: input builders and the oracle-side bookkeeping.

Every case is one batch in which frame i puts a tone on ONE bin of the dechirped spectrum, so that every bin of both
search windows is, in some frame, the maximum the kernel has to find -- with its own lane, twiddle and place in the
first-max search -- instead of one of the many bins that only ever have to stay below the modem's own peak.

Nothing here is derived from sign conventions: for every frame, history and window the float64 oracle spectrum says
which bin wins and whether it wins CLEARLY (second-largest bin of the window <= CLEAR x the largest, in a window that
holds the signal).  The tests compare indices exactly on the clear ones and count which bins that reaches.

  tests/test_tone_sweep_cpu.py    oracle only: the builders cover what the GPU test relies on
  tests/test_gpu_tone_sweep.py    the kernels against that
"""
import functools

import numpy as np

from oracle import uco

CLEAR = 0.99            # "clear": second-largest bin of the window <= 0.99 x the largest
SIGNAL = 0.1            # ... and the window's largest bin >= 0.1 x the frame's largest WINDOW magnitude, which is what the
#                         magnitude bar is relative to: SYNC_CPLX and I/Q spectra are one-sided, the window across DC from
#                         the tone holds leakage 1e-6 of it, and float32 cannot order that.  A clear lead is then
#                         >= 0.01 x 0.1 / MAG_TOL = 50 bars, where two (one per bin) could overturn it
APART = 0.01            # max_freq is compared where the two window maxima differ by more than 1 % of the larger:
#                         GPU and oracle are each within MAG_TOL = 2e-5 of it, a lead of 500 such bars
HALO = 26               # FIR history in front of every I/Q frame
AMP = 1000.0

BAND = {"rx_real": uco.RX_REAL, "sync_cplx": uco.SYNC_CPLX, "dechirp_down": uco.DECHIRP_DOWN}

# (name, variant, engine/oracle configuration, recipe, {expected geometry}).  The geometry selects the kernel build and
# is asserted by the tests: bandwidth2 <= 191 the two-round band build, above it WIDE; I/Q base band: bandwidth
# <= 32 (n 1024) / <= 64 (n 2048) the one-bin-per-lane build BB = 2, above it BB = 1; without the flag BB = 0.
_BB = dict(fs=100000.0, carrier=18000.0, flags=uco.FLAG_IQ_BASEBAND)
_FW = dict(fs=100000.0, f0=2750.0, f1=4250.0, carrier=5000.0)
CASES = {
    # band kernel, default two-round build (bandwidth2 156)
    "rx_real-literal": ("rx_real", dict(), "chirp", dict(bw2=156)),
    "rx_real-matched": ("rx_real", dict(time_frame=2048.0 / 78125.0), "chirp", dict(bw2=156)),
    "sync_cplx-literal": ("sync_cplx", dict(), "chirp", dict(bw2=156)),
    "sync_cplx-matched": ("sync_cplx", dict(time_frame=2048.0 / 78125.0), "chirp", dict(bw2=156)),
    "dechirp_down-default": ("dechirp_down", dict(), "ref_tone", dict(bw2=160)),
    # band kernel, WIDE build: the geometries of tests/test_gpu_wide.py
    "rx_real-wide294": ("rx_real", dict(fs=125000.0 / 3.0, time_frame=2048.0 / (125000.0 / 3.0)), "chirp", dict(bw2=294)),
    "rx_real-wide318": ("rx_real", dict(fs=38600.0, time_frame=2048.0 / 38600.0), "chirp", dict(bw2=318)),
    "sync_cplx-wide294": ("sync_cplx", dict(fs=125000.0 / 3.0, time_frame=2048.0 / (125000.0 / 3.0)), "chirp", dict(bw2=294)),
    "sync_cplx-wide318": ("sync_cplx", dict(fs=38600.0, f0=12000.0, f1=15000.0, time_frame=2048.0 / 38600.0), "chirp",
                          dict(bw2=318)),
    "dechirp_down-wide240": ("dechirp_down", dict(fs=100000.0, f0=17000.0, f1=18500.0), "ref_tone", dict(bw2=240)),
    "dechirp_down-wide312": ("dechirp_down", dict(fs=100000.0, f0=17000.0, f1=18930.0), "ref_tone", dict(bw2=312)),
    # I/Q, base band: BASELINE configs[2] (BB = 2) and the first windows past it (BB = 1)
    "iq1024-bb2": ("iq", dict(_BB, n=1024, f0=16500.0, f1=19500.0), "iq_bb", dict(bw2=30)),
    "iq2048-bb2": ("iq", dict(_BB, n=2048, f0=16500.0, f1=19500.0), "iq_bb", dict(bw2=61)),
    "iq1024-bb1": ("iq", dict(_BB, n=1024, f0=16350.0, f1=19650.0), "iq_bb", dict(bw2=33)),
    "iq2048-bb1": ("iq", dict(_BB, n=2048, f0=16400.0, f1=19600.0), "iq_bb", dict(bw2=65)),
    # I/Q, the firmware's windows (BB = 0): the constants of test_firmware_windows_with_the_tone_inside
    "iq1024-bb0": ("iq", dict(_FW, n=1024), "iq_fw", dict(bw2=30)),
    "iq2048-bb0": ("iq", dict(_FW, n=2048), "iq_fw", dict(bw2=60)),
}

# The seams of the band kernel's window search (csrc/uc_band_kernel.hip): the widths at which bin bandwidth2 -- the left window's
# first element -- changes its owner.  Default build: thread j owns bin j, wave 1 also bin 128 + lane; bin bandwidth2 belongs to
# wave 0 below 64, to wave 1 from 64 (slot 0) and from 128 (slot 1, lane 0 first); wave 1 has no common bins up to 64 and no
# slot-1 bins up to 128.  WIDE build (from 192): the third round, 256 + lane on wave 1, has its first bin at 256.
SEAM_WIDTHS = {
    "rx_real": (2, 62, 64, 66, 126, 128, 130, 190, 192, 254, 256, 258),
    "sync_cplx": (2, 62, 64, 66, 126, 128, 130, 190, 192, 254, 256, 258),
    "dechirp_down": (8, 56, 64, 72, 120, 128, 136, 184, 192, 248, 256, 264),
}


def _band(b, fs, f0):
    """The band that gives `bandwidth` b: (f1 - f0) n / fs = b + 0.5 -- the half bin keeps the float32 truncation of
    build_tables away from an integer."""
    return dict(f0=f0, f1=f0 + (b + 0.5) * fs / 2048)


def seam_name(kind, bw2):
    return "%s-%s%d" % (kind, "wide" if bw2 > 191 else "w", bw2)


for _kind, _widths in SEAM_WIDTHS.items():
    for _w in _widths:
        if _kind == "dechirp_down":       # bandwidth2 = 8 x bandwidth
            CASES[seam_name(_kind, _w)] = (_kind, dict(fs=100000.0, **_band(_w // 8, 100000.0, 17000.0)), "ref_tone", dict(bw2=_w))
        else:                             # bandwidth2 = 2 x bandwidth, at the default 78 125 Hz and time_frame
            CASES[seam_name(_kind, _w)] = (_kind, _band(_w // 2, 78125.0, 14000.0), "chirp", dict(bw2=_w))
SEAM_CASES = [seam_name(k, w) for k, ws in SEAM_WIDTHS.items() for w in ws]


def config(name):
    """(variant, keyword arguments of Oracle / Engine) of a case; mag_mean is the caller's."""
    kind, cfg, _, _ = CASES[name]
    cfg = dict(cfg)
    if kind == "iq":
        cfg.setdefault("time_frame", cfg["n"] / cfg["fs"])
        return uco.IQ, cfg
    return BAND[kind], cfg


def _chirp(n, fs, f0, f1, tf, up, shift_hz):
    """synth.chirp_pair's law (the transmitter's orthogonal chirp) with every frequency moved by shift_hz."""
    t = np.arange(n, dtype=np.float64) / fs
    k = (f1 - f0) / tf
    f = (f0 + k * t / 2.0) if up else (f1 - k * t / 2.0)
    arg = 2.0 * np.pi * (f + shift_hz) * t - np.pi / 2.0
    return AMP * (np.cos(arg) + np.sin(arg))


def build_frames(name, o):
    """float64 [n_frames, n] and, per frame, the b the recipe was given (bookkeeping only: what a frame's tone does is
    read off the oracle's spectrum, never off b).  `o`: an Oracle of the case (tables, geometry)."""
    kind, _, recipe, _ = CASES[name]
    n, fs, bw2 = o.n, float(o.cfg.fs), o.bandwidth2
    tf = float(o.cfg.time_frame) if o.cfg.time_frame > 0 else n / fs
    f0, f1 = float(o.cfg.f0), float(o.cfg.f1)
    t = np.arange(n, dtype=np.float64)
    frames, bs = [], []
    if recipe == "chirp" and kind == "rx_real":
        for up in (True, False):
            for b in range(0, bw2 + 2):
                frames.append(_chirp(n, fs, f0, f1, tf, up, b * fs / n))
                bs.append(b)
    elif recipe == "chirp":
        for up in (True, False):
            for b in range(-bw2 - 1, bw2 + 2):
                frames.append(_chirp(n, fs, f0, f1, tf, up, -b * fs / n))
                bs.append(b)
    elif recipe == "ref_tone":
        ref = o.table(uco.TABLE_DOWN).astype(np.float64)
        for b in range(0, bw2 + 2):
            frames.append(AMP * ref * np.cos(2.0 * np.pi * b * t / n + 0.3))
            bs.append(b)
    elif recipe == "iq_bb":
        carrier, bw = float(o.cfg.carrier), f1 - f0
        ts = t / fs
        k = bw / (n / fs)
        for up in (True, False):
            fb = (-bw / 2 + k * ts / 2.0) if up else (bw / 2 - k * ts / 2.0)
            for b in range(-bw2 - 3, bw2 + 4):
                frames.append(AMP * np.cos(2.0 * np.pi * (carrier - fb - b * fs / n) * ts))
                bs.append(b)
    elif recipe == "iq_fw":
        d = o.table(uco.TABLE_DOWN).astype(np.float64)
        ref = d[0::2] + 1j * d[1::2]
        car = o.table(uco.TABLE_CARRIER_C).astype(np.float64) + 1j * o.table(uco.TABLE_CARRIER_S).astype(np.float64)
        lo = o.idx_left_zero
        for k in range(lo, lo + 2 * bw2):
            frames.append(AMP * np.real(ref * car * np.exp(-2j * np.pi * k * t / n)))
            bs.append(k)
    else:
        raise ValueError(recipe)
    return np.stack(frames), np.array(bs)


def to_dtype(x, dtype):
    """float32 samples, or DFSDM words: the 24-bit sample in bits 31:8."""
    if dtype == np.int32:
        return (np.round(x).astype(np.int64) * 256).astype(np.int32)
    return x.astype(np.float32)


def lay_out(frames, n, halo=0, stride=None):
    """One buffer with frame f at [f * stride, f * stride + halo + n): `halo` zeros, then the frame.

    stride None: frames (each behind its own halo) back to back, so no frame depends on its neighbour and a batch may
    be permuted.  A stride < n overlaps the frames; where two frames share samples the EARLIER frame's values stand (at
    stride n - 1 the shared sample is the later frame's sample 0, which the periodic Hann weights with 0)."""
    nf = len(frames)
    stride = (halo + n) if stride is None else stride
    buf = np.zeros((nf - 1) * stride + halo + n, frames.dtype)
    for f in range(nf - 1, -1, -1):
        buf[f * stride: f * stride + halo] = 0
        buf[f * stride + halo: f * stride + halo + n] = frames[f]
    return buf, stride


def windows_of(o, firmware):
    """{'right': (a, b), 'left': (a, b)}: the FFT bins behind max_freq_right / max_freq_left."""
    if firmware:      # experiments/iq_modulation: [lo, center) and [center, center + bw2)
        lo, bw2 = o.idx_left_zero, o.bandwidth2
        return {"left": (lo, lo + bw2), "right": (lo + bw2, lo + 2 * bw2)}
    return {"right": (0, o.bandwidth2), "left": (o.idx_left_zero, o.n)}


class Sweep:
    """What the oracle says about one laid-out batch: records, and per (history, side, frame) the winning bin, whether
    it is clear, and per (history, frame) whether the two window maxima are APART."""

    def __init__(self, o, buf, n_frames, stride, halo, firmware=False, raw_idx=False):
        self.o, self.buf, self.n_frames, self.stride, self.halo = o, buf, n_frames, stride, halo
        self.firmware, self.raw_idx = firmware, raw_idx
        self.real_spectrum = o.cfg.variant in (uco.RX_REAL, uco.DECHIRP_DOWN)
        self.windows = windows_of(o, firmware)
        self._inv = {}
        self.symbols, self.records = o.process(buf, halo=halo, stride=stride, n_frames=n_frames)
        spf = o.spf
        self.win = {s: np.zeros((spf, n_frames), np.int64) for s in self.windows}
        self.clear = {s: np.zeros((spf, n_frames), bool) for s in self.windows}
        self.ratio = {s: np.zeros((spf, n_frames)) for s in self.windows}       # second / first of the window
        self.apart = np.zeros((spf, n_frames), bool)
        self.side_of_max = np.zeros((spf, n_frames), "U5")
        for f in range(n_frames):
            spec = self.spectrum(f)
            for h in range(spf):
                top = {}
                scale = max(spec[h][a:b].max() for a, b in self.windows.values())
                for s, (a, b) in self.windows.items():
                    w = spec[h][a:b]
                    i = int(np.argmax(w))              # first maximum, as arm_max_f32
                    second = np.partition(w, -2)[-2]
                    top[s] = w[i]
                    self.win[s][h, f] = a + i
                    self.ratio[s][h, f] = second / max(w[i], 1e-300)
                    self.clear[s][h, f] = w[i] > 0 and second <= CLEAR * w[i] and w[i] >= SIGNAL * scale
                big = max(top.values())
                self.apart[h, f] = abs(top["left"] - top["right"]) > APART * big
                self.side_of_max[h, f] = "left" if top["left"] > top["right"] else "right"

    def frame(self, f):
        return self.buf[f * self.stride: f * self.stride + self.halo + self.o.n]

    def spectrum(self, f):
        return self.o.spectrum(self.frame(f), halo=self.halo)

    def bin_of_record(self, side, v):
        """The FFT bin of that window behind a record's max_freq_left / max_freq_right."""
        a, b = self.windows[side]
        if self._inv.get(side) is None:
            self._inv[side] = {self.record_of_bin(side, k): k for k in range(a, b)}
            assert len(self._inv[side]) == b - a          # injective inside a window
        return self._inv[side][int(v)]

    def record_of_bin(self, side, k):
        """What the records hold for FFT bin k of that window (frequencies; DECHIRP_DOWN: raw indices)."""
        if self.raw_idx:
            return k if side == "right" else self.o.n - k
        return self.o.idx2freq(k)

    def coverage(self, per_history=False):
        """{(side, bin)} -- or {(history, side, bin)} -- that are the clear winner of their window in >= 1 frame."""
        out = set()
        for s in self.windows:
            for h in range(self.o.spf):
                for k in np.unique(self.win[s][h][self.clear[s][h]]):
                    out.add((h, s, int(k)) if per_history else (s, int(k)))
        return out

    def whole(self):
        return {(s, k) for s, (a, b) in self.windows.items() for k in range(a, b)}


def exact_comparisons(sw, g, h):
    """The exact rule on history h of GPU records g[:, h]: wherever the oracle's window winner is clear, the GPU's
    max_freq_left / max_freq_right IS the oracle's; and max_freq too where the window maxima are APART and the winning
    side is clear.  -> (set of (side, bin) compared, number of comparisons, list of failures)."""
    r = sw.records[:, h]
    hit, count, bad = set(), 0, []
    for s in sw.windows:
        fld = "max_freq_" + s
        for f in np.nonzero(sw.clear[s][h])[0]:
            count += 1
            hit.add((s, int(sw.win[s][h, f])))
            if g[fld][f] != r[fld][f]:
                bad.append((h, f, fld, int(g[fld][f]), int(r[fld][f])))
    for f in np.nonzero(sw.apart[h])[0]:
        if sw.clear[str(sw.side_of_max[h, f])][h, f]:
            count += 1
            if g["max_freq"][f] != r["max_freq"][f]:
                bad.append((h, f, "max_freq", int(g["max_freq"][f]), int(r["max_freq"][f])))
    return hit, count, bad


PERM_SEED = 20240611


def permutation(n_frames, keep_pairs=False):
    """A fixed permutation of the frames; keep_pairs: of the frame PAIRS (2u, 2u + 1), each pair left as it is."""
    rng = np.random.default_rng(PERM_SEED)
    if not keep_pairs:
        return rng.permutation(n_frames)
    pairs = rng.permutation(n_frames // 2)
    perm = np.stack([2 * pairs, 2 * pairs + 1], axis=1).reshape(-1)
    return np.concatenate([perm, np.arange(2 * (n_frames // 2), n_frames)])


@functools.lru_cache(maxsize=None)
def batch(name, dtype_name="float32", stride=None, perm=None):
    """The laid-out batch of a case (built once per process and argument set) -> (Oracle, buffer, n_frames, stride, halo,
    order).  perm: None, 'frames' or 'pairs' -- the batch in the fixed permutation, order[i] the recipe's frame at place i."""
    dtype = np.dtype(dtype_name).type
    variant, cfg = config(name)
    scale = 256.0 if dtype == np.int32 else 1.0
    o = uco.Oracle(variant, mag_mean=1000.0 * scale, **cfg)
    frames, _ = build_frames(name, o)
    order = np.arange(len(frames))
    if perm is not None:
        order = permutation(len(frames), keep_pairs=(perm == "pairs"))
    halo = HALO if variant == uco.IQ else 0
    buf, st = lay_out(to_dtype(frames[order], dtype), o.n, halo=halo, stride=stride)
    return o, buf, len(frames), st, halo, order


@functools.lru_cache(maxsize=None)
def sweep(name, dtype_name="float32", stride=None, perm=None):
    """batch() and the oracle's account of it -> (Sweep, order)."""
    o, buf, n_frames, st, halo, order = batch(name, dtype_name, stride, perm)
    variant, _ = config(name)
    return Sweep(o, buf, n_frames, st, halo, firmware=(CASES[name][2] == "iq_fw"), raw_idx=(variant == uco.DECHIRP_DOWN)), order

def noisy_stream(name, dtype_name="float32", n_frames=200):
    """The -10 dB stream of tests/test_gpu_iq_baseband.py (synth.iq_stream, the notebook's modulation) in the geometry
    of an I/Q base-band case -> (stream behind HALO zeros, transmitted bits, Oracle)."""
    from uchirp import synth
    variant, cfg = config(name)
    scale = 256.0 if dtype_name == "int32" else 1.0
    o = uco.Oracle(variant, mag_mean=1000.0 * scale, **cfg)
    x, bits = synth.iq_stream(n_frames, cfg["n"], fs=cfg["fs"], carrier=cfg["carrier"], bw=cfg["f1"] - cfg["f0"],
                              sigma=AMP * 10 ** 0.5, seed=3 + cfg["n"])
    return to_dtype(x.astype(np.float64), np.dtype(dtype_name).type), bits, o


def prove_near_ties(sw, g, h, tol, label):
    """Every index mismatch between GPU records g (history h) and the oracle's must be a near-tie in the oracle's float64
    spectrum: the GPU's bin within tol x (the frame's largest window magnitude) of its window's maximum.  This is
    parity_util.prove_ties with the scale of the MAGNITUDE bar (parity_util.window_scale) in place of the one window's own
    maximum, as test_gpu_parity._iq_prove_ties has it: the tone of a one-sided spectrum leaves the window across DC
    leakage 1e-6 of the frame's peak, which no float32 transform can order.  -> number of near-ties proven."""
    r = sw.records[:, h]
    bad = np.nonzero((g["max_freq"] != r["max_freq"]) | (g["max_freq_left"] != r["max_freq_left"])
                     | (g["max_freq_right"] != r["max_freq_right"]))[0]
    for f in bad:
        spec = sw.spectrum(f)[h]
        top = {s: spec[a:b].max() for s, (a, b) in sw.windows.items()}
        scale = max(top.values())
        for s in sw.windows:
            fld = "max_freq_" + s
            if g[fld][f] != r[fld][f]:
                gi = sw.bin_of_record(s, g[fld][f])
                assert top[s] - spec[gi] <= tol * scale, \
                    "%s frame %d %s: GPU bin %d is not a near-tie (%.6g vs max %.6g)" % (label, f, fld, gi, spec[gi], top[s])
        if g["max_freq"][f] != r["max_freq"][f]:
            assert g["max_freq"][f] in (g["max_freq_left"][f], g["max_freq_right"][f]), "%s frame %d" % (label, f)
            side_same = (g["max_freq"][f] == g["max_freq_left"][f]) == (r["max_freq"][f] == r["max_freq_left"][f])
            if not side_same or g["max_freq_left"][f] == g["max_freq_right"][f]:
                assert abs(top["left"] - top["right"]) <= tol * scale, \
                    "%s frame %d: left/right winner differs without a near-tie" % (label, f)
    return len(bad)
