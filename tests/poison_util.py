"""One non-finite sample: which outputs of a call it reaches, by index arithmetic alone.

For every library of LIBRARIES (array, retime, rate, align, xcorr, track, wcorr, spec, mf) the header's paragraph
"Non-finite samples" names three zones for one non-finite float sample at row element q:
  MUST      outputs whose defining sum has a term with x[q]: they are not finite;
  MAY       further outputs this implementation may turn non-finite, each bit-identical to the clean call's or not finite;
  MUST NOT  everything else the call writes: bit for bit what the clean call writes.
A case holds small inputs, poison positions and the two masks `reads(pos)` (MUST) and `may(pos)` (MAY, without MUST) over
what ONE copy of the inputs writes.  tests/test_poison_cpu.py proves the masks against the float64 models without a GPU
(it moves x[q] by a finite amount and looks at which outputs change); tests/test_gpu_poison.py puts many copies, each
with one poisoned sample, into one call and compares zones with the clean call of the same shape.

A position is (label, row, q, part, want): `part` is "re" / "im" for complex rows (None otherwise) and `want` the zones
the position is there to hit: a subset of {"must", "may"}; empty for a sample just outside every zone.  Position
arithmetic that a library's host functions own (uc_mf_plan, uc_spec_frames, uc_rate_plan / _count / _step,
uc_array_tap_coefficients, uc_retime_fixed, uc_wcorr_band_weights) goes through the ctypes bindings.
"""
import collections

import numpy as np

from uchirp import align, array, mf, rate, retime, spec, track, wcorr, xcorr

Pos = collections.namedtuple("Pos", "label row q part want")

POISONS = (("nan", np.float32(np.nan)), ("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)))
GRIDS = (None, 1, 2)          # UC_<LIB>_GRID: the default, one workgroup walking every unit back to back, and two


def rows_f32(seed, n_rows, n_in):
    """standard normal x 1000, float32"""
    return (np.random.default_rng(seed).standard_normal((n_rows, n_in)) * 1000.0).astype(np.float32)


def poisoned(rows, pos, value):
    """a copy of `rows` with the sample of `pos` replaced by `value` (the real or the imaginary part alone for complex rows)"""
    out = rows.copy()
    if pos.part is None:
        out[pos.row, pos.q] = value
    elif pos.part == "re":
        out[pos.row, pos.q] = complex(value, out[pos.row, pos.q].imag)
    else:
        out[pos.row, pos.q] = complex(out[pos.row, pos.q].real, value)
    return out


def moved(rows, pos, delta=37.0):
    """a copy of `rows` with the sample of `pos` moved by a finite amount"""
    out = rows.copy()
    if pos.part is None or pos.part == "re":
        out[pos.row, pos.q] += delta
    else:
        out[pos.row, pos.q] += 1j * delta
    return out


# ------------------------------------------------------------------------------------------------- xcorr and align

class CorrCase:
    """uc_xcorr_correlate / uc_align_correlate over two rows and the pairs (0, 1) and (1, 1): row 0 is a reference only,
    row 1 the microphone of both pairs and the reference of the second (ref = mic).  What a copy writes: corr [2, 2 L + 1]."""
    PAIRS = ((0, 1), (1, 1))

    def __init__(self, lib, name, n_in, first, n, L, positions, seed):
        self.lib, self.name = lib, "%s-%s" % (lib, name)
        self.n_in, self.first, self.n, self.L = n_in, first, n, L
        self.rows = rows_f32(seed, 2, n_in)
        self.positions = positions

    @property
    def n_up(self):
        """align: the reference range as the kernel walks it -- every segment in passes of 256 samples, so the last one
        rounded up; xcorr pads nothing"""
        if self.lib != "align":
            return self.n
        i0 = (self.n - 1) // align.SEGMENT * align.SEGMENT
        return i0 + -(-(self.n - i0) // 256) * 256

    def model(self, rows):
        m = xcorr.model if self.lib == "xcorr" else align.model
        return {"corr": m(rows, list(self.PAIRS), first=self.first, n=self.n, max_lag=self.L)}

    def _lags(self):
        return np.arange(-self.L, self.L + 1)

    def reads(self, pos):
        """r_p[l] has the term x_ref[j] x_mic[j + l], j in [first, first + n): with x[q] as the reference's sample for every
        l, as the microphone's for first <= q - l < first + n"""
        l = self._lags()
        out = np.zeros((len(self.PAIRS), l.size), bool)
        for p, (ref, mic) in enumerate(self.PAIRS):
            if pos.row == ref and self.first <= pos.q < self.first + self.n:
                out[p] = True
            if pos.row == mic:
                out[p] |= (self.first <= pos.q - l) & (pos.q - l < self.first + self.n)
        return {"corr": out}

    def zero_terms(self, pos):
        """the terms of `reads` whose other factor is exactly zero: x[q] as a reference sample times a microphone sample
        outside the row, which reads as +0"""
        l = self._lags()
        out = np.zeros((len(self.PAIRS), l.size), bool)
        for p, (ref, mic) in enumerate(self.PAIRS):
            if pos.row == ref and self.first <= pos.q < self.first + self.n:
                out[p] = (pos.q + l < 0) | (pos.q + l >= self.n_in)
                if pos.row == mic:   # ... unless the same sample is a microphone sample of that lag as well
                    out[p] &= ~((self.first <= pos.q - l) & (pos.q - l < self.first + self.n))
        return {"corr": out}

    def may(self, pos):
        """xcorr: a pair's sums come out of one inverse transform, so the lags of a pair with a MUST lag that the definition
        does not reach.  align: lag l also multiplies the microphone samples of the last pass's padded lanes,
        first + n <= q - l < first + n_up."""
        must = self.reads(pos)["corr"]
        if self.lib == "xcorr":
            return {"corr": must.any(axis=1)[:, None] & ~must}
        l = self._lags()
        out = np.zeros_like(must)
        for p, (ref, mic) in enumerate(self.PAIRS):
            if pos.row == mic:
                out[p] = (self.first + self.n <= pos.q - l) & (pos.q - l < self.first + self.n_up)
        return {"corr": out & ~must}


def _corr_edges(first, n, L, lo_may, hi_may):
    """the eight range edges: the reference's first - 1 / first / first + n - 1 / first + n, the microphone's
    first - L - 1 / first - L / first + n + L - 1 / first + n + L"""
    m = {"must"}
    return [Pos("ref first-1", 0, first - 1, None, set()), Pos("ref first", 0, first, None, m),
            Pos("ref first+n-1", 0, first + n - 1, None, m), Pos("ref first+n", 0, first + n, None, set()),
            Pos("mic first-L-1", 1, first - L - 1, None, set()), Pos("mic first-L", 1, first - L, None, m | lo_may),
            Pos("mic first+n+L-1", 1, first + n + L - 1, None, m | hi_may)]


def corr_cases():
    both = {"must", "may"}
    out = []
    # ---- xcorr: one segment; five segments in two groups, with q on a segment seam; the row clipping the window
    f, n, L = 700, 1500, 64
    out.append(CorrCase("xcorr", "L64", 6000, f, n, L, _corr_edges(f, n, L, {"may"}, {"may"}) +
                        [Pos("mic first+n+L", 1, f + n + L, None, set())], seed=11))
    f, n, L = 600, 4200, 512
    S = xcorr.POINTS - 2 * L
    out.append(CorrCase("xcorr", "L512", 6000, f, n, L, _corr_edges(f, n, L, {"may"}, {"may"}) +
                        [Pos("mic first+n+L", 1, f + n + L, None, set()),
                         Pos("ref seam-1", 0, f + S - 1, None, {"must"}), Pos("ref seam", 0, f + S, None, {"must"}),
                         Pos("mic group seam-1", 1, f + 4 * S - 1, None, both), Pos("mic group seam", 1, f + 4 * S, None, both)],
                        seed=12))
    out.append(CorrCase("xcorr", "clip", 6000, 0, 6000, 512,
                        [Pos("ref 0", 0, 0, None, {"must"}), Pos("ref last", 0, 5999, None, {"must"}),
                         Pos("mic 0", 1, 0, None, both), Pos("mic last", 1, 5999, None, both)], seed=13))
    # ---- align: a second, short segment with a partial pass (300 samples: two passes, 212 padded lanes)
    for L, seed in ((5, 21), (64, 22)):
        f, n = 300, align.SEGMENT + 300
        c = CorrCase("align", "L%d" % L, 5400, f, n, L, [], seed=seed)
        up = c.n_up
        assert up == align.SEGMENT + 512
        c.positions = _corr_edges(f, n, L, set(), {"may"}) + [
            Pos("mic first+n+L", 1, f + n + L, None, {"may"}),
            Pos("mic pad mid", 1, f + n + 100, None, {"may"}),
            Pos("mic pad last", 1, f + up + L - 1, None, {"may"}),          # just inside the bound: lag +L alone
            Pos("mic pad end", 1, f + up + L, None, set()),                  # just outside
            Pos("ref seam-1", 0, f + align.SEGMENT - 1, None, {"must"}), Pos("ref seam", 0, f + align.SEGMENT, None, {"must"}),
            Pos("mic seam", 1, f + align.SEGMENT, None, {"must"})]
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------ mf

class MfCase:
    """uc_mf_run over one row through two templates (two jobs).  What a copy writes: y [2, n] and rec [2, n_segments]."""
    T = 255
    JOBS = ((0, 0), (0, 1))

    def __init__(self, name, pos0, is_complex, seed):
        self.lib, self.name = "mf", "mf-%s" % name
        self.pos0, self.complex = pos0, is_complex
        self.hop = mf.POINTS - self.T - 1
        self.n_in = 2 * self.hop + 700
        self.first, self.n = 100, self.n_in - 300                          # the last 200 elements lie behind first + n
        rng = np.random.default_rng(seed)
        if is_complex:
            self.rows = ((rng.standard_normal((1, self.n_in)) + 1j * rng.standard_normal((1, self.n_in))) * 1000.0).astype(np.complex64)
        else:
            self.rows = rows_f32(seed, 1, self.n_in)
        self.taps = (rng.standard_normal((2, self.T)) + 1j * rng.standard_normal((2, self.T))).astype(np.complex64)
        hop, self.k0, self.ns = mf.plan(self.T, pos0, self.first, self.n)   # uc_mf_plan
        assert hop == self.hop and self.ns == 3
        # row element of output 0 of the call's segments
        self.base = [(self.k0 + s) * self.hop - pos0 for s in range(self.ns)]
        b, T, S = self.base[1], self.T, self.hop
        parts = ("re", "im") if is_complex else (None,)
        both = {"must", "may"}
        self.positions = []
        for part in parts:
            self.positions += [
                # (a MUST output's segment always has further outputs that no term reaches: MAY is never empty with it)
                Pos("base-T-1", 0, b - T - 1, part, both),                  # segment 0 alone
                Pos("base-T", 0, b - T, part, both),                        # the window's first element: no sum of segment 1 reads it
                Pos("base-T+1", 0, b - T + 1, part, both),
                Pos("base+S-1", 0, b + S - 1, part, both),
                Pos("base+S", 0, b + S, part, both),                        # the window's last element
                Pos("base+S+1", 0, b + S + 1, part, both),                  # segment 2 alone
                Pos("row 0", 0, 0, part, both),
                Pos("first+n", 0, self.first + self.n, part, {"may"}),      # inside the row, behind first + n
                Pos("row last", 0, self.n_in - 1, part, {"may"})]

    def model(self, rows):
        return {"y": mf.model(rows, self.taps, list(self.JOBS), first=self.first, n=self.n)}

    def _segment_of_output(self):
        """the call's segment of every output"""
        return (self.pos0 + self.first + np.arange(self.n)) // self.hop - self.k0

    def _windows(self, q):
        """the call's segments whose window base - T .. base + S holds row element q"""
        return np.array([b - self.T <= q <= b + self.hop for b in self.base])

    def reads(self, pos):
        """y of row element e has the term h[e - q] x[q] for e - T + 1 <= q <= e; a record is computed from its segment's e"""
        e = self.first + np.arange(self.n)
        y = np.tile((e - self.T + 1 <= pos.q) & (pos.q <= e), (len(self.JOBS), 1))
        seg = self._segment_of_output()
        rec = np.array([[y[j, seg == s].any() for s in range(self.ns)] for j in range(len(self.JOBS))])
        return {"y": y, "rec": rec}

    def zero_terms(self, pos):
        return {"y": np.zeros((len(self.JOBS), self.n), bool)}

    def may(self, pos):
        """the outputs of every segment whose window holds q: a segment comes out of one inverse transform"""
        must = self.reads(pos)
        win = self._windows(pos.q)
        y = np.tile(win[self._segment_of_output()], (len(self.JOBS), 1))
        rec = np.tile(win, (len(self.JOBS), 1))
        return {"y": y & ~must["y"], "rec": rec & ~must["rec"]}


def mf_cases():
    return [MfCase("c32-pos0", 0, True, 31), MfCase("c32-far", 2 ** 40 + 5, True, 32), MfCase("f32-far", 2 ** 40 + 5, False, 33),
            MfCase("f32-pos0", 0, False, 34)]


# ---------------------------------------------------------------------------------------------------------- spec

class SpecCase:
    """uc_spec_run over one row: frames of 300 samples under the periodic Hann, whose first coefficient is exactly zero.  What
    a copy writes: out [1, n_frames, n_bins] and one peak record a frame.  The kinds (MAG, POWER, DB) share one reach."""
    FRAME_LEN, N_IN, FIRST = 300, 1000, -50

    def __init__(self, name, hop, ac_bins, bin_first, n_bins, positions, seed):
        self.lib, self.name = "spec", "spec-%s" % name
        self.hop, self.ac_bins, self.bin_first = hop, ac_bins, bin_first
        self.n_bins = spec.BINS - bin_first if n_bins is None else n_bins
        self.rows = rows_f32(seed, 1, self.N_IN)
        self.n_frames = spec.frames(self.N_IN, self.FIRST, self.FRAME_LEN, hop)       # uc_spec_frames
        self.positions = positions

    def kw(self, kind=spec.MAG):
        return dict(hop=self.hop, first=self.FIRST, bin_first=self.bin_first, n_bins=self.n_bins, ac_bins=self.ac_bins, kind=kind)

    def model(self, rows):
        return {"out": spec.model(rows, frame_len=self.FRAME_LEN, **self.kw())}

    def frames_of(self, q):
        """the frames with first + f hop <= q < first + f hop + frame_len"""
        s = self.FIRST + self.hop * np.arange(self.n_frames)
        return (s <= q) & (q < s + self.FRAME_LEN)

    def reads(self, pos):
        """every stored bin of a frame that holds q -- but a bin below ac_bins stores its constant"""
        k = self.bin_first + np.arange(self.n_bins)
        out = self.frames_of(pos.q)[:, None] & (k >= self.ac_bins)[None, :]
        return {"out": out[None], "peak": self.frames_of(pos.q)[None]}

    def zero_terms(self, pos):
        """q is the frame's sample 0, and the periodic Hann starts with w[0] = 0 exactly"""
        s = self.FIRST + self.hop * np.arange(self.n_frames)
        return {"out": ((s == pos.q)[:, None] & self.reads(pos)["out"][0])[None]}

    def may(self, pos):
        return {"out": np.zeros((1, self.n_frames, self.n_bins), bool), "peak": np.zeros((1, self.n_frames), bool)}


def spec_cases():
    m = {"must"}
    # hop 100: three frames share a sample; frame 5 starts at 450.  Every sample of the row lies in a frame.
    dense = [Pos("row 0", 0, 0, None, m), Pos("shared", 0, 500, None, m), Pos("frame 5 first", 0, 450, None, m),
             Pos("frame 5 first-1", 0, 449, None, m), Pos("frame 5 last", 0, 749, None, m), Pos("frame 5 last+1", 0, 750, None, m),
             Pos("row last", 0, 999, None, m)]
    # hop 400: frames [-50, 250), [350, 650), [750, 1050), gaps between them
    sparse = [Pos("row 0", 0, 0, None, m), Pos("frame 0 last", 0, 249, None, m), Pos("gap first", 0, 250, None, set()),
              Pos("gap last", 0, 349, None, set()), Pos("frame 1 first", 0, 350, None, m), Pos("frame 1 second", 0, 351, None, m),
              Pos("frame 1 last", 0, 649, None, m), Pos("gap 2", 0, 650, None, set()), Pos("row last", 0, 999, None, m)]
    return [SpecCase("hop100-all", 100, 0, 0, None, dense, 41), SpecCase("hop100-ac-sub", 100, 27, 100, 100, dense, 42),
            SpecCase("hop400-ac-all", 400, 27, 0, None, sparse, 43), SpecCase("hop400-sub", 400, 0, 100, 100, sparse, 44)]


# ---------------------------------------------------------------------------------------------------------- rate

class RateCase:
    """uc_rate_convert of one row of 400 samples (in_first = out_first = 0) to all its outputs.  What a copy writes:
    out [1, n_out].  On the GPU the copies are the rows of one call, so a poisoned row shares its block of 16 rows, its
    LDS window and (as one half of a packed pair) its multiply-adds with clean ones."""
    N_IN, HALF = 400, 24

    def __init__(self, name, up, down, seed):
        self.lib, self.name = "rate", "rate-%s" % name
        self.up, self.down = up, down
        self.info = rate.plan(up, down, self.HALF)                                   # uc_rate_plan
        self.T = int(self.info.taps)
        self.n_out = rate.count(self.info, self.N_IN)                                # uc_rate_count
        steps = [rate.step(self.info, m) for m in range(self.n_out)]                 # uc_rate_step
        self.k = np.array([k for k, _ in steps], np.int64)
        self.p = np.array([p for _, p in steps], np.int64)
        self.rows = rows_f32(seed, 1, self.N_IN)
        self.mid = self.n_out // 2
        k, T, m = int(self.k[self.mid]), self.T, {"must"}
        assert 0 < k - T and k + 1 < self.N_IN - 1
        # (every sample of the row is under a tap of some output: no position lies outside every zone)
        self.positions = [Pos("k-T", 0, k - T, None, m), Pos("k-T+1", 0, k - T + 1, None, m), Pos("k", 0, k, None, m),
                          Pos("k+1", 0, k + 1, None, m), Pos("row 0", 0, 0, None, m), Pos("row last", 0, self.N_IN - 1, None, m)]

    def model(self, rows):
        return {"out": rate.model(rows, self.up, self.down, self.HALF)}

    def reads(self, pos):
        """output m is the chain over x[k - j], j = T - 1 .. 0: k - T + 1 <= q <= k, zero coefficients included"""
        return {"out": ((self.k - self.T + 1 <= pos.q) & (pos.q <= self.k))[None]}

    def zero_terms(self, pos):
        """prototype index i = p + j up of the tap over x[q]: the taps behind the prototype's end, i >= N_h, which the table
        holds as zeros, and the zeros of the sinc, i - c a multiple of q = max(up, down) other than 0 (integer phases; the
        float64 prototype holds about 1e-17 there, which no float64 sum shows)"""
        i = self.p + (self.k - pos.q) * int(self.info.up)
        big = max(int(self.info.up), int(self.info.down))
        zero = (i >= 2 * self.HALF * big + 1) | (((i - int(self.info.centre)) % big == 0) & (i != int(self.info.centre)))
        return {"out": (self.reads(pos)["out"][0] & zero)[None]}

    def may(self, pos):
        return {"out": np.zeros((1, self.n_out), bool)}


def rate_cases():
    return [RateCase("3125-1764", 3125, 1764, 51), RateCase("5-13", 5, 13, 52)]


# --------------------------------------------------------------------------------------------------------- array

class ArrayCase:
    """uc_array_combine of 3 microphones x 600 samples (in_first 0) into the outputs 40 .. 439 of three beams: one tap with
    an integer delay, one tap with a fractional delay, three taps.  What a copy writes: out [3, 400]."""
    N_IN, OUT_FIRST, N_OUT, J = 600, 40, 400, 240              # J: the output whose support the positions walk round
    BEAMS = (((0, 1.0, 3.0),), ((1, 0.7, 2.37),), ((0, 0.3, 1.5), (1, 0.3, -2.25), (2, 0.4, 4.0)))   # (mic, weight, delay)

    def __init__(self, seed):
        self.lib, self.name = "array", "array-3x600"
        self.rows = rows_f32(seed, 3, self.N_IN)
        # uc_array_tap_coefficients: (c [16], shift) of every tap
        self.coef = [[array.coefficients(d, w) for (_, w, d) in taps] for taps in self.BEAMS]
        m = {"must"}
        s1 = self.coef[1][0][1]                                 # the fractional tap of microphone 1
        s2 = self.coef[2][2][1]                                 # the integer tap of microphone 2 in the 3-tap beam
        s0 = self.coef[0][0][1]                                 # the integer tap of microphone 0
        J = self.J
        self.positions = [
            Pos("frac support-1", 1, J + s1 - 1, None, m), Pos("frac support 0", 1, J + s1, None, m),
            Pos("frac support 15", 1, J + s1 + 15, None, m), Pos("frac support 16", 1, J + s1 + 16, None, m),
            Pos("int support 0", 2, J + s2, None, m), Pos("int support 15", 2, J + s2 + 15, None, m),
            Pos("int centre", 0, J + s0 + 7, None, m),
            Pos("first output support 0", 2, self.OUT_FIRST + s2, None, m),
            Pos("before first output", 2, self.OUT_FIRST + s2 - 1, None, set()),
            Pos("last output support 15", 2, self.OUT_FIRST + self.N_OUT - 1 + s2 + 15, None, m),
            Pos("behind last output", 2, self.OUT_FIRST + self.N_OUT + s2 + 15, None, set()),
            Pos("row 0", 1, 0, None, set()), Pos("row last", 1, self.N_IN - 1, None, set())]   # supports wholly outside the call

    def model(self, rows):
        return {"out": array.model(rows, [list(b) for b in self.BEAMS], out_first=self.OUT_FIRST, n_out=self.N_OUT,
                                   coef=array.coefficients)}

    def _support(self, pos, zero):
        j = self.OUT_FIRST + np.arange(self.N_OUT)
        out = np.zeros((len(self.BEAMS), self.N_OUT), bool)
        nonzero = np.zeros_like(out)
        for b, taps in enumerate(self.BEAMS):
            for (mic, _, _), (c, shift) in zip(taps, self.coef[b]):
                if mic == pos.row:
                    t = pos.q - j - shift                       # the coefficient over x[q] for output j
                    inside = (t >= 0) & (t < 16)
                    out[b] |= inside
                    nonzero[b] |= inside & (c[np.clip(t, 0, 15)] != 0)
        return out & ~nonzero if zero else out

    def reads(self, pos):
        """output j of a beam has the term c_k[t] x_k[j + shift_k + t], t = 0 .. 15, for each of its taps: zeros included"""
        return {"out": self._support(pos, False)}

    def zero_terms(self, pos):
        """an integer delay: c[7] alone is not zero"""
        return {"out": self._support(pos, True)}

    def may(self, pos):
        return {"out": np.zeros((len(self.BEAMS), self.N_OUT), bool)}


def array_cases():
    return [ArrayCase(61)]


# -------------------------------------------------------------------------------------------------------- retime

class RetimeCase:
    """uc_retime_rows of the array case's rows into the outputs 40 .. 439 of four lines: slope 0 with an integer delay,
    slopes +2^-9 and -2^-9, slope 0 with a fraction.  What a copy writes: out [4, 400]."""
    N_IN, OUT_FIRST, N_OUT, J = 600, 40, 400, 240
    LINES = ((0, 3.0, 0.0), (1, 1.25, 2.0 ** -9), (2, 2.0, -2.0 ** -9), (1, 2.37, 0.0))          # (mic, delay, slope)

    def __init__(self, seed):
        self.lib, self.name = "retime", "retime-3x600"
        self.rows = rows_f32(seed, 3, self.N_IN)
        # the retimer's own step: uc_retime_fixed, then the integer side of the definition
        self.steps = [retime.positions(d, s, self.OUT_FIRST, self.N_OUT, fix=retime.fixed) for (_, d, s) in self.LINES]
        m, j = {"must"}, self.J - self.OUT_FIRST
        I1, I2, I0 = int(self.steps[1][0][j]), self.steps[2][0], int(self.steps[0][0][j])
        self.positions = [
            Pos("support-1", 1, I1 - 8, None, m), Pos("support 0", 1, I1 - 7, None, m), Pos("support 15", 1, I1 + 8, None, m),
            Pos("support 16", 1, I1 + 9, None, m), Pos("int centre", 0, I0, None, m),
            Pos("first output support 0", 2, int(I2[0]) - 7, None, m), Pos("before first output", 2, int(I2[0]) - 8, None, set()),
            Pos("last output support 15", 2, int(I2[-1]) + 8, None, m), Pos("behind last output", 2, int(I2[-1]) + 9, None, set()),
            Pos("row 0", 1, 0, None, set()), Pos("row last", 1, self.N_IN - 1, None, set())]

    def model(self, rows):
        return {"out": retime.model(rows, [tuple(l) for l in self.LINES], out_first=self.OUT_FIRST, n_out=self.N_OUT,
                                    table=retime.table)}

    def _support(self, pos, zero):
        out = np.zeros((len(self.LINES), self.N_OUT), bool)
        for r, ((mic, _, _), (I, q, mu)) in enumerate(zip(self.LINES, self.steps)):
            if mic == pos.row:
                t = pos.q - (I - 7)
                inside = (t >= 0) & (t < 16)
                # c[t] = fmaf(mu, D[q][t], T[q][t]) is zero only on a whole sample (q = 0, mu = 0), and there for t != 7
                out[r] = inside & (q == 0) & (mu == 0) & (t != 7) if zero else inside
        return out

    def reads(self, pos):
        """output j of a line reads x[I - 7 + t], t = 0 .. 15, of its microphone: zero coefficients included"""
        return {"out": self._support(pos, False)}

    def zero_terms(self, pos):
        return {"out": self._support(pos, True)}

    def may(self, pos):
        return {"out": np.zeros((len(self.LINES), self.N_OUT), bool)}


def retime_cases():
    return [RetimeCase(61)]


# --------------------------------------------------------------------------------------------------------- track

class TrackCase:
    """uc_track_windows over the correlators' two rows and pairs: four windows of 2048 reference samples out to 512 lags.
    By definition a window is uc_xcorr_correlate at first + w hop, so the zones of a window are those of the xcorr case
    with that range.  What a copy writes: corr [2, 4, 1025] and one crest record per (pair, window)."""
    PAIRS = CorrCase.PAIRS
    FIRST, WINDOW, N_WINDOWS, L = 600, 2048, 4, 512

    def __init__(self, name, n_in, hop, positions, seed):
        self.lib, self.name = "track", "track-%s" % name
        self.n_in, self.hop = n_in, hop
        self.rows = rows_f32(seed, 2, n_in)
        self.win = [CorrCase("xcorr", "w%d" % w, n_in, self.FIRST + w * hop, self.WINDOW, self.L, [], seed) for w in range(self.N_WINDOWS)]
        self.positions = positions

    def model(self, rows):
        return {"corr": track.windows_model(rows, list(self.PAIRS), self.FIRST, self.WINDOW, self.hop, self.N_WINDOWS, self.L)}

    def _stack(self, what, pos):
        corr = np.stack([getattr(w, what)(pos)["corr"] for w in self.win], axis=1)
        return {"corr": corr, "crest": corr.any(axis=2)}

    def reads(self, pos):
        return self._stack("reads", pos)

    def zero_terms(self, pos):
        return self._stack("zero_terms", pos)

    def may(self, pos):
        """the other lags of a (pair, window) with a MUST lag; its crest record is MUST already"""
        out = self._stack("may", pos)
        out["crest"][:] = False
        return out


def track_cases():
    m, both = {"must"}, {"must", "may"}
    f, n, L = TrackCase.FIRST, TrackCase.WINDOW, TrackCase.L

    def edges(hop, ref_out):
        """the edges of window 1; with overlapping windows its neighbours hold what lies just outside it"""
        f1 = f + hop
        return [Pos("ref first-1", 0, f1 - 1, None, ref_out), Pos("ref first", 0, f1, None, m),
                Pos("ref first+n-1", 0, f1 + n - 1, None, m), Pos("ref first+n", 0, f1 + n, None, ref_out),
                # (a microphone sample at an edge of window 1 is in the reach of a neighbour too, in part of its lags)
                Pos("mic first-L-1", 1, f1 - L - 1, None, both), Pos("mic first-L", 1, f1 - L, None, both),
                Pos("mic first+n+L-1", 1, f1 + n + L - 1, None, both), Pos("mic first+n+L", 1, f1 + n + L, None, both),
                Pos("mic before window 0", 1, f - L - 1, None, set()), Pos("mic window 0 first", 1, f - L, None, both)]
    return [TrackCase("hop1024", 6000, 1024, edges(1024, m) + [Pos("mic row last", 1, 5999, None, both)], 71),
            TrackCase("hop3000", 12000, 3000, edges(3000, set()) + [Pos("mic row last", 1, 11999, None, both)], 72)]


# --------------------------------------------------------------------------------------------------------- wcorr

class WcorrCase:
    """uc_wcorr_windows over the correlators' two rows and pairs: four windows of 2048 reference samples, max_lag 448 and
    guard 64, so the segments are cut for L' = 512.  The header's definition is total: a stored lag is the circular
    convolution of every segment's whole 2048-point correlation with the weights' impulse response h, so every sample of
    a segment -- the reference's [first', first' + n'), the microphone's [first' - L', first' + n' + L') -- has a term in
    every stored lag of its (pair, window), whatever the weights.  What a copy writes: corr [2, 4, 897].
    weights: "ones" (h is the unit impulse: the terms outside uc_xcorr_correlate's reach at L' have the coefficient 0),
    "band" (16 .. 19 kHz with 1 kHz edges at 78 125 Hz: bins of weight 0, 1 and between) and "zero" (every coefficient 0)."""
    PAIRS = CorrCase.PAIRS
    FIRST, WINDOW, N_WINDOWS, L, GUARD = 600, 2048, 4, 448, 64

    def __init__(self, kind, name, n_in, hop, positions, seed):
        self.lib, self.name, self.kind = "wcorr", "wcorr-%s-%s" % (kind, name), kind
        self.n_in, self.hop = n_in, hop
        self.rows = rows_f32(seed, 2, n_in)
        self.weights = {"ones": None, "zero": np.zeros(wcorr.BINS, np.float32),
                        "band": wcorr.band_weights(78125.0, 16000.0, 19000.0, 1000.0, self.GUARD)[0]}[kind]   # uc_wcorr_band_weights
        Lp = self.L + self.GUARD
        self.win = [CorrCase("xcorr", "w%d" % w, n_in, self.FIRST + w * hop, self.WINDOW, Lp, [], seed) for w in range(self.N_WINDOWS)]
        self.positions = positions

    def model(self, rows):
        if self.kind == "ones":
            # the header's bit contract: with weights of ones the central 2 L + 1 values of uc_xcorr_correlate at L + guard
            # (the plain sums: a float64 transform would blur which terms a lag has)
            full = track.windows_model(rows, list(self.PAIRS), self.FIRST, self.WINDOW, self.hop, self.N_WINDOWS, self.L + self.GUARD)
            return {"corr": full[:, :, self.GUARD:self.GUARD + 2 * self.L + 1]}
        return {"corr": wcorr.windows_model(rows, list(self.PAIRS), self.FIRST, self.WINDOW, self.hop, self.N_WINDOWS, self.L,
                                            self.GUARD, self.weights)}

    def _xcorr_reach(self, pos):
        """uc_xcorr_correlate's reach at L', its central 2 L + 1 lags: [pairs, windows, 2 L + 1]"""
        full = np.stack([w.reads(pos)["corr"] for w in self.win], axis=1)
        return full[:, :, self.GUARD:self.GUARD + 2 * self.L + 1]

    def reads(self, pos):
        """every stored lag of a (pair, window) one of whose segments holds q"""
        touched = np.stack([w.reads(pos)["corr"].any(axis=1) for w in self.win], axis=1)       # at L': guard lags included
        return {"corr": np.repeat(touched[:, :, None], 2 * self.L + 1, axis=2)}

    def zero_terms(self, pos):
        """ones: h[u] = 0 for u != 0, so what uc_xcorr_correlate at L' does not reach; zero: everything; band: nothing"""
        must = self.reads(pos)["corr"]
        if self.kind == "band":
            return {"corr": np.zeros_like(must)}
        if self.kind == "zero":
            return {"corr": must}
        zero_xcorr = np.stack([w.zero_terms(pos)["corr"] for w in self.win], axis=1)[:, :, self.GUARD:self.GUARD + 2 * self.L + 1]
        return {"corr": must & (~self._xcorr_reach(pos) | zero_xcorr)}

    def may(self, pos):
        return {"corr": np.zeros((len(self.PAIRS), self.N_WINDOWS, 2 * self.L + 1), bool)}


def wcorr_cases():
    m = {"must"}
    f, n, Lp = WcorrCase.FIRST, WcorrCase.WINDOW, WcorrCase.L + WcorrCase.GUARD

    def edges(hop, n_in, ref_out):
        """the edges of window 1, the guard included: the microphone's [first' - L - guard, first' + n' + L + guard)"""
        f1 = f + hop
        return [Pos("ref first-1", 0, f1 - 1, None, ref_out), Pos("ref first", 0, f1, None, m),
                Pos("ref first+n-1", 0, f1 + n - 1, None, m), Pos("ref first+n", 0, f1 + n, None, ref_out),
                Pos("mic first-L-g-1", 1, f1 - Lp - 1, None, m), Pos("mic first-L-g", 1, f1 - Lp, None, m),
                Pos("mic first+n+L+g-1", 1, f1 + n + Lp - 1, None, m), Pos("mic first+n+L+g", 1, f1 + n + Lp, None, m),
                Pos("mic before window 0", 1, f - Lp - 1, None, set()), Pos("mic window 0 first", 1, f - Lp, None, m),
                Pos("mic in the guard alone", 1, f - WcorrCase.L - 1, None, m), Pos("mic row last", 1, n_in - 1, None, m)]
    return [WcorrCase("ones", "hop1024", 6000, 1024, edges(1024, 6000, m), 81),
            WcorrCase("band", "hop1024", 6000, 1024, edges(1024, 6000, m), 82),
            WcorrCase("band", "hop3000", 12000, 3000, edges(3000, 12000, set()), 83),
            WcorrCase("zero", "hop3000", 12000, 3000, edges(3000, 12000, set()), 84)]


def all_cases():
    return (corr_cases() + mf_cases() + spec_cases() + rate_cases() + array_cases() + retime_cases() + track_cases() +
            wcorr_cases())


LIBRARIES = ("xcorr", "align", "mf", "spec", "rate", "array", "retime", "track", "wcorr")
HAVE_MAY = ("xcorr", "align", "mf", "track")          # spec has no MAY zone (a frame has a transform of its own), nor has rate; wcorr's definition is total
