"""What tests/test_ddc_cpu.py and tests/test_gpu_ddc.py share: the tap counts and decimations of the bit-for-bit tests, their tap
sets, input rows (noise with four rows replaced), starting states and carriers, the covering list of cases, the -0 case, and
the definition's answer to a row that holds one unit pulse.  Everything is a function of the seeds below; nothing here needs
a GPU."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAP_COUNTS = (1, 2, 27, 63, 64, 65, 128)
DECIMS = (1, 2, 3, 8, 64)
ROWS, SAMPLES = 130, 2049
IMPULSE_ROW, NAN_ROW, STILL_ROW, DENORMAL_STATE_ROW = 0, 1, 2, 3
FIRST = 2 ** 32 - 1000 - 1                   # not a multiple of 2, 3, 8 or 64; the phase's index wraps inside the row

# (n_taps, decim, format of the input, format of the output): every tap count, every decimation, every pair of formats
CASES = ((1, 1, "f32", "iq"), (2, 2, "i32", "i"), (27, 1, "i32", "iq"), (27, 8, "f32", "i"), (63, 3, "f32", "iq"), (64, 64, "i32", "iq"),
         (65, 2, "f32", "i"), (128, 1, "f32", "iq"), (128, 3, "i32", "i"), (128, 64, "f32", "i"), (27, 64, "i32", "i"), (2, 8, "i32", "iq"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.complex64 else a.view(np.float32).view(np.uint32)


def taps_of(n_taps):
    """float32 [n_taps]: noise of the size of a low-pass's taps, signs mixed."""
    return (np.random.default_rng(100 + n_taps).standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)


def inputs():
    """(float32 [130, 2049], int32 [130, 2049]): normal noise x 20 000, as floats and as DFSDM words (the rounded value << 8,
    low byte random), with three rows replaced.  Floats: an impulse of 1e-39 (a denormal: every output it reaches is one), a
    row with NaN and +-Inf in it, a row of zeros of both signs.  Words: an impulse of one LSB, a row with the extreme words in
    it, a row of low bytes alone (value 0)."""
    rng = np.random.default_rng(31)
    f = (rng.standard_normal((ROWS, SAMPLES)) * 20000.0).astype(np.float32)
    w = ((np.rint(f).astype(np.int64) << 8) | rng.integers(0, 256, size=f.shape)).astype(np.int32)
    f[IMPULSE_ROW] = 0.0
    f[IMPULSE_ROW, 700] = 1e-39
    f[NAN_ROW, [0, 5, 127, 128, 2048]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    f[STILL_ROW] = np.where(np.arange(SAMPLES) % 3 == 0, -0.0, 0.0)
    w[IMPULSE_ROW] = 0
    w[IMPULSE_ROW, 700] = 256
    w[NAN_ROW, [0, 5, 127, 128, 2048]] = [-2 ** 31, 2 ** 31 - 1, -1, -256, -257]
    w[STILL_ROW] = rng.integers(0, 256, size=SAMPLES)
    return f, w


def states():
    """float32 [130, 128] to start from: noise of the signal's size; zeros for the replaced rows, denormals in row 3."""
    rng = np.random.default_rng(32)
    st = (rng.standard_normal((ROWS, 128)) * 20000.0).astype(np.float32)
    st[[IMPULSE_ROW, NAN_ROW, STILL_ROW]] = 0.0
    st[DENORMAL_STATE_ROW] = (rng.standard_normal(128) * 1e-40).astype(np.float32)
    return st


def carriers():
    """(steps, phases) uint32 [130]: any step and phase; row 4 has the plain filter's (0, 0), row 5 the firmware's 17.5 kHz at
    78 125 Hz, row 6 its negative."""
    from uchirp import ddc
    rng = np.random.default_rng(33)
    steps = rng.integers(0, 2 ** 32, size=ROWS, dtype=np.uint64)
    phases = rng.integers(0, 2 ** 32, size=ROWS, dtype=np.uint64)
    steps[4], phases[4] = 0, 0
    steps[5], steps[6] = ddc.step_of(17500.0, 78125.0), ddc.step_of(-17500.0, 78125.0)
    return steps, phases


def minus_zero_case():
    """(taps [1], the same padded with a zero tap [2], x float32 [64]): samples of +1e-30 and -1e-30 in turn against the one
    tap 1e-30 and the carrier (1, 0).  The product -1e-60 rounds to -0, so I is -0 at every odd sample; behind it the padded
    set adds (+0) x (+1e-30) = +0 to that -0 and gives +0."""
    x = np.where(np.arange(64) % 2 == 1, -1e-30, 1e-30).astype(np.float32)
    return np.array([1e-30], np.float32), np.array([1e-30, 0.0], np.float32), x


def pulse_answer(taps, decim, n_rows, n_samples, steps, phases, first=0):
    """The definition's outputs (complex64 [n_rows, count]) where row q holds the one sample 1.0 at position q and zeros
    elsewhere, from rest: every chain starts from +0 and adds zeros of either sign, which leave +0, until tap k meets the
    pulse: acc = fmaf(h[k], m, +0), the product rounded once (never a zero here: no tap and no carrier value is one); the
    zeros behind it leave it as it is.  So output o of row q is fma32(h[k], m_q, 0) with k = lead + o D - q where that is a
    tap, +0 elsewhere.  The caller checks this restatement against `emulate32` on some rows."""
    from uchirp import ddc
    h = np.asarray(taps, np.float32)
    assert (h != 0).all()
    _, count, lead = ddc._span_of(first, n_samples, decim)
    q = np.arange(n_rows)
    ph = ((np.asarray(phases, np.uint64)[:n_rows] + np.asarray(steps, np.uint64)[:n_rows] * ((np.uint64(first) + q.astype(np.uint64)) & np.uint64(0xFFFFFFFF)))
          & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c, s = ddc.carrier32(ph)
    one = np.float32(1.0)
    mi, mq = one * c, one * s
    assert (mi != 0).all() and (mq != 0).all()
    out = np.zeros((n_rows, count), np.complex64)
    zero = np.zeros(n_rows, np.float32)
    for k in range(h.size):
        # the output whose tap k meets the pulse: lead + o D - q = k
        num = q + k - lead
        ok = (num >= 0) & (num % decim == 0) & (num // decim < count)
        o = num[ok] // decim
        out.real[q[ok], o] = ddc.fma32(h[k], mi[ok], zero[ok])
        out.imag[q[ok], o] = ddc.fma32(h[k], mq[ok], zero[ok])
    return out
