"""What tests/test_duc_cpu.py and tests/test_gpu_duc.py share: the (K, L) cases of the bit-for-bit tests with their formats and
channel counts, their prototypes, input rows (noise with three rows replaced), starting states and channel tables, the -0
case, and the definition's answer to a row that holds one unit pulse.  Everything is a function of the seeds below; nothing
here needs a GPU."""
import numpy as np

# (taps per phase K, interpolation L): one tap, the firmware's 27, the longest chain, the flagship interpolation, an L that
# divides neither 256 nor 2048, the largest L with the longest prototype (2048 taps), the largest L with the shortest
KL = ((1, 1), (27, 1), (128, 1), (27, 8), (5, 3), (32, 64), (1, 64))
# (K, L, format of the input, channels per output row, format of the output): every (K, L), both formats of either side,
# n_chan 1, 3 and 16
CASES = ((1, 1, "iq", 1, "f32"), (27, 1, "iq", 1, "i16"), (128, 1, "i", 1, "f32"), (27, 8, "iq", 3, "i16"), (5, 3, "iq", 3, "f32"),
         (32, 64, "i", 1, "i16"), (1, 64, "iq", 16, "f32"))
ROWS = (1, 2, 5, 67)                         # output rows
IN_ROWS = 70
IMPULSE_ROW, NAN_ROW, STILL_ROW, DENORMAL_STATE_ROW = 0, 1, 2, 3
SPAN = 2048


def span_in(L):
    """the input samples of one unit of the kernel's work: uc_duc_span(L) / L"""
    return SPAN // L


def max_samples(L):
    return max(sample_counts(L))


def sample_counts(L):
    s = span_in(L)
    return sorted({1, 127, 128, 129, s - 1, s, s + 1, 2 * s + 3} - {0})


def first_of(L):
    """not a multiple of anything; the phase's index (first L + o) wraps 2^32 inside the row"""
    return 2 ** 32 // L - 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.complex64 else a.view(np.float32).view(np.uint32)


def taps_of(K, L, seed=0):
    """float32 [K L]: noise of the size of an interpolator's taps (gain L), signs mixed, no zero among them."""
    h = (np.random.default_rng(200 + 1000 * seed + 7 * K + L).standard_normal(K * L) / np.sqrt(K)).astype(np.float32)
    assert (h != 0).all()
    return h


def inputs(fmt, n):
    """float32 [70, n words]: normal noise x 12 000 (loud enough for int16 sums to clip now and then) with three rows replaced: an impulse of 1e-39 (a denormal: every output it
    reaches is one), a row with NaN and +-Inf in it, a row of zeros of both signs."""
    w = 2 if fmt == "iq" else 1
    f = (np.random.default_rng(71 + w).standard_normal((IN_ROWS, n * w)) * 12000.0).astype(np.float32)
    f[IMPULSE_ROW] = 0.0
    f[IMPULSE_ROW, min(40, n - 1) * w] = 1e-39
    at = [i for i in (0, 5, 127, 128, n * w - 1) if i < n * w]
    f[NAN_ROW, at] = [np.nan, np.inf, -np.inf, np.nan, np.inf][:len(at)]
    f[STILL_ROW] = np.where(np.arange(n * w) % 3 == 0, -0.0, 0.0)
    return f


def states(fmt):
    """float32 [70, 128 words] to start from: noise of the signal's size; zeros for the replaced rows, denormals in row 3."""
    w = 2 if fmt == "iq" else 1
    rng = np.random.default_rng(72 + w)
    st = (rng.standard_normal((IN_ROWS, 128 * w)) * 12000.0).astype(np.float32)
    st[[IMPULSE_ROW, NAN_ROW, STILL_ROW]] = 0.0
    st[DENORMAL_STATE_ROW] = (rng.standard_normal(128 * w) * 1e-40).astype(np.float32)
    return st


def channels(n_rows, n_chan, n_sets=1, seed=0):
    """(row_map, set_index, steps, phases) uint32 [n_rows n_chan]: the first output rows read the replaced input rows; any step
    and phase, but channel 0 of row 4 has the plain filter's (0, 0) and channel 0 of row 3 the modem's 17.5 kHz at 78 125 Hz."""
    from uchirp import duc
    rng = np.random.default_rng(73 + seed + n_chan)
    slots = n_rows * n_chan
    row_map = rng.integers(0, IN_ROWS, size=slots, dtype=np.uint64)
    for r in range(min(n_rows, 4)):
        row_map[r * n_chan] = r
    steps = rng.integers(0, 2 ** 32, size=slots, dtype=np.uint64)
    phases = rng.integers(0, 2 ** 32, size=slots, dtype=np.uint64)
    if n_rows > 4:
        steps[4 * n_chan], phases[4 * n_chan] = 0, 0
    if n_rows > 3:
        steps[3 * n_chan] = duc.step_of(17500.0, 78125.0)
    set_index = rng.integers(0, n_sets, size=slots, dtype=np.uint64)
    return row_map.astype(np.uint32), set_index.astype(np.uint32), steps.astype(np.uint32), phases.astype(np.uint32)


def new_state(x, st0, n, fmt):
    """the definition's state behind n samples: the last 128 of the old state and the sanitised samples"""
    from uchirp import duc
    w = 2 if fmt == "iq" else 1
    return np.ascontiguousarray(np.concatenate([st0, duc.samples32(x[:, :n * w])], axis=1)[:, n * w:])


def minus_zero_case():
    """(taps [1], the same padded with a zero tap [2], x float32 [64]): samples of +1e-30 and -1e-30 in turn (I alone, L = 1)
    against the one tap 1e-30 and the carrier (1, 0).  The product -1e-60 rounds to -0, so the output is -0 at every odd
    sample; behind it the padded set adds (+0) x (+1e-30) = +0 to that -0 and gives +0."""
    x = np.where(np.arange(64) % 2 == 1, -1e-30, 1e-30).astype(np.float32)
    return np.array([1e-30], np.float32), np.array([1e-30, 0.0], np.float32), x


def pulse_answer(taps, L, n_rows, n_samples, steps, phases, first=0):
    """The definition's outputs (float32 [n_rows, n_samples L]) where input row q holds the one I, Q pair (1, 0.5) at position
    q and zeros elsewhere, from rest, one channel: a chain starts from +0 and adds zeros of either sign, which leave +0,
    until tap rho + k L meets the pulse: fmaf(h, 1, +0) = h and fmaf(h, 0.5, +0) = h / 2, both exact (no tap is zero or so
    small that its half is not a float); the zeros behind leave them.  So output (m, rho) of row q has ai = h[rho + (m - q) L]
    where m - q is a tap's k, +0 elsewhere, aq = ai / 2, and y = (ai c) + (aq s) at the output's phase.  The caller checks
    this restatement against `emulate32` on some rows."""
    from uchirp import duc
    h = np.asarray(taps, np.float32)
    K = h.size // L
    assert (h != 0).all() and (np.abs(h) > 1e-30).all()
    q = np.arange(n_rows)[:, None]
    o = np.arange(n_samples * L)[None, :]
    k = o // L - q
    ok = (k >= 0) & (k < K)
    ai = np.where(ok, h[np.clip(o % L + k * L, 0, h.size - 1)], np.float32(0.0)).astype(np.float32)
    aq = ai * np.float32(0.5)
    c, s = duc.carrier32(duc.phases32(first * L, n_samples * L, np.asarray(steps, np.uint64)[:n_rows], np.asarray(phases, np.uint64)[:n_rows]))
    return (ai * c) + (aq * s)
