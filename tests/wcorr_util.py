"""Inputs that tests/test_wcorr_cpu.py and tests/test_gpu_wcorr.py share: made on the host with the float64 models
(`uchirp.link.model`), seeded, made once per process and never written.  The CPU file measures on them what the GPU file
then relies on (the error constant's yardstick, the runner-up of the delay test's pairs)."""
import functools

import numpy as np

N = 2048
FS = 78125.0
NM = 4
NS = 3 * 2048 + 37                     # the smallest rows at which a full group and one more sample fit at L' >= 253
PAIRS = [(0, 1), (2, 2), (3, 0), (1, 0), (3, 3), (2, 1)]
LAG_GUARD = ((1, 0), (1, 511), (64, 0), (64, 128), (65, 63), (200, 56), (384, 128), (512, 0))
BAND = (16000.0, 19000.0, 1000.0)      # f_lo, f_hi, taper_hz: the chirps' band with cos^2 edges
ONE_HOT_BINS = (0, 1, 127, 128, 1023, 1024)
TEXT = "Hello, World"
AMP = 2000.0

# the delay pairs: one text, two leads, a window of 8192 samples well inside the message
DELAY_WINDOW, DELAY_L, DELAY_GUARD, DELAY_FIRST = 8192, 64, 128, 256
DELAY_NS = DELAY_WINDOW + 2 * DELAY_FIRST


@functools.lru_cache(maxsize=None)
def mics():
    """{"f32": 4 rows x NS float32: the message at amplitude 2000 at a lead of its own per row, plus noise of sigma 300;
    "i32": int32 words most of which are no floats (word 0 of every row is 0)}"""
    from uchirp import link
    rng = np.random.default_rng(26)
    lead = rng.uniform(0.0, 600.0, size=NM)
    x = link.model([TEXT] * NM, [float(v) for v in lead], AMP, 300.0, n_samples=NS, first_sample=30000, seed=8).astype(np.float32)
    assert np.abs(x).max() > AMP
    words = rng.integers(-2 ** 27, 2 ** 27, size=(NM, NS)).astype(np.int32)
    words[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    x.setflags(write=False)
    words.setflags(write=False)
    return {"f32": x, "i32": words}


@functools.lru_cache(maxsize=None)
def weight_tables():
    """[(name, BINS float32)]: the band, pseudo-random weights of either sign, and a one-hot table per bin of ONE_HOT_BINS"""
    from uchirp import wcorr
    rng = np.random.default_rng(77)
    out = [("band", wcorr.band_weights(FS, *BAND, guard=128)[0]), ("random", rng.uniform(-2.0, 2.0, wcorr.BINS).astype(np.float32))]
    for k in ONE_HOT_BINS:
        w = np.zeros(wcorr.BINS, np.float32)
        w[k] = 1.5
        out.append(("one-hot %d" % k, w))
    for _, w in out:
        w.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def impulses():
    """(rows, places): NM rows x NS with ONE non-zero sample each; places[m] = (index, value)"""
    places = [(1500, 3.0), (1463, -2.5), (2048 + 700, 1024.0), (2048 + 850, 0.75)]
    x = np.zeros((NM, NS), np.float32)
    for m, (i, v) in enumerate(places):
        x[m, i] = v
    x.setflags(write=False)
    return x, places


@functools.lru_cache(maxsize=None)
def delay_pairs(n_pairs, snr_db, seed0=0):
    """(x [2 n_pairs, DELAY_NS] float32, pairs, truth): pair i is rows (2 i, 2 i + 1), two receptions of one text whose
    leads differ by truth[i], uniform in +-40 samples, with noise of their own at `snr_db` (sigma = amplitude /
    10^(snr_db / 20)); the window [DELAY_FIRST, DELAY_FIRST + DELAY_WINDOW) lies inside the message's random bits"""
    from uchirp import link
    rng = np.random.default_rng(2024)
    sigma = AMP / 10.0 ** (snr_db / 20.0)
    rows, truth = [], []
    for i in range(n_pairs):
        d = float(rng.uniform(-40.0, 40.0))
        rows.append(link.model([TEXT] * 2, [100.0, 100.0 + d], AMP, sigma, n_samples=DELAY_NS, first_sample=20000 + 900 * i, seed=seed0 + i))
        truth.append(d)
    x = np.concatenate(rows).astype(np.float32)
    x.setflags(write=False)
    return x, [(2 * i, 2 * i + 1) for i in range(n_pairs)], truth


def band():
    from uchirp import wcorr
    return wcorr.band_weights(FS, *BAND, guard=DELAY_GUARD)[0]


def cases(Lp, ns=NS):
    """(first, window_len, hop, n_windows): every window_len of {1, S - 1, S, S + 1, 2048, 4 S, 4 S + 1} (S = 2048 - 2 L')
    that fits, with every hop of {1, window_len - 3, window_len, window_len + 5} and every count of {1, 2, 3, 7} windows that
    fit, `first` taking 0, an odd value and the value at which the last window ends at n_in in turn"""
    S = 2048 - 2 * Lp
    out, turn = [], 0
    for wl in (1, S - 1, S, S + 1, 2048, 4 * S, 4 * S + 1):
        if wl > ns:
            continue
        for hop in (1, wl - 3, wl, wl + 5):
            if hop < 1:
                continue
            for nw in (1, 2, 3, 7):
                span = (nw - 1) * hop + wl
                if span > ns:
                    continue
                room = ns - span
                first = (0, min(room, 701) | 1 if room else 0, room)[turn % 3]
                if first > room:
                    first = room
                turn += 1
                out.append((first, wl, hop, nw))
    return out


def error_ratio(got, want, E, wmax):
    """the worst |got - want| / (2^-24 wmax E) over the rows with E > 0; rows with E = 0 must be 0"""
    E = np.asarray(E, np.float64)
    zero = E == 0
    assert (got[zero] == 0).all()
    if zero.all() or wmax == 0:
        assert wmax != 0 or (got == 0).all()
        return 0.0
    return float((np.abs(got - want)[~zero] / (2.0 ** -24 * wmax * E[~zero, None])).max())
