"""What tests/test_iir_cpu.py and tests/test_gpu_iir.py share: the cascades of 1, 2, 7 and 8 sections, the input rows of the
bit-for-bit tests (noise with three rows replaced), their starting states, and the four mixed rows of the notebook's I/Q
demodulation (fixture K3) with the reference's own low-pass outputs.  Everything is a function of the seeds below and of the
committed fixtures; nothing here needs a GPU."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SECTION_COUNTS = (1, 2, 7, 8)
ROWS, SAMPLES = 130, 300
IMPULSE_ROW, MINUS_ZERO_ROW, NAN_ROW, DENORMAL_STATE_ROW = 0, 1, 2, 3


def cascades():
    """{section count: float64 [count, 5]}: a DC blocker, the 16-19 kHz band-pass of order 2, the reference's low-pass (order
    14) and the band-pass of order 8.  All stable, with unity gain in their pass bands."""
    from uchirp import iir
    out = {1: iir.dc_block_sections(78125.0, 200.0), 2: iir.bandpass_sections(78125.0, 16000.0, 19000.0, 2),
           7: iir.lpf_sections(44100.0, 3000.0), 8: iir.bandpass_sections(78125.0, 16000.0, 19000.0, 8)}
    assert all(v.shape == (k, 5) for k, v in out.items())
    return out


def inputs():
    """(float32 [130, 300], int32 [130, 300]): normal noise x 20 000, as floats and as DFSDM words (the rounded value << 8,
    low byte random), with three rows replaced.  Floats: an impulse of 1e-34 (its response runs through the denormals), a row
    that starts with -0.0, and a row with NaN and +-Inf in it.  Words: an impulse of one LSB, a row that starts with the
    low byte alone (value 0), and a row with the extreme words in it.  |x| <= 2^24 after the input rule."""
    rng = np.random.default_rng(21)
    f = (rng.standard_normal((ROWS, SAMPLES)) * 20000.0).astype(np.float32)
    w = ((np.rint(f).astype(np.int64) << 8) | rng.integers(0, 256, size=f.shape)).astype(np.int32)
    f[IMPULSE_ROW] = 0.0
    f[IMPULSE_ROW, 0] = 1e-34
    f[MINUS_ZERO_ROW, 0] = -0.0
    f[NAN_ROW, [0, 5, 17, 64, 299]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    w[IMPULSE_ROW] = 0
    w[IMPULSE_ROW, 0] = 256
    w[MINUS_ZERO_ROW, 0] = 255
    w[NAN_ROW, [0, 5, 17, 64, 299]] = [-2 ** 31, 2 ** 31 - 1, -1, -256, -257]
    return f, w


def states():
    """float32 [130, 16] to start from: noise of the signal's size; zeros for the three replaced rows, but -0.0 throughout
    the row that starts with -0.0 (so that -0.0 comes out of every section, and an identity section behind the last one
    would show), and denormals in row 3."""
    rng = np.random.default_rng(22)
    st = (rng.standard_normal((ROWS, 16)) * 1000.0).astype(np.float32)
    st[IMPULSE_ROW] = 0.0
    st[MINUS_ZERO_ROW] = -0.0
    st[NAN_ROW] = 0.0
    st[DENORMAL_STATE_ROW] = (rng.standard_normal(16) * 1e-40).astype(np.float32)
    return st


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def k3_rows():
    """The notebook's cells 16-22 up to the filter: k3_WW and k3_WWd times the cosine and the sine of the carrier on
    np.linspace(0, T, samples) -> (float64 [4, 1155], the reference's lpf() outputs [4, 1155], fs, cutoff)."""
    v = np.load(os.path.join(GOLD, "notebook_vectors_k3k5.npz"))
    p = json.load(open(os.path.join(GOLD, "known_answers.json")))["IQ_modulation_params"]
    t = np.linspace(0, p["T"], p["samples"])
    c, s = np.cos(2 * np.pi * p["CARRIER"] * t), np.sin(2 * np.pi * p["CARRIER"] * t)
    rows = np.stack([v["k3_WW"] * c, v["k3_WW"] * s, v["k3_WWd"] * c, v["k3_WWd"] * s])
    want = np.stack([v["k3_R"].real, v["k3_R"].imag, v["k3_Rd"].real, v["k3_Rd"].imag])
    return rows, want, float(p["Fs"]), float(p["CUTOFF"])
