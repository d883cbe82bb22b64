"""Inputs that the CPU and the GPU tests of the spectrum analyser share (tests/test_spec_cpu.py, tests/test_gpu_spec.py): the
K6 captures, and the rows the error constant of include/uchirp_spec.h is measured on.  Everything comes from a seed or
from tests/golden; nothing here needs a GPU."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 2048
K6_MISMATCHED = "chirp_experiment/48.1(kHz)_M2A"      # the one trio whose files belong to different captures
PRINT_STEP = 0.5e-6                                    # the device prints mag / sqrt(N) with six decimals
SCALE_K6 = 1.0 / np.sqrt(N)                            # main.c: magnitude / sqrt(N)

_k6 = None


def k6():
    """[(name, raw int32 [2048], freq [1024], fftmag [1024])], the 24 captures; fftmag is what the device printed."""
    global _k6
    if _k6 is None:
        z = np.load(os.path.join(GOLD, "k6_all.npz"))
        _k6 = [(str(name), z["raw_%02d" % i].astype(np.int32), z["fftfreq_%02d" % i], z["fftmag_%02d" % i])
               for i, name in enumerate(z["names"])]
    return _k6


def k6_words():
    return np.stack([c[1] for c in k6()])


def ac_bins_of(freq):
    """the bins below 1 kHz: the ones the firmware forces to 1.0"""
    return int(np.count_nonzero(freq < 1000.0))


def k6_verdict(got, mag_dev, freq, mag_tol):
    """tests/test_gpu_k6.py's criterion on every bin at or above 1 kHz, in the device's own units (magnitude / sqrt(N)):
    err <= MAG_TOL * (largest magnitude) + PRINT_STEP, and the same arg-max.  Returns (ok, err / largest magnitude)."""
    got = np.asarray(got, np.float64)[:1024]
    live = np.nonzero(freq >= 1000.0)[0]
    scale = got.max()                                  # (the DC region: the spectrum's own largest bin)
    err = np.abs(got[live] - mag_dev[live]).max()
    ok = err <= mag_tol * scale + PRINT_STEP and np.argmax(got[live]) == np.argmax(mag_dev[live])
    return bool(ok), float(err / scale)


def error_rows():
    """The rows the error constant is measured on and the GPU test holds the kernel to: {name: (x [rows, n_in], kwargs)}.
    noise: Gaussian at sigma 1000, whole frames and short overlapping ones; chirps: the modem's symbols at -10 dB; the K6
    words (int32, dominated by their DC region); and the same three as the other dtype."""
    from uchirp import synth
    rng = np.random.default_rng(18)
    noise = (1000.0 * rng.standard_normal((4, 3 * N))).astype(np.float32)
    chirps, _ = synth.make_frames(8, seed=18, snr_db=-10.0)
    chirps = chirps.reshape(2, 4 * N)
    words = k6_words()
    return {
        "noise f32": (noise, dict(hop=N)),
        "noise f32, 300-sample frames": (noise[:, :N], dict(frame_len=300, hop=177, first=-150)),
        "noise i32": (np.rint(noise * 64.0).astype(np.int32), dict(hop=1000)),
        "chirps at -10 dB f32": (chirps, dict(hop=N)),
        "chirps at -10 dB i32": (np.rint(chirps * 256.0).astype(np.int32), dict(hop=512, first=-1024)),
        "K6 words i32": (words, dict(hop=N, scale=SCALE_K6)),
        "K6 words f32": (words.astype(np.float32), dict(hop=N, scale=SCALE_K6)),
    }
