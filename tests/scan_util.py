"""What tests/test_scan_cpu.py and tests/test_gpu_scan.py share: the rows and steering sets of the bit-for-bit tests, and the
-12 dB experiment (16 line arrays of eight microphones, 181 candidate directions) whose inputs the CPU test proves on the
float64 models before a GPU sees them.  Everything is a function of the seeds below; nothing here needs a GPU."""
import numpy as np

# ---- the bit-for-bit tests: one array of 6 rows, 9300 samples from absolute sample 2^20 on
ARRAY_ROWS, N_IN, IN_FIRST = 6, 9300, 1 << 20
FIRST = IN_FIRST + 40                       # windows start here: inside the rows, and so is a tap 5000 samples on (4100 + 5000 + 40 + 8 < 9300)
TAP_COUNTS = (1, 2, 8, 32)
BEAM_COUNTS = (1, 3, 4, 5, 63, 64, 65)
N_BASE = 9                                  # the beams of the window sweeps
FAR = 5000.0                                # a delay that no staged image holds next to the small ones


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rows():
    """(float32 [6, 9300], int32 [6, 9300]): normal noise x 20 000 as floats, and as DFSDM words (the rounded value << 8, low
    byte random; cast whole, as the array combiner casts them)."""
    rng = np.random.default_rng(31)
    f = (rng.standard_normal((ARRAY_ROWS, N_IN)) * 20000.0).astype(np.float32)
    w = ((np.rint(f).astype(np.int64) << 8) | rng.integers(0, 256, size=f.shape)).astype(np.int32)
    return f, w


def steering(n_taps):
    """(mics [n_taps], weights float32 [n_taps], delays float64 [65, n_taps]).  Microphones repeat (k mod 6) where there are
    more taps than rows.  Beams 0 .. 8: integer delays; k + 255/256; negative; FAR on tap 0 beside small ones; random in
    [0, 16); random in [-8, 40); ties of the quantiser (odd multiples of 1/512); the far edge of the staged spread; random in
    [0, 64).  Beams 9 .. 64: random in [0, 16), but beam 40 has -3000 on its last tap."""
    rng = np.random.default_rng(32 + n_taps)
    k = np.arange(n_taps)
    mics = k % ARRAY_ROWS
    weights = ((1.0 + 0.1 * k) * np.where(k % 3 == 2, -1.0, 1.0) / n_taps).astype(np.float32)
    d = rng.uniform(0.0, 16.0, size=(65, n_taps))
    d[0] = (3 * k) % 17
    d[1] = k % 11 + 255.0 / 256.0
    d[2] = -(k % 5) - 0.5
    d[3] = k % 7 + 0.25
    d[3, 0] = FAR
    d[5] = rng.uniform(-8.0, 40.0, size=n_taps)
    d[6] = k % 9 + (2 * (k % 4) + 1) / 512.0
    d[7] = 60.0 + k % 4 + 0.75
    d[8] = rng.uniform(0.0, 64.0, size=n_taps)
    d[40, -1] = -3000.0
    return mics, weights, d


# ---- the -12 dB experiment
FS, SOUND = 78125.0, 343.0
N_ARRAYS, N_MICS, SPACING = 16, 8, 0.0098
N = 24 * 2048
W_FIRST, W_LEN = 2048, N - 4096
AMPLITUDE, LEAD = 2000.0, 300.0
SIGMA = AMPLITUDE * 10.0 ** (12.0 / 20.0)
CANDIDATES_DEG = np.arange(-90.0, 91.0)     # 181 directions one degree apart
CAP_DEG, CAP_SAMPLES = 3.0, 0.75


def mic_xyz():
    return np.stack([np.arange(N_MICS) * SPACING, np.zeros(N_MICS), np.zeros(N_MICS)], axis=1)


def units(deg):
    t = np.radians(np.asarray(deg, np.float64))
    return np.stack([np.sin(t), np.cos(t), np.zeros_like(t)], axis=1)


def experiment():
    """{true_deg [16], true_delays [16, 8], candidates [181, 8], scenes: per array the microphones of Scene.render /
    scene.model (seed 200 + a)}"""
    from uchirp import scan
    true_deg = np.random.default_rng(7).uniform(-45.0, 45.0, N_ARRAYS)
    true_delays = scan.direction_delays(mic_xyz(), units(true_deg), FS, SOUND)
    cand = scan.direction_delays(mic_xyz(), units(CANDIDATES_DEG), FS, SOUND)
    scenes = [[(SIGMA, [(0, AMPLITUDE, LEAD + float(d), 0.0)]) for d in true_delays[a]] for a in range(N_ARRAYS)]
    return {"true_deg": true_deg, "true_delays": true_delays, "candidates": cand, "scenes": scenes}


def judge(exp, beams):
    """(worst direction error in degrees, worst delay error in samples) of the chosen candidates `beams` [16]"""
    from uchirp import scan
    beams = np.asarray(beams, np.int64)
    deg = np.abs(CANDIDATES_DEG[beams] - exp["true_deg"]).max()
    q = scan.quantise_model(exp["candidates"])[beams] / 256.0
    return float(deg), float(np.abs(q - exp["true_delays"]).max())
