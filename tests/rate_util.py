"""What tests/test_rate_cpu.py and tests/test_gpu_rate.py share: the 15 sound-card recordings of the end-to-end tests (the
transmitter's own int16 waveform at 44.1, 48 and 96 kHz, five texts each) and the noise they are laid into once they are at
the receivers' 78 125 Hz.  Everything is a function of SEED; nothing here needs a GPU or the library."""
import numpy as np

N = 2048
FS_OUT = 78125
RATES = (44100, 48000, 96000)
SEED = 5
GAIN = 0.1                  # a transmitter of amplitude 2000 * sqrt 2 at the microphone
SIGMA = 5.0
LEAD_BLOCKS = TAIL_BLOCKS = 30


def texts():
    """five texts of 6 .. 16 printable characters per rate: {fs: [str]}"""
    rng = np.random.default_rng(SEED)
    return {fs: ["".join(chr(int(c)) for c in rng.integers(33, 127, size=int(rng.integers(6, 17)))) for _ in range(5)] for fs in RATES}


def pcm(text, fs):
    """what a sound card running at fs would play: the transmitter's waveform as int16 (uchirp.tx)"""
    from uchirp import tx
    return tx.tone(text, fs).astype(np.int16)


def skews():
    """where each of the 15 transmissions starts behind its 30 blocks of noise: {fs: [int]}, 0 .. 2047 samples"""
    rng = np.random.default_rng(SEED + 1)
    return {fs: [int(s) for s in rng.integers(0, N, size=5)] for fs in RATES}


def in_noise(y, skew, index):
    """GAIN * y behind 30 blocks and `skew` samples of noise, noise on the signal, 30 blocks of noise behind it, cut to whole
    blocks: float32.  `index` (0 .. 14) picks the noise."""
    rng = np.random.default_rng([SEED, 100 + index])
    lead = LEAD_BLOCKS * N + int(skew)
    total = (lead + len(y) + TAIL_BLOCKS * N) // N * N
    x = SIGMA * rng.standard_normal(total)
    x[lead:lead + len(y)] += GAIN * np.asarray(y, np.float64)
    return x.astype(np.float32)
