"""What tests/test_mic_cpu.py and tests/test_gpu_mic.py share: the nine 2048-sample inputs of the bound and quality tests, and
the transmissions of the end-to-end tests (rendered as tests/test_dfsdm.py::_pdm_transmissions renders them, but at
78 125 Hz, in front of the microphone instead of behind it).  Everything is a function of the seeds below; nothing here needs
a GPU."""
import numpy as np

N = 2048
FS = 78125.0
Q_MAX = 2 ** 23 - 1
BLOCKS = 112
STREAMS = 6                                     # per variant
# seeds of the transmissions by receiver variant, and the streams that decode through the model alone (uco.RX_REAL = 0: every
# one; uco.SYNC_CPLX = 1: all but one, a bit slip at acquisition, the firmware's own): tests/test_mic_cpu.py asserts exactly
# these counts on the oracle, tests/test_gpu_mic.py on the GPU
SEEDS = {0: 7, 1: 10}
DECODED = {0: 6, 1: 5}
PDM_SILENCE = 0xAAAAAAAA                        # UC_PDM_SILENCE: the sinc^5's history of a stream that starts


def nine_inputs():
    """{name: float64 [2048]} at full scale 2^23 - 1: a 16 -> 19 kHz chirp, the same at 0.1, a 1 kHz tone, uniform noise
    (default_rng(0)), DC+ and DC-, the alternating +-1, random +-1, zeros."""
    t = np.arange(N) / FS
    chirp = np.sin(2.0 * np.pi * (16000.0 * t + 0.5 * (3000.0 / (N / FS)) * t ** 2))
    rng = np.random.default_rng(0)
    a = float(Q_MAX)
    return {"chirp": a * chirp, "chirp at 0.1": 0.1 * a * chirp, "1 kHz tone": a * np.sin(2.0 * np.pi * 1000.0 * t),
            "uniform noise": a * rng.uniform(-1.0, 1.0, N), "DC+": np.full(N, a), "DC-": np.full(N, -a),
            "alternating": a * (1.0 - 2.0 * (np.arange(N) % 2)), "random +-1": a * (1.0 - 2.0 * rng.integers(0, 2, N)),
            "zeros": np.zeros(N)}


def transmissions(variant, count=STREAMS, blocks=BLOCKS):
    """`count` microphones: 0.01 noise, one transmission each of amplitude 0.35 behind a lead of 25 .. 40 blocks and a
    fraction of one, times 2^23 - 1 -> (float32 [count, blocks * 2048] in LSB of the 24-bit value, messages)."""
    from uchirp import tx
    rng = np.random.default_rng(SEEDS[variant])
    n = blocks * N
    x = np.zeros((count, n), np.float32)
    msgs = []
    for s in range(count):
        msg = "".join(chr(int(c)) for c in rng.integers(48, 123, size=int(rng.integers(2, 6))))
        tone = tx.render(msg, fs_rx=FS, amplitude=0.35)
        lead = int(rng.integers(25, 40)) * N + int(rng.integers(0, N))
        v = rng.standard_normal(n) * 0.01
        assert lead + tone.size <= n
        v[lead:lead + tone.size] += tone
        x[s] = (np.clip(v, -1.0, 1.0) * Q_MAX).astype(np.float32)
        msgs.append(msg)
    return x, msgs


def model_bits(x):
    """The model's PDM words of float rows at scale 1: uint32, row by row through the library's plain-C definition
    (uc_mic_modulate_row, which tests/test_mic_cpu.py proves equal to `model` bit for bit: the numpy loop would take a
    minute on these 229 376-sample rows)."""
    from uchirp import mic
    return np.stack([mic.modulate_row(mic.quantise_model(r))[0] for r in np.atleast_2d(x)])


def sinc5_behind_silence(words):
    """The oracle's DFSDM words of PDM rows behind four UC_PDM_SILENCE words each."""
    from oracle import uco
    h = np.full(4, PDM_SILENCE, np.uint32)
    return np.stack([uco.dfsdm_sinc5(np.concatenate([h, np.asarray(r, np.uint32)])) for r in np.atleast_2d(words)])
