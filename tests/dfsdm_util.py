"""What tests/test_dfsdm_filter_cpu.py and tests/test_gpu_dfsdm_filter.py share: the configurations of the DFSDM filter
(include/uchirp_dfsdm.h) that are tested, and the bit patterns."""
import numpy as np

# (order, ratio, integrator, shift, offset): the receiver's own, the SINC3 of eight firmware projects with and without its
# shift, FastSinc short and at the largest ratio, ratios that do not divide 32 (7, 20, 5, 73), one output per bit, a ratio
# above 32 with an integrator, an integrator of 256, and the largest ratios of Sinc3, Sinc4 and Sinc5 under the 32-bit limit
CONFIGS = [(5, 32, 1, 2, 0), (3, 32, 1, 2, 0), (3, 32, 1, 0, 0), (0, 16, 1, 0, 5), (0, 1024, 1, 8, 0), (1, 7, 3, 0, -3), (1, 1, 1, 0, 0),
           (2, 64, 2, 0, 0), (3, 20, 1, 0, 0), (3, 5, 256, 0, 0), (3, 1024, 1, 8, 0), (4, 215, 1, 8, 0), (5, 73, 1, 8, 100)]
# the word path crossing an integrator boundary that is not every word (the GPU tests add it)
WORD_PATH_INTEGRATOR = (3, 64, 3, 0, 0)

CUTS = (1, 16, 17, 33)          # 67 words
N_WORDS = sum(CUTS)
SILENCE = 0x99999999            # uc_mic_modulate's word of a silent microphone


def stages(cfg):
    return 2 if cfg[0] == 0 else cfg[0]


def patterns(n, seed=0):
    """The patterns of tests/test_dfsdm.py::patterns, restated, and the silent microphone's word."""
    rng = np.random.default_rng(seed)
    yield "random", rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    yield "ones", np.full(n, 0xFFFFFFFF, np.uint32)
    yield "zeros", np.zeros(n, np.uint32)
    yield "alternating", np.full(n, 0xAAAAAAAA, np.uint32)
    step = np.zeros(n, np.uint32)
    step[n // 2:] = 0xFFFFFFFF
    yield "step", step
    sparse = np.zeros(n, np.uint32)
    sparse[::7] = 1 << (np.arange(sparse[::7].size) % 32).astype(np.uint32)
    yield "single bits", sparse
    yield "0x99999999", np.full(n, SILENCE, np.uint32)


def pattern(name, n, seed=0):
    return dict(patterns(n, seed))[name]


def random_state(rng, rows=None):
    """Any int32 in the 13 words the filter may read; the reserved three as the library leaves them."""
    st = rng.integers(-2 ** 31, 2 ** 31, size=(rows or 1, 16)).astype(np.int32)
    st[:, 13:] = 0
    return st if rows else st[0]
