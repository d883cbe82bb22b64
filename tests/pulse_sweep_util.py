"""Pulse sweeps for the two kernels built on the full inverse transform of csrc/uc_xform.hpp -- compress_kernel
(csrc/uc_full_kernel.hip) and stream_kernel<DTYPE, D> (csrc/uc_stream_kernel.hip): inputs and oracle-side bookkeeping.

compress_kernel hands out ONE number and ONE index per frame, the signed maximum over 2048 outputs; stream_kernel one
peak record per overlap-save block, found over hop = 1537 / 1793 / 1921 offsets.  The parity tests leave it to random
numbers which output wins.  Here every output index of a frame (in either slot of a frame pair) and every offset of a
block is, in some frame or block, the CLEAR maximum, so that its own thread, slot t, last-pass twiddle and place in the
first-maximum search decide a record.

Nothing is derived from sign conventions or group delays: the float64 oracle says which output wins and whether it wins
clearly; the tests compare indices exactly on the clear ones and count what that reaches.

  tests/test_pulse_sweep_cpu.py    oracle only: the inputs do what the GPU test relies on
  tests/test_gpu_pulse_sweep.py    the kernels against that
"""
import functools

import numpy as np

from oracle import uco
from tone_sweep_util import PERM_SEED, permutation, to_dtype

N = 2048
AMP = 1000.0

# ------------------------------------------------------------------------------------------------ compress: frames

CLEAR = 0.99            # a frame is clear when the second-largest of its 2048 compressed outputs <= 0.99 x the largest:
#                         GPU and oracle are each within MAG_TOL = 2e-5 of it, a lead of 500 such bars
PHASES = 8              # carrier phases pi ph / 4 of the analytic up chirp
ZERO = -1               # in a layout: an all-zero frame


def analytic_up(o):
    """The analytic signal of the oracle's TABLE_UP: FFT, negative bins zeroed, positive ones doubled."""
    up = o.table(uco.TABLE_UP).astype(np.float64)
    f = np.fft.fft(up)
    f[N // 2 + 1:] = 0.0
    f[1:N // 2] *= 2.0
    return np.fft.ifft(f)


@functools.lru_cache(maxsize=None)
def compress_frames(dtype_name):
    """[PHASES * 2048, 2048]: frame ph * 2048 + s is 1000 Re(a e^{j pi ph / 4}) rolled by s (np.roll: sample i moves to
    i + s); the compressed pulse follows the roll and the phase moves the carrier crests under its envelope."""
    o = uco.Oracle(uco.COMPRESS)
    a = analytic_up(o)
    idx = (np.arange(N)[None, :] - np.arange(N)[:, None]) % N          # row s: np.roll(., s)
    out = np.empty((PHASES * N, N), np.dtype(dtype_name))
    for ph in range(PHASES):
        base = AMP * np.real(a * np.exp(1j * np.pi * ph / 4.0))
        out[ph * N:(ph + 1) * N] = to_dtype(base[idx], out.dtype.type)
    out.setflags(write=False)
    return out


class CompressAccount:
    """What the float64 oracle says about every frame of compress_frames(dtype): its record, the winning output index,
    second / first of the 2048 outputs and whether the frame is clear.  The oracle works frame by frame, so the account
    of a batch in another order, or with zero frames in it, is this one re-indexed (`layout`)."""

    def __init__(self, dtype_name):
        self.dtype_name = dtype_name
        self.frames = compress_frames(dtype_name)
        self.o = uco.Oracle(uco.COMPRESS, mag_mean=1.0)
        nf = len(self.frames)
        _, rec = self.o.process(self.frames)
        self.rec = rec[:, 0]
        self.win = np.zeros(nf, np.int64)
        self.ratio = np.zeros(nf)
        for f in range(nf):
            y = self.o.spectrum(self.frames[f])[0]
            i = int(np.argmax(y))                      # first maximum, as arm_max_f32
            self.win[f] = i
            self.ratio[f] = np.partition(y, -2)[-2] / y[i] if y[i] > 0 else np.inf
        self.clear = self.ratio <= CLEAR
        _, z = self.o.process(np.zeros((1, N), self.frames.dtype))
        self.zero_rec = z[0, 0]

    def spectrum(self, f):
        return self.o.spectrum(self.frames[f] if f != ZERO else np.zeros(N, self.frames.dtype))[0]

    def coverage(self):
        """Output indices that are the winner of at least one clear frame."""
        return set(int(k) for k in np.unique(self.win[self.clear]))

    def batch(self, order):
        """The frames of a layout as one array (ZERO: an all-zero frame)."""
        order = np.asarray(order)
        out = self.frames[np.maximum(order, 0)]
        out[order == ZERO] = 0
        return out

    def records(self, order):
        order = np.asarray(order)
        out = self.rec[np.maximum(order, 0)]
        out[order == ZERO] = self.zero_rec
        return out


@functools.lru_cache(maxsize=None)
def compress_account(dtype_name):
    return CompressAccount(dtype_name)


def layout(kind, n_frames=PHASES * N):
    """order[i]: the frame of compress_frames at place i of the batch (ZERO: an all-zero frame).
      base        as built: frame ph * 2048 + s rides in slot s & 1 of pair (ph * 2048 + s) >> 1
      zero_front  one all-zero frame in front: every frame changes slot and partner, the last pair is ragged
      pairs       a fixed permutation of whole pairs
      frames      a fixed permutation of the frames: other partners"""
    if kind == "base":
        return np.arange(n_frames)
    if kind == "zero_front":
        return np.concatenate([[ZERO], np.arange(n_frames)])
    if kind == "pairs":
        return permutation(n_frames, keep_pairs=True)
    if kind == "frames":
        return permutation(n_frames)
    raise ValueError(kind)


def slot_hits(acc, order, paired=True):
    """(indices exact-compared in slot a, in slot b) of a layout: the winners of its clear frames by the slot they ride
    in (place & 1; without pairing every frame rides in slot a)."""
    order = np.asarray(order)
    place = np.nonzero(order != ZERO)[0]
    f = order[place]
    c = acc.clear[f]
    slot = (place & 1) if paired else np.zeros_like(place)
    return (set(int(k) for k in acc.win[f][c & (slot == 0)]), set(int(k) for k in acc.win[f][c & (slot == 1)]))


def distinct_mag_mean(n_frames, scale=1.0, seed=PERM_SEED):
    """[n_frames, 2] float32 noise floors, the two floats of a frame distinct (the kernel reads the first)."""
    rng = np.random.default_rng(seed)
    mm = (rng.uniform(50.0, 400.0, size=(n_frames, 2)) * scale).astype(np.float32)
    mm[:, 1] = mm[:, 0] * np.float32(1.5) + np.float32(scale)
    assert (mm[:, 0] != mm[:, 1]).all()
    return mm


# ------------------------------------------------------------------------------------------------ stream: blocks

STREAM_CLEAR = 0.995    # a block is clear when the second-largest of its outputs <= 0.995 x the largest: 5e-3 = 250 x
#                         STREAM_TOL below the peak, where two bars (one per output) could overturn the order
STREAM_SIGNAL = 0.1     # ... and the largest is >= 0.1 x the stream's largest value, which is what the bar is relative to: a
#                         block of sidelobes only, 1e-3 of the stream's peak, has no lead that float32 can keep
BEHIND = 1.01           # ragged last block: the largest value behind `valid` >= 1.01 x the largest in front of it

STREAM_CASES = {
    "D4": dict(decim=4, flags=0),
    "D8": dict(decim=8, flags=0),
    "D16": dict(decim=16, flags=0),
    "D8-up": dict(decim=8, flags=uco.FLAG_STREAM_UP),
}
RAGGED_VALID = (1, 2, 63, 64, 65, 127, 128, 129, -1)      # -1: hop - 1


def stream_oracle(case):
    return uco.Oracle(uco.STREAM, **STREAM_CASES[case])


def stream_symbol(case):
    """The symbol the case's template compresses: an up chirp for the default (down) template, a down chirp under
    FLAG_STREAM_UP -- amplitude as synth.chirp_pair gives it."""
    from uchirp import synth
    up, down = synth.chirp_pair()
    return down if STREAM_CASES[case]["flags"] & uco.FLAG_STREAM_UP else up


def calibrate(o, sym):
    """One symbol in silence, then arg-max -> delay in samples: a symbol that starts at sample halo + q D - delay of the
    buffer compresses to a peak at output q.  (A shift by D samples moves every output by one: the mixer's phase is a
    constant factor, which |y| drops.)"""
    halo, _, _, _ = o.stream_geometry(0)
    D = int(o.cfg.decim)
    p0 = 2 * N
    x = np.zeros(halo + 6 * N, np.float32)
    x[halo + p0: halo + p0 + N] = sym
    comp, _ = o.process_stream(x)
    q0 = int(np.argmax(comp))
    assert 0 < q0 < comp.size - 1 and comp[q0] > 0
    return q0 * D - p0


def place(x, o, sym, delay, q):
    """Add to x the symbol that compresses to a peak at output q; a symbol cut off by the end of x stays cut off."""
    halo, _, _, _ = o.stream_geometry(0)
    start = halo + q * int(o.cfg.decim) - delay
    assert start >= 0
    part = sym[:max(0, min(N, x.size - start))]
    x[start:start + part.size] += part
    return start


def sweep_stream(case, dtype_name="float32"):
    """hop + 1 blocks: block 0 silence, block b = 1 .. hop ONE symbol placed so that its compressed peak is output
    b hop + (b - 1), offset b - 1 of the block; silence everywhere else -> (Oracle, samples, aimed offsets per block)."""
    o = stream_oracle(case)
    sym = stream_symbol(case)
    halo, _, _, hop = o.stream_geometry(0)
    D = int(o.cfg.decim)
    delay = calibrate(o, sym)
    x = np.zeros(halo + (hop + 1) * hop * D, np.float64)
    last = -N
    for b in range(1, hop + 1):
        start = place(x, o, sym, delay, b * hop + (b - 1))
        assert start >= last + N and start + N <= x.size          # no two symbols overlap, none is cut off
        last = start
    aimed = np.concatenate([[-1], np.arange(hop)])
    return o, to_dtype(x, np.dtype(dtype_name).type), aimed


class StreamAccount:
    """The oracle's outputs of a stream and, per block, its peak, second / first and whether the block is clear."""

    def __init__(self, o, x):
        self.o, self.x = o, x
        self.halo, self.n_out, self.n_blocks, self.hop = o.stream_geometry(x.size)
        self.comp, self.peaks = o.process_stream(x)
        self.scale = float(self.comp.max()) if self.comp.size else 0.0
        self.ratio = np.full(self.n_blocks, np.inf)
        self.clear = np.zeros(self.n_blocks, bool)
        whole = self.n_out // self.hop
        if whole:       # the whole blocks in one go
            segs = self.comp[:whole * self.hop].astype(np.float64).reshape(whole, self.hop)
            top = segs.max(axis=1)
            second = np.partition(segs, -2, axis=1)[:, -2]
            self.ratio[:whole] = np.where(top > 0, second / np.maximum(top, 1e-300), np.inf)
            self.clear[:whole] = (top > 0) & (second <= STREAM_CLEAR * top) & (top >= STREAM_SIGNAL * self.scale)
        for b in range(whole, self.n_blocks):
            seg = self.comp[b * self.hop:(b + 1) * self.hop].astype(np.float64)
            top = seg.max()
            if seg.size == 1:       # one candidate: nothing to confuse it with
                self.ratio[b], self.clear[b] = 0.0, True
                continue
            second = np.partition(seg, -2)[-2]
            self.ratio[b] = second / top if top > 0 else np.inf
            self.clear[b] = top > 0 and second <= STREAM_CLEAR * top and top >= STREAM_SIGNAL * self.scale

    def valid(self, b):
        return min(self.hop, self.n_out - b * self.hop)


def ragged_stream(valid, dtype_name="float32", case="D8"):
    """Two whole blocks with one symbol each and a last block of `valid` outputs; one more symbol is cut off by the end of
    the stream and compresses to a maximum BEHIND `valid` (what the kernel's out-of-range loads make of it: the same
    stream extended with zeros) -> (Oracle, samples, samples extended with zeros to a whole block, valid)."""
    o = stream_oracle(case)
    sym = stream_symbol(case)
    halo, _, _, hop = o.stream_geometry(0)
    D = int(o.cfg.decim)
    valid = hop - 1 if valid < 0 else valid
    delay = calibrate(o, sym)
    n_out = 2 * hop + valid
    x = np.zeros(halo + n_out * D, np.float64)
    ext = np.zeros(halo + 3 * hop * D, np.float64)
    behind = valid + 3          # the symbol ends 16 samples before its peak's: three outputs past the end, 8 samples are cut off
    for buf in (x, ext):
        place(buf, o, sym, delay, 700)
        place(buf, o, sym, delay, hop + 300)
        place(buf, o, sym, delay, 2 * hop + behind)
    assert np.array_equal(x, ext[:x.size]) and ext[x.size:].any()      # the end of the stream cuts the symbol off
    dt = np.dtype(dtype_name).type
    return o, to_dtype(x, dt), to_dtype(ext, dt), valid


# ------------------------------------------------------------------------------------------------ stream: non-finite samples

def blocks_reading(o, n_samples, s):
    """The overlap-save blocks that read sample s of a buffer (include/uchirp.h): block b computes the decimated
    samples z[p], p = b hop - (L - 1) .. (b + 1) hop - 1, each from the 27 samples that end at halo + p D -- samples
    b hop D .. halo + ((b + 1) hop - 1) D of the buffer."""
    halo, n_out, n_blocks, hop = o.stream_geometry(n_samples)
    D = int(o.cfg.decim)
    return [b for b in range(n_blocks) if b * hop * D <= s <= halo + ((b + 1) * hop - 1) * D]


def nonfinite_positions(o, n_samples):
    """{name: sample index}: one that only block 3 reads, the overlap blocks 3 and 4 share and its two edges, and one
    of the first `halo` samples."""
    halo, _, n_blocks, hop = o.stream_geometry(n_samples)
    D = int(o.cfg.decim)
    assert n_blocks >= 7
    return {
        "block3": halo + 3 * hop * D + 100,
        "overlap34": 4 * hop * D + 5,
        "last-of-3-alone": 4 * hop * D - 1,
        "first-of-overlap34": 4 * hop * D,
        "last-of-overlap34": halo + (4 * hop - 1) * D,
        "first-of-4-alone": halo + (4 * hop - 1) * D + 1,
        "halo": 5,
    }


def noise_stream(o, n_blocks=7, tail=13, seed=41):
    """n_blocks - 1 whole blocks and a ragged one of `tail` outputs, noise at the amplitude of the other tests."""
    halo, _, _, hop = o.stream_geometry(0)
    D = int(o.cfg.decim)
    rng = np.random.default_rng(seed + D)
    return (1000.0 * rng.standard_normal(halo + D * ((n_blocks - 1) * hop + tail))).astype(np.float32)
