"""The records of the receivers' band kernel (the ROWS build), oracle side.

uc_receive_streams[_next] run a build of the band kernel of their own: every frame is read through two buffer resources
(the tail of the block in front, the head of the new block), unit -> (row, block, m) goes through a magic divisor, and a
second finaliser writes only (up, down) mag_max.  uc_debug_rx_records reads those records back; this module says what
they must be.

THE DEFINITION.  P = the block in front of the call (zeros at power-on), X = the stream's ACCEPTED blocks.  Unit (jb, m),
m = 1 .. 8, is the frame concat(P, X)[2048 jb + 256 m : 2048 jb + 256 m + 2048]: frame k = 8 jb + m of
Oracle.process(concat(P, X), n_frames = 8 nb + 1, stride = 256); frame 0 is P itself and no unit.  The record is
(stats[k, 0].mag_max, stats[k, 1].mag_max) of the float64 oracle, at index u = k - 1 = 8 jb + (m - 1).

THE BAR (worst_of).  parity_util.MAG_TOL x the frame's largest window magnitude -- which is the oracle's record itself,
floored at 1e-30 as parity_util.window_scale does.  Where the oracle's record is exactly 0 (an all-zero frame) the GPU's
is exactly +0; where it is NaN the GPU's is NaN.

THE SWEEP (Sweep).  The frames of tone_sweep_util.build_frames, 2048 + 256 samples apart behind a power-on block, in 8
rows, row r shifted by 256 r samples, zeros elsewhere: frame q lies whole on FIFO offset m = (q + r) mod 8 (0: 8) of row
r, so every tone frame lies on every offset once.  For each frame the oracle's float64 spectrum says which bin wins each
window of each history and whether that winner DECIDES the record clearly: second <= CLEAR x first, window >= SIGNAL x
the history's window maximum, and this window's maximum >= the other window's (mag_max is the larger of the two).

  tests/test_rows_records_cpu.py   oracle only: the coverage the GPU test relies on, the mapping, the state machine
  tests/test_gpu_rows_records.py   the kernel against that
"""
import functools

import numpy as np

from oracle import uco
from parity_util import MAG_TOL
import tone_sweep_util as tsu

N = 2048
STEP = 256                    # FIFO offsets are 256 samples apart (main.c:406: offset = n / 8)
PER_BLOCK = N // STEP
PITCH = N + STEP              # the sweep's frames lie 2304 samples apart
ROWS = 8
NAN_WORD = {"float32": np.float32(np.nan), "int32": np.int32(-2 ** 31)}     # what fills the gaps between strided streams

SWEEP_CASES = ["rx_real-literal", "rx_real-matched", "sync_cplx-literal", "sync_cplx-matched",
               "rx_real-wide294", "rx_real-wide318", "sync_cplx-wide294", "sync_cplx-wide318"]
# ... and the widths at which the owner of bin bandwidth2 changes (tone_sweep_util.SEAM_WIDTHS): wave 1 slot 0, wave 1 slot 1,
# the first WIDE window, the first bin of the third round
SWEEP_CASES += [tsu.seam_name(kind, w) for w in (64, 128, 192, 256) for kind in ("rx_real", "sync_cplx")]
DTYPES = ["float32", "int32"]


def oracle_for(name, dtype_name="float32"):
    variant, cfg = tsu.config(name)
    return uco.Oracle(variant, mag_mean=1000.0 * (256.0 if dtype_name == "int32" else 1.0), **cfg)


def accepted_rows(x, busy=None):
    """The ISR drops a block that arrives while the consumer is busy (main.c:659-668): the FIFO holds accepted blocks only.
    x [n_streams, nb * N] -> list of arrays [na_s * N]."""
    x = np.asarray(x)
    nb = x.shape[1] // N
    if busy is None:
        return [x[s, :nb * N] for s in range(x.shape[0])]
    return [np.concatenate([x[s, b * N:(b + 1) * N] for b in range(nb) if not busy[s, b]] + [x[s, :0]]) for s in range(x.shape[0])]


def expected_row(o, row, prev=None):
    """One stream: float64 [8 na, 2] -- the definition.  row: its accepted blocks; prev: the block in front (None: zeros)."""
    na = row.size // N
    p = np.zeros(N, row.dtype) if prev is None else np.asarray(prev, row.dtype)
    buf = np.concatenate([p, row[:na * N]])
    _, st = o.process(buf, n_frames=PER_BLOCK * na + 1, stride=STEP)
    out = np.empty((PER_BLOCK * na, 2), np.float64)
    out[:, 0] = st[1:, 0]["mag_max"]
    out[:, 1] = st[1:, 1]["mag_max"]
    return out


def expected(o, x, prev=None, busy=None):
    """Every stream of a call: list (one entry per stream) of float64 [8 na_s, 2]; without a busy mask one array
    [n_streams, 8 nb, 2].  prev: [n_streams, N] or None (power-on)."""
    rows = accepted_rows(x, busy)
    out = [expected_row(o, r, None if prev is None else prev[s]) for s, r in enumerate(rows)]
    return out if busy is not None else np.stack(out)


def last_accepted(x, prev, busy=None):
    """The block in front of the NEXT call: every stream's newest accepted block (a stream that accepted nothing keeps its own)."""
    rows = accepted_rows(x, busy)
    out = np.zeros((len(rows), N), np.asarray(x).dtype) if prev is None else np.array(prev, copy=True)
    for s, r in enumerate(rows):
        if r.size >= N:
            out[s] = r[-N:]
    return out


def ratios(got, want):
    """|gpu - oracle| / (MAG_TOL x scale) per component, scale = the oracle's record floored at 1e-30; inf where the oracle
    has an exact 0 and the GPU not +0 (bit for bit), or the oracle has NaN and the GPU not; 0 where they have it alike."""
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        r = np.abs(got.astype(np.float64) - want) / (MAG_TOL * np.maximum(want, 1e-30))
    zero, nan = want == 0.0, np.isnan(want)
    r[zero] = np.where(got.view(np.uint32)[zero] == 0, 0.0, np.inf)
    r[nan] = np.where(np.isnan(got[nan]), 0.0, np.inf)
    r[~nan & ~np.isfinite(got)] = np.inf
    return r


def worst_of(got, want):
    r = ratios(got, want)
    return float(r.max()) if r.size else 0.0


def passed_over(got, poison=False):
    """Components a one-block call of a live state passed over: exactly +0, or exactly 1e15f under UC_RX_POISON=1."""
    got = np.asarray(got, np.float32)
    return got.view(np.uint32) == np.float32(1e15 if poison else 0.0).view(np.uint32)


class Sweep:
    """The sweep layout of one case and the oracle's account of it."""

    def __init__(self, name, dtype_name):
        self.name, self.dtype_name = name, dtype_name
        o = self.o = oracle_for(name, dtype_name)
        frames, _ = tsu.build_frames(name, o)
        self.frames = tsu.to_dtype(frames, np.dtype(dtype_name).type)
        nf = self.n_frames = len(frames)
        self.nb = -(-((nf - 1) * PITCH + N + (ROWS - 1) * STEP) // N)          # whole blocks, one length for all rows
        self.x = np.zeros((ROWS, self.nb * N), self.frames.dtype)
        for r in range(ROWS):
            for q in range(nf):
                at = q * PITCH + r * STEP
                self.x[r, at:at + N] = self.frames[q]
        self.x.setflags(write=False)
        # designed unit of (row r, frame q): the frame starts at sample N + q PITCH + r STEP of concat(P, X) = 256 k
        q, r = np.meshgrid(np.arange(nf), np.arange(ROWS))
        k = PER_BLOCK + (PER_BLOCK + 1) * q + r
        self.unit = k - 1                                                      # [ROWS, nf]
        self.m = (k - 1) % PER_BLOCK + 1
        self.windows = tsu.windows_of(o, False)
        # per frame: the (history, side, bin) that decide a record clearly
        self.deciders = []                                                     # [nf] lists of (h, side, bin)
        for f in range(nf):
            spec = o.spectrum(self.frames[f])
            dec = []
            for h in range(o.spf):
                top, win, second = {}, {}, {}
                for s, (a, b) in self.windows.items():
                    w = spec[h][a:b]
                    i = int(np.argmax(w))
                    top[s], win[s], second[s] = w[i], a + i, np.partition(w, -2)[-2]
                scale = max(top.values())
                for s, other in (("left", "right"), ("right", "left")):
                    if top[s] > 0 and second[s] <= tsu.CLEAR * top[s] and top[s] >= tsu.SIGNAL * scale and top[s] >= top[other]:
                        dec.append((h, s, win[s]))
            self.deciders.append(dec)
        self.want = expected(o, self.x)                                        # [ROWS, 8 nb, 2] float64
        self.want.setflags(write=False)

    def whole(self):
        return {(s, k) for s, (a, b) in self.windows.items() for k in range(a, b)}

    def coverage(self, m):
        """{(side, bin)} that decide a record clearly in a designed unit at FIFO offset m."""
        out = set()
        for r in range(ROWS):
            for f in np.nonzero(self.m[r] == m)[0]:
                out |= {(s, k) for _, s, k in self.deciders[f]}
        return out

    def designed(self):
        """(row, unit, history) of every record a clear winner decides -- the components the coverage rests on."""
        return [(r, int(self.unit[r, f]), h) for r in range(ROWS) for f in range(self.n_frames) for h, _, _ in self.deciders[f]]


@functools.lru_cache(maxsize=2)
def sweep(name, dtype_name):
    return Sweep(name, dtype_name)


# ---- noise plus a few chirp symbols: the inputs of the geometry, live and edge tests ---------------------------------------
GEOMETRIES = {                # name -> (tone-sweep case whose configuration it takes)
    "rx_real": "rx_real-literal",
    "sync_cplx": "sync_cplx-literal",
    "sync_cplx-wide294": "sync_cplx-wide294",
}


@functools.lru_cache(maxsize=None)
def noisy_streams(geometry, dtype_name, n_streams=37, nb=31, seed=7):
    """[n_streams, nb * N]: noise in EVERY sample (sigma 50; no true record is 0) and a few up / down chirps of amplitude 2000 at
    random places, so that some streams lock and track -> (streams, Oracle)."""
    from uchirp import synth
    o = oracle_for(GEOMETRIES[geometry], dtype_name)
    up, down = synth.chirp_pair(fs=float(o.cfg.fs), f0=float(o.cfg.f0), f1=float(o.cfg.f1), amp=2000.0)
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 50.0, size=(n_streams, nb * N))
    for s in range(n_streams):
        at = int(rng.integers(0, 4 * N))
        for kind in rng.integers(0, 2, size=int(rng.integers(3, 2 * nb // 3 + 1))):
            if at + N > nb * N:
                break
            x[s, at:at + N] += up if kind else down
            at += N
    x = tsu.to_dtype(x, np.dtype(dtype_name).type)
    x.setflags(write=False)
    return x, o


@functools.lru_cache(maxsize=None)
def noisy_expected(geometry, dtype_name):
    """The oracle's records of noisy_streams at power-on, [n_streams, 8 nb, 2]: records of the first k blocks do not depend on
    the later ones, so every prefix of every subset of the streams reads its expectation here."""
    x, o = noisy_streams(geometry, dtype_name)
    want = expected(o, x)
    want.setflags(write=False)
    return want


# ---- main()'s switch over the helper's records (include/uchirp_mainloop.hpp restated in float32 numpy) ---------------------
def replay(records, blocks, n=N, thr=2.0):
    """records float32 [8 na, 2] of a stream at power-on -> trace (uco.RX_EVENT_DTYPE) of the receiver whose dsp(position) looks
    the frame up in `records`: FIFO position p of accepted block i is frame k = 8 (i - 1) + p / 256, zeros for k <= 0.
    blocks: the original index of every accepted block."""
    f32 = np.float32
    rec = np.asarray(records, f32)
    na = rec.shape[0] // PER_BLOCK
    offset, shift = n // 8, n // 4
    hist = [dict(mag_max=f32(0), mag_mean=f32(0), snr=f32(0)) for _ in range(8)]
    mag_stat = [f32(1e37)] * 12
    state = {"v": 0, "turn": 0, "max_idx": 0, "sync_cnt": 0, "pos": n // 2, "mag_mean": f32(0)}
    trace = np.zeros(na, uco.RX_EVENT_DTYPE)

    def dsp(i, pos, h, mag_mean, updown):
        k = PER_BLOCK * (i - 1) + pos // STEP
        assert pos % STEP == 0
        mx = rec[k - 1, 0 if updown else 1] if k >= 1 else f32(0)
        h["mag_max"], h["mag_mean"] = mx, f32(mag_mean)
        with np.errstate(all="ignore"):
            h["snr"] = f32(f32(mx - f32(mag_mean)) / f32(mag_mean))

    def symbol_snr(i, pos, h, updown):
        dsp(i, pos, h, h["mag_mean"], updown)
        return h["snr"]

    def resync(i, snr, updown):
        pl, pr = state["pos"] - offset, state["pos"] + offset
        sl = sr = f32(-np.inf)
        if pl >= 0:
            sl = symbol_snr(i, pl, hist[2], updown)
        if pr <= 2 * n:
            sr = symbol_snr(i, pr, hist[3], updown)
        if snr > sl and snr > sr:
            return
        if sl >= sr:
            if pl >= 0:
                state["pos"] = pl
        elif sl < sr:
            if pr <= 2 * n:
                state["pos"] = pr

    for i in range(na):
        ev = trace[i]
        ev["block"], ev["state_before"], ev["bit"] = blocks[i], state["v"], -1
        if state["v"] in (0, 1):
            if state["v"] == 0:
                state["sync_cnt"] = 0
                acc = f32(0)
                for v in mag_stat[4:12]:
                    acc = f32(acc + v)
                state["mag_mean"] = f32(acc / f32(8))
            for j in range(4):
                state["pos"] = n // 2 + state["turn"] * offset + shift * j
                dsp(i, state["pos"], hist[j * 2 + state["turn"]], state["mag_mean"], 1)
            state["turn"] ^= 1
            if state["turn"] == 1:
                mag_stat = [None] + mag_stat[:11]
                mmm = f32(0)
                for j in range(8):
                    if hist[j]["mag_max"] > mmm:
                        mmm, state["max_idx"] = hist[j]["mag_max"], j
                mag_stat[0] = mmm
                snr = f32(f32(mmm - state["mag_mean"]) / state["mag_mean"])
                if snr >= thr:
                    state["v"] = 1
                    state["sync_cnt"] += 1
                    if state["sync_cnt"] >= 3:
                        state["v"] = 2
                        state["pos"] = n // 2 + state["max_idx"] * offset
                else:
                    state["v"] = 0
        else:
            su = symbol_snr(i, state["pos"], hist[0], 1)
            sd = symbol_snr(i, state["pos"], hist[1], 0)
            ev["snr_up"], ev["snr_down"] = su, sd
            if su >= thr or sd >= thr:
                if sd > su:
                    if state["v"] == 3:
                        ev["bit"] = 0
                    resync(i, sd, 0)
                    state["v"] = 3
                else:
                    if state["v"] == 3:
                        ev["bit"] = 1
                    resync(i, su, 1)
            else:
                state["v"] = 0
        ev["state_after"], ev["sync_position"] = state["v"], state["pos"]
    return trace
