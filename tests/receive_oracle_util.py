"""Shared by tests/test_gpu_receive_oracle.py (GPU) and tests/test_receive_oracle_inputs.py (CPU): the fixed inputs of the
oracle legs, the oracle run over many streams from a thread pool, and the verdict of a leg.

The verdict is the rule of test_a_thousand_random_transmissions_with_dropped_blocks_against_the_oracle: a stream passes when its
text, its trace length and every field of FIELDS equal the float64 oracle's; otherwise classify_divergence judges the first
differing block by the ORACLE's own margin there."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from uchirp import synth, tx
from oracle import uco
from test_gpu_receive_many import FIELDS, SOFT_GAP, _transmissions, classify_divergence

N = 2048
SEED, STREAMS, BLOCKS = 2601, 1024, 150
WORKERS = min(16, os.cpu_count() or 1)
SNR_RTOL, SNR_ATOL = 1e-4, 1e-3          # tests/test_gpu_parity.py: test_receive_stream_state_machine_matches_oracle
WIDE_FS = 125000.0 / 3.0
WIDE_KW = dict(fs=WIDE_FS, time_frame=2048.0 / WIDE_FS)
WIDE_STREAMS, WIDE_BLOCKS = 64, 110


@functools.lru_cache(maxsize=None)
def transmissions():
    """The 1024 streams of seed 2601 (150 blocks each) and their messages; the busy masks the generator draws are set aside."""
    x, _, msgs = _transmissions(STREAMS, seed=SEED, blocks=BLOCKS)
    x.setflags(write=False)
    return x, msgs


@functools.lru_cache(maxsize=None)
def busy_masks():
    """The busy masks of the 1000-transmission test (seed 5): about half of the rows drop 2 .. 30 % of their blocks."""
    _, busy, _ = _transmissions(1000, seed=5, blocks=BLOCKS)
    busy.setflags(write=False)
    return busy


@functools.lru_cache(maxsize=None)
def wide_transmissions():
    """The stream generator of test_live_receivers_with_wide_windows (41.7 kHz DFSDM setting, bandwidth2 = 294, one symbol = one
    frame, seed 17), extended to 64 streams."""
    up, down = synth.chirp_pair(fs=WIDE_FS, amp=2000.0)
    sym = {1: up, 0: down, -1: np.zeros(N)}
    rng = np.random.default_rng(17)
    x = np.zeros((WIDE_STREAMS, WIDE_BLOCKS * N), np.float32)
    msgs = []
    for s in range(WIDE_STREAMS):
        msg = "".join(chr(int(c)) for c in rng.integers(48, 123, size=int(rng.integers(1, 4))))
        tone = np.concatenate([sym[int(v)] for v in tx.symbol_sequence(msg)])
        lead = int(rng.integers(26, 40)) * N + int(rng.integers(0, N))
        row = rng.normal(0.0, 50.0, size=WIDE_BLOCKS * N)
        row[lead:lead + tone.size] += tone
        x[s] = row.astype(np.float32)
        msgs.append(msg)
    x.setflags(write=False)
    return x, msgs


def words(x):
    """The int32 DFSDM words of float32 samples (24-bit data left-aligned in 32)."""
    return (np.round(x).astype(np.int64) * 256).astype(np.int32)


def oracle_many(variant, x, busy=None, precision=uco.F64, **kw):
    """uco.Oracle(variant, **kw).receive(x[s], precision, busy[s], margins=True) for every stream, from a pool of at most 16
    threads with one Oracle each (the call releases the GIL) -> list of (text, trace, margins)."""
    ns = x.shape[0]
    workers = max(1, min(WORKERS, ns))

    def part(w):
        o = uco.Oracle(variant, **kw)
        out = [(s, o.receive(x[s], precision=precision, busy=None if busy is None else busy[s], margins=True))
               for s in range(w, ns, workers)]
        o.close()
        return out

    res = [None] * ns
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for chunk in pool.map(part, range(workers)):
            for s, r in chunk:
                res[s] = r
    return res


def judge(label, got, ref, msgs=None):
    """The verdict of a leg.  got: iterable of (source stream, text, trace) -- the receiver under test; several entries may name
    the same source (tiled streams).  ref: oracle_many()'s result, indexed by source.  -> dict(bad, soft, decoded, streams,
    snr_blocks, snr_worst): `soft` / `bad` count distinct SOURCE streams (every copy of a diverging source must diverge the same
    way, else the source is bad); snr_worst is the largest |got - oracle| / (atol + rtol |oracle|) of snr_up / snr_down over the
    blocks with state_before >= 2 of the streams whose FIELDS match -- above 1 the bar is missed."""
    seen = {}                                         # source -> (kind, block, what the receiver said there)
    lanes = lines = 0
    snr_blocks, snr_worst, snr_ok = 0, 0.0, True
    for src, text_g, tr_g in got:
        lanes += 1
        text_o, tr_o, mg_o = ref[src]
        same = text_g == text_o and len(tr_g) == len(tr_o) and all(np.array_equal(tr_g[f], tr_o[f]) for f in FIELDS)
        if same:
            sig = ("same", -1, ())
            act = tr_o["state_before"] >= 2
            for f in ("snr_up", "snr_down"):
                g, o = tr_g[f][act].astype(np.float64), tr_o[f][act].astype(np.float64)
                if not np.allclose(g, o, rtol=SNR_RTOL, atol=SNR_ATOL):
                    snr_ok = False
                    i = int(np.nonzero(~np.isclose(g, o, rtol=SNR_RTOL, atol=SNR_ATOL))[0][0])
                    print("%s: SNR source %d %s block %d: %r vs the oracle's %r" % (label, src, f, tr_o["block"][act][i], g[i], o[i]))
                fin = np.isfinite(g) & np.isfinite(o)
                if fin.any():
                    snr_worst = max(snr_worst, float((np.abs(g[fin] - o[fin]) / (SNR_ATOL + SNR_RTOL * np.abs(o[fin]))).max()))
            snr_blocks += int(act.sum())
        else:
            kind, i, gap = classify_divergence(tr_g, tr_o, mg_o)
            there = tuple(int(tr_g[f][i]) for f in FIELDS) if i < len(tr_g) else ()
            sig = (kind, i, there + (text_g,))
            lines += int(src not in seen)
            if src not in seen and lines <= 12:           # (a control leg diverges everywhere: the first dozen tell the story)
                print("%s: %s source %d block %d, the oracle's closest decision there had a relative gap of %.3e: %r vs %r"
                      % (label, "soft" if kind == "soft" else "FAIL", src, i, gap, text_o, text_g))
        if src not in seen:
            seen[src] = sig
        elif seen[src] != sig and seen[src][2] != "copies disagree":
            print("%s: FAIL source %d: its copies disagree, %r and %r" % (label, src, seen[src][:2], sig[:2]))
            seen[src] = ("bad", sig[1], "copies disagree")
    bad = sum(1 for v in seen.values() if v[0] == "bad")
    soft = sum(1 for v in seen.values() if v[0] == "soft")
    decoded = None if msgs is None else sum(int(msgs[src] in ref[src][0]) for src in seen)
    out = dict(bad=bad, soft=soft, decoded=decoded, sources=len(seen), streams=lanes, snr_blocks=snr_blocks,
               snr_worst=snr_worst, snr_ok=snr_ok)
    print("%s: %d streams of %d sources: bad %d, soft %d (gap < %.0e), oracle decoded %s; snr_up / snr_down on %d tracking blocks: "
          "worst %.4f of the bar (rtol %.0e, atol %.0e)" % (label, lanes, len(seen), bad, soft, SOFT_GAP,
                                                            "-" if decoded is None else "%d of %d" % (decoded, len(seen)),
                                                            snr_blocks, snr_worst, SNR_RTOL, SNR_ATOL))
    return out


def decoded_floor(sources):
    """At least 1000 of the 1024 messages, or the same share of a subset."""
    return -(-1000 * sources // 1024)
