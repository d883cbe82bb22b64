#!/usr/bin/env python3
"""uc_receive_stream[_isr] vs the oracle's literal sequential main loop on random transmissions: random text, noise
level, lead length, sample skew, busy (dropped-block) masks, both up/down variants.  The traces must agree field by
field wherever the state machine's decisions are not within round-off of a threshold.
path: single (default) = uc_receive_stream_isr, one stream at a time; stepped = uc_receive_streams served block by block
(UC_TUNING=1 UC_RX_STEP_MIN=1; a busy-masked case is served in one launch as ever); live = uc_receive_streams_next, one block
per call, default contract; kept = the same with uc_rx_state_keep_previous on a ring of two device buffers (a busy-masked call
hands the block to the state as ever).  The classifier is the tests' own (tests/test_gpu_receive_many.py: classify_divergence).
Usage: python tools/fuzz_receive.py [cases=60] [seed=1] [path=single|stepped|live|kept]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
path = sys.argv[3] if len(sys.argv) > 3 else "single"
if path not in ("single", "stepped", "live", "kept"):
    sys.exit("path must be single, stepped, live or kept")
if path == "stepped":            # (read when a context is created)
    os.environ["UC_TUNING"] = "1"
    os.environ["UC_RX_STEP_MIN"] = "1"
import numpy as np
import uchirp
from uchirp import tx
from oracle import uco
from test_gpu_receive_many import FIELDS, classify_divergence


def receive(e, x, busy):
    """One stream through the chosen path -> (text, trace)."""
    if path == "single":
        return e.receive(x, busy=busy)
    nb = x.size // 2048
    rows = x[:nb * 2048].reshape(1, -1)
    bz = None if busy is None else np.ascontiguousarray(busy, np.uint8).reshape(1, nb)
    if path == "stepped":
        texts, traces = e.receive_many(rows, busy=bz)
        return texts[0], traces[0]
    import torch
    xd = torch.from_numpy(rows).to("cuda:0")
    live = e.live(1)
    live.keep_previous(path == "kept")
    ring = [torch.zeros((1, 2048), dtype=xd.dtype, device="cuda:0") for _ in range(2)]
    text, trace = "", []
    for b in range(nb):
        ring[b % 2].copy_(xd[:, b * 2048:(b + 1) * 2048])
        t, tr = live.next(ring[b % 2], busy=None if bz is None else np.ascontiguousarray(bz[:, b:b + 1]))
        text += t[0]
        trace.append(tr[0])
    live.close()
    return text, np.concatenate(trace) if trace else np.zeros(0, uchirp.RX_EVENT_DTYPE)


cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = soft = decoded = 0
for case in range(cases):
    variant = int(rng.choice([uco.RX_REAL, uco.SYNC_CPLX]))
    msg = "".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(1, 9))))
    amp = float(rng.choice([500.0, 2000.0, 8000.0]))
    sigma = amp * float(rng.choice([0.01, 0.05, 0.2, 0.5]))
    tone = tx.render(msg, fs_rx=78125.0, amplitude=amp)
    lead = rng.standard_normal(int(rng.integers(25, 50)) * 2048 + int(rng.integers(0, 2048))) * sigma
    tail = rng.standard_normal(int(rng.integers(4, 30)) * 2048) * sigma
    x = np.concatenate([lead, tone + rng.standard_normal(tone.size) * sigma, tail]).astype(np.float32)
    nb = x.size // 2048
    busy = None
    if rng.random() < 0.4:
        busy = rng.random(nb) < float(rng.choice([0.02, 0.1, 0.3]))
    if rng.random() < 0.3:
        x = (np.round(x).astype(np.int64) * 256).astype(np.int32)
    o, e = uco.Oracle(variant), uchirp.Engine(variant)
    text_o, tr_o, mg_o = o.receive(x, precision=uco.F64, busy=busy, margins=True)
    text_g, tr_g = receive(e, x, busy)
    e.close()
    decoded += int(msg in text_o)
    same = text_g == text_o and len(tr_g) == len(tr_o) and all(np.array_equal(tr_g[f], tr_o[f]) for f in FIELDS)
    if not same:
        # a decision within float32 round-off of going the other way is allowed to differ: the first diverging block is
        # judged by the ORACLE's own closest decision there (uco_receive_stream_diag: the acquisition maximum against
        # (1 + SNR_THRESHOLD) x mag_mean and against the runner-up, the snrs against the threshold and each other,
        # resync()'s compares) -- the rule of tests/test_gpu_receive_many.py
        kind, i, gap = classify_divergence(tr_g, tr_o, mg_o)
        if kind == "soft":
            soft += 1
            print("near-tie divergence case %d block %d: the oracle's closest decision there had a relative gap of %.2e" % (case, i, gap), flush=True)
        else:
            bad += 1
            print("FAIL case %d variant %d msg %r amp %g sigma %g busy %s: first differing block %d (gap %.3e)\n  oracle %r\n  gpu    %r"
                  % (case, variant, msg, amp, sigma, busy is not None, i, gap, text_o, text_g), flush=True)
    if case % 20 == 19:
        print("%d cases, %d failures, %d near-threshold divergences" % (case + 1, bad, soft), flush=True)
print("done: %d cases, %d failures, %d near-threshold divergences; the oracle decoded the transmitted text in %d cases (path %s)" % (cases, bad, soft, decoded, path))
sys.exit(1 if bad else 0)
