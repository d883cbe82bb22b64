"""Which sample skews do the receivers decode, and at which noise level?  (VERDICT "missing" 2, at scale.)
A grid of skew (64 values in [0, 2048)) x SNR x {RX_REAL, SYNC_CPLX} x {literal TIME_FRAME 0.0205 s, matched 2048 / 78125 s};
every cell is 2048 independent transmissions (random text of 1 .. 6 characters, random whole blocks of lead 25 .. 45 plus
the cell's skew, amplitude 2000, the cell's noise) made by uc_link_transmit on the device and decoded from the same buffer
by uc_receive_streams.  Records the share of streams whose decoded text contains the sent message per cell, and per
receiver and SNR the skews where fewer than half do.  Nothing is asserted: it is a record.
Usage: python tools/link_sweep.py [out=profiles/r07_link_sweep.json] [streams_per_cell=2048] [skews=64]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, FS, NB = 2048, 78125.0, 104
SNR_DB = (26.0, 14.0, 0.0, -10.0)     # 20 log10(A / sigma): the symbol's rms is A


def main():
    import torch
    import uchirp
    from uchirp import link
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_link_sweep.json")
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    n_skew = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    skews = [int(round(k * N / n_skew)) for k in range(n_skew)]
    tl = link.Link()
    engines = {}
    for vname, var in (("rx_real", uchirp.RX_REAL), ("sync_cplx", uchirp.SYNC_CPLX)):
        for tname, kw in (("literal", {}), ("matched", {"time_frame": N / FS})):
            engines["%s/%s" % (vname, tname)] = uchirp.Engine(var, **kw)
    rng = np.random.default_rng(7)
    buf = torch.empty((ns, NB * N), dtype=torch.float32, device="cuda:0")
    amp = 2000.0
    cells = []
    t0 = time.time()
    for ci, skew in enumerate(skews):
        texts = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(1, 7)))) for _ in range(ns)]
        lead = rng.integers(25, 46, size=ns) * float(N) + skew
        for snr in SNR_DB:
            sigma = amp / 10.0 ** (snr / 20.0)
            tl.transmit(texts, lead, amp, sigma, out=buf, seed=ci * 16 + SNR_DB.index(snr))
            for name, eng in engines.items():
                got, _ = eng.receive_many(buf, want_trace=False)
                ok = sum(1 for s in range(ns) if texts[s] in got[s])
                cells.append({"skew": skew, "snr_db": snr, "receiver": name, "streams": ns, "decode_rate": ok / ns})
        print("skew %4d done (%.0f s)" % (skew, time.time() - t0), flush=True)
    failing = {}
    for name in engines:
        for snr in SNR_DB:
            sel = [c for c in cells if c["receiver"] == name and c["snr_db"] == snr]
            failing["%s @ %+.0f dB" % (name, snr)] = {
                "mean_decode_rate": float(np.mean([c["decode_rate"] for c in sel])),
                "skews_below_half": [c["skew"] for c in sel if c["decode_rate"] < 0.5]}
    rec = {"what": "decode rate of uc_receive_streams on transmissions rendered by uc_link_transmit (tools/link_sweep.py); "
                   "measured on one MI355X; decode = the decoded text contains the sent message",
           "streams_per_cell": ns, "blocks_per_stream": NB, "amplitude": amp, "skews": skews, "snr_db": list(SNR_DB),
           "summary": failing, "cells": cells}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0)
    print(json.dumps(failing, indent=1))


if __name__ == "__main__":
    main()
