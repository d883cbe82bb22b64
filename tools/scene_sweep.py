"""What do an echo and a second transmitter do to each receiver?  A grid of echo gain (-3, -6, -12, -20 dB) x echo delay
(0.1, 0.5, 1, 2, 5 ms, one symbol) at +14 dB SNR, the echo-free cell next to it, and one cell with an interferer (another
text at the same level, its own random lead) x {RX_REAL, SYNC_CPLX} x {literal TIME_FRAME 0.0205 s, matched 2048 / 78125 s};
every cell is 2048 independent transmissions (random text of 1 .. 6 characters, random lead of 25 .. 46 blocks, amplitude
2000) rendered by uc_scene_render on the device and decoded from the same buffer by uc_receive_streams.  Records per cell
the share of microphones whose decoded text contains the sent message.  Nothing is asserted: it is a record.
Usage: python tools/scene_sweep.py [out=profiles/r08_scene_sweep.json] [mics_per_cell=2048]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, FS, NB = 2048, 78125.0, 104
SNR_DB = 14.0                          # 20 log10(A / sigma): the symbol's rms is A
ECHO_DB = (-3.0, -6.0, -12.0, -20.0)
SYMBOL_S = int(0.0262 * 44100) / 44100.0
DELAY_S = (1e-4, 5e-4, 1e-3, 2e-3, 5e-3, SYMBOL_S)


def main():
    import torch
    import uchirp
    from uchirp import scene
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_scene_sweep.json")
    nm = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    sc = scene.Scene()
    engines = {}
    for vname, var in (("rx_real", uchirp.RX_REAL), ("sync_cplx", uchirp.SYNC_CPLX)):
        for tname, kw in (("literal", {}), ("matched", {"time_frame": N / FS})):
            engines["%s/%s" % (vname, tname)] = uchirp.Engine(var, **kw)
    rng = np.random.default_rng(8)
    buf = torch.empty((nm, NB * N), dtype=torch.float32, device="cuda:0")
    amp = 2000.0
    sigma = amp / 10.0 ** (SNR_DB / 20.0)
    cells = []
    t0 = time.time()

    def texts_and_leads():
        texts = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(1, 7)))) for _ in range(nm)]
        return texts, rng.integers(25, 46, size=nm) * float(N) + rng.uniform(0.0, N, size=nm)

    def run(kind, texts, mics, seed, **rec):
        sc.render(texts, mics, out=buf, seed=seed)
        for name, eng in engines.items():
            got, _ = eng.receive_many(buf, want_trace=False)
            ok = sum(1 for s in range(nm) if texts[s] in got[s])
            cells.append(dict(rec, kind=kind, receiver=name, mics=nm, decode_rate=ok / nm))
        print("%s %s done (%.0f s)" % (kind, rec, time.time() - t0), flush=True)

    texts, lead = texts_and_leads()
    run("clean", texts, [(sigma, [(i, amp, lead[i], 0.0)]) for i in range(nm)], 1)
    seed = 2
    for g_db in ECHO_DB:
        g = 10.0 ** (g_db / 20.0)
        for d in DELAY_S:
            texts, lead = texts_and_leads()
            run("echo", texts, [(sigma, [(i, amp, lead[i], 0.0), (i, amp * g, lead[i] + d * FS, 0.0)]) for i in range(nm)], seed,
                echo_db=g_db, delay_ms=round(d * 1e3, 4))
            seed += 1
    texts, lead = texts_and_leads()
    other, other_lead = texts_and_leads()
    run("interferer", texts + other, [(sigma, [(i, amp, lead[i], 0.0), (nm + i, amp, other_lead[i], 0.0)]) for i in range(nm)], seed)
    summary = {}
    for name in engines:
        sel = [c for c in cells if c["receiver"] == name]
        summary[name] = {"clean": [c["decode_rate"] for c in sel if c["kind"] == "clean"][0],
                         "interferer": [c["decode_rate"] for c in sel if c["kind"] == "interferer"][0],
                         "echo_rows_db": list(ECHO_DB), "echo_columns_ms": [round(d * 1e3, 4) for d in DELAY_S],
                         "echo": [[[c["decode_rate"] for c in sel if c["kind"] == "echo" and c["echo_db"] == g and
                                    c["delay_ms"] == round(d * 1e3, 4)][0] for d in DELAY_S] for g in ECHO_DB]}
    rec = {"what": "decode rate of uc_receive_streams on scenes rendered by uc_scene_render (tools/scene_sweep.py); measured on one "
                   "MI355X; decode = the decoded text contains the sent message; interferer: another text, same level, own random lead",
           "mics_per_cell": nm, "blocks_per_mic": NB, "amplitude": amp, "snr_db": SNR_DB, "summary": summary, "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
