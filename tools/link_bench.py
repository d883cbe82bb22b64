"""uc_link_transmit against the torch way of making the same receiver input (bench_legs.py's receive leg: torch.randn * 50,
then the slice-add of one tone), same process, same shape: 4096 streams x 176 blocks of 2048 float samples (5.9 GB).
torch gives every stream one message, one amplitude, one lead; the link call gives each of the 4096 its own text and
fractional lead.  HIP events around each call, after a clock ramp of >= 300 ms of work (batches of four calls of each kind
enqueued back to back, one synchronisation a batch), the two alternated three times; medians.  The fused call must not be
slower than the torch path by more than the 3 % box spread.  The figures under "side" (the Python wrapper, the signal
alone, int16 output) are timed once each after the alternated section, not alternated: they are no part of the verdict.
Usage: python tools/link_bench.py [streams=4096] [blocks=176] [iters=5]   (exit code 1 if the fused call is slower)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, FS, MSG = 2048, 78125.0, "Hello WorldC"
HBM_PEAK = 8.0e12


def main():
    import torch
    from uchirp import link, tx
    ns = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 176
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda:0")
    tone = torch.from_numpy(tx.render(MSG, fs_rx=FS, amplitude=2000.0).astype(np.float32)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(ns)

    def torch_path():
        x = torch.randn((ns, nb * N), generator=g, device=dev) * 50.0
        lead = 40 * N + 777
        x[:, lead:lead + tone.numel()] += tone
        return x

    rng = np.random.default_rng(1)
    texts = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=12)) for _ in range(ns)]
    lead = rng.uniform(25 * N, 46 * N, size=ns)
    text, p = link.pack(texts, lead, 2000.0, 50.0)
    tl = link.Link()
    L = link.lib()
    out = torch.empty((ns, nb * N), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def link_path(dtype=link.DTYPE_F32, buf=out):
        rc = L.uc_link_transmit(tl._h, text.ctypes.data_as(C.c_void_p), text.shape[1], p.ctypes.data_as(C.c_void_p), ns,
                                C.c_void_p(buf.data_ptr()), dtype, FS, 0, nb * N, 0, 1, stream)
        if rc:
            raise RuntimeError(L.uc_link_last_error().decode())

    def link_python():
        tl.transmit(texts, lead, 2000.0, 50.0, out=out, seed=1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(iters):
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return ts

    # clock ramp before anything is timed: batches of back-to-back calls, the host joins once a batch
    t0 = time.time()
    while time.time() - t0 < 0.3:
        for _ in range(4):
            link_path()
            torch_path()
        torch.cuda.synchronize()
    t_torch, t_link = [], []
    for _ in range(3):
        t_torch += timed(torch_path)
        t_link += timed(link_path)
    t_py = timed(link_python)
    p0 = p.copy()
    p["sigma"] = 0.0
    t_sig = timed(link_path)          # the signal alone (no generator): what the noise costs is the difference
    p[:] = p0
    out16 = torch.empty((ns, nb * N), dtype=torch.int16, device=dev)
    t_i16 = timed(lambda: link_path(link.DTYPE_I16, out16))
    mt, ml = float(np.median(t_torch)), float(np.median(t_link))
    nbytes = ns * nb * N * 4
    res = {"shape": [ns, nb * N], "bytes": nbytes, "torch_ms": mt, "link_ms": ml, "ratio_torch_over_link": mt / ml,
           "torch_ms_all": [round(t, 3) for t in t_torch], "link_ms_all": [round(t, 3) for t in t_link],
           "side": {"timed": "once each after the alternated section, not alternated",
                    "link_python_wrapper_ms": float(np.median(t_py)), "link_signal_only_ms": float(np.median(t_sig)),
                    "link_int16_ms": float(np.median(t_i16))},
           "link_bytes_per_s": nbytes / (ml * 1e-3), "link_fraction_of_8TBps": nbytes / (ml * 1e-3) / HBM_PEAK,
           "link_samples_per_s": ns * nb * N / (ml * 1e-3)}
    print(json.dumps(res))
    if ml > mt * 1.03:
        print("FAIL: the fused call (%.3f ms) is slower than the torch path (%.3f ms)" % (ml, mt))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
