"""uc_scene_render against what the libraries offered before it for the same buffer, same process, same shape: 4096
microphones x 176 blocks of 2048 float samples (5.9 GB), P = 4 paths each (a direct path and three echoes of a 12-byte
message, every microphone its own text and leads, noise once).
  composition   4 uc_link_transmit calls into 4 buffers (the noise in the first) + 3 in-place torch adds
  scene         1 uc_scene_render call
and P = 1: uc_scene_render against uc_link_transmit itself (the same bits).
HIP events around each variant, after a clock ramp of >= 300 ms of work (batches of back-to-back calls, one
synchronisation a batch), the variants alternated three times with `iters` timings each; medians.  The figure under
"side" (P = 4 of a 1-byte message: most tiles of most paths are silent and skipped) is timed once after the alternated
section, not alternated: it is no part of the verdict.
Usage: python tools/scene_bench.py [mics=4096] [blocks=176] [iters=5]
(exit code 1 if the one-pass render is not faster than the composition at P = 4)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, FS = 2048, 78125.0
HBM_PEAK, HBM_WRITE = 8.0e12, 6.0e12
GAINS = (1.0, 0.5, 0.3, 0.2)


def main():
    import torch
    from uchirp import link, scene
    nm = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 176
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    P = len(GAINS)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    lead = rng.uniform(25 * N, 46 * N, size=nm)
    delay = np.concatenate([np.zeros((nm, 1)), np.cumsum(rng.uniform(8.0, 160.0, size=(nm, P - 1)), axis=1)], axis=1)   # 0.1 .. 6 ms

    def scene_of(texts, paths):
        return scene.pack(texts, [(50.0, [(i, 2000.0 * GAINS[k], lead[i] + delay[i, k], 0.0) for k in range(paths)]) for i in range(nm)])

    texts = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=12)) for _ in range(nm)]
    packed4, packed1, short4 = scene_of(texts, P), scene_of(texts, 1), scene_of([t[:1] for t in texts], P)
    text, _, _, _ = packed4
    params = [link.pack(texts, lead + delay[:, k], 2000.0 * GAINS[k], 50.0 if k == 0 else 0.0)[1] for k in range(P)]
    sc, tl = scene.Scene(), link.Link()
    LS, LL = scene.lib(), link.lib()
    bufs = [torch.empty((nm, nb * N), dtype=torch.float32, device=dev) for _ in range(P)]
    out = torch.empty((nm, nb * N), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def transmit(k, buf):
        rc = LL.uc_link_transmit(tl._h, vp(text), text.shape[1], vp(params[k]), nm, C.c_void_p(buf.data_ptr()), link.DTYPE_F32, FS, 0,
                                 nb * N, 0, 1, stream)
        if rc:
            raise RuntimeError(LL.uc_link_last_error().decode())

    def composition():
        for k in range(P):
            transmit(k, bufs[k])
        for k in range(1, P):
            bufs[0].add_(bufs[k])

    def render(packed):
        t, tlen, p, m = packed
        rc = LS.uc_scene_render(sc._h, vp(t), t.shape[1], vp(tlen), len(tlen), vp(p), len(p), vp(m), nm, C.c_void_p(out.data_ptr()),
                                link.DTYPE_F32, FS, 0, nb * N, 0, 1, stream)
        if rc:
            raise RuntimeError(LS.uc_scene_last_error().decode())

    variants = {"composition_p4": composition, "scene_p4": lambda: render(packed4), "link_p1": lambda: transmit(0, bufs[1]),
                "scene_p1": lambda: render(packed1)}

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

    # the two ways give the same buffer up to the order of the float additions (and P = 1 the same bits)
    composition()
    render(packed4)
    torch.cuda.synchronize()
    d4 = float((out[::64] - bufs[0][::64]).abs().max())
    transmit(0, bufs[1])
    render(packed1)
    torch.cuda.synchronize()
    same1 = bool(torch.equal(out[::64], bufs[1][::64]))
    # clock ramp before anything is timed
    t0 = time.time()
    while time.time() - t0 < 0.3:
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    t_short = timed(lambda: render(short4))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    nbytes = nm * nb * N * 4
    res = {"shape": [nm, nb * N], "paths": P, "bytes": nbytes, "ms": med,
           "ratio_composition_over_scene_p4": med["composition_p4"] / med["scene_p4"],
           "ratio_scene_over_link_p1": med["scene_p1"] / med["link_p1"],
           "ms_all": {k: [round(t, 3) for t in v] for k, v in ts.items()},
           "scene_p4_bytes_per_s": nbytes / (med["scene_p4"] * 1e-3),
           "scene_p4_fraction_of_8TBps_pin": nbytes / (med["scene_p4"] * 1e-3) / HBM_PEAK,
           "scene_p4_fraction_of_6TBps_write": nbytes / (med["scene_p4"] * 1e-3) / HBM_WRITE,
           "scene_p4_path_samples_per_s": P * nm * nb * N / (med["scene_p4"] * 1e-3),
           "check": {"max_abs_scene_minus_composition_p4_on_64_rows": d4, "scene_p1_equals_link_bits_on_64_rows": same1},
           "side": {"timed": "once after the alternated section, not alternated", "scene_p4_one_byte_message_ms": float(np.median(t_short))}}
    print(json.dumps(res))
    if med["scene_p4"] >= med["composition_p4"]:
        print("FAIL: the one-pass render (%.3f ms) does not beat the composition (%.3f ms)" % (med["scene_p4"], med["composition_p4"]))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
