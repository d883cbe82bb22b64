"""uc_retime_rows against a torch composition on the same buffer and against the read rate of tools/libhbm_probe.so, same
process: 4096 rows x 176 blocks of 2048 float samples (5.9 GB in, 5.9 GB out), one line per row, slopes uniform in +-50 ppm,
delays uniform in +-40 samples.
  composition   per chunk of 64 rows: the positions in int64, the table rows gathered and blended (T[q] + mu D[q]), 16
                gathers of the input and 16 multiply-adds (interior samples only).  Run on `comp_rows` rows (default 256) and
                scaled to all rows: it needs 80 bytes of temporaries per sample
  retime        1 uc_retime_rows call
  probe         hbm_probe_read over the input buffer (a read-only stream: the achievable read rate)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, samples per second, the algorithmic bytes (4 B read + 4 B written per
sample) over time as a fraction of the probe's rate, and the static instruction counts of the kernel by class (whole kernel,
every path, from the library's code object).  Nothing is asserted: it is a record.
Usage: python tools/retime_bench.py [rows=4096] [blocks=176] [iters=5] [comp_rows=256] [ppm=50]
       python tools/retime_bench.py profile [rows] [blocks] [iters]     (only the retime calls: the program to put behind
       `rocprofv3 --kernel-trace --stats --` or behind a separate `rocprofv3 --kernel-trace --pmc <counters> --`)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, EDGE, CHUNK = 2048, 128, 64


def main():
    import torch
    from uchirp import retime
    from isa_counts import instruction_counts
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"      # the target of a profiler: the retime calls alone
    args = sys.argv[2:] if profile else sys.argv[1:]
    nr = int(args[0]) if len(args) > 0 else 4096
    nblk = int(args[1]) if len(args) > 1 else 176
    iters = int(args[2]) if len(args) > 2 else 5
    comp_rows = min(nr, int(args[3]) if len(args) > 3 else 256)
    ppm = float(args[4]) if len(args) > 4 else 50.0
    n = nblk * N
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x = torch.empty((nr, n), dtype=torch.float32, device=dev).normal_(0.0, 1000.0)
    lines = [(r, float(rng.uniform(-40.0, 40.0)), float(rng.uniform(-ppm, ppm)) * 1e-6) for r in range(nr)]
    packed = retime.pack(lines)
    rt = retime.Retimer()
    L = retime.lib()
    out = torch.empty((nr, n), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run():
        rc = L.uc_retime_rows(rt._h, C.c_void_p(x.data_ptr()), retime.DTYPE_F32, nr, 0, n, 0, packed.ctypes.data_as(C.c_void_p), nr,
                              C.c_void_p(out.data_ptr()), 0, n, 0, stream)
        if rc:
            raise RuntimeError(L.uc_retime_last_error().decode())

    if profile:
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        print("profile target: %d uc_retime_rows calls, %d rows x %d samples, slopes in +-%g ppm" % (iters, nr, n, ppm))
        return 0

    T = torch.from_numpy(retime.table().copy()).to(dev)
    D = T[1:] - T[:-1]
    fx = np.array([retime.fixed(d, s) for (_, d, s) in lines[:comp_rows]], np.int64)
    lead = torch.from_numpy(fx[:, 0].copy()).to(dev)[:, None]
    drift = torch.from_numpy(fx[:, 1].copy()).to(dev)[:, None]
    j = torch.arange(EDGE, n - EDGE, dtype=torch.int64, device=dev)[None, :]
    ref = torch.zeros((comp_rows, n), dtype=torch.float32, device=dev)

    def composition():
        for a in range(0, comp_rows, CHUNK):
            b = min(a + CHUNK, comp_rows)
            off = lead[a:b] + j * drift[a:b]
            frac = off & 0xFFFFFFFF
            q = frac >> 24
            mu = (frac & 0xFFFFFF).to(torch.float32) * 2.0 ** -24
            idx = j + (off >> 32) - 7
            acc = None
            for t in range(16):
                c = torch.addcmul(T[:, t][q], mu, D[:, t][q])
                v = c * torch.gather(x[a:b], 1, idx + t)
                acc = v if acc is None else acc + v
            ref[a:b, EDGE:n - EDGE] = acc

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        P = C.CDLL(ppath)
        P.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        probe = lambda: P.hbm_probe_read(x.data_ptr(), x.numel() * 4, sink.data_ptr(), blocks, stream.value)   # noqa: E731

    variants = {"retime": run, "composition": composition}
    if probe:
        variants["probe_read"] = probe

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

    run()
    composition()
    torch.cuda.synchronize()
    diff = float((out[:comp_rows, EDGE:n - EDGE] - ref[:, EDGE:n - EDGE]).abs().max())
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run()
        if probe:
            probe()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    samples = nr * n
    alg_bytes = 8 * samples
    comp_scaled = med["composition"] * nr / comp_rows
    counts = instruction_counts(retime.LIB_PATH, "retime_kernel")
    res = {"input": [nr, n], "slopes_ppm": ppm, "ms": med, "ms_all": {k: [round(t, 3) for t in v] for k, v in ts.items()},
           "samples": samples, "retime_samples_per_s": samples / (med["retime"] * 1e-3),
           "algorithmic_bytes": alg_bytes, "retime_algorithmic_bytes_per_s": alg_bytes / (med["retime"] * 1e-3),
           "composition_rows": comp_rows, "composition_ms_scaled_to_all_rows": comp_scaled,
           "ratio_composition_over_retime": comp_scaled / med["retime"],
           "check": {"max_abs_retime_minus_composition": diff, "input_sigma": 1000.0},
           "instructions_static_whole_kernel": counts}
    if probe:
        rate = x.numel() * 4 / (med["probe_read"] * 1e-3)
        res["probe_read_bytes_per_s"] = rate
        res["retime_algorithmic_fraction_of_probe_read"] = res["retime_algorithmic_bytes_per_s"] / rate
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
