"""uc_align_correlate against a torch composition on the same buffer, same process: 4096 microphones x 176 blocks of 2048
float samples (5.9 GB, the array bench's buffer), 512 arrays of 8, every array's 7 microphones against its first, lags
-48 .. 48, the sums over the interior samples [L, n - L) (the composition does not pad).
  composition   per lag a shifted slice of the 7 microphones of every array, a product with the array's reference row and
                a row sum (three torch kernels per lag over all arrays at once, float32 sums)
  correlate     1 uc_align_correlate call (two kernels: the unit sums in float, their sum in double)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, multiply-adds per second, and the two floors of the call: the
multiply-adds at the chip's packed-fp32 rate, and the bytes the kernel asks the caches for (every unit stages its window of
both rows again) at the rate of a streaming read of the buffer (tools/libhbm_probe.so).  Nothing is asserted: it is a
record.
Usage: python tools/align_bench.py [mics=4096] [blocks=176] [iters=5]
       python tools/align_bench.py profile [mics] [blocks] [iters]     (only the correlate calls: the program to put behind
       `rocprofv3 --kernel-trace --stats --`, which times the two kernels alone)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, MICS, L = 2048, 8, 48
PEAK_FMA_PER_S = 157.3e12 / 2.0        # the chip's vector fp32 rate (packed), in multiply-adds


def main():
    import torch
    from uchirp import align
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"      # the target of a profiler: the correlate calls alone
    args = sys.argv[2:] if profile else sys.argv[1:]
    nm = int(args[0]) if len(args) > 0 else 4096
    nblk = int(args[1]) if len(args) > 1 else 176
    iters = int(args[2]) if len(args) > 2 else 5
    n_in = nblk * N
    first, n = L, n_in - 2 * L
    na = nm // MICS
    dev = torch.device("cuda:0")
    x = torch.empty((nm, n_in), dtype=torch.float32, device=dev).normal_(0.0, 1000.0)
    pairs = np.zeros(na * (MICS - 1), align.PAIR_DTYPE)
    pairs["ref"] = np.repeat(np.arange(na) * MICS, MICS - 1)
    pairs["mic"] = (np.arange(na)[:, None] * MICS + np.arange(1, MICS)[None, :]).ravel()
    al = align.Aligner()
    lags = 2 * L + 1
    out = torch.empty((len(pairs), lags), dtype=torch.float64, device=dev)
    ref = torch.zeros((len(pairs), lags), dtype=torch.float32, device=dev)
    xv = x.view(na, MICS, n_in)

    def correlate():
        al.correlate(x, pairs, first=first, n=n, max_lag=L, out=out)

    def composition():
        a = xv[:, 0:1, first:first + n]
        for k in range(lags):
            lag = k - L
            ref[:, k] = (a * xv[:, 1:, first + lag:first + lag + n]).sum(2).view(-1)

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        P = C.CDLL(ppath)
        P.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        probe = lambda: P.hbm_probe_read(x.data_ptr(), x.numel() * 4, sink.data_ptr(), blocks, stream)   # noqa: E731

    variants = {"correlate": correlate, "composition": composition}
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

    if profile:
        for _ in range(iters):
            correlate()
        torch.cuda.synchronize()
        print("profile target: %d uc_align_correlate calls, %d microphones x %d samples, %d pairs, lags -%d .. %d" % (iters, nm, n_in, len(pairs), L, L))
        return 0
    correlate()
    composition()
    torch.cuda.synchronize()
    scale = float(out.abs().max())
    diff = float((out - ref.double()).abs().max())
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        correlate()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    fmas = len(pairs) * n * lags
    n_blocks = (lags + 31) // 32
    fmas_issued = len(pairs) * n * n_blocks * 32          # whole blocks of 32 lags
    staged = len(pairs) * n * n_blocks * (256 + 292) / 256.0 * 4.0      # per pass of 256 samples: 256 + 292 floats
    res = {"input": [nm, n_in], "pairs": len(pairs), "max_lag": L, "first": first, "n": n, "ms": med,
           "ms_all": {k: [round(t, 3) for t in v] for k, v in ts.items()},
           "multiply_adds": fmas, "multiply_adds_issued": fmas_issued, "correlate_multiply_adds_per_s": fmas / (med["correlate"] * 1e-3),
           "ratio_composition_over_correlate": med["composition"] / med["correlate"],
           "floor_ms_packed_fma_issued": fmas_issued / PEAK_FMA_PER_S * 1e3, "staged_bytes": staged,
           "check": {"max_abs_correlate_minus_composition": diff, "max_abs_correlation": scale, "input_sigma": 1000.0}}
    if probe:
        rate = x.numel() * 4 / (med["probe_read"] * 1e-3)
        res["probe_read_bytes_per_s"] = rate
        res["floor_ms_one_read_of_the_buffer"] = med["probe_read"]
        res["staged_bytes_per_s_over_probe_read"] = staged / (med["correlate"] * 1e-3) / rate
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
