"""uc_xcorr_correlate on the array bench's buffer, same process: 4096 microphones x 176 blocks of 2048 float samples
(5.9 GB), 512 arrays of 8, every array's 7 microphones against its first (3584 pairs), the sums over the interior samples
[L, n_in - L).
  L = 48    xcorr      1 uc_xcorr_correlate call (two kernels: the unit sums by FFT in float, their sum in double)
            align      1 uc_align_correlate call on the same pairs (the direct kernel)
  L = 512   xcorr      as above
            rfft       a torch composition over the same segments: torch.fft.rfft of the zero-padded reference segments
                       and of the microphone windows (unfold), conj(A) B summed over the segments, one irfft; arrays in
                       chunks of 16 (the windows of all of them at once would not fit)
            probe_read one streaming read of the buffer (tools/libhbm_probe.so)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, segments per second, and the bytes the kernel asks the caches for
(per segment S + S + 2 L samples) against the probe's rate.  Nothing is asserted: it is a record.
Usage: python tools/xcorr_bench.py [mics=4096] [blocks=176] [iters=5]
       python tools/xcorr_bench.py profile [mics] [blocks] [iters]     (only the uc_xcorr_correlate calls at L = 48 and
       L = 512: the program to put behind `rocprofv3 --kernel-trace --stats --`, which times the two kernels alone)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, MICS, P = 2048, 8, 2048


def main():
    import torch
    from uchirp import align, xcorr
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
    args = sys.argv[2:] if profile else sys.argv[1:]
    nm = int(args[0]) if len(args) > 0 else 4096
    nblk = int(args[1]) if len(args) > 1 else 176
    iters = int(args[2]) if len(args) > 2 else 5
    n_in = nblk * N
    na = nm // MICS
    dev = torch.device("cuda:0")
    x = torch.empty((nm, n_in), dtype=torch.float32, device=dev).normal_(0.0, 1000.0)
    pairs = np.zeros(na * (MICS - 1), xcorr.PAIR_DTYPE)
    pairs["ref"] = np.repeat(np.arange(na) * MICS, MICS - 1)
    pairs["mic"] = (np.arange(na)[:, None] * MICS + np.arange(1, MICS)[None, :]).ravel()
    apairs = pairs.astype(align.PAIR_DTYPE)
    xc, al = xcorr.Xcorr(), align.Aligner()
    xv = x.view(na, MICS, n_in)
    out = {L: torch.empty((len(pairs), 2 * L + 1), dtype=torch.float64, device=dev) for L in (48, 512)}
    out_align = torch.empty((len(pairs), 97), dtype=torch.float64, device=dev)
    out_rfft = torch.zeros((len(pairs), 1025), dtype=torch.float32, device=dev)

    def run_xcorr(L):
        xc.correlate(x, pairs, first=L, n=n_in - 2 * L, max_lag=L, out=out[L])

    def run_align():
        al.correlate(x, apairs, first=48, n=n_in - 96, max_lag=48, out=out_align)

    def run_rfft(chunk=16):
        L = 512
        S = P - 2 * L
        nseg = (n_in - 2 * L) // S                      # n_in - 2 L is a whole number of segments of 1024
        for a0 in range(0, na, chunk):
            blk = xv[a0:a0 + chunk]
            A = torch.fft.rfft(blk[:, 0:1, L:L + nseg * S].reshape(-1, 1, nseg, S), n=P)
            B = torch.fft.rfft(blk[:, 1:, :(nseg - 1) * S + P].unfold(-1, P, S))
            c = torch.fft.irfft((A.conj() * B).sum(2), n=P)[..., :2 * L + 1]
            out_rfft[a0 * (MICS - 1):(a0 + blk.shape[0]) * (MICS - 1)] = c.reshape(-1, 2 * L + 1)

    if profile:
        for _ in range(iters):
            run_xcorr(48)
            run_xcorr(512)
        torch.cuda.synchronize()
        print("profile target: %d uc_xcorr_correlate calls each at L = 48 and L = 512, %d microphones x %d samples, %d pairs" % (iters, nm, n_in, len(pairs)))
        return 0

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        Pr = C.CDLL(ppath)
        Pr.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        probe = lambda: Pr.hbm_probe_read(x.data_ptr(), x.numel() * 4, sink.data_ptr(), blocks, stream)   # noqa: E731

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

    sets = {"L48": {"xcorr": lambda: run_xcorr(48), "align": run_align},
            "L512": {"xcorr": lambda: run_xcorr(512), "rfft": run_rfft}}
    if probe:
        sets["L512"]["probe_read"] = probe
    for variants in sets.values():
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    check = {"L48_max_abs_xcorr_minus_align": float((out[48] - out_align).abs().max()), "L48_max_abs_correlation": float(out_align.abs().max()),
             "L512_max_abs_xcorr_minus_rfft": float((out[512] - out_rfft.double()).abs().max()), "L512_max_abs_correlation": float(out[512].abs().max()),
             "input_sigma": 1000.0}
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run_xcorr(48)
        torch.cuda.synchronize()
    res = {"input": [nm, n_in], "pairs": len(pairs), "check": check}
    for name, variants in sets.items():
        ts = {k: [] for k in variants}
        for _ in range(3):
            for k, fn in variants.items():
                ts[k] += timed(fn)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        L = int(name[1:])
        S = P - 2 * L
        n = n_in - 2 * L
        segs = len(pairs) * ((n + S - 1) // S)
        asked = len(pairs) * (2.0 * n + 2 * L * ((n + S - 1) // S)) * 4.0
        r = {"max_lag": L, "first": L, "n": n, "ms": med, "ms_all": {k: [round(t, 3) for t in v] for k, v in ts.items()},
             "segments": segs, "xcorr_segments_per_s": segs / (med["xcorr"] * 1e-3), "bytes_asked": asked,
             "unit_sum_bytes_written": len(pairs) * ((((n + S - 1) // S) + xcorr.GROUP - 1) // xcorr.GROUP) * (2 * L + 1) * 4.0}
        if "align" in med:
            r["ratio_align_over_xcorr"] = med["align"] / med["xcorr"]
        if "rfft" in med:
            r["ratio_rfft_over_xcorr"] = med["rfft"] / med["xcorr"]
        if "probe_read" in med:
            rate = x.numel() * 4 / (med["probe_read"] * 1e-3)
            r["probe_read_bytes_per_s"] = rate
            r["bytes_asked_per_s_over_probe_read"] = asked / (med["xcorr"] * 1e-3) / rate
        res[name] = r
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
