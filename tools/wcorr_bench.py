"""uc_wcorr_windows against uc_track_windows on the tracker bench's buffer, same process: 4096 microphones x 176 blocks of
2048 float samples (5.9 GB), 512 arrays of 8, every array's 7 microphones against its first (3584 pairs), L = 128, windows
of 4 blocks, hop = window (44 windows).
  HIP events (device only), correlations as doubles in both:
    track_windows     1 uc_track_windows call, correlations only (track_kernel and the sum-and-crest kernel)
    wcorr_guard0      1 uc_wcorr_windows call, weights of one, guard 0 (wcorr_kernel and its sum kernel): track_kernel's
                      segments plus 16 packed multiplies a thread and unit; the same bits
    wcorr_guard128    the same with the band weights and guard 128: L' = 256, segments of 1536 samples instead of 1792
After a clock ramp of >= 150 ms of work; the variants alternated three times with `iters` timings each; medians and spreads.
Nothing is asserted but that guard 0 with ones gives the tracker's bits: it is a record.
Usage: python tools/wcorr_bench.py [mics=4096] [blocks=176] [iters=5]
       python tools/wcorr_bench.py profile [mics] [blocks] [iters]     (only the three calls: the program to put behind
       `rocprofv3 --kernel-trace --stats --`, which times the kernels one by one)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, MICS, L, GUARD, WINDOW = 2048, 8, 128, 128, 4 * 2048


def main():
    import torch
    from uchirp import track, wcorr, xcorr
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
    args = sys.argv[2:] if profile else sys.argv[1:]
    nm = int(args[0]) if len(args) > 0 else 4096
    nblk = int(args[1]) if len(args) > 1 else 176
    iters = int(args[2]) if len(args) > 2 else 5
    n_in = nblk * N
    na = nm // MICS
    nw = n_in // WINDOW
    dev = torch.device("cuda:0")
    x = torch.empty((nm, n_in), dtype=torch.float32, device=dev).normal_(0.0, 1000.0)
    arrays = [[a * MICS + m for m in range(MICS)] for a in range(na)]
    pairs = xcorr._pairs([(a[0], m) for a in arrays for m in a[1:]])
    tr, wc = track.Tracker(), wcorr.Wcorr()
    band = wcorr.band_weights(78125.0, 16000.0, 19000.0, 1000.0, GUARD)[0]
    out_t = torch.empty((len(pairs), nw, 2 * L + 1), dtype=torch.float64, device=dev)
    out_w = torch.empty_like(out_t)

    def run_track():
        tr.windows(x, pairs, 0, WINDOW, WINDOW, nw, L, corr=out_t, crest=False)

    def run_guard0():
        wc.windows(x, pairs, 0, WINDOW, WINDOW, nw, L, 0, None, out=out_w)

    def run_guard128():
        wc.windows(x, pairs, 0, WINDOW, WINDOW, nw, L, GUARD, band, out=out_w)

    variants = {"track_windows": run_track, "wcorr_guard0": run_guard0, "wcorr_guard128": run_guard128}
    if profile:
        for _ in range(iters):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        print("profile target: %d calls each of uc_track_windows, uc_wcorr_windows (ones, guard 0) and uc_wcorr_windows (band, guard %d) at L = %d, "
              "%d microphones x %d samples, %d pairs, %d windows" % (iters, GUARD, L, nm, n_in, len(pairs), nw))
        return 0

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(iters):
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return ts

    run_track()
    run_guard0()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_t, out_w))
    run_guard128()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run_track()
        torch.cuda.synchronize()

    def segments(lp):
        s = 2048 - 2 * lp
        per = (WINDOW + s - 1) // s
        return {"samples": s, "per_window": per, "groups_per_window": (per + 3) // 4, "total": len(pairs) * nw * per}

    res = {"input": [nm, n_in], "pairs": len(pairs), "max_lag": L, "guard": GUARD, "window": WINDOW, "windows": nw,
           "guard0_ones_has_the_trackers_bits": same,
           "segments": {"guard0": segments(L), "guard128": segments(L + GUARD)}}
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += events(fn)
    res["device_ms"] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": [round(t, 3) for t in v]}
                        for k, v in ts.items()}
    base = res["device_ms"]["track_windows"]["median"]
    res["ratio_wcorr_guard0_over_track_windows"] = res["device_ms"]["wcorr_guard0"]["median"] / base
    res["ratio_wcorr_guard128_over_track_windows"] = res["device_ms"]["wcorr_guard128"]["median"] / base
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
