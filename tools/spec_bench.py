"""uc_spec_run against a torch composition on the same buffer and against the read rate of tools/libhbm_probe.so, same
process: 4096 rows x 2 s at 78 125 Hz (156 250 float samples a row), magnitude spectra with the default Hann window.
  spec_a        1 uc_spec_run call, hop 2048, bins 0 .. 1023: 8 KB read and 4 KB written per frame
  spec_b        1 uc_spec_run call, hop 512, bins 300 .. 519 (the receivers' band): the output is no longer the larger stream
  torch_a/_b    the torch composition of the same frames: unfold x window -> torch.fft.rfft -> abs (-> the bin slice), on
                `comp_rows` rows (default 512) and scaled to all rows; whole frames only
  probe         hbm_probe_read over the input buffer (a read-only stream: the achievable read rate)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, frames per second, the algorithmic bytes (every input sample once -- the
overlap of (b) is expected from the caches -- plus 4 B per stored bin) over time as a fraction of the probe's rate, and the
static instruction counts of the kernel by class (whole kernel, every path, from the library's code object; one frame is
one pass of the loop).  Nothing is asserted: it is a record.
Usage: python tools/spec_bench.py [rows=4096] [seconds=2] [iters=5] [comp_rows=512]
       python tools/spec_bench.py profile [rows] [seconds] [iters]     (only the uc_spec_run calls of (a): the program to put
       behind `rocprofv3 --kernel-trace --stats --` or behind a separate `rocprofv3 --pmc <counters> --`)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FS = 78125
N = 2048
SHAPES = {"a": dict(hop=2048, bin_first=0, n_bins=1024), "b": dict(hop=512, bin_first=300, n_bins=220)}


def main():
    import torch
    from uchirp import spec
    from isa_counts import instruction_counts
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"      # the target of a profiler: the calls of (a) alone
    args = sys.argv[2:] if profile else sys.argv[1:]
    nr = int(args[0]) if len(args) > 0 else 4096
    seconds = float(args[1]) if len(args) > 1 else 2.0
    iters = int(args[2]) if len(args) > 2 else 5
    comp_rows = min(nr, int(args[3]) if len(args) > 3 else 512)
    n_in = int(round(seconds * FS))
    dev = torch.device("cuda:0")
    an = spec.Analyser(0)
    x = torch.randn((nr, n_in), dtype=torch.float32, device=dev) * 1000.0
    window = torch.from_numpy(spec.hann(N)).to(dev)
    outs = {k: an.spectra(x, **kw) for k, kw in SHAPES.items()}

    def run(k):
        an.spectra(x, out=outs[k], **SHAPES[k])

    if profile:
        for _ in range(iters):
            run("a")
        torch.cuda.synchronize()
        print("profile target: %d uc_spec_run calls, %d rows x %d float samples -> %d frames each" % (iters, nr, n_in, outs["a"].shape[1]))
        return 0

    whole = {k: (n_in - N) // kw["hop"] + 1 for k, kw in SHAPES.items()}      # the frames unfold makes: whole ones
    refs = {}

    def composition(k):
        kw = SHAPES[k]
        f = x[:comp_rows].unfold(1, N, kw["hop"]) * window
        refs[k] = torch.fft.rfft(f, dim=2).abs()[:, :, kw["bin_first"]:kw["bin_first"] + kw["n_bins"]]

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if os.path.exists(ppath):
        P = C.CDLL(ppath)
        P.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        probe = lambda: P.hbm_probe_read(x.data_ptr(), x.numel() * 4, sink.data_ptr(), blocks, stream.value)   # noqa: E731

    variants = {"spec_a": lambda: run("a"), "torch_a": lambda: composition("a"), "spec_b": lambda: run("b"), "torch_b": lambda: composition("b")}
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

    check = {}
    for k in SHAPES:
        run(k)
        composition(k)
        torch.cuda.synchronize()
        d = (outs[k][:comp_rows, :whole[k]] - refs[k]).abs().max()
        check[k] = {"max_abs_spec_minus_torch": float(d), "peak": float(refs[k].max())}
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run("a")
        if probe:
            probe()
        torch.cuda.synchronize()
    ts = {k_: [] for k_ in variants}
    for _ in range(3):
        for k_, fn in variants.items():
            ts[k_] += timed(fn)
    med = {k_: float(np.median(v)) for k_, v in ts.items()}
    res = {"rows": nr, "n_in": n_in, "ms": med, "ms_all": {k_: [round(t, 3) for t in v] for k_, v in ts.items()}, "composition_rows": comp_rows,
           "check": check, "instructions_static_whole_kernel": instruction_counts(spec.LIB_PATH, "spec_kernel")}
    prate = x.numel() * 4 / (med["probe_read"] * 1e-3) if probe else None
    if probe:
        res["probe_read_bytes_per_s"] = prate
    for k, kw in SHAPES.items():
        frames = nr * int(outs[k].shape[1])
        sec = med["spec_" + k] * 1e-3
        alg = 4 * nr * n_in + 4 * frames * kw["n_bins"]
        comp_scaled = med["torch_" + k] * nr / comp_rows * outs[k].shape[1] / whole[k]
        res[k] = {"hop": kw["hop"], "bins": [kw["bin_first"], kw["bin_first"] + kw["n_bins"] - 1], "frames": frames, "frames_per_s": frames / sec,
                  "algorithmic_bytes": alg, "algorithmic_bytes_per_s": alg / sec, "bytes_loaded_by_the_kernel": 4 * N * frames + 4 * frames * kw["n_bins"],
                  "torch_ms_scaled_to_all_rows_and_frames": comp_scaled, "ratio_torch_over_spec": comp_scaled / med["spec_" + k]}
        if probe:
            res[k]["algorithmic_fraction_of_probe_read"] = alg / sec / prate
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
