"""uc_rate_convert against a torch composition on the same buffer, against uchirp/resample.py on one row and against the
read rate of tools/libhbm_probe.so, same process: 4096 microphones x 2 s at 44.1 kHz (88 200 samples a row) to 78 125 Hz
(156 250 outputs a row, 6.4e8 in all), int16 and float input.
  composition   per chunk of 64 rows: for each of the 49 taps one index gather of the input along the row, times the tap's
                table column gathered by phase, summed in the definition's order (interior outputs only).  Run on `comp_rows`
                rows (default 256) and scaled to all rows
  convert_i16   1 uc_rate_convert call, int16 input
  convert_f32   1 uc_rate_convert call, float input
  probe         hbm_probe_read over the float input buffer (a read-only stream: the achievable read rate)
  resample      resample.resample (float64 numpy) on ONE row, wall clock: for scale
HIP events around each GPU variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with
`iters` timings each; medians.  Reports the time of each, outputs per second, the algorithmic bytes (2 or 4 B read per input
sample + 4 B written per output) over time as a fraction of the probe's rate, the multiply-adds per second against the
packed-FMA peak (157.3 TFLOP/s of f32 vector arithmetic), and the static instruction counts of the kernel by class (whole
kernel, every path, from the library's code object).  Nothing is asserted: it is a record.
Usage: python tools/rate_bench.py [rows=4096] [seconds=2] [iters=5] [comp_rows=256] [fs_in=44100]
       python tools/rate_bench.py profile [rows] [seconds] [iters]     (only the float convert calls: the program to put
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

CHUNK = 64
FMA_PEAK = 157.3e12 / 2.0        # f32 multiply-adds per second, packed


def main():
    import torch
    from uchirp import rate, resample
    from isa_counts import instruction_counts
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"      # the target of a profiler: the convert calls alone
    args = sys.argv[2:] if profile else sys.argv[1:]
    nr = int(args[0]) if len(args) > 0 else 4096
    seconds = float(args[1]) if len(args) > 1 else 2.0
    iters = int(args[2]) if len(args) > 2 else 5
    comp_rows = min(nr, int(args[3]) if len(args) > 3 else 256)
    fs_in = int(args[4]) if len(args) > 4 else 44100
    n_in = int(round(seconds * fs_in))
    dev = torch.device("cuda:0")
    cv = rate.Converter.for_rates(fs_in)
    info = cv.info
    n_out = rate.count(info, n_in)
    xi = torch.randint(-20000, 20000, (nr, n_in), dtype=torch.int16, device=dev)
    xf = xi.to(torch.float32)
    out = torch.empty((nr, n_out), dtype=torch.float32, device=dev)
    L = rate.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(x, dt):
        rc = L.uc_rate_convert(cv._h, C.c_void_p(x.data_ptr()), dt, nr, 0, n_in, 0, C.c_void_p(out.data_ptr()), 0, n_out, 0, stream)
        if rc:
            raise RuntimeError(L.uc_rate_last_error().decode())

    run_i16 = lambda: run(xi, rate.DTYPE_I16)       # noqa: E731
    run_f32 = lambda: run(xf, rate.DTYPE_F32)       # noqa: E731
    if profile:
        for _ in range(iters):
            run_f32()
        torch.cuda.synchronize()
        print("profile target: %d uc_rate_convert calls, %d rows x %d float samples -> %d outputs each" % (iters, nr, n_in, n_out))
        return 0

    table = torch.from_numpy(rate.table(info, cv.beta)).to(dev)       # [up, taps]
    edge = 2 * info.taps * info.up // info.down + 2
    m = torch.arange(edge, n_out - edge, dtype=torch.int64, device=dev)
    pos = m * info.down + info.centre
    k = pos // info.up
    ph = pos - k * info.up
    ref = torch.zeros((comp_rows, n_out), dtype=torch.float32, device=dev)

    def composition():
        for a in range(0, comp_rows, CHUNK):
            b = min(a + CHUNK, comp_rows)
            acc = None
            for j in range(info.taps - 1, -1, -1):
                v = table[:, j][ph][None, :] * xf[a:b].index_select(1, k - j)
                acc = v if acc is None else acc + v
            ref[a:b, edge:n_out - edge] = acc

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        P = C.CDLL(ppath)
        P.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        probe = lambda: P.hbm_probe_read(xf.data_ptr(), xf.numel() * 4, sink.data_ptr(), blocks, stream.value)   # noqa: E731

    variants = {"convert_i16": run_i16, "convert_f32": run_f32, "composition": composition}
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

    run_f32()
    composition()
    torch.cuda.synchronize()
    diff = float((out[:comp_rows, edge:n_out - edge] - ref[:, edge:n_out - edge]).abs().max())
    peak = float(ref.abs().max())
    one = xi[0].cpu().numpy()
    t0 = time.perf_counter()
    want = resample.resample(one, info.up, info.down, info.half, cv.beta)
    resample_s = time.perf_counter() - t0
    diff_resample = float(np.abs(out[0].cpu().numpy() - want).max())
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run_f32()
        if probe:
            probe()
        torch.cuda.synchronize()
    ts = {k_: [] for k_ in variants}
    for _ in range(3):
        for k_, fn in variants.items():
            ts[k_] += timed(fn)
    med = {k_: float(np.median(v)) for k_, v in ts.items()}
    outputs = nr * n_out
    comp_scaled = med["composition"] * nr / comp_rows
    res = {"rows": nr, "fs_in": fs_in, "ratio": [info.up, info.down], "taps": info.taps, "n_in": n_in, "n_out": n_out, "outputs": outputs,
           "tile_outputs": rate.tile_outputs(info), "ms": med, "ms_all": {k_: [round(t, 3) for t in v] for k_, v in ts.items()},
           "composition_rows": comp_rows, "composition_ms_scaled_to_all_rows": comp_scaled,
           "resample_one_row_s": resample_s, "resample_all_rows_s_scaled": resample_s * nr,
           "check": {"max_abs_convert_minus_composition": diff, "max_abs_convert_minus_resample_row0": diff_resample, "peak": peak},
           "instructions_static_whole_kernel": instruction_counts(rate.LIB_PATH, "rate_kernel")}
    for name, elem in (("convert_i16", 2), ("convert_f32", 4)):
        sec = med[name] * 1e-3
        alg = elem * nr * n_in + 4 * outputs
        res[name] = {"outputs_per_s": outputs / sec, "algorithmic_bytes": alg, "algorithmic_bytes_per_s": alg / sec,
                     "fma_per_s": outputs * info.taps / sec, "fraction_of_packed_fma_peak": outputs * info.taps / sec / FMA_PEAK,
                     "ratio_composition_over_convert": comp_scaled / med[name],
                     "ratio_resample_all_rows_over_convert": resample_s * nr / sec}
    if probe:
        prate = xf.numel() * 4 / (med["probe_read"] * 1e-3)
        res["probe_read_bytes_per_s"] = prate
        for name in ("convert_i16", "convert_f32"):
            res[name]["algorithmic_fraction_of_probe_read"] = res[name]["algorithmic_bytes_per_s"] / prate
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
