"""uc_mf_run timed: `rows` complex rows (what uc_ddc_run writes) of `blocks` x 256 samples compressed with two templates of 256
taps in one call (2 jobs a row; S = 1791, so blocks = 176 gives 26 segments a job), in four variants:
  records      the records alone (out_dev NULL): what a caller who wants arrivals asks for
  power        the records and the stored power
  complex      the records and the stored complex outputs
  noselect     the records alone from libuchirp_mf_noselect.so (`make libuchirp_mf_noselect.so`: the same kernel with the
               four selection rounds knocked out), where that library has been built: the rounds' share of the time
and two yardsticks in the same process:
  torch        the torch composition over the same segments: unfold the windows, torch.fft.fft, times H, torch.fft.ifft,
               |.|^2, rows in chunks of 256 (the windows of all of them at once would not fit); no candidates are picked
  probe_read   one streaming read of the input (tools/libhbm_probe.so)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, ns per unit (job, segment) against the 5.0 ns DESIGN section 13 records for
one xcorr segment, and the bytes the kernel asks the caches for (2048 elements of 8 bytes per unit, and what it stores)
against the probe's rate.  Before anything is timed 4 rows are compared with the float64 model.  Nothing else is asserted:
it is a record.
Usage: python tools/mf_bench.py [rows=4096] [blocks=176] [iters=5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ultrasonic-communication_amd")):
    sys.path.insert(0, p)

TAPS = 256
XCORR_SEGMENT_NS = 5.0


def main():
    import torch
    from uchirp import mf
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 176
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda:0")
    n_in = blocks * 256
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.view_as_complex(torch.randn((rows, n_in, 2), dtype=torch.float32, device=dev, generator=g) * 700.0)
    rng = np.random.default_rng(6)
    taps = ((rng.standard_normal((2, TAPS)) + 1j * rng.standard_normal((2, TAPS))) / np.sqrt(2.0 * TAPS)).astype(np.complex64)
    jobs = np.zeros(2 * rows, mf.JOB_DTYPE)
    jobs["row"], jobs["set"] = np.repeat(np.arange(rows), 2), np.tile([0, 1], rows)
    hop, k0, ns = mf.plan(TAPS, 0, 0, n_in)
    units = 2 * rows * ns

    # the values first
    m = mf.Mf(taps, 0)
    y, _ = m.run(x[:4].contiguous(), [(0, 0), (1, 1), (2, 0), (3, 1)])
    xh = x[:4].cpu().numpy()
    want = mf.model(xh, taps, [(0, 0), (1, 1), (2, 0), (3, 1)])
    ratio = float((np.abs(y.cpu().numpy() - want) / (2.0 ** -24 * mf.bound(xh, taps, [(0, 0), (1, 1), (2, 0), (3, 1)]))).max())
    if ratio > mf.ERROR_C:
        print("mf_bench: the outputs differ from the model: %.3f of the bound's unit" % ratio)
        return 1

    out_c = torch.empty((2 * rows, n_in), dtype=torch.complex64, device=dev)
    out_p = out_c.view(torch.float32)[:, :n_in]                       # (the same memory: a float row per job inside it)
    variants = {"records": lambda: m.run(x, jobs, out=None), "power": lambda: m.run(x, jobs, out="power", y=out_p),
                "complex": lambda: m.run(x, jobs, out="complex", y=out_c)}
    knock = os.path.join(ROOT, "ultrasonic-communication_amd", "libuchirp_mf_noselect.so")
    if os.path.exists(knock):
        L = C.CDLL(knock)
        mf._declare(L)
        L.uc_mf_destroy.argtypes = [C.c_void_p]
        h = C.c_void_p()
        assert L.uc_mf_create(0, C.byref(h)) == 0 and L.uc_mf_set_templates(h, taps.ctypes.data_as(C.c_void_p), 2, TAPS) == 0
        rec = torch.empty((2 * rows, ns, 20), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        variants["noselect"] = lambda: L.uc_mf_run(h, C.c_void_p(x.data_ptr()), mf.DTYPE_C32, rows, n_in, n_in, jobs.ctypes.data_as(C.c_void_p),
                                                   2 * rows, 0, 0, n_in, None, 0, 0, C.c_void_p(rec.data_ptr()), C.c_void_p(stream))

    H = torch.from_numpy(np.stack([mf.spectrum(t) for t in taps])).to(dev)
    pad = torch.zeros((rows, TAPS + n_in + 2048), dtype=torch.complex64, device=dev)
    pad[:, TAPS:TAPS + n_in] = x

    def run_torch():
        for r0 in range(0, rows, 256):
            w = pad[r0:r0 + 256].unfold(1, 2048, hop)[:, :ns]               # [256, ns, 2048]: a_k of every segment
            A = torch.fft.fft(w)
            for s in range(2):
                z = torch.fft.ifft(A * H[s], norm="forward")[..., TAPS:TAPS + hop]
                e = z.real * z.real + z.imag * z.imag                        # noqa: F841

    variants["torch"] = run_torch
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        Pr = C.CDLL(ppath)
        Pr.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        nblk = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(nblk, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        variants["probe_read"] = lambda: Pr.hbm_probe_read(x.data_ptr(), x.numel() * 8, sink.data_ptr(), nblk, st)

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

    for fn in variants.values():                                             # everything once: plans, buffers, staging
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < 0.15:                                           # clock ramp before anything is timed
        variants["records"]()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    res = {"rows": rows, "samples_per_row": n_in, "taps": TAPS, "jobs": 2 * rows, "hop": hop, "segments_per_job": ns, "units": units,
           "check_ratio_of_the_bound_unit": ratio, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "ns_per_unit": {k: med[k] * 1e6 / units for k in med if k not in ("probe_read",)},
           "xcorr_segment_ns_design_13": XCORR_SEGMENT_NS}
    asked = units * 2048 * 8
    stored = {"records": units * 80, "power": units * 80 + 2 * rows * n_in * 4, "complex": units * 80 + 2 * rows * n_in * 8}
    res["bytes_asked_of_the_caches"] = asked
    res["bytes_stored"] = stored
    if "probe_read" in med:
        rate = x.numel() * 8 / (med["probe_read"] * 1e-3)
        res["probe_read_bytes_per_s"] = rate
        res["input_read_once_ms"] = med["probe_read"]
        res["ms_over_input_read_once"] = {k: med[k] / med["probe_read"] for k in stored}
        res["asked_bytes_at_probe_rate_ms"] = asked / rate * 1e3
    if "noselect" in med:
        res["selection_share_of_records"] = 1.0 - med["noselect"] / med["records"]
    res["torch_over_records"] = med["torch"] / med["records"]
    res["torch_over_power"] = med["torch"] / med["power"]
    print(json.dumps(res, indent=1))
    print("\n%-12s %10s %12s" % ("variant", "ms", "ns per unit"))
    for k in variants:
        print("%-12s %10.3f %12s" % (k, med[k], "%.2f" % (med[k] * 1e6 / units) if k != "probe_read" else "-"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
