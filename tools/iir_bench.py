"""uc_iir_run timed: one receiver block (2048 samples, 26.2 ms of sound) of 65 536 and of 4 096 rows through cascades of 1, 7
and 8 sections (a DC blocker, the reference's Butterworth low-pass, a 16-19 kHz band-pass of order 8), float input and DFSDM
words, one coefficient set, no row_map: the tiled path.
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports, per variant: ms per block, section-samples per second, the block's share of the 26.2 ms it
lasts; the issue floor -- the vector instructions per sample of the kernel's listing (static count of the whole kernel over
the 9 sample bodies it holds: the four of the tile loop's group, the four of the direct group, the tail's one; the input rule,
the addresses and the tile moves included, so a little above 9 per section) times the 4 cycles one wave alone on a SIMD needs
per vector instruction, at the shader clock the SMU reported while the timed region ran (bench_telemetry.PowerSampler; "not
measured" where the files are not readable, and then 2.4 GHz is assumed and labelled); and the algorithmic bytes (4 B read and
4 B written per sample) over time.  Before anything is timed the first 64 samples of 130 rows of every variant are compared
with the float32 definition.  Nothing else is asserted: it is a record.
Usage: python tools/iir_bench.py [iters=5]
       python tools/iir_bench.py profile [iters] [rows=65536] [sections=7]   (only the float calls of one shape: the program to
       put behind `rocprofv3 --kernel-trace --stats --` or behind a separate counter run)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ultrasonic-communication_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

N = 2048
BLOCK_MS = N / 78125.0 * 1e3
SHAPES = (65536, 4096)
COUNTS = (1, 7, 8)
BODIES = 4 + 4 + 1             # sample bodies in the kernel's listing: the tile loop's group, the direct group, the tail
CYCLES_ALONE = 4               # per vector instruction, one wave alone on its SIMD (2 when two waves share it)
SIMDS = 1024


def cascades(iir):
    return {1: iir.dc_block_sections(78125.0, 200.0), 7: iir.lpf_sections(44100.0, 3000.0), 8: iir.bandpass_sections(78125.0, 16000.0, 19000.0, 8)}


def main():
    import torch
    from uchirp import iir
    from isa_counts import instruction_counts
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
    args = sys.argv[2:] if profile else sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 5
    dev = torch.device("cuda:0")
    sets = cascades(iir)
    counts = (int(args[2]),) if profile and len(args) > 2 else COUNTS
    shapes = (int(args[1]),) if profile and len(args) > 1 else SHAPES
    objs = {c: iir.Iir(sets[c], 0) for c in counts}
    data = {}
    for nr in shapes:
        f = torch.randn((nr, N), dtype=torch.float32, device=dev) * 20000.0
        w = f.round().to(torch.int32) * 256
        data[nr] = {"f32": f, "i32": w, "out": torch.empty((nr, N), dtype=torch.float32, device=dev), "state": objs[counts[0]].new_state(nr)}

    def run(nr, c, fmt):
        d = data[nr]
        objs[c].run(d[fmt], state=d["state"], out=d["out"])

    if profile:
        for _ in range(iters):
            run(shapes[0], counts[0], "f32")
        torch.cuda.synchronize()
        print("profile target: %d uc_iir_run calls, %d rows x %d float samples, %d sections: %d B read and %d B written by the algorithm each"
              % (iters, shapes[0], N, counts[0], 4 * shapes[0] * N, 4 * shapes[0] * N))
        return 0

    # the bits first: 130 rows of the largest shape against the float32 definition
    nr0 = SHAPES[0]
    for c in COUNTS:
        for fmt in ("f32", "i32"):
            x = data[nr0][fmt][:130, :64]
            got, st = objs[c].run(x)
            want, want_st = iir.emulate32(sets[c], x.cpu().numpy())
            if not (np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and
                    np.array_equal(st.cpu().numpy().view(np.uint32), want_st.view(np.uint32))):
                print("iir_bench: %d sections, %s: the floats differ from the definition" % (c, fmt))
                return 1

    variants = {"%d_%d_%s" % (nr, c, fmt): (lambda nr=nr, c=c, fmt=fmt: run(nr, c, fmt)) for nr in SHAPES for c in COUNTS for fmt in ("f32", "i32")}

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

    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run(nr0, 7, "f32")
        torch.cuda.synchronize()
    from bench_telemetry import PowerSampler
    sampler = PowerSampler(torch, dev)
    sampler.start()
    ts = {k: [] for k in variants}
    p0 = time.perf_counter()
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    p1 = time.perf_counter()
    smu = sampler.stop(p0, p1)
    mhz = smu.get("sclk_MHz_smu_mean") if smu else None
    ghz = mhz / 1e3 if mhz else 2.4
    med = {k: float(np.median(v)) for k, v in ts.items()}
    listing = instruction_counts(iir.LIB_PATH, "iir_kernel") or {}
    res = {"samples_per_row": N, "block_ms_of_sound": BLOCK_MS, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "smu": smu}
    for nr in SHAPES:
        for c in COUNTS:
            for fmt in ("f32", "i32"):
                k = "%d_%d_%s" % (nr, c, fmt)
                sec = med[k] * 1e-3
                r = {"rows": nr, "sections": c, "ms_per_block": med[k], "section_samples_per_s": nr * N * c / sec,
                     "share_of_the_block_s_26_2_ms": med[k] / BLOCK_MS, "algorithmic_bytes": 8 * nr * N, "algorithmic_bytes_per_s": 8 * nr * N / sec,
                     "waves": -(-nr // 64), "waves_per_simd": -(-nr // 64) / SIMDS}
                name = [n for n in listing if ("ILi1ELi%dEE" if fmt == "f32" else "ILi0ELi%dEE") % c in n]
                if name:
                    cl = listing[name[0]]
                    valu = (cl.get("valu_other", 0) + cl.get("valu_fma", 0)) / BODIES
                    serial = -(-(-(-nr // 64)) // SIMDS)                  # waves that one SIMD runs: 1 up to 65 536 rows
                    floor_ms = serial * N * valu * (CYCLES_ALONE if serial == 1 else 2) / (ghz * 1e9) * 1e3
                    r.update({"instructions_static_whole_kernel": cl, "valu_per_sample_static": valu, "issue_floor_ms": floor_ms,
                              "floor_over_measured": floor_ms / med[k]})
                res[k] = r
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
