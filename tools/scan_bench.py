"""uc_scan_power timed: one receiver block (2048 samples, 26.2 ms of sound) of 64 arrays of 8 microphones scanned over 1024 and
4096 candidate delay vectors (delays 0 .. 16 samples), float input and DFSDM words, and the same work as 1 array x 65 536 beams;
powers and best records written.  Beside it the composition the scanner replaces, in the same process and alternated with it:
Array.combine of the same taps into a buffer of n_beams x 2048 floats, then a torch square-and-sum per beam (timed for the
65 536-beam shapes in float: 64 x 1024 and 1 x 65 536).
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports, per variant: ms by the events (the two launches of a call, power and best; no profiler ran,
so the kernels' own times are NOT separated from the gap between them), ms by the host's clock from the call to the end of a
synchronise (the call's time), tap-samples per second, the block's share of the 26.2 ms it lasts, and the issue floor: a lane
holds 4 samples, a tap is 16 multiply-adds a sample, so 32 packed multiply-adds (v_pk_mul_f32 / v_pk_fma_f32) per lane and
tap, 4 cycles each on a SIMD, 1024 SIMDs, at the shader clock the SMU reported while the timed region ran
(bench_telemetry.PowerSampler; "not measured" where the files are not readable, and then 2.4 GHz is assumed and labelled).
The floor counts the multiply-adds alone; the kernel's static instruction mix (tools/isa_counts.py) is printed next to it.
Before anything is timed every shape's first 3 beams of array 0 are compared with uc_scan_power_row.  Asserted: the bits, and
that every shape is scanned in less than the 26.2 ms the block lasts.
NOT measured here: the direct path (no beam of these sets takes it), windows longer than a block, more than 8 taps.
Usage: python tools/scan_bench.py [iters=5]"""
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
MICS = 8
SHAPES = ((64, 1024), (64, 4096), (1, 65536))       # (arrays, beams)
YARDSTICK = ((64, 1024), (1, 65536))
PK_PER_LANE_TAP = 32           # 4 samples x 16 multiply-adds, two to a packed instruction
CYCLES = 4                     # per packed instruction of one wave on its SIMD
SIMDS = 1024


def main():
    import torch
    from uchirp import array, scan
    from isa_counts import instruction_counts
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    mics, wt = np.arange(MICS), np.full(MICS, 1.0 / MICS, np.float32)
    data, objs, sets = {}, {}, {}
    for na, nb in SHAPES:
        f = torch.randn((na * MICS, N), dtype=torch.float32, device=dev) * 20000.0
        data[(na, nb)] = {"f32": f, "i32": f.round().to(torch.int32) * 256, "power": torch.empty((na, 1, nb), dtype=torch.float64, device=dev)}
        sets[(na, nb)] = rng.uniform(0.0, 16.0, size=(nb, MICS))
        objs[(na, nb)] = scan.Scanner(0)
        objs[(na, nb)].set_beams(mics, wt, sets[(na, nb)])
        if objs[(na, nb)].direct_beams():
            print("scan_bench: %d beams of %r on the direct path" % (objs[(na, nb)].direct_beams(), (na, nb)))
            return 1

    def run(shape, fmt):
        return objs[shape].power(data[shape][fmt], 0, N, n_arrays=shape[0], power=data[shape]["power"])

    # the bits first
    for shape in SHAPES:
        q = scan.quantise_model(sets[shape][:3])
        for fmt in ("f32", "i32"):
            p, _ = run(shape, fmt)
            xh = data[shape][fmt][:MICS].cpu().numpy()
            want = np.array([scan.power_row(xh, mics, wt, q[b], 0, N) for b in range(3)])
            if not np.array_equal(p[0, 0, :3].cpu().numpy().view(np.uint64), want.view(np.uint64)):
                print("scan_bench: %r, %s: the powers differ from the definition" % (shape, fmt))
                return 1

    # the composition: the same taps through the array combiner, then square and add
    ar = array.Array(0)
    comp = {}
    for na, nb in YARDSTICK:
        beams = [[(a * MICS + m, float(wt[m]), float(sets[(na, nb)][b, m])) for m in range(MICS)] for a in range(na) for b in range(nb)]
        comp[(na, nb)] = {"packed": array.pack(beams), "out": torch.empty((na * nb, N), dtype=torch.float32, device=dev)}

    def compose(shape):
        c = comp[shape]
        y = ar.combine_packed(data[shape]["f32"], *c["packed"], out=c["out"])
        return (y * y).sum(dim=1, dtype=torch.float64)

    variants = {"scan_%dx%d_%s" % (na, nb, fmt): (lambda s=(na, nb), fmt=fmt: run(s, fmt)) for na, nb in SHAPES for fmt in ("f32", "i32")}
    variants.update({"composition_%dx%d_f32" % s: (lambda s=s: compose(s)) for s in YARDSTICK})

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev, wall = [], []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        return ev, wall

    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run(SHAPES[1], "f32")
        torch.cuda.synchronize()
    from bench_telemetry import PowerSampler
    sampler = PowerSampler(torch, dev)
    sampler.start()
    ev, wall = {k: [] for k in variants}, {k: [] for k in variants}
    p0 = time.perf_counter()
    for _ in range(3):
        for k, fn in variants.items():
            e, w = timed(fn)
            ev[k] += e
            wall[k] += w
    p1 = time.perf_counter()
    smu = sampler.stop(p0, p1)
    mhz = smu.get("sclk_MHz_smu_mean") if smu else None
    ghz = mhz / 1e3 if mhz else 2.4
    med = {k: float(np.median(v)) for k, v in ev.items()}
    med_wall = {k: float(np.median(v)) for k, v in wall.items()}
    listing = instruction_counts(scan.LIB_PATH, "scan_kernel") or {}
    res = {"samples_per_row": N, "block_ms_of_sound": BLOCK_MS, "microphones": MICS, "ms_events": med, "ms_call_wall": med_wall,
           "ms_events_all": {k: [round(t, 4) for t in v] for k, v in ev.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "smu": smu, "instructions_static_whole_kernel": {k: v for k, v in listing.items() if "ILi1ELi8EE" in k},
           "not_measured": ["the direct path", "windows longer than a block", "more than 8 taps", "the kernels' own times apart from the call's events"]}
    late = []
    for na, nb in SHAPES:
        tap_samples = na * nb * N * MICS
        floor_ms = tap_samples / 256.0 * PK_PER_LANE_TAP * CYCLES / SIMDS / (ghz * 1e9) * 1e3
        for fmt in ("f32", "i32"):
            k = "scan_%dx%d_%s" % (na, nb, fmt)
            r = {"arrays": na, "beams": nb, "ms_events": med[k], "ms_call_wall": med_wall[k], "tap_samples_per_s": tap_samples / (med[k] * 1e-3),
                 "share_of_the_block_s_26_2_ms": med_wall[k] / BLOCK_MS, "issue_floor_ms": floor_ms, "floor_over_measured": floor_ms / med[k],
                 "bytes_written": na * nb * 8 + na * 16}
            ck = "composition_%dx%d_f32" % (na, nb)
            if fmt == "f32" and ck in med:
                r.update({"composition_ms_events": med[ck], "composition_ms_call_wall": med_wall[ck], "composition_over_scan_events": med[ck] / med[k],
                          "composition_over_scan_wall": med_wall[ck] / med_wall[k], "composition_bytes_written_and_read": 2 * na * nb * N * 4})
            res[k] = r
            if med_wall[k] >= BLOCK_MS:
                late.append(k)
    print(json.dumps(res, indent=1))
    if late:
        print("scan_bench: NOT scanned within the block's 26.2 ms: %s" % ", ".join(late))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
