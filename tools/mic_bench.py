"""uc_mic_modulate timed: one receiver block (2048 samples, 26.2 ms of sound) of 65 536 and of 4 096 microphones, float input
(scale 1) and DFSDM words, into the PDM words the receivers read.
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports, per variant: ms per block, bit-steps per second, the block's share of the 26.2 ms it lasts;
the issue floor -- the vector instructions per bit-step of the kernel's listing (static count of the whole kernel over the
672 bit-step bodies it holds: a little above the loop's own figure of 8, the quantiser and the addresses included) times the
4 cycles one wave alone on a SIMD needs per vector instruction, at the shader clock the SMU reported while the timed region
ran (bench_telemetry.PowerSampler; "not measured" where the files are not readable, and then 2.4 GHz is assumed and
labelled); the algorithmic bytes (4 B read and 4 B written per sample) over time; and, for context only, the one-core rate of
the oracle's test helper uco.pdm_modulate (floating point, other arithmetic: no pass mark).  Before anything is timed the
first 64 samples of 130 rows are compared with the integer model.  Nothing else is asserted: it is a record.
Usage: python tools/mic_bench.py [iters=5]
       python tools/mic_bench.py profile [iters] [rows=65536]   (only the float calls of one shape: the program to put behind
       `rocprofv3 --kernel-trace --stats --` or behind a separate `rocprofv3 --kernel-trace --pmc FETCH_SIZE --` / `WRITE_SIZE`)"""
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
BODIES = (16 + 4 + 1) * 32     # bit-steps in the kernel's listing: the 16 samples of a tile, the four of a group, the tail's one
CYCLES_ALONE = 4               # per vector instruction, one wave alone on its SIMD (2 when two waves share it)
SIMDS = 1024


def main():
    import torch
    from uchirp import mic
    from isa_counts import instruction_counts
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
    args = sys.argv[2:] if profile else sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 5
    dev = torch.device("cuda:0")
    m = mic.Mic(1.0, 0)
    rng = np.random.default_rng(18)
    shapes = (int(args[1]),) if profile and len(args) > 1 else SHAPES
    data = {}
    for nr in shapes:
        f = (torch.rand((nr, N), dtype=torch.float32, device=dev) * 2.0 - 1.0) * float(mic.Q_MAX)
        w = f.to(torch.int32) * 256
        data[nr] = {"f32": f, "i32": w, "out": torch.empty((nr, N), dtype=torch.int32, device=dev), "state": m.new_state(nr)}

    def run(nr, fmt):
        d = data[nr]
        m.modulate(d[fmt], state=d["state"], out=d["out"])

    if profile:
        for _ in range(iters):
            run(shapes[0], "f32")
        torch.cuda.synchronize()
        print("profile target: %d uc_mic_modulate calls, %d rows x %d float samples: %d B read and %d B written by the algorithm each"
              % (iters, shapes[0], N, 4 * shapes[0] * N, 4 * shapes[0] * N))
        return 0

    # the bits first: 130 rows of the largest shape against the integer model
    nr0 = SHAPES[0]
    for fmt in ("f32", "i32"):
        got, st = m.modulate(data[nr0][fmt][:130, :64])
        x = data[nr0][fmt][:130, :64].cpu().numpy()
        want, want_st = mic.model(mic.quantise_model(x))
        if not (np.array_equal(got.cpu().numpy().view(np.uint32), want) and np.array_equal(st.cpu().numpy(), want_st)):
            print("mic_bench: the %s words differ from the model" % fmt)
            return 1

    variants = {"%d_%s" % (nr, fmt): (lambda nr=nr, fmt=fmt: run(nr, fmt)) for nr in SHAPES for fmt in ("f32", "i32")}

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
        run(nr0, "f32")
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
    counts = instruction_counts(mic.LIB_PATH, "mic_kernel") or {}
    res = {"samples_per_row": N, "block_ms_of_sound": BLOCK_MS, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "smu": smu, "instructions_static_whole_kernel": counts}
    for nr in SHAPES:
        for fmt in ("f32", "i32"):
            k = "%d_%s" % (nr, fmt)
            sec = med[k] * 1e-3
            steps = nr * N * 32
            r = {"rows": nr, "ms_per_block": med[k], "bit_steps_per_s": steps / sec, "share_of_the_block_s_26_2_ms": med[k] / BLOCK_MS,
                 "algorithmic_bytes": 8 * nr * N, "algorithmic_bytes_per_s": 8 * nr * N / sec, "waves": -(-nr // 64),
                 "waves_per_simd": -(-nr // 64) / SIMDS}
            name = [c for c in counts if ("ILi1E" if fmt == "f32" else "ILi0E") in c]
            if name:
                c = counts[name[0]]
                valu = (c.get("valu_other", 0) + c.get("valu_fma", 0)) / BODIES
                serial = -(-(-(-nr // 64)) // SIMDS)                  # waves that one SIMD runs: 1 up to 65 536 rows
                floor_ms = serial * N * 32 * valu * (CYCLES_ALONE if serial == 1 else 2) / (ghz * 1e9) * 1e3
                r.update({"valu_per_bit_step_static": valu, "issue_floor_ms": floor_ms, "floor_over_measured": floor_ms / med[k]})
            res[k] = r
    # for context: the oracle's helper on one core (float arithmetic of its own: not the same bits)
    try:
        from oracle import uco
        x = (rng.uniform(-0.5, 0.5, size=32 * N * 16)).astype(np.float32)
        uco.pdm_modulate(x[:32 * N])
        c0 = time.perf_counter()
        uco.pdm_modulate(x)
        c1 = time.perf_counter()
        res["oracle_pdm_modulate_one_core_bit_steps_per_s"] = x.size / (c1 - c0)
    except Exception as ex:                                           # (the oracle is test infrastructure: it may not be built)
        res["oracle_pdm_modulate_one_core_bit_steps_per_s"] = "not measured: %s" % ex
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
