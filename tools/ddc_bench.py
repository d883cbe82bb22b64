"""uc_ddc_run timed: one receiver block (2048 samples, 26.2 ms of sound) of 65 536 and of 4 096 rows converted at 17.5 kHz
through 27 and 128 taps, D = 1 and 8, float input and DFSDM words, I/Q and I output: one tap set, no row_map, every row its own
phase.
HIP events around bursts of four calls of each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians; the shader clock the SMU reported while the timed region ran (bench_telemetry.PowerSampler; "not
measured" where the files are not readable, and then 2.4 GHz is assumed and labelled).  Reports, per variant: ms per block,
output-taps per second, the block's share of the 26.2 ms it lasts, and three yardsticks:
  the issue floor   from the listing's static counts: the innermost loops of the kernel that hold multiply-adds are found in
                    the code object (llvm-objdump, as tools/isa_counts.py reads it); the cheapest one per output-tap (D = 1: a floor for any
                    count of outputs a lane has) and the one a lane with a single output runs (D = 8) give the vector instructions and the LDS reads per
                    output-tap of a wave; a vector instruction takes 2 cycles of its SIMD (a packed one 4) with two or more
                    waves on it, a 8-byte LDS read of a wave 2 cycles and a 4-byte one 2 cycles of the CU's one LDS; the floor
                    is the larger of the two over the chip's 256 CUs at the clock read in the run;
  the HBM floor     the algorithmic bytes (4 B read per sample, 8 or 4 B written per output) over the rate of a device copy
                    of 512 MB measured in this process;
  torch             the same arithmetic in torch on the same GPU (float input, I/Q): x * cos, x * sin with the carrier of the
                    full phase in float32, conv1d with the flipped taps and stride D over the zero-padded rows.
Before anything is timed the first 300 samples of 130 rows of every variant are compared with the float32 definition.  One
condition is the project's own (derived, not tuned) and is printed as met or missed: the 65 536-row block, 27 taps, D = 1, I/Q
takes less than the 26.2 ms it lasts.  Nothing else is asserted: it is a record.
Usage: python tools/ddc_bench.py [iters=5]
       python tools/ddc_bench.py profile [iters] [rows=65536] [taps=27] [decim=1]   (only the float I/Q calls of one shape: the
       program to put behind `rocprofv3 --kernel-trace --stats --` or behind a separate counter run)"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ultrasonic-communication_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

N = 2048
FS = 78125.0
BLOCK_MS = N / FS * 1e3
SHAPES = (65536, 4096)
TAPS = (27, 128)
DECIMS = (1, 8)
CUS = 256
BURST = 4
LLVM = "/opt/rocm/lib/llvm/bin"


def inner_loops(lib_path, match):
    """{kernel: [counts of one innermost loop that holds multiply-adds, ...]} from the gfx950 code object: a loop is the
    instructions from the target of a backward branch to the branch, innermost where no other backward branch lies inside."""
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        return None
    work = tempfile.mkdtemp()
    try:
        lib = shutil.copy(lib_path, os.path.join(work, "lib.so"))
        subprocess.run([objdump, "--offloading", lib], check=True, cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = {}
        for f in sorted(os.listdir(work)):
            if "amdgcn" not in f:
                continue
            text = subprocess.run([objdump, "-d", os.path.join(work, f)], check=True, capture_output=True, text=True).stdout
            kernels, name = {}, None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    name = m.group(1)
                    kernels[name] = []
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\b.*?//\s*([0-9A-Fa-f]+):(.*)$", line)
                if m and name:
                    kernels[name].append((int(m.group(2), 16), m.group(1), m.group(3)))
            for k, ins in kernels.items():
                if match not in k:
                    continue
                back = []
                for at, (addr, op, rest) in enumerate(ins):
                    t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$", rest)
                    if op.startswith("s_cbranch") and t and int(t.group(1), 16) + ins[0][0] <= addr:
                        back.append((int(t.group(1), 16) + ins[0][0], addr))
                loops = []
                for lo, hi in back:
                    if any(lo <= l2 and h2 <= hi and (l2, h2) != (lo, hi) for l2, h2 in back):
                        continue
                    c = {"pk_fma": 0, "fma": 0, "valu_other": 0, "lds_b64": 0, "lds_other": 0, "salu": 0}
                    for addr, op, _ in ins:
                        if not lo <= addr <= hi:
                            continue
                        key = ("pk_fma" if op.startswith("v_pk_fma") else "fma" if op.startswith(("v_fma_f32", "v_fmac_f32")) else
                               "valu_other" if op.startswith("v_") else "lds_b64" if op.startswith("ds_read_b64") else
                               "lds_other" if op.startswith("ds_") else "salu" if op.startswith("s_") else None)
                        if key:
                            c[key] += 1
                    if c["pk_fma"] + c["fma"]:
                        loops.append(c)
                out[k] = loops
        return out
    finally:
        shutil.rmtree(work, ignore_errors=True)


def floors_of(loops, iq):
    """(cycles of a SIMD, cycles of the CU's LDS) per output-tap of a wave: of the loop that is cheapest per output-tap (a
    floor for every count of outputs a lane has: "dense") and of the loop with the fewest multiply-adds, the one a lane with
    a single output runs ("sparse")"""
    res = {}
    if not loops:
        return res
    lanes = lambda c: 2 * c["pk_fma"] + c["fma"]

    def cost(c):
        out_taps = lanes(c) / (2.0 if iq else 1.0)
        return {"loop": c, "output_taps_per_iteration": out_taps, "simd_cycles_per_output_tap": (4 * c["pk_fma"] + 2 * (c["fma"] + c["valu_other"])) / out_taps,
                "lds_cycles_per_output_tap": 2 * (c["lds_b64"] + c["lds_other"]) / out_taps}

    costs = [cost(c) for c in loops]
    res["dense"] = min(costs, key=lambda r: max(r["simd_cycles_per_output_tap"] / 4.0, r["lds_cycles_per_output_tap"]))
    res["sparse"] = cost(min(loops, key=lanes))
    return res


def main():
    import torch
    import torch.nn.functional as F
    from uchirp import ddc
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
    args = sys.argv[2:] if profile else sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 5
    dev = torch.device("cuda:0")
    shapes = (int(args[1]),) if profile and len(args) > 1 else SHAPES
    taps = (int(args[2]),) if profile and len(args) > 2 else TAPS
    decims = (int(args[3]),) if profile and len(args) > 3 else DECIMS
    sets = {t: ddc.lpf_taps(FS, 3000.0, n_taps=t) for t in taps}
    objs = {(t, d): ddc.Ddc(sets[t], d, 0) for t in taps for d in decims}
    step = ddc.step_of(17500.0, FS)
    rng = np.random.default_rng(70)
    data = {}
    for nr in shapes:
        f = torch.randn((nr, N), dtype=torch.float32, device=dev) * 20000.0
        data[nr] = {"f32": f, "i32": f.round().to(torch.int32) * 256, "y": torch.empty((nr, 2 * N), dtype=torch.float32, device=dev),
                    "state": torch.zeros((nr, ddc.STATE_WORDS), dtype=torch.float32, device=dev), "steps": np.full(nr, step, np.uint32),
                    "phases": rng.integers(0, 2 ** 32, size=nr, dtype=np.uint64).astype(np.uint32)}

    def run(nr, t, d, fmt, o):
        dd = data[nr]
        words = (N // d) * (2 if o == "iq" else 1)
        objs[(t, d)].run(dd[fmt], 0, dd["steps"], dd["phases"], state=dd["state"], out=o, y=dd["y"][:, :words])

    if profile:
        for _ in range(iters):
            run(shapes[0], taps[0], decims[0], "f32", "iq")
        torch.cuda.synchronize()
        print("profile target: %d uc_ddc_run calls, %d rows x %d float samples, %d taps, D = %d, I/Q" % (iters, shapes[0], N, taps[0], decims[0]))
        return 0

    # the bits first: 130 rows of the largest shape against the float32 definition
    nr0 = SHAPES[0]
    for t in TAPS:
        for d in DECIMS:
            for fmt in ("f32", "i32"):
                for o in ("iq", "i"):
                    dd = data[nr0]
                    x = dd[fmt][:130, :300].contiguous()
                    got, st = objs[(t, d)].run(x, 0, dd["steps"][:130], dd["phases"][:130], out=o)
                    want, want_st = ddc.emulate32(sets[t], x.cpu().numpy(), d, 0, dd["steps"][:130], dd["phases"][:130], None, o)
                    g = (torch.view_as_real(got) if o == "iq" else got).cpu().numpy().reshape(130, -1)
                    if not (np.array_equal(g.view(np.uint32), np.ascontiguousarray(want).view(np.float32).view(np.uint32).reshape(130, -1)) and
                            np.array_equal(st.cpu().numpy().view(np.uint32), want_st.view(np.uint32))):
                        print("ddc_bench: %d taps, D = %d, %s, %s: the floats differ from the definition" % (t, d, fmt, o))
                        return 1

    variants = {"%d_%d_%d_%s_%s" % (nr, t, d, fmt, o): (lambda nr=nr, t=t, d=d, fmt=fmt, o=o: run(nr, t, d, fmt, o))
                for nr in SHAPES for t in TAPS for d in DECIMS for fmt in ("f32", "i32") for o in ("iq", "i")}

    # torch: the same arithmetic (float input, I/Q), the carrier of the full phase in float32 made once outside the timed region
    ang = {nr: (torch.from_numpy(ddc.phases32(0, N, data[nr]["steps"], data[nr]["phases"]).astype(np.float64) * (2.0 * np.pi / 2.0 ** 32))).to(dev)
           for nr in (SHAPES[1],)}
    cs = {nr: (torch.cos(a).float(), torch.sin(a).float()) for nr, a in ang.items()}
    cs[SHAPES[0]] = tuple(v.repeat(SHAPES[0] // SHAPES[1], 1) for v in cs[SHAPES[1]])        # (timing only: the same work per row)
    kernels = {t: torch.from_numpy(sets[t][::-1].astype(np.float32).copy()).to(dev)[None, None, :] for t in TAPS}

    def run_torch(nr, t, d):
        x = data[nr]["f32"]
        c, s = cs[nr]
        zi = F.conv1d(F.pad(x * c, (t - 1, 0))[:, None, :], kernels[t], stride=d)
        zq = F.conv1d(F.pad(x * s, (t - 1, 0))[:, None, :], kernels[t], stride=d)
        return zi, zq

    torch_variants = {"torch_%d_%d_%d" % (nr, t, d): (lambda nr=nr, t=t, d=d: run_torch(nr, t, d)) for nr in SHAPES for t in TAPS for d in DECIMS}
    zi, _ = run_torch(SHAPES[1], 27, 1)
    got, _ = objs[(27, 1)].run(data[SHAPES[1]]["f32"], 0, data[SHAPES[1]]["steps"], data[SHAPES[1]]["phases"])
    torch_err = float((zi[:, 0, :] - got.real).abs().max() / got.real.abs().max())

    def timed(fn):
        """ms per call: BURST calls between two events, so that the host's part of a call (the copy of the row arrays into
        the staging pair) runs while the call in front of it computes"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(iters):
            a.record()
            for _ in range(BURST):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / BURST)
        return ts

    # every torch variant once before anything is timed: the first call of a shape picks and builds its convolution
    for k, fn in torch_variants.items():
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        print("warm-up %s: %.1f s" % (k, time.time() - t0), file=sys.stderr, flush=True)

    # the copy rate of this process: 512 MB read and 512 MB written
    src, dst = data[nr0]["f32"], torch.empty_like(data[nr0]["f32"])
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run(nr0, 27, 1, "f32", "iq")
        torch.cuda.synchronize()
    copy_ms = float(np.median(timed(lambda: dst.copy_(src)) + timed(lambda: dst.copy_(src))))
    copy_rate = 2.0 * src.numel() * 4 / (copy_ms * 1e-3)
    del dst
    from bench_telemetry import PowerSampler
    sampler = PowerSampler(torch, dev)
    sampler.start()
    everything = dict(variants)
    everything.update(torch_variants)
    ts = {k: [] for k in everything}
    p0 = time.perf_counter()
    for _ in range(3):
        for k, fn in everything.items():
            ts[k] += timed(fn)
    p1 = time.perf_counter()
    smu = sampler.stop(p0, p1)
    mhz = smu.get("sclk_MHz_smu_mean") if smu else None
    ghz = mhz / 1e3 if mhz else 2.4
    med = {k: float(np.median(v)) for k, v in ts.items()}
    loops = inner_loops(ddc.LIB_PATH, "ddc_kernel") or {}
    res = {"samples_per_row": N, "block_ms_of_sound": BLOCK_MS, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "smu": smu, "copy_ms_512MB": copy_ms, "copy_bytes_per_s": copy_rate, "torch_vs_library_first_check_rel_err": torch_err}
    for nr in SHAPES:
        for t in TAPS:
            for d in DECIMS:
                for fmt in ("f32", "i32"):
                    for o in ("iq", "i"):
                        k = "%d_%d_%d_%s_%s" % (nr, t, d, fmt, o)
                        sec = med[k] * 1e-3
                        outs = nr * (N // d)
                        nbytes = 4 * nr * N + (8 if o == "iq" else 4) * outs
                        r = {"rows": nr, "taps": t, "decim": d, "in": fmt, "out": o, "ms_per_block": med[k], "output_taps_per_s": outs * t / sec,
                             "share_of_the_block_s_26_2_ms": med[k] / BLOCK_MS, "algorithmic_bytes": nbytes, "hbm_floor_ms": nbytes / copy_rate * 1e3,
                             "hbm_floor_over_measured": nbytes / copy_rate * 1e3 / med[k]}
                        name = [n for n in loops if "ILi%dELi%dEE" % (1 if fmt == "f32" else 0, 0 if o == "iq" else 1) in n]
                        fl = floors_of(loops[name[0]], o == "iq").get("dense" if d == 1 else "sparse") if name else None
                        if fl:
                            waves = outs * t / 64.0                       # output-taps of a wave
                            simd = waves * fl["simd_cycles_per_output_tap"] / (4 * CUS) / (ghz * 1e9) * 1e3
                            lds = waves * fl["lds_cycles_per_output_tap"] / CUS / (ghz * 1e9) * 1e3
                            r.update({"listing": fl, "issue_floor_ms": max(simd, lds), "issue_floor_is": "LDS" if lds > simd else "VALU",
                                      "issue_floor_over_measured": max(simd, lds) / med[k]})
                        if fmt == "f32" and o == "iq":
                            r["torch_ms"] = med["torch_%d_%d_%d" % (nr, t, d)]
                            r["torch_over_library"] = r["torch_ms"] / med[k]
                        res[k] = r
    flag = res["65536_27_1_f32_iq"]
    res["condition"] = "the 65 536-row block, 27 taps, D = 1, I/Q takes %.3f ms of the %.1f ms it lasts: %s" % (
        flag["ms_per_block"], BLOCK_MS, "met" if flag["ms_per_block"] < BLOCK_MS else "MISSED")
    print(json.dumps(res, indent=1))
    print("\n%-28s %9s %9s %9s %9s %9s" % ("rows_taps_D_in_out", "ms", "issue fl.", "HBM fl.", "torch ms", "of 26.2"))
    for k in variants:
        r = res[k]
        print("%-28s %9.4f %9s %9.4f %9s %9.4f" % (k, r["ms_per_block"], "%.4f" % r["issue_floor_ms"] if "issue_floor_ms" in r else "-", r["hbm_floor_ms"],
                                                   "%.3f" % r["torch_ms"] if "torch_ms" in r else "-", r["share_of_the_block_s_26_2_ms"]))
    print(res["condition"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
