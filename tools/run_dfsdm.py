#!/usr/bin/env python3
"""uc_dfsdm_run timed next to the specialised sinc^5 kernel and this chip's own copy rate, in ONE process on ONE box: one
receiver block of 65 536 rows x 2048 PDM words at SINC3 / 32 and SINC5 / 32 (the word path) and at SINC3 / 20 (the bit path),
uc_dfsdm_sinc5_streams on the same words, and tools/hbm_probe.hip's 1:1 copy (4 B in, 4 B out per word: the traffic shape of
every ratio-32 configuration; the probe the sinc5 measurement used).
HIP events around each variant after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports per variant: ms per block, its share of the 26.2 ms a block lasts, the ratio to the
specialised kernel, the copy's time over the variant's (the share of the copy floor), and the share of the issue floor: the
vector instructions per word of the kernel's listing (static count over the word bodies it holds) times the 4 cycles one wave
alone on a SIMD needs per vector instruction, at the shader clock the SMU reported while the timed region ran ("not
measured" where the files are not readable, and then 2.4 GHz is assumed and labelled).  Before anything is timed 130 rows of
each configuration are compared with uc_dfsdm_filter_row.  Nothing else is asserted: it is a record.
Usage: python tools/run_dfsdm.py [iters=5] [rows=65536]
       python tools/run_dfsdm.py profile ORDER RATIO [iters] [rows]   (only the calls of one configuration: the program to put
       behind `rocprofv3 --kernel-trace --stats --` or behind a separate `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --`)"""
import ctypes as C
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
CONFIGS = {"sinc3_32": (3, 32, 1, 2, 0), "sinc5_32": (5, 32, 1, 2, 0), "sinc3_20_bit_path": (3, 20, 1, 0, 0)}
WORD_BODIES = 4 + 1            # word steps in a word-path kernel's listing: the four of a 16-byte group, the direct tail's one
CYCLES_ALONE = 4               # per vector instruction, one wave alone on its SIMD
SIMDS = 1024


def main():
    import torch
    import uchirp
    from uchirp import dfsdm
    from isa_counts import instruction_counts
    args = sys.argv[1:]
    profile = bool(args) and args[0] == "profile"
    if profile:
        cfgs = {"profiled": (int(args[1]), int(args[2]), 1, 0, 0)}
        args = args[3:]
    else:
        cfgs = CONFIGS
    iters = int(args[0]) if len(args) > 0 else 5
    nr = int(args[1]) if len(args) > 1 else 65536
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(27)
    w = torch.randint(-(1 << 31), (1 << 31) - 1, (nr, N), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
    objs = {k: dfsdm.Dfsdm(c, 0) for k, c in cfgs.items()}
    state = {k: o.new_state(nr) for k, o in objs.items()}
    outs = {k: torch.empty((nr, dfsdm.plan(c, 0, N)), dtype=torch.int32, device=dev) for k, c in cfgs.items()}

    def run(k):
        objs[k].run(w, state=state[k], words_before=0, out=outs[k])    # (the state runs on; the time does not depend on it)

    if profile:
        for _ in range(iters):
            run("profiled")
        torch.cuda.synchronize()
        print("profile target: %d uc_dfsdm_run calls at %r, %d rows x %d words" % (iters, cfgs["profiled"], nr, N))
        return 0

    # the bits first
    host = w[:130, :64].cpu().numpy()
    for k, c in cfgs.items():
        got, st = objs[k].run(w[:130, :64])
        for r in (0, 63, 64, 129):
            o, s = dfsdm.filter_row(host[r], c)
            if not (np.array_equal(got[r].cpu().numpy(), o) and np.array_equal(st[r].cpu().numpy(), s)):
                print("run_dfsdm: %s: row %d differs from uc_dfsdm_filter_row" % (k, r))
                return 1

    e = uchirp.Engine(uchirp.RX_REAL)
    L = uchirp.lib()
    stream = torch.cuda.current_stream(dev)
    hist = torch.full((nr, 4), -1431655766, dtype=torch.int32, device=dev)
    out5 = torch.empty((nr, N), dtype=torch.int32, device=dev)
    P = C.CDLL(os.path.join(ROOT, "tools", "libhbm_probe.so"))
    P.hbm_probe_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8

    def sinc5_streams():
        rc = L.uc_dfsdm_sinc5_streams(e._h, C.c_void_p(w.data_ptr()), nr, N, 0, C.c_void_p(hist.data_ptr()), C.c_void_p(out5.data_ptr()), 0,
                                      C.c_void_p(stream.cuda_stream))
        assert rc == 0, L.uc_last_error()

    variants = {k: (lambda k=k: run(k)) for k in cfgs}
    variants["uc_dfsdm_sinc5_streams"] = sinc5_streams
    variants["copy_probe"] = lambda: P.hbm_probe_copy(w.data_ptr(), out5.data_ptr(), nr * N * 4, blocks, stream.cuda_stream)

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
        run("sinc3_32")
        torch.cuda.synchronize()
    for fn in variants.values():             # every shape once, untimed
        fn()
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
    counts = instruction_counts(dfsdm.LIB_PATH, "dfsdm_kernel") or {}
    res = {"rows": nr, "words_per_row": N, "block_ms_of_sound": BLOCK_MS, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "instructions_static_whole_kernel": counts}
    for k, c in cfgs.items():
        r = {"config": c, "ms_per_block": med[k], "share_of_the_block_s_26_2_ms": med[k] / BLOCK_MS,
             "times_the_specialised_sinc5_kernel": med[k] / med["uc_dfsdm_sinc5_streams"], "copy_probe_over_this": med["copy_probe"] / med[k],
             "words_per_s": nr * N / (med[k] * 1e-3)}
        name = [n for n in counts if "ILi%dELb%dEE" % (c[0], 1 if c[1] % 32 == 0 else 0) in n]
        if name and c[1] % 32 == 0:
            valu = counts[name[0]].get("valu_other", 0) / WORD_BODIES
            serial = -(-(-(-nr // 64)) // SIMDS)
            floor_ms = serial * N * valu * (CYCLES_ALONE if serial == 1 else 2) / (ghz * 1e9) * 1e3
            r.update({"valu_per_word_static": valu, "lds_per_word_static": counts[name[0]].get("lds", 0) / WORD_BODIES,
                      "issue_floor_ms": floor_ms, "floor_over_measured": floor_ms / med[k]})
        res[k] = r
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
