"""uc_duc_run timed: one transmitter block (2048 outputs a row, 26.2 ms of sound at 78 125 Hz) put onto 17.5 kHz carriers:
  65536_27_1_1_f32   65 536 rows, 27 taps, L = 1, I/Q in, one channel, floats out (2048 input pairs a row)
  65536_27_8_1_i16   65 536 rows, 27 taps per phase, L = 8, one channel, int16 out (256 input pairs a row)
  4096_27_8_4_f32    4 096 rows, 27 taps per phase, L = 8, four channels (four input rows and four carriers) summed, floats out
  65536_128_1_1_f32  65 536 rows, 128 taps, L = 1, one channel, floats out
every channel with its own phase, one tap set, the channel arrays given (so every call stages them).
HIP events around bursts of four calls of each variant, after a clock ramp of >= 150 ms of work; the variants alternated three
times with `iters` timings each; medians; the shader clock the SMU reported while the timed region ran
(bench_telemetry.PowerSampler; "not measured" where the files are not readable, and then 2.4 GHz is assumed and labelled).
Reports, per variant: ms per block, output-taps per second, the block's share of the 26.2 ms it lasts, and three yardsticks:
  the LDS floor     from the kernel's text (L divides 256): per output and tap of a channel a wave issues one 8-byte LDS read
                    of the sample pair and an eighth of a 4-byte read of the tap (one tap serves a lane's 8 outputs), 2 cycles
                    of the CU's one LDS each, against one packed multiply-add (4 cycles of one of four SIMDs): 2.25 LDS cycles
                    per 64 output-taps, over the chip's 256 CUs at the clock read in the run;
  the HBM floor     the algorithmic bytes (8 B read per input pair and channel, 4 or 2 B written per output) over the rate of a
                    device copy of 512 MB measured in this process;
  torch             the same arithmetic in torch on the same GPU: the I and the Q rows zero-stuffed by L, conv1d with the flipped
                    prototype over the zero-padded rows, times cos and sin of the full phase in float32 (made once outside the
                    timed region), added, summed over the channels, and for int16 rounded, clamped and converted.
Before anything is timed the first 300 samples of 130 rows of every variant are compared with the float32 definition.  One
condition is the project's own (derived, not tuned) and is printed as met or missed: the 65 536-row block, 27 taps, L = 1 takes
less than the 26.2 ms it lasts.  Nothing else is asserted: it is a record.
Usage: python tools/duc_bench.py [iters=5]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ultrasonic-communication_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

N_OUT = 2048
FS = 78125.0
BLOCK_MS = N_OUT / FS * 1e3
# (rows, K, L, channels, out)
VARIANTS = ((65536, 27, 1, 1, "f32"), (65536, 27, 8, 1, "i16"), (4096, 27, 8, 4, "f32"), (65536, 128, 1, 1, "f32"))
CUS = 256
BURST = 4
LDS_CYCLES_PER_WAVE_OUTPUT_TAP = 2.0 + 2.0 / 8.0


def name_of(v):
    return "%d_%d_%d_%d_%s" % v


def main():
    import torch
    import torch.nn.functional as F
    from uchirp import duc
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    step = duc.step_of(17500.0, FS)
    rng = np.random.default_rng(80)
    data = {}
    for v in VARIANTS:
        rows, K, L, n_chan, o = v
        n = N_OUT // L
        h = duc.interp_taps(L, K).astype(np.float32)
        slots = rows * n_chan
        data[v] = {"h": h, "obj": duc.Duc(h, L, 0), "n": n, "x": torch.randn((slots, 2 * n), dtype=torch.float32, device=dev) * (6000.0 / n_chan),
                   "y": torch.empty((rows, N_OUT), dtype=torch.float32 if o == "f32" else torch.int16, device=dev),
                   "state": torch.zeros((slots, 2 * duc.STATE_SAMPLES), dtype=torch.float32, device=dev),
                   "clip": torch.zeros(rows, dtype=torch.int32, device=dev), "steps": np.full(slots, step, np.uint32),
                   "phases": rng.integers(0, 2 ** 32, size=slots, dtype=np.uint64).astype(np.uint32)}

    def run(v):
        d = data[v]
        d["obj"].run(d["x"], 0, v[3], d["steps"], d["phases"], state=d["state"], out=v[4], y=d["y"], clip=d["clip"] if v[4] == "i16" else None)

    # the bits first: 130 rows against the float32 definition
    for v in VARIANTS:
        rows, K, L, n_chan, o = v
        d = data[v]
        ns = min(300, d["n"])
        x = d["x"][:130 * n_chan, :2 * ns].contiguous()
        got, st = d["obj"].run(x, 0, n_chan, d["steps"][:130 * n_chan], d["phases"][:130 * n_chan], out=o)
        want, want_st, _ = duc.emulate32(d["h"], x.cpu().numpy(), L, 0, n_chan, steps=d["steps"][:130 * n_chan], phases=d["phases"][:130 * n_chan], out=o)
        g = got.cpu().numpy()
        same = np.array_equal(g.view(np.uint32), want.view(np.uint32)) if o == "f32" else np.array_equal(g, want)
        if not (same and np.array_equal(st.cpu().numpy().view(np.uint32), want_st.view(np.uint32))):
            print("duc_bench: %s: the values differ from the definition" % name_of(v))
            return 1

    # torch: the same arithmetic, the carrier of the full phase in float32 made once outside the timed region
    tdata = {}
    for v in VARIANTS:
        rows, K, L, n_chan, o = v
        d = data[v]
        few = min(rows * n_chan, 4096)
        ang = torch.from_numpy(duc.phases32(0, N_OUT, d["steps"][:few], d["phases"][:few]).astype(np.float64) * (2.0 * np.pi / 2.0 ** 32)).to(dev)
        rep = rows * n_chan // few                                    # (timing only: the same work per row)
        tdata[v] = {"c": torch.cos(ang).float().repeat(rep, 1), "s": torch.sin(ang).float().repeat(rep, 1),
                    "k": torch.from_numpy(d["h"][::-1].copy()).to(dev)[None, None, :]}

    def run_torch(v):
        rows, K, L, n_chan, o = v
        d, t = data[v], tdata[v]
        acc = None
        for part, trig in ((0, t["c"]), (1, t["s"])):
            z = d["x"][:, part::2]
            if L > 1:
                up = torch.zeros((z.shape[0], N_OUT), dtype=torch.float32, device=dev)
                up[:, ::L] = z
                z = up
            f = F.conv1d(F.pad(z, (K * L - 1, 0))[:, None, :], t["k"])[:, 0, :] * trig
            acc = f if acc is None else acc + f
        y = acc.view(rows, n_chan, N_OUT).sum(dim=1) if n_chan > 1 else acc
        return y.round().clamp(-32768.0, 32767.0).to(torch.int16) if o == "i16" else y

    variants = {name_of(v): (lambda v=v: run(v)) for v in VARIANTS}
    torch_variants = {"torch_" + name_of(v): (lambda v=v: run_torch(v)) for v in VARIANTS}
    # every torch variant once before anything is timed: the first call of a shape picks and builds its convolution
    torch_err = {}
    for v in VARIANTS:
        t0 = time.time()
        y = run_torch(v)
        torch.cuda.synchronize()
        run(v)
        own = min(v[0] * v[3], 4096) // v[3]                          # the rows whose carriers are their own, not repeated ones
        got = data[v]["y"][:own].float()
        torch_err[name_of(v)] = float((y[:own].float() - got).abs().max() / got.abs().max())
        print("warm-up torch_%s: %.1f s" % (name_of(v), time.time() - t0), file=sys.stderr, flush=True)
        del y, got

    def timed(fn):
        """ms per call: BURST calls between two events, so that the host's part of a call (the copy of the channel records
        into the staging pair) runs while the call in front of it computes"""
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

    # the copy rate of this process: 512 MB read and 512 MB written
    src = torch.empty(128 * 1024 * 1024, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        run(VARIANTS[0])
        torch.cuda.synchronize()
    copy_ms = float(np.median(timed(lambda: dst.copy_(src)) + timed(lambda: dst.copy_(src))))
    copy_rate = 2.0 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
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
    res = {"outputs_per_row": N_OUT, "block_ms_of_sound": BLOCK_MS, "ms": med, "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
           "shader_clock_GHz": ghz, "shader_clock_source": (smu["source"] + ", mean of %d samples inside the timed region" % smu["samples"]) if mhz
           else "NOT measured in this run (hwmon files not readable): 2.4 GHz, the chip's maximum, assumed",
           "smu": smu, "copy_ms_512MB": copy_ms, "copy_bytes_per_s": copy_rate, "torch_vs_library_rel_err": torch_err}
    for v in VARIANTS:
        rows, K, L, n_chan, o = v
        k = name_of(v)
        sec = med[k] * 1e-3
        outs = rows * N_OUT
        nbytes = rows * n_chan * (N_OUT // L) * 8 + outs * (4 if o == "f32" else 2)
        waves = outs * K * n_chan / 64.0                              # output-taps of a wave
        lds = waves * LDS_CYCLES_PER_WAVE_OUTPUT_TAP / CUS / (ghz * 1e9) * 1e3
        res[k] = {"rows": rows, "taps_per_phase": K, "interp": L, "channels": n_chan, "out": o, "ms_per_block": med[k], "output_taps_per_s": outs * K * n_chan / sec,
                  "share_of_the_block_s_26_2_ms": med[k] / BLOCK_MS, "algorithmic_bytes": nbytes, "hbm_floor_ms": nbytes / copy_rate * 1e3,
                  "hbm_floor_over_measured": nbytes / copy_rate * 1e3 / med[k], "lds_floor_ms": lds, "lds_floor_over_measured": lds / med[k],
                  "torch_ms": med["torch_" + k], "torch_over_library": med["torch_" + k] / med[k]}
    flag = res[name_of(VARIANTS[0])]
    res["condition"] = "the 65 536-row block, 27 taps, L = 1, I/Q -> floats takes %.3f ms of the %.1f ms it lasts: %s" % (
        flag["ms_per_block"], BLOCK_MS, "met" if flag["ms_per_block"] < BLOCK_MS else "MISSED")
    print(json.dumps(res, indent=1))
    print("\n%-22s %9s %9s %9s %9s %9s" % ("rows_K_L_chan_out", "ms", "LDS fl.", "HBM fl.", "torch ms", "of 26.2"))
    for v in VARIANTS:
        r = res[name_of(v)]
        print("%-22s %9.4f %9.4f %9.4f %9.3f %9.4f" % (name_of(v), r["ms_per_block"], r["lds_floor_ms"], r["hbm_floor_ms"], r["torch_ms"], r["share_of_the_block_s_26_2_ms"]))
    print(res["condition"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
