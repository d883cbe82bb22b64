"""uc_array_combine against a torch composition on the same buffer and against the read rate of tools/libhbm_probe.so, same
process: 4096 microphones x 176 blocks of 2048 float samples (5.9 GB), 512 beams of 8 taps (every beam its own 8
microphones), delays uniform in 0 .. 40 samples.
  composition   per tap a shifted slice of the microphone's row, a 16-tap torch conv1d with the library's coefficients and
                an add into the beam's row (interior samples only: the composition does not pad)
  combine       1 uc_array_combine call
  probe         hbm_probe_read over the input buffer (a read-only stream: the achievable read rate)
HIP events around each variant, after a clock ramp of >= 150 ms of work; the variants alternated three times with `iters`
timings each; medians.  Reports the time of each, tap-samples per second, the algorithmic bytes (4 B per tap-sample read +
4 B per output written) over time as a fraction of the probe's rate, and the static instruction counts of the kernel by
class (whole kernel, from the library's code object).  Nothing is asserted: it is a record.
The instruction counts are those of the WHOLE kernel (every path, the edge forms and the store tail included); the split per
lane and tap in DESIGN.md section 11 and profiles/r09_array.txt is read off the inner loop of the compiler's listing by hand.
Usage: python tools/array_bench.py [mics=4096] [blocks=176] [beams=512] [iters=5]
       python tools/array_bench.py profile [mics] [blocks] [beams] [iters]     (only the combine calls: the program to put
       behind `rocprofv3 --kernel-trace --stats --` or behind a separate `rocprofv3 --kernel-trace --pmc <counters> --`)"""
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

N, TAPS, EDGE = 2048, 8, 64
LLVM = "/opt/rocm/lib/llvm/bin"


def instruction_counts(lib_path):
    """{kernel: {class: static count}} of the gfx950 code object bundled in the library (None without ROCm's llvm-objdump)."""
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
            name = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    name = m.group(1)
                    out[name] = {}
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\b", line)
                if not (m and name):
                    continue
                op = m.group(1)
                cls = ("valu_fma" if op.startswith(("v_pk_fma", "v_fma", "v_pk_mul", "v_mul_f32")) else "valu_other" if op.startswith("v_") else
                       "lds" if op.startswith("ds_") else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else
                       "smem" if op.startswith("s_load") else "salu" if op.startswith("s_") else "other")
                out[name][cls] = out[name].get(cls, 0) + 1
        return {k: v for k, v in out.items() if "array_kernel" in k}
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    import torch
    import torch.nn.functional as F
    from uchirp import array
    profile = len(sys.argv) > 1 and sys.argv[1] == "profile"      # the target of a profiler: the combine calls alone
    args = sys.argv[2:] if profile else sys.argv[1:]
    nm = int(args[0]) if len(args) > 0 else 4096
    nblk = int(args[1]) if len(args) > 1 else 176
    nb = int(args[2]) if len(args) > 2 else 512
    iters = int(args[3]) if len(args) > 3 else 5
    n = nblk * N
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x = torch.empty((nm, n), dtype=torch.float32, device=dev).normal_(0.0, 1000.0)
    beams = [[(int((b * TAPS + k) % nm), 1.0 / TAPS, float(d)) for k, d in enumerate(rng.uniform(0.0, 40.0, size=TAPS))] for b in range(nb)]
    taps, bm = array.pack(beams)
    ar = array.Array()
    L = array.lib()
    out = torch.empty((nb, n), dtype=torch.float32, device=dev)
    ref = torch.zeros((nb, n), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    coefs = [[array.coefficients(d, w) for (_, w, d) in beam] for beam in beams]
    weights = [[torch.from_numpy(c).to(dev).view(1, 1, -1) for (c, _) in row] for row in coefs]

    def combine():
        rc = L.uc_array_combine(ar._h, C.c_void_p(x.data_ptr()), array.DTYPE_F32, nm, 0, n, 0, taps.ctypes.data_as(C.c_void_p), len(taps),
                                bm.ctypes.data_as(C.c_void_p), nb, C.c_void_p(out.data_ptr()), 0, n, 0, stream)
        if rc:
            raise RuntimeError(L.uc_array_last_error().decode())

    def composition():
        for b in range(nb):
            row = ref[b, EDGE:n - EDGE].view(1, 1, -1)
            for k, (mic, _, _) in enumerate(beams[b]):
                s = EDGE + coefs[b][k][1]
                y = F.conv1d(x[mic, s:s + n - 2 * EDGE + 15].view(1, 1, -1), weights[b][k])
                if k == 0:
                    row.copy_(y)
                else:
                    row.add_(y)

    probe = None
    ppath = os.path.join(ROOT, "tools", "libhbm_probe.so")
    if os.path.exists(ppath):
        P = C.CDLL(ppath)
        P.hbm_probe_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count * 8
        sink = torch.zeros(blocks, dtype=torch.int32, device=dev)
        probe = lambda: P.hbm_probe_read(x.data_ptr(), x.numel() * 4, sink.data_ptr(), blocks, stream.value)   # noqa: E731

    variants = {"combine": combine, "composition": composition}
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

    if profile:
        for _ in range(iters):
            combine()
        torch.cuda.synchronize()
        print("profile target: %d uc_array_combine calls, %d microphones x %d samples, %d beams of %d taps" % (iters, nm, n, nb, TAPS))
        return 0
    combine()
    composition()
    torch.cuda.synchronize()
    diff = float((out[::16, EDGE:n - EDGE] - ref[::16, EDGE:n - EDGE]).abs().max())
    t0 = time.time()
    while time.time() - t0 < 0.15:           # clock ramp before anything is timed
        combine()
        if probe:
            probe()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ts[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    tap_samples = nb * TAPS * n
    alg_bytes = 4 * tap_samples + 4 * nb * n
    res = {"input": [nm, n], "beams": nb, "taps_per_beam": TAPS, "ms": med, "ms_all": {k: [round(t, 3) for t in v] for k, v in ts.items()},
           "tap_samples": tap_samples, "combine_tap_samples_per_s": tap_samples / (med["combine"] * 1e-3),
           "algorithmic_bytes": alg_bytes, "combine_algorithmic_bytes_per_s": alg_bytes / (med["combine"] * 1e-3),
           "ratio_composition_over_combine": med["composition"] / med["combine"],
           "check": {"max_abs_combine_minus_composition_on_32_beams": diff, "input_sigma": 1000.0},
           "instructions_static_whole_kernel": instruction_counts(array.LIB_PATH)}
    if probe:
        rate = x.numel() * 4 / (med["probe_read"] * 1e-3)
        res["probe_read_bytes_per_s"] = rate
        res["combine_algorithmic_fraction_of_probe_read"] = res["combine_algorithmic_bytes_per_s"] / rate
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
