"""Static instruction counts of a library's gfx950 kernels by class, read from the code object with llvm-objdump: the helper
of tools/retime_bench.py (tools/array_bench.py carries its own copy for its own kernel).
Usage: python tools/isa_counts.py LIBRARY [part of the kernel's name]"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def instruction_counts(lib_path, match):
    """{kernel: {class: static count}} of the kernels whose names hold `match`, from the gfx950 code object bundled in the
    library (None without ROCm's llvm-objdump)."""
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
        return {k: v for k, v in out.items() if match in k}
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    print(json.dumps(instruction_counts(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""), indent=1))
