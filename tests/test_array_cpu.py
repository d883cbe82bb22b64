"""CPU tests of the array combiner (include/uchirp_array.h, libuchirp_array.so, uchirp/array.py): the boundary, the
coefficients the library computes on the host, what the compiler made of the kernels, and the numpy model the GPU tests
hold the kernels against."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_array.h")
FS = 78125.0
DELAYS = (0.0, 1.0, -1.0, 0.5, -0.5, 3.37, -2.9, 100.125, 0.999, 1e6 + 0.25)
FRACTIONAL = tuple(d for d in DELAYS if d != np.floor(d))


@pytest.fixture(scope="module")
def array():
    from uchirp import array as m
    m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def link():
    from uchirp import link as m
    return m


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_array_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_the_structs_have_their_sizes(array, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_array.h"\nint main(void) { return sizeof(uc_array_tap) == 16 && sizeof(uc_array_beam) == 8 && '
                   'UC_ARRAY_MAX_TAPS == 32 && UC_ARRAY_ABI_VERSION == 1 && UC_ARRAY_DTYPE_I32 == 0 && UC_ARRAY_DTYPE_F32 == 1 ? 0 : 1; }\n')
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    assert C.sizeof(array.ArrayTap) == 16 == array.TAP_DTYPE.itemsize and C.sizeof(array.ArrayBeam) == 8 == array.BEAM_DTYPE.itemsize
    for struct, dt in ((array.ArrayTap, array.TAP_DTYPE), (array.ArrayBeam, array.BEAM_DTYPE)):
        for (name, _), np_name in zip(struct._fields_, dt.names):
            assert name == np_name and getattr(struct, name).offset == dt.fields[name][1]


def test_every_declared_symbol_is_exported(array):
    decl = _declared_functions()
    assert len(decl) == 6, decl
    L = array.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(array.EXPORTS) == decl
    assert L.uc_array_abi_version() == 1 == array.ABI_VERSION


def test_array_library_stands_alone(array):
    """libuchirp_array.so links none of the other three libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", array.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", array.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_array(array):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = array.lib().uc_array_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in array.lib().uc_array_last_error()
    with pytest.raises(array.ArrayError):
        array.Array()


def test_coefficients_are_the_definition(array):
    L = array.lib()
    for d in DELAYS:
        for w in (1.0, -0.37, 0.125):
            got, shift = array.coefficients(d, w)
            want, wshift = array.coefficients_model(d, w)
            assert shift == wshift == int(np.floor(d)) - 7, d
            ulp = float(np.spacing(np.abs(want).max()))
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            print("delay %-12r weight %-6r shift %-7d max |library - numpy| %.3g (1 ulp of the largest coefficient %.3g)" % (d, w, shift, err, ulp))
            assert err <= ulp, (d, w)
            if d == np.floor(d):
                exact = np.zeros(16, np.float32)
                exact[7] = np.float32(w)
                assert np.array_equal(got, exact) and np.array_equal(want, exact), d
            else:
                assert abs(float(got.astype(np.float64).sum()) / w - 1.0) < 1e-3, d        # an interpolator passes DC
    # a tiny negative delay: D - floor(D) rounds to 1.0; both take the integer tap of delay 0
    assert array.coefficients(-1e-20, 1.0)[1] == -7 == array.coefficients_model(-1e-20, 1.0)[1]
    assert np.array_equal(array.coefficients(-1e-20, 1.0)[0], array.coefficients(0.0, 1.0)[0])
    c = (C.c_float * 16)()
    s = C.c_int64()
    for d, w in ((np.inf, 1.0), (np.nan, 1.0), (0.0, np.inf), (2.0 ** 30 + 1, 1.0), (-2.0 ** 30 - 1, 1.0)):
        assert L.uc_array_tap_coefficients(d, w, C.byref(s), c) == -errno.EINVAL, (d, w)
        assert L.uc_array_last_error()
    assert L.uc_array_tap_coefficients(2.0 ** 30, 1.0, C.byref(s), c) == 0 and s.value == 2 ** 30 - 7
    assert L.uc_array_tap_coefficients(0.5, 1.0, None, c) == -errno.EINVAL


def test_interpolator_against_the_analytic_signal(array, link):
    """One tap of delay D on link.signal(text, lead) is link.signal(text, lead - D): away from the buffer's ends and at
    least 12 samples from every symbol boundary (there the frame's phase jumps, which no band-limited interpolator follows)
    the worst error stays at or below 2e-4 of the peak amplitude * sqrt 2 (1.02e-4 measured with these delays; the factor 2
    covers delays that are not in the list)."""
    amp, lead, text = 2000.0, 3000.25, "Hi!"
    period = 1155.0 / 44100.0 * FS                      # one symbol in samples of fs_out
    n = 48 * 2048
    j = np.arange(n, dtype=np.float64)
    worst = 0.0
    for d in FRACTIONAL:
        first = int(np.floor(d)) if d > 1000.0 else 0   # for the large delay the buffer holds the samples the tap reads
        x = link.signal(text, lead + (d if d > 1000.0 else 0.0), amp, 0.0, n, FS, first_sample=first)
        shown = lead - (0.0 if d > 1000.0 else d)
        y = array.model(x[None, :], [[(0, 1.0, d)]], in_first=first, out_first=0, n_out=n)[0]
        ref = link.signal(text, shown, amp, 0.0, n, FS)
        assert np.abs(ref).max() > amp
        phase = np.mod(j - shown, period)
        keep = (np.minimum(phase, period - phase) >= 12.0) & (j >= 32) & (j < n - 32)
        err = float(np.abs(y - ref)[keep].max()) / (amp * 2 ** 0.5)
        print("delay %-12r worst |model - analytic| / peak %.3g over %d samples (%d sounding)" % (d, err, keep.sum(), (ref[keep] != 0).sum()))
        assert (ref[keep] != 0).sum() > 20000
        worst = max(worst, err)
    assert worst <= 2e-4, worst


def test_gain_of_a_delay_and_sum_beam_over_noise(array, link):
    M, n, sigma = 8, 65536, 50.0
    x = np.stack([sigma * link.normals(11, m, 0, n)[0] for m in range(M)])
    y = array.model(x, [array.steer([0.0] * M)])[0]
    ratio = y.var() / (sigma ** 2 / M)
    print("noise only, %d microphones, weights 1/M: variance of the beam / (sigma^2 / M) = %.4f" % (M, ratio))
    assert abs(ratio - 1.0) <= 0.10


def test_model_copy_window_and_steer(array):
    rng = np.random.default_rng(4)
    x = rng.integers(-2 ** 20, 2 ** 20, size=(3, 500)).astype(np.int32)
    # an integer delay with weight 1 is a shifted copy with zeros shifted in; integer words are cast to float
    for d in (0, 5, -3, 499, -600):
        y = array.model(x, [[(2, 1.0, float(d))]])[0]
        want = np.zeros(500)
        src = np.arange(500) + d
        ok = (src >= 0) & (src < 500)
        want[ok] = x[2, src[ok]].astype(np.float32)
        assert np.array_equal(y, want), d
    # in_first / out_first / n_out name absolute samples
    beams = [[(0, 0.5, 2.25), (1, -1.0, -7.5)], [(2, 1.0, 0.0)]]
    whole = array.model(x, beams, in_first=1000)
    part = array.model(x[:, 100:400], beams, in_first=1100, out_first=1150, n_out=200)
    assert np.array_equal(part, whole[:, 150:350])
    assert array.steer([10.5, 3.25, 7.0]) == [(0, 1 / 3, 7.25), (1, 1 / 3, 0.0), (2, 1 / 3, 3.75)]
    assert array.steer([10.5, 3.25], ref=1.25) == [(0, 0.5, 9.25), (1, 0.5, 2.0)]
    taps, b = array.pack(beams)
    assert list(b["first_tap"]) == [0, 2] and list(b["n_taps"]) == [2, 1]
    assert list(taps["mic"]) == [0, 1, 2] and list(taps["weight"]) == [0.5, -1.0, 1.0] and list(taps["delay_samples"]) == [2.25, -7.5, 0.0]
    with pytest.raises(ValueError):
        array.pack([[]])
    with pytest.raises(ValueError):
        array.pack([[(0, 1.0, 0.0)] * 33])
    assert len(array.pack([[(0, 1.0, 0.0)] * 32])[0]) == 32


def build_host(tmp_path):
    import uchirp
    from uchirp import array, scene
    for m in (uchirp, scene, array):          # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_array")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_array.c"), "-o", exe, "-L" + libdir, "-luchirp_array", "-luchirp_scene",
                           "-luchirp", "-Wl,-rpath," + libdir])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(array, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "uc_array_abi_version 1 (header 1)" in out.stdout and "uc_array_create: -19" in out.stdout and "no CPU path" in out.stdout


def test_kernels_are_gfx950_without_spills_or_scratch(array, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    if not os.path.exists(array.LIB_PATH):
        pytest.skip("libuchirp_array.so not built")
    monkeypatch.setattr(kr, "LIB", array.LIB_PATH)
    ks = kr._kernels(tmp_path)
    assert len(ks) == 2 and all("array_kernel" in k for k in ks), sorted(ks)      # f32, i32
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            assert e["private_segment_fixed_size"] == 0, (k, e)
            assert e["vgpr_count"] <= 64, (k, e)      # 8 waves per SIMD
            assert e["group_segment_fixed_size"] == 4 * 272 * 4, (k, e)     # four wave-private windows of 272 floats
