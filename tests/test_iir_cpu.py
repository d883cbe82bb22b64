"""CPU tests of the recursive filter bank (include/uchirp_iir.h, libuchirp_iir.so, uchirp/iir.py): the boundary, the designs
against the reference's own coefficients (fixture K3), the float64 model and the float32 definition against the reference's
own low-pass outputs, the library's plain-C row function against the definition bit for bit (denormals and -0.0 included),
cuts, and what the compiler made of the kernels.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import iir_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_iir.h")


@pytest.fixture(scope="module")
def iir():
    from uchirp import iir as m
    m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def k3(iir):
    rows, want, fs, cutoff = iu.k3_rows()
    return rows, want, iir.lpf_sections(fs, cutoff)


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_iir_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(iir, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_iir.h"\nint main(void) { return UC_IIR_ABI_VERSION == %d && UC_IIR_DTYPE_I32 == %d && '
                   'UC_IIR_DTYPE_F32 == %d && UC_IIR_MAX_SECTIONS == %d && UC_IIR_MAX_SETS == %d && UC_IIR_SECTION_WORDS == %d && '
                   'UC_IIR_STATE_WORDS == %d ? 0 : 1; }\n'
                   % (iir.ABI_VERSION, iir.DTYPE_I32, iir.DTYPE_F32, iir.MAX_SECTIONS, iir.MAX_SETS, iir.SECTION_WORDS, iir.STATE_WORDS))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    decl = _declared_functions()
    assert len(decl) == 7, decl
    L = iir.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(iir.EXPORTS) == decl
    assert L.uc_iir_abi_version() == 1 == iir.ABI_VERSION


def test_iir_library_stands_alone(iir):
    """libuchirp_iir.so links none of the other libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", iir.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", iir.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_filter_bank(iir):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = iir.lib().uc_iir_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in iir.lib().uc_iir_last_error()
    with pytest.raises(iir.IirError):
        iir.Iir()


def build_host(tmp_path):
    import uchirp
    from uchirp import iir
    for m in (uchirp, iir):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_iir")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_iir.c"), "-o", exe, "-L" + libdir, "-luchirp_iir", "-luchirp",
                           "-Wl,-rpath," + libdir])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(iir, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0
    assert "uc_iir_abi_version 1 (header 1)" in out.stdout and "uc_iir_create: -19" in out.stdout and "no CPU path" in out.stdout
    assert "dtype 7 refused" in out.stdout
    assert "step response of the one-pole low-pass after 64 samples: 1.000000" in out.stdout


# ---- 1. the designs

def test_lpf_sections_are_the_reference_s_butterworth(iir):
    """lpf_sections(44100, 3000): order 14 as the fixture records, 7 sections whose polynomials multiply to the b, a that the
    reference's lpf() designed (k3_butter_b / k3_butter_a), within 1e-9 of the largest coefficient of each; where scipy
    imports, the same poles as scipy.signal.butter(..., output="sos") to 1e-12."""
    v = np.load(os.path.join(iu.GOLD, "notebook_vectors_k3k5.npz"))
    s = iir.lpf_sections(44100, 3000)
    order, wn = iir.lpf_order(44100, 3000)
    assert s.shape == (7, 5) and s.dtype == np.float64 and order == 14
    b, a = iir.polynomials(s)
    eb = np.abs(b - v["k3_butter_b"]).max() / np.abs(v["k3_butter_b"]).max()
    ea = np.abs(a - v["k3_butter_a"]).max() / np.abs(v["k3_butter_a"]).max()
    print("products of the sections against the fixture: b %.3g, a %.3g of the largest coefficient" % (eb, ea))
    assert b.size == 15 == v["k3_butter_b"].size and eb <= 1e-9 and ea <= 1e-9
    radius = np.sqrt(s[:, 4])
    print("pole radii:", np.round(radius, 6))
    assert (np.diff(radius) > 0).all() and radius.max() < 1.0                  # ascending, stable
    for k in range(7):                                                          # unity gain at DC, section by section
        assert abs(abs(iir.response(s[k], [0.0], 44100.0)[0]) - 1.0) <= 1e-12, k
    try:
        import scipy.signal as sg
    except ImportError:
        print("scipy does not import: the comparison with its sos design did not run")
        return
    n, w = sg.buttord(wp=3000 / 22050.0, ws=1.3 * 3000 / 22050.0, gpass=2, gstop=30)
    sos = sg.butter(n, w, btype="low", output="sos")
    mine = np.sort_complex(np.concatenate([np.roots([1.0, r[3], r[4]]) for r in s]))
    theirs = np.sort_complex(np.concatenate([np.roots([1.0, r[4], r[5]]) for r in sos]))
    print("poles against scipy's sos: %.3g" % np.abs(mine - theirs).max())
    assert n == 14 and np.abs(mine - theirs).max() <= 1e-12


def test_bandpass_and_dc_block_are_butterworth(iir):
    bp = iir.bandpass_sections(78125.0, 16000.0, 19000.0, 4)
    h = np.abs(iir.response(bp, [16000.0, 19000.0, np.sqrt(16000.0 * 19000.0), 12000.0, 24000.0], 78125.0))
    print("band-pass 16-19 kHz, order 4: |H| at the edges %.6f %.6f, inside %.6f, at 12 and 24 kHz %.2e %.2e" % tuple(h))
    assert bp.shape == (4, 5) and abs(h[0] - 0.5 ** 0.5) <= 1e-9 and abs(h[1] - 0.5 ** 0.5) <= 1e-9 and 0.99 < h[2] <= 1.0 + 1e-9
    assert h[3] < 1e-2 and h[4] < 1e-2 and (np.diff(np.sqrt(bp[:, 4])) >= 0).all() and np.sqrt(bp[:, 4]).max() < 1.0
    w0 = 78125.0 / np.pi * np.arctan(np.sqrt(np.tan(np.pi * 16000.0 / 78125.0) * np.tan(np.pi * 19000.0 / 78125.0)))
    for k in range(4):                                                          # unity gain at the centre, section by section
        assert abs(abs(iir.response(bp[k], [w0], 78125.0)[0]) - 1.0) <= 1e-12, k
    dc = iir.dc_block_sections(78125.0, 20.0)
    h = np.abs(iir.response(dc, [0.0, 20.0, 39062.5], 78125.0))
    print("DC blocker, corner 20 Hz: |H| at 0, 20 Hz and fs / 2: %.3g %.6f %.6f" % tuple(h))
    assert dc.shape == (1, 5) and h[0] <= 1e-12 and abs(h[1] - 0.5 ** 0.5) <= 1e-9 and abs(h[2] - 1.0) <= 1e-12
    hp3 = iir.dc_block_sections(78125.0, 200.0, order=3)
    assert hp3.shape == (2, 5) and abs(abs(iir.response(hp3, [200.0], 78125.0)[0]) - 0.5 ** 0.5) <= 1e-9
    try:
        import scipy.signal as sg
    except ImportError:
        return
    sos = sg.butter(4, [16000.0, 19000.0], btype="band", fs=78125.0, output="sos")
    mine = np.sort_complex(np.concatenate([np.roots([1.0, r[3], r[4]]) for r in bp]))
    theirs = np.sort_complex(np.concatenate([np.roots([1.0, r[4], r[5]]) for r in sos]))
    assert np.abs(mine - theirs).max() <= 1e-12
    for bad in (lambda: iir.bandpass_sections(78125.0, 19000.0, 16000.0, 4), lambda: iir.bandpass_sections(78125.0, 16000.0, 19000.0, 9),
                lambda: iir.lpf_sections(44100.0, 20000.0), lambda: iir.dc_block_sections(78125.0, 0.0)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. against the reference's own output

def test_float64_model_reproduces_the_reference_s_lpf_output(iir, k3):
    """The notebook's four mixed rows through `model` (float64 on the float32 coefficients and samples) against k3_R and k3_Rd,
    what the reference's lfilter gave: measured 2.7e-7 of the peak (the samples' rounding to float32 is 6e-8 of it).  The
    bound of 1e-6 allows for a design that differs in the last digits, against a reference whose b, a form is itself the
    ill-conditioned one."""
    rows, want, s = k3
    got = iir.model(s, rows)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("float64 model against the reference's lpf(): %.3g of the peak" % err)
    assert got.shape == want.shape == (4, 1155) and err <= 1e-6


def test_float32_definition_reproduces_the_reference_s_lpf_output(iir, k3):
    """emulate32 on the same rows: measured 3.5e-6 of the peak with unity-gain sections."""
    rows, want, s = k3
    got, st = iir.emulate32(s, rows.astype(np.float32))
    err = np.abs(got - want).max() / np.abs(want).max()
    print("float32 definition against the reference's lpf(): %.3g of the peak" % err)
    assert got.dtype == np.float32 and st.shape == (4, 16) and not st[:, 14:].any() and err <= 2e-5


# ---- 3. the plain C row function

@pytest.mark.parametrize("count", iu.SECTION_COUNTS)
def test_filter_row_is_the_definition_bit_for_bit(iir, count):
    """uc_iir_filter_row against emulate32 on noise, on an impulse of 1e-34 over 300 samples, on a row that starts with -0.0
    and on one with NaN and +-Inf, floats and words, from states that hold -0.0 and denormals.  The impulse discriminates: a
    flushing variant of the emulation differs from the definition in all 300 outputs (7 sections: the reference's low-pass;
    the DC blocker alone passes the impulse on at 1e-34 and its tail stays normal for 300 samples: nothing to flush there)."""
    c = iu.cascades()[count]
    f, w = iu.inputs()
    st0 = iu.states()
    for name, x in (("f32", f), ("i32", w)):
        rows = [iu.IMPULSE_ROW, iu.MINUS_ZERO_ROW, iu.NAN_ROW, iu.DENORMAL_STATE_ROW, 4, 129]
        want, want_st = iir.emulate32(c, x[rows], st0[rows])
        assert np.isfinite(want).all() and np.isfinite(want_st).all()
        for k, r in enumerate(rows):
            got, st = iir.filter_row(c, x[r], st0[r])
            assert np.array_equal(iu.bits(got), iu.bits(want[k])) and np.array_equal(iu.bits(st), iu.bits(want_st[k])), (name, r)
            assert np.array_equal(iu.bits(st[2 * count:]), iu.bits(st0[r, 2 * count:]))          # sections that do not exist: untouched
        if name == "f32":
            assert (iu.bits(want[1, :1]) == 0x80000000).all()                    # -0.0 in, -0.0 state: -0.0 out
    imp, _ = iir.emulate32(c, f[iu.IMPULSE_ROW])
    flushed, _ = iir.emulate32(c, f[iu.IMPULSE_ROW], flush=True)
    differ = int((iu.bits(imp) != iu.bits(flushed)).sum())
    tiny = np.finfo(np.float32).tiny
    print("%d sections: the 1e-34 impulse: %d of 300 outputs are denormal; a flushing emulation differs in %d"
          % (count, int(((np.abs(imp) < tiny) & (imp != 0)).sum()), differ))
    if count == 7:
        assert differ == 300
    assert (differ > 0 or count == 1) and np.array_equal(iu.bits(iir.filter_row(c, f[iu.IMPULSE_ROW])[0]), iu.bits(imp))


@pytest.mark.parametrize("count", iu.SECTION_COUNTS)
def test_cuts_give_the_bits_of_one_call(iir, count):
    c = iu.cascades()[count]
    f, w = iu.inputs()
    st0 = iu.states()
    rows = [0, 1, 2, 3, 7]
    for x in (f, w):
        whole, whole_st = iir.emulate32(c, x[rows], st0[rows])
        s, parts, a = st0[rows], [], 0
        for n in (1, 77, 222):
            o, s = iir.emulate32(c, x[rows, a:a + n], s)
            parts.append(o)
            a += n
        assert a == 300 and np.array_equal(iu.bits(np.concatenate(parts, axis=1)), iu.bits(whole)) and np.array_equal(iu.bits(s), iu.bits(whole_st))
        for k, r in enumerate(rows):
            s, parts, a = st0[r], [], 0
            for n in (1, 77, 222):
                o, s = iir.filter_row(c, x[r, a:a + n], s)
                parts.append(o)
                a += n
            assert np.array_equal(iu.bits(np.concatenate(parts)), iu.bits(whole[k])) and np.array_equal(iu.bits(s), iu.bits(whole_st[k])), r


def test_model_and_definition_agree_to_float32_accuracy(iir):
    """The float64 model and the float32 definition on noise through every cascade: the difference stays within 1e-4 of the
    output's peak (the band-pass of order 8 has poles at radius 0.98: its noise gain is the largest)."""
    f, _ = iu.inputs()
    for count, c in iu.cascades().items():
        m = iir.model(c, f[4:12])
        e, _ = iir.emulate32(c, f[4:12])
        err = np.abs(e - m).max() / np.abs(m).max()
        print("%d sections: |emulate32 - model| = %.3g of the peak" % (count, err))
        assert err <= 1e-4


def test_host_function_refuses_what_the_header_says(iir):
    L = iir.lib()
    c = np.ascontiguousarray(iu.cascades()[2], np.float32)
    x = np.zeros(4, np.float32)
    out = np.full(4, 7.0, np.float32)
    st = np.zeros(16, np.float32)
    bad = c.copy()
    bad[1, 3] = np.nan
    inf = c.copy()
    inf[0, 0] = np.inf
    fp = C.POINTER(C.c_float)
    cp, bp, ip, xp, op, sp = (a.ctypes.data_as(t) for a, t in ((c, fp), (bad, fp), (inf, fp), (x, C.c_void_p), (out, fp), (st, fp)))
    for name, args in (("sections NULL", (None, 2, xp, 1, 4, sp, op)), ("in NULL", (cp, 2, None, 1, 4, sp, op)), ("state NULL", (cp, 2, xp, 1, 4, None, op)),
                       ("out NULL", (cp, 2, xp, 1, 4, sp, None)), ("0 sections", (cp, 0, xp, 1, 4, sp, op)), ("9 sections", (cp, 9, xp, 1, 4, sp, op)),
                       ("-1 sections", (cp, -1, xp, 1, 4, sp, op)), ("dtype 2", (cp, 2, xp, 2, 4, sp, op)), ("dtype -1", (cp, 2, xp, -1, 4, sp, op)),
                       ("n 0", (cp, 2, xp, 1, 0, sp, op)), ("NaN coefficient", (bp, 2, xp, 1, 4, sp, op)), ("Inf coefficient", (ip, 2, xp, 1, 4, sp, op))):
        assert L.uc_iir_filter_row(*args) == -errno.EINVAL and L.uc_iir_last_error(), name
    assert (out == 7.0).all() and not st.any()
    assert L.uc_iir_create(0, None) == -errno.EINVAL
    with pytest.raises(ValueError):
        iir.emulate32(np.zeros((9, 5)), x)


# ---- what the compiler made of the kernels

def code_objects(iir, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    monkeypatch.setattr(kr, "LIB", iir.LIB_PATH)
    ks = kr._kernels(tmp_path)
    assert len(ks) == 16 and all("iir_kernel" in k for k in ks), sorted(ks)      # f32, i32 x 1 .. 8 sections
    for k, v in sorted(ks.items()):
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            print(k, {f: e.get(f) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            # two tiles of 64 rows x (16 + 4) words in LDS; one wave per workgroup; at most 128 registers: four waves a SIMD
            assert e["private_segment_fixed_size"] == 0 and e["group_segment_fixed_size"] == 2 * 64 * 20 * 4, (k, e)
            assert e["max_flat_workgroup_size"] == 64 and e["vgpr_count"] <= 128, (k, e)
    return ks


def test_kernels_are_gfx950_without_spills_or_scratch(iir, tmp_path, monkeypatch):
    if not os.path.exists(iir.LIB_PATH):
        pytest.skip("libuchirp_iir.so not built")
    code_objects(iir, tmp_path, monkeypatch)
