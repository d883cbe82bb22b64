"""CPU tests of the retimer (include/uchirp_retime.h, libuchirp_retime.so, uchirp/retime.py): the boundary, the table and the
fixed-point step the library evaluates on the host against Python's own arithmetic, the float64 model against the
definition and against the analytic signal of the link's law, the host-side line estimator on the project's own signal,
and what the compiler made of the kernels.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_retime.h")
N = 2048
FS = 78125.0


@pytest.fixture(scope="module")
def retime():
    from uchirp import retime as m
    m.build()
    m.lib()
    return m


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
    return sorted(set(re.findall(r"\b(uc_retime_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(retime, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_retime.h"\nint main(void) { return sizeof(uc_retime_line) == 24 && UC_RETIME_ABI_VERSION == %d && '
                   'UC_RETIME_DTYPE_I32 == %d && UC_RETIME_DTYPE_F32 == %d && UC_RETIME_COEFS == %d && UC_RETIME_TABLE_ROWS == %d ? 0 : 1; }\n'
                   % (retime.ABI_VERSION, retime.DTYPE_I32, retime.DTYPE_F32, retime.COEFS, retime.TABLE_ROWS))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    assert C.sizeof(retime.RetimeLine) == 24 == retime.LINE_DTYPE.itemsize
    assert [retime.LINE_DTYPE.fields[k][1] for k in ("delay_samples", "slope", "mic", "reserved")] == [0, 8, 16, 20]
    decl = _declared_functions()
    assert len(decl) == 7, decl
    L = retime.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(retime.EXPORTS) == decl
    assert L.uc_retime_abi_version() == 1 == retime.ABI_VERSION


def test_retime_library_stands_alone(retime):
    """libuchirp_retime.so links none of the other six libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", retime.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", retime.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_retimer(retime):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = retime.lib().uc_retime_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in retime.lib().uc_retime_last_error()
    with pytest.raises(retime.RetimeError):
        retime.Retimer()


def test_table_rows_are_the_array_combiner_s_coefficients(retime, array):
    t = retime.table()
    assert t.shape == (257, 16) and t.dtype == np.float32
    differ = 0
    for q in range(256):
        c, shift = array.coefficients(q / 256.0, 1.0)
        assert shift == -7
        differ += int((c.view(np.uint32) != t[q].view(np.uint32)).sum())
    print("table: %d of 4096 entries differ in a bit from uc_array_tap_coefficients(q / 256, 1)" % differ)
    assert differ == 0
    unit7, unit8 = np.zeros(16, np.float32), np.zeros(16, np.float32)
    unit7[7], unit8[8] = 1.0, 1.0
    assert np.array_equal(t[0].view(np.uint32), unit7.view(np.uint32)) and np.array_equal(t[256].view(np.uint32), unit8.view(np.uint32))
    # numpy's twin: its sine and Bessel function may round an entry the other way, no more
    worst = float(np.abs(retime.table_model().astype(np.float64) - t.astype(np.float64)).max())
    print("table_model: worst |numpy - library| %.3g" % worst)
    assert worst <= 2.0 ** -23
    # the rows run into each other, row 256 (the next sample) included: no step between rows larger than the slope of the
    # windowed sinc allows, pi / 2 per sample, over 1 / 256 of a sample
    step = float(np.abs(np.diff(t.astype(np.float64), axis=0)).max())
    print("table: largest step between neighbouring rows %.5f" % step)
    assert step <= np.pi / 2.0 / 256.0
    assert retime.lib().uc_retime_table(None) == -errno.EINVAL and retime.lib().uc_retime_last_error()


def test_fixed_is_python_integer_arithmetic(retime):
    L = retime.lib()
    rng = np.random.default_rng(11)
    draws = [(float(rng.uniform(-1.0, 1.0) * 10.0 ** rng.uniform(-12, 9)), float(rng.uniform(-1.0, 1.0) * 10.0 ** rng.uniform(-14, -2.71)))
             for _ in range(200)]
    draws += [(2.0 ** 30, 2.0 ** -9), (-2.0 ** 30, -2.0 ** -9), (0.0, 0.0), (-0.0, -0.0), (2.0 ** -33, 2.0 ** -33), (-2.0 ** -33, -2.0 ** -33),
              (3.0 * 2.0 ** -33, -3.0 * 2.0 ** -33), (0.5 + 2.0 ** -33, 2.0 ** -32), (37.25, 60e-6), (5e-324, -5e-324),
              (np.nextafter(2.0 ** 30, 0.0), np.nextafter(2.0 ** -9, 0.0))]
    for d, s in draws:
        want = (int(round(Fraction(d) * 2 ** 32)), int(round(Fraction(s) * 2 ** 32)))
        assert retime.fixed(d, s) == want == retime.fixed_model(d, s), (d, s)
        assert abs(want[0]) <= 2 ** 62 and abs(want[1]) <= 2 ** 23
    assert retime.fixed(2.0 ** -33, 3.0 * 2.0 ** -33) == (0, 2)                   # ties go to the even integer
    a, b = C.c_int64(7), C.c_int64(7)
    for name, d, s in (("delay beyond 2^30", np.nextafter(2.0 ** 30, np.inf), 0.0), ("delay below -2^30", -np.nextafter(2.0 ** 30, np.inf), 0.0),
                       ("slope beyond 2^-9", 0.0, np.nextafter(2.0 ** -9, 1.0)), ("slope below -2^-9", 0.0, -np.nextafter(2.0 ** -9, 1.0)),
                       ("delay nan", np.nan, 0.0), ("delay inf", np.inf, 0.0), ("slope nan", 0.0, np.nan), ("slope -inf", 0.0, -np.inf)):
        assert L.uc_retime_fixed(d, s, C.byref(a), C.byref(b)) == -errno.EINVAL, name
        assert L.uc_retime_last_error() and a.value == 7 and b.value == 7, name
        with pytest.raises(ValueError):
            retime.fixed_model(d, s)
    assert L.uc_retime_fixed(1.0, 0.0, None, C.byref(b)) == -errno.EINVAL and L.uc_retime_fixed(1.0, 0.0, C.byref(a), None) == -errno.EINVAL


def _definition(xf, n_in, in_first, T, delay, slope, j):
    """one output sample by the header's words, in Python integers and float64"""
    lead_fx, drift_fx = int(round(Fraction(delay) * 2 ** 32)), int(round(Fraction(slope) * 2 ** 32))
    off = lead_fx + j * drift_fx
    i_whole = j + (off >> 32)
    frac = off & 0xFFFFFFFF
    q, mu = frac >> 24, (frac & 0xFFFFFF) * 2.0 ** -24
    y = mag = 0.0
    for t in range(16):
        d = float(np.float32(T[q + 1][t]) - np.float32(T[q][t]))
        c = float(T[q][t]) + mu * d
        i = i_whole - 7 + t - in_first
        v = xf[i] if 0 <= i < n_in else 0.0
        y += c * v
        mag += abs(c * v)
    return y, mag


def test_model_is_the_definition(retime):
    rng = np.random.default_rng(2)
    x = rng.integers(-2 ** 27, 2 ** 27, size=(3, 300)).astype(np.int32)       # mostly no floats: the cast rounds
    xf = x.astype(np.float32).astype(np.float64)
    T = retime.table()
    lines = [(0, 2.25, 0.0), (2, -7.5, 1e-3), (1, 100.0 + 255.0 / 256.0, -2.0 ** -9), (1, 0.0, 2.0 ** -32), (0, -400.0, 0.0), (2, 3.0, 0.0)]
    for in_first, out_first, n_out in ((0, 0, 300), (50, 40, 333), (2 ** 37, 2 ** 37 - 3, 310)):
        lines_here = [(m, d - s * out_first if abs(s) > 1e-6 else d, s) for (m, d, s) in lines]     # keep the positions inside the row
        got = retime.model(x, lines_here, in_first, out_first, n_out, table=retime.table)
        mag = retime.model(x, lines_here, in_first, out_first, n_out, table=retime.table, magnitude=True)
        for r, (m, d, s) in enumerate(lines_here):
            for i in range(n_out):
                y, a = _definition(xf[m], 300, in_first, T, d, s, out_first + i)
                assert abs(got[r, i] - y) <= 1e-12 * a and abs(mag[r, i] - a) <= 1e-12 * a, (in_first, r, i)
        assert np.abs(got).max() > 1e6
    # an integer delay and no slope: a shifted copy, exactly
    got = retime.model(x, [(2, 3.0, 0.0), (0, -400.0, 0.0)], table=retime.table)
    assert np.array_equal(got[0][:297], xf[2][3:]) and not got[0][297:].any() and not got[1].any()
    with pytest.raises(ValueError):
        retime.model(x, [(0, 0.0, 0.0)], out_first=2 ** 38 - 5, n_out=6)
    with pytest.raises(ValueError):
        retime.model(x, [(0, 0.0, 2.0 ** -8)])


def test_retimed_rows_against_the_analytic_signal(retime, link):
    """A row rendered by the link's law at (lead, ppm), read along `undo(lead, ppm, target)`, is link.signal at the target
    lead and ppm 0: away from the buffer's ends and at least 12 samples from every symbol boundary the worst error stays at
    or below 2e-4 of the peak amplitude * sqrt 2, the bar of the array interpolator (tests/test_array_cpu.py), whose own
    worst is 1.02e-4.  Measured here: 1.01e-4 at the worst of the five clock offsets; the blend between table rows adds at
    most 1.1e-5 against coefficients evaluated at the exact fraction."""
    amp, text = 2000.0, "Hi!"
    period = 1155.0 / 44100.0 * FS                      # one symbol in samples of fs_out
    n = 48 * 2048
    j = np.arange(n, dtype=np.float64)
    worst = 0.0
    for lead, ppm, target in ((3000.25, 40.0, 2990.0), (3011.7, -75.0, 3000.25), (2950.3, 200.0, 3000.0), (3100.0, 1000.0, 3000.5),
                              (3000.0, -1000.0, 3050.125)):
        x = link.signal(text, lead, amp, ppm, n, FS)
        d, s = retime.undo(lead, ppm, target)
        y = retime.model(x[None, :], [(0, d, s)], table=retime.table)[0]
        ref = link.signal(text, target, amp, 0.0, n, FS)
        assert np.abs(ref).max() > amp
        phase = np.mod(j - target, period)
        pos = j + d + s * j
        keep = (np.minimum(phase, period - phase) >= 12.0) & (j >= 32) & (j < n - 32) & (pos >= 32) & (pos < n - 32)
        err = float(np.abs(y - ref)[keep].max()) / (amp * 2 ** 0.5)
        print("lead %-8r ppm %-7r -> lead %-9r worst |model - analytic| / peak %.3g over %d samples (%d sounding)"
              % (lead, ppm, target, err, keep.sum(), (ref[keep] != 0).sum()))
        assert (ref[keep] != 0).sum() > 20000
        worst = max(worst, err)
    assert worst <= 2e-4, worst


def test_fit_line_survives_cycle_slips_and_silent_windows(retime):
    c = 4096.0 + 8192.0 * np.arange(7)
    truth = (12.345, -63e-6)
    d = truth[0] + truth[1] * c
    D, s, kept = retime.fit_line(c, d, np.ones(7, bool))
    assert abs(D - truth[0]) <= 1e-9 and abs(s - truth[1]) <= 1e-14 and kept.all()
    for bad in ((0,), (6,), (3,), (0, 6), (1, 5)):
        for slip in (4.46, -4.46):
            e = d.copy()
            e[list(bad)] += slip
            D, s, kept = retime.fit_line(c, e, np.ones(7, bool))
            assert abs(D - truth[0]) <= 1e-9 and abs(s - truth[1]) <= 1e-14 and sorted(np.nonzero(~kept)[0]) == list(bad), (bad, slip)
    e = d.copy()
    e[[0, 1]] = (99.0, -99.0)                                    # windows without a signal hold anything
    usable = np.ones(7, bool)
    usable[[0, 1]] = False
    D, s, kept = retime.fit_line(c, e, usable)
    assert abs(D - truth[0]) <= 1e-9 and abs(s - truth[1]) <= 1e-14 and not kept[:2].any() and kept[2:].all()
    with pytest.raises(ValueError):
        retime.fit_line(c, d, np.arange(7) == 3)


def test_drift_model_on_the_modem_signal(retime, link):
    """Eight microphones with clocks of their own (ppm uniform in +-50, leads within +-30 samples) at +14 dB, 104 blocks,
    in float64 (drift_model over align.delays_model, two passes over windows of 4 blocks, lags -64 .. 64): every slope within 1 ppm of the
    truth (0.2 samples over the transmission, 1 / 20 of a carrier cycle: DESIGN.md section 14) and every delay at the
    transmission's centre within 0.01 samples, the bar of tests/test_align_cpu.py."""
    rng = np.random.default_rng(14)
    nb, amp, M = 104, 2000.0, 8
    n = nb * N
    sigma = amp / 10.0 ** (14.0 / 20.0)
    text = "Hello, World"
    base = 4000.0
    ppm = rng.uniform(-50.0, 50.0, size=M)
    lead = base + rng.uniform(-30.0, 30.0, size=M)
    x = np.stack([link.signal(text, lead[m], amp, ppm[m], n, FS) + sigma * rng.standard_normal(n) for m in range(M)]).astype(np.float32)
    sounding = np.nonzero(link.signal(text, lead[0], amp, ppm[0], n, FS))[0]
    centre = 0.5 * (sounding[0] + sounding[-1])
    print("transmission: samples %d .. %d of %d" % (sounding[0], sounding[-1], n))
    assert sounding[-1] - sounding[0] > 150000
    lines, fits = retime.drift_model(x, [list(range(M))])
    assert lines[0] == (0, 0.0, 0.0) and fits[0] is None and [ln[0] for ln in lines] == list(range(M))
    worst_s = worst_d = 0.0
    for m in range(1, M):
        d, s = retime.undo(lead[m], ppm[m], lead[0], ppm[0])
        _, got_d, got_s = lines[m]
        es, ed = abs(got_s - s) * 1e6, abs((got_d + got_s * centre) - (d + s * centre))
        print("  microphone %d: slope %+8.3f ppm (truth %+8.3f), delay at the centre %+8.4f (truth %+8.4f); windows %r"
              % (m, got_s * 1e6, s * 1e6, got_d + got_s * centre, d + s * centre, fits[m]))
        worst_s, worst_d = max(worst_s, es), max(worst_d, ed)
    print("drift_model, +14 dB, 7 pairs: worst |slope error| %.4f ppm, worst |delay error| at the centre %.4f samples" % (worst_s, worst_d))
    assert worst_s <= 1.0, worst_s
    assert worst_d <= 0.01, worst_d


def test_kernels_are_gfx950_without_spills_or_scratch(retime, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    if not os.path.exists(retime.LIB_PATH):
        pytest.skip("libuchirp_retime.so not built")
    monkeypatch.setattr(kr, "LIB", retime.LIB_PATH)
    ks = kr._kernels(tmp_path)
    assert len(ks) == 2 and all("retime_kernel" in k for k in ks), sorted(ks)      # f32, i32
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            assert e["private_segment_fixed_size"] == 0, (k, e)
            assert e["vgpr_count"] <= 128, (k, e)     # 4 waves per SIMD (100)
            assert e["group_segment_fixed_size"] == 257 * 16 * 4 + 4 * 272 * 4, (k, e)     # the table and four wave-private windows
