"""CPU tests of the up-converter (include/uchirp_duc.h, libuchirp_duc.so, uchirp/duc.py): the boundary, the carrier's tables
against the down-converter's, the library's plain-C functions against the numpy definition bit for bit (denormals, -0, NaN and
Inf included), cuts at 32- and 64-bit positions, the int16 stage, the refusals, the reference's chirp_x_carrier, the float32
definition against the float64 model, the loop through the down-converter's arithmetic, the transmitter's symbol from base
band, and what the compiler made of the kernels.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import duc_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_duc.h")
PIN_BOUND = 1.3e-5            # of the amplitude: the down-converter's asserted bound for the same carrier (tests/test_ddc_cpu.py)


@pytest.fixture(scope="module")
def duc():
    from uchirp import duc as m
    m.build()
    m.lib()
    return m


# ---- the boundary

def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_duc_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(duc, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_duc.h"\nint main(void) { return UC_DUC_ABI_VERSION == %d && UC_DUC_IN_IQ == %d && UC_DUC_IN_I == %d && '
                   'UC_DUC_OUT_F32 == %d && UC_DUC_OUT_I16 == %d && UC_DUC_MAX_PHASE_TAPS == %d && UC_DUC_MAX_INTERP == %d && UC_DUC_MAX_TAPS == %d && '
                   'UC_DUC_MAX_SETS == %d && UC_DUC_MAX_CHAN == %d && UC_DUC_STATE_SAMPLES == %d && UC_DUC_TABLE_WORDS == %d ? 0 : 1; }\n'
                   % (duc.ABI_VERSION, duc.IN_IQ, duc.IN_I, duc.OUT_F32, duc.OUT_I16, duc.MAX_PHASE_TAPS, duc.MAX_INTERP, duc.MAX_TAPS, duc.MAX_SETS,
                      duc.MAX_CHAN, duc.STATE_SAMPLES, duc.TABLE_WORDS))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    decl = _declared_functions()
    assert len(decl) == 10, decl
    L = duc.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(duc.EXPORTS) == decl
    assert L.uc_duc_abi_version() == 1 == duc.ABI_VERSION


def test_duc_library_stands_alone(duc):
    """libuchirp_duc.so links none of the other libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", duc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", duc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_up_converter(duc):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = duc.lib().uc_duc_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in duc.lib().uc_duc_last_error()
    with pytest.raises(duc.DucError):
        duc.Duc()


def build_host(tmp_path):
    import uchirp
    from uchirp import duc
    for m in (uchirp, duc):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_duc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_duc.c"), "-o", exe, "-L" + libdir, "-luchirp_duc", "-luchirp",
                           "-Wl,-rpath," + libdir])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(duc, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0
    assert "uc_duc_abi_version 1 (header 1)" in out.stdout and "uc_duc_create: -19" in out.stdout and "no CPU path" in out.stdout
    assert "format 7 refused" in out.stdout
    assert "a step held over 4 outputs: 1.000000 1.000000 2.000000 2.000000 3.000000 ... 4.000000 (state's last 4.000000)" in out.stdout


# ---- the carrier

def test_tables_are_the_down_converter_s_bits(duc):
    from uchirp import ddc
    ddc.build()
    for a, b in zip(duc.tables(), ddc.tables()):
        assert a.shape == b.shape == (1024, 2) and a.dtype == np.float32 and np.array_equal(du.bits(a), du.bits(b))
    rng = np.random.default_rng(41)
    ph = rng.integers(0, 2 ** 32, size=1 << 16, dtype=np.uint64).astype(np.uint32)
    for a, b in zip(duc.carrier32(ph), ddc.carrier32(ph)):
        assert np.array_equal(du.bits(a), du.bits(b))
    c, s = duc.carrier32(np.zeros(4, np.uint32))
    assert du.bits(c).tolist() == [0x3F800000] * 4 and du.bits(s).tolist() == [0] * 4          # step 0, phase 0: exactly (1, +0)
    assert duc.lib().uc_duc_carrier_tables(None, None) == -errno.EINVAL
    assert duc.step_of(25000.0, 100000.0) == 2 ** 30 and duc.fma32 is ddc.fma32


# ---- the plain C functions

@pytest.mark.parametrize("out", ("f32", "i16"))
@pytest.mark.parametrize("n_chan", (1, 3, 16))
@pytest.mark.parametrize("fmt", ("iq", "i"))
@pytest.mark.parametrize("K,L", du.KL)
def test_filter_row_and_sum_row_are_the_definition_bit_for_bit(duc, K, L, fmt, n_chan, out):
    """uc_duc_filter_row + uc_duc_sum_row against emulate32: outputs, states and clip counts, on noise, on a denormal
    impulse, on NaN and +-Inf and on zeros of both signs, from states that hold noise and denormals, at a `first` whose output
    index passes 2^32 inside the row, with two tap sets."""
    n = 150 if L < 8 else (40 if L == 8 else 9)
    x, st0 = du.inputs(fmt, n), du.states(fmt)
    sets = np.stack([du.taps_of(K, L), du.taps_of(K, L, 1)])
    rows = 5
    ch = du.channels(rows, n_chan, 2)
    first = du.first_of(L)
    want, want_st, want_clip = duc.emulate32(sets, x, L, first, n_chan, *ch, state=st0, in_format=fmt, out=out)
    assert want.shape == (rows, n * L) and (out == "i16" or np.isfinite(want).all())
    states = {}
    for r in range(rows):
        ys = []
        for j in range(n_chan):
            s = r * n_chan + j
            y, st = duc.filter_row(sets[ch[1][s]], x[ch[0][s]], L, first, ch[2][s], ch[3][s], st0[ch[0][s]], fmt)
            ys.append(y)
            states[int(ch[0][s])] = st
        got, clipped = duc.sum_row(np.stack(ys), out)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32 if out == "f32" else np.int16), want[r].view(np.uint32 if out == "f32" else np.int16)), r
        assert clipped == want_clip[r], r
    for src, st in states.items():
        assert np.array_equal(du.bits(st), du.bits(want_st[src])), src
    if (K, L, fmt, n_chan, out) == (128, 1, "i", 1, "f32"):
        imp = want[0]                                                             # output row 0 reads the impulse row
        tiny = np.finfo(np.float32).tiny
        reached = int(((np.abs(imp) < tiny) & (imp != 0)).sum())
        print("128 taps: the 1e-39 impulse leaves %d denormal outputs" % reached)
        assert reached >= 100                                                     # a flushing device would show zeros there


def test_minus_zero_needs_the_tap_count(duc):
    """-0 out of a -0 product: samples of -1e-30 against the tap 1e-30 round to -0; the same set padded with a zero tap gives
    +0 there, in the definition and in the C function alike: K is part of the definition.  One channel is y0 itself: the sum
    adds no +0."""
    one, padded, x = du.minus_zero_case()
    for fn in (lambda h: duc.emulate32(h, x, 1, in_format="i")[0][0], lambda h: duc.sum_row(duc.filter_row(h, x, 1, in_format="i")[0][None])[0]):
        a, b = fn(one), fn(padded)
        assert (du.bits(a[1::2]) == 0x80000000).all() and (du.bits(a[0::2]) == 0).all()
        assert (du.bits(b) == 0).all()
    # with a Q chain: (ai c) + (aq s) = (-0 x 1) + (+0 x +0) = +0
    z = (x + 0j).astype(np.complex64)
    assert (du.bits(duc.emulate32(one, z, 1)[0][0]) == 0).all()


# ---- cuts and positions

@pytest.mark.parametrize("K,L", ((27, 1), (5, 3), (32, 64)))
def test_cuts_give_the_bits_of_one_call(duc, K, L):
    """One call of 600 samples against calls of 1, 5, 127, 128, 129 and the rest, at first = 0, 7, 2^32 div L - 3 and 2^63 div L -
    4096: the same bits, the same final state and the same clip count, from emulate32 and from the C functions."""
    rng = np.random.default_rng(43)
    n = 600
    x = (rng.standard_normal((2, 2 * n)) * 9000.0).astype(np.float32)
    st0 = (rng.standard_normal((2, 256)) * 9000.0).astype(np.float32)
    steps, phases = [duc.step_of(17500.0, 78125.0), 0xFFFF1234], [77, 2 ** 31]
    cuts = (1, 5, 127, 128, 129, n - 390)
    assert sum(cuts) == n
    h = du.taps_of(K, L)
    for first in (0, 7, 2 ** 32 // L - 3, 2 ** 63 // L - 4096):
        whole, whole_st, whole_clip = duc.emulate32(h, x, L, first, 2, steps=steps, phases=phases, state=st0, out="i16")
        for fn in ("emulate32", "c"):
            parts, s, a, clip = [], st0, 0, 0
            for c in cuts:
                xs = x[:, 2 * a:2 * (a + c)]
                if fn == "emulate32":
                    y, s, k = duc.emulate32(h, xs, L, first + a, 2, steps=steps, phases=phases, state=s, out="i16")
                    clip += int(k[0])
                else:
                    rows = [duc.filter_row(h, xs[r], L, first + a, steps[r], phases[r], s[r]) for r in range(2)]
                    y, k = duc.sum_row(np.stack([v[0] for v in rows]), "i16")
                    y, s = y[None], np.stack([v[1] for v in rows])
                    clip += k
                parts.append(y)
                a += c
            assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(du.bits(s), du.bits(whole_st)) and clip == whole_clip[0], (first, fn)
    assert duc.lib().uc_duc_span(L) == (2048 // L) * L and duc.lib().uc_duc_span(0) == -errno.EINVAL == duc.lib().uc_duc_span(65)


# ---- the int16 stage

def test_int16_rounds_to_even_clamps_and_counts(duc):
    y = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32766.5, 32767.0, 32767.4, 32767.5, 40000.0, -32768.0, -32768.5, -32769.0, -1e9, np.inf, -np.inf, np.nan,
                  -0.0, 1e-40, 0.49999997], np.float32)
    want = np.array([0, 2, 2, 0, -2, -2, 32766, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, 32767, -32768, 0, 0, 0, 0], np.int16)
    clips = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0])
    got, n = duc.to_int16(y)
    assert np.array_equal(got, want) and n == clips.sum()
    c, k = duc.sum_row(y[None], "i16")
    assert np.array_equal(c, want) and k == clips.sum()
    for i in range(y.size):                                                       # one by one: the count is per value
        assert duc.sum_row(y[None, i:i + 1], "i16")[1] == clips[i] == duc.to_int16(y[i:i + 1])[1], y[i]
    # against a brute-force count on loud noise, with NaN from Inf - Inf among the sums
    rng = np.random.default_rng(45)
    ys = (rng.standard_normal((3, 5000)) * 30000.0).astype(np.float32)
    ys[0, 7], ys[1, 7] = np.inf, -np.inf
    with np.errstate(invalid="ignore"):
        total = (ys[0] + ys[1]) + ys[2]
    brute = sum(1 for v in total if np.isnan(v) or np.rint(v) > 32767 or np.rint(v) < -32768)
    c, k = duc.sum_row(ys, "i16")
    print("int16: %d of 5000 loud sums clipped" % k)
    assert k == brute == duc.to_int16(total)[1] and brute > 500 and np.array_equal(c, duc.to_int16(total)[0]) and c[7] == 0


def test_host_functions_refuse_what_the_header_says(duc):
    L = duc.lib()
    h = du.taps_of(9, 3)
    x = np.zeros(16, np.float32)
    out = np.full(48, 7.0, np.float32)
    st = np.zeros(256, np.float32)
    bad = h.copy()
    bad[26] = np.nan
    inf = h.copy()
    inf[0] = np.inf
    big = np.zeros(2112, np.float32)
    fp = C.POINTER(C.c_float)
    hp, bp, ip, gp, xp, op, sp = (a.ctypes.data_as(t) for a, t in ((h, fp), (bad, fp), (inf, fp), (big, fp), (x, C.c_void_p), (out, fp), (st, fp)))

    def args(taps=hp, k_taps=9, interp=3, in_=xp, fmt=0, n=8, first=0, state=sp, out_=op):
        return (taps, k_taps, interp, in_, fmt, n, first, 0, 0, state, out_)

    for name, a in (("taps NULL", args(taps=None)), ("in NULL", args(in_=None)), ("state NULL", args(state=None)), ("out NULL", args(out_=None)),
                    ("0 taps", args(k_taps=0)), ("129 taps per phase", args(taps=gp, k_taps=129, interp=1)), ("interp 0", args(interp=0)),
                    ("interp 65", args(interp=65)), ("2112 taps", args(taps=gp, k_taps=33, interp=64)), ("format 2", args(fmt=2)), ("format -1", args(fmt=-1)),
                    ("n 0", args(n=0)), ("NaN tap", args(taps=bp)), ("Inf tap", args(taps=ip)), ("(first + n) L > 2^63", args(first=2 ** 63 // 3 - 7)),
                    ("first > 2^63", args(first=2 ** 64 - 1))):
        assert L.uc_duc_filter_row(*a) == -errno.EINVAL and L.uc_duc_last_error(), name
    assert (out == 7.0).all() and not st.any()
    assert L.uc_duc_filter_row(*args(first=2 ** 63 // 3 - 8)) == 0
    rows = (fp * 2)(op, op)
    none = (fp * 2)(op, None)
    res = np.zeros(48, np.float32)
    rp = res.ctypes.data_as(C.c_void_p)
    for name, a in (("y NULL", (None, 2, 8, rp, 0, None)), ("a row NULL", (none, 2, 8, rp, 0, None)), ("out NULL", (rows, 2, 8, None, 0, None)),
                    ("no channels", (rows, 0, 8, rp, 0, None)), ("17 channels", (rows, 17, 8, rp, 0, None)), ("n 0", (rows, 2, 0, rp, 0, None)),
                    ("format 2", (rows, 2, 8, rp, 2, None)), ("format -1", (rows, 2, 8, rp, -1, None))):
        assert L.uc_duc_sum_row(*a) == -errno.EINVAL and L.uc_duc_last_error(), name
    assert not res.any() and L.uc_duc_sum_row(rows, 2, 8, rp, 0, None) == 0
    assert L.uc_duc_create(0, None) == -errno.EINVAL
    for bad_call in (lambda: duc.emulate32(np.zeros(129), x, 1), lambda: duc.emulate32(np.zeros(10), x, 3), lambda: duc.emulate32(h, x, 3, n_chan=17),
                     lambda: duc.emulate32(h, x, 3, out="u8"), lambda: duc.interp_taps(65, 1), lambda: duc.interp_taps(8, 27, cutoff=0.6)):
        with pytest.raises(ValueError):
            bad_call()


# ---- the reference, the model, the loop

def _chirp_case(fs_nominal=44100.0, T=0.0262, A=20000.0, fc=17000.0, f0=-1000.0, f1=1000.0):
    """IQ_modulation.ipynb cell 4 (chirp_x_carrier, updown="up") in float64 on its own time axis linspace(0, T, int(T Fs)),
    whose sample rate is (N - 1) / T: the pass-band signal A cos(2 pi (fc - f) t), f = f0 + k t / 2, and the base-band pair
    I = A cos, Q = A sin of 2 pi f t."""
    n = int(T * fs_nominal)
    t = np.linspace(0.0, T, n)
    k = (f1 - f0) / T
    f = f0 + k * t / 2.0
    theta = 2.0 * np.pi * f * t
    return (n - 1) / T, A * np.cos(2.0 * np.pi * (fc - f) * t), (A * np.cos(theta) + 1j * A * np.sin(theta)).astype(np.complex64)


def test_reference_pin_chirp_x_carrier(duc):
    """The reference's chirp_x_carrier (Fs 44 100, T 0.0262, A 20 000, carrier 17 000, +-1000 Hz) from its base-band pair with
    L = 1 and one tap of 1: emulate32 within 1.3e-5 A of it, the down-converter's asserted bound for the same carrier (2 pi /
    2^20 from the dropped phase bits plus float rounding and the step's quantisation).  Measured here: 5.76e-6 A.  The same row
    through `to_int16` equals astype(int16) of the model within 1 LSB (truncation against rounding)."""
    A = 20000.0
    fs, want, z = _chirp_case()
    assert want.size == 1155 and abs(fs - 1154 / 0.0262) < 1e-9
    got, _, _ = duc.emulate32([1.0], z, 1, steps=[duc.step_of(17000.0, fs)])
    err = np.abs(got[0].astype(np.float64) - want).max() / A
    print("chirp_x_carrier: |emulate32 - reference| = %.3g of A" % err)
    assert err <= PIN_BOUND
    pcm, clipped = duc.to_int16(got[0])
    lsb = np.abs(pcm.astype(np.int64) - want.astype(np.int16).astype(np.int64)).max()
    print("chirp_x_carrier as int16: %d LSB from astype(int16) of the model, %d clipped" % (lsb, clipped))
    assert lsb <= 1 and clipped == 0
    assert np.array_equal(duc.filter_row([1.0], z, 1, step=duc.step_of(17000.0, fs))[0], got[0])


def test_definition_against_the_float64_model(duc):
    """K = 27, L = 8, the Kaiser prototype, 1024 noise pairs, carrier 17.5 kHz at 78 125 Hz: emulate32 against `model` with the
    carrier at the quantised frequency.  Measured on this definition: 5.43e-6 of the output's peak (the phase truncation, up to
    6.0e-6 of a sample, dominates; the roundings of the chains grow with K); asserted at three times that, 1.63e-5."""
    rng = np.random.default_rng(46)
    h = duc.interp_taps(8, 27)
    z = ((rng.standard_normal(1024) + 1j * rng.standard_normal(1024)) * 5000.0).astype(np.complex64)
    step = duc.step_of(17500.0, 78125.0)
    got, _, _ = duc.emulate32(h, z, 8, steps=[step])
    want = duc.model(h, z, 8, step=step)
    loose = duc.model(h, z, 8, freq=17500.0, fs=78125.0)
    peak = np.abs(want).max()
    err, moved = np.abs(got[0] - want).max() / peak, np.abs(loose - want).max() / peak
    print("K 27, L 8: |emulate32 - model| = %.3g of the peak %.1f; the unquantised carrier moves the model by %.3g" % (err, peak, moved))
    assert got.shape == (1, 8192) and h.shape == (216,) and abs(h.sum() - 8.0) < 0.02 and peak > 8000.0
    assert err <= 1.63e-5


def test_loop_back_at_the_model_level(duc):
    """emulate32 -> the down-converter's arithmetic (ddc.emulate32: the same carrier, the prototype / L as low-pass, D = L)
    against the float64 models of the same two stages, on a band-limited input (noise through a 0.1 cycles-per-sample
    low-pass), K = 16, L = 8 (the down-converter's 128 taps).  Measured 5.12e-7 of the peak (both stages drop the same phase bits, so the carrier's
    truncation cancels at base band and the roundings are left); asserted at three times that, 1.54e-6.  And the loop returns
    the input: 2 ddc(duc(z)) is z delayed by the two filters' (K L - 1) / L = 15.875 samples.  The test interpolates z linearly
    to that delay, which on a signal band-limited to 0.1 cycles per sample errs by up to (2 pi 0.1)^2 / 8 = 4.9 % of the peak:
    asserted at 5 % (measured 0.96 %); a wrong sign of Q or swapped chains would miss by the peak itself."""
    from uchirp import ddc
    ddc.build()
    rng = np.random.default_rng(47)
    L, K, n = 8, 16, 1024
    h = duc.interp_taps(L, K, cutoff=0.3)
    lp = 0.2 * np.sinc(0.2 * (np.arange(81) - 40.0)) * np.kaiser(81, 9.0)
    z = (np.convolve((rng.standard_normal(n + 80) + 1j * rng.standard_normal(n + 80)) * 5000.0, lp, "valid")).astype(np.complex64)
    step = duc.step_of(17500.0, 78125.0)
    up32, _, _ = duc.emulate32(h, z, L, steps=[step])
    got, _ = ddc.emulate32(h / L, up32[0], L, 0, [step])
    want = ddc.model((h / L).astype(np.float32), duc.model(h, z, L, step=step), L, 0, steps=[step])
    peak = np.abs(want).max()
    err = np.abs(got - want).max() / peak
    d = (K * L - 1) / L                                                           # 15.875 samples: compare at 16 with the input shifted by 1/8
    back = 2.0 * want[32:]
    zi = z.astype(np.complex128)
    frac = zi[16:n - 16] + (zi[17:n - 15] - zi[16:n - 16]) * (16.0 - d)
    dev = np.abs(back - frac).max() / np.abs(zi).max()
    print("loop-back: |emulate32 - model| = %.3g of the peak %.1f; 2 ddc(duc(z)) lies %.3g of the peak from z delayed by %.3f samples" % (err, peak, dev, d))
    assert got.shape == want.shape == (n,) and peak > 2000.0
    assert err <= 1.54e-6
    assert dev <= 0.05


def test_transmitter_s_symbol_from_base_band(duc):
    """uchirp.tx.symbol (the orthogonal chirp 16 -> 19 kHz, A (sin - cos) of 2 pi f t) shifted to base band at 17.5 kHz:
    I = A (sin - cos), Q = A (sin + cos) of 2 pi (f - 17 500) t.  The up-converter (L = 1, one tap of 1) gives the symbol back
    within the pin's bound of its amplitude, A sqrt 2."""
    from uchirp import tx
    for updown in ("up", "down"):
        want = tx.symbol(updown)
        n = want.size
        t = np.linspace(0, tx.T_SYMBOL, n)
        fs = (n - 1) / tx.T_SYMBOL
        k = float(tx.F1 - tx.F0) / tx.T_SYMBOL
        f = tx.F0 + k * t / 2.0 if updown == "up" else tx.F1 - k * t / 2.0
        th = 2.0 * np.pi * (f - 17500.0) * t
        z = (tx.AMPLITUDE * ((np.sin(th) - np.cos(th)) + 1j * (np.sin(th) + np.cos(th)))).astype(np.complex64)
        got, _, _ = duc.emulate32([1.0], z, 1, steps=[duc.step_of(17500.0, fs)])
        err = np.abs(got[0] - want).max() / (tx.AMPLITUDE * np.sqrt(2.0))
        print("tx.symbol(%s) from base band: %.3g of its amplitude" % (updown, err))
        assert err <= PIN_BOUND


# ---- what the compiler made of the kernels

def code_objects(duc, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    monkeypatch.setattr(kr, "LIB", duc.LIB_PATH)
    ks = kr._kernels(tmp_path)
    main = {k: v for k, v in ks.items() if "duc_kernel" in k}
    state = {k: v for k, v in ks.items() if "duc_state_kernel" in k}
    # I/Q, I x f32, i16 x 1, 2, 4, 8 outputs a lane x L divides 256 or not; the states' I/Q, I
    assert len(main) == 32 and len(state) == 2 and len(ks) == 34, sorted(ks)
    for k, v in sorted(ks.items()):
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            print(k, {f: e.get(f) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0 and e["private_segment_fixed_size"] == 0, (k, e)
    for k, v in main.items():
        # four workgroups of four waves on a CU: at most 128 registers, at most a quarter of the CU's 160 KiB of LDS
        e = v[0]
        assert e["max_flat_workgroup_size"] == 256 and e["vgpr_count"] <= 128 and e["group_segment_fixed_size"] <= 160 * 1024 // 4, (k, e)
    return ks


def test_kernels_are_gfx950_without_spills_or_scratch(duc, tmp_path, monkeypatch):
    code_objects(duc, tmp_path, monkeypatch)
