"""CPU tests of the band-weighted correlator (include/uchirp_wcorr.h, libuchirp_wcorr.so, uchirp/wcorr.py): the boundary,
the band weights against their formula and the header's tail table, the float64 model against a brute-force restatement of
the definition, the float32 emulation against the model (the yardstick of UC_WCORR_ERROR_C), impulse rows that pin every
bin's place, uc_wcorr_peak against uc_xcorr_peak bit for bit, the effect the library exists for (the right carrier cycle at
-12 dB, on the model), the precondition of the GPU delay test, and what the compiler made of the kernels."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import wcorr_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ultrasonic-communication_amd")
HEADER = os.path.join(ROOT, "include", "uchirp_wcorr.h")


@pytest.fixture(scope="module")
def wcorr():
    from uchirp import wcorr as m
    m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def xcorr():
    from uchirp import xcorr as m
    m.build()
    m.lib()
    return m


# ---- boundary

def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_wcorr_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(wcorr, xcorr, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_wcorr.h"\nint main(void) { return sizeof(uc_wcorr_pair) == 8 && sizeof(uc_wcorr_peak_t) == 32 && '
                   'UC_WCORR_ABI_VERSION == %d && UC_WCORR_DTYPE_I32 == %d && UC_WCORR_DTYPE_F32 == %d && UC_WCORR_MAX_LAG == %d && '
                   'UC_WCORR_POINTS == %d && UC_WCORR_GROUP == %d && UC_WCORR_BINS == %d && UC_WCORR_ERROR_C == %d && UC_WCORR_NO_PEAK == %d && '
                   'UC_WCORR_AT_EDGE == %d ? 0 : 1; }\n'
                   % (wcorr.ABI_VERSION, wcorr.DTYPE_I32, wcorr.DTYPE_F32, wcorr.MAX_LAG, wcorr.POINTS, wcorr.GROUP, wcorr.BINS, wcorr.ERROR_C,
                      wcorr.NO_PEAK, wcorr.AT_EDGE))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    assert C.sizeof(wcorr.WcorrPair) == 8 == wcorr.PAIR_DTYPE.itemsize and C.sizeof(wcorr.WcorrPeak) == 32
    # the peak record, the pair and the shared constants are those of the wide-lag correlator
    assert [(f[0], getattr(wcorr.WcorrPeak, f[0]).offset) for f in wcorr.WcorrPeak._fields_] == \
        [(f[0], getattr(xcorr.XcorrPeak, f[0]).offset) for f in xcorr.XcorrPeak._fields_]
    assert (wcorr.MAX_LAG, wcorr.POINTS, wcorr.GROUP, wcorr.NO_PEAK, wcorr.AT_EDGE) == (xcorr.MAX_LAG, xcorr.POINTS, xcorr.GROUP, xcorr.NO_PEAK, xcorr.AT_EDGE)
    assert wcorr.BINS == wcorr.POINTS // 2 + 1 and wcorr.GUARD + 384 == wcorr.MAX_LAG
    decl = _declared_functions()
    assert len(decl) == 7, decl
    L = wcorr.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(wcorr.EXPORTS) == decl
    exported = subprocess.run(["nm", "-D", "--defined-only", wcorr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (uc_[a-z0-9_]+)", exported))) == decl
    assert L.uc_wcorr_abi_version() == 1 == wcorr.ABI_VERSION


def test_wcorr_library_stands_alone(wcorr):
    """libuchirp_wcorr.so links none of the other eleven libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", wcorr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", wcorr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_correlator(wcorr):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = wcorr.lib().uc_wcorr_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in wcorr.lib().uc_wcorr_last_error()
    with pytest.raises(wcorr.WcorrError):
        wcorr.Wcorr()


def build_host(tmp_path):
    import uchirp
    from uchirp import scene, wcorr
    for m in (uchirp, scene, wcorr):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    exe = str(tmp_path / "host_wcorr")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_wcorr.c"), "-o", exe, "-L" + PKG, "-luchirp_wcorr", "-luchirp_scene",
                           "-luchirp", "-Wl,-rpath," + PKG])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(wcorr, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "uc_wcorr_abi_version 1 (header 1)" in out.stdout and "uc_wcorr_create: -19" in out.stdout and "no CPU path" in out.stdout
    assert "w[380] 0.0, w[406] 0.4" in out.stdout and "w[446] 1.0, w[530] 0.0; tail beyond guard 128: 1.82e-05" in out.stdout
    assert "f_lo > f_hi refused" in out.stdout and "delay 0.000, height 3.000" in out.stdout


def test_host_translation_unit_is_clean_under_the_sanitizers(wcorr):
    """`make sanitize-wcorr`: csrc/uc_wcorr_api.cpp and tests/cpp/san_wcorr.cpp under ASan + UBSan, a stand-alone program on the CPU."""
    out = subprocess.run(["make", "-C", PKG, "sanitize-wcorr"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert re.search(r"san_wcorr: \d+ tables, \d+ peaks, \d+ refusals", out.stdout)


# ---- the band weights

def _formula(fs, f_lo, f_hi, taper):
    f = np.arange(1025, dtype=np.float64) * fs / 2048.0
    d = np.where(f < f_lo, f_lo - f, np.where(f > f_hi, f - f_hi, 0.0))
    with np.errstate(all="ignore"):
        edge = np.cos(0.5 * np.pi * d / taper) ** 2 if taper > 0 else np.zeros_like(d)
    return np.where(d == 0.0, 1.0, np.where(d < taper, edge, 0.0))


def test_band_weights_are_the_formula_and_the_tail_table_holds(wcorr):
    for fs, lo, hi, taper in ((wu.FS,) + wu.BAND, (wu.FS, 16000.0, 19000.0, 0.0), (48000.0, 0.0, 5000.0, 2500.0), (wu.FS, 17000.0, 17000.0, 300.0),
                              (wu.FS, 30000.0, 50000.0, 4000.0), (wu.FS, 17000.5, 17000.5, 0.0)):
        w, tail = wcorr.band_weights(fs, lo, hi, taper, 128)
        want = _formula(fs, lo, hi, taper)
        assert w.dtype == np.float32 and w.shape == (1025,)
        assert np.array_equal(w, want.astype(np.float32)) or np.abs(w - want).max() <= 2.0 ** -24, (fs, lo, hi, taper)   # cos of two libraries
        # the tail by its definition, from the rounded weights
        h = np.fft.irfft(w.astype(np.float64), 2048)
        dist = np.minimum(np.arange(2048), 2048 - np.arange(2048))
        e = float((h ** 2).sum())
        assert abs(tail - (float((h[dist > 128] ** 2).sum()) / e if e else 0.0)) <= 1e-9 * max(tail, 1e-12) + 1e-18, (fs, lo, hi, taper, tail)
    brick = wcorr.band_weights(wu.FS, 16000.0, 19000.0, 0.0, 0)[0]
    assert set(np.unique(brick)) == {0.0, 1.0} and brick.sum() == 79                      # bins 420 .. 498
    assert not wcorr.band_weights(wu.FS, 17000.5, 17000.5, 0.0, 0)[0].any()                # between two bins: a wall around nothing
    # the header's table, to 5 % relative
    for guard, share in ((0, 0.89), (32, 1.6e-2), (64, 1.8e-3), (128, 1.8e-5), (256, 3.6e-7)):
        tail = wcorr.band_weights(wu.FS, *wu.BAND, guard=guard)[1]
        print("guard %3d: tail share %.4g (table %.2g)" % (guard, tail, share))
        assert abs(tail - share) <= 0.05 * share, (guard, tail)
    for guard in (1024, 1025, 2 ** 32 - 1):
        assert wcorr.band_weights(wu.FS, *wu.BAND, guard=guard)[1] == 0.0
    assert wcorr.band_weights(wu.FS, *wu.BAND, guard=1023)[1] > 0.0
    lib = wcorr.lib()
    buf = np.zeros(1025, np.float32)
    tail = C.c_double()

    def call(fs=wu.FS, lo=16000.0, hi=19000.0, taper=1000.0, out=buf.ctypes.data, t=C.byref(tail)):
        return lib.uc_wcorr_band_weights(fs, lo, hi, taper, 128, out, t)

    assert call() == 0 and call(t=None) == 0 and call(taper=0.0) == 0
    for name, kw in (("f_lo > f_hi", dict(lo=19000.0, hi=16000.0)), ("taper < 0", dict(taper=-1.0)), ("fs NaN", dict(fs=np.nan)), ("f_lo NaN", dict(lo=np.nan)),
                     ("f_hi NaN", dict(hi=np.nan)), ("taper NaN", dict(taper=np.nan)), ("f_hi inf", dict(hi=np.inf)), ("fs 0", dict(fs=0.0)),
                     ("f_lo < 0", dict(lo=-1.0)), ("w_out NULL", dict(out=None))):
        assert call(**kw) == -errno.EINVAL, name
        assert lib.uc_wcorr_last_error(), name
    with pytest.raises(wcorr.WcorrError):
        wcorr.band_weights(wu.FS, 19000.0, 16000.0)


# ---- the model

def _brute(xf, ref, mic, first, n, L, g, h):
    """the definition with loops: per segment the 2048-point circular correlation by dot products, convolved circularly
    with h, the values g .. g + 2 L"""
    P, Lp = 2048, L + g
    S = P - 2 * Lp
    n_in = xf.shape[1]
    out = np.zeros(2 * L + 1)
    for i0 in range(0, n, S):
        cnt = min(S, n - i0)
        a = np.zeros(P)
        a[:cnt] = xf[ref, first + i0:first + i0 + cnt]
        b = np.zeros(P)
        for t in range(cnt + 2 * Lp):
            j = first + i0 - Lp + t
            if 0 <= j < n_in:
                b[t] = xf[mic, j]
        bb = np.concatenate([b, b])
        c = np.array([np.dot(a, bb[t:t + P]) for t in range(P)])            # c_s[t] = sum_i a[i] b[(i + t) mod P]
        for l in range(2 * L + 1):
            t = l + g
            out[l] += sum(h[u] * c[(t - u) % P] for u in range(P))
    return out


def test_model_is_the_definition(wcorr, xcorr):
    rng = np.random.default_rng(12)
    x = rng.integers(-2 ** 27, 2 ** 27, size=(2, 2048 + 300)).astype(np.int32)   # mostly no floats: the cast rounds
    xf = x.astype(np.float32).astype(np.float64)
    tables = dict(wu.weight_tables())
    for first, n, L, g, name in ((0, 2348, 3, 0, "band"), (5, 2300, 2, 100, "random"), (1, 2347, 1, 511, "random"), (300, 2048, 4, 128, "band"),
                                 (7, 1, 2, 0, "one-hot 1"), (0, 2042, 3, 0, "one-hot 1024")):
        w = tables[name]
        h = wcorr.impulse_response(w)
        # h by its formula
        k = np.arange(2048)
        W = np.concatenate([w, w[-2:0:-1]]).astype(np.float64)
        for t in (0, 1, 5, 1024, 2047):
            assert abs(h[t] - (W * np.cos(2.0 * np.pi * k * t / 2048.0)).sum() / 2048.0) <= 1e-12 * np.abs(W).sum() / 2048.0
        got = wcorr.model(x, [(0, 1), (1, 1)], first, n, L, g, w)
        E = wcorr.model(x, [(0, 1), (1, 1)], first, n, L, g, w, magnitude=True)
        assert got.shape == (2, 2 * L + 1) and np.array_equal(E, xcorr.model(x, [(0, 1), (1, 1)], first, n, L + g, magnitude=True))
        for i, (ref, mic) in enumerate([(0, 1), (1, 1)]):
            want = _brute(xf, ref, mic, first, n, L, g, h)
            assert np.abs(got[i] - want).max() <= 1e-12 * np.abs(w).max() * E[i], (first, n, L, g, name, i)
    # ones: the plain correlation, whatever the guard (the transforms' rounding: some 1e-15 of E_p)
    for first, n, L, g in ((3, 2045, 1, 0), (0, 2348, 64, 0), (7, 2000, 64, 128), (100, 2248, 200, 312), (0, 2348, 512, 0)):
        for weights in (None, np.ones(1025, np.float32)):
            got = wcorr.model(x, [(0, 1), (1, 0)], first, n, L, g, weights)
            E = xcorr.model(x, [(0, 1), (1, 0)], first, n, L + g, magnitude=True)
            assert np.abs(got - xcorr.model(x, [(0, 1), (1, 0)], first, n, L)).max() <= 1e-12 * E.min(), (first, n, L, g)
    wm = wcorr.windows_model(x, [(0, 1)], 3, 500, 300, 4, 8, 16, tables["band"])
    assert wm.shape == (1, 4, 17) and np.array_equal(wm[0, 2], wcorr.model(x, [(0, 1)], 603, 500, 8, 16, tables["band"])[0])
    for bad in (dict(max_lag=0), dict(max_lag=385, guard=128), dict(guard=-1), dict(weights=np.ones(1024)), dict(n=3000),
                dict(weights=np.full(1025, np.nan))):
        with pytest.raises(ValueError):
            wcorr.model(x, [(0, 1)], **bad)


def test_ideal_model_is_the_linear_filter_and_the_guard_closes_the_gap(wcorr, xcorr):
    """`ideal_model` with ones is the plain correlation; with the band weights `model` comes closer to it as the guard
    grows (the header's tail), on a pair of the effect test."""
    x, pairs, _ = wu.delay_pairs(4, -12.0)
    one = wcorr.ideal_model(x, pairs[:1], wu.DELAY_FIRST, wu.DELAY_WINDOW, 64, None)
    E = xcorr.model(x, pairs[:1], wu.DELAY_FIRST, wu.DELAY_WINDOW, 64, magnitude=True)
    assert np.abs(one - xcorr.model(x, pairs[:1], wu.DELAY_FIRST, wu.DELAY_WINDOW, 64)).max() <= 1e-12 * E[0]
    w = wu.band()
    ideal = wcorr.ideal_model(x, pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, 64, w)
    dev = {}
    for g in (0, 128):
        m = wcorr.model(x, pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, 64, g, w)
        dev[g] = float(np.median(np.abs(m - ideal).max(axis=1) / np.abs(ideal).max(axis=1)))
    print("largest deviation from the ideal as a share of the peak, median of 4 pairs at -12 dB: guard 0 %.2g, guard 128 %.2g" % (dev[0], dev[128]))
    assert dev[128] < 1e-3 and dev[128] < 0.1 * dev[0]


def test_emulation_stays_within_the_error_form(wcorr):
    """The float32 emulation (pocketfft, complex64) of the definition against the float64 model, as a multiple of
    2^-24 max|w| E_p, on the GPU tests' rows and weight tables.  UC_WCORR_ERROR_C is four times the worst ratio printed
    here, rounded up: measured 2.22, so 9."""
    data = wu.mics()
    pairs = wu.PAIRS[:3]
    worst = 0.0
    shapes = ((1, 0, 0, None), (64, 0, 3, 1921), (64, 128, 0, 4000), (65, 63, 5, 6000), (200, 56, 1, 4105), (384, 128, 0, None), (512, 0, 7, 4097),
              (1, 511, 3, 5000))
    for key in ("f32", "i32"):
        for i, (L, g, first, n) in enumerate(shapes):
            for name, w in [(None, None)] + wu.weight_tables()[:2] + [wu.weight_tables()[2 + (i % len(wu.ONE_HOT_BINS))]]:
                want = wcorr.model(data[key], pairs, first, n, L, g, w)
                E = wcorr.model(data[key], pairs, first, n, L, g, w, magnitude=True)
                emu = wcorr.emulate32(data[key], pairs, first, n, L, g, w)
                r = wu.error_ratio(emu, want, E, 1.0 if w is None else float(np.abs(w).max()))
                print("%s L %3d guard %3d first %d n %s weights %s: emulation ratio %.3f" % (key, L, g, first, n, name, r))
                worst = max(worst, r)
    print("emulation: worst |emulate32 - model| / (2^-24 max|w| E_p) %.3f; UC_WCORR_ERROR_C = %d" % (worst, wcorr.ERROR_C))
    assert 0.0 < worst and 4.0 * worst <= wcorr.ERROR_C, worst


def test_impulse_rows_give_the_weights_impulse_response(wcorr):
    """Rows with one non-zero sample each: the correlation of a pair is value_ref * value_mic * h[(l - d) mod 2048] with d
    the distance of the two samples and h = irfft(w).  With pseudo-random weights this pins every bin's place."""
    x, places = wu.impulses()
    seen = 0
    for name, w in wu.weight_tables():
        h = np.fft.irfft(w.astype(np.float64), 2048)
        for L, g in ((64, 128), (512, 0), (1, 40), (300, 100)):
            for ref, mic in ((0, 1), (1, 0), (2, 3), (3, 2), (0, 0)):
                d = places[mic][0] - places[ref][0]
                if abs(d) > L + g:                                          # (the microphone's sample lies outside b_s)
                    continue
                seen += 1
                got = wcorr.model(x, [(ref, mic)], 0, None, L, g, w)[0]
                want = places[ref][1] * places[mic][1] * h[(np.arange(-L, L + 1) - d) % 2048]
                scale = abs(places[ref][1] * places[mic][1]) * np.abs(w).max()
                assert np.abs(got - want).max() <= 1e-12 * scale, (name, L, g, ref, mic)
    assert seen == len(wu.weight_tables()) * (5 + 5 + 3 + 5)


# ---- the peak

def _same_bits(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("delay_samples", "height", "runner_up")) and \
        a["lag"] == b["lag"] and a["flags"] == b["flags"]


def test_peak_returns_the_bits_of_uc_xcorr_peak(wcorr, xcorr):
    rng = np.random.default_rng(5)
    rows = []
    for i in range(200):
        L = int(rng.integers(1, 513))
        row = rng.standard_normal(2 * L + 1) * 10.0 ** rng.uniform(-3, 12)
        if i % 7 == 0:
            row = np.round(row / np.abs(row).max() * 3.0)                   # many ties and plateaus
        rows.append(row)
    # the crafted rows of tests/test_xcorr_cpu.py
    rows += [np.array(r) for r in ([5.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.1], [-1.0, -0.5, -0.2, -0.1, -0.3, -0.6, -2.0], [0.0, 2.0, 0.0, -1.0, 0.0, 2.0, 0.0],
                                   [9.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0])]
    w = 2.0 * np.pi / 4.46
    k = np.arange(-512, 513, dtype=np.float64)
    for off in (0.0, 0.25, -0.49, 311.25, -402.5, 499.999, -510.3):
        rows.append(1e9 * np.cos(w * (k - off)))
        rows.append(1e9 * np.cos(w * (k - off)) * np.exp(-0.5 * ((k - off) / 11.0) ** 2))
    flags = set()
    for i, row in enumerate(rows):
        got = wcorr.peak(row)
        assert _same_bits(got, xcorr.peak(row)), i
        flags.add(got["flags"])
    assert flags == {0, wcorr.NO_PEAK, wcorr.AT_EDGE, wcorr.NO_PEAK | wcorr.AT_EDGE}
    assert wcorr.peak_model(rows[-1])["lag"] == wcorr.peak(rows[-1])["lag"]
    lib = wcorr.lib()
    out = wcorr.WcorrPeak()
    ok = np.ones(1025)
    bad = ok.copy()
    bad[900] = np.nan

    def call(row, L, o=out):
        return lib.uc_wcorr_peak(row.ctypes.data_as(C.c_void_p) if row is not None else None, L, C.byref(o) if o is not None else None)

    assert call(ok, 512) == 0
    for name, args in (("nan", (bad, 512)), ("corr NULL", (None, 512)), ("out NULL", (ok, 512, None)), ("L = 0", (ok, 0)), ("L = 513", (ok, 513))):
        assert call(*args) == -errno.EINVAL, name
        assert lib.uc_wcorr_last_error(), name
    assert call(bad, 300) == 0                                              # the value that is not finite lies outside the row


# ---- what the library is for

MEASURED_PLAIN, MEASURED_WEIGHTED = 0.385, 0.870


def test_band_weights_put_the_delay_on_the_right_carrier_cycle_at_minus_12_db(wcorr):
    """200 seeded pairs of `link.model`: one text, two leads that differ by uniform +-40 samples, -12 dB; window 8192,
    L = 64, guard 128; the crest rule on the float64 model of the correlation with weights of one and with the band
    16 .. 19 kHz, 1 kHz cos^2 edges.  The share of pairs whose delay lies within 1 sample of the truth was measured with
    these inputs as 0.385 (ones) and 0.870 (band): a difference of 0.485.  Required: at least half of that, 0.2425 (the
    margin is for a change of seed: with 200 pairs one standard deviation is about 0.035)."""
    x, pairs, truth = wu.delay_pairs(200, -12.0)
    w = wu.band()
    share = []
    for weights in (None, w):
        rows = wcorr.model(x, pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, wu.DELAY_L, wu.DELAY_GUARD, weights)
        share.append(float(np.mean([abs(wcorr.peak_model(r)["delay_samples"] - d) <= 1.0 for r, d in zip(rows, truth)])))
    print("within 1 sample of the truth at -12 dB, 200 pairs: ones %.3f, band weights %.3f" % tuple(share))
    assert share[1] - share[0] >= 0.5 * (MEASURED_WEIGHTED - MEASURED_PLAIN) >= 0.1, share


def test_the_gpu_delay_tests_pairs_have_a_clear_crest(wcorr):
    """The precondition of the GPU delay test: at 0 dB the model's runner-up stays below 0.99 in every one of its 32 pairs,
    so an error of the size of the error form cannot move the estimate to another crest."""
    x, pairs, truth = wu.delay_pairs(32, 0.0, 1000)
    rows = wcorr.model(x, pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, wu.DELAY_L, wu.DELAY_GUARD, wu.band())
    pk = [wcorr.peak_model(r) for r in rows]
    worst = max(p["runner_up"] for p in pk)
    print("32 pairs at 0 dB: greatest runner-up %.4f, greatest |delay - truth| %.3f" % (worst, max(abs(p["delay_samples"] - d) for p, d in zip(pk, truth))))
    assert worst < 0.99 and all(p["flags"] == 0 and abs(p["delay_samples"] - d) <= 1.0 for p, d in zip(pk, truth))


# ---- the kernels

def test_kernels_are_gfx950_without_spills_and_keep_the_trackers_occupancy(wcorr, tmp_path, monkeypatch):
    """The code object's metadata: no spilled register, no scratch, and -- with a thread's sixteen weights resident over the
    unit loop -- registers and LDS that let a CU hold as many workgroups as it holds of track_kernel."""
    import test_kernel_resources as kr
    from uchirp import track
    track.build()

    def kernels(path, sub):
        monkeypatch.setattr(kr, "LIB", path)
        d = tmp_path / sub
        d.mkdir()
        return kr._kernels(d)

    def workgroups_per_cu(e):
        # 2 waves of a workgroup on 2 of the 4 SIMDs; a SIMD has 512 VGPRs a lane (allocated in eights), a CU 160 KiB of LDS
        waves_per_simd = 512 // (-(-(e["vgpr_count"] + e.get("agpr_count", 0)) // 8) * 8)
        return min(waves_per_simd * 4 // 2, (160 * 1024) // e["group_segment_fixed_size"])

    ks = kernels(wcorr.LIB_PATH, "wcorr")
    corr = {k: v for k, v in ks.items() if "wcorr_kernel" in k}
    sums = {k: v for k, v in ks.items() if "wcorr_sum_kernel" in k}
    assert len(ks) == 3 and len(corr) == 2 and len(sums) == 1, sorted(ks)         # f32, i32; the sum in double
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            assert e["private_segment_fixed_size"] == 0, (k, e)
    tk = {k: v for k, v in kernels(track.LIB_PATH, "track").items() if "track_kernel" in k}
    assert len(tk) == 2
    have = min(workgroups_per_cu(v[0]) for v in tk.values())
    for k, v in corr.items():
        assert v[0]["vgpr_count"] <= 256, (k, v)      # the budget of 2 waves per SIMD
        assert v[0]["group_segment_fixed_size"] == (2 * 2 * 2048 + 2 * 256 + 2 * 128) * 4, (k, v)
        print("%s: %d VGPRs, %d workgroups per CU (track_kernel: %d)" % (k[:60], v[0]["vgpr_count"], workgroups_per_cu(v[0]), have))
        assert workgroups_per_cu(v[0]) >= have == 4, (k, v)
    for k, v in sums.items():
        assert v[0]["vgpr_count"] <= 32 and v[0]["group_segment_fixed_size"] == 0, (k, v)
