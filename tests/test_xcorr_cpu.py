"""CPU tests of the wide-lag correlator (include/uchirp_xcorr.h, libuchirp_xcorr.so, uchirp/xcorr.py): the boundary, the
float64 model against a brute-force loop, the float32 emulation against the model, the peak rule against the align
library's (the same bits) and on rows of 1025 lags, the estimator's accuracy out to +-500 samples in float64, and what the
compiler made of the kernels."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_xcorr.h")
N = 2048
FS = 78125.0


@pytest.fixture(scope="module")
def xcorr():
    from uchirp import xcorr as m
    m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def align():
    from uchirp import align as m
    m.build()
    m.lib()
    return m


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_xcorr_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(xcorr, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_xcorr.h"\nint main(void) { return sizeof(uc_xcorr_pair) == 8 && sizeof(uc_xcorr_peak_t) == 32 && '
                   'UC_XCORR_ABI_VERSION == %d && UC_XCORR_DTYPE_I32 == %d && UC_XCORR_DTYPE_F32 == %d && UC_XCORR_MAX_LAG == %d && '
                   'UC_XCORR_POINTS == %d && UC_XCORR_GROUP == %d && UC_XCORR_ERROR_C == %d && UC_XCORR_NO_PEAK == %d && '
                   'UC_XCORR_AT_EDGE == %d ? 0 : 1; }\n'
                   % (xcorr.ABI_VERSION, xcorr.DTYPE_I32, xcorr.DTYPE_F32, xcorr.MAX_LAG, xcorr.POINTS, xcorr.GROUP, xcorr.ERROR_C,
                      xcorr.NO_PEAK, xcorr.AT_EDGE))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    assert C.sizeof(xcorr.XcorrPair) == 8 == xcorr.PAIR_DTYPE.itemsize and C.sizeof(xcorr.XcorrPeak) == 32
    assert xcorr.MAX_LAG == 512 and xcorr.POINTS == 2048
    decl = _declared_functions()
    assert len(decl) == 6, decl
    L = xcorr.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(xcorr.EXPORTS) == decl
    assert L.uc_xcorr_abi_version() == 1 == xcorr.ABI_VERSION


def test_xcorr_library_stands_alone(xcorr):
    """libuchirp_xcorr.so links none of the other five libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", xcorr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", xcorr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_correlator(xcorr):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = xcorr.lib().uc_xcorr_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in xcorr.lib().uc_xcorr_last_error()
    with pytest.raises(xcorr.XcorrError):
        xcorr.Xcorr()


def build_host(tmp_path):
    import uchirp
    from uchirp import array, scene, xcorr
    for m in (uchirp, scene, array, xcorr):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_xcorr")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_xcorr.c"), "-o", exe, "-L" + libdir, "-luchirp_xcorr", "-luchirp_array",
                           "-luchirp_scene", "-luchirp", "-Wl,-rpath," + libdir])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(xcorr, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "uc_xcorr_abi_version 1 (header 1)" in out.stdout and "uc_xcorr_create: -19" in out.stdout and "no CPU path" in out.stdout


def _brute(xf, ref, mic, first, n, L):
    n_in = xf.shape[1]
    out = np.zeros(2 * L + 1)
    for lag in range(-L, L + 1):
        s = 0.0
        for j in range(first, first + n):
            if 0 <= j + lag < n_in:
                s += xf[ref, j] * xf[mic, j + lag]
        out[lag + L] = s
    return out


def test_model_is_the_definition(xcorr):
    rng = np.random.default_rng(2)
    x = rng.integers(-2 ** 27, 2 ** 27, size=(3, 2100)).astype(np.int32)       # mostly no floats: the cast rounds
    xf = x.astype(np.float32).astype(np.float64)
    pairs = [(0, 1), (2, 2), (1, 0)]
    # L = 1: S = 2046; L = 512: S = 1024 (brute force over a few lags only there: the loop is slow)
    for first, n, L, lags in ((3, 2045, 1, None), (3, 2046, 1, None), (2, 2047, 1, None), (0, 2100, 1, None), (7, 300, 9, None),
                              (500, 1023, 512, (-512, -511, -1, 0, 3, 511, 512)), (0, 1025, 512, (-512, 0, 512)),
                              (1076, 1024, 512, (-512, -7, 512))):
        got = xcorr.model(x, pairs, first, n, L)
        assert got.shape == (3, 2 * L + 1)
        E = xcorr.model(x, pairs, first, n, L, magnitude=True)
        assert E.shape == (3,) and (E > 0).all()
        for i, (ref, mic) in enumerate(pairs):
            if lags is None:
                want = _brute(xf, ref, mic, first, n, L)
                assert np.abs(got[i] - want).max() <= 1e-12 * E[i], (first, n, L, i)
            else:
                for lag in lags:
                    s = sum(xf[ref, j] * xf[mic, j + lag] for j in range(first, first + n) if 0 <= j + lag < 2100)
                    assert abs(got[i, lag + L] - s) <= 1e-12 * E[i], (first, n, L, i, lag)
            # E_p by its definition: the segments' norms
            S = xcorr.POINTS - 2 * L
            e = 0.0
            for i0 in range(0, n, S):
                cnt = min(S, n - i0)
                a = xf[ref, first + i0:first + i0 + cnt]
                b = np.array([xf[mic, j] if 0 <= j < 2100 else 0.0 for j in range(first + i0 - L, first + i0 + cnt + L)])
                e += np.linalg.norm(a) * np.linalg.norm(b)
            assert abs(E[i] - e) <= 1e-12 * e
    with pytest.raises(ValueError):
        xcorr.model(x, [(0, 1)], 0, 2101, 4)
    with pytest.raises(ValueError):
        xcorr.model(x, [(0, 1)], 0, 10, 513)
    with pytest.raises(ValueError):
        xcorr.model(x, [(0, 1)], 0, 10, 0)
    d, p = xcorr.delays_model(np.stack([xf[0], np.roll(xf[0], 305), np.roll(xf[0], -402)]), [[0, 1, 2]], first=600, n=900, max_lag=512)
    assert [round(v) for v in d[0]] == [0, 305, -402] and p[0][0] is None and p[0][1]["lag"] == 305


def test_emulation_stays_within_its_recorded_ratio_of_the_model(xcorr):
    """The float32 emulation (pocketfft, complex64) of the definition against the float64 model, as a multiple of
    2^-24 E_p.  Recorded: 1.3 - 1.8 over shapes like these; the bar is twice the largest seen."""
    rng = np.random.default_rng(3)
    ns = 3 * 2048 + 37
    x = (rng.standard_normal((4, ns)) * 1000.0).astype(np.float32)
    words = rng.integers(-2 ** 27, 2 ** 27, size=(4, ns)).astype(np.int32)
    pairs = [(0, 1), (2, 2), (3, 0)]
    worst = 0.0
    for data in (x, words):
        for L, first, n in ((1, 0, None), (64, 3, 1921), (65, 0, 4000), (200, 5, 6000), (511, 1, 4105), (512, 0, None), (512, 7, 4097)):
            want = xcorr.model(data, pairs, first, n, L)
            E = xcorr.model(data, pairs, first, n, L, magnitude=True)
            emu = xcorr.emulate32(data, pairs, first, n, L)
            r = float((np.abs(emu - want) / (2.0 ** -24 * E[:, None])).max())
            print("%s L %3d first %d n %s: emulation ratio %.3f" % (data.dtype, L, first, n, r))
            worst = max(worst, r)
    print("emulation: worst |emulate32 - model| / (2^-24 E_p) %.3f" % worst)
    assert 0.0 < worst <= 3.6, worst


def _same_bits(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("delay_samples", "height", "runner_up")) and \
        a["lag"] == b["lag"] and a["flags"] == b["flags"]


def test_peak_returns_the_bits_of_the_align_library(xcorr, align):
    assert (xcorr.NO_PEAK, xcorr.AT_EDGE) == (align.NO_PEAK, align.AT_EDGE)
    assert [f[0] for f in xcorr.XcorrPeak._fields_] == [f[0] for f in align.AlignPeak._fields_]
    assert [getattr(xcorr.XcorrPeak, f[0]).offset for f in xcorr.XcorrPeak._fields_] == [getattr(align.AlignPeak, f[0]).offset for f in align.AlignPeak._fields_]
    rng = np.random.default_rng(5)
    for i in range(1000):
        L = int(rng.integers(1, 65))
        row = rng.standard_normal(2 * L + 1) * 10.0 ** rng.uniform(-3, 12)
        if i % 7 == 0:
            row = np.round(row / np.abs(row).max() * 3.0)                   # many ties and plateaus
        assert _same_bits(xcorr.peak(row), align.peak(row)), (i, L)
    for row in ([5.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.1], [-1.0, -0.5, -0.2, -0.1, -0.3, -0.6, -2.0], [0.0, 2.0, 0.0, -1.0, 0.0, 2.0, 0.0],
                [9.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0]):
        assert _same_bits(xcorr.peak(row), align.peak(row)), row
    lib = xcorr.lib()
    out = xcorr.XcorrPeak()
    ok = np.ones(1025)
    bad = ok.copy()
    bad[900] = np.nan

    def call(row, L, o=out):
        return lib.uc_xcorr_peak(row.ctypes.data_as(C.c_void_p) if row is not None else None, L, C.byref(o) if o is not None else None)

    assert call(ok, 512) == 0
    for name, args in (("nan", (bad, 512)), ("corr NULL", (None, 512)), ("out NULL", (ok, 512, None)), ("L = 0", (ok, 0)), ("L = 513", (ok, 513))):
        assert call(*args) == -errno.EINVAL, name
        assert lib.uc_xcorr_last_error(), name
    assert call(bad, 300) == 0                                              # the value that is not finite lies outside the row


def test_peak_is_exact_on_sampled_cosines_at_512_lags(xcorr):
    w = 2.0 * np.pi / 4.46
    L = 512
    k = np.arange(-L, L + 1, dtype=np.float64)
    for off in (0.0, 0.25, -0.49, 311.25, -402.5, 499.999, -510.3):
        for got in (xcorr.peak(1e9 * np.cos(w * (k - off))), xcorr.peak_model(1e9 * np.cos(w * (k - off)))):
            cycles = (got["delay_samples"] - off) / 4.46
            assert abs(cycles - round(cycles)) * 4.46 <= 1e-8 and abs(got["height"] / 1e9 - 1.0) <= 1e-9, (off, got)
        # under a Gaussian envelope the tallest crest is the true one
        row = 1e9 * np.cos(w * (k - off)) * np.exp(-0.5 * ((k - off) / 11.0) ** 2)
        got, want = xcorr.peak(row), xcorr.peak_model(row)
        assert got["lag"] == want["lag"] and got["flags"] == want["flags"] == 0
        assert abs(got["delay_samples"] - want["delay_samples"]) <= 1e-12 * max(1.0, abs(off))
        assert abs(got["delay_samples"] - off) <= 0.05 and 0.8 < got["runner_up"] < 1.0, (off, got)


def test_estimator_recovers_delays_anywhere_in_500_samples(xcorr):
    """24 delays drawn in +-500 samples at +14 dB, 104 blocks, L = 512, in float64 (model + peak_model): each within 0.01
    samples of the truth, the bar of the align library's test (the margin seen is 5x)."""
    from uchirp import link
    rng = np.random.default_rng(11)
    nb, L, amp = 104, 512, 2000.0
    n = nb * N
    sigma = amp / 10.0 ** (14.0 / 20.0)
    err = []
    for a in range(6):
        lead = float(rng.integers(25, 46)) * N + rng.uniform(0.0, N)
        delay = np.concatenate([[0.0], rng.uniform(-500.0, 500.0, size=4)])
        text = "".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(2, 7))))
        x = np.stack([link.signal(text, lead + delay[m], amp, 0.0, n, FS) + sigma * rng.standard_normal(n) for m in range(5)]).astype(np.float32)
        d, peaks = xcorr.delays_model(x, [[0, 1, 2, 3, 4]], max_lag=L)
        for m in range(1, 5):
            assert peaks[0][m]["flags"] == 0
            err.append(d[0][m] - delay[m])
    err = np.abs(err)
    print("+14 dB, 24 delays in +-500 samples: worst |error| %.4f median %.4f samples" % (err.max(), np.median(err)))
    assert len(err) == 24 and err.max() <= 0.01, err.max()


def test_kernels_are_gfx950_without_spills_or_scratch(xcorr, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    if not os.path.exists(xcorr.LIB_PATH):
        pytest.skip("libuchirp_xcorr.so not built")
    monkeypatch.setattr(kr, "LIB", xcorr.LIB_PATH)
    ks = kr._kernels(tmp_path)
    corr = {k: v for k, v in ks.items() if "xcorr_kernel" in k}
    summ = {k: v for k, v in ks.items() if "xcorr_sum_kernel" in k}
    assert len(ks) == 3 and len(corr) == 2 and len(summ) == 1, sorted(ks)        # f32, i32; the sum in double
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            assert e["private_segment_fixed_size"] == 0, (k, e)
    for k, v in corr.items():
        assert v[0]["vgpr_count"] <= 240, (k, v)      # 236; the budget of 2 waves per SIMD is 256
        # two tiles of 2048 complex values and the two small twiddle tables: 35 KiB, four workgroups (eight waves) per CU
        assert v[0]["group_segment_fixed_size"] == (2 * 2 * 2048 + 2 * 256 + 2 * 128) * 4, (k, v)
        assert 4 * v[0]["group_segment_fixed_size"] <= 160 * 1024
    for k, v in summ.items():
        assert v[0]["vgpr_count"] <= 64 and v[0]["group_segment_fixed_size"] == 0, (k, v)
