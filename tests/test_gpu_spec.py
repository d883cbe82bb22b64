"""The spectrum analyser's kernel (libuchirp_spec.so, uchirp/spec.py) on the GPU: against what the STM32 itself printed
(the K6 captures), against its float64 model within the error form of include/uchirp_spec.h, every bin, sample and
coefficient in its place, the edges of every argument, the same bits whatever the grid and the cut into calls, the three
kinds and the peak records, refused calls, and the C host.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

import spec_util as su
from parity_util import MAG_TOL

pytestmark = pytest.mark.gpu

N = 2048
DEV = "cuda:0"
TIE = (256, 768)                                       # two tones whose stored magnitudes tie bit for bit


@pytest.fixture(scope="module")
def spec():
    from uchirp import spec as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def an(spec):
    a = spec.Analyser(0)
    yield a
    a.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _first_argmax(row):
    k = int(np.argmax(row))                            # numpy's arg-max is the first one
    return row[k], k


def _bound(spec, x, scale=1.0, **kw):
    """the error form's bound per frame, [rows, frames, 1]"""
    return (spec.ERROR_C * 2.0 ** -24 * abs(float(np.float32(scale))) * spec.model(np.atleast_2d(x), norm=True, **kw))[:, :, None]


# ------------------------------------------------------------------------------------------------------------------ 1: K6

def test_k6_words_through_the_kernel_are_what_the_firmware_printed(spec, an):
    """24 int32 rows, one frame each, one call, the firmware's own Hann table through set_window; test_gpu_k6.py's criterion
    on all bins 0 .. 1023 at or above 1 kHz; then once per sampling-rate group with ac_bins set: the whole `.fft` column."""
    import uchirp
    hann = uchirp.Engine(uchirp.RX_REAL).table(uchirp.TABLE_HANN)
    assert hann.shape == (N,) and hann.dtype == np.float32
    an.set_window(hann)
    caps = su.k6()
    words = _dev(su.k6_words())
    got, rec = an.spectra(words, scale=su.SCALE_K6, n_bins=1024, peaks=True)
    got, pk = got.cpu().numpy(), spec.peaks_of(rec)
    assert got.shape == (24, 1, 1024)
    passed, worst = 0, 0.0
    for i, (name, raw, freq, mag_dev) in enumerate(caps):
        ok, rel = su.k6_verdict(got[i, 0], mag_dev, freq, MAG_TOL)
        if name == su.K6_MISMATCHED:
            assert not ok, "the mismatched trio is expected to disagree"
            continue
        assert ok, (name, rel)
        assert (pk[i, 0]["value"], pk[i, 0]["bin"]) == _first_argmax(got[i, 0])
        worst = max(worst, rel)
        passed += 1
    print("23 captures: worst err / largest magnitude %.3g against MAG_TOL %.3g" % (worst, MAG_TOL))
    assert passed == 23
    # with the AC coupling: every printed value, the 1.0s included; the peak is the firmware's arg-max (main.c:140)
    groups = {}
    for i, c in enumerate(caps):
        groups.setdefault(su.ac_bins_of(c[2]), []).append(i)
    assert sorted(groups) == [21, 43, 50]
    for ac, rows in groups.items():
        g, rec = an.spectra(words[rows], scale=su.SCALE_K6, n_bins=1024, ac_bins=ac, peaks=True)
        g, pk = g.cpu().numpy().astype(np.float64), spec.peaks_of(rec)
        for r, i in enumerate(rows):
            name, raw, freq, mag_dev = caps[i]
            if name == su.K6_MISMATCHED:
                continue
            assert np.all(g[r, 0, :ac] == 1.0) and np.all(mag_dev[:ac] == 1.0)
            tol = MAG_TOL * got[i, 0].max() + su.PRINT_STEP
            assert np.abs(g[r, 0] - mag_dev).max() <= tol, (name, np.abs(g[r, 0] - mag_dev).max(), tol)
            assert int(pk[r, 0]["bin"]) == int(np.argmax(mag_dev)), name


# -------------------------------------------------------------------------------------------------- 2, 3: everything in place

def test_every_bin_is_in_its_place(spec, an):
    """1025 frames in one call, window of ones, frame k = cos(2 pi k i / 2048): the peak record's bin is k for k = 1 .. 1023,
    bin 1024 for (-1)^i (frame 1024 is that) and bin 0 for a constant (frame 0)."""
    an.set_window(np.ones(N, np.float32))
    i = np.arange(N)
    x = np.cos(2.0 * np.pi * np.outer(np.arange(1025), i) / N).astype(np.float32)
    assert np.all(x[0] == 1.0) and np.array_equal(x[1024], np.where(i % 2, -1.0, 1.0).astype(np.float32))
    g, rec = an.spectra(_dev(x.reshape(1, -1)), peaks=True)
    g, pk = g.cpu().numpy()[0], spec.peaks_of(rec)[0]
    assert g.shape == (1025, 1025)
    assert np.array_equal(pk["bin"], np.arange(1025))
    want = np.where((np.arange(1025) == 0) | (np.arange(1025) == 1024), 2048.0, 1024.0)
    assert np.abs(pk["value"] - want).max() <= 2048.0 * 1e-5
    # and nothing anywhere else: a tone's other bins are round-off of its norm
    off = g.copy()
    off[np.arange(1025), np.arange(1025)] = 0.0
    bound = _bound(spec, x.reshape(1, -1), window=np.ones(N, np.float32))[0]
    print("largest value off the tone's bin %.3g, bound %.3g" % (off.max(), bound.min()))
    assert np.all(off <= bound)


def test_every_sample_and_coefficient_is_in_its_place(spec, an):
    """2048 frames, frame p a single 1 at sample p, window w[p] = 1 + p / 4096: all 1025 values of frame p are w[p]."""
    w = (1.0 + np.arange(N) / 4096.0).astype(np.float32)
    an.set_window(w)
    x = np.zeros((N, N), np.float32)
    x[np.arange(N), np.arange(N)] = 1.0
    g = an.spectra(_dev(x.reshape(1, -1))).cpu().numpy()[0].astype(np.float64)
    assert g.shape == (N, 1025)
    err = np.abs(g - w[:, None].astype(np.float64)).max(axis=1)
    bound = spec.ERROR_C * 2.0 ** -24 * w.astype(np.float64)      # ||u|| = w[p]
    print("worst |v - w[p]| / (2^-24 w[p]) %.3f" % (err / (2.0 ** -24 * w)).max())
    assert np.all(err <= bound)
    # the next frame's window value is 2^-12 away: a sample or a coefficient one place off would show
    assert np.all(np.abs(g[:-1] - w[1:, None]).min(axis=1) > 2 * bound[:-1])


# ------------------------------------------------------------------------------------------------------- 4: the error form

def test_error_form_holds_on_noise_chirps_and_the_k6_words(spec, an):
    worst = 0.0
    for name, (x, kw) in su.error_rows().items():
        kw = dict(kw)
        fl = kw.pop("frame_len", N)
        an.set_window(None, fl)
        g = an.spectra(_dev(x), **kw).cpu().numpy()
        r = spec.error_ratio(g, x, frame_len=fl, **kw)
        print("%-32s %3d frames: worst |gpu - model| / (2^-24 scale ||u||) %7.3f" % (name, r.size, r.max()))
        worst = max(worst, float(r.max()))
    print("worst ratio %.3f, UC_SPEC_ERROR_C %d" % (worst, spec.ERROR_C))
    assert worst <= spec.ERROR_C


def test_a_frame_of_zeros_is_zeros(spec, an):
    import torch
    an.set_window(None, N)
    x = np.zeros((2, 3 * N), np.float32)
    x[1, :N] = 1000.0 * np.random.default_rng(7).standard_normal(N)          # a loud frame next to silent ones
    for xd in (_dev(x), _dev(x.astype(np.int32))):
        for kw in (dict(), dict(bin_first=200, n_bins=320)):
            g, rec = an.spectra(xd, peaks=True, **kw)
            b, pk = _bits(g), spec.peaks_of(rec)
            assert b[1, 0].any()
            for m, f in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)):
                assert not b[m, f].any(), (m, f)                                  # +0.0f: all bits clear
                assert pk[m, f]["value"] == 0.0 and not np.signbit(pk[m, f]["value"]) and pk[m, f]["bin"] == kw.get("bin_first", 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 5: edges

EDGES = [dict(frame_len=1, hop=1, n_in=5), dict(frame_len=1, hop=3000, n_in=6001), dict(frame_len=2047, hop=512, n_in=2047, first=-1),
         dict(frame_len=2048, hop=2048, n_in=4096, first=-2047), dict(frame_len=2048, hop=1, n_in=1, first=-2047, n_frames=2048),
         dict(frame_len=2048, hop=3000, n_in=7001, first=-1), dict(frame_len=2048, hop=512, n_in=2047, first=-333),
         dict(frame_len=2047, hop=2048, n_in=5000, first=777), dict(frame_len=2048, hop=1, n_in=2060, first=-5, n_frames=40),
         dict(frame_len=300, hop=177, n_in=1, first=-299), dict(frame_len=2048, hop=512, n_in=6000, first=4095)]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "len%d-hop%d-n%d-first%d" % (c["frame_len"], c["hop"], c["n_in"], c.get("first", 0)))
def test_edges_of_frames_and_rows(spec, an, case):
    """frame_len 1, 2047, 2048; first -2047, -1, odd values; last frames that overhang the row; hop 1, 512, 2048, 3000; rows of 1
    and 2047 samples: against the model within the error form, both dtypes, with a window that has no symmetry."""
    case = dict(case)
    n_in, fl = case.pop("n_in"), case["frame_len"]
    rng = np.random.default_rng(n_in + fl)
    w = rng.uniform(0.5, 1.5, fl).astype(np.float32)
    an.set_window(w)
    x = np.rint(1000.0 * rng.standard_normal((3, n_in))).astype(np.float32)
    x[:, 0] += 500.0                                   # a row of one sample is not silent
    kw = dict(hop=case["hop"], first=case.get("first", 0), n_frames=case.get("n_frames", 0))
    want = spec.model(x, window=w, frame_len=fl, **kw)
    bound = _bound(spec, x, window=w, frame_len=fl, **kw)
    assert want.shape[1] == (case.get("n_frames") or spec.frames(n_in, kw["first"], fl, kw["hop"]))
    for xd in (_dev(x), _dev(x.astype(np.int32))):
        g = an.spectra(xd, **kw).cpu().numpy().astype(np.float64)
        assert g.shape == want.shape
        assert np.all(np.abs(g - want) <= bound), np.abs(g - want).max()
    print("%d frames of %d rows, worst error %.3g of the bound" % (want.shape[1], 3, (np.abs(g - want) / np.maximum(bound, 1e-300)).max()))


def test_bin_ranges_strides_guards_and_no_peaks(spec, an):
    import torch
    an.set_window(None, N)
    rng = np.random.default_rng(8)
    x = (1000.0 * rng.standard_normal((2, 3 * N))).astype(np.float32)
    xd = _dev(x)
    full, rec = an.spectra(xd, hop=1000, peaks=True)
    fb, pk = _bits(full), spec.peaks_of(rec)
    nf = full.shape[1]
    assert full.shape == (2, 7, 1025)
    for b0, nb in ((0, 1025), (1024, 1), (200, 320), (127, 2), (0, 1), (63, 130)):
        # a guard in front, between and behind: rows 40 floats wider than the bins, in a buffer with 64 spare floats at each end
        stride = nb + 40
        buf = torch.full((64 + 2 * nf * stride + 64,), -7.0, dtype=torch.float32, device=DEV)
        out = buf[64:64 + 2 * nf * stride].view(2, nf, stride)[:, :, :nb]
        got, rec = an.spectra(xd, hop=1000, bin_first=b0, n_bins=nb, out=out, peaks=True)
        assert got.data_ptr() == out.data_ptr()
        h = buf.cpu().numpy()
        body = h[64:-64].reshape(2, nf, stride)
        assert np.array_equal(body[:, :, :nb].view(np.uint32), fb[:, :, b0:b0 + nb]), (b0, nb)        # the same bits as the full range
        assert np.all(body[:, :, nb:] == -7.0) and np.all(h[:64] == -7.0) and np.all(h[-64:] == -7.0), (b0, nb)
        sub = spec.peaks_of(rec)
        for m in range(2):
            for f in range(nf):
                v, k = _first_argmax(body[m, f, :nb])
                assert (sub[m, f]["value"], sub[m, f]["bin"]) == (v, b0 + k), (b0, nb, m, f)
    # peaks_dev NULL: the same spectra
    assert np.array_equal(_bits(an.spectra(xd, hop=1000)), fb)
    assert all((pk[m, f]["value"], pk[m, f]["bin"]) == _first_argmax(full[m, f].cpu().numpy()) for m in range(2) for f in range(nf))


# ------------------------------------------------------------------------------------------------------------ 6: same bits

def test_same_bits_whatever_the_grid_the_cut_and_the_rows(spec, an, uc_tuning, monkeypatch):
    an.set_window(None, N)
    rng = np.random.default_rng(9)
    hop, nf = 300, 37
    x = (1000.0 * rng.standard_normal((3, 36 * hop + 700))).astype(np.float32)
    assert spec.frames(x.shape[1], -100, N, hop) >= nf
    xd = _dev(x)
    kw = dict(hop=hop, bin_first=5, n_bins=1000)
    ref, rec = an.spectra(xd, first=-100, n_frames=nf, peaks=True, **kw)
    rb, rp = _bits(ref), rec.cpu().numpy()
    # calls in a row on one object
    for _ in range(3):
        g, r = an.spectra(xd, first=-100, n_frames=nf, peaks=True, **kw)
        assert np.array_equal(_bits(g), rb) and np.array_equal(r.cpu().numpy(), rp)
    # grids of 1 .. 5 workgroups
    for grid in (1, 2, 3, 4, 5):
        monkeypatch.setenv("UC_SPEC_GRID", str(grid))
        a = spec.Analyser(0)
        g, r = a.spectra(xd, first=-100, n_frames=nf, peaks=True, **kw)
        assert np.array_equal(_bits(g), rb) and np.array_equal(r.cpu().numpy(), rp), grid
        a.close()
    monkeypatch.delenv("UC_SPEC_GRID")
    # the range of 37 frames cut at 1, 2 and 36 into two calls: first moved by whole hops
    for cut in (1, 2, 36):
        g0, r0 = an.spectra(xd, first=-100, n_frames=cut, peaks=True, **kw)
        g1, r1 = an.spectra(xd, first=-100 + cut * hop, n_frames=nf - cut, peaks=True, **kw)
        assert np.array_equal(np.concatenate([_bits(g0), _bits(g1)], axis=1), rb), cut
        assert np.array_equal(np.concatenate([r0.cpu().numpy(), r1.cpu().numpy()], axis=1), rp), cut
    # each row alone, and as a sub-matrix of strided rows
    for m in range(3):
        g, r = an.spectra(xd[m:m + 1], first=-100, n_frames=nf, peaks=True, **kw)
        assert np.array_equal(_bits(g)[0], rb[m]) and np.array_equal(r.cpu().numpy()[0], rp[m]), m
    wide = _dev(np.concatenate([rng.standard_normal((3, 11)).astype(np.float32), x, rng.standard_normal((3, 6)).astype(np.float32)], axis=1))
    sub = wide[:, 11:11 + x.shape[1]]
    assert sub.stride(0) == x.shape[1] + 17
    g, r = an.spectra(sub, first=-100, n_frames=nf, peaks=True, **kw)
    assert np.array_equal(_bits(g), rb) and np.array_equal(r.cpu().numpy(), rp)
    g, r = an.spectra(sub[1:], first=-100, n_frames=nf, peaks=True, **kw)
    assert np.array_equal(_bits(g), rb[1:]) and np.array_equal(r.cpu().numpy(), rp[1:])


# ---------------------------------------------------------------------------------------------------------------- 7: kinds

def _db_inputs():
    """the values lambda is measured on: 16 rows of noise whose levels span nine decades"""
    rng = np.random.default_rng(3)
    return (rng.standard_normal((16, N)) * 10.0 ** rng.uniform(-3, 6, (16, 1))).astype(np.float32)


def test_power_and_db_are_functions_of_the_kernels_own_magnitude(spec, an):
    an.set_window(np.ones(N, np.float32))
    xd = _dev(_db_inputs())
    v32 = an.spectra(xd).cpu().numpy()
    v = v32.astype(np.float64)
    assert 1e-8 < v.min() and v.max() < 1e8
    pw = an.spectra(xd, kind="power").cpu().numpy()
    assert np.array_equal(pw.view(np.uint32), (v32 * v32).view(np.uint32))                 # fl(v v), bit for bit
    for floor, some_below in ((np.float32(1e-3), False), (np.float32(1.0), True)):
        assert bool((v32 < floor).any()) == some_below and (v32 > floor).any()
        for mul in (10.0, 20.0, -10.0):
            d = an.spectra(xd, kind="db", db_mul=mul, floor=float(floor)).cpu().numpy()
            want = mul * np.log10(np.maximum(v, float(floor)))
            err = np.abs(d.astype(np.float64) - want).max() / abs(mul)
            print("floor %g, db_mul %5.1f: worst |gpu - db_mul log10(max(v, floor))| / |db_mul| %.3e over log10 in [%.2f, %.2f], lambda %.1e"
                  % (floor, mul, err, (want / mul).min(), (want / mul).max(), spec.LOG10_ERROR))
            assert err <= spec.LOG10_ERROR
            if some_below:                          # below the floor: db_mul * log10f(floor), one value
                below = d[v32 < floor]
                assert np.all(below == below[0]) and abs(float(below[0]) - mul * np.log10(float(floor))) <= abs(mul) * spec.LOG10_ERROR


def test_peak_record_is_the_first_argmax_of_the_stored_row(spec, an):
    """The record equals the first arg-max of the stored row exactly, in all three kinds and with bin sub-ranges, on frames
    built to tie among them: two equal tones on bins 256 and 768 (the stored values are asserted to tie, bit for bit, before
    the bin is), a quiet frame under the AC coupling (400 values of 1.0), and levels under the floor (every value the same)."""
    an.set_window(np.ones(N, np.float32))
    i = np.arange(N)
    rng = np.random.default_rng(10)
    x = np.zeros((3, N), np.float32)
    x[0] = (np.cos(2 * np.pi * TIE[0] * i / N) + np.cos(2 * np.pi * TIE[1] * i / N)).astype(np.float32)
    x[1] = rng.standard_normal(N).astype(np.float32)
    x[2] = 0.001 * rng.standard_normal(N).astype(np.float32)
    xd = _dev(x.reshape(1, -1))
    ties = 0
    for kw in (dict(), dict(kind="power"), dict(kind="db", floor=1e-6), dict(kind="db", db_mul=-20.0, floor=1e-6), dict(bin_first=TIE[0] + 1, n_bins=600),
               dict(bin_first=1, n_bins=1024, kind="power"), dict(ac_bins=400), dict(ac_bins=400, kind="db"), dict(kind="db", floor=1e6),
               dict(kind="db", floor=1e6, bin_first=127, n_bins=2)):
        g, rec = an.spectra(xd, peaks=True, **kw)
        g, pk = g.cpu().numpy()[0], spec.peaks_of(rec)[0]
        b0 = kw.get("bin_first", 0)
        for f in range(3):
            v, k = _first_argmax(g[f])
            tied = int((g[f] == v).sum())
            ties += tied > 1
            print("%-50r frame %d: peak %.6g at bin %d, %d stored values tie" % (kw, f, pk[f]["value"], pk[f]["bin"], tied))
            assert (pk[f]["value"], pk[f]["bin"]) == (v, b0 + k), (kw, f)
    assert ties >= 10, ties
    # two equal tones: the stored values tie, then the lowest bin wins
    for kw in (dict(), dict(kind="power"), dict(kind="db", floor=1e-6)):
        g, rec = an.spectra(xd, peaks=True, **kw)
        g, pk = g.cpu().numpy()[0], spec.peaks_of(rec)[0]
        assert g[0, TIE[0]] == g[0, TIE[1]] == g[0].max(), (kw, g[0, TIE[0]], g[0, TIE[1]])
        assert pk[0]["bin"] == TIE[0] and pk[0]["value"] == g[0, TIE[0]]
    g, rec = an.spectra(xd, peaks=True, bin_first=TIE[0] + 1, n_bins=600)
    assert spec.peaks_of(rec)[0][0]["bin"] == TIE[1]
    # the AC coupling ties 400 bins at 1.0 above everything of the quiet frame; the floor ties every bin
    g, rec = an.spectra(xd, peaks=True, ac_bins=400)
    assert (spec.peaks_of(rec)[0][2]["value"], spec.peaks_of(rec)[0][2]["bin"]) == (1.0, 0) and g.cpu().numpy()[0, 2, 400:].max() < 1.0
    g, rec = an.spectra(xd, peaks=True, kind="db", floor=1e6, bin_first=127, n_bins=2)
    assert np.all(spec.peaks_of(rec)[0]["bin"] == 127) and np.all(g.cpu().numpy() == g.cpu().numpy()[0, 0, 0])


# -------------------------------------------------------------------------------------------------------- 8: refused calls

def test_a_refused_call_enqueues_nothing_and_the_next_one_works(spec, an):
    import torch
    an.set_window(None, N)
    L = spec.lib()
    x = _dev((1000.0 * np.random.default_rng(11).standard_normal((2, 3 * N))).astype(np.float32))
    good = an.spectra(x)
    want = _bits(good)
    out = torch.full_like(good, -7.0)
    pk = torch.zeros((2, 3, 8), dtype=torch.uint8, device=DEV)
    host = np.zeros(64, np.float32)
    other = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)

    def run(p=None, in_dev=x.data_ptr(), dtype=spec.DTYPE_F32, n_rows=2, n_in=3 * N, in_stride=0, out_dev=out.data_ptr(), out_stride=0,
            peaks=pk.data_ptr(), handle=an._h):
        p = p or spec.params()
        return L.uc_spec_run(handle, C.c_void_p(in_dev), dtype, n_rows, n_in, in_stride, C.byref(p), C.c_void_p(out_dev), out_stride,
                             C.c_void_p(peaks), None)

    refused = [("spec NULL", dict(handle=None)), ("in NULL", dict(in_dev=0)), ("out NULL", dict(out_dev=0)), ("dtype 2", dict(dtype=2)),
               ("no rows", dict(n_rows=0)), ("in_stride < n_in", dict(in_stride=3 * N - 1)), ("out_stride < n_bins", dict(out_stride=1024)),
               ("frame_len is not the window's", dict(p=spec.params(frame_len=2047))), ("hop 0", dict(p=spec.params(hop=0))),
               ("first = n_in", dict(p=spec.params(first=3 * N))), ("n_frames above the count", dict(p=spec.params(n_frames=4))),
               ("kind 3", dict(p=spec.SpecParams(0, 0, N, N, 0, 1025, 0, 3, 1.0, 1e-20, 10.0, 0))), ("floor 0", dict(p=spec.params(floor=0.0))),
               ("scale nan", dict(p=spec.params(scale=float("nan")))), ("bins beyond 1024", dict(p=spec.params(bin_first=1, n_bins=1025))),
               ("host memory in", dict(in_dev=host.ctypes.data, n_rows=1, n_in=64, p=spec.params(n_frames=1))),
               ("host memory out", dict(out_dev=host.ctypes.data)), ("host memory peaks", dict(peaks=host.ctypes.data)),
               ("out overlaps in", dict(out_dev=x.data_ptr() + 4 * N)), ("peaks overlap in", dict(peaks=x.data_ptr() + 8)),
               ("peaks overlap out", dict(peaks=out.data_ptr() + 16))]
    for name, kw in refused:
        rc = run(**kw)
        assert rc == -errno.EINVAL and L.uc_spec_last_error(), (name, rc)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0) and not pk.cpu().numpy().any()                   # nothing was enqueued
    assert run() == 0                                                                        # and the object is usable
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), want) and pk.cpu().numpy().any()
    for bad in (dict(window=np.ones(0, np.float32)), dict(window=np.ones(2049, np.float32)), dict(window=np.array([1.0, np.nan], np.float32))):
        with pytest.raises(spec.SpecError):
            an.set_window(**bad)
    assert np.array_equal(_bits(an.spectra(x)), want)                                        # a refused window leaves the old one
    assert other.sum().item() == 0.0


# ------------------------------------------------------------------------------------------------------------------- 9: C

def test_c_host_prints_the_expected_peak(spec, tmp_path):
    from test_spec_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    assert "uc_spec_abi_version 1 (header 1)" in out.stdout
    assert "tone at 17000 Hz of 78125 Hz: peak at bin 446 (17013.5 Hz)" in out.stdout and "3 of 3 frames" in out.stdout
