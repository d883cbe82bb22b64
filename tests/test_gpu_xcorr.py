"""The wide-lag correlator on the GPU (uc_xcorr_correlate, uchirp/xcorr.py): correlations against the float64 model,
bit-identity under every way of dealing the work, agreement with the direct correlator of libuchirp_align.so where both
apply, estimated delays out to +-480 samples against the model's and the scene's, end to end through the scene renderer,
the array combiner and the receivers of libuchirp.so, the contract of the call, and a plain C host.

Tolerance of the model test: the error form of the header, |gpu - model| / (2^-24 E_p), is held against the same figure
of `xcorr.emulate32` -- an independent float32 evaluation of the same definition (pocketfft, complex64) -- on the same
inputs: the GPU's worst ratio may be at most FOUR times the emulation's worst.  The factor covers the radix-16
butterflies' different order and twiddles built as products up to three factors deep.  It is not tuned to what the kernel
gives.  Every test prints its figures before it asserts (pytest -s).

Recorded on one MI355X (profiles/r11_xcorr.txt): model test, worst GPU ratio 4.41 against 4 x 2.60 = 10.39 (emulation);
|xcorr - align| at most 0.066 of the sum of the two bounds; delays at +14 dB, L = 512: worst |gpu - model| 2.5e-08 samples,
worst |gpu - scene| 0.0017 samples; 8 arrays of 8 over +-400 samples: no text differs, worst delay error 0.0020 samples;
full groups at L <= 200 (longer rows): worst GPU ratio 3.45 against 4 x 2.95."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
NM = 4
NS = 3 * 2048 + 37


@pytest.fixture(scope="module")
def xcorr():
    from uchirp import xcorr as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def align():
    from uchirp import align as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def array():
    from uchirp import array as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def scene():
    from uchirp import scene as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def mics(xcorr, scene):
    """4 microphones x (3 x 2048 + 37) samples: a message of amplitude 2000 at a lead of its own per microphone, plus noise
    (device tensor and host copy), and int32 words most of which are no floats; made once and never written."""
    import torch
    rng = np.random.default_rng(26)
    lead = rng.uniform(0.0, 600.0, size=NM)
    x = scene.Scene().render(["Hi"], [(300.0, [(0, 2000.0, float(lead[m]), 0.0)]) for m in range(NM)], n_samples=NS, seed=8)
    h = x.cpu().numpy()
    assert np.abs(h).max() > 2000.0
    words = rng.integers(-2 ** 27, 2 ** 27, size=(NM, NS)).astype(np.int32)
    words[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    return {"f32": (x, h), "i32": (torch.from_numpy(words).to("cuda:0"), words)}


PAIRS = [(0, 1), (2, 2), (3, 0), (1, 0), (3, 3), (2, 1)]


class Reference:
    """model, E_p and emulate32 of one case, computed once"""
    cache = {}

    @classmethod
    def of(cls, xcorr, name, host, first, n, L):
        key = (name, first, n, L)
        if key not in cls.cache:
            cls.cache[key] = (xcorr.model(host, PAIRS, first, n, L), xcorr.model(host, PAIRS, first, n, L, magnitude=True),
                              xcorr.emulate32(host, PAIRS, first, n, L))
        return cls.cache[key]


def _ratios(xcorr, name, got, host, first, n, L):
    want, E, emu = Reference.of(xcorr, name, host, first, n, L)
    zero = E == 0                                    # a reference of zeros: the error form leaves no room at all
    assert (got[zero] == 0).all() and (emu[zero] == 0).all()
    if zero.all():
        return 0.0, 0.0
    unit = 2.0 ** -24 * E[~zero, None]
    return float((np.abs(got - want)[~zero] / unit).max()), float((np.abs(emu - want)[~zero] / unit).max())


def _cases():
    cases = []
    for L in (1, 64, 65, 200, 511, 512):
        S, G = 2048 - 2 * L, 4
        cases += [(L, 0, None), (L, 37, NS - 37), (L, 701, 1)]            # first = 0, first + n = n_in, first odd, n = 1
        cases += [(L, f, n) for f, n in ((5, S - 1), (4, S), (3, S + 1), (0, G * S), (1, G * S + 1)) if f + n <= NS]
    cases += [(65, NS - 1, 1), (512, 0, 1), (512, 2077, 4 * 1024), (1, 0, 3 * 2046 + 1)]
    return cases


def test_correlation_against_the_model_within_four_times_the_emulation(xcorr, mics):
    import torch
    xc = xcorr.Xcorr()
    cases = _cases()
    assert (512, 1, 4097) in cases and (511, 1, 4105) in cases and (512, 0, 4096) in cases      # G S and G S + 1 are among them
    worst_gpu = worst_emu = 0.0
    for name in ("f32", "i32"):
        dev, host = mics[name]
        for L, first, n in cases:
            got = xc.correlate(dev, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
            assert got.shape == (len(PAIRS), 2 * L + 1) and got.dtype == np.float64
            rg, re = _ratios(xcorr, name, got, host, first, n, L)
            print("%s L %3d first %4d n %5s: |gpu - model| / (2^-24 E) %.3f, emulation %.3f" % (name, L, first, n, rg, re))
            worst_gpu, worst_emu = max(worst_gpu, rg), max(worst_emu, re)
            assert np.abs(got).max() > 0 or (name, L, first, n) == ("i32", 512, 0, 1)      # (word 0 of every row of words is 0)
        # strided rows with an odd pitch: rows that are not 16-byte aligned
        xs = torch.zeros((NM, NS + 131), dtype=dev.dtype, device="cuda:0")[:, 3:3 + NS]
        xs.copy_(dev)
        for L, first, n in ((200, 5, 1647), (512, 0, None)):
            got = xc.correlate(xs, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
            rg, re = _ratios(xcorr, name, got, host, first, n, L)
            print("%s strided rows, L %d: |gpu - model| / (2^-24 E) %.3f, emulation %.3f" % (name, L, rg, re))
            worst_gpu, worst_emu = max(worst_gpu, rg), max(worst_emu, re)
    print("correlation: worst GPU ratio %.3f, worst emulation ratio %.3f, bar 4 x emulation = %.3f; UC_XCORR_ERROR_C = %d"
          % (worst_gpu, worst_emu, 4.0 * worst_emu, xcorr.ERROR_C))
    assert worst_gpu <= 4.0 * worst_emu, (worst_gpu, worst_emu)
    assert 4.0 * worst_emu <= xcorr.ERROR_C          # the header's constant is that bar, rounded up


def test_a_full_group_and_one_sample_more_at_small_lags(xcorr):
    """n = G S and G S + 1 for L in {1, 64, 65, 200}: the rows of `mics` (3 x 2048 + 37 samples) hold a full group only for
    L >= 253, where S is close to 1024.  Rows of 4 x 2046 + 37 samples hold one at every L; same pairs, same condition."""
    import torch
    ns = 4 * 2046 + 37
    rng = np.random.default_rng(31)
    data = {"f32": (rng.standard_normal((NM, ns)) * 1500.0).astype(np.float32),
            "i32": rng.integers(-2 ** 27, 2 ** 27, size=(NM, ns)).astype(np.int32)}
    xc = xcorr.Xcorr()
    worst_gpu = worst_emu = 0.0
    for name, host in data.items():
        dev = torch.from_numpy(host).to("cuda:0")
        for L in (1, 64, 65, 200):
            S = 2048 - 2 * L
            for first, n in ((0, 4 * S), (1, 4 * S + 1)):
                got = xc.correlate(dev, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
                rg, re = _ratios(xcorr, name + " long", got, host, first, n, L)
                print("%s L %3d first %d n %4d: |gpu - model| / (2^-24 E) %.3f, emulation %.3f" % (name, L, first, n, rg, re))
                worst_gpu, worst_emu = max(worst_gpu, rg), max(worst_emu, re)
    print("full groups at small L: worst GPU ratio %.3f, worst emulation ratio %.3f, bar %.3f" % (worst_gpu, worst_emu, 4.0 * worst_emu))
    assert worst_gpu <= 4.0 * worst_emu, (worst_gpu, worst_emu)
    assert worst_gpu <= xcorr.ERROR_C


def test_grids_calls_and_pair_order_give_the_same_bits(xcorr, mics, uc_tuning, monkeypatch):
    import torch
    x, h = mics["f32"]
    xc = xcorr.Xcorr()
    for L, first, n in ((512, 0, None), (511, 1, 4105), (64, 3, 1921), (1, 0, None)):
        whole = xc.correlate(x, PAIRS, first=first, n=n, max_lag=L)
        assert float(whole.abs().max()) > 0
        assert torch.equal(xc.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), L       # the other staging slot
        assert torch.equal(xc.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), L
        order = [4, 0, 2, 5, 1, 3]
        other = xc.correlate(x, [PAIRS[i] for i in order], first=first, n=n, max_lag=L)
        assert torch.equal(other, whole[order]), L
        assert torch.equal(xc.correlate(x, PAIRS[2:3], first=first, n=n, max_lag=L), whole[2:3]), L   # alone as among others
        for grid in range(1, 6):
            monkeypatch.setenv("UC_XCORR_GRID", str(grid))
            x2 = xcorr.Xcorr()
            assert torch.equal(x2.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), (L, grid)
            x2.close()
        monkeypatch.delenv("UC_XCORR_GRID")
        # a strided output: the guard values around every row stay
        lags = 2 * L + 1
        ys = torch.full((len(PAIRS), lags + 9), 7.0, dtype=torch.float64, device="cuda:0")
        xc.correlate(x, PAIRS, first=first, n=n, max_lag=L, out=ys[:, 4:4 + lags])
        assert torch.equal(ys[:, 4:4 + lags], whole), L
        assert float(ys[:, :4].min()) == 7.0 == float(ys[:, :4].max()) and float(ys[:, 4 + lags:].min()) == 7.0 == float(ys[:, 4 + lags:].max())


def test_agrees_with_the_direct_correlator_within_both_bounds(xcorr, align, mics):
    """For L <= 64 both libraries compute the same sums by different algorithms: they differ by at most the sum of their
    stated bounds on the same inputs."""
    xc, al = xcorr.Xcorr(), align.Aligner()
    worst = 0.0
    for name in ("f32", "i32"):
        dev, host = mics[name]
        for L, first, n in ((1, 0, None), (33, 5, 4000), (64, 37, NS - 37), (64, 0, 1920)):
            a = xc.correlate(dev, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
            b = al.correlate(dev, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
            E = xcorr.model(host, PAIRS, first, n, L, magnitude=True)
            mag = align.model(host, PAIRS, first, n, L, magnitude=True)
            bound = xcorr.ERROR_C * 2.0 ** -24 * E[:, None] + align.ROUNDINGS * 2.0 ** -24 * mag
            r = float((np.abs(a - b) / bound).max())
            print("%s L %2d first %2d n %5s: worst |xcorr - align| / (sum of the bounds) %.4f" % (name, L, first, n, r))
            worst = max(worst, r)
    assert 0.0 < worst <= 1.0, worst


# ---- delays: arrays rendered by the scene renderer, the microphones hundreds of samples apart

def _wide_arrays(array, seed, n_arrays, n_mics, spread, snr_db, amp=2000.0):
    rng = np.random.default_rng(seed)
    texts = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(2, 7)))) for _ in range(n_arrays)]
    lead = rng.integers(25, 46, size=n_arrays) * float(N) + rng.uniform(0.0, N, size=n_arrays)
    delay = rng.uniform(-spread, spread, size=(n_arrays, n_mics))
    delay[:, 0] = 0.0
    delay[:, 1] = spread * np.where(rng.integers(0, 2, size=n_arrays) == 1, 1.0, -1.0) * rng.uniform(0.9, 1.0, size=n_arrays)
    sigma = amp / 10.0 ** (snr_db / 20.0)
    mics = [(sigma, [(a, amp, float(lead[a] + delay[a, m]), 0.0)]) for a in range(n_arrays) for m in range(n_mics)]
    beams = [[(a * n_mics + m, w, d) for (m, w, d) in array.steer(lead[a] + delay[a])] for a in range(n_arrays)]
    rows = [[a * n_mics + m for m in range(n_mics)] for a in range(n_arrays)]
    return texts, mics, beams, rows, delay


def test_delays_match_the_model_and_the_scene_and_exceed_the_direct_range(xcorr, align, array, scene):
    na, nm, nb, L = 4, 4, 104, 512
    texts, mics, beams, rows, truth = _wide_arrays(array, 21, na, nm, 480.0, 14.0)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=45)
    got, peaks = xcorr.Xcorr().delays(x, rows, max_lag=L)
    want, _ = xcorr.delays_model(x.cpu().numpy(), rows, max_lag=L)
    got, want = np.array(got), np.array(want)
    assert got.shape == (na, nm) and (got[:, 0] == 0).all() and all(p[0] is None and all(q["flags"] == 0 for q in p[1:]) for p in peaks)
    print("+14 dB, %d arrays of %d, delays over +-480, L = 512: worst |gpu - model| %.3g samples, worst |gpu - scene| %.4f samples, "
          "largest runner-up %.3f" % (na, nm, np.abs(got - want).max(), np.abs(got - truth).max(), max(q["runner_up"] for p in peaks for q in p[1:])))
    assert np.abs(truth).max() > 430.0
    assert np.abs(got - truth).max() <= 0.01
    assert np.abs(got - want).max() <= 1e-3
    # what the feature adds: the direct correlator, at its widest, cannot see these delays
    near, near_peaks = align.Aligner().delays(x, rows, max_lag=align.MAX_LAG)
    far = [(a, m) for a in range(na) for m in range(1, nm) if abs(truth[a, m]) > align.MAX_LAG]
    assert len(far) >= na
    for a, m in far:
        assert near_peaks[a][m]["flags"] & align.AT_EDGE or abs(near[a][m] - truth[a, m]) > 1.0, (a, m, near[a][m], truth[a, m])
    print("uc_align_correlate at L = 64 on the same buffer: %d of %d microphones beyond 64 samples flagged AT_EDGE, the others "
          "more than one sample off" % (sum(1 for a, m in far if near_peaks[a][m]["flags"] & align.AT_EDGE), len(far)))


def test_end_to_end_wide_steering_decodes_what_true_steering_decodes(xcorr, array, scene, uchirp):
    na, nm, nb = 8, 8, 104
    texts, mics, beams, rows, truth = _wide_arrays(array, 16, na, nm, 400.0, 14.0)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=47)
    est_beams, delays, _ = xcorr.steer(x, rows)
    ar = array.Array()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    got_true, _ = eng.receive_many(ar.combine(x, beams), want_trace=False)
    got_est, _ = eng.receive_many(ar.combine(x, est_beams), want_trace=False)
    differ = [a for a in range(na) if got_true[a] != got_est[a]]
    for a in differ:
        print("  array %d: estimated steering decodes %r, true steering %r (sent %r)" % (a, got_est[a], got_true[a], texts[a]))
    print("+14 dB, %d arrays of %d, delays over +-400: %d texts differ between estimated and true steering; worst delay error %.4f samples"
          % (na, nm, len(differ), np.abs(np.array(delays) - truth).max()))
    assert sum(1 for t, g in zip(texts, got_true) if t in g) == na
    assert not differ, differ


@pytest.fixture
def other_device():
    """The calling thread's current device while the object lives on device 0: device 1 where the machine has one, so that
    an entry point that left the object's device current would be seen.  With a single GPU device 0 is always current and
    the assertions on the current device cannot fail: the restore is then not tested."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_refused_calls_leave_the_object_usable(xcorr, mics, other_device):
    import torch
    L = xcorr.lib()
    x, h = mics["f32"]
    ns = NS
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    xc = xcorr.Xcorr(0)
    assert torch.cuda.current_device() == dev0
    pairs = np.zeros(3, xcorr.PAIR_DTYPE)
    pairs["ref"], pairs["mic"] = [0, 2, 3], [1, 2, 0]
    lag, lags = 300, 601
    out = torch.full((3, lags), 7.0, dtype=torch.float64, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=xcorr.DTYPE_F32, n_mics=NM, n_in=ns, in_stride=0, pairs=pairs, n_pairs=3, first=10, n=ns - 20,
             max_lag=lag, out_ptr=out.data_ptr(), corr_stride=0):
        rc = L.uc_xcorr_correlate(xc._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_mics, n_in, in_stride,
                                  pairs.ctypes.data_as(C.c_void_p) if pairs is not None else None, n_pairs, first, n, max_lag,
                                  C.c_void_p(out_ptr), corr_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    def changed(field, i, v):
        b = pairs.copy()
        b[field][i] = v
        return b

    host = np.zeros(NM * ns, np.float32)
    refusals = [("ref >= n_mics", dict(pairs=changed("ref", 1, NM))), ("mic >= n_mics", dict(pairs=changed("mic", 2, NM))),
                ("mic >= n_mics (fewer microphones)", dict(n_mics=3)),
                ("first + n > n_in", dict(first=21)), ("first + n > n_in (n alone)", dict(first=0, n=ns + 1)),
                ("first beyond the row", dict(first=ns + 1, n=1)), ("first + n wraps", dict(first=2 ** 64 - 1, n=2)),
                ("max_lag 0", dict(max_lag=0)), ("max_lag 513", dict(max_lag=513)),
                ("corr_stride < 2L + 1", dict(corr_stride=lags - 1)), ("in_stride < n_in", dict(in_stride=ns - 1)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("no microphones", dict(n_mics=0)), ("no input samples", dict(n_in=0)), ("no pairs", dict(n_pairs=0)), ("n = 0", dict(n=0)),
                ("pairs NULL", dict(pairs=None)), ("in NULL", dict(in_ptr=None)), ("corr NULL", dict(out_ptr=None)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("corr: host memory", dict(out_ptr=host.ctypes.data)),
                ("corr overlaps in", dict(out_ptr=x.data_ptr() + 4 * ns)),
                ("corr overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (NM * ns - 1) - 4)),
                ("in overlaps the end of corr", dict(in_ptr=out.data_ptr() + 8 * (3 * lags - 1)))]
    if two:
        far_in = torch.zeros((NM, ns), dtype=torch.float32, device="cuda:1")
        far_out = torch.zeros((3, lags), dtype=torch.float64, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far_in.data_ptr())), ("corr: memory of another device", dict(out_ptr=far_out.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_xcorr_last_error(), name
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())          # nothing was enqueued
    assert call() == 0                                           # and the object is as usable as before
    torch.cuda.synchronize()
    p = list(zip(pairs["ref"].tolist(), pairs["mic"].tolist()))
    want = xcorr.model(h, p, 10, ns - 20, lag)
    E = xcorr.model(h, p, 10, ns - 20, lag, magnitude=True)
    assert (np.abs(out.cpu().numpy() - want) <= xcorr.ERROR_C * 2.0 ** -24 * E[:, None]).all()
    assert torch.equal(out, xcorr.Xcorr(0).correlate(x, p, first=10, n=ns - 20, max_lag=lag))
    # five calls in a row that reuse (and overwrite) the same host array: the library has copied it when a call returns
    outs = [torch.empty((3, lags), dtype=torch.float64, device="cuda:0") for _ in range(5)]
    sets = []
    for i in range(4):
        sets.append([(i, 3 - i), (i, i), (3 - i, 0)])
        pairs["ref"], pairs["mic"] = [q[0] for q in sets[i]], [q[1] for q in sets[i]]
        assert call(out_ptr=outs[i].data_ptr()) == 0
    pairs["ref"] = pairs["mic"] = 0
    torch.cuda.synchronize()
    for i in range(4):
        want = xcorr.model(h, sets[i], 10, ns - 20, lag)
        E = xcorr.model(h, sets[i], 10, ns - 20, lag, magnitude=True)
        assert (np.abs(outs[i].cpu().numpy() - want) <= xcorr.ERROR_C * 2.0 ** -24 * E[:, None]).all(), i
    h2 = C.c_void_p()
    assert L.uc_xcorr_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_xcorr_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    xc.close()
    assert torch.cuda.current_device() == dev0


def test_plain_c_host_estimates_combines_and_receives_hello_world(xcorr, tmp_path):
    from test_xcorr_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_xcorr_abi_version 1 (header 1)"
    est = [ln for ln in lines if ln.startswith("microphone ")]
    assert len(est) == 3, lines
    for ln, off in zip(est, (97.5, 311.25, 460.375)):
        assert abs(float(ln.split("estimated delay")[1].split()[0]) - off) <= 0.01, ln
    beam = [ln for ln in lines if ln.startswith("beam of 4 microphones steered by estimated delays received")]
    assert len(beam) == 1 and "Hello World!" in beam[0], lines
