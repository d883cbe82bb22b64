"""The delay estimator on the GPU (uc_align_correlate, uchirp/align.py): correlations against the float64 model within the
header's bound, bit-identity under every way of dealing the work, the contract of the call, estimated delays against the
model's and the scene's, end to end through the scene renderer, the array combiner and the receivers of libuchirp.so, and
a plain C host.

Bound of the model test: the header states the order of every sum; the longest path from a product to a segment's float
sum has K = UC_ALIGN_ROUNDINGS roundings, each at most half an ulp (2^-24 relative) of a partial sum that the sum of the
magnitudes bounds, and the double additions behind them add 2^-53 each: |gpu - model| <= K 2^-24 sum |x_ref x_mic| per
lag.  It is not tuned to what the kernel gives.  Every test prints its figures before it asserts (pytest -s).

Recorded on one MI355X (profiles/r10_align.txt): model test, worst |gpu - model| / bound 0.0362 (K = 70); delays at
+14 dB, worst |gpu - model| 9.4e-09 samples, worst |gpu - scene| 0.0018 samples; -12 dB, 64 arrays of 8: true steering
decodes 64 / 64, estimated steering 64 / 64, microphone 0 alone 0 / 64, with 241 of 448 pairs more than 0.5 samples off
(whole carrier cycles; worst 37.3 samples); +14 dB, 16 arrays: no text differs, worst delay error 0.0022 samples."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
NM = 6
# the shortfall of estimated against true steering allowed at -12 dB (arrays of 64): twice the first measurement's (0), at least 4
MARGIN = 4


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
def mics(align, scene):
    """6 microphones x (2 segments + 77) samples: a message of amplitude 2000 at a lead of its own per microphone, plus noise
    (device tensor and host copy), and int32 words most of which are no floats; made once and never written."""
    import torch
    ns = 2 * align.SEGMENT + 77
    rng = np.random.default_rng(26)
    lead = rng.uniform(0.0, 600.0, size=NM)
    x = scene.Scene().render(["Hi"], [(300.0, [(0, 2000.0, float(lead[m]), 0.0)]) for m in range(NM)], n_samples=ns, seed=8)
    h = x.cpu().numpy()
    assert np.abs(h).max() > 2000.0
    words = rng.integers(-2 ** 27, 2 ** 27, size=(NM, ns)).astype(np.int32)
    words[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    return {"f32": (x, h), "i32": (torch.from_numpy(words).to("cuda:0"), words), "ns": ns}


PAIRS = [(0, 1), (2, 2), (5, 0), (3, 4), (1, 0), (5, 5), (4, 2)]


def _ratio(align, got, host, pairs, first, n, L):
    want = align.model(host, pairs, first, n, L)
    mag = align.model(host, pairs, first, n, L, magnitude=True)
    bound = align.ROUNDINGS * 2.0 ** -24 * mag
    err = np.abs(got - want)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def test_correlation_within_the_bound_of_the_model(align, mics):
    import torch
    S, ns = align.SEGMENT, mics["ns"]
    al = align.Aligner()
    worst = 0.0
    cases = [(L, 0, None) for L in (1, 5, 33, 64)]                        # first = 0 and first + n = n_in: zeros on both sides
    cases += [(33, 700, 1), (33, 5, S - 1), (33, 4, S), (33, 3, S + 1), (5, ns - 1, 1), (64, 1001, 2 * S - 1000), (5, 3, 255), (5, 2, 257)]
    for name in ("f32", "i32"):
        dev, host = mics[name]
        for L, first, n in cases:
            got = al.correlate(dev, PAIRS, first=first, n=n, max_lag=L).cpu().numpy()
            assert got.shape == (len(PAIRS), 2 * L + 1) and got.dtype == np.float64
            r = _ratio(align, got, host, PAIRS, first, n, L)
            print("%s L %2d first %4d n %5s: worst |gpu - model| / bound %.4f" % (name, L, first, n, r))
            worst = max(worst, r)
            assert np.abs(got).max() > 0
        # strided rows with an odd pitch: rows that are not 16-byte aligned
        xs = torch.zeros((NM, ns + 131), dtype=dev.dtype, device="cuda:0")[:, 3:3 + ns]
        xs.copy_(dev)
        got = al.correlate(xs, PAIRS, first=1, n=ns - 2, max_lag=33).cpu().numpy()
        r = _ratio(align, got, host, PAIRS, 1, ns - 2, 33)
        print("%s strided rows: worst |gpu - model| / bound %.4f" % (name, r))
        worst = max(worst, r)
    print("correlation: worst |gpu - model| / bound %.4f (K = %d)" % (worst, align.ROUNDINGS))
    assert worst <= 1.0, worst


def test_grids_calls_and_pair_order_give_the_same_bits(align, mics, uc_tuning, monkeypatch):
    import torch
    x, h = mics["f32"]
    S = align.SEGMENT
    al = align.Aligner()
    for L, first, n in ((48, 0, None), (64, 3, S + 1), (5, 0, 2 * S)):
        whole = al.correlate(x, PAIRS, first=first, n=n, max_lag=L)
        assert float(whole.abs().max()) > 0
        assert torch.equal(al.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), L       # the other staging slot
        assert torch.equal(al.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), L
        order = [4, 0, 6, 2, 5, 1, 3]
        other = al.correlate(x, [PAIRS[i] for i in order], first=first, n=n, max_lag=L)
        assert torch.equal(other, whole[order]), L
        assert torch.equal(al.correlate(x, PAIRS[2:3], first=first, n=n, max_lag=L), whole[2:3]), L   # alone as among others
        for grid in range(1, 6):
            monkeypatch.setenv("UC_ALIGN_GRID", str(grid))
            a2 = align.Aligner()
            assert torch.equal(a2.correlate(x, PAIRS, first=first, n=n, max_lag=L), whole), (L, grid)
            a2.close()
        monkeypatch.delenv("UC_ALIGN_GRID")
        # a strided output: the guard values around every row stay
        lags = 2 * L + 1
        ys = torch.full((len(PAIRS), lags + 9), 7.0, dtype=torch.float64, device="cuda:0")
        al.correlate(x, PAIRS, first=first, n=n, max_lag=L, out=ys[:, 4:4 + lags])
        assert torch.equal(ys[:, 4:4 + lags], whole), L
        assert float(ys[:, :4].min()) == 7.0 == float(ys[:, :4].max()) and float(ys[:, 4 + lags:].min()) == 7.0 == float(ys[:, 4 + lags:].max())


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


def test_contract(align, mics, other_device):
    import torch
    L = align.lib()
    x, h = mics["f32"]
    ns = mics["ns"]
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    al = align.Aligner(0)
    assert torch.cuda.current_device() == dev0
    pairs = np.zeros(3, align.PAIR_DTYPE)
    pairs["ref"], pairs["mic"] = [0, 2, 5], [1, 2, 0]
    lag, lags = 9, 19
    out = torch.full((3, lags), 7.0, dtype=torch.float64, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=align.DTYPE_F32, n_mics=NM, n_in=ns, in_stride=0, pairs=pairs, n_pairs=3, first=10, n=ns - 20,
             max_lag=lag, out_ptr=out.data_ptr(), corr_stride=0):
        rc = L.uc_align_correlate(al._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_mics, n_in, in_stride,
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
                ("mic >= n_mics (fewer microphones)", dict(n_mics=5)),
                ("first + n > n_in", dict(first=21)), ("first + n > n_in (n alone)", dict(first=0, n=ns + 1)),
                ("first beyond the row", dict(first=ns + 1, n=1)), ("first + n wraps", dict(first=2 ** 64 - 1, n=2)),
                ("max_lag 0", dict(max_lag=0)), ("max_lag 65", dict(max_lag=65)),
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
        assert L.uc_align_last_error(), name
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())          # nothing was enqueued
    assert call() == 0                                           # and the object is as usable as before
    torch.cuda.synchronize()
    p = list(zip(pairs["ref"].tolist(), pairs["mic"].tolist()))
    assert _ratio(align, out.cpu().numpy(), h, p, 10, ns - 20, lag) <= 1.0
    assert torch.equal(out, align.Aligner(0).correlate(x, p, first=10, n=ns - 20, max_lag=lag))
    # five calls in a row that reuse (and overwrite) the same host array: the library has copied it when a call returns
    outs = [torch.empty((3, lags), dtype=torch.float64, device="cuda:0") for _ in range(5)]
    sets = []
    for i in range(5):
        sets.append([(i, 5 - i), (i, i), (5 - i, 0)])
        pairs["ref"], pairs["mic"] = [q[0] for q in sets[i]], [q[1] for q in sets[i]]
        assert call(out_ptr=outs[i].data_ptr()) == 0
    pairs["ref"] = pairs["mic"] = 0
    torch.cuda.synchronize()
    for i in range(5):
        assert _ratio(align, outs[i].cpu().numpy(), h, sets[i], 10, ns - 20, lag) <= 1.0, i
    h2 = C.c_void_p()
    assert L.uc_align_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_align_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    al.close()
    assert torch.cuda.current_device() == dev0


# ---- delays: arrays of 8 microphones rendered by the scene renderer, as the array combiner's tests make them

def _scene_arrays(array, seed, n_arrays, snr_db):
    from test_gpu_array import _arrays
    rng = np.random.default_rng(seed)
    texts, mics, beams = _arrays(array, rng, n_arrays, 8, 2000.0, snr_db, False)
    rows = [[a * 8 + m for m in range(8)] for a in range(n_arrays)]
    truth = [[beams[a][m][2] - beams[a][0][2] for m in range(8)] for a in range(n_arrays)]      # against microphone 0
    return texts, mics, beams, rows, truth


def test_delays_match_the_model_and_the_scene(align, array, scene):
    na, nb, L = 8, 104, 48
    texts, mics, beams, rows, truth = _scene_arrays(array, 21, na, 14.0)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=45)
    got, peaks = align.Aligner().delays(x, rows, max_lag=L)
    want, _ = align.delays_model(x.cpu().numpy(), rows, max_lag=L)
    got, want, truth = np.array(got), np.array(want), np.array(truth)
    assert got.shape == (na, 8) and (got[:, 0] == 0).all() and all(p[0] is None and p[1]["flags"] == 0 for p in peaks)
    print("+14 dB, %d arrays of 8: worst |gpu - model| %.3g samples, worst |gpu - scene| %.4f samples, largest runner-up %.3f"
          % (na, np.abs(got - want).max(), np.abs(got - truth).max(), max(q["runner_up"] for p in peaks for q in p[1:])))
    assert np.abs(got - want).max() <= 1e-3
    assert np.abs(got - truth).max() <= 0.01


def test_end_to_end_estimated_steering_at_minus_12_db(align, array, scene, uchirp):
    from test_gpu_array import _decoded
    na, nb = 64, 104
    texts, mics, beams, rows, truth = _scene_arrays(array, 12, na, -12.0)         # the array combiner's own end-to-end scene
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=41)
    est_beams, delays, _ = align.steer(x, rows)
    ar = array.Array()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    got_true, _ = eng.receive_many(ar.combine(x, beams), want_trace=False)
    got_est, _ = eng.receive_many(ar.combine(x, est_beams), want_trace=False)
    alone, _ = eng.receive_many(x[0::8], want_trace=False)
    ok_true, ok_est, ok_alone = _decoded(texts, got_true), _decoded(texts, got_est), _decoded(texts, alone)
    off = np.abs(np.array(delays) - np.array(truth))[:, 1:]
    print("noise, -12 dB, %d arrays of 8: true steering decodes %d / %d, estimated steering %d / %d, microphone 0 alone %d / %d; "
          "%d of %d pairs more than 0.5 samples off (worst %.1f)" % (na, ok_true, na, ok_est, na, ok_alone, na, int((off > 0.5).sum()), off.size, off.max()))
    assert ok_alone <= 8, ok_alone
    assert ok_est > ok_alone, (ok_est, ok_alone)
    assert ok_true - ok_est <= MARGIN, (ok_true, ok_est)


def test_end_to_end_estimated_steering_at_plus_14_db(align, array, scene, uchirp):
    na, nb = 16, 104
    texts, mics, beams, rows, truth = _scene_arrays(array, 16, na, 14.0)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=47)
    est_beams, delays, _ = align.steer(x, rows)
    ar = array.Array()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    got_true, _ = eng.receive_many(ar.combine(x, beams), want_trace=False)
    got_est, _ = eng.receive_many(ar.combine(x, est_beams), want_trace=False)
    differ = [a for a in range(na) if got_true[a] != got_est[a]]
    for a in differ:
        print("  array %d: estimated steering decodes %r, true steering %r (sent %r)" % (a, got_est[a], got_true[a], texts[a]))
    print("+14 dB, %d arrays of 8: %d texts differ between estimated and true steering; worst delay error %.4f samples"
          % (na, len(differ), np.abs(np.array(delays) - np.array(truth)).max()))
    assert sum(1 for t, g in zip(texts, got_true) if t in g) == na
    assert not differ, differ


def test_plain_c_host_estimates_combines_and_receives_hello_world(align, tmp_path):
    from test_align_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_align_abi_version 1 (header 1)"
    est = [ln for ln in lines if ln.startswith("microphone ")]
    assert len(est) == 3, lines
    beam = [ln for ln in lines if ln.startswith("beam of 4 microphones steered by estimated delays received")]
    assert len(beam) == 1 and "Hello World!" in beam[0], lines
