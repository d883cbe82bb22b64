"""The array combiner on the GPU (uc_array_combine, uchirp/array.py): shifted copies bit for bit, random beams against the
float64 model (array.model with the library's own coefficients), bit-identity under every way of cutting the work, end to
end through the scene renderer and the receivers of libuchirp.so, the contract of the call, and a plain C host.

Bound of the model test: a tap is one product and 15 fused multiply-adds, a beam of K taps K - 1 additions more; every one of
these 16 + K - 1 roundings is at most half an ulp (2^-24 relative) of a partial sum that the sum of the magnitudes
sum_k sum_t |c_k[t] x| bounds, so |gpu - model| <= (16 + K) 2^-24 sum |c x| per sample with room to spare.  It is not tuned
to what the kernel gives.  Every test prints its figures before it asserts (pytest -s).

Recorded on one MI355X (profiles/r09_array.txt): model test, worst |gpu - model| / bound 0.2632; noise test (-12 dB, 64 arrays
of 8), beams decode 64 / 64, microphone 0 alone 0 / 64, 0 beams differ from the model's twin; interferer test (+14 dB, 32
arrays of 8), beams decode 29 / 32, microphone 0 alone 3 / 32."""
import ctypes as C
import errno
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
NM, NS = 24, 3 * N + 77


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


def _texts(rng, count, lo, hi):
    return ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(lo, hi + 1)))) for _ in range(count)]


@pytest.fixture(scope="module")
def mics(scene):
    """24 microphones x (3 blocks + 77) samples: a message of amplitude 2000 at a lead of its own per microphone, plus noise
    (device tensor and host copy); rendered once and never written."""
    rng = np.random.default_rng(24)
    lead = rng.uniform(0.0, 600.0, size=NM)
    x = scene.Scene().render(["Hi"], [(300.0, [(0, 2000.0, float(lead[m]), 0.0)]) for m in range(NM)], n_samples=NS, seed=6)
    h = x.cpu().numpy()
    assert np.abs(h).max() > 2000.0
    return x, h


def _random_beams(rng, count, span, max_taps=32):
    beams = []
    for b in range(count):
        k = int(rng.integers(1, max_taps + 1)) if b >= 2 else (1, max_taps)[b]       # 1 and 32 taps are always there
        d = rng.uniform(-span, span, size=k)
        whole = rng.random(k) < 1.0 / 3.0
        d[whole] = np.round(d[whole])
        beams.append([(int(rng.integers(0, NM)), float(np.float32(rng.uniform(-1.0, 1.0))), float(d[i])) for i in range(k)])
    return beams


def _shifted(row, d):
    """row[j + d] with zeros shifted in"""
    want = np.zeros(len(row), np.float32)
    src = np.arange(len(row)) + d
    ok = (src >= 0) & (src < len(row))
    want[ok] = row[src[ok]]
    return want


def test_one_integer_tap_is_a_shifted_copy(array, mics):
    import torch
    x, h = mics
    rng = np.random.default_rng(1)
    words = rng.integers(-2 ** 27, 2 ** 27, size=(NM, NS)).astype(np.int32)        # most of them are no floats: the cast rounds
    words[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    ar = array.Array()
    delays = (0, 5, -3, 1500, -2049)
    beams = [[(m, 1.0, float(d))] for d in delays for m in (0, 7, NM - 1)]
    for name, dev, host in (("f32", x, h), ("i32", torch.from_numpy(words).to("cuda:0"), words.astype(np.float32))):
        got = ar.combine(dev, beams).cpu().numpy()
        want = np.stack([_shifted(host[m], int(d)) for ((m, _, d),) in beams])
        print("copy, %s: %d of %d elements differ from the shifted input" % (name, int((got != want).sum()), got.size))
        assert got.dtype == np.float32 and np.array_equal(got, want), name
        assert np.count_nonzero(want[-1]) > 1000 and not want[-1][:2049].any()


def test_random_beams_within_the_bound_of_the_model(array, mics):
    x, h = mics
    rng = np.random.default_rng(64)
    beams = _random_beams(rng, 64, 3000.0)
    assert sorted(set(len(b) for b in beams))[0] == 1 and max(len(b) for b in beams) == 32
    got = array.Array().combine(x, beams).cpu().numpy().astype(np.float64)
    with ThreadPoolExecutor(8) as ex:
        want = np.concatenate(list(ex.map(lambda b: array.model(h, [b], coef=array.coefficients), beams)))
        mag = np.concatenate(list(ex.map(lambda b: array.magnitude(h, [b], coef=array.coefficients), beams)))
    k = np.array([len(b) for b in beams], np.float64)[:, None]
    bound = (16.0 + k) * 2.0 ** -24 * mag
    err = np.abs(got - want)
    assert np.abs(want).max() > 1000.0 and (mag > 0).mean() > 0.5
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    w = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print("random beams: worst |gpu - model| / bound %.4f (beam %d of %d taps, sample %d, error %.4g, bound %.4g); median over the "
          "samples with a signal %.4f" % (ratio[w], w[0], len(beams[w[0]]), w[1], err[w], bound[w], np.median(ratio[bound > 0])))
    assert ratio.max() <= 1.0, (w, ratio[w])


def test_chunks_windows_grids_and_strides_are_bit_identical(array, mics, uc_tuning, monkeypatch):
    import torch
    x, h = mics
    rng = np.random.default_rng(3)
    ar = array.Array()
    for span, halo in ((3000.0, 3008), (40.0, 48)):
        beams = _random_beams(rng, 9, span, max_taps=12)
        packed = array.pack(beams)
        nb = len(beams)
        whole = ar.combine_packed(x, *packed)
        assert float(whole.abs().max()) > 100.0
        # the output range cut into calls: 1001 samples (no multiple of four: rows start unaligned, lanes hang over the end), one block
        for step in (1001, N):
            y = torch.zeros_like(whole)
            for a in range(0, NS, step):
                b = min(a + step, NS)
                ar.combine_packed(x, *packed, out_first=a, out=y[:, a:b])
            assert torch.equal(y, whole), (span, step)
        # the input handed over as the window [a - halo, b + halo) of the buffer (clipped to it): what lies outside the window and
        # inside the buffer is never needed, what lies outside the buffer reads as zero in both
        y = torch.zeros_like(whole)
        for a in range(0, NS, 1001):
            b = min(a + 1001, NS)
            lo, hi = max(0, a - halo), min(NS, b + halo)
            ar.combine_packed(x[:, lo:hi], *packed, in_first=lo, out_first=a, out=y[:, a:b])
        assert torch.equal(y, whole), span
        # absolute sample numbers far from zero
        y = ar.combine_packed(x, *packed, in_first=2 ** 40 + 3)
        assert torch.equal(y, whole), span
        # launch geometry: 1 .. 5 workgroups (UC_ARRAY_GRID, read under UC_TUNING=1 when the object is created)
        for grid in range(1, 6):
            monkeypatch.setenv("UC_ARRAY_GRID", str(grid))
            a2 = array.Array()
            assert torch.equal(a2.combine_packed(x, *packed), whole), (span, grid)
            a2.close()
        monkeypatch.delenv("UC_ARRAY_GRID")
        # strided rows on both sides (odd pitches: rows that are not 16-byte aligned)
        xs = torch.zeros((NM, NS + 131), dtype=torch.float32, device="cuda:0")[:, 3:3 + NS]
        xs.copy_(x)
        ys = torch.full((nb, NS + 57), 7.0, dtype=torch.float32, device="cuda:0")
        ar.combine_packed(xs, *packed, out=ys[:, 1:1 + NS])
        assert torch.equal(ys[:, 1:1 + NS], whole), span
        assert float(ys[:, 0].min()) == 7.0 == float(ys[:, 0].max()) and float(ys[:, 1 + NS:].min()) == 7.0 == float(ys[:, 1 + NS:].max())


# ---- end to end: arrays of 8 microphones rendered by the scene renderer, beams decoded by the complex-reference receiver

def _arrays(array, rng, n_arrays, n_mics, amp, snr_db, interferer):
    texts = _texts(rng, n_arrays, 2, 6)
    lead = rng.integers(25, 46, size=n_arrays) * float(N) + rng.uniform(0.0, N, size=n_arrays)
    delay = rng.uniform(0.0, 40.0, size=(n_arrays, n_mics))
    sigma = amp / 10.0 ** (snr_db / 20.0)
    mics = [(sigma, [(a, amp, float(lead[a] + delay[a, m]), 0.0)]) for a in range(n_arrays) for m in range(n_mics)]
    if interferer:
        other = _texts(rng, n_arrays, 2, 6)
        other_lead = rng.integers(25, 46, size=n_arrays) * float(N) + rng.uniform(0.0, N, size=n_arrays)
        other_delay = rng.uniform(0.0, 40.0, size=(n_arrays, n_mics))
        mics = [(s, p + [(n_arrays + i // n_mics, amp, float(other_lead[i // n_mics] + other_delay[i // n_mics, i % n_mics]), 0.0)])
                for i, (s, p) in enumerate(mics)]
        texts = texts + other
    beams = [[(a * n_mics + m, w, d) for (m, w, d) in array.steer(lead[a] + delay[a])]
             for a in range(n_arrays)]
    return texts, mics, beams


def _decoded(texts, got):
    return sum(1 for t, g in zip(texts, got) if t in g)


def test_end_to_end_beams_decode_what_one_microphone_cannot(array, scene, uchirp):
    import torch
    na, nm, nb = 64, 8, 104
    rng = np.random.default_rng(12)
    texts, mics, beams = _arrays(array, rng, na, nm, 2000.0, -12.0, False)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=41)
    y = array.Array().combine(x, beams)
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    got, _ = eng.receive_many(y, want_trace=False)
    alone, _ = eng.receive_many(x[0::nm], want_trace=False)
    h = x.cpu().numpy()

    def twin(a):
        rows = h[a * nm:(a + 1) * nm]
        return array.model(rows, [[(m - a * nm, w, d) for (m, w, d) in beams[a]]], coef=array.coefficients)[0].astype(np.float32)

    with ThreadPoolExecutor(8) as ex:
        t = np.stack(list(ex.map(twin, range(na))))
    want, _ = eng.receive_many(torch.from_numpy(t).to("cuda:0"), want_trace=False)
    differ = [a for a in range(na) if got[a] != want[a]]
    for a in differ:
        print("  array %d: the GPU beam decodes %r, the model's beam %r (sent %r)" % (a, got[a], want[a], texts[a]))
    ok_beam, ok_alone = _decoded(texts, got), _decoded(texts, alone)
    print("noise, -12 dB, %d arrays of %d: beams decode %d / %d, microphone 0 alone %d / %d; %d beams differ from the model's twin; "
          "max |gpu - twin| %.3g" % (na, nm, ok_beam, na, ok_alone, na, len(differ), float(np.abs(y.cpu().numpy() - t).max())))
    assert ok_beam >= 56, ok_beam
    assert ok_alone <= 8, ok_alone
    assert len(differ) <= 1, differ


def test_end_to_end_beams_decode_next_to_an_interferer(array, scene, uchirp):
    na, nm, nb = 32, 8, 104
    rng = np.random.default_rng(14)
    texts, mics, beams = _arrays(array, rng, na, nm, 2000.0, 14.0, True)
    x = scene.Scene().render(texts, mics, n_samples=nb * N, seed=43)
    y = array.Array().combine(x, beams)
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    got, _ = eng.receive_many(y, want_trace=False)
    alone, _ = eng.receive_many(x[0::nm], want_trace=False)
    ok_beam, ok_alone = _decoded(texts[:na], got), _decoded(texts[:na], alone)
    print("interferer of equal level, +14 dB, %d arrays of %d: beams decode %d / %d, microphone 0 alone %d / %d" % (na, nm, ok_beam, na, ok_alone, na))
    assert ok_beam >= 16, ok_beam
    assert ok_alone <= 10, ok_alone


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


def test_contract(array, mics, other_device):
    import torch
    L = array.lib()
    x, h = mics
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    ar = array.Array(0)
    assert torch.cuda.current_device() == dev0
    beams = [[(0, 0.5, 2.25), (5, -1.0, -7.5), (23, 0.25, 100.0)], [(2, 1.0, 0.0)]]
    taps, bm = array.pack(beams)
    want = array.model(h, beams, coef=array.coefficients)
    bound = 19.0 * 2.0 ** -24 * array.magnitude(h, beams, coef=array.coefficients)
    out = torch.full((2, NS), 7.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(h_=None, in_ptr=x.data_ptr(), dtype=array.DTYPE_F32, n_mics=NM, n_in=NS, in_stride=0, taps=taps, n_taps=len(taps), bm=bm,
             n_beams=2, out_ptr=out.data_ptr(), n_out=NS, out_stride=0):
        rc = L.uc_array_combine(ar._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_mics, 0, n_in, in_stride, ptr(taps), n_taps,
                                ptr(bm), n_beams, C.c_void_p(out_ptr), 0, n_out, out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    def changed(a, field, i, v):
        b = a.copy()
        b[field][i] = v
        return b

    host = np.zeros(NM * NS, np.float32)
    refusals = [("mic >= n_mics", dict(taps=changed(taps, "mic", 1, NM))),
                ("mic >= n_mics (fewer microphones)", dict(n_mics=23)),
                ("beam beyond n_taps", dict(bm=changed(bm, "first_tap", 1, 4))),
                ("beam beyond n_taps (fewer taps)", dict(n_taps=3)),
                ("first_tap + n_taps wraps", dict(bm=changed(bm, "first_tap", 1, 0xFFFFFFFF))),
                ("a beam of 0 taps", dict(bm=changed(bm, "n_taps", 1, 0))),
                ("a beam of 33 taps", dict(bm=changed(bm, "n_taps", 0, 33), taps=np.repeat(taps[:1], 40), n_taps=40)),
                ("delay inf", dict(taps=changed(taps, "delay_samples", 0, np.inf))),
                ("delay nan", dict(taps=changed(taps, "delay_samples", 2, np.nan))),
                ("weight nan", dict(taps=changed(taps, "weight", 1, np.nan))),
                ("weight inf", dict(taps=changed(taps, "weight", 3, -np.inf))),
                ("|delay| > 2^30", dict(taps=changed(taps, "delay_samples", 0, 2.0 ** 30 + 1.0))),
                ("|delay| > 2^30, negative", dict(taps=changed(taps, "delay_samples", 0, -2.0 ** 30 - 1.0))),
                ("in_stride < n_in", dict(in_stride=NS - 1)), ("out_stride < n_out", dict(out_stride=NS - 1)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("no microphones", dict(n_mics=0)), ("no input samples", dict(n_in=0)), ("no taps", dict(n_taps=0)),
                ("no beams", dict(n_beams=0)), ("no output samples", dict(n_out=0)),
                ("taps NULL", dict(taps=None)), ("beams NULL", dict(bm=None)), ("in NULL", dict(in_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)),
                ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * NS)),
                ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (NM * NS - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (2 * NS - 1)))]
    if two:
        far_in = torch.zeros((NM, NS), dtype=torch.float32, device="cuda:1")
        far_out = torch.zeros((2, NS), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far_in.data_ptr())), ("out: memory of another device", dict(out_ptr=far_out.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_array_last_error(), name
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())          # nothing was enqueued
    assert call() == 0                                           # and the object is as usable as before
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.abs(want).max() > 500.0 and (np.abs(got - want) <= bound).all()
    assert torch.equal(out, array.Array(0).combine(x, beams))
    # overlapping tap ranges are allowed: beam 1 is beam 0's last tap and its own
    shared = changed(changed(bm, "first_tap", 1, 2), "n_taps", 1, 2)
    assert call(bm=shared) == 0
    torch.cuda.synchronize()
    b2 = [beams[0], [beams[0][2], beams[1][0]]]
    assert (np.abs(out.cpu().numpy() - array.model(h, b2, coef=array.coefficients)) <= 19.0 * 2.0 ** -24 * array.magnitude(h, b2, coef=array.coefficients)).all()
    # five calls in a row that reuse (and overwrite) the same host arrays: the library has copied them when a call returns
    outs = [torch.empty((2, NS), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    sets = []
    for i in range(5):
        bi = [[(i, 0.5, 2.25 + i), (5 + i, -1.0, -7.5 * i), (23 - i, 0.25, 100.0)], [(2 + i, 1.0, float(i))]]
        sets.append(bi)
        taps[:] = array.pack(bi)[0]
        assert call(out_ptr=outs[i].data_ptr()) == 0
    taps["weight"] = 0.0
    torch.cuda.synchronize()
    for i in range(5):
        w = array.model(h, sets[i], coef=array.coefficients)
        assert (np.abs(outs[i].cpu().numpy() - w) <= 19.0 * 2.0 ** -24 * array.magnitude(h, sets[i], coef=array.coefficients)).all(), i
        assert np.array_equal(outs[i][1].cpu().numpy(), _shifted(h[2 + i], i)), i
    h2 = C.c_void_p()
    assert L.uc_array_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_array_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    ar.close()
    assert torch.cuda.current_device() == dev0


def test_plain_c_host_renders_combines_and_receives_hello_world(array, tmp_path):
    from test_array_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_array_abi_version 1 (header 1)"
    beam = [ln for ln in lines if ln.startswith("beam of 8 microphones received")]
    assert len(beam) == 1 and "Hello World!" in beam[0], lines
