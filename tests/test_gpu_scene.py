"""The scene renderer on the GPU (uc_scene_render, uchirp/scene.py) against the link simulator (one path IS the link, bit
for bit), against its float64 model (scene.model: link.signal per path, summed; link.normals once per microphone), and
end to end through the receivers of libuchirp.so, which read the rendered buffer in place.

Bounds: a path within 8 float ulp of its own peak |g| sqrt 2 (the link's bound), one float rounding per addition of a sum
that cannot exceed the sum of the peaks; the noise within 1e-5 of the model (the link's bound) plus the rounding of the
one addition.  None of them is tuned to what the kernel gives.  Every test prints its figures before it asserts
(pytest -s)."""
import ctypes as C
import errno
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
SQRT2 = 2 ** 0.5


@pytest.fixture(scope="module")
def link():
    from uchirp import link as m
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


def _link_case(rng, ns):
    from test_gpu_link import _case
    return _case(rng, ns)


def test_one_path_is_the_link(scene, link):
    import torch
    rng = np.random.default_rng(9)
    ns, nb = 37, 24
    texts, lead, amp, sigma, ppm = _link_case(rng, ns)
    mics = [(sigma[i], [(i, amp[i], lead[i], ppm[i])]) for i in range(ns)]
    tl, sc = link.Link(), scene.Scene()
    for dtype in (link.DTYPE_F32, link.DTYPE_I32, link.DTYPE_I16):
        want = tl.transmit(texts, lead, amp, sigma, ppm=ppm, n_samples=nb * N, dtype=dtype, seed=77)
        got = sc.render(texts, mics, n_samples=nb * N, dtype=dtype, seed=77)
        assert float(want.float().abs().max()) > 100.0
        differ = int((got != want).sum())
        print("one path, dtype %d: %d of %d elements differ from uc_link_transmit" % (dtype, differ, got.numel()))
        assert torch.equal(got, want), dtype


# ---- the many-path scene of the model and noise tests: built, rendered and modelled once

class _Many:
    nm, nb, n_tx = 128, 40, 12

    def __init__(self, scene, link):
        rng = np.random.default_rng(1605)
        self.texts = _texts(rng, self.n_tx, 1, 6)
        assert len(set(self.texts)) >= 8
        counts = np.concatenate([np.arange(1, 17), rng.integers(1, 17, size=self.nm - 16)])
        rng.shuffle(counts)
        assert set(counts) == set(range(1, 17))
        self.mics = []
        for c in counts:
            gain = rng.choice([500.0, 2000.0, 8000.0, 20000.0], size=c) * rng.choice([1.0, 0.5, 0.1], size=c) * rng.choice([-1.0, 1.0], size=c)
            lead = rng.uniform(0.0, 20 * N, size=c)
            ppm = rng.uniform(-200.0, 200.0, size=c)
            tx_i = rng.integers(0, self.n_tx, size=c)
            self.mics.append((0.0, [(int(tx_i[k]), float(gain[k]), float(lead[k]), float(ppm[k])) for k in range(c)]))
        self.sigma = np.abs(np.array([m[1][0][1] for m in self.mics])) * rng.choice([0.01, 0.05, 0.2], size=self.nm)
        n = self.nb * N
        _, _, p, m = scene.pack(self.texts, self.mics)
        self.model = np.empty((self.nm, n), np.float64)
        self.sounding = np.zeros((self.nm, n), np.int32)        # paths that sound at each sample

        def one(i):
            acc = np.zeros(n, np.float64)
            for q in p[int(m["first_path"][i]):int(m["first_path"][i]) + int(m["n_paths"][i])]:
                s = link.signal(self.texts[int(q["tx"])], float(q["lead_samples"]), float(q["gain"]), float(q["ppm"]), n, FS)
                acc += s
                self.sounding[i] += s != 0.0
            self.model[i] = acc

        with ThreadPoolExecutor(8) as ex:
            list(ex.map(one, range(self.nm)))
        g = [np.array([np.float32(q[1]) for q in mc[1]], np.float64) for mc in self.mics]
        self.bound = np.array([sum(8 * float(np.spacing(np.float32(abs(a) * SQRT2))) for a in gi) +
                               (len(gi) - 1) * 0.5 * float(np.spacing(np.float32(np.abs(gi).sum() * SQRT2))) for gi in g])
        self.quiet = scene.Scene().render(self.texts, self.mics, n_samples=n, seed=5).cpu().numpy()


@pytest.fixture(scope="module")
def many(scene, link):
    return _Many(scene, link)


def test_many_paths_within_the_bound_of_the_model(scene, many):
    assert np.array_equal(scene.model(many.texts, many.mics[:3], n_samples=many.nb * N), many.model[:3])   # the shared reference IS scene.model
    top = many.sounding.max(axis=1)
    print("many paths: paths sounding at once, per microphone: max %d, mean %.2f; samples with 0 / 1 / >= 2 paths sounding: %.2f / %.2f / %.2f"
          % (top.max(), many.sounding.mean(), (many.sounding == 0).mean(), (many.sounding == 1).mean(), (many.sounding >= 2).mean()))
    assert (many.sounding == 0).any() and (many.sounding == 1).any() and (many.sounding >= 4).any()
    err = np.abs(many.quiet.astype(np.float64) - many.model).max(axis=1)
    ratio = err / many.bound
    w = int(ratio.argmax())
    print("many paths: worst |gpu - model| / bound %.4f (microphone %d, %d paths, error %.4g, bound %.4g); median %.4f"
          % (ratio[w], w, len(many.mics[w][1]), err[w], many.bound[w], np.median(ratio)))
    assert ratio.max() <= 1.0, (w, ratio[w])


def test_noise_is_drawn_once_per_microphone(scene, link, many):
    import torch
    n, seed = many.nb * N, 0x1234567890ABCDEF
    mics = [(float(many.sigma[i]), many.mics[i][1]) for i in range(many.nm)] + [(30.0, []), (0.0, []), (7.5, [])]
    sc = scene.Scene()
    got = sc.render(many.texts, mics, n_samples=n, seed=seed)
    loud = got[:many.nm].cpu().numpy()
    quiet = sc.render(many.texts, many.mics, n_samples=n, seed=seed).cpu().numpy()
    assert np.array_equal(quiet, many.quiet)                       # the seed is nothing to a noiseless microphone
    worst = 0.0
    for i in range(many.nm):
        sg = float(np.float32(many.sigma[i]))
        z = link.normals(seed, i, 0, n)[0]
        d = np.abs((loud[i].astype(np.float64) - quiet[i].astype(np.float64)) - sg * z)
        bound = 0.5 * np.spacing(np.abs(loud[i])).astype(np.float64) + 1e-5 * sg * np.maximum(1.0, np.abs(z))
        worst = max(worst, float((d / bound).max()))
    print("noise: worst |(noisy - noiseless) - sigma z(seed, m, j)| / bound %.4f over %d microphones" % (worst, many.nm))
    assert worst <= 1.0
    # microphones without paths are the link's noise of that stream index, bit for bit
    ns = many.nm + 3
    sig = np.zeros(ns, np.float32)
    sig[many.nm:] = [30.0, 0.0, 7.5]
    ref = link.Link().transmit([""] * ns, 0.0, 0.0, sig, n_samples=n, seed=seed)
    assert float(ref[many.nm].abs().max()) > 60.0 and float(ref[many.nm + 1].abs().max()) == 0.0
    assert torch.equal(got[many.nm:], ref[many.nm:])


def _scene_case(rng, nm, n_tx, lo, hi):
    from test_gpu_link import _case
    texts, lead, amp, sigma, ppm = _case(rng, n_tx)
    mics = []
    for i in range(nm):
        c = int(rng.integers(lo, hi + 1))
        k = rng.integers(0, n_tx, size=c)
        mics.append((float(sigma[k[0]]), [(int(t), float(amp[t] * rng.choice([1.0, -0.5, 0.3])), float(lead[t] + rng.uniform(0.0, 3 * N)),
                                          float(ppm[t])) for t in k]))
    return texts, mics


def test_chunking_geometry_and_dtypes_are_bit_identical(scene, link, uc_tuning, monkeypatch):
    import torch
    rng = np.random.default_rng(9)
    nm, nb = 37, 24
    texts, mics = _scene_case(rng, nm, 11, 1, 5)
    packed = scene.pack(texts, mics)
    sc = scene.Scene()
    whole = sc.render_packed(*packed, n_samples=nb * N, seed=77)
    assert float(whole.abs().max()) > 100.0
    # chunks through first_sample, into column slices of one buffer (row pitch > n_samples)
    for blocks in (1, 3, 8):
        x = torch.zeros_like(whole)
        for b in range(0, nb, blocks):
            sc.render_packed(*packed, first_sample=b * N, out=x[:, b * N:(b + blocks) * N], seed=77)
        assert torch.equal(x, whole), blocks
    # chunks that are no multiple of four samples: lanes at a chunk's ends own part of a counter, rows start unaligned
    x = torch.zeros_like(whole)
    for a in range(0, nb * N, 1001):
        b = min(a + 1001, nb * N)
        sc.render_packed(*packed, first_sample=a, out=x[:, a:b], seed=77)
    assert torch.equal(x, whole)
    # launch geometry: 1 .. 5 workgroups (UC_SCENE_GRID, read under UC_TUNING=1 when the scene is created)
    for grid in range(1, 6):
        monkeypatch.setenv("UC_SCENE_GRID", str(grid))
        s2 = scene.Scene()
        assert torch.equal(s2.render_packed(*packed, n_samples=nb * N, seed=77), whole), grid
        s2.close()
    monkeypatch.delenv("UC_SCENE_GRID")
    # the three formats are one signal
    f = whole.cpu().numpy()
    i32 = sc.render_packed(*packed, n_samples=nb * N, dtype=link.DTYPE_I32, seed=77).cpu().numpy()
    i16 = sc.render_packed(*packed, n_samples=nb * N, dtype=torch.int16, seed=77).cpu().numpy()
    assert np.array_equal(i32, link.convert(f, link.DTYPE_I32)) and np.array_equal(i16, link.convert(f, link.DTYPE_I16))


def _twin(link, texts, mics, i, n, first, seed):
    """scene.model's row of microphone i (its own operations in its own order, without packing the whole scene again)"""
    sigma, paths = mics[i]
    x = None
    for (t, g, lead, ppm) in paths:
        s = link.signal(texts[t], lead, float(np.float32(g)), float(np.float32(ppm)), n, FS, first)
        x = s if x is None else x + s
    return x + float(np.float32(sigma)) * link.normals(seed, i, first, n)[0]


def test_end_to_end_recorded_and_live(scene, link, uchirp):
    """1024 microphones (the stepped path of uc_receive_streams for SYNC_CPLX) in three classes -- one path; a direct path
    and an echo of gain 0.3, 40 .. 240 samples late; two different transmissions one after the other -- rendered on the GPU
    and decoded from the device buffer by the complex-reference receiver.  The texts equal what the same receiver decodes
    from the float32 cast of the float64 model's twin for all but 1 % of the microphones (the inputs differ by a few float
    ulp: only near-ties may flip); the one-path class decodes exactly as the link simulator's buffer does; and the scene
    rendered block by block through first_sample into a ring of two, fed to uc_receive_streams_next, gives the recorded
    call's texts.  Decode rates are printed, not asserted."""
    import torch
    nm, nb, seed = 1024, 104, 31
    n = nb * N
    rng = np.random.default_rng(2048)
    texts = _texts(rng, nm, 1, 6) + _texts(rng, nm, 1, 2) + _texts(rng, nm, 1, 2)
    amp = rng.choice([500.0, 2000.0, 8000.0], size=nm)
    rel = rng.choice([0.01, 0.05, 0.2], size=nm)
    lead = rng.integers(25, 46, size=nm) * float(N) + rng.uniform(0.0, N, size=nm)
    sym = int(0.0262 * 44100) / 44100.0 * FS                   # one symbol in samples of fs_out
    mics, sent = [], []
    for i in range(nm):
        cls = i % 3
        if cls == 0:
            paths, msgs = [(i, amp[i], lead[i], 0.0)], [texts[i]]
        elif cls == 1:
            paths, msgs = [(i, amp[i], lead[i], 0.0), (i, 0.3 * amp[i], lead[i] + rng.uniform(40.0, 240.0), 0.0)], [texts[i]]
        else:
            a, b = nm + i, 2 * nm + i
            first = rng.uniform(20.0, 25.0) * N
            second = first + (1 + 7 + 1 + 8 * len(texts[a]) + 12 + rng.uniform(2.0, 4.0)) * sym
            paths, msgs = [(a, amp[i], first, 0.0), (b, amp[i], second, 0.0)], [texts[a], texts[b]]
        mics.append((float(amp[i] * rel[i]), [(int(t), float(g), float(ld), float(pp)) for (t, g, ld, pp) in paths]))
        sent.append(msgs)
    packed = scene.pack(texts, mics)
    sc = scene.Scene()
    eng = uchirp.Engine(uchirp.SYNC_CPLX)
    x = sc.render_packed(*packed, n_samples=n, seed=seed)
    got, _ = eng.receive_many(x, want_trace=False)
    # the one-path class against the link simulator (stream index = microphone index)
    xl = link.Link().transmit([texts[m[1][0][0]] for m in mics], [m[1][0][2] for m in mics], [m[1][0][1] for m in mics],
                              [m[0] for m in mics], n_samples=n, seed=seed)
    assert torch.equal(x[0::3], xl[0::3])
    got_link, _ = eng.receive_many(xl, want_trace=False)
    assert got[0::3] == got_link[0::3]
    # live: one block of every microphone per call, rendered straight into the chunk the receiver reads
    live = eng.live(nm)
    ring = [torch.empty((nm, N), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    parts = [[] for _ in range(nm)]
    for b in range(nb):
        chunk = sc.render_packed(*packed, first_sample=b * N, seed=seed, out=ring[b & 1])
        t, _ = live.next(chunk, want_trace=False)
        for s in range(nm):
            if t[s]:
                parts[s].append(t[s])
    live.close()
    assert ["".join(p) for p in parts] == got
    # the model's twin
    twin = np.empty((nm, n), np.float32)

    assert np.array_equal(scene.model(texts, mics[:2], n_samples=4 * N, first_sample=60 * N, seed=seed),
                          np.stack([_twin(link, texts, mics, i, 4 * N, 60 * N, seed) for i in range(2)]))

    def render(i):
        twin[i] = _twin(link, texts, mics, i, n, 0, seed).astype(np.float32)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(render, range(nm)))
    want, _ = eng.receive_many(twin, want_trace=False)
    differ = sum(1 for a, b in zip(got, want) if a != b)
    xs = x[::64].cpu().numpy().astype(np.float64)
    print("end to end: %d of %d microphones decode to another text than the model's twin; max |gpu - twin| on 16 microphones %.3g"
          % (differ, nm, np.abs(xs - twin[::64]).max()))
    for cls, name in enumerate(("one path", "direct + echo 0.3", "two transmissions")):
        sel = range(cls, nm, 3)
        print("  %-18s %d of %d microphones' text contains every message" % (name + ":", sum(1 for s in sel if all(t in got[s] for t in sent[s])), len(sel)))
    assert differ <= nm // 100, differ


@pytest.fixture
def other_device():
    """The calling thread's current device while the scene lives on device 0: device 1 where the machine has one, so that
    an entry point that left the scene's device current would be seen.  With a single GPU device 0 is always current and
    the assertions on the current device cannot fail: the restore is then not tested."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_contract(scene, link, other_device):
    import torch
    L = scene.lib()
    dev0 = other_device
    if torch.cuda.device_count() < 2:
        print("contract: one GPU visible: the two-GPU branch (current device != the scene's) did not run")
    sc = scene.Scene(0)
    assert torch.cuda.current_device() == dev0
    texts = ["abc", "defgh"]
    mics = [(0.0, [(0, 1000.0, 0.0, 0.0), (1, -400.0, 300.5, 50.0)]), (0.0, [(1, 1000.0, 10.0, 0.0)])]
    text, text_len, p, m = scene.pack(texts, mics)
    out = torch.full((2, 4 * N), 7.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(text=text, stride=text.shape[1], text_len=text_len, n_tx=2, p=p, n_p=len(p), m=m, n_m=2, out_ptr=out.data_ptr(),
             dtype=link.DTYPE_F32, fs=FS, nsmp=4 * N, pitch=0):
        rc = L.uc_scene_render(sc._h, ptr(text), stride, ptr(text_len), n_tx, ptr(p), n_p, ptr(m), n_m, C.c_void_p(out_ptr), dtype, fs,
                               0, nsmp, pitch, 1, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    def changed(a, field, i, v):
        b = a.copy()
        b[field][i] = v
        return b

    long_len = text_len.copy()
    long_len[1] = text.shape[1] + 1
    host = np.zeros(16, np.float32)
    refusals = [("tx >= n_tx", dict(p=changed(p, "tx", 1, 2))),
                ("tx >= n_tx (fewer transmissions)", dict(n_tx=1)),
                ("first_path + n_paths beyond the call's", dict(m=changed(m, "first_path", 1, 3))),
                ("first_path + n_paths beyond the call's (fewer paths)", dict(n_p=2)),
                ("first_path + n_paths wraps", dict(m=changed(m, "first_path", 1, 0xFFFFFFFF))),
                ("more than 16 paths", dict(m=changed(m, "n_paths", 0, 17), p=np.repeat(p[:1], 20), n_p=20)),
                ("text_len > text_stride", dict(text_len=long_len)),
                ("text_stride > UC_LINK_MAX_TEXT", dict(stride=link.MAX_TEXT + 1)),
                ("lead not finite", dict(p=changed(p, "lead_samples", 0, np.inf))),
                ("gain not finite", dict(p=changed(p, "gain", 1, np.nan))),
                ("ppm not finite", dict(p=changed(p, "ppm", 2, -np.inf))),
                ("sigma not finite", dict(m=changed(m, "sigma", 0, np.nan))),
                ("sigma negative", dict(m=changed(m, "sigma", 1, -1.0))),
                ("dtype 2", dict(dtype=2)), ("dtype 17", dict(dtype=17)),
                ("paths NULL", dict(p=None)), ("mics NULL", dict(m=None)), ("text_len NULL", dict(text_len=None)),
                ("text NULL", dict(text=None)), ("out NULL", dict(out_ptr=None)), ("no microphones", dict(n_m=0)),
                ("fs 0", dict(fs=0.0)), ("no samples", dict(nsmp=0)), ("pitch < n_samples", dict(pitch=N)),
                ("host memory", dict(out_ptr=host.ctypes.data, nsmp=8))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_scene_last_error(), name
    assert L.uc_scene_render(None, ptr(text), text.shape[1], ptr(text_len), 2, ptr(p), len(p), ptr(m), 2, C.c_void_p(out.data_ptr()),
                             link.DTYPE_F32, FS, 0, 4 * N, 0, 1, stream) == -errno.EINVAL
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())          # nothing was enqueued
    assert call() == 0                                           # and the scene is as usable as before
    torch.cuda.synchronize()
    fresh = scene.Scene(0).render(texts, mics, n_samples=4 * N, seed=1)
    assert torch.equal(out, fresh) and float(out.abs().max()) > 1000.0
    want = scene.model(texts, mics, n_samples=4 * N)
    bound = 8 * (np.spacing(np.float32(1000.0 * SQRT2)) + np.spacing(np.float32(400.0 * SQRT2))) + 0.5 * np.spacing(np.float32(1400.0 * SQRT2))
    assert np.abs(out.cpu().numpy() - want).max() <= bound
    # overlapping ranges are allowed: microphone 1 hears microphone 0's second path and its own
    shared = changed(changed(m, "first_path", 1, 1), "n_paths", 1, 2)
    assert call(m=shared) == 0
    torch.cuda.synchronize()
    want = scene.model(texts, [mics[0], (0.0, [mics[0][1][1], mics[1][1][0]])], n_samples=4 * N)
    assert np.abs(out.cpu().numpy() - want).max() <= bound
    h = C.c_void_p()
    cfg = scene.default_config()
    assert L.uc_scene_create(torch.cuda.device_count(), C.byref(cfg), C.byref(h)) == -errno.ENODEV and not h.value
    assert L.uc_scene_create(0, C.byref(scene.default_config(fs_tx=0.0)), C.byref(h)) == -errno.EINVAL
    assert L.uc_scene_default_config(None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    sc.close()
    assert torch.cuda.current_device() == dev0


def test_plain_c_host_renders_and_receives_hello_world(scene, tmp_path):
    from test_scene_cpu import build_host
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_scene_abi_version 1 (header 1)"
    mic_lines = [ln for ln in lines if ln.startswith("microphone ")]
    assert len(mic_lines) == 4 and [int(ln.split()[1]) for ln in mic_lines] == [0, 1, 2, 3]
    # +32 dB SNR, an echo of 0.3 between 0.5 and 3 ms late, 30 blocks of noise in front: the complex-reference receiver decodes
    # all of these (the echo class of test_end_to_end_recorded_and_live is the same scene at lower SNR)
    assert all("Hello World!" in ln.split("received", 1)[1] for ln in mic_lines), mic_lines
