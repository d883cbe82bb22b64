"""The link simulator and the scene renderer on the GPU far from sample 0 (first_sample from 2^31 to 2^52): a live node
at 78 125 Hz passes 2^32 samples in 15 hours, and the calls accept first_sample up to 2^52.

The reference is the float64 model (uchirp.link.signal, uchirp.scene.model), which tests/test_far_cpu.py holds within
0.01 float ulp of the definition in rational arithmetic at these very cases (tests/far_util.py).  The bounds are the
headers' own: a stream or a path within 8 float ulp of its peak A sqrt 2, one float rounding per addition of a scene's sum,
the noise within 1e-5 of the model (absolute for u0 >= 2^-20, relative in the tail).  None of them is tuned to what the
kernels give.  Every test prints its figures before it asserts (pytest -s); the record: profiles/far_positions.txt."""
from fractions import Fraction as F

import numpy as np
import pytest

import far_util as fu

pytestmark = pytest.mark.gpu

N = fu.N
FS = fu.FS
SQRT2 = 2 ** 0.5
CASES = fu.link_cases()
TOP = 2 ** 52 - 2 ** 20


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
def tl(link):
    return link.Link()


@pytest.fixture(scope="module")
def sc(scene):
    return scene.Scene()


def _bits(x):
    return x.view(np.uint32)


# ---- a. the link's signal against the model, every sample

@pytest.mark.parametrize("c", CASES, ids=fu.case_name)
def test_link_signal_within_8_ulp_of_the_model(link, tl, c):
    n, first = c["n_samples"], c["first_sample"]
    got = tl.transmit(c["texts"], c["lead"], c["amp"], 0.0, ppm=c["ppm"], n_samples=n, first_sample=first).cpu().numpy()
    ratio = np.zeros(fu.N_STREAMS)
    for s in range(fu.N_STREAMS):
        m = link.signal(c["texts"][s], float(c["lead"][s]), float(c["amp"][s]), float(c["ppm"][s]), n, FS, first)
        sounding = np.flatnonzero(m)
        assert sounding.size > 30000 and sounding[0] >= N and sounding[-1] < n - 1            # the whole frame, inside the call
        ratio[s] = np.abs(got[s].astype(np.float64) - m).max() / fu.ulp_of_peak(c["amp"][s])
        assert not _bits(got[s])[m == 0.0].any(), (s, "not +0 where the model is silent")
    w = int(ratio.argmax())
    print("link signal, first_sample %-10s: worst |gpu - model| %.3f ulp of A sqrt 2 (stream %d, ppm %+.0f); median of the streams %.3f"
          % (fu.case_name(c), ratio[w], w, c["ppm"][w], np.median(ratio)))
    assert ratio.max() <= 8.0, (w, ratio[w])


# ---- b. with ppm 0 the signal belongs to j - lead alone

@pytest.mark.parametrize("shift, den", [(2 ** 32, 16), (2 ** 40, 16), (TOP, 1)], ids=["2^32", "2^40", "2^52-2^20"])
def test_common_shift_of_lead_and_first_sample_changes_no_bit(link, tl, shift, den):
    import torch
    rng = np.random.default_rng(52)
    ns, n, first = 16, 24 * N, 3 * N
    texts = [chr(int(v)) for v in rng.integers(33, 127, size=ns)]
    amp = rng.choice(fu.AMPS, size=ns)
    lead = [F(int(v), den) for v in rng.integers(4 * N * den, 9 * N * den, size=ns)]      # sixteenths (integers at the top)
    far = [ld + shift for ld in lead]
    assert all(F(float(v)) == v for v in lead + far)                                       # both leads are doubles
    assert first + shift <= link.MAX_FIRST_SAMPLE
    near = tl.transmit(texts, [float(v) for v in lead], amp, 0.0, n_samples=n, first_sample=first)
    moved = tl.transmit(texts, [float(v) for v in far], amp, 0.0, n_samples=n, first_sample=first + shift)
    differ = int((near.view(torch.int32) != moved.view(torch.int32)).sum())
    print("shift %s: %d of %d elements differ; peak %.1f" % (shift, differ, near.numel(), float(near.abs().max())))
    assert float(near.abs().max()) > 20000.0
    assert torch.equal(near.view(torch.int32), moved.view(torch.int32))


# ---- c. the noise of link_kernel itself, across the counter's high word

def _noise_bars(z, model, u):
    tail = u < 2.0 ** -20
    err = np.abs(z - model)
    worst_abs = float(err[~tail].max())
    worst_rel = float((err[tail] / np.maximum(np.abs(model[tail]), 1e-300)).max()) if tail.any() else 0.0
    return worst_abs, worst_rel


@pytest.mark.parametrize("first", [2 ** 34 - 6, 2 ** 52 - 8192], ids=["2^34-6", "2^52-8192"])
def test_link_noise_equals_the_model_where_the_counter_has_a_high_word(link, tl, first):
    ns, n, seed = 4, 8192, 0x1234567890ABCDEF
    z = tl.transmit([""] * ns, 0.0, 0.0, 1.0, n_samples=n, first_sample=first, seed=seed).cpu().numpy().astype(np.float64)
    assert (first + n - 1) // 4 >> 32 != 0 and (first == 2 ** 52 - 8192 or first // 4 >> 32 == 0)
    worst_abs = worst_rel = 0.0
    for s in range(ns):
        m, u = link.normals(seed, s, first, n)
        a, r = _noise_bars(z[s], m, u)
        worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
    print("link noise at %d: max |z - model| %.3g (u0 >= 2^-20), max relative error in the tail %.3g" % (first, worst_abs, worst_rel))
    assert worst_abs <= 1e-5 and worst_rel <= 1e-5
    assert len({z[s].tobytes() for s in range(ns)}) == ns


# ---- d. cuts, grids and formats at 2^40 + 3

def test_link_cuts_grids_and_formats_at_2_40_plus_3(link, tl, uc_tuning, monkeypatch):
    import torch
    c = CASES[-1]
    n, first = c["n_samples"], c["first_sample"]
    assert first == 2 ** 40 + 3
    sigma = 0.05 * c["amp"]
    kw = dict(ppm=c["ppm"], seed=77)
    args = (c["texts"], c["lead"], c["amp"], sigma)
    whole = tl.transmit(*args, n_samples=n, first_sample=first, **kw)
    assert float(whole.abs().max()) > 20000.0
    x = torch.zeros_like(whole)
    for a in range(0, n, 1001):
        b = min(a + 1001, n)
        tl.transmit(*args, first_sample=first + a, out=x[:, a:b], **kw)
    assert torch.equal(x, whole)
    for grid in (1, 2, 3):
        monkeypatch.setenv("UC_LINK_GRID", str(grid))
        t2 = link.Link()
        assert torch.equal(t2.transmit(*args, n_samples=n, first_sample=first, **kw), whole), grid
        t2.close()
    monkeypatch.delenv("UC_LINK_GRID")
    f = whole.cpu().numpy()
    i32 = tl.transmit(*args, n_samples=n, first_sample=first, dtype=link.DTYPE_I32, **kw).cpu().numpy()
    i16 = tl.transmit(*args, n_samples=n, first_sample=first, dtype=torch.int16, **kw).cpu().numpy()
    assert np.array_equal(i32, link.convert(f, link.DTYPE_I32)) and np.array_equal(i16, link.convert(f, link.DTYPE_I16))


# ---- e. the scene

class _Scene:
    """Three microphones with 1, 5 and 16 paths whose frames begin within +-4096 samples of each other, 2 to 5 blocks
    into the call; two of the 16 are silent over the whole call, one whose frame ended long ago and one that has not begun."""

    def __init__(self, base, scene):
        rng = np.random.default_rng([base % (1 << 63), 5])
        self.base, self.n = base, 24 * N
        self.texts = [chr(int(v)) for v in rng.integers(33, 127, size=4)]
        centre = base + 3 * N + N // 2

        def path(silent=None):
            ppm = float(np.float32(rng.choice(fu.PPMS)))
            gain = float(rng.choice(fu.AMPS) * rng.choice([1.0, 0.5, 0.1]) * rng.choice([-1.0, 1.0]))
            off = F(int(rng.integers(-4096 * 1024, 4096 * 1024)), 1024)
            lead = float((centre + off) * (1 + F(ppm) / 10 ** 6)) if silent is None else float(silent)
            return (int(rng.integers(0, 4)), gain, lead, ppm)

        many = [path() for _ in range(16)]
        many[5], many[11] = path(2 ** 20), path(base + 2 ** 30)
        self.silent = (5, 11)
        self.mics = [(0.0, [path()]), (0.0, [path() for _ in range(5)]), (0.0, many)]
        self.model = scene.model(self.texts, self.mics, n_samples=self.n, first_sample=base)
        self.model.setflags(write=False)
        self.bound = []
        for i, (_, paths) in enumerate(self.mics):
            g = np.array([np.float32(q[1]) for k, q in enumerate(paths) if not (i == 2 and k in self.silent)], np.float64)
            self.bound.append(sum(8 * fu.ulp_of_peak(a) for a in g) + (len(g) - 1) * 0.5 * float(np.spacing(np.float32(np.abs(g).sum() * SQRT2))))


_SCENES = {}


def _scene_at(base, scene):
    if base not in _SCENES:
        _SCENES[base] = _Scene(base, scene)
    return _SCENES[base]


SCENE_BASES = [2 ** 33, 2 ** 40, TOP]
SCENE_IDS = ["2^33", "2^40", "2^52-2^20"]


@pytest.mark.parametrize("base", SCENE_BASES, ids=SCENE_IDS)
def test_scene_within_the_bound_of_the_model(scene, link, sc, base):
    s = _scene_at(base, scene)
    for k in s.silent:                            # silent over the whole call, by the model of the path alone
        t, g, lead, ppm = s.mics[2][1][k]
        assert not link.signal(s.texts[t], lead, g, ppm, s.n, FS, base).any()
    got = sc.render(s.texts, s.mics, n_samples=s.n, first_sample=base).cpu().numpy()
    assert all(np.abs(s.model[i]).max() > 40.0 for i in range(3))
    err = np.abs(got.astype(np.float64) - s.model).max(axis=1)
    ratio = err / np.array(s.bound)
    for i in range(3):
        print("scene, first_sample %-10s microphone %d (%2d paths): worst |gpu - model| / bound %.4f (error %.4g, bound %.4g)"
              % (SCENE_IDS[SCENE_BASES.index(base)], i, len(s.mics[i][1]), ratio[i], err[i], s.bound[i]))
    assert not _bits(got)[s.model == 0.0].any()                     # +0 where no path sounds
    assert ratio.max() <= 1.0, ratio


@pytest.mark.parametrize("base", SCENE_BASES, ids=SCENE_IDS)
def test_scene_noise_and_cuts(scene, link, sc, base):
    import torch
    s = _scene_at(base, scene)
    seed = 0x1234567890ABCDEF
    sigma = [float(np.float32(0.05 * abs(m[1][0][1]))) for m in s.mics]
    mics = [(sg, m[1]) for sg, m in zip(sigma, s.mics)]
    packed = scene.pack(s.texts, mics)
    quiet = sc.render(s.texts, s.mics, n_samples=s.n, first_sample=base, seed=seed).cpu().numpy()
    whole = sc.render_packed(*packed, n_samples=s.n, first_sample=base, seed=seed)
    loud = whole.cpu().numpy()
    worst = 0.0
    for i in range(3):                            # one draw per microphone, keyed by its index and the absolute sample
        z = link.normals(seed, i, base, s.n)[0]
        d = np.abs((loud[i].astype(np.float64) - quiet[i].astype(np.float64)) - sigma[i] * z)
        bound = 0.5 * np.spacing(np.abs(loud[i])).astype(np.float64) + 1e-5 * sigma[i] * np.maximum(1.0, np.abs(z))
        worst = max(worst, float((d / bound).max()))
    print("scene noise at %s: worst |(noisy - noiseless) - sigma z(seed, m, j)| / bound %.4f" % (SCENE_IDS[SCENE_BASES.index(base)], worst))
    assert worst <= 1.0
    x = torch.zeros_like(whole)
    for a in range(0, s.n, 1001):
        b = min(a + 1001, s.n)
        sc.render_packed(*packed, first_sample=base + a, out=x[:, a:b], seed=seed)
    assert torch.equal(x, whole)


def test_scene_with_one_path_is_the_link_at_2_40(scene, link, sc, tl):
    import torch
    c = CASES[-1]
    n, first = c["n_samples"], c["first_sample"]
    sigma = 0.05 * c["amp"]
    mics = [(sigma[i], [(i, c["amp"][i], c["lead"][i], c["ppm"][i])]) for i in range(fu.N_STREAMS)]
    want = tl.transmit(c["texts"], c["lead"], c["amp"], sigma, ppm=c["ppm"], n_samples=n, first_sample=first, seed=77)
    got = sc.render(c["texts"], mics, n_samples=n, first_sample=first, seed=77)
    print("one path at 2^40+3: %d of %d elements differ from uc_link_transmit" % (int((got != want).sum()), got.numel()))
    assert float(want.abs().max()) > 20000.0 and torch.equal(got, want)


# ---- f. the reach: first_sample <= 2^52

def test_one_sample_past_the_reach_is_refused_and_the_next_call_is_right(scene, link):
    import torch
    top = link.MAX_FIRST_SAMPLE
    assert top == 2 ** 52
    n = 24 * N
    texts, amp = ["a", "Z"], [2000.0, 20000.0]
    lead = [float(top + 2 * N + 77), float(top + 3 * N)]
    mics = [(0.0, [(0, amp[0], lead[0], 0.0), (1, -amp[1], lead[1], 0.0)]), (0.0, [(1, amp[1], lead[1], 0.0)])]
    tl, sc = link.Link(), scene.Scene()
    out = torch.full((2, n), 7.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(link.LinkError, match=r"rc=-22"):
        tl.transmit(texts, lead, amp, 0.0, first_sample=top + 1, out=out)
    with pytest.raises(link.LinkError, match=r"rc=-22"):
        tl.transmit(texts, lead, amp, 0.0, first_sample=2 ** 63, out=out)
    with pytest.raises(scene.SceneError, match=r"rc=-22"):
        sc.render(texts, mics, first_sample=top + 1, out=out)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())              # nothing was enqueued
    # the last position the calls accept: the link's bits from a link that was never refused, and the model
    tl.transmit(texts, lead, amp, 0.0, first_sample=top, out=out)
    fresh = link.Link().transmit(texts, lead, amp, 0.0, first_sample=top, n_samples=n)
    assert torch.equal(out, fresh)
    want = link.model(texts, lead, amp, 0.0, n_samples=n, first_sample=top)
    ratio = np.abs(out.cpu().numpy() - want).max(axis=1) / np.array([fu.ulp_of_peak(a) for a in amp])
    print("link at first_sample 2^52 after a refusal: worst |gpu - model| %.3f ulp of A sqrt 2" % ratio.max())
    assert np.abs(want).max(axis=1).min() > 2000.0 and ratio.max() <= 8.0
    out.fill_(7.0)
    sc.render(texts, mics, first_sample=top, out=out)
    assert torch.equal(out, scene.Scene().render(texts, mics, first_sample=top, n_samples=n))
    want = scene.model(texts, mics, n_samples=n, first_sample=top)
    bound = np.array([8 * (fu.ulp_of_peak(amp[0]) + fu.ulp_of_peak(amp[1])) + 0.5 * float(np.spacing(np.float32((amp[0] + amp[1]) * SQRT2))),
                      8 * fu.ulp_of_peak(amp[1])])
    ratio = np.abs(out.cpu().numpy() - want).max(axis=1) / bound
    print("scene at first_sample 2^52 after a refusal: worst |gpu - model| / bound %.4f" % ratio.max())
    assert ratio.max() <= 1.0
