"""The link simulator on the GPU (uc_link_transmit / uc_link_noise_words, uchirp/link.py) against its float64 model
(link.model: tx.render's law with a clock offset and a fractional lead, Philox4x32-10, Box-Muller), and end to end
through the receivers of libuchirp.so, which read the rendered buffer in place.

Bounds: the signal within 8 float ulp at the peak A sqrt 2 (2.7 for the phase rounded to float, 4 for the sine, 1 for
the product); the noise within 1e-5 of the model; sample statistics within 5 standard errors.  None of them is tuned to
what the kernel gives.  Every test prints its figures before it asserts (pytest -s); the record: profiles/r07_link_tx.txt."""
import ctypes as C
import errno
import hashlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from uchirp import tx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048
FS = 78125.0


@pytest.fixture(scope="module")
def link():
    from uchirp import link as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


def _texts(rng, count, lo, hi):
    return ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(lo, hi + 1)))) for _ in range(count)]


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_noise_words_equal_the_model(link):
    from test_link_cpu import KAT
    tl = link.Link()
    for ctr, key, words in KAT:
        seed, s, c = key[0] | (key[1] << 32), ctr[2] | (ctr[3] << 32), ctr[0] | (ctr[1] << 32)
        got = _words(tl.noise_words(seed, s, c, 1))[0]
        assert " ".join("%08x" % w for w in got) == words
    rng = np.random.default_rng(5)
    total = 0
    while total < 1000000:
        seed, s, c = (int(x) for x in rng.integers(0, 1 << 63, size=3, dtype=np.uint64) * 2 + rng.integers(0, 2, size=3, dtype=np.uint64))
        n = int(rng.integers(1, 150000))
        c = min(c, (1 << 64) - n)          # (the counter does not wrap inside a call)
        assert np.array_equal(_words(tl.noise_words(seed, s, c, n)), link.noise_words(seed, s, c, n)), (seed, s, c, n)
        total += n


def test_signal_float_within_8_ulp_of_the_model(link):
    rng = np.random.default_rng(61)
    ns, nsmp = 1024, 152 * N
    texts = _texts(rng, ns, 1, 12)
    amp = rng.choice([500.0, 2000.0, 8000.0, 20000.0], size=ns)
    lead = rng.uniform(0.0, 46 * N, size=ns)
    ppm = rng.uniform(-200.0, 200.0, size=ns)
    tl = link.Link()
    got = tl.transmit(texts, lead, amp, 0.0, ppm=ppm, n_samples=nsmp).cpu().numpy()
    _, p = link.pack(texts, lead, amp, 0.0, ppm)

    def worst(s):
        m = link.signal(texts[s], float(p["lead_samples"][s]), float(p["amplitude"][s]), float(p["ppm"][s]), nsmp, FS)
        ulp = float(np.spacing(np.float32(float(p["amplitude"][s]) * 2 ** 0.5)))
        # the whole frame lies inside the buffer: its last sounding symbol, 1 + preamble + delimiter + 8 bits a character,
        # ends at this sample of the receiver's clock, and the model sounds up to there
        n_on = 2 + tx.N_PREAMBLE + 8 * len(texts[s])
        end = (float(p["lead_samples"][s]) / FS + n_on * int(tx.T_SYMBOL * tx.FS_TX) / tx.FS_TX) * FS / (1.0 + float(p["ppm"][s]) * 1e-6)
        assert end + 1 <= nsmp, (s, end)
        assert end - 16 < np.flatnonzero(m)[-1] < end, (s, end)
        return float(np.abs(got[s].astype(np.float64) - m).max() / ulp)

    with ThreadPoolExecutor(8) as ex:
        w = np.array(list(ex.map(worst, range(ns))))
    print("signal float: max error %.3f ulp of A sqrt 2 over %d streams (median of the streams' maxima %.3f)" % (w.max(), ns, np.median(w)))
    assert w.max() <= 8.0, "stream %d: %.2f ulp" % (int(w.argmax()), w.max())


def test_signal_at_the_wav_rate_is_the_wav(link):
    want = tx.tone_int16()
    tl = link.Link()
    got = tl.transmit(["Hello World!"], 0.0, float(tx.AMPLITUDE), 0.0, n_samples=want.size, fs_out=float(tx.FS_TX),
                      dtype=link.DTYPE_I16).cpu().numpy()[0]
    d = np.abs(got.astype(int) - want.astype(int))
    share = float((d != 0).mean())
    same = hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.tobytes()).hexdigest()
    print("wav rate: %d of %d samples differ (%.3f %%), max %d LSB; bytes equal to the WAV's: %s; first samples %s"
          % (int((d != 0).sum()), want.size, 100 * share, d.max(), same, got[1155:1160]))
    assert d.max() <= 1
    assert share <= 0.01, "%.3f %% of the samples differ" % (100 * share)


def test_noise_equals_the_model_and_is_white(link):
    ns, n = 64, 1 << 20
    tl = link.Link()
    z = tl.transmit([""] * ns, 0.0, 0.0, 1.0, n_samples=n, seed=0x1234567890ABCDEF).cpu().numpy().astype(np.float64)
    worst_abs = worst_rel = 0.0
    for s in range(ns):
        m, u = link.normals(0x1234567890ABCDEF, s, 0, n)
        tail = u < 2.0 ** -20
        err = np.abs(z[s] - m)
        worst_abs = max(worst_abs, float(err[~tail].max()))
        if tail.any():
            worst_rel = max(worst_rel, float((err[tail] / np.maximum(np.abs(m[tail]), 1e-300)).max()))
    print("noise: max |z - model| %.3g (u0 >= 2^-20), max relative error in the tail %.3g" % (worst_abs, worst_rel))
    assert worst_abs <= 1e-5 and worst_rel <= 1e-5
    se = 1.0 / np.sqrt(n)
    mean, var = z.mean(axis=1), z.var(axis=1)
    assert np.abs(mean).max() <= 5 * se, np.abs(mean).max()
    assert np.abs(var - 1).max() <= 5 * np.sqrt(2.0 / n), np.abs(var - 1).max()
    tot = ns * n
    assert abs(z.mean()) <= 5 / np.sqrt(tot) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / tot)
    zc = (z - mean[:, None]) / np.sqrt(var)[:, None]
    ac = np.array([[np.dot(zc[s, :-k], zc[s, k:]) / n for k in range(1, 9)] for s in range(ns)])
    assert np.abs(ac).max() <= 5 * se, np.abs(ac).max()
    cc = zc @ zc.T / n
    cc[np.diag_indices(ns)] = 0.0
    assert np.abs(cc).max() <= 5 * se, np.abs(cc).max()
    print("noise: max |mean| %.2e, |var - 1| %.2e, |autocorrelation lag 1..8| %.2e, |cross-correlation| %.2e (5 se = %.2e)"
          % (np.abs(mean).max(), np.abs(var - 1).max(), np.abs(ac).max(), np.abs(cc).max(), 5 * se))


def _case(rng, ns):
    texts = _texts(rng, ns, 1, 6)
    amp = rng.choice([500.0, 2000.0, 8000.0], size=ns)
    sigma = amp * rng.choice([0.01, 0.05, 0.2], size=ns)
    lead = rng.uniform(0.0, 6 * N, size=ns)
    ppm = rng.uniform(-200.0, 200.0, size=ns)
    return texts, lead, amp, sigma, ppm


def test_chunking_geometry_and_dtypes_are_bit_identical(link, uc_tuning, monkeypatch):
    import torch
    rng = np.random.default_rng(9)
    ns, nb = 37, 24
    texts, lead, amp, sigma, ppm = _case(rng, ns)
    kw = dict(ppm=ppm, seed=77)
    tl = link.Link()
    whole = tl.transmit(texts, lead, amp, sigma, n_samples=nb * N, **kw)
    assert float(whole.abs().max()) > 100.0
    # chunks through first_sample, into column slices of one buffer (row pitch > n_samples)
    for blocks in (1, 3, 8):
        x = torch.zeros_like(whole)
        for b in range(0, nb, blocks):
            tl.transmit(texts, lead, amp, sigma, first_sample=b * N, out=x[:, b * N:(b + blocks) * N], **kw)
        assert torch.equal(x, whole), blocks
    # chunks that are no multiple of four samples: lanes at a chunk's ends own part of a counter, rows start unaligned
    x = torch.zeros_like(whole)
    for a in range(0, nb * N, 1001):
        b = min(a + 1001, nb * N)
        tl.transmit(texts, lead, amp, sigma, first_sample=a, out=x[:, a:b], **kw)
    assert torch.equal(x, whole)
    # launch geometry: 1 .. 5 workgroups (UC_LINK_GRID, read under UC_TUNING=1 when the link is created)
    for grid in range(1, 6):
        monkeypatch.setenv("UC_LINK_GRID", str(grid))
        t2 = link.Link()
        assert torch.equal(t2.transmit(texts, lead, amp, sigma, n_samples=nb * N, **kw), whole), grid
        t2.close()
    monkeypatch.delenv("UC_LINK_GRID")
    # the three formats are one signal
    f = whole.cpu().numpy()
    i32 = tl.transmit(texts, lead, amp, sigma, n_samples=nb * N, dtype=link.DTYPE_I32, **kw).cpu().numpy()
    i16 = tl.transmit(texts, lead, amp, sigma, n_samples=nb * N, dtype=torch.int16, **kw).cpu().numpy()
    assert np.array_equal(i32, (np.round(f).astype(np.int64) * 256).astype(np.int32))
    assert np.abs(f).max() < 32767 and np.array_equal(i16, np.trunc(f).astype(np.int16))
    assert np.array_equal(i32, link.convert(f, link.DTYPE_I32)) and np.array_equal(i16, link.convert(f, link.DTYPE_I16))


def _end_to_end_case(ns):
    rng = np.random.default_rng(2048)
    texts = _texts(rng, ns, 1, 6)
    amp = rng.choice([500.0, 2000.0, 8000.0], size=ns)
    rel = rng.choice([0.01, 0.05, 0.2], size=ns)
    lead = rng.integers(25, 46, size=ns) * float(N) + rng.uniform(0.0, N, size=ns)
    return texts, lead, amp, amp * rel, rel


def test_end_to_end_recorded_and_live(link, uchirp):
    """>= 2048 streams (the stepped path of uc_receive_streams) rendered on the GPU and decoded from the device buffer by
    the complex-reference receiver: the texts equal what the same receiver decodes from the float64 model's twin of every
    stream for all but 1 % (the inputs differ by a few float ulp: only near-ties may flip); and the same transmissions
    rendered block by block through first_sample and fed to uc_receive_streams_next decode to the recorded call's texts."""
    ns, nb = 2048, 104
    texts, lead, amp, sigma, rel = _end_to_end_case(ns)
    tl = link.Link()
    eng = uchirp.Engine(uchirp.SYNC_CPLX)
    x = tl.transmit(texts, lead, amp, sigma, n_samples=nb * N, seed=31)
    got, _ = eng.receive_many(x, want_trace=False)
    # live: one block of every stream per call, rendered straight into the chunk the receiver reads
    import torch
    live = eng.live(ns)
    ring = [torch.empty((ns, N), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    parts = [[] for _ in range(ns)]
    for b in range(nb):
        chunk = tl.transmit(texts, lead, amp, sigma, first_sample=b * N, seed=31, out=ring[b & 1])
        t, _ = live.next(chunk, want_trace=False)
        for s in range(ns):
            if t[s]:
                parts[s].append(t[s])
    live.close()
    live_texts = ["".join(p) for p in parts]
    assert live_texts == got
    # the model's twin
    twin = np.empty((ns, nb * N), np.float32)
    _, p = link.pack(texts, lead, amp, sigma)

    def render(s):
        m = link.signal(texts[s], float(p["lead_samples"][s]), float(p["amplitude"][s]), 0.0, nb * N, FS)
        twin[s] = (m + float(p["sigma"][s]) * link.normals(31, s, 0, nb * N)[0]).astype(np.float32)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(render, range(ns)))
    want, _ = eng.receive_many(twin, want_trace=False)
    differ = sum(1 for a, b in zip(got, want) if a != b)
    xs = x[::64].cpu().numpy().astype(np.float64)
    print("end to end: %d of %d streams decode to another text than the model's twin; max |gpu - twin| on 32 streams %.3g"
          % (differ, ns, np.abs(xs - twin[::64]).max()))
    for r in (0.01, 0.05, 0.2):
        sel = np.flatnonzero(rel == r)
        print("  sigma = %.2f A: %d of %d streams' text contains the message" % (r, sum(1 for s in sel if texts[s] in got[s]), sel.size))
    assert differ <= ns // 100, differ


@pytest.fixture
def other_device():
    """The calling thread's current device while the link lives on device 0: device 1 where the machine has one, so that
    an entry point that left the link's device current would be seen.  With a single GPU device 0 is always current and
    the assertions on the current device cannot fail: the restore is then not tested."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_contract(link, other_device, tmp_path):
    import torch
    L = link.lib()
    dev0 = other_device
    tl = link.Link(0)
    assert torch.cuda.current_device() == dev0
    text, p = link.pack(["abc", "defgh"], 0.0, 1000.0, 0.0)
    out = torch.full((2, 4 * N), 7.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(text=text, stride=text.shape[1], p=p, n=2, ptr=out.data_ptr(), dtype=link.DTYPE_F32, fs=FS, nsmp=4 * N, pitch=0):
        rc = L.uc_link_transmit(tl._h, text.ctypes.data_as(C.c_void_p) if text is not None else None, stride,
                                p.ctypes.data_as(C.c_void_p) if p is not None else None, n, C.c_void_p(ptr), dtype, fs, 0, nsmp,
                                pitch, 1, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    bad = p.copy()
    bad["text_len"][1] = text.shape[1] + 1
    host = np.zeros(16, np.float32)
    for kw in (dict(ptr=None), dict(n=0), dict(dtype=2), dict(dtype=17), dict(p=bad), dict(fs=0.0), dict(fs=-1.0), dict(p=None),
               dict(nsmp=0), dict(pitch=N), dict(ptr=host.ctypes.data, nsmp=16), dict(stride=link.MAX_TEXT + 1)):
        rc = call(**kw)
        assert rc < 0 and rc in (-errno.EINVAL,), (kw.keys(), rc)
        assert L.uc_link_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())          # nothing was enqueued
    assert call() == 0                                           # and the link is as usable as before
    torch.cuda.synchronize()
    want = link.model(["abc", "defgh"], 0.0, 1000.0, 0.0, n_samples=4 * N)
    assert np.abs(out.cpu().numpy() - want).max() <= 8 * np.spacing(np.float32(1000.0 * 2 ** 0.5))
    rc = L.uc_link_noise_words(tl._h, 1, 2, 3, 0, C.c_void_p(out.data_ptr()), stream)
    assert rc == -errno.EINVAL and torch.cuda.current_device() == dev0
    rc = L.uc_link_noise_words(tl._h, 1, 2, 3, 4, None, stream)
    assert rc == -errno.EINVAL
    h = C.c_void_p()
    cfg = link.default_config()
    assert L.uc_link_create(torch.cuda.device_count(), C.byref(cfg), C.byref(h)) == -errno.ENODEV and not h.value
    assert L.uc_link_create(0, C.byref(link.default_config(fs_tx=0.0)), C.byref(h)) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    tl.close()
    assert torch.cuda.current_device() == dev0


def test_plain_c_host_transmits_hello_world(link, tmp_path):
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_link")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_link.c"), "-o", exe, "-L" + libdir, "-luchirp_link", "-luchirp",
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "uc_link_abi_version 2 (header 2)"
    got = [int(v) for v in lines[1].split()[1:]]
    want = tx.tone_int16()[1155:1155 + 8]
    assert list(want[:3]) == [-19999, 28207, -16859]
    assert len(got) == 8 and np.abs(np.array(got) - want).max() <= 1, (got, want)
