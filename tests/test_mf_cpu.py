"""CPU tests of the pulse compressor (include/uchirp_mf.h, libuchirp_mf.so, uchirp/mf.py): the boundary, the notebook's
"Compress chirp in time domain" case in float64, the host functions (spectrum, plan, selection rule, arrival) against numpy
and brute force, every refusal that needs no GPU, the float32 emulation inside the header's bound on the GPU tests' own
inputs (this fixes the constant), the chain scene -> down-converter -> compressor -> arrivals in float64, the sanitizer
target, and what the compiler made of the kernels."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import mf_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_mf.h")
PKG = os.path.join(ROOT, "ultrasonic-communication_amd")


@pytest.fixture(scope="module")
def mf():
    from uchirp import mf as m
    m.build()
    m.lib()
    return m


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_mf_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(mf, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_mf.h"\nint main(void) { return sizeof(uc_mf_job) == 8 && sizeof(uc_mf_candidate) == 16 && '
                   'sizeof(uc_mf_record) == 80 && UC_MF_ABI_VERSION == %d && UC_MF_DTYPE_I32 == %d && UC_MF_DTYPE_F32 == %d && '
                   'UC_MF_DTYPE_C32 == %d && UC_MF_OUT_COMPLEX == %d && UC_MF_OUT_REAL == %d && UC_MF_OUT_POWER == %d && UC_MF_OUT_MAG == %d && '
                   'UC_MF_POINTS == %d && UC_MF_MAX_TAPS == %d && UC_MF_MAX_SETS == %d && UC_MF_CANDIDATES == %d && UC_MF_ERROR_C == %d ? 0 : 1; }\n'
                   % (mf.ABI_VERSION, mf.DTYPE_I32, mf.DTYPE_F32, mf.DTYPE_C32, mf.OUT_COMPLEX, mf.OUT_REAL, mf.OUT_POWER, mf.OUT_MAG,
                      mf.POINTS, mf.MAX_TAPS, mf.MAX_SETS, mf.CANDIDATES, mf.ERROR_C))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    assert C.sizeof(mf.MfJob) == 8 == mf.JOB_DTYPE.itemsize and C.sizeof(mf.MfCandidate) == 16 == mf.CANDIDATE_DTYPE.itemsize
    assert C.sizeof(mf.MfRecord) == 80 == mf.RECORD_DTYPE.itemsize
    assert [mf.RECORD_DTYPE.fields[k][1] for k in ("cand", "sum", "count", "n_cand", "reserved")] == \
        [getattr(mf.MfRecord, k).offset for k in ("cand", "sum", "count", "n_cand", "reserved")] == [0, 64, 68, 72, 76]
    assert (mf.POINTS, mf.MAX_TAPS, mf.CANDIDATES) == (2048, 1664, 4)
    decl = _declared_functions()
    assert len(decl) == 10, decl
    L = mf.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(mf.EXPORTS) == decl
    assert L.uc_mf_abi_version() == 1 == mf.ABI_VERSION


def test_mf_library_stands_alone(mf):
    """libuchirp_mf.so links none of the other libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", mf.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", mf.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_compressor(mf):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = mf.lib().uc_mf_create(0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in mf.lib().uc_mf_last_error()
    with pytest.raises(mf.MfError):
        mf.Mf()


def build_host(tmp_path):
    import uchirp
    from uchirp import mf
    for m in (uchirp, mf):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    exe = str(tmp_path / "host_mf")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_mf.c"), "-o", exe, "-L" + PKG, "-luchirp_mf", "-luchirp", "-lm",
                           "-Wl,-rpath," + PKG])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(mf, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "uc_mf_abi_version 1 (header 1)" in out.stdout and "a crest of height 3 at offset 2" in out.stdout
    assert "0 taps refused" in out.stdout and "uc_mf_create: -19" in out.stdout and "no CPU path" in out.stdout


def test_notebook_case_in_float64(mf):
    """ChirpSimulation.ipynb, 'Compress chirp in time domain': lfilter(matched_filter, 1, receive_buf) and its
    ifft(fft * fft) twin.  mf.model on the notebook's own float64 values equals both to 1e-9 of the peak (they differ from
    each other by 2.7e-16 of it), and the crest lies where the chirp ends: index 881."""
    import scipy.signal
    buf, down = u.notebook_case()
    assert buf.size == 1764 and down.size == 882
    want = scipy.signal.lfilter(down, 1, buf)
    ref = np.zeros_like(buf)
    ref[:down.size] = down
    twin = np.fft.ifft(np.fft.fft(buf) * np.fft.fft(ref))
    peak = np.abs(want).max()
    got = mf.model(buf, down, exact=True)[0]
    print("notebook: model - lfilter %.3g, model - ifft(fft fft) %.3g, lfilter - ifft(fft fft) %.3g of the peak %.6g"
          % (np.abs(got - want).max() / peak, np.abs(got - twin).max() / peak, np.abs(want - twin).max() / peak, peak))
    assert np.abs(got - want).max() <= 1e-9 * peak and np.abs(got - twin).max() <= 1e-9 * peak
    assert int(np.argmax(np.abs(got))) == 881 == int(np.argmax(np.abs(want)))
    # as the library reads it (inputs and taps rounded to float32) the crest stays
    assert int(np.argmax(np.abs(mf.model(buf, down)[0]))) == 881
    # and the record of the one segment names it: hop 1165, two segments, the crest in the first
    assert mf.plan(882, 0, 0, 1764) == (1165, 0, 2)
    e = np.zeros(1165 + 2, np.float32)
    e[1:] = (np.abs(got[:1166]) ** 2).astype(np.float32)
    rec = mf.select(e)
    assert int(rec["cand"][0]["offset"]) == 881 and rec["n_cand"] > 4
    off, top = mf.arrival(rec["cand"][0])
    assert abs(off - 881.0) <= 0.01 and abs(top / peak - 1.0) <= 1e-3


def test_spectrum_is_within_one_ulp_of_numpys(mf):
    rng = np.random.default_rng(41)
    buf, down = u.notebook_case()
    sets = [u.templates(T)[s] for T in u.TAPS for s in (0, 1)] + [down.astype(np.complex64), u.chain_template().astype(np.complex64),
                                                                  np.array([1.0], np.complex64), np.array([0.0, 1j], np.complex64)]
    sets.append((rng.standard_normal(882) * 10.0 ** rng.uniform(-20, 20, 882)).astype(np.complex64))
    worst = 0.0
    for h in sets:
        got = mf.spectrum(h)
        want = np.fft.fft(np.concatenate([h.astype(np.complex128), np.zeros(2048 - h.size)])) / 2048.0
        # numpy's transform has its own error, a few 2^-53 of the largest bin: part of the yardstick
        slack = 8.0 * 2.0 ** -53 * np.abs(want).max()
        for g, w in ((got.real, want.real), (got.imag, want.imag)):
            ulp = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(((np.abs(g.astype(np.float64) - w) - slack) / ulp).max()))
    print("spectrum: worst |library - numpy| %.3f ulp of float32" % worst)
    assert worst <= 1.0
    assert mf.spectrum(np.array([2.0], np.complex64)).tobytes() == np.full(2048, 2.0 / 2048, np.complex64).tobytes()


def test_plan_agrees_with_a_count_by_hand(mf):
    rng = np.random.default_rng(42)
    for T in (1, 2, 255, 256, 882, 1023, 1024, 1664):
        S = 2048 - T - 1
        for pos0 in (0, 1, S - 1, S, 2 ** 40 + 5, 2 ** 63 + 11, 2 ** 64 - 10000):
            for _ in range(6):
                first = int(rng.integers(0, 3000))
                n = int(rng.integers(1, 6000))
                hop, k0, ns = mf.plan(T, pos0, first, n)
                # brute force in Python integers: the set of segments the outputs fall in
                q0 = pos0 + first
                segs = sorted({q // S for q in (q0, q0 + n - 1)} | {(q0 + i) // S for i in range(0, n, max(1, S // 2))})
                assert hop == S and k0 == segs[0] and ns == len(segs) == segs[-1] - segs[0] + 1, (T, pos0, first, n)
    assert mf.plan(1, 2 ** 64 - 1, 0, 1) == (2046, (2 ** 64 - 1) // 2046, 1)
    for args in ((1, 2 ** 64 - 1, 0, 2), (1, 2 ** 64 - 1, 1, 1), (1, 0, 0, 0), (0, 0, 0, 1), (1665, 0, 0, 1)):
        with pytest.raises(mf.MfError):
            mf.plan(*args)


def _same_record(a, b):
    return a.tobytes() == b.tobytes()


def test_select_is_the_rule(mf):
    rng = np.random.default_rng(43)
    for i in range(300):
        hop = int(rng.choice([1, 2, 3, 7, 383, 1023, 1791, 2046]))
        e = (rng.standard_normal(hop + 2) ** 2 * 10.0 ** rng.uniform(-30, 30)).astype(np.float32)
        if i % 3 == 0:
            e = np.round(e / max(e.max(), 1e-30) * 3.0).astype(np.float32)          # many ties and plateaus
        lo = int(rng.integers(0, hop))
        hi = int(rng.integers(lo + 1, hop + 1))
        for a, b in ((0, hop), (lo, hi)):
            assert _same_record(mf.select(e, a, b), mf.select_model(e, a, b)), (i, hop, a, b)
    # crafted: ties keep the lower q first; a plateau's LAST sample is the candidate (>= on the left, > on the right)
    r = mf.select(np.array([0, 5, 0, 5, 0, 5, 0, 5, 0, 5, 0, 0], np.float32))
    assert [int(c["offset"]) for c in r["cand"]] == [0, 2, 4, 6] and r["n_cand"] == 5 and r["count"] == 10 and r["sum"] == 25.0
    r = mf.select(np.array([0, 1, 3, 3, 3, 1, 0, 0], np.float32))
    assert r["n_cand"] == 1 and tuple(r["cand"][0]) == (3, 3.0, 3.0, 1.0) and not r["cand"][1]["peak"]
    # a greater one later goes in front; fewer than four leave zero slots
    r = mf.select(np.array([0, 2, 0, 9, 0, 4, 0, 0], np.float32))
    assert [(int(c["offset"]), float(c["peak"])) for c in r["cand"]] == [(2, 9.0), (4, 4.0), (0, 2.0), (0, 0.0)] and r["n_cand"] == 3
    # the neighbours outside the range count, the outputs outside do not
    r = mf.select(np.array([9, 1, 2, 3, 4, 9, 0], np.float32), 1, 4)
    assert r["n_cand"] == 0 and r["count"] == 3 and r["sum"] == 9.0
    r = mf.select(np.array([0, 1, 2, 3, 4, 1, 0], np.float32), 1, 4)
    assert r["n_cand"] == 1 and int(r["cand"][0]["offset"]) == 3
    # nothing at all
    r = mf.select(np.zeros(385, np.float32))
    assert r["n_cand"] == 0 and r["count"] == 383 and r["sum"] == 0.0 and not r["cand"]["peak"].any() and not r["cand"]["offset"].any()
    assert _same_record(r, mf.select_model(np.zeros(385, np.float32)))


def test_arrival_is_the_parabola_through_the_roots(mf):
    rng = np.random.default_rng(44)
    for _ in range(300):
        b = float(rng.uniform(0.1, 1e6))
        a, c = b * rng.uniform(0.0, 1.0), b * rng.uniform(0.0, 0.999)
        cand = (int(rng.integers(0, 2046)), np.float32(a * a), np.float32(b * b), np.float32(c * c))
        off, top = mf.arrival(cand)
        ra, rb, rc = (np.sqrt(np.float64(v)) for v in cand[1:])
        d = ra - 2.0 * rb + rc
        delta = (ra - rc) / (2.0 * d) if d < 0 else 0.0
        assert off == cand[0] + delta and top == rb - (ra - rc) * delta / 4.0
        assert (off, top) == mf.arrival_model(cand)
        if rb >= ra and rb > rc:
            assert abs(off - cand[0]) <= 0.5 and top >= rb
    # a sampled parabola of amplitudes is recovered exactly
    amp = lambda t: 7.0 - 0.5 * (t - 0.3) ** 2
    off, top = mf.arrival((10, np.float64(amp(-1.0) ** 2), np.float64(amp(0.0) ** 2), np.float64(amp(1.0) ** 2)))
    assert abs(off - 10.3) <= 1e-6 and abs(top - 7.0) <= 1e-6
    assert mf.arrival((5, 4.0, 4.0, 4.0)) == (5.0, 2.0)
    for bad in ((1, -1.0, 1.0, 1.0), (1, 1.0, float("nan"), 1.0), (1, 1.0, 1.0, float("inf"))):
        with pytest.raises(mf.MfError):
            mf.arrival(bad)


def test_refusals_that_need_no_gpu(mf):
    L = mf.lib()
    hop, k0, ns = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert L.uc_mf_plan(1, 0, 0, 1, None, C.byref(k0), C.byref(ns)) == -errno.EINVAL
    assert L.uc_mf_plan(1, 0, 0, 1, C.byref(hop), None, C.byref(ns)) == -errno.EINVAL
    assert L.uc_mf_plan(1, 0, 0, 1, C.byref(hop), C.byref(k0), None) == -errno.EINVAL
    taps = np.ones(4, np.float32)
    spec = np.zeros(4096, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.uc_mf_spectrum(None, 2, vp(spec)) == -errno.EINVAL and L.uc_mf_spectrum(vp(taps), 2, None) == -errno.EINVAL
    assert L.uc_mf_spectrum(vp(taps), 0, vp(spec)) == -errno.EINVAL and L.uc_mf_spectrum(vp(taps), 1665, vp(spec)) == -errno.EINVAL
    bad = taps.copy()
    bad[3] = np.inf
    assert L.uc_mf_spectrum(vp(bad), 2, vp(spec)) == -errno.EINVAL and b"not finite" in L.uc_mf_last_error()
    e = np.zeros(6, np.float32)
    rec = np.zeros(1, mf.RECORD_DTYPE)
    assert L.uc_mf_select(None, 4, 0, 4, vp(rec)) == -errno.EINVAL and L.uc_mf_select(vp(e), 4, 0, 4, None) == -errno.EINVAL
    for hop_, lo, hi in ((0, 0, 1), (2047, 0, 1), (4, 2, 2), (4, 3, 2), (4, 0, 5)):
        assert L.uc_mf_select(vp(e), hop_, lo, hi, vp(rec)) == -errno.EINVAL, (hop_, lo, hi)
    assert L.uc_mf_select(vp(e), 4, 0, 4, vp(rec)) == 0
    off, top = C.c_double(), C.c_double()
    c = mf.MfCandidate(1, 1.0, 2.0, 1.0)
    assert L.uc_mf_arrival(None, C.byref(off), C.byref(top)) == -errno.EINVAL
    assert L.uc_mf_arrival(C.byref(c), None, C.byref(top)) == -errno.EINVAL and L.uc_mf_arrival(C.byref(c), C.byref(off), None) == -errno.EINVAL
    # the entry points that take an object refuse a missing one before anything else
    assert L.uc_mf_create(0, None) == -errno.EINVAL
    assert L.uc_mf_set_templates(None, vp(taps), 1, 2) == -errno.EINVAL
    job = np.zeros(1, mf.JOB_DTYPE)
    assert L.uc_mf_run(None, vp(spec), mf.DTYPE_F32, 1, 8, 0, vp(job), 1, 0, 0, 8, vp(spec), mf.OUT_REAL, 0, None, None) == -errno.EINVAL
    assert L.uc_mf_last_error()


def test_emulation_stays_inside_the_bound_on_the_gpu_tests_inputs(mf):
    """The float32 emulation (pocketfft, complex64; the library's own H) of the definition against the float64 model, as a
    multiple of 2^-24 ||a_k|| ||h||, on every row, template and position the GPU comparison uses, on the notebook's chirp and
    on the chain's base-band rows.  Recorded: 0.2 - 0.4 where the window is full; 1.3 - 2.06 at pos0 = S - 1, where the first
    window holds ONE sample (DFSDM words through the one-tap template: 2.06); 1.56 on the notebook's chirp; 0.88 on the
    chain.  UC_MF_ERROR_C is four times the worst, rounded up: 9."""
    worst = {}
    for kind in u.DTYPES:
        for T in u.TAPS:
            want = u.model_rows(kind, T)
            for pos0 in u.positions(T):
                y, _ = mf.emulate32(u.rows(kind), u.templates(T), u.JOBS, pos0)
                B = mf.bound(u.rows(kind), u.templates(T), u.JOBS, pos0)
                r = float((np.abs(y - want) / (2.0 ** -24 * B)).max())
                key = "full windows" if pos0 != u.P - T - 2 else "one-sample window"
                worst[key] = max(worst.get(key, 0.0), r)
    buf, down = u.notebook_case()
    y, _ = mf.emulate32(buf.astype(np.float32), down)
    worst["notebook"] = float((np.abs(y - mf.model(buf, down)) / (2.0 ** -24 * mf.bound(buf.astype(np.float32), down))).max())
    x = chain_rows()
    z, yc, _ = u.chain64(x)
    z32 = z.astype(np.complex64)
    y, _ = mf.emulate32(z32, u.chain_template())
    worst["chain"] = float((np.abs(y - yc) / (2.0 ** -24 * mf.bound(z32, u.chain_template()))).max())
    print("emulation: worst |emulate32 - model| / (2^-24 ||a_k|| ||h||): " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert 0.0 < max(worst.values()) <= mf.ERROR_C / 4.0, worst
    assert mf.ERROR_C == int(np.ceil(4.0 * 2.06))


def test_emulation_reads_its_windows_as_the_definition_says(mf):
    """emulate32's powers of a segment are those of the outputs -1 .. S, whatever pos0 is: the records the GPU test derives
    from them line up with the model's."""
    T = 255
    want = np.abs(u.model_rows("c32", T)) ** 2
    for pos0 in u.positions(T):
        hop, k0, ns = mf.plan(T, pos0, 0, u.NS)
        y, e = mf.emulate32(u.rows("c32"), u.templates(T), u.JOBS, pos0)
        assert e.shape == (4, ns, hop + 2)
        for k in range(ns):
            q = (k0 + k) * hop - pos0 + np.arange(-1, hop + 1)               # elements of the row
            ok = (q >= 0) & (q < u.NS)
            assert ok.any() and np.allclose(e[:, k][:, ok], want[:, q[ok]], rtol=1e-4, atol=1e-4 * want.max())


# --------------------------------------------------------------------------------------------------------------- the chain

CHAIN_THREE = [(u.chain_sigma(), [(0, u.AMPLITUDE * 1.0, 500.25, 0.0), (0, u.AMPLITUDE * 0.5, 650.75, 0.0), (0, u.AMPLITUDE * 0.7, 8000.6, 0.0)])]


def chain_rows(mics=None, seed=21):
    """the GPU closure's two microphones of two paths each (150.5 samples apart), or the microphones given: float32 values"""
    from uchirp import scene
    return scene.model([""], u.CHAIN_MICS if mics is None else mics, n_samples=u.CHAIN_SAMPLES, seed=seed, **u.CHAIN_FMT).astype(np.float32)


def _chain_errors(mics, seed):
    x = chain_rows(mics, seed)
    _, y, cand = u.chain64(x)
    errs = []
    for row, (_, paths) in zip(cand, mics):
        truth = sorted(u.chain_truth(ld) for (_, _, ld, _) in paths)
        hop = u.P - u.MF_TAPS - 1
        for k, seg in enumerate(row):
            here = [t for t in truth if k * hop <= t < (k + 1) * hop]
            if not here:
                continue
            top = sorted(seg[:len(here)])                                   # the highest candidates, by position
            # the arrivals ARE the highest candidates: each lies within a sample of its truth ...
            assert len(top) == len(here) and all(abs(p - t) < 1.0 for (p, _, _), t in zip(top, here)), (k, top, here)
            # ... and no other candidate comes within 1e-3 (relative height) of the lowest of them: float32 cannot reorder them
            if len(seg) > len(here):
                assert seg[len(here)][1] < (1.0 - 1e-3) * min(h for (_, h, _) in top), (k, seg[:len(here) + 1])
            errs += [p - t for (p, _, _), t in zip(top, here)]
    return np.array(errs)


def test_chain_in_float64(mf):
    """Three arrivals of the up chirp (16 -> 19 kHz, 26.2 ms) at fractional leads with gains 1, 0.5 and 0.7, two of them
    150.5 samples apart, in noise at +1 dB of the strongest; ddc.model at a 17.5 kHz carrier with a 65-tap low-pass and
    D = 8; mf.model with the Hann-weighted base-band chirp of 255 taps padded to 256.  The three arrivals are the three
    highest candidates of their segment and nothing else comes near; the same for the two microphones of two paths that
    the GPU closure renders.  Recorded position errors against the truth: 0.01 - 0.13 decimated samples at this noise
    (without noise: at most 0.011, the residue of the paths' overlap); mf_util.CHAIN_RECORDED holds the worst."""
    e3 = _chain_errors(CHAIN_THREE, 21)
    e2 = _chain_errors(u.CHAIN_MICS, 21)
    quiet = _chain_errors([(0.0, p) for (_, p) in CHAIN_THREE], 21)
    print("chain: position errors of three arrivals %s, of the closure's four %s, without noise %s (decimated samples)"
          % (np.round(e3, 4), np.round(e2, 4), np.round(quiet, 4)))
    assert len(e3) == 3 and len(e2) == 4
    assert max(np.abs(e3).max(), np.abs(e2).max()) <= u.CHAIN_RECORDED and np.abs(quiet).max() <= 0.02


# ------------------------------------------------------------------------------------------------- the build's own checks

def test_sanitize_mf_is_clean(mf):
    """`make sanitize-mf`: csrc/uc_mf_api.cpp and tests/cpp/san_mf.cpp under ASan + UBSan, a stand-alone program on the CPU."""
    out = subprocess.run(["make", "-C", PKG, "sanitize-mf"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert re.search(r"san_mf: \d+ plans, \d+ spectra, \d+ records", out.stdout), out.stdout[-2000:]


def test_kernels_are_gfx950_without_spills_or_scratch(mf, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    if not os.path.exists(mf.LIB_PATH):
        pytest.skip("libuchirp_mf.so not built")
    monkeypatch.setattr(kr, "LIB", mf.LIB_PATH)
    ks = kr._kernels(tmp_path)
    assert len(ks) == 3 and all("mf_kernel" in k for k in ks), sorted(ks)        # i32, f32, c32
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        e = v[0]
        assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
        assert e["private_segment_fixed_size"] == 0, (k, e)
        assert e["vgpr_count"] <= 256, (k, e)         # __launch_bounds__(128, 2): 2 waves per SIMD
        # two tiles of 2048 complex values, the two small twiddle tables and 20 words the waves exchange: 35 KiB
        assert e["group_segment_fixed_size"] == (2 * 2 * 2048 + 2 * 256 + 2 * 128 + 20) * 4, (k, e)
        assert 4 * e["group_segment_fixed_size"] <= 160 * 1024
