"""CPU tests of the microphone model (include/uchirp_mic.h, libuchirp_mic.so, uchirp/mic.py): the boundary, the library's two
host functions against the definition in numpy integers, chunking, how far the integrators go, how far the decimated bits lie
from the linear path, the delay of that path, what the compiler made of the kernels, and the inputs of the end-to-end GPU
test proven on the oracle alone.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import mic_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uchirp_mic.h")


@pytest.fixture(scope="module")
def mic():
    from uchirp import mic as m
    m.build()
    m.lib()
    return m


@pytest.fixture(scope="module")
def nine(mic):
    """The nine inputs quantised (scale 1), through the model once: (names, q, words, final states, max |s1|, max |s2|)."""
    inputs = mu.nine_inputs()
    q = np.stack([mic.quantise(v.astype(np.float32)) for v in inputs.values()])
    track = {}
    words, state = mic.model(q, track=track)
    return list(inputs), q, words, state, track["s1"], track["s2"]


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(uc_mic_[a-z0-9_]+)\s*\(", src)))


def test_header_is_plain_c99_and_matches_the_binding(mic, tmp_path):
    src = tmp_path / "inc.c"
    src.write_text('#include "uchirp_mic.h"\nint main(void) { return UC_MIC_ABI_VERSION == %d && UC_MIC_DTYPE_I32 == %d && '
                   'UC_MIC_DTYPE_F32 == %d && UC_MIC_Q_MAX == %d && UC_MIC_Y == %d && UC_MIC_OSR == %d && UC_MIC_SILENCE == %du ? 0 : 1; }\n'
                   % (mic.ABI_VERSION, mic.DTYPE_I32, mic.DTYPE_F32, mic.Q_MAX, mic.Y, mic.OSR, mic.SILENCE))
    exe = str(tmp_path / "inc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
    decl = _declared_functions()
    assert len(decl) == 7, decl
    L = mic.lib()
    assert not [s for s in decl if not hasattr(L, s)]
    assert sorted(mic.EXPORTS) == decl
    assert L.uc_mic_abi_version() == 1 == mic.ABI_VERSION


def test_mic_library_stands_alone(mic):
    """libuchirp_mic.so links none of the other ten libraries and imports no symbol of theirs."""
    out = subprocess.run(["readelf", "-d", mic.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.*?)\]", out)
    assert needed and not [n for n in needed if "uchirp" in n], needed
    syms = subprocess.run(["nm", "-D", "--undefined-only", mic.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\buc_[a-z0-9_]+", syms), syms


def test_no_gpu_means_no_microphone(mic):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = mic.lib().uc_mic_create(0, 1.0, C.byref(h))
    assert rc == -errno.ENODEV and not h.value
    assert b"no CPU path" in mic.lib().uc_mic_last_error()
    with pytest.raises(mic.MicError):
        mic.Mic()


def build_host(tmp_path):
    import uchirp
    from uchirp import mic
    for m in (uchirp, mic):   # the libraries the program links; a library that is there is taken as it is
        if not os.path.exists(m.LIB_PATH):
            m.build()
    libdir = os.path.join(ROOT, "ultrasonic-communication_amd")
    exe = str(tmp_path / "host_mic")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "host_mic.c"), "-o", exe, "-L" + libdir, "-luchirp_mic", "-luchirp",
                           "-Wl,-rpath," + libdir])
    return exe


def test_c_host_builds_and_fails_loudly_without_a_gpu(mic, tmp_path):
    exe = build_host(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU suite runs the program")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0
    assert "uc_mic_abi_version 1 (header 1)" in out.stdout and "uc_mic_create: -19" in out.stdout and "no CPU path" in out.stdout
    assert "silence: 8 of 8 words are 0x99999999, state 0 0 0 0" in out.stdout and "dtype 7 refused" in out.stdout
    ones = int(re.search(r"q 8388607, (\d+) ones in 9632 bits", out.stdout).group(1))
    assert abs(ones - 0.75 * 9632) <= 16, ones


# ---- 1. the host functions against the model

def test_quantise_is_the_numpy_restatement(mic):
    rng = np.random.default_rng(1)
    corners = np.array([0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 8388606.5, 8388607.0, 8388607.5, 8388608.0, -8388606.5, -8388607.0,
                        -8388608.0, 1e30, -1e30, np.nan, np.inf, -np.inf, 3.4e38, 1e-45], np.float32)
    want = [0, 0, 0, 2, 2, 0, -2, -2, 8388606, 8388607, 8388607, 8388607, -8388606, -8388607, -8388607, 8388607, -8388607, 0, 8388607,
            -8388607, 8388607, 0]
    got = mic.quantise(corners)
    print("corners:", dict(zip(corners.tolist(), got.tolist())))
    assert got.tolist() == want and got.dtype == np.int32
    assert np.array_equal(mic.quantise_model(corners), got)
    x = np.concatenate([corners, (rng.integers(-2 ** 25, 2 ** 25, size=20000) * 0.5).astype(np.float32),
                        rng.uniform(-1.2, 1.2, size=20000).astype(np.float32)])
    for scale in (1.0, 8388607.0, 0.37, 1e-30, 1e30):
        got = mic.quantise(x, scale)
        assert np.array_equal(got, mic.quantise_model(x, scale)), scale
        assert np.abs(got).max() <= mic.Q_MAX
    assert mic.quantise(np.array([1.0, -1.0, 0.25], np.float32), 8388607.0).tolist() == [8388607, -8388607, 2097152]
    # DFSDM words: the 24-bit value, -2^23 clamped; the scale is not applied
    w = np.concatenate([np.array([0, 255, 256, -1, -256, -257, -2 ** 31, -2 ** 31 + 255, -2 ** 31 + 256, 2 ** 31 - 1], np.int64),
                        rng.integers(-2 ** 31, 2 ** 31, size=20000)]).astype(np.int32)
    got = mic.quantise(w, 123.0)
    assert got[:10].tolist() == [0, 0, 1, -1, -1, -2, -8388607, -8388607, -8388607, 8388607]
    assert np.array_equal(got, mic.quantise_model(w)) and np.array_equal(got, np.maximum(w >> 8, -mic.Q_MAX))
    assert mic.quantise(np.zeros((3, 5), np.float32)).shape == (3, 5)


def test_modulate_row_is_the_model_bit_for_bit(mic, nine):
    names, q, words, state, _, _ = nine
    for k, name in enumerate(names):
        w, s = mic.modulate_row(q[k])
        assert np.array_equal(w, words[k]) and np.array_equal(s, state[k]), name
        assert s[0] == q[k, -1] and s[3] == 0
    # arbitrary states and samples beyond the quantiser's range: every sum wraps, in C as in numpy
    rng = np.random.default_rng(2)
    qs = rng.integers(-2 ** 31, 2 ** 31, size=(6, 150)).astype(np.int32)
    qs[:3] = rng.integers(-mic.Q_MAX, mic.Q_MAX + 1, size=(3, 150))
    st = rng.integers(-2 ** 31, 2 ** 31, size=(6, 4)).astype(np.int32)
    w, s = mic.model(qs, st)
    for r in range(6):
        w1, s1 = mic.modulate_row(qs[r], st[r])
        assert np.array_equal(w1, w[r]) and np.array_equal(s1, s[r]), r
    assert (s[:, 3] == 0).all() and w.dtype == np.uint32 and s.dtype == np.int32
    # one row in, one row out
    w1, s1 = mic.model(qs[0], st[0])
    assert w1.shape == (150,) and s1.shape == (4,) and np.array_equal(w1, w[0])


def test_host_functions_refuse_what_the_header_says(mic):
    L = mic.lib()
    x = np.zeros(4, np.float32)
    q = np.full(4, 7, np.int32)
    w = np.full(4, 7, np.uint32)
    st = np.zeros(4, np.int32)
    xp, qp, wp, sp = (a.ctypes.data_as(t) for a, t in ((x, C.c_void_p), (q, C.POINTER(C.c_int32)), (w, C.POINTER(C.c_uint32)), (st, C.POINTER(C.c_int32))))
    for name, args in (("in NULL", (None, 1, 1.0, 4, qp)), ("q_out NULL", (xp, 1, 1.0, 4, None)), ("dtype 2", (xp, 2, 1.0, 4, qp)),
                       ("dtype -1", (xp, -1, 1.0, 4, qp)), ("n 0", (xp, 1, 1.0, 0, qp)), ("scale 0", (xp, 1, 0.0, 4, qp)),
                       ("scale < 0", (xp, 1, -1.0, 4, qp)), ("scale nan", (xp, 1, float("nan"), 4, qp)), ("scale inf", (xp, 1, float("inf"), 4, qp))):
        assert L.uc_mic_quantise(*args) == -errno.EINVAL and L.uc_mic_last_error(), name
    for name, args in (("q NULL", (None, 4, sp, wp)), ("state NULL", (qp, 4, None, wp)), ("words NULL", (qp, 4, sp, None)), ("n 0", (qp, 0, sp, wp))):
        assert L.uc_mic_modulate_row(*args) == -errno.EINVAL and L.uc_mic_last_error(), name
    assert (q == 7).all() and (w == 7).all()
    h = C.c_void_p()
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert L.uc_mic_create(0, scale, C.byref(h)) == -errno.EINVAL and not h.value, scale
    assert L.uc_mic_create(0, 1.0, None) == -errno.EINVAL


# ---- 2. chunking

def test_any_cut_of_a_row_gives_the_words_and_state_of_one_call(mic):
    rng = np.random.default_rng(3)
    q = rng.integers(-mic.Q_MAX, mic.Q_MAX + 1, size=(3, 300)).astype(np.int32)
    st = rng.integers(-2 ** 27, 2 ** 27, size=(3, 4)).astype(np.int32)
    st[0] = 0
    whole_w, whole_s = mic.model(q, st)
    for cuts in ((77,), (77, 78), (1,), (299,), (1, 2, 3)):
        s, parts, a = st, [], 0
        for b in cuts + (300,):
            w, s = mic.model(q[:, a:b], s)
            parts.append(w)
            a = b
        assert np.array_equal(np.concatenate(parts, axis=1), whole_w) and np.array_equal(s, whole_s), cuts
    # sample by sample, through the C definition
    for r in range(3):
        s, ws = st[r], []
        for j in range(300):
            w, s = mic.modulate_row(q[r, j:j + 1], s)
            ws.append(w[0])
        assert np.array_equal(np.array(ws, np.uint32), whole_w[r]) and np.array_equal(s, whole_s[r]), r


# ---- 3. bounds

def test_integrators_stay_within_eight_y(nine):
    names, _, _, _, m1, m2 = nine
    for name, a, b in zip(names, m1, m2):
        print("%-14s max |s1| = %.3f Y, max |s2| = %.3f Y" % (name, a / 2.0 ** 25, b / 2.0 ** 25))
    assert len(names) == 9 and m1.max() <= 8 * 2 ** 25 and m2.max() <= 8 * 2 ** 25


# ---- 4. quality

def test_decimated_bits_lie_within_minus_sixty_db_of_the_linear_path(mic, nine):
    names, q, words, _, _, _ = nine
    lin = mic.linear(q)
    silence = np.full((len(names), 4), mic.SILENCE, np.uint32)
    from oracle import uco
    worst_rms = worst_max = 0.0
    for k, name in enumerate(names):
        y = uco.dfsdm_sinc5(np.concatenate([silence[k], words[k]])).astype(np.int64) >> 8
        e = (y - lin[k])[8:]
        rms, top = float(np.sqrt((e ** 2).mean())), float(np.abs(e).max())
        print("%-14s sinc5(bits) - linear: rms %.1f, max %.1f LSB of the 24-bit value" % (name, rms, top))
        worst_rms, worst_max = max(worst_rms, rms), max(worst_max, top)
        if name == "zeros":
            assert rms == 0.0 and top == 0.0 and (words[k] == mic.SILENCE).all() and not y.any()
    assert worst_rms <= 8192 and worst_max <= 32768


# ---- 5. delay

def test_linear_path_is_half_the_input_2_45_samples_late(mic, nine):
    names, q, _, _, _, _ = nine
    k = names.index("1 kHz tone")
    lin = mic.linear(q[k])
    t = np.arange(mu.N) / mu.FS
    ref = np.exp(-2j * np.pi * 1000.0 * t)[64:1984]              # 1920 samples: 24.576 periods; the window's ends weigh 1e-2
    win = np.hanning(ref.size)
    a, b = np.sum(win * ref * 0.5 * q[k, 64:1984]), np.sum(win * ref * lin[64:1984])
    delay = (np.angle(a) - np.angle(b)) / (2.0 * np.pi * 1000.0) * mu.FS
    print("1 kHz: the linear path is %.4f of half the input, %.4f samples late" % (abs(b) / abs(a), delay))
    assert abs(delay - 2.45) <= 0.05
    # the gain the header states: sinc^2(f / 78 125) of the interpolation times the sinc^5's own response (1 - 1.9e-3 at 1 kHz)
    x = 1000.0 / mu.FS
    want = np.sinc(x) ** 2 * (np.sin(np.pi * x) / (32.0 * np.sin(np.pi * x / 32.0))) ** 5
    assert abs(abs(b) / abs(a) - want) <= 2e-4, want


# ---- what the compiler made of the kernels

def code_objects(mic, tmp_path, monkeypatch):
    import test_kernel_resources as kr
    monkeypatch.setattr(kr, "LIB", mic.LIB_PATH)
    ks = kr._kernels(tmp_path)
    assert len(ks) == 2 and all("mic_kernel" in k for k in ks), sorted(ks)      # f32, i32
    for k, v in ks.items():
        assert len(v) == 1, (k, v)                    # one code object
        for e in v:
            print(k, {f: e.get(f) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
            assert e.get("vgpr_spill_count", 0) == 0 and e.get("sgpr_spill_count", 0) == 0, (k, e)
            # two tiles of 64 rows x (16 + 4) words in LDS; one wave per workgroup; 128 registers would still let four waves
            # share a SIMD (four times 65 536 microphones resident), and one wave per SIMD is what the design rests on
            assert e["private_segment_fixed_size"] == 0 and e["group_segment_fixed_size"] == 2 * 64 * 20 * 4, (k, e)
            assert e["max_flat_workgroup_size"] == 64 and e["vgpr_count"] <= 128, (k, e)
    return ks


def test_kernels_are_gfx950_without_spills_or_scratch(mic, tmp_path, monkeypatch):
    if not os.path.exists(mic.LIB_PATH):
        pytest.skip("libuchirp_mic.so not built")
    code_objects(mic, tmp_path, monkeypatch)


# ---- 6. end to end on the CPU

@pytest.mark.parametrize("variant", [0, 1])
def test_transmissions_decode_through_the_model_on_the_oracle(mic, variant):
    """Rendered transmissions at 78 125 Hz -> the model's bits -> the oracle's sinc^5 behind four UC_PDM_SILENCE words -> the
    oracle's receiver: every RX_REAL stream decodes, and all but one SYNC_CPLX stream (a bit slip at acquisition: the
    firmware's own, tests/test_dfsdm.py allows for two).  Fed directly, without the microphone, every stream decodes."""
    from oracle import uco
    assert (uco.RX_REAL, uco.SYNC_CPLX) == (0, 1)
    x, msgs = mu.transmissions(variant)
    assert x.shape == (mu.STREAMS, mu.BLOCKS * mu.N) and np.abs(x).max() < 2 ** 23
    bits = mu.model_bits(x)
    # the long rows went through the C definition: a stretch of each through the numpy model too, from the state in front of it
    q = mic.quantise_model(x[:, :4096 + 40])
    _, st = zip(*[mic.modulate_row(r[:4096]) for r in q])
    w, _ = mic.model(q[:, 4096:], np.stack(st))
    assert np.array_equal(w, bits[:, 4096:4096 + 40])
    words = mu.sinc5_behind_silence(bits)
    o = uco.Oracle(variant)
    got = [o.receive(w)[0] for w in words]
    direct = [o.receive(np.rint(r).astype(np.int32) << 8)[0] for r in x]
    print("variant %d: sent %r, through the microphone %r, directly %r" % (variant, msgs, got, direct))
    assert sum(m in g for m, g in zip(msgs, direct)) == mu.STREAMS
    assert sum(m in g for m, g in zip(msgs, got)) == mu.DECODED[variant]
