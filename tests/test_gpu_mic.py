"""The microphone model on the GPU (uc_mic_modulate, uchirp/mic.py): every word and every final state against the definition
in numpy integers, bit for bit -- all row and sample counts around the wave and the 16-byte group, both formats and both
scales, aligned and misaligned matrices, guard words, cuts and grids -- the contract of the call, and end to end into the
receivers and the sinc^5 of libuchirp.so.  Nothing here has a tolerance: the arithmetic is int32.  Every test prints its
figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import mic_util as mu

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
SAMPLES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 67, 2048)      # (15 .. 33: around the tile of 16 samples that goes through LDS)
FORMATS = ("f32 scale 1", "f32 scale 8388607", "i32")
GUARD = -7654321


@pytest.fixture(scope="module")
def mic():
    from uchirp import mic as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ref(mic):
    """130 rows x 2048 samples per format -- random full-scale input (a tenth of it beyond the clamps) with the quantiser's
    corner values in front, random starting states (every second row any int32, the others within 2^27, row 0 zeros) -- and
    the model's words and its states behind each of SAMPLES; made once and never written."""
    import torch
    rng = np.random.default_rng(18)
    nr, n = max(ROWS), max(SAMPLES)
    f = (rng.uniform(-1.1, 1.1, size=(nr, n)) * 2.0 ** 23).astype(np.float32)
    corners = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 8388606.5, 8388607.5, -8388607.5, 8388608.0, -8388608.0, np.nan, np.inf, -np.inf, 3.4e38, -0.0], np.float32)
    f[1::2, :16] = corners
    f[2::4, 3:19] = corners                     # (at another place in the group of four)
    u = (f / np.float32(2.0 ** 23)).astype(np.float32)
    u[1::2, :16] = [1.0, -1.0, 0.25, 2.0, 3.4e38, -3.4e38, 0.5 / 8388607, 1.5 / 8388607, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 0.99999994, -0.99999994]
    w = rng.integers(-2 ** 31, 2 ** 31, size=(nr, n)).astype(np.int32)
    w[1::2, :10] = [0, 255, 256, -1, -256, -257, -2 ** 31, -2 ** 31 + 255, -2 ** 31 + 256, 2 ** 31 - 1]
    st = rng.integers(-2 ** 27, 2 ** 27, size=(nr, 4)).astype(np.int32)
    st[1::2] = rng.integers(-2 ** 31, 2 ** 31, size=st[1::2].shape)
    st[0] = 0
    out = {"state0": st, "state0_dev": torch.from_numpy(st).to("cuda:0")}
    for fmt, x, scale in zip(FORMATS, (f, u, w), (1.0, 8388607.0, 1.0)):
        q = mic.quantise_model(x, scale)
        words, states, s, a = [], {}, st, 0
        for b in SAMPLES:                        # the model cut at every sample count: its state behind each
            wd, s = mic.model(q[:, a:b], s)
            words.append(wd)
            states[b] = s
            a = b
        out[fmt] = {"host": x, "dev": torch.from_numpy(x).to("cuda:0"), "scale": scale, "q": q, "words": np.concatenate(words, axis=1), "states": states}
    return out


def _layouts(x, nr, n, torch):
    """The first n samples of the first nr rows of x three times: rows on 16 bytes (a stride that is a multiple of 4, larger than
    n), rows one word off 16 bytes, and rows without a gap (on 16 bytes only where n is a multiple of 4)."""
    stride = (n + 3) // 4 * 4 + 8
    for name, off, st in (("on 16 bytes", 4, stride), ("one word off", 1, stride + 1), ("no gap", 0, n)):
        big = torch.full((nr * st + 8,), 0x7FC00000 if x.dtype == torch.int32 else float("nan"), dtype=x.dtype, device=x.device)
        view = big[off:off + nr * st].view(nr, st)[:, :n]
        view.copy_(x[:nr, :n])
        assert view.data_ptr() % 16 == (4 * off) % 16
        yield name, view


def _guarded(nr, n, off, torch, device="cuda:0"):
    """an output matrix of nr rows of n words inside a buffer of guard words: behind every row and behind the last one"""
    st = (n + 3) // 4 * 4 + 4 + (1 if off % 4 else 0)
    big = torch.full((nr * st + 16,), GUARD, dtype=torch.int32, device=device)
    return big, big[off:off + nr * st].view(nr, st)[:, :n]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nr", ROWS)
def test_words_and_states_equal_the_model_bit_for_bit(mic, ref, nr, fmt):
    import torch
    r = ref[fmt]
    m = mic.Mic(r["scale"], 0)
    calls = 0
    for n in SAMPLES:
        for (name, x), off in zip(_layouts(r["dev"], nr, n, torch), (4, 1, 0)):
            state = ref["state0_dev"][:nr].clone()
            big, out = _guarded(nr, n, off, torch)
            got, st = m.modulate(x, state=state, out=out)
            assert got.data_ptr() == out.data_ptr() and st.data_ptr() == state.data_ptr()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), r["words"][:nr, :n]), (n, name)
            assert np.array_equal(state.cpu().numpy(), r["states"][n][:nr]), (n, name)
            calls += 1
    # a microphone that starts: no state given
    got, st = m.modulate(r["dev"][:nr, :67].contiguous())
    want, want_st = mic.model(r["q"][:nr, :67])
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), want) and np.array_equal(st.cpu().numpy(), want_st)
    print("%d rows, %s: %d calls (%d sample counts x 3 layouts), every word and state equal" % (nr, fmt, calls, len(SAMPLES)))
    m.close()


@pytest.mark.parametrize("nr", ROWS)
def test_ragged_tails_change_no_guard_word(mic, ref, nr):
    """Rows whose last group of four is short, next to guard words: behind every row and behind the last row nothing changes,
    with 16-byte stores (rows on 16 bytes) and with dword stores (one word off)."""
    import torch
    for fmt in ("f32 scale 1", "i32"):
        r = ref[fmt]
        m = mic.Mic(r["scale"], 0)
        for n in SAMPLES:
            x = r["dev"][:nr, :n]
            for off in (4, 5, 7):
                big, out = _guarded(nr, n, off, torch)
                m.modulate(x, state=ref["state0_dev"][:nr].clone(), out=out)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), r["words"][:nr, :n]), (fmt, n, off)
                out.fill_(GUARD)
                assert int(big.min()) == GUARD == int(big.max()), (fmt, n, off)
        m.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_cuts_and_grids_give_the_same_bits(mic, ref, uc_tuning, monkeypatch, fmt):
    import torch
    r = ref[fmt]
    nr, n = 130, 300
    x = r["dev"][:, :n].contiguous()
    m = mic.Mic(r["scale"], 0)
    state = ref["state0_dev"].clone()
    whole, _ = m.modulate(x, state=state)
    want, want_st = mic.model(r["q"][:, :n], ref["state0"])
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), want) and np.array_equal(state.cpu().numpy(), want_st)
    # calls of 77, 1 and 222 samples, the state carried on the device; not synchronised in between
    st2 = ref["state0_dev"].clone()
    parts = torch.zeros_like(whole)
    a = 0
    for k in (77, 1, 222):
        m.modulate(x[:, a:a + k], state=st2, out=parts[:, a:a + k])
        a += k
    assert a == n and torch.equal(parts, whole) and torch.equal(st2, state)
    # launch geometry: 1 and 3 workgroups walk the 3 row blocks (UC_MIC_GRID, read under UC_TUNING=1 when the object is created)
    for grid in (1, 3, 2):
        monkeypatch.setenv("UC_MIC_GRID", str(grid))
        m2 = mic.Mic(r["scale"], 0)
        st3 = ref["state0_dev"].clone()
        got, _ = m2.modulate(x, state=st3)
        assert torch.equal(got, whole) and torch.equal(st3, state), grid
        m2.close()
    monkeypatch.delenv("UC_MIC_GRID")
    m.close()


def test_float_and_word_renders_of_one_link_give_the_same_bits(mic):
    """uc_link_transmit of the same streams once as float and once as DFSDM words (its I32 output: the float rounded to nearest
    even, times 256), both through Mic(scale=1): the PDM words are identical.  Amplitude and noise keep |x| below 2^23."""
    import torch
    from uchirp import link
    texts = ["Hi", "mic", "0123"]
    ln = link.Link(0)
    kw = dict(lead_samples=[700.25, 0.0, 1500.5], amplitude=[2.0e6, 3.0e4, 5.0e6], sigma=[1000.0, 50.0, 1.0e5], n_samples=6 * 2048, seed=4)
    xf = ln.transmit(texts, dtype=link.DTYPE_F32, **kw)
    xw = ln.transmit(texts, dtype=link.DTYPE_I32, **kw)
    top = float(xf.abs().max())
    print("link render: max |x| = %.0f of 2^23 = 8388608" % top)
    assert 4.0e6 < top < 2 ** 23 and xw.dtype == torch.int32
    m = mic.Mic(1.0, 0)
    bf, sf = m.modulate(xf)
    bw, sw = m.modulate(xw)
    assert torch.equal(bf, bw) and torch.equal(sf, sw)
    assert len(set(bf[2].cpu().numpy().tolist())) > 1000                    # (bits of a signal, not of silence, somewhere in the loudest row)
    m.close()
    ln.close()


@pytest.fixture
def other_device():
    """The calling thread's current device while the object lives on device 0: device 1 where the machine has one, so that
    an entry point that left the object's device current would be seen."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_contract(mic, ref, other_device):
    import torch
    L = mic.lib()
    r = ref["f32 scale 1"]
    nr, n = 5, 67
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    m = mic.Mic(1.0, 0)
    assert torch.cuda.current_device() == dev0
    x = r["dev"][:nr, :n].contiguous()
    want, want_st = r["words"][:nr, :n], r["states"][n][:nr]
    out = torch.full((nr, n), GUARD, dtype=torch.int32, device="cuda:0")
    state = ref["state0_dev"][:nr].clone()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=mic.DTYPE_F32, n_rows=nr, n_samples=n, in_stride=0, state_ptr=state.data_ptr(), out_ptr=out.data_ptr(),
             out_stride=0):
        rc = L.uc_mic_modulate(m._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_rows, n_samples, in_stride, C.c_void_p(state_ptr),
                               C.c_void_p(out_ptr), out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(nr * n, np.int32)
    refusals = [("in NULL", dict(in_ptr=None)), ("state NULL", dict(state_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no samples", dict(n_samples=0)), ("too many rows", dict(n_rows=2 ** 32)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("in_stride < n_samples", dict(in_stride=n - 1)), ("out_stride < n_samples", dict(out_stride=n - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("out_stride > 2^40", dict(out_stride=2 ** 40 + 1)),
                ("in not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("out not on 4 bytes", dict(out_ptr=out.data_ptr() + 1)),
                ("state not on 4 bytes", dict(state_ptr=state.data_ptr() + 2)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("state: host memory", dict(state_ptr=host.ctypes.data)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * n)), ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (nr * n - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (nr * n - 1))),
                ("state overlaps in", dict(state_ptr=x.data_ptr() + 4 * (nr * n - 1))), ("state overlaps out", dict(state_ptr=out.data_ptr() + 16)),
                ("out overlaps the end of state", dict(out_ptr=state.data_ptr() + 4 * (4 * nr - 1))),
                ("in overlaps state", dict(in_ptr=state.data_ptr()))]
    if two:
        far = torch.zeros((nr, n), dtype=torch.int32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far.data_ptr())), ("out: memory of another device", dict(out_ptr=far.data_ptr())),
                     ("state: memory of another device", dict(state_ptr=far.data_ptr()))]
    state0 = ref["state0_dev"][:nr]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_mic_last_error(), name
        torch.cuda.synchronize()
        assert int(out.min()) == GUARD == int(out.max()) and torch.equal(state, state0), name          # nothing was enqueued
        assert call() == 0, name                                                                     # and the object is as usable as before
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want) and np.array_equal(state.cpu().numpy(), want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    print("contract: %d refused calls, a valid call behind each gives the model's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    h2 = C.c_void_p()
    assert L.uc_mic_create(torch.cuda.device_count(), 1.0, C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_mic_create(0, 1.0, None) == -errno.EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.uc_mic_create(0, bad, C.byref(h2)) == -errno.EINVAL and not h2.value, bad
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        m.modulate(x.double())
    with pytest.raises(ValueError):
        m.modulate(x, state=torch.zeros((nr + 1, 4), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.modulate(x, out=torch.zeros((nr, n + 1), dtype=torch.int32, device="cuda:0"))
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    m.close()
    assert torch.cuda.current_device() == dev0


def test_c_host_modulates_rows_in_two_calls(mic, tmp_path):
    import re
    import subprocess
    from test_mic_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, equal = [int(v) for v in re.search(r"(\d+) words in two calls, (\d+) equal", out.stdout).groups()]
    assert n == 5 * 301 == equal and "states equal" in out.stdout


def test_code_object_shows_no_spill_and_no_scratch(mic, tmp_path, monkeypatch):
    from test_mic_cpu import code_objects
    code_objects(mic, tmp_path, monkeypatch)


# ---- end to end: the microphone in front of the receivers and the sinc^5

@pytest.mark.parametrize("variant", [0, 1])
def test_receivers_behind_the_microphone_equal_the_oracle_chain(mic, uchirp, variant):
    """The CPU test's transmissions on the device -> Mic.modulate -> Engine.receive_many(pdm=True), and block by block through
    LiveStreams.next(pdm=True): texts and traces equal, byte for byte, the receiver fed with the ORACLE's DFSDM words of the
    MODEL's bits; the decode counts are those of the CPU twin; and uc_dfsdm_sinc5_streams of the GPU's bits equals the oracle's
    sinc^5 of the model's bits."""
    import torch
    N = mu.N
    x, msgs = mu.transmissions(variant)
    ns, blocks = x.shape[0], mu.BLOCKS
    bits = mu.model_bits(x)
    words = mu.sinc5_behind_silence(bits)
    e = uchirp.Engine(variant)
    ref_t, ref_tr = e.receive_many(words)
    decoded = sum(m_ in t for m_, t in zip(msgs, ref_t))
    print("variant %d: sent %r, decoded %r" % (variant, msgs, ref_t))
    assert decoded == mu.DECODED[variant]
    m = mic.Mic(1.0, 0)
    xd = torch.from_numpy(x).to("cuda:0")
    pdm, state = m.modulate(xd)
    assert np.array_equal(pdm.cpu().numpy().view(np.uint32), bits)
    # recorded, one call
    t, tr = e.receive_many(pdm, pdm=True)
    assert t == ref_t and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(tr, ref_tr))
    # live: the microphones and the receivers block by block, both states carried on the device
    live = e.live(ns)
    st = m.new_state(ns)
    ring = torch.zeros((2, ns, N), dtype=torch.int32, device="cuda:0")
    texts, traces = [""] * ns, [[] for _ in range(ns)]
    for b in range(blocks):
        chunk, _ = m.modulate(xd[:, b * N:(b + 1) * N], state=st, out=ring[b & 1])
        t, tr = live.next(chunk, pdm=True)
        for s in range(ns):
            texts[s] += t[s]
            traces[s].append(tr[s])
    assert torch.equal(st, state)
    for s in range(ns):
        assert texts[s] == ref_t[s], s
        assert np.array_equal(np.concatenate(traces[s]).view(np.uint8), ref_tr[s].view(np.uint8)), s
    live.close()
    # the sinc^5 of libuchirp.so on the GPU's bits, behind a silent history
    hist = torch.full((ns, 4), mu.PDM_SILENCE - 2 ** 32, dtype=torch.int32, device="cuda:0")
    got = e.dfsdm_streams(pdm, hist)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), words)
    e.close()
    m.close()
