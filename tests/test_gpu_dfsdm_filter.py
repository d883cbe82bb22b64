"""The DFSDM filter on the GPU (uc_dfsdm_run, uchirp/dfsdm.py): every output word, every final state and every guard word
against uc_dfsdm_filter_row (the definition in plain C, which tests/test_dfsdm_filter_cpu.py pins to the FIR), bit for bit --
every configuration, row counts around the wave, word counts around the tile, rows on and off 16 bytes, grids, cuts, the
existing sinc^5 kernel behind the microphone model, the contract of the call, two streams and destroy, and the large calls.
Nothing here has a tolerance: the arithmetic is int32.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import dfsdm_util as du
import large_util as lu

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 64, 65, 130)            # around the wave of 64 rows
WORDS = (1, 15, 16, 17, 33, 67)       # around the tile of 16 words
PATTERNS = ("random", "ones", "single bits")
CONFIGS = du.CONFIGS + [du.WORD_PATH_INTEGRATOR]
GUARD = -7654321
WORDS_BEFORE = {"random": 5, "ones": 0, "single bits": 0}      # (random rows also start from random states, between boundaries)


@pytest.fixture(scope="module")
def dfsdm():
    from uchirp import dfsdm as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def inputs(torch):
    """130 rows x 67 words per pattern and their starting states, on the host and on the device; made once, never written.
    Random: every row its own words and (odd rows) any int32 in its state.  Ones: every row ones.  Single bits: row r is the
    pattern rolled by r words."""
    rng = np.random.default_rng(27)
    nr, n = max(ROWS), max(WORDS)
    out = {}
    for name in PATTERNS:
        if name == "random":
            w = rng.integers(0, 1 << 32, size=(nr, n), dtype=np.uint64).astype(np.uint32)
            st = du.random_state(rng, nr)
            st[::2] = 0
        else:
            base = du.pattern(name, n)
            w = np.stack([np.roll(base, r) for r in range(nr)])
            st = np.zeros((nr, 16), np.int32)
        out[name] = {"w": w, "st": st, "w_dev": torch.from_numpy(w.view(np.int32)).to("cuda:0"), "st_dev": torch.from_numpy(st).to("cuda:0")}
    return out


_REF = {}


def reference(dfsdm, inputs, cfg, name):
    """uc_dfsdm_filter_row of all 130 rows, cut at every word count of WORDS: {n: (out [130, n_out(n)], state [130, 16])};
    computed once per (configuration, pattern) and shared."""
    key = (tuple(cfg), name)
    if key not in _REF:
        d, wb = inputs[name], WORDS_BEFORE[name]
        res = {}
        nr = d["w"].shape[0]
        outs = [[] for _ in range(nr)]
        sts = [d["st"][r] for r in range(nr)]
        a = 0
        for n in WORDS:
            for r in range(nr):
                o, sts[r] = dfsdm.filter_row(d["w"][r, a:n], cfg, state=sts[r], words_before=wb + a)
                outs[r].append(o)
            a = n
            res[n] = (np.stack([np.concatenate(o) for o in outs]), np.stack(sts))
            assert res[n][0].shape[1] == dfsdm.plan(cfg, wb, n)
        _REF[key] = res
    return _REF[key]


def _layouts(x, nr, n, torch):
    """The first n words of the first nr rows of x twice: rows on 16 bytes (a stride that is a multiple of 4: the tile path)
    and rows one word off 16 bytes with an odd stride (the direct path)."""
    stride = (n + 3) // 4 * 4 + 8
    for name, off, st in (("on 16 bytes", 4, stride), ("one word off", 1, stride + 1)):
        big = torch.full((nr * st + 8,), 0x5A5A5A5A, dtype=torch.int32, device=x.device)
        view = big[off:off + nr * st].view(nr, st)[:, :n]
        view.copy_(x[:nr, :n])
        assert view.data_ptr() % 16 == (4 * off) % 16 and (st % 4 == 0) == (off == 4)
        yield name, view


def _guarded(nr, n, off, torch):
    """an output matrix of nr rows of n words inside a buffer of guard words: in front, behind every row, behind the last"""
    st = (n + 3) // 4 * 4 + 4 + (1 if off % 4 else 0)
    big = torch.full((nr * st + 16,), GUARD, dtype=torch.int32, device="cuda:0")
    return big, big[off:off + nr * st].view(nr, st)[:, :n]


def _expect(big, out, want):
    """the whole buffer: the expected words where the matrix lies, the guard everywhere else"""
    e = np.full(big.numel(), GUARD, np.int32)
    nr, n = want.shape
    if n == 0:
        return e
    off = (out.data_ptr() - big.data_ptr()) // 4
    st = out.stride(0) if nr > 1 else n
    for r in range(nr):
        e[off + r * st:off + r * st + n] = want[r]
    return e


# ---- 1. the sweep

@pytest.mark.parametrize("cfg", CONFIGS, ids=str)
def test_words_states_and_guards_equal_the_definition(dfsdm, torch, inputs, cfg):
    f = dfsdm.Dfsdm(cfg, 0)
    calls = 0
    for name in PATTERNS:
        d, wb = inputs[name], WORDS_BEFORE[name]
        ref = reference(dfsdm, inputs, cfg, name)
        for nr in ROWS:
            for n in WORDS:
                want, want_st = ref[n][0][:nr], ref[n][1][:nr]
                for (lname, x), off in zip(_layouts(d["w_dev"], nr, n, torch), (4, 1)):
                    state = d["st_dev"][:nr].clone()
                    big, out = _guarded(nr, want.shape[1], off, torch)
                    got, st = f.run(x, state=state, words_before=wb, out=out)
                    assert st.data_ptr() == state.data_ptr() and got.data_ptr() == out.data_ptr()
                    torch.cuda.synchronize()
                    assert np.array_equal(big.cpu().numpy(), _expect(big, out, want)), (name, nr, n, lname)
                    assert np.array_equal(state.cpu().numpy(), want_st), (name, nr, n, lname)
                    calls += 1
    # filters that start: no state given
    got, st = f.run(inputs["random"]["w_dev"][:5, :67].contiguous())
    for r in range(5):
        o, s = dfsdm.filter_row(inputs["random"]["w"][r], cfg)
        assert np.array_equal(got[r].cpu().numpy(), o) and np.array_equal(st[r].cpu().numpy(), s), r
    print("%r (%s path): %d calls (3 patterns x 5 row counts x 6 word counts x 2 layouts), every word, state and guard word equal"
          % (cfg, "word" if cfg[1] % 32 == 0 else "bit", calls))
    f.close()


# ---- 2. the paths

@pytest.mark.parametrize("cfg", [(3, 32, 1, 2, 0), (3, 20, 1, 0, 0), du.WORD_PATH_INTEGRATOR, (5, 32, 1, 2, 0), (0, 1024, 1, 8, 0)], ids=str)
def test_tile_path_and_direct_path_give_the_same_bits(dfsdm, torch, inputs, cfg):
    """Dense rows on 16 bytes take the tiles through LDS; a pointer off by 4 bytes and an odd stride take the direct way.
    (3, 32) and (3, 64, I = 3) run the word path -- the second one crosses an integrator boundary every sixth word --, (3, 20)
    the bit path.  400 words: 25 tiles."""
    rng = np.random.default_rng(31)
    nr, n = 70, 400
    w = rng.integers(0, 1 << 32, size=(nr, n), dtype=np.uint64).astype(np.uint32)
    st0 = du.random_state(rng, nr)
    wd = torch.from_numpy(w.view(np.int32)).to("cuda:0")
    f = dfsdm.Dfsdm(cfg, 0)
    n_out = dfsdm.plan(cfg, 7, n)
    assert wd.data_ptr() % 16 == 0 and wd.stride(0) % 4 == 0
    s_tile = torch.from_numpy(st0).to("cuda:0")
    tile_out = torch.full((nr, (n_out + 3) // 4 * 4 + 4), GUARD, dtype=torch.int32, device="cuda:0")
    assert tile_out.data_ptr() % 16 == 0
    f.run(wd, state=s_tile, words_before=7, out=tile_out[:, :n_out])
    off = torch.full((nr * (n + 1) + 1,), 0, dtype=torch.int32, device="cuda:0")
    x = off[1:].view(nr, n + 1)[:, :n]
    x.copy_(wd)
    assert x.data_ptr() % 16 == 4 and x.stride(0) % 2 == 1
    s_direct = torch.from_numpy(st0).to("cuda:0")
    big, direct_out = _guarded(nr, n_out, 1, torch)
    f.run(x, state=s_direct, words_before=7, out=direct_out)
    torch.cuda.synchronize()
    assert torch.equal(tile_out[:, :n_out], direct_out) and torch.equal(s_tile, s_direct)
    assert int((tile_out[:, n_out:] != GUARD).sum()) == 0
    for r in (0, 63, 64, 69):
        o, s = dfsdm.filter_row(w[r], cfg, state=st0[r], words_before=7)
        assert np.array_equal(direct_out[r].cpu().numpy(), o) and np.array_equal(s_direct[r].cpu().numpy(), s), r
    print("%r: %d rows x %d words -> %d outputs, tiles and direct equal" % (cfg, nr, n, n_out))
    f.close()


# ---- 3. grids and cuts

@pytest.mark.parametrize("cfg", [(3, 32, 1, 2, 0), (3, 20, 1, 0, 0), (1, 7, 3, 0, -3)], ids=str)
def test_grids_and_cuts_give_the_same_bits(dfsdm, torch, inputs, uc_tuning, monkeypatch, cfg):
    d = inputs["random"]
    x = d["w_dev"]                                          # 130 rows x 67 words: three row blocks
    f = dfsdm.Dfsdm(cfg, 0)
    state = d["st_dev"].clone()
    whole, _ = f.run(x, state=state, words_before=5)
    ref = reference(dfsdm, inputs, cfg, "random")[67]
    assert np.array_equal(whole.cpu().numpy(), ref[0]) and np.array_equal(state.cpu().numpy(), ref[1])
    # 1 + 16 + 17 + 33 words, the state carried on the device, words_before advanced by the caller; not synchronised in between
    st2 = d["st_dev"].clone()
    parts = torch.full_like(whole, GUARD)
    a = k_out = 0
    counts = []
    for k in du.CUTS:
        n = dfsdm.plan(cfg, 5 + a, k)
        f.run(x[:, a:a + k], state=st2, words_before=5 + a, out=parts[:, k_out:k_out + n])
        a, k_out = a + k, k_out + n
        counts.append(n)
    assert a == 67 and k_out == whole.shape[1] and torch.equal(parts, whole) and torch.equal(st2, state), counts
    # launch geometry: 1 and 2 workgroups walk the 3 row blocks (UC_DFSDM_GRID, read under UC_TUNING=1 when the object is created)
    for grid in (1, 2):
        monkeypatch.setenv("UC_DFSDM_GRID", str(grid))
        f2 = dfsdm.Dfsdm(cfg, 0)
        st3 = d["st_dev"].clone()
        got, _ = f2.run(x, state=st3, words_before=5)
        assert torch.equal(got, whole) and torch.equal(st3, state), grid
        f2.close()
    monkeypatch.delenv("UC_DFSDM_GRID")
    print("%r: outputs per cut %r; grids of 1, 2 and 3 workgroups equal" % (cfg, counts))
    f.close()


# ---- 4. against the existing kernel

def test_receivers_configuration_equals_the_sinc5_kernel_behind_the_microphone(dfsdm, torch):
    """Mic.modulate of three rows of 70 samples -> Dfsdm.run at (5, 32, 1, 2, 0) equals uc_dfsdm_sinc5_streams of the same
    words behind a history of UC_PDM_SILENCE, from output 4 on, bit for bit."""
    import uchirp
    from uchirp import mic
    rng = np.random.default_rng(33)
    x = (rng.uniform(-1.0, 1.0, (3, 70)) * mic.Q_MAX).astype(np.float32)
    x[2] = 0.0
    m = mic.Mic(1.0, 0)
    pdm, _ = m.modulate(torch.from_numpy(x).to("cuda:0"))
    f = dfsdm.Dfsdm((5, 32, 1, 2, 0), 0)
    got, _ = f.run(pdm)
    e = uchirp.Engine(uchirp.RX_REAL)
    # (host arrays: the library pads its staging rows, 70-word device rows would not lie on 16 bytes)
    hist = np.full((3, 4), 0xAAAAAAAA, np.uint32)
    want = e.dfsdm_streams(pdm.cpu().numpy().view(np.uint32), hist)
    got = got.cpu().numpy()
    assert got.shape == want.shape == (3, 70)
    assert np.array_equal(got[:, 4:], want[:, 4:]) and np.abs(got[:2, 4:].astype(np.int64)).max() > 2 ** 24
    assert not got[2, 5:].any()                             # the silent microphone: 0 behind the fill
    e.close()
    f.close()
    m.close()


# ---- 5. the contract

@pytest.fixture
def other_device(torch):
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_contract(dfsdm, torch, inputs, other_device):
    L = dfsdm.lib()
    cfg = (3, 20, 1, 0, 0)
    nr, n, wb = 5, 67, 5
    d = inputs["random"]
    ref = reference(dfsdm, inputs, cfg, "random")[n]
    want, want_st = ref[0][:nr], ref[1][:nr]
    n_out = want.shape[1]
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    f = dfsdm.Dfsdm(cfg, 0)
    assert torch.cuda.current_device() == dev0
    x = d["w_dev"][:nr, :n].contiguous()
    out = torch.full((nr, n_out), GUARD, dtype=torch.int32, device="cuda:0")
    state0 = d["st_dev"][:nr]
    state = state0.clone()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), n_rows=nr, n_words=n, in_stride=0, words_before=wb, state_ptr=state.data_ptr(), out_ptr=out.data_ptr(),
             out_stride=0):
        rc = L.uc_dfsdm_run(f._h if h_ is None else h_, C.c_void_p(in_ptr), n_rows, n_words, in_stride, words_before, C.c_void_p(state_ptr),
                            C.c_void_p(out_ptr), out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(nr * max(n, n_out), np.int32)
    refusals = [("pdm NULL", dict(in_ptr=None)), ("state NULL", dict(state_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no words", dict(n_words=0)), ("too many rows", dict(n_rows=2 ** 32)),
                ("words_before + n_words > 2^58", dict(words_before=2 ** 58)),
                ("in_stride < n_words", dict(in_stride=n - 1)), ("out_stride < n_out", dict(out_stride=n_out - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("out_stride > 2^40", dict(out_stride=2 ** 40 + 1)),
                ("pdm not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("out not on 4 bytes", dict(out_ptr=out.data_ptr() + 1)),
                ("state not on 4 bytes", dict(state_ptr=state.data_ptr() + 2)),
                ("pdm: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("state: host memory", dict(state_ptr=host.ctypes.data)),
                ("out overlaps pdm", dict(out_ptr=x.data_ptr() + 4 * n)), ("out overlaps the end of pdm", dict(out_ptr=x.data_ptr() + 4 * (nr * n - 1))),
                ("pdm overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (nr * n_out - 1))),
                ("state overlaps pdm", dict(state_ptr=x.data_ptr() + 4 * (nr * n - 1))), ("state overlaps out", dict(state_ptr=out.data_ptr() + 16)),
                ("out overlaps the end of state", dict(out_ptr=state.data_ptr() + 4 * (16 * nr - 1))),
                ("pdm overlaps state", dict(in_ptr=state.data_ptr()))]
    if two:
        far = torch.zeros((nr, max(n, n_out)), dtype=torch.int32, device="cuda:1")
        refusals += [("pdm: memory of another device", dict(in_ptr=far.data_ptr())), ("out: memory of another device", dict(out_ptr=far.data_ptr())),
                     ("state: memory of another device", dict(state_ptr=far.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_dfsdm_last_error(), name
        torch.cuda.synchronize()
        assert int(out.min()) == GUARD == int(out.max()) and torch.equal(state, state0), name          # nothing was enqueued
        assert call() == 0, name                                                                     # and the object is as usable as before
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(state.cpu().numpy(), want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    print("contract: %d refused calls, a valid call behind each gives the definition's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    # a call without outputs is a call: the states move on, one word of `out` would be the most it may own and none is written
    f2 = dfsdm.Dfsdm((3, 1024, 1, 8, 0), 0)
    st = f2.new_state(nr)
    got, _ = f2.run(x[:, :16], state=st)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (nr, 0)
    for r in range(nr):
        assert np.array_equal(st[r].cpu().numpy(), dfsdm.filter_row(d["w"][r, :16], (3, 1024, 1, 8, 0))[1]), r
    f2.close()
    h2 = C.c_void_p()
    c = dfsdm._c(cfg)
    assert L.uc_dfsdm_create(torch.cuda.device_count(), C.byref(c), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_dfsdm_create(0, C.byref(c), None) == -errno.EINVAL and L.uc_dfsdm_create(0, None, C.byref(h2)) == -errno.EINVAL
    for bad in ((5, 74, 1, 0, 0), (3, 1024, 2, 0, 0), (6, 32, 1, 0, 0), (3, 0, 1, 0, 0), (3, 32, 257, 0, 0), (3, 32, 1, 32, 0), (3, 32, 1, 0, 2 ** 23)):
        cb = dfsdm._c(bad)
        assert L.uc_dfsdm_create(0, C.byref(cb), C.byref(h2)) == -errno.EINVAL and not h2.value, bad
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        f.run(x.float())
    with pytest.raises(ValueError):
        f.run(x, state=torch.zeros((nr + 1, 16), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        f.run(x, out=torch.zeros((nr, n_out + 1), dtype=torch.int32, device="cuda:0"))
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    f.close()
    assert torch.cuda.current_device() == dev0


def test_c_host_filters_rows_in_two_calls(dfsdm, tmp_path):
    import re
    import subprocess
    from test_dfsdm_filter_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    found = re.findall(r"order (\d+) ratio (\d+): (\d+) words in two calls, (\d+) equal uc_dfsdm_filter_row's, states equal", out.stdout)
    assert [(int(a), int(b)) for a, b, _, _ in found] == [(3, 32), (0, 20)] and all(int(c) == int(e) > 0 for _, _, c, e in found), found


def test_code_object_shows_no_spill_and_no_scratch(dfsdm, tmp_path, monkeypatch):
    from test_dfsdm_filter_cpu import code_objects
    code_objects(dfsdm, tmp_path, monkeypatch)


# ---- 6. two streams and destroy

def _hold(torch, stream):
    from test_gpu_streams import _Hold
    return _Hold(stream)


@pytest.mark.parametrize("cfg", [(3, 32, 1, 2, 0), (3, 20, 1, 0, 0)], ids=str)
def test_two_streams_and_close_with_a_call_pending(dfsdm, torch, cfg):
    """Two calls of one object on two non-blocking streams, the first pending behind a held stream A, the second on B (neither
    call blocks the host: the hold is still pending behind both); then close() while the call on A is pending: destroy frees
    the word path's tables, which that call reads, so it waits for the device.  Every output equals the call alone.
    (Stream B is not synchronised while A is held: with few hardware queues the two streams may share one, and B would then
    wait for the hold, which says nothing about the library.)"""
    rng = np.random.default_rng(35)
    nr, n = 130, 256
    w = [torch.from_numpy(rng.integers(0, 1 << 32, size=(nr, n), dtype=np.uint64).astype(np.uint32).view(np.int32)).to("cuda:0") for _ in range(2)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    alone = dfsdm.Dfsdm(cfg, 0)
    want = [alone.run(x) for x in w]
    torch.cuda.synchronize()
    alone.close()
    f = dfsdm.Dfsdm(cfg, 0)
    hold = _hold(torch, a)
    with torch.cuda.stream(a):
        out_a = f.run(w[0])
    with torch.cuda.stream(b):
        out_b = f.run(w[1])
    hold.must_be_pending("after the call on B")
    f.close()                                               # blocks until the hold and the call on A have ended: the design
    assert hold.t1.query(), "close() returned while the call on stream A was pending"
    a.synchronize()
    b.synchronize()
    hold.finish("dfsdm %r" % (cfg,))
    assert torch.equal(out_a[0], want[0][0]) and torch.equal(out_a[1], want[0][1])
    assert torch.equal(out_b[0], want[1][0]) and torch.equal(out_b[1], want[1][1])


# ---- 7. large calls

def test_many_rows(dfsdm, torch):
    """65 601 rows x 17 words whose content has the period 131: a row index cut to 16 bits, or a row served by the wrong lap of
    a grid, meets other content.  Word path and bit path; the last row against uc_dfsdm_filter_row."""
    R, P = lu.ROWS, lu.PERIOD
    idx = torch.from_numpy(lu.residues()).to("cuda:0")
    rng = np.random.default_rng(37)
    w = rng.integers(0, 1 << 32, size=(P, 17), dtype=np.uint64).astype(np.uint32)
    st = du.random_state(rng, P)
    wd, sd = torch.from_numpy(w.view(np.int32)).to("cuda:0"), torch.from_numpy(st).to("cuda:0")
    for cfg in ((3, 32, 1, 2, 0), (3, 20, 1, 0, 0)):
        f = dfsdm.Dfsdm(cfg, 0)
        n_out = dfsdm.plan(cfg, 3, 17)
        # rows 20 words apart lie on 16 bytes (one tile and a word through the direct way); rows of 17 do not.  Both; the
        # second call's words are the ones looked at, the first one's must equal them
        padded = torch.zeros((R, 20), dtype=torch.int32, device="cuda:0")
        padded[:, :17] = wd[idx]
        assert padded.data_ptr() % 16 == 0
        tiled, tiled_st = f.run(padded[:, :17], state=sd[idx].clone(), words_before=3)
        x, state = wd[idx], sd[idx].clone()
        big, out = _guarded(R, n_out, 4, torch)
        f.run(x, state=state, words_before=3, out=out)
        torch.cuda.synchronize()
        assert torch.equal(tiled, out) and torch.equal(tiled_st, state), cfg
        first, first_st = out[:P].contiguous(), state[:P].contiguous()
        assert torch.equal(out, first[idx]) and torch.equal(state, first_st[idx]), cfg
        for r in (0, 1, P - 1):
            o, s = dfsdm.filter_row(w[r], cfg, state=st[r], words_before=3)
            assert np.array_equal(first[r].cpu().numpy(), o) and np.array_equal(first_st[r].cpu().numpy(), s), (cfg, r)
        last = (R - 1) % P
        o, s = dfsdm.filter_row(w[last], cfg, state=st[last], words_before=3)
        assert np.array_equal(out[R - 1].cpu().numpy(), o) and np.array_equal(state[R - 1].cpu().numpy(), s), cfg
        out.fill_(GUARD)
        assert bool((big == GUARD).all()), cfg
        print("%r: %d rows of 17 words -> %d outputs; classes identical, rows 0, 1, 130 and %d equal the definition" % (cfg, R, n_out, R - 1))
        f.close()


def test_far_rows(dfsdm, torch):
    """One call whose row offsets pass 2^32 bytes: three rows 2^31 + 24 words apart (rows on 16 bytes: tiles) and 2^31 + 25
    (direct), as the input and as the output, in an arena whose every other byte must stay as it was."""
    need = lu.arena_bytes(4) + 4 * 2 ** 30
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("far rows: %.1f GiB free, the arena and 4 GiB are %.1f GiB" % (free / 2 ** 30, need / 2 ** 30))
    arena = lu.Arena(torch, 4)
    rng = np.random.default_rng(39)
    n = 17
    w = rng.integers(0, 1 << 32, size=(3, n), dtype=np.uint64).astype(np.uint32)
    st = du.random_state(rng, 3)
    wd, sd = torch.from_numpy(w.view(np.int32)).to("cuda:0"), torch.from_numpy(st).to("cuda:0")
    for cfg in ((3, 32, 1, 2, 0), (3, 20, 1, 0, 0)):
        f = dfsdm.Dfsdm(cfg, 0)
        n_out = dfsdm.plan(cfg, 3, n)
        want = np.stack([dfsdm.filter_row(w[r], cfg, state=st[r], words_before=3)[0] for r in range(3)])
        want_st = np.stack([dfsdm.filter_row(w[r], cfg, state=st[r], words_before=3)[1] for r in range(3)])
        for stride in (lu.STRIDE, lu.STRIDE + 1):
            # far input
            arena.fill()
            far = arena.matrix(torch.int32, n, stride)
            for r in range(3):
                far[r].copy_(wd[r])
            state = sd.clone()
            big, out = _guarded(3, n_out, 4, torch)
            f.run(far, state=state, words_before=3, out=out)
            torch.cuda.synchronize()
            assert np.array_equal(big.cpu().numpy(), _expect(big, out, want)) and np.array_equal(state.cpu().numpy(), want_st), (cfg, stride, "in")
            arena.erase(far)
            assert arena.dirty() == 0, (cfg, stride, "in")
            # far output
            far = arena.matrix(torch.int32, n_out, stride)
            state = sd.clone()
            f.run(wd, state=state, words_before=3, out=far)
            torch.cuda.synchronize()
            assert all(np.array_equal(far[r].cpu().numpy(), want[r]) for r in range(3)) and np.array_equal(state.cpu().numpy(), want_st), (cfg, stride, "out")
            arena.erase(far)
            bad = arena.dirty()
            print("%r, stride 2^31 + %d: far input and far output equal the definition, %d arena bytes touched besides" % (cfg, stride - 2 ** 31, bad))
            assert bad == 0, (cfg, stride, "out")
        f.close()
    arena.free()
