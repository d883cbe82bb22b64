"""The recursive filter bank on the GPU (uc_iir_run, uchirp/iir.py): every output float and every final state against the
definition in numpy float32 (`emulate32`), bit for bit -- row counts around the wave, sample counts around the 16-byte group
and the tile of 16, cascades of 1, 2, 7 and 8 sections, floats and words, aligned and misaligned matrices, denormals, -0.0,
NaN and Inf, guard words, cuts and grids, a filter bank through row_map and set_index -- the notebook's I/Q rows (fixture K3),
the contract of the calls, the C host, the code object, and the chain into the receiver.  Nothing here has a tolerance of its
own: the GPU's bits are the definition's.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import iir_util as iu

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
SAMPLES = (1, 2, 3, 15, 16, 17, 33, 67, 300)                   # (15 .. 33: around the tile of 16 samples that goes through LDS)
FORMATS = ("f32", "i32")
GUARD = -7654321.0


@pytest.fixture(scope="module")
def iir():
    from uchirp import iir as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ref(iir):
    """The 130 x 300 inputs of tests/iir_util.py per format, the starting states, and per cascade the definition's outputs and
    its states behind each of SAMPLES; made once and never written.  The float inputs discriminate: a flushing emulation of
    the 7-section cascade differs on the 1e-34 impulse in all 300 outputs."""
    import torch
    f, w = iu.inputs()
    st0 = iu.states()
    cascades = iu.cascades()
    out = {"state0": st0, "state0_dev": torch.from_numpy(st0).to("cuda:0"), "cascades": cascades,
           "dev": {"f32": torch.from_numpy(f).to("cuda:0"), "i32": torch.from_numpy(w).to("cuda:0")}, "host": {"f32": f, "i32": w}}
    for count, c in cascades.items():
        for fmt, x in (("f32", f), ("i32", w)):
            states = {n: iir.emulate32(c, x[:, :n], st0)[1] for n in SAMPLES[:-1]}
            want, states[SAMPLES[-1]] = iir.emulate32(c, x, st0)
            assert np.isfinite(want).all() and np.abs(iir.samples32(x)).max() <= 2.0 ** 24
            out[(count, fmt)] = {"out": want, "states": states}
    imp = f[iu.IMPULSE_ROW]
    assert (iu.bits(iir.emulate32(cascades[7], imp)[0]) != iu.bits(iir.emulate32(cascades[7], imp, flush=True)[0])).all()
    assert iu.bits(out[(7, "f32")]["out"][iu.MINUS_ZERO_ROW, :1])[0] == 0x80000000      # -0.0 comes out: an identity section behind would show
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
    """an output matrix of nr rows of n floats inside a buffer of guard words: behind every row and behind the last one"""
    st = (n + 3) // 4 * 4 + 4 + (1 if off % 4 else 0)
    big = torch.full((nr * st + 16,), GUARD, dtype=torch.float32, device=device)
    return big, big[off:off + nr * st].view(nr, st)[:, :n]


def _same(t, want):
    return np.array_equal(iu.bits(t.cpu().numpy()), iu.bits(want))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("count", iu.SECTION_COUNTS)
@pytest.mark.parametrize("nr", ROWS)
def test_outputs_and_states_equal_the_definition_bit_for_bit(iir, ref, nr, count, fmt):
    import torch
    r = ref[(count, fmt)]
    m = iir.Iir(ref["cascades"][count])
    calls = 0
    for n in SAMPLES:
        for (name, x), off in zip(_layouts(ref["dev"][fmt], nr, n, torch), (4, 1, 0)):
            state = ref["state0_dev"][:nr].clone()
            big, out = _guarded(nr, n, off, torch)
            got, st = m.run(x, state=state, out=out)
            assert got.data_ptr() == out.data_ptr() and st.data_ptr() == state.data_ptr()
            torch.cuda.synchronize()
            assert _same(out, r["out"][:nr, :n]), (n, name)
            assert _same(state, r["states"][n][:nr]), (n, name)
            calls += 1
    # filters at rest: no state given
    got, st = m.run(ref["dev"][fmt][:nr, :67].contiguous())
    want, want_st = iir.emulate32(ref["cascades"][count], ref["host"][fmt][:nr, :67])
    assert got.dtype == torch.float32 and _same(got, want) and _same(st, want_st)
    print("%d rows, %d sections, %s: %d calls (%d sample counts x 3 layouts), every float and state equal" % (nr, count, fmt, calls, len(SAMPLES)))
    m.close()


@pytest.mark.parametrize("nr", ROWS)
def test_ragged_tails_change_no_guard_word(iir, ref, nr):
    """Rows whose last group of four is short, next to guard words: behind every row and behind the last row nothing changes,
    with 16-byte stores (rows on 16 bytes) and with dword stores (one word off)."""
    import torch
    for count, fmt in ((7, "f32"), (2, "i32")):
        r = ref[(count, fmt)]
        m = iir.Iir(ref["cascades"][count])
        for n in SAMPLES:
            x = ref["dev"][fmt][:nr, :n]
            for off in (4, 5, 7):
                big, out = _guarded(nr, n, off, torch)
                m.run(x, state=ref["state0_dev"][:nr].clone(), out=out)
                torch.cuda.synchronize()
                assert _same(out, r["out"][:nr, :n]), (fmt, n, off)
                out.fill_(GUARD)
                assert float(big.min()) == GUARD == float(big.max()), (fmt, n, off)
        m.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("count", (1, 7, 8))
def test_cuts_and_grids_give_the_same_bits(iir, ref, uc_tuning, monkeypatch, count, fmt):
    import torch
    r = ref[(count, fmt)]
    n = 300
    x = ref["dev"][fmt]
    m = iir.Iir(ref["cascades"][count])
    state = ref["state0_dev"].clone()
    whole, _ = m.run(x, state=state)
    assert _same(whole, r["out"]) and _same(state, r["states"][n])
    # calls of 77, 1 and 222 samples, the state carried on the device; not synchronised in between
    st2 = ref["state0_dev"].clone()
    parts = torch.zeros_like(whole)
    a = 0
    for k in (77, 1, 222):
        m.run(x[:, a:a + k], state=st2, out=parts[:, a:a + k])
        a += k
    assert a == n and torch.equal(parts.view(torch.int32), whole.view(torch.int32)) and torch.equal(st2.view(torch.int32), state.view(torch.int32))
    # launch geometry: 1, 3 and 2 workgroups walk the 3 row blocks (UC_IIR_GRID, read under UC_TUNING=1 when the object is created)
    for grid in (1, 3, 2):
        monkeypatch.setenv("UC_IIR_GRID", str(grid))
        m2 = iir.Iir(ref["cascades"][count])
        st3 = ref["state0_dev"].clone()
        got, _ = m2.run(x, state=st3)
        assert torch.equal(got.view(torch.int32), whole.view(torch.int32)) and torch.equal(st3.view(torch.int32), state.view(torch.int32)), grid
        m2.close()
    monkeypatch.delenv("UC_IIR_GRID")
    m.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_filter_bank_of_three_rows_and_four_sets(iir, ref, fmt):
    """3 input rows feed 130 output rows through a shuffled row_map and 4 sets of 2 sections: every output row equals one
    emulate32 of its input row through its set.  Then a row_map that is the identity on the first wave and shuffled behind
    it (tiles and the direct path in one call), and set_index alone."""
    import torch
    rng = np.random.default_rng(23)
    sets = np.stack([iir.bandpass_sections(78125.0, lo, hi, 2) for lo, hi in ((16000.0, 17500.0), (17500.0, 19000.0), (16000.0, 19000.0), (2000.0, 3000.0))])
    m = iir.Iir(sets)
    assert (m.n_sets, m.n_sections) == (4, 2)
    n = 67
    host, x = ref["host"][fmt], ref["dev"][fmt]
    st0 = ref["state0"]
    for n_in, row_map in ((3, rng.integers(0, 3, size=130)), (130, np.concatenate([np.arange(64), rng.permutation(66)])), (130, None)):
        set_index = rng.integers(0, 4, size=130)
        xin = x[:n_in, :n]                                          # (rows 300 floats apart: on 16 bytes)
        state = ref["state0_dev"].clone()
        got, _ = m.run(xin, state=state, row_map=row_map, set_index=set_index)
        torch.cuda.synchronize()
        g, s = got.cpu().numpy(), state.cpu().numpy()
        src = np.arange(130) if row_map is None else row_map
        for k in range(4):
            rows = np.nonzero(set_index == k)[0]
            want, want_st = iir.emulate32(sets[k], host[src[rows], :n], st0[rows])
            assert np.array_equal(iu.bits(g[rows]), iu.bits(want)) and np.array_equal(iu.bits(s[rows]), iu.bits(want_st)), (n_in, k)
    m.close()


def test_k3_rows_equal_the_definition_hence_the_reference(iir):
    """The notebook's four mixed rows through the 7-section low-pass on the GPU: emulate32's bits, hence within 2e-5 of the
    peak of k3_R / k3_Rd, the reference's own lpf() output (tests/test_iir_cpu.py holds emulate32 to that bound)."""
    import torch
    rows, ref_out, fs, cutoff = iu.k3_rows()
    c = iir.lpf_sections(fs, cutoff)
    x = rows.astype(np.float32)
    m = iir.Iir(c)
    got, st = m.run(torch.from_numpy(x).to("cuda:0"))
    want, want_st = iir.emulate32(c, x)
    g = got.cpu().numpy()
    err = np.abs(g.astype(np.float64) - ref_out).max() / np.abs(ref_out).max()
    print("K3 through the GPU: %.3g of the peak from the reference's lpf()" % err)
    assert _same(got, want) and _same(st, want_st) and err <= 2e-5
    m.close()


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


def test_contract(iir, ref, other_device):
    import torch
    L = iir.lib()
    count, fmt = 2, "f32"
    r = ref[(count, fmt)]
    c32 = np.ascontiguousarray(ref["cascades"][count], np.float32)
    nr, n = 5, 67
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    m = iir.Iir(c32)
    assert torch.cuda.current_device() == dev0
    x = ref["dev"][fmt][:nr, :n].contiguous()
    want, want_st = r["out"][:nr, :n], r["states"][n][:nr]
    out = torch.full((nr, n), GUARD, dtype=torch.float32, device="cuda:0")
    state0 = ref["state0_dev"][:nr]
    state = state0.clone()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    u32 = C.POINTER(C.c_uint32)
    ident = (C.c_uint32 * nr)(*range(nr))
    zeros = (C.c_uint32 * nr)()

    def call(h_=None, in_ptr=x.data_ptr(), dtype=iir.DTYPE_F32, n_in=nr, in_stride=0, n_rows=nr, n_samples=n, row_map=None, set_index=None,
             state_ptr=state.data_ptr(), out_ptr=out.data_ptr(), out_stride=0):
        rc = L.uc_iir_run(m._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_in, in_stride, n_rows, n_samples,
                          C.cast(row_map, u32) if row_map is not None else None, C.cast(set_index, u32) if set_index is not None else None,
                          C.c_void_p(state_ptr), C.c_void_p(out_ptr), out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(nr * n, np.float32)
    bad_map = (C.c_uint32 * nr)(0, 1, 2, 3, nr)
    bad_set = (C.c_uint32 * nr)(0, 0, 0, 0, 1)
    refusals = [("in NULL", dict(in_ptr=None)), ("state NULL", dict(state_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no input rows", dict(n_in=0)), ("no samples", dict(n_samples=0)), ("too many rows", dict(n_rows=2 ** 32)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("in_stride < n_samples", dict(in_stride=n - 1)), ("out_stride < n_samples", dict(out_stride=n - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("out_stride > 2^40", dict(out_stride=2 ** 40 + 1)),
                ("in not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("out not on 4 bytes", dict(out_ptr=out.data_ptr() + 1)),
                ("state not on 4 bytes", dict(state_ptr=state.data_ptr() + 2)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("state: host memory", dict(state_ptr=host.ctypes.data)),
                ("row_map out of range", dict(row_map=bad_map)), ("set_index out of range", dict(set_index=bad_set)),
                ("more rows than input rows without a row_map", dict(n_in=nr - 1)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * n)), ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (nr * n - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (nr * n - 1))),
                ("state overlaps in", dict(state_ptr=x.data_ptr() + 4 * (nr * n - 1))), ("state overlaps out", dict(state_ptr=out.data_ptr() + 16)),
                ("out overlaps the end of state", dict(out_ptr=state.data_ptr() + 4 * (16 * nr - 1))),
                ("in overlaps state", dict(in_ptr=state.data_ptr()))]
    if two:
        far = torch.zeros((nr, 80), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far.data_ptr())), ("out: memory of another device", dict(out_ptr=far.data_ptr())),
                     ("state: memory of another device", dict(state_ptr=far.data_ptr()))]
    for k, (name, kw) in enumerate(refusals):
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_iir_last_error(), name
        torch.cuda.synchronize()
        assert float(out.min()) == GUARD == float(out.max()) and torch.equal(state.view(torch.int32), state0.view(torch.int32)), name   # nothing was enqueued
        good = dict(row_map=ident, set_index=zeros) if k % 2 else {}                                # (staged and unstaged calls in turn)
        assert call(**good) == 0, name                                                              # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same(out, want) and _same(state, want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    print("contract: %d refused calls, a valid call behind each gives the definition's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    # set_sections is all or nothing: a refused upload leaves the sets as they were
    other = np.ascontiguousarray(ref["cascades"][7], np.float32)
    poisoned = other.copy()
    poisoned[6, 4] = np.nan
    fp = C.POINTER(C.c_float)
    for name, args in (("NaN in the last section", (poisoned.ctypes.data_as(fp), 1, 7)), ("no sets", (other.ctypes.data_as(fp), 0, 7)),
                       ("257 sets", (other.ctypes.data_as(fp), 257, 7)), ("9 sections", (other.ctypes.data_as(fp), 1, 9)),
                       ("0 sections", (other.ctypes.data_as(fp), 1, 0)), ("NULL", (None, 1, 7))):
        assert L.uc_iir_set_sections(m._h, *args) == -errno.EINVAL and L.uc_iir_last_error(), name
        assert call() == 0
        torch.cuda.synchronize()
        assert _same(out, want) and _same(state, want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    # an object without sets refuses to run; with sets it runs
    h2 = C.c_void_p()
    assert L.uc_iir_create(0, C.byref(h2)) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == -errno.EINVAL and b"no coefficient sets" in L.uc_iir_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == GUARD == float(out.max())
    assert L.uc_iir_set_sections(h2, c32.ctypes.data_as(fp), 1, count) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == 0
    torch.cuda.synchronize()
    assert _same(out, want)
    L.uc_iir_destroy(h2)
    h2 = C.c_void_p()
    assert L.uc_iir_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_iir_create(0, None) == -errno.EINVAL
    if two:
        # an object on the other device: its own memory runs, device 0's is refused
        m1 = iir.Iir(c32, device=1)
        got, st = m1.run(x.to("cuda:1"), state=state0.to("cuda:1"))
        torch.cuda.synchronize(1)
        assert _same(got, want) and _same(st, want_st) and torch.cuda.current_device() == dev0
        assert L.uc_iir_run(m1._h, C.c_void_p(x.data_ptr()), iir.DTYPE_F32, nr, 0, nr, n, None, None, C.c_void_p(st.data_ptr()),
                            C.c_void_p(got.data_ptr()), 0, None) == -errno.EINVAL
        m1.close()
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        m.run(x.double())
    with pytest.raises(ValueError):
        m.run(x, state=torch.zeros((nr + 1, 16), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, out=torch.zeros((nr, n + 1), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, row_map=[0, 1], set_index=[0, 0, 0])
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    m.close()
    assert torch.cuda.current_device() == dev0


def test_c_host_filters_rows_in_two_calls(iir, tmp_path):
    import re
    import subprocess
    from test_iir_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, equal = [int(v) for v in re.search(r"(\d+) samples in two calls, (\d+) equal", out.stdout).groups()]
    assert n == 5 * 301 == equal and "states equal" in out.stdout


def test_code_object_shows_no_spill_and_no_scratch(iir, tmp_path, monkeypatch):
    from test_iir_cpu import code_objects
    code_objects(iir, tmp_path, monkeypatch)


def test_receiver_behind_the_band_pass_equals_the_oracle_chain(iir):
    """A uc_link_transmit render -> bandpass_sections(78125, 16000, 19000, 4) on the GPU -> uc_process_batch RX_REAL: the
    symbols the oracle gives on the same rows filtered by emulate32.  (The filtered rows are equal bit for bit, which is
    asserted first.)"""
    import torch
    import uchirp
    from oracle import uco
    from uchirp import link
    n = 6 * 2048
    ln = link.Link(0)
    x = ln.transmit(["Hi", "iir", "0123"], lead_samples=[0.0, 0.0, 0.0], amplitude=[2000.0, 1000.0, 4000.0], sigma=[200.0, 300.0, 2000.0],
                    n_samples=n, seed=9)
    c = iir.bandpass_sections(78125.0, 16000.0, 19000.0, 4)
    m = iir.Iir(c)
    y, _ = m.run(x)
    want, _ = iir.emulate32(c, x.cpu().numpy())
    assert _same(y, want)
    e = uchirp.Engine(uchirp.RX_REAL, device=0, mag_mean=1000.0)
    sym, _ = e.process(y.view(-1, 2048))
    torch.cuda.synchronize()
    sym = sym.cpu().numpy()
    o = uco.Oracle(uco.RX_REAL, mag_mean=1000.0)
    ref_sym, _ = o.process(np.ascontiguousarray(want.reshape(-1, 2048)))
    print("symbols behind the band-pass:", sym.tolist())
    assert sym.shape == (18,) and np.array_equal(sym, ref_sym)
    e.close()
    m.close()
    ln.close()
