"""The down-converter on the GPU (uc_ddc_run, uchirp/ddc.py): every output float and every final state against the definition
in numpy float32 (`emulate32`), bit for bit -- row counts around the wave, sample counts around the state's 128 words and the
span, every tap count and decimation of tests/ddc_util.py, floats and words, I/Q and I alone, aligned and misaligned
matrices, denormals, -0, NaN and Inf, guard words -- a unit pulse swept across the seams of the kernel's spans, grids and
cuts, banks through row_map, set_index, steps and phases, the contract of the calls, the C host and the code object.  Nothing
here has a tolerance: the GPU's bits are the definition's.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import ddc_util as du

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
GUARD = -7654321.0


@pytest.fixture(scope="module")
def ddc():
    from uchirp import ddc as m
    m.lib()
    return m


def _sample_counts(decim):
    return sorted({1, 127, 128, 129, 2048, 2049} | ({decim - 1} if decim > 1 else set()))


@pytest.fixture(scope="module")
def ref(ddc):
    """The 130 x 2049 inputs of tests/ddc_util.py per format, the starting states, the carriers, per case the definition's
    outputs of the whole rows (a shorter call's outputs are their first ones: the same `first` and state) and per format the
    definition's states behind every sample count; made once and never written."""
    import torch
    f, w = du.inputs()
    st0 = du.states()
    steps, phases = du.carriers()
    out = {"state0": st0, "state0_dev": torch.from_numpy(st0).to("cuda:0"), "steps": steps, "phases": phases,
           "dev": {"f32": torch.from_numpy(f).to("cuda:0"), "i32": torch.from_numpy(w).to("cuda:0")}, "host": {"f32": f, "i32": w}, "states": {}}
    counts = sorted({n for d in du.DECIMS for n in _sample_counts(d)})
    for fmt, x in (("f32", f), ("i32", w)):
        for n in counts:
            st = ddc.emulate32([1.0], x[:, :n], 1, du.FIRST, state=st0, out="i")[1]
            out["states"][(fmt, n)] = torch.from_numpy(st).to("cuda:0")
    for case in du.CASES:
        n_taps, decim, fmt, o = case
        want, _ = ddc.emulate32(du.taps_of(n_taps), out["host"][fmt], decim, du.FIRST, steps, phases, st0, o)
        assert np.isfinite(want.view(np.float32)).all()
        out[case] = torch.from_numpy(np.ascontiguousarray(want).view(np.float32)).to("cuda:0")       # [130, count x (2 | 1)]
    return out


def _layouts(x, nr, n, torch):
    """The first n samples of the first nr rows of x three times: rows on 16 bytes, rows one word off, and rows without a gap."""
    stride = (n + 3) // 4 * 4 + 8
    for name, off, st in (("on 16 bytes", 4, stride), ("one word off", 1, stride + 1), ("no gap", 0, n)):
        big = torch.full((nr * st + 8,), 0x7FC00000 if x.dtype == torch.int32 else float("nan"), dtype=x.dtype, device=x.device)
        view = big[off:off + nr * st].view(nr, st)[:, :n]
        view.copy_(x[:nr, :n])
        assert view.data_ptr() % 16 == (4 * off) % 16
        yield name, view


def _guarded(nr, words, off, torch, device="cuda:0"):
    """an output matrix of nr rows of `words` floats inside a buffer of guard words: behind every row and around the matrix"""
    st = (words + 3) // 4 * 4 + 4 + (1 if off % 4 else 0)
    big = torch.full((nr * st + 16,), GUARD, dtype=torch.float32, device=device)
    return big, big[off:off + nr * st].view(nr, st)[:, :words]


def _guarded_state(state0, torch):
    nr = state0.shape[0]
    big = torch.full((nr * 128 + 32,), GUARD, dtype=torch.float32, device=state0.device)
    view = big[16:16 + nr * 128].view(nr, 128)
    view.copy_(state0)
    return big, view


def _ibits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(t, want):
    """bit for bit; `want` a device tensor or a numpy array"""
    import torch
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(np.ascontiguousarray(want).view(np.float32) if want.dtype == np.complex64 else np.ascontiguousarray(want)).to(t.device)
    if t.is_complex():
        t = torch.view_as_real(t).reshape(t.shape[0], -1)
    return t.shape == want.shape and torch.equal(_ibits(t), _ibits(want))


@pytest.mark.parametrize("nr", ROWS)
def test_outputs_and_states_equal_the_definition_bit_for_bit(ddc, ref, nr):
    import torch
    calls = empty = 0
    for case in du.CASES:
        n_taps, decim, fmt, o = case
        per = 2 if o == "iq" else 1
        m = ddc.Ddc(du.taps_of(n_taps), decim)
        for n in _sample_counts(decim):
            count = ddc.outputs(du.FIRST, n, decim)[1]
            words = count * per
            empty += count == 0
            for (name, x), off in zip(_layouts(ref["dev"][fmt], nr, n, torch), (4, 1, 0)):
                sbig, state = _guarded_state(ref["state0_dev"][:nr], torch)
                big, out = _guarded(nr, words, off, torch)
                got, st = m.run(x, du.FIRST, ref["steps"][:nr], ref["phases"][:nr], state=state, out=o, y=out)
                assert st.data_ptr() == state.data_ptr()
                assert _same(out, ref[case][:nr, :words]), (case, n, name)
                assert _same(state, ref["states"][(fmt, n)][:nr]), (case, n, name)
                out.fill_(GUARD)
                state.fill_(GUARD)
                assert float(big.min()) == GUARD == float(big.max()) and float(sbig.min()) == GUARD == float(sbig.max()), (case, n, name)
                calls += 1
        # filters at rest, buffers of the binding's own, the complex view
        x = ref["dev"][fmt][:nr, :300].contiguous()
        got, st = m.run(x, 5, ref["steps"][:nr], ref["phases"][:nr], out=o)
        want, want_st = ddc.emulate32(du.taps_of(n_taps), ref["host"][fmt][:nr, :300], decim, 5, ref["steps"][:nr], ref["phases"][:nr], None, o)
        assert got.dtype == (torch.complex64 if o == "iq" else torch.float32) and _same(got, want) and _same(st, want_st), case
        m.close()
    print("%d rows: %d calls (%d cases x their sample counts x 3 layouts), %d of them without an output; every float, state and guard word as defined"
          % (nr, calls, len(du.CASES), empty))
    assert empty >= 3


def test_minus_zero_and_denormals_come_out(ddc, ref):
    """-0 where the definition says -0, +0 from the padded set; the 1e-39 impulse comes out as denormals (the bit-for-bit test
    holds them; here they are shown to be there)."""
    import torch
    one, padded, x = du.minus_zero_case()
    xd = torch.from_numpy(x[None, :]).to("cuda:0")
    a, _ = ddc.Ddc(one).run(xd, out="i")
    b, _ = ddc.Ddc(padded).run(xd, out="i")
    a, b = du.bits(a.cpu().numpy()[0]), du.bits(b.cpu().numpy()[0])
    assert (a[1::2] == 0x80000000).all() and (a[0::2] == 0).all() and (b == 0).all()
    h = du.taps_of(27)
    got, _ = ddc.Ddc(h).run(ref["dev"]["f32"][:1].contiguous(), out="i")
    g = got.cpu().numpy()[0]
    tiny = np.finfo(np.float32).tiny
    assert int(((np.abs(g) < tiny) & (g != 0)).sum()) >= 25 and np.array_equal(du.bits(g), du.bits(ddc.emulate32(h, ref["host"]["f32"][0], out="i")[0]))


@pytest.mark.parametrize("decim", (1, 3, 8))
@pytest.mark.parametrize("n_taps", (27, 128))
def test_a_unit_pulse_swept_across_the_seams_of_two_spans(ddc, n_taps, decim):
    """Row q holds the one sample 1.0 at position q, for every q from 0 to two of the kernel's spans plus n_taps (the span's
    length from the library), every row with a carrier of its own: every output of every row equals the definition, so the
    impulse response lands on the right outputs across span and workgroup boundaries.  The definition's answer to such a row
    is restated in tests/ddc_util.py (`pulse_answer`) and held against emulate32 on the rows next to the seams."""
    import torch
    s = ddc.span(decim)
    rows = 2 * s * decim + n_taps
    n = rows + n_taps
    rng = np.random.default_rng(50 + n_taps + decim)
    steps, phases = rng.integers(0, 2 ** 32, size=rows, dtype=np.uint64), rng.integers(0, 2 ** 32, size=rows, dtype=np.uint64)
    h = du.taps_of(n_taps)
    want = du.pulse_answer(h, decim, rows, n, steps, phases)
    seam = s * decim
    near = sorted({0, 1, n_taps - 1, seam - n_taps, seam - 1, seam, seam + 1, 2 * seam - 1, 2 * seam, 2 * seam + 1, rows - 1} | set(rng.integers(0, rows, size=8).tolist()))
    xs = np.zeros((len(near), n), np.float32)
    xs[np.arange(len(near)), near] = 1.0
    chk, _ = ddc.emulate32(h, xs, decim, 0, steps[near], phases[near])
    assert np.array_equal(du.bits(chk), du.bits(want[near]))
    x = torch.zeros((rows, n), dtype=torch.float32, device="cuda:0")
    idx = torch.arange(rows, device="cuda:0")
    x[idx, idx] = 1.0
    m = ddc.Ddc(h, decim)
    got, _ = m.run(x, 0, steps, phases)
    g = torch.view_as_real(got).cpu().numpy().reshape(rows, -1)
    bad = np.nonzero((du.bits(g) != du.bits(want)).any(axis=1))[0]
    print("%d taps, D = %d: span %d outputs; %d rows x %d outputs, %d non-zero; rows that differ: %s" % (n_taps, decim, s, rows, want.shape[1], int((want != 0).sum()), bad[:8]))
    assert want.shape[1] > 2 * s and bad.size == 0
    m.close()


@pytest.mark.parametrize("case", ((27, 3, "f32", "iq"), (128, 1, "i32", "iq"), (65, 8, "f32", "i")), ids=lambda c: "%d-%d-%s-%s" % c)
def test_grids_and_cuts_give_the_same_bits(ddc, ref, uc_tuning, monkeypatch, case):
    """Calls of 77, 1, 222 and the rest, the state carried on the device and nothing synchronised in between, and 1, 2 and 3
    workgroups walking the units (UC_DDC_GRID): the bits of one call on the default grid.  `first` is 1001 samples in front of
    2^32, so the phase's index wraps inside the second cut."""
    import torch
    n_taps, decim, fmt, o = case
    per = 2 if o == "iq" else 1
    x = ref["dev"][fmt]
    n = du.SAMPLES
    h = du.taps_of(n_taps)
    st, ph = ref["steps"], ref["phases"]
    m = ddc.Ddc(h, decim)
    state = ref["state0_dev"].clone()
    total = ddc.outputs(du.FIRST, n, decim)[1]
    whole = torch.full((du.ROWS, total * per), GUARD, dtype=torch.float32, device="cuda:0")
    m.run(x, du.FIRST, st, ph, state=state, out=o, y=whole)
    want, want_st = ddc.emulate32(h, ref["host"][fmt], decim, du.FIRST, st, ph, ref["state0"], o)
    assert _same(whole, want) and _same(state, want_st)
    st2 = ref["state0_dev"].clone()
    parts = torch.full_like(whole, GUARD)
    a = at = 0
    for k in (77, 1, 222, n - 300):
        c = ddc.outputs(du.FIRST + a, k, decim)[1]
        m.run(x[:, a:a + k], du.FIRST + a, st, ph, state=st2, out=o, y=parts[:, at:at + c * per])
        a, at = a + k, at + c * per
    assert a == n and at == total * per and torch.equal(_ibits(parts), _ibits(whole)) and torch.equal(_ibits(st2), _ibits(state))
    for grid in (1, 2, 3):
        monkeypatch.setenv("UC_DDC_GRID", str(grid))
        m2 = ddc.Ddc(h, decim)
        st3 = ref["state0_dev"].clone()
        got = torch.full_like(whole, GUARD)
        m2.run(x, du.FIRST, st, ph, state=st3, out=o, y=got)
        assert torch.equal(_ibits(got), _ibits(whole)) and torch.equal(_ibits(st3), _ibits(state)), grid
        m2.close()
    monkeypatch.delenv("UC_DDC_GRID")
    m.close()


def test_banks(ddc, ref):
    """One input row against 5 output rows with five steps and phases and two tap sets equals five single calls, and so do
    three input rows behind a permuted row_map; 130 rows without a row_map equal the same rows with the identity; an
    UC_DDC_OUT_I call with step 0 equals the I half of the UC_DDC_OUT_IQ call bit for bit."""
    import torch
    sets = np.stack([du.taps_of(27), du.taps_of(27)[::-1] * np.float32(0.5)])
    decim, n = 3, 700
    m = ddc.Ddc(sets, decim)
    assert (m.n_sets, m.n_taps, m.decim) == (2, 27, 3)
    x = ref["dev"]["f32"][:, :n]
    steps = [ddc.step_of(f, 78125.0) for f in (16000.0, 17500.0, 19000.0, -17500.0, 0.0)]
    phases = [0, 1 << 30, 12345, 0xFFFFFFFF, 7]
    set_index = [0, 1, 0, 1, 1]
    for n_in, row_map in ((1, [0, 0, 0, 0, 0]), (3, [2, 0, 1, 0, 2])):
        state = ref["state0_dev"][4:4 + n_in].clone()
        got, _ = m.run(x[4:4 + n_in], du.FIRST, steps, phases, row_map, set_index, state=state)
        for r in range(5):
            src = 4 + row_map[r]
            s1 = ref["state0_dev"][src:src + 1].clone()
            one, _ = m.run(x[src:src + 1], du.FIRST, [steps[r]], [phases[r]], None, [set_index[r]], state=s1)
            want, want_st = ddc.emulate32(sets[set_index[r]], ref["host"]["f32"][src, :n], decim, du.FIRST, [steps[r]], [phases[r]], ref["state0"][src])
            assert torch.equal(_ibits(torch.view_as_real(got[r:r + 1])), _ibits(torch.view_as_real(one))) and _same(one, want[None, :]), (n_in, r)
            assert torch.equal(_ibits(state[row_map[r]]), _ibits(s1[0])) and _same(s1, want_st[None, :]), (n_in, r)
    sa, sb = ref["state0_dev"].clone(), ref["state0_dev"].clone()
    a, _ = m.run(x, du.FIRST, ref["steps"], ref["phases"], state=sa)
    b, _ = m.run(x, du.FIRST, ref["steps"], ref["phases"], row_map=np.arange(du.ROWS), state=sb)
    assert torch.equal(_ibits(torch.view_as_real(a)), _ibits(torch.view_as_real(b))) and torch.equal(_ibits(sa), _ibits(sb))
    iq, _ = m.run(x, du.FIRST)
    i, _ = m.run(x, du.FIRST, out="i")
    assert i.dtype == torch.float32 and torch.equal(_ibits(torch.view_as_real(iq)[..., 0]), _ibits(i))
    want, _ = ddc.emulate32(sets[0], ref["host"]["f32"][:, :n], decim, du.FIRST, out="i")
    assert _same(i, want)
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


def test_contract(ddc, ref, other_device):
    import torch
    L = ddc.lib()
    n_taps, decim, fmt, o = case = (27, 8, "f32", "i")
    h = du.taps_of(n_taps)
    nr, n = 5, 300
    dev0 = other_device
    m = ddc.Ddc(h, decim)
    assert torch.cuda.current_device() == dev0
    x = ref["dev"][fmt][:nr, :n].contiguous()
    count = ddc.outputs(du.FIRST, n, decim)[1]
    steps_h, phases_h = ref["steps"][:nr].astype(np.uint32), ref["phases"][:nr].astype(np.uint32)
    want, want_st = ddc.emulate32(h, ref["host"][fmt][:nr, :n], decim, du.FIRST, steps_h, phases_h, ref["state0"][:nr], o)
    out = torch.full((nr, count), GUARD, dtype=torch.float32, device="cuda:0")
    state0 = ref["state0_dev"][:nr]
    state = state0.clone()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    u32 = C.POINTER(C.c_uint32)
    steps, phases = steps_h.ctypes.data_as(u32), phases_h.ctypes.data_as(u32)
    ident = (C.c_uint32 * nr)(*range(nr))
    zeros = (C.c_uint32 * nr)()

    def call(h_=None, in_ptr=x.data_ptr(), dtype=ddc.DTYPE_F32, n_in=nr, in_stride=0, n_rows=nr, n_samples=n, first=du.FIRST, row_map=None,
             set_index=None, state_ptr=state.data_ptr(), out_ptr=out.data_ptr(), fmt_=ddc.OUT_I, out_stride=0):
        rc = L.uc_ddc_run(m._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_in, in_stride, n_rows, n_samples, first,
                          C.cast(row_map, u32) if row_map is not None else None, C.cast(set_index, u32) if set_index is not None else None,
                          steps, phases, C.c_void_p(state_ptr), C.c_void_p(out_ptr), fmt_, out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(nr * n, np.float32)
    bad_map = (C.c_uint32 * nr)(0, 1, 2, 3, nr)
    bad_set = (C.c_uint32 * nr)(0, 0, 0, 0, 1)
    refusals = [("in NULL", dict(in_ptr=None)), ("state NULL", dict(state_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no input rows", dict(n_in=0)), ("no samples", dict(n_samples=0)), ("too many rows", dict(n_rows=2 ** 32)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)), ("format 2", dict(fmt_=2)), ("format -1", dict(fmt_=-1)),
                ("in_stride < n_samples", dict(in_stride=n - 1)), ("out_stride < the row's floats", dict(out_stride=count - 1)),
                ("out_stride < the row's pairs", dict(fmt_=ddc.OUT_IQ, out_stride=2 * count - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("out_stride > 2^40", dict(out_stride=2 ** 40 + 1)),
                ("first + n_samples > 2^63", dict(first=2 ** 63 - n + 1)), ("first > 2^63", dict(first=2 ** 64 - 1)),
                ("in not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("out not on 4 bytes", dict(out_ptr=out.data_ptr() + 1)),
                ("state not on 4 bytes", dict(state_ptr=state.data_ptr() + 2)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("state: host memory", dict(state_ptr=host.ctypes.data)),
                ("row_map out of range", dict(row_map=bad_map)), ("set_index out of range", dict(set_index=bad_set)),
                ("more rows than input rows without a row_map", dict(n_in=nr - 1)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * n)), ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (nr * n - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (nr * count - 1))),
                ("state overlaps in", dict(state_ptr=x.data_ptr() + 4 * (nr * n - 1))), ("state overlaps out", dict(state_ptr=out.data_ptr() + 16)),
                ("out overlaps the end of state", dict(out_ptr=state.data_ptr() + 4 * (128 * nr - 1))),
                ("in overlaps state", dict(in_ptr=state.data_ptr()))]
    two = torch.cuda.device_count() >= 2
    if two:
        far = torch.zeros((nr, 400), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far.data_ptr())), ("out: memory of another device", dict(out_ptr=far.data_ptr())),
                     ("state: memory of another device", dict(state_ptr=far.data_ptr()))]
    for k, (name, kw) in enumerate(refusals):
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_ddc_last_error(), name
        torch.cuda.synchronize()
        assert float(out.min()) == GUARD == float(out.max()) and torch.equal(_ibits(state), _ibits(state0)), name   # nothing was enqueued
        good = dict(row_map=ident, set_index=zeros) if k % 2 else {}
        assert call(**good) == 0, name                                                              # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same(out, want) and _same(state, want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    print("contract: %d refused calls, a valid call behind each gives the definition's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    # set_taps is all or nothing: a refused upload leaves the sets and the decimation as they were
    other = du.taps_of(63)
    poisoned = other.copy()
    poisoned[62] = np.nan
    fp = C.POINTER(C.c_float)
    for name, args in (("NaN in the last tap", (poisoned.ctypes.data_as(fp), 1, 63, 2)), ("no sets", (other.ctypes.data_as(fp), 0, 63, 2)),
                       ("257 sets", (other.ctypes.data_as(fp), 257, 63, 2)), ("129 taps", (other.ctypes.data_as(fp), 1, 129, 2)),
                       ("0 taps", (other.ctypes.data_as(fp), 1, 0, 2)), ("decim 0", (other.ctypes.data_as(fp), 1, 63, 0)),
                       ("decim 65", (other.ctypes.data_as(fp), 1, 63, 65)), ("NULL", (None, 1, 63, 2))):
        assert L.uc_ddc_set_taps(m._h, *args) == -errno.EINVAL and L.uc_ddc_last_error(), name
        assert call() == 0
        torch.cuda.synchronize()
        assert _same(out, want) and _same(state, want_st), name
        out.fill_(GUARD)
        state.copy_(state0)
    # an object without taps refuses to run; with taps it runs
    h2 = C.c_void_p()
    assert L.uc_ddc_create(0, C.byref(h2)) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == -errno.EINVAL and b"no taps" in L.uc_ddc_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == GUARD == float(out.max())
    assert L.uc_ddc_set_taps(h2, h.ctypes.data_as(fp), 1, n_taps, decim) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == 0
    torch.cuda.synchronize()
    assert _same(out, want)
    L.uc_ddc_destroy(h2)
    h2 = C.c_void_p()
    assert L.uc_ddc_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_ddc_create(0, None) == -errno.EINVAL
    if not two:
        print("contract: one GPU visible: the object on a second device did not run")
    else:
        m1 = ddc.Ddc(h, decim, device=1)
        got, st = m1.run(x.to("cuda:1"), du.FIRST, steps_h, phases_h, state=state0.to("cuda:1"), out=o)
        torch.cuda.synchronize(1)
        assert _same(got, want) and _same(st, want_st) and torch.cuda.current_device() == dev0
        m1.close()
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        m.run(x.double())
    with pytest.raises(ValueError):
        m.run(x, state=torch.zeros((nr + 1, 128), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, y=torch.zeros((nr, 3), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, row_map=[0, 1], set_index=[0, 0, 0])
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    m.close()
    assert torch.cuda.current_device() == dev0


def test_memory_of_another_device_is_refused(ddc):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    m = ddc.Ddc(du.taps_of(27))
    x = torch.zeros((2, 64), dtype=torch.float32, device="cuda:1")
    with pytest.raises(ValueError):
        m.run(x)
    st = torch.zeros((2, 128), dtype=torch.float32, device="cuda:0")
    y = torch.zeros((2, 128), dtype=torch.float32, device="cuda:0")
    rc = ddc.lib().uc_ddc_run(m._h, C.c_void_p(x.data_ptr()), ddc.DTYPE_F32, 2, 64, 2, 64, 0, None, None, None, None, C.c_void_p(st.data_ptr()),
                              C.c_void_p(y.data_ptr()), ddc.OUT_IQ, 128, None)
    assert rc == -errno.EINVAL and b"not device memory of device 0" in ddc.lib().uc_ddc_last_error()
    m.close()


def test_four_unsynchronised_calls_on_one_stream(ddc, ref):
    """The staging protocol: four calls with four different sets of row arrays, enqueued back to back on one stream with
    nothing synchronised in between (two staging pairs: the third call waits for the first one's copy), give the four right
    results."""
    import torch
    h = du.taps_of(63)
    m = ddc.Ddc(h, 2)
    n = 500
    rng = np.random.default_rng(60)
    s = torch.cuda.Stream(device="cuda:0")
    x = ref["dev"]["i32"][:, :n]
    jobs = []
    with torch.cuda.stream(s):
        for k in range(4):
            row_map = rng.integers(0, du.ROWS, size=97)
            steps, phases = rng.integers(0, 2 ** 32, size=97, dtype=np.uint64), rng.integers(0, 2 ** 32, size=97, dtype=np.uint64)
            got, st = m.run(x, 1000 * k + 1, steps, phases, row_map, state=ref["state0_dev"].clone())
            jobs.append((row_map, steps, phases, got, st, 1000 * k + 1))
    s.synchronize()
    for row_map, steps, phases, got, st, first in jobs:
        want, _ = ddc.emulate32(h, ref["host"]["i32"][row_map, :n], 2, first, steps, phases, ref["state0"][row_map])
        _, want_st = ddc.emulate32(h, ref["host"]["i32"][:, :n], 2, first, state=ref["state0"], out="i")
        assert _same(got, want) and _same(st, want_st), first
    m.close()


def test_c_host_converts_rows_in_two_calls(ddc, tmp_path):
    import re
    import subprocess
    from test_ddc_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, equal = [int(v) for v in re.search(r"(\d+) floats in two calls, (\d+) equal", out.stdout).groups()]
    assert n == equal > 0 and "states equal" in out.stdout


def test_code_object_shows_no_spill_no_scratch_and_the_stated_budget(ddc, tmp_path, monkeypatch):
    from test_ddc_cpu import code_objects
    code_objects(ddc, tmp_path, monkeypatch)
