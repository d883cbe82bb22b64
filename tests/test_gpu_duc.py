"""The up-converter on the GPU (uc_duc_run, uchirp/duc.py): every output value, every final state and every clip count against
the definition in numpy float32 (`emulate32`), bit for bit -- 1 to 67 output rows, sample counts around the state's 128
samples and the span, every (K, L) of tests/duc_util.py, I/Q and I alone, floats and int16, 1, 3 and 16 channels, tight,
padded and misaligned matrices, denormals, -0, NaN and Inf, guard words round every buffer -- a unit pulse swept across the
seams of the kernel's spans, grids and cuts across 2^32, banks through row_map, set_index, steps and phases, int16 at odd and
even alignments, the loop through the down-converter, the contract of the calls, and the C host.  Nothing here has a
tolerance: the GPU's bits are the definition's.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import duc_util as du

pytestmark = pytest.mark.gpu

GUARD = -7654321.0
GUARD16 = -12345
CLIP0 = 5


@pytest.fixture(scope="module")
def duc():
    from uchirp import duc as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ref(duc):
    """Per case of tests/duc_util.py: the 70 input rows of the longest call, the starting states, two tap sets, the channel
    tables of 67 output rows, the definition's float sums of the whole rows (a shorter call's outputs are their first ones: the
    same `first` and state; the int16 values and the clip counts follow from them by `to_int16`) and the definition's states
    behind every sample count; made once and never written."""
    import torch
    out = {}
    for case in du.CASES:
        K, L, fmt, n_chan, o = case
        n = du.max_samples(L)
        x, st0 = du.inputs(fmt, n), du.states(fmt)
        sets = np.stack([du.taps_of(K, L), du.taps_of(K, L, 1)])
        ch = du.channels(max(du.ROWS), n_chan, 2)
        y, _, _ = duc.emulate32(sets, x, L, du.first_of(L), n_chan, *ch[:1], set_index=ch[1], steps=ch[2], phases=ch[3], state=st0, in_format=fmt)
        assert y.shape == (max(du.ROWS), n * L)
        y16, _ = duc.to_int16(y)
        out[case] = {"x": torch.from_numpy(x).to("cuda:0"), "x_host": x, "st0": st0, "st0_dev": torch.from_numpy(st0).to("cuda:0"), "sets": sets, "ch": ch,
                     "y": torch.from_numpy(y).to("cuda:0"), "y16": torch.from_numpy(y16).to("cuda:0"), "y_host": y,
                     "states": {c: torch.from_numpy(du.new_state(x, st0, c, fmt)).to("cuda:0") for c in du.sample_counts(L)}}
    return out


def _layouts(x, n_words, torch):
    """The first n_words floats of the rows of x three times: rows on 16 bytes, rows one float off, and rows without a gap."""
    nr = x.shape[0]
    stride = (n_words + 3) // 4 * 4 + 8
    for name, off, st in (("on 16 bytes", 4, stride), ("one float off", 1, stride + 1), ("no gap", 0, n_words)):
        big = torch.full((nr * st + 8,), float("nan"), dtype=torch.float32, device=x.device)
        view = big[off:off + nr * st].view(nr, st)[:, :n_words]
        view.copy_(x[:, :n_words])
        yield name, view


def _guarded(nr, words, off, torch, dtype=None, device="cuda:0"):
    """an output matrix of nr rows of `words` elements inside a buffer of guard words: behind every row and around the matrix;
    off: the matrix's first element, so off = 1 puts int16 rows on odd 2-byte addresses and floats one word off 16 bytes"""
    dtype = dtype or torch.float32
    st = (words + 3) // 4 * 4 + 4 + (1 if off % 4 else 0)
    big = torch.full((nr * st + 16,), GUARD if dtype == torch.float32 else GUARD16, dtype=dtype, device=device)
    return big, big[off:off + nr * st].view(nr, st)[:, :words]


def _guarded_rows(t0, torch, fill=GUARD):
    nr, w = t0.shape
    big = torch.full((nr * w + 32,), fill, dtype=t0.dtype, device=t0.device)
    view = big[16:16 + nr * w].view(nr, w)
    view.copy_(t0)
    return big, view


def _ibits(t):
    import torch
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(t, want):
    """bit for bit; `want` a device tensor or a numpy array"""
    import torch
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(np.ascontiguousarray(want)).to(t.device)
    return t.shape == want.shape and t.dtype == want.dtype and torch.equal(_ibits(t), _ibits(want))


def _only_guards(big, view, fill, torch):
    view.fill_(fill)
    return float(big.min()) == fill == float(big.max())


@pytest.mark.parametrize("nr", du.ROWS)
def test_outputs_states_and_clip_counts_equal_the_definition_bit_for_bit(duc, ref, nr):
    import torch
    calls = clipped_calls = 0
    for case in du.CASES:
        K, L, fmt, n_chan, o = case
        w = 2 if fmt == "iq" else 1
        c = ref[case]
        m = duc.Duc(c["sets"], L)
        ch = [a[:nr * n_chan] for a in c["ch"]]
        dt = torch.float32 if o == "f32" else torch.int16
        for n in du.sample_counts(L):
            count = n * L
            want = (c["y"] if o == "f32" else c["y16"])[:nr, :count]
            want_clip = duc.to_int16(c["y_host"][:nr, :count])[1].astype(np.int32) if o == "i16" else np.zeros(nr, np.int32)
            for (name, x), off in zip(_layouts(c["x"], n * w, torch), (4, 1, 0)):
                sbig, state = _guarded_rows(c["st0_dev"], torch)
                big, out = _guarded(nr, count, off, torch, dt)
                cbig, clip = _guarded_rows(torch.full((1, nr), CLIP0, dtype=torch.int32, device="cuda:0"), torch, GUARD16)
                got, st = m.run(x, du.first_of(L), n_chan, ch[2], ch[3], ch[0], ch[1], state=state, in_format=fmt, out=o, y=out, clip=clip[0])
                assert st.data_ptr() == state.data_ptr() and got.data_ptr() == out.data_ptr()
                assert _same(out, want), (case, n, name)
                assert _same(state, c["states"][n]), (case, n, name)
                assert _same(clip[0], want_clip + CLIP0), (case, n, name, clip, want_clip)
                assert _only_guards(big, out, GUARD if o == "f32" else GUARD16, torch) and _only_guards(sbig, state, GUARD, torch) \
                    and _only_guards(cbig, clip, GUARD16, torch), (case, n, name)
                calls += 1
                clipped_calls += int(want_clip.sum() > 0)
        m.close()
    print("%d rows: %d calls (%d cases x their sample counts x 3 layouts), %d of them with clipped values; every value, state, count and guard word as defined"
          % (nr, calls, len(du.CASES), clipped_calls))
    assert clipped_calls >= 3 or nr < 5                                            # (the first rows read the impulse, the NaN and the still row)


def test_filters_at_rest_and_the_binding_s_own_buffers(duc, ref):
    """No state, no output tensor, no channel arrays: input row r n_chan + j is channel j of row r, set 0, carrier (1, 0); a
    complex tensor is its pairs."""
    import torch
    for case in du.CASES:
        K, L, fmt, n_chan, o = case
        c = ref[case]
        w = 2 if fmt == "iq" else 1
        n = min(300, du.max_samples(L))
        rows = (du.IN_ROWS // n_chan) * n_chan
        x = c["x"][:rows, :n * w].contiguous()
        got, st = duc.Duc(c["sets"], L).run(x, 5, n_chan, in_format=fmt, out=o)
        want, want_st, _ = duc.emulate32(c["sets"], c["x_host"][:rows, :n * w], L, 5, n_chan, in_format=fmt, out=o)
        assert _same(got, want) and _same(st, want_st), case
        if fmt == "iq":
            z = torch.view_as_complex(x.view(rows, n, 2))
            again, _ = duc.Duc(c["sets"], L).run(z, 5, n_chan, out=o)
            assert _same(again, want), case


def test_minus_zero_and_denormals_come_out(duc, ref):
    """-0 where the definition says -0, +0 from the padded set; the 1e-39 impulse comes out as denormals (the bit-for-bit test
    holds them; here they are shown to be there)."""
    import torch
    one, padded, x = du.minus_zero_case()
    xd = torch.from_numpy(x[None, :]).to("cuda:0")
    a, _ = duc.Duc(one).run(xd, in_format="i")
    b, _ = duc.Duc(padded).run(xd, in_format="i")
    a, b = du.bits(a.cpu().numpy()[0]), du.bits(b.cpu().numpy()[0])
    assert (a[1::2] == 0x80000000).all() and (a[0::2] == 0).all() and (b == 0).all()
    case = du.CASES[2]                                                            # (128, 1, I alone, one channel, floats)
    c = ref[case]
    h = c["sets"][0]
    got, _ = duc.Duc(h).run(c["x"][:1, :300].contiguous(), in_format="i")
    g = got.cpu().numpy()[0]
    tiny = np.finfo(np.float32).tiny
    assert int(((np.abs(g) < tiny) & (g != 0)).sum()) >= 100
    assert np.array_equal(du.bits(g), du.bits(duc.emulate32(h, c["x_host"][:1, :300], 1, in_format="i")[0][0]))


def test_nan_and_inf_inputs_read_as_zero(duc, ref):
    """The row with NaN and +-Inf gives what the same row with +0 in their places gives, outputs and state."""
    import torch
    case = du.CASES[3]                                                            # (27, 8, I/Q)
    c = ref[case]
    n = 200
    x = c["x_host"][du.NAN_ROW:du.NAN_ROW + 1, :2 * n]
    clean = np.where(np.isfinite(x), x, np.float32(0.0))
    assert not np.isfinite(x).all()
    m = duc.Duc(c["sets"][0], 8)
    a, sa = m.run(torch.from_numpy(x).to("cuda:0"), 3, steps=[12345678])
    b, sb = m.run(torch.from_numpy(clean).to("cuda:0"), 3, steps=[12345678])
    assert _same(a, b) and _same(sa, sb) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(sa).all())
    assert _same(a, duc.emulate32(c["sets"][0], x, 8, 3, steps=[12345678])[0])


@pytest.mark.parametrize("K,L", ((27, 1), (27, 8), (5, 3)))
def test_a_unit_pulse_swept_across_the_seams_of_two_spans(duc, K, L):
    """Input row q holds the one pair (1, 0.5) at position q, for every q from 0 to two of the kernel's spans plus K (the
    span's length from the library), every row with a carrier of its own: every output of every row equals the definition, so
    the impulse response lands on the right outputs across span and workgroup boundaries.  The definition's answer to such a
    row is restated in tests/duc_util.py (`pulse_answer`) and held against emulate32 on the rows next to the seams."""
    import torch
    s = duc.span(L) // L
    assert duc.span(L) == (2048 // L) * L and s == du.span_in(L)
    rows = 2 * s + K
    n = rows + K
    rng = np.random.default_rng(50 + K + L)
    steps, phases = rng.integers(0, 2 ** 32, size=rows, dtype=np.uint64), rng.integers(0, 2 ** 32, size=rows, dtype=np.uint64)
    h = du.taps_of(K, L)
    want = du.pulse_answer(h, L, rows, n, steps, phases)
    near = sorted({0, 1, K - 1, s - K, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, rows - 1} | set(rng.integers(0, rows, size=6).tolist()))
    xs = np.zeros((len(near), n), np.complex64)
    xs[np.arange(len(near)), near] = 1.0 + 0.5j
    chk, _, _ = duc.emulate32(h, xs, L, 0, steps=steps[near], phases=phases[near])
    assert np.array_equal(du.bits(chk), du.bits(want[near]))
    x = torch.zeros((rows, 2 * n), dtype=torch.float32, device="cuda:0")
    idx = torch.arange(rows, device="cuda:0")
    x[idx, 2 * idx] = 1.0
    x[idx, 2 * idx + 1] = 0.5
    m = duc.Duc(h, L)
    got, _ = m.run(x, 0, steps=steps, phases=phases)
    wd = torch.from_numpy(want).to("cuda:0")
    bad = torch.nonzero((_ibits(got) != _ibits(wd)).any(dim=1)).flatten().cpu().numpy()
    print("K = %d, L = %d: span %d outputs; %d rows x %d outputs, %d non-zero; rows that differ: %s" % (K, L, duc.span(L), rows, want.shape[1], int((want != 0).sum()), bad[:8]))
    assert want.shape[1] > 2 * duc.span(L) and bad.size == 0
    m.close()


@pytest.mark.parametrize("case", (du.CASES[1], du.CASES[3], du.CASES[4]), ids=lambda c: "%d-%d-%s-%d-%s" % c)
def test_grids_and_cuts_give_the_same_bits(duc, ref, uc_tuning, monkeypatch, case):
    """Calls of 77, 1, 222 and the rest (for short rows: 5, 1, 40 and the rest), the state carried on the device and nothing
    synchronised in between, and 1 to 5 workgroups walking the units (UC_DUC_GRID): the bits, states and clip counts of one
    call on the default grid.  The outputs' index passes 2^32 inside the first cut."""
    import torch
    K, L, fmt, n_chan, o = case
    w = 2 if fmt == "iq" else 1
    c = ref[case]
    n = du.max_samples(L)
    nr = max(du.ROWS)
    ch = c["ch"]
    first = du.first_of(L)
    dt = torch.float32 if o == "f32" else torch.int16
    m = duc.Duc(c["sets"], L)

    def run(obj, cuts):
        state = c["st0_dev"].clone()
        y = torch.full((nr, n * L), 77, dtype=dt, device="cuda:0")
        clip = torch.zeros(nr, dtype=torch.int32, device="cuda:0")
        a = 0
        for k in cuts:
            obj.run(c["x"][:, a * w:(a + k) * w], first + a, n_chan, ch[2], ch[3], ch[0], ch[1], state=state, in_format=fmt, out=o,
                    y=y[:, a * L:(a + k) * L], clip=clip)
            a += k
        assert a == n
        return y, state, clip

    whole, state, clip = run(m, (n,))
    assert _same(whole, c["y"] if o == "f32" else c["y16"]) and _same(state, c["states"][n])
    assert o == "f32" or _same(clip, duc.to_int16(c["y_host"])[1].astype(np.int32))
    cuts = (77, 1, 222, n - 300) if n > 400 else (5, 1, 40, n - 46)
    parts, st2, clip2 = run(m, cuts)
    assert _same(parts, whole) and _same(st2, state) and _same(clip2, clip)
    for grid in (1, 2, 3, 4, 5):
        monkeypatch.setenv("UC_DUC_GRID", str(grid))
        m2 = duc.Duc(c["sets"], L)
        got, st3, clip3 = run(m2, (n,))
        assert _same(got, whole) and _same(st3, state) and _same(clip3, clip), grid
        m2.close()
    monkeypatch.delenv("UC_DUC_GRID")
    m.close()


def test_banks(duc, ref):
    """One base-band row on 4 carriers summed into one output row equals the sum of four single calls in channel order;
    several output rows that share input rows through row_map, with two tap sets, equal single calls; a call without arrays
    equals the same call with the identity."""
    import torch
    case = du.CASES[3]                                                            # (27, 8, I/Q)
    c = ref[case]
    L, n = 8, 300
    sets = c["sets"]
    m = duc.Duc(sets, L)
    assert (m.n_sets, m.k_taps, m.interp) == (2, 27, 8)
    x = c["x"][:, :2 * n].contiguous()
    xh = c["x_host"][:, :2 * n]
    steps = [duc.step_of(f, 78125.0) for f in (12000.0, 15000.0, 18000.0, -21000.0)]
    phases = [0, 1 << 30, 12345, 0xFFFFFFFF]
    first = du.first_of(L)
    state = c["st0_dev"][4:5].clone()
    got, st = m.run(x[4:5], first, 4, steps, phases, [0, 0, 0, 0], [0, 1, 0, 1], state=state)
    singles = [m.run(x[4:5], first, 1, [steps[j]], [phases[j]], None, [j & 1], state=c["st0_dev"][4:5].clone())[0] for j in range(4)]
    acc = singles[0]
    for s in singles[1:]:
        acc = acc + s                                                             # (torch adds floats with one rounding)
    want, want_st, _ = duc.emulate32(sets, xh[4:5], L, first, 4, [0, 0, 0, 0], [0, 1, 0, 1], steps, phases, c["st0"][4:5])
    assert _same(got, acc) and _same(got, want) and _same(st, want_st)
    # 3 output rows of 2 channels over 3 input rows, shared
    row_map, set_index = [2, 0, 1, 0, 2, 2], [0, 1, 1, 0, 0, 1]
    st6, ph6 = steps + steps[:2], phases + phases[2:]
    state = c["st0_dev"][4:7].clone()
    got, st = m.run(x[4:7], first, 2, st6, ph6, row_map, set_index, state=state)
    want, want_st, _ = duc.emulate32(sets, xh[4:7], L, first, 2, row_map, set_index, st6, ph6, c["st0"][4:7])
    assert got.shape == (3, n * L) and _same(got, want) and _same(st, want_st)
    # no arrays against the identity
    a, sa = m.run(x, first, 2, state=c["st0_dev"].clone())
    b, sb = m.run(x, first, 2, row_map=np.arange(du.IN_ROWS), state=c["st0_dev"].clone())
    want, _, _ = duc.emulate32(sets, xh, L, first, 2, state=c["st0"])
    assert a.shape == (du.IN_ROWS // 2, n * L) and _same(a, b) and _same(sa, sb) and _same(a, want)
    m.close()


def test_int16_at_odd_and_even_alignments_with_clip_counts(duc, ref):
    """int16 rows at every 2-byte place of 8 bytes, even and odd strides, lengths 1 .. 9 and a long one: values and clip
    counts equal `to_int16` of the definition's floats, and no guard word moves."""
    import torch
    case = du.CASES[1]                                                            # (27, 1, I/Q, one channel, int16)
    c = ref[case]
    m = duc.Duc(c["sets"], 1)
    nr = 3
    ch = [a[:nr] for a in c["ch"]]
    x = c["x"]
    calls = 0
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 1031):
        want, want_clip = duc.to_int16(c["y_host"][:nr, :n])
        for off in range(8):
            for stride in (n + 8, n + 9):
                big = torch.full((nr * stride + 32,), GUARD16, dtype=torch.int16, device="cuda:0")
                out = big[8 + off:8 + off + nr * stride].view(nr, stride)[:, :n]
                assert out.data_ptr() % 8 == (2 * off) % 8
                clip = torch.zeros(nr, dtype=torch.int32, device="cuda:0")
                m.run(x[:, :2 * n], du.first_of(1), 1, ch[2], ch[3], ch[0], ch[1], state=c["st0_dev"].clone(), out="i16", y=out, clip=clip)
                assert _same(out, want) and _same(clip, want_clip.astype(np.int32)), (n, off, stride)
                assert _only_guards(big, out, GUARD16, torch), (n, off, stride)
                calls += 1
    print("int16: %d calls at 8 alignments x 2 strides x 10 lengths; %d values clipped in the long rows" % (calls, int(want_clip.sum())))
    assert want_clip.sum() > 0
    m.close()


def test_loop_back_through_the_down_converter(duc):
    """Duc.run (2 output rows, 4 carriers each, L = 8, 128 prototype taps) -> Ddc.run at each carrier (the prototype / 8 as
    low-pass, D = 8) equals ddc.emulate32(duc.emulate32(...)) bit for bit, in two cuts."""
    import torch
    from uchirp import ddc
    L, K, n = 8, 16, 700
    h = duc.interp_taps(L, K, cutoff=0.2).astype(np.float32)
    rng = np.random.default_rng(90)
    z = (rng.standard_normal((4, 2 * n)) * 1500.0).astype(np.float32)
    freqs = (12000.0, 15000.0, 18000.0, 21000.0)
    steps = [duc.step_of(f, 78125.0) for f in freqs] * 2
    row_map = [0, 1, 2, 3, 3, 2, 1, 0]
    first = 2 ** 32 // L - 300
    up = duc.Duc(h, L)
    down = ddc.Ddc(h / np.float32(L), L)
    zd = torch.from_numpy(z).to("cuda:0")
    ust, dst = up.new_state(4), down.new_state(2)
    got = []
    for a, b in ((0, 333), (333, n)):
        y, _ = up.run(zd[:, 2 * a:2 * b], first + a, 4, steps, None, row_map, state=ust)
        iq, _ = down.run(y, (first + a) * L, steps, None, [0, 0, 0, 0, 1, 1, 1, 1], state=dst)
        got.append(iq)
    got = torch.cat(got, dim=1)
    y_ref, _, _ = duc.emulate32(h, z, L, first, 4, row_map, None, steps)
    want, _ = ddc.emulate32(h / np.float32(L), y_ref[[0, 0, 0, 0, 1, 1, 1, 1]], L, first * L, steps)
    g = torch.view_as_real(got).cpu().numpy()
    assert g.shape[:2] == want.shape == (8, n) and np.array_equal(du.bits(g).reshape(8, -1), du.bits(want).reshape(8, -1))
    up.close()
    down.close()


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


def test_contract(duc, ref, other_device):
    import torch
    L_ = duc.lib()
    case = du.CASES[3]                                                            # (27, 8, I/Q, 3 channels, int16)
    K, L, fmt, n_chan, o = case
    c = ref[case]
    nr, n = 5, 100
    count = n * L
    dev0 = other_device
    m = duc.Duc(c["sets"], L)
    assert torch.cuda.current_device() == dev0
    n_in = du.IN_ROWS
    x = c["x"][:, :2 * n].contiguous()
    ch = [np.ascontiguousarray(a[:nr * n_chan]) for a in c["ch"]]
    first = du.first_of(L)
    want, want_st, want_clip = duc.emulate32(c["sets"], c["x_host"][:, :2 * n], L, first, n_chan, *ch, state=c["st0"], in_format=fmt, out=o)
    out = torch.full((nr, count), GUARD16, dtype=torch.int16, device="cuda:0")
    state0 = c["st0_dev"]
    state = state0.clone()
    clip = torch.zeros(nr, dtype=torch.int32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    u32 = C.POINTER(C.c_uint32)
    ptrs = [a.ctypes.data_as(u32) for a in ch]

    def call(h_=None, in_ptr=x.data_ptr(), in_fmt=duc.IN_IQ, n_in_=n_in, in_stride=0, n_rows=nr, n_chan_=n_chan, n_samples=n, first_=first, row_map=ptrs[0],
             set_index=ptrs[1], state_ptr=state.data_ptr(), out_ptr=out.data_ptr(), out_fmt=duc.OUT_I16, out_stride=0, clip_ptr=clip.data_ptr()):
        rc = L_.uc_duc_run(m._h if h_ is None else h_, C.c_void_p(in_ptr), in_fmt, n_in_, in_stride, n_rows, n_chan_, n_samples, first_,
                           C.cast(row_map, u32) if row_map is not None else None, C.cast(set_index, u32) if set_index is not None else None,
                           ptrs[2], ptrs[3], C.c_void_p(state_ptr), C.c_void_p(out_ptr), out_fmt, out_stride, C.c_void_p(clip_ptr), stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(n_in * 2 * n, np.float32)
    slots = nr * n_chan
    bad_map = (C.c_uint32 * slots)(*([0] * (slots - 1) + [n_in]))
    bad_set = (C.c_uint32 * slots)(*([0] * (slots - 1) + [2]))
    refusals = [("in NULL", dict(in_ptr=None)), ("state NULL", dict(state_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no input rows", dict(n_in_=0)), ("no samples", dict(n_samples=0)), ("too many rows", dict(n_rows=2 ** 32)),
                ("no channels", dict(n_chan_=0)), ("17 channels", dict(n_chan_=17)), ("-1 channels", dict(n_chan_=-1)),
                ("input format 2", dict(in_fmt=2)), ("input format -1", dict(in_fmt=-1)), ("output format 2", dict(out_fmt=2)), ("output format -1", dict(out_fmt=-1)),
                ("in_stride < the row's floats", dict(in_stride=2 * n - 1)), ("out_stride < the row's outputs", dict(out_stride=count - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("out_stride > 2^40", dict(out_stride=2 ** 40 + 1)),
                ("(first + n_samples) L > 2^63", dict(first_=2 ** 63 // L - n + 1)), ("first > 2^63", dict(first_=2 ** 64 - 1)),
                ("in not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("int16 out not on 2 bytes", dict(out_ptr=out.data_ptr() + 1)),
                ("float out not on 4 bytes", dict(out_fmt=duc.OUT_F32, out_ptr=x.data_ptr() + 2)),
                ("state not on 4 bytes", dict(state_ptr=state.data_ptr() + 2)), ("clip not on 4 bytes", dict(clip_ptr=clip.data_ptr() + 2)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("state: host memory", dict(state_ptr=host.ctypes.data)), ("clip: host memory", dict(clip_ptr=host.ctypes.data)),
                ("row_map out of range", dict(row_map=bad_map)), ("set_index out of range", dict(set_index=bad_set)),
                ("more channels than input rows without a row_map", dict(row_map=None, n_in_=slots - 1)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 8 * n)), ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (n_in * 2 * n - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 2 * (nr * count - 2))),
                ("state overlaps in", dict(state_ptr=x.data_ptr() + 4 * (n_in * 2 * n - 1))), ("state overlaps out", dict(state_ptr=out.data_ptr() + 16)),
                ("out overlaps the end of state", dict(out_ptr=state.data_ptr() + 4 * (256 * n_in - 1))),
                ("in overlaps state", dict(in_ptr=state.data_ptr())),
                ("clip overlaps in", dict(clip_ptr=x.data_ptr() + 16)), ("clip overlaps out", dict(clip_ptr=out.data_ptr() + 2 * (nr * count - 2))),
                ("clip overlaps state", dict(clip_ptr=state.data_ptr() + 4 * (256 * n_in - 1)))]
    two = torch.cuda.device_count() >= 2
    if two:
        far = torch.zeros((n_in, 2 * n * L), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far.data_ptr())), ("out: memory of another device", dict(out_ptr=far.data_ptr())),
                     ("state: memory of another device", dict(state_ptr=far.data_ptr())), ("clip: memory of another device", dict(clip_ptr=far.data_ptr()))]
    for k, (name, kw) in enumerate(refusals):
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L_.uc_duc_last_error(), name
        torch.cuda.synchronize()
        assert int(out.min()) == GUARD16 == int(out.max()) and _same(state, state0) and int(clip.abs().max()) == 0, name     # nothing was enqueued
        assert call() == 0, name                                                                   # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same(out, want[:nr]) and _same(state, want_st) and _same(clip, want_clip.astype(np.int32)), name
        out.fill_(GUARD16)
        state.copy_(state0)
        clip.zero_()
    print("contract: %d refused calls, a valid call behind each gives the definition's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    # set_taps is all or nothing: a refused upload leaves the sets, K and L as they were
    other = du.taps_of(5, 3)
    poisoned = other.copy()
    poisoned[14] = np.nan
    fp = C.POINTER(C.c_float)
    big = np.zeros(2112, np.float32)
    for name, args in (("NaN in the last tap", (poisoned.ctypes.data_as(fp), 1, 5, 3)), ("no sets", (other.ctypes.data_as(fp), 0, 5, 3)),
                       ("257 sets", (other.ctypes.data_as(fp), 257, 5, 3)), ("129 taps per phase", (big.ctypes.data_as(fp), 1, 129, 1)),
                       ("0 taps", (other.ctypes.data_as(fp), 1, 0, 3)), ("interp 0", (other.ctypes.data_as(fp), 1, 5, 0)),
                       ("interp 65", (other.ctypes.data_as(fp), 1, 5, 65)), ("2112 taps", (big.ctypes.data_as(fp), 1, 33, 64)), ("NULL", (None, 1, 5, 3))):
        assert L_.uc_duc_set_taps(m._h, *args) == -errno.EINVAL and L_.uc_duc_last_error(), name
        assert call() == 0
        torch.cuda.synchronize()
        assert _same(out, want[:nr]) and _same(state, want_st), name
        out.fill_(GUARD16)
        state.copy_(state0)
        clip.zero_()
    # an object without taps refuses to run; with taps it runs
    h2 = C.c_void_p()
    assert L_.uc_duc_create(0, C.byref(h2)) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == -errno.EINVAL and b"no taps" in L_.uc_duc_last_error()
    torch.cuda.synchronize()
    assert int(out.min()) == GUARD16 == int(out.max())
    assert L_.uc_duc_set_taps(h2, c["sets"].ctypes.data_as(fp), 2, K, L) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == 0
    torch.cuda.synchronize()
    assert _same(out, want[:nr])
    L_.uc_duc_destroy(h2)
    h2 = C.c_void_p()
    assert L_.uc_duc_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L_.uc_duc_create(0, None) == -errno.EINVAL
    if not two:
        print("contract: one GPU visible: the object on a second device did not run")
    else:
        m1 = duc.Duc(c["sets"], L, device=1)
        got, st = m1.run(x.to("cuda:1"), first, n_chan, ch[2], ch[3], ch[0], ch[1], state=state0.to("cuda:1"), out=o)
        torch.cuda.synchronize(1)
        assert _same(got, want[:nr]) and _same(st, want_st) and torch.cuda.current_device() == dev0
        m1.close()
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        m.run(x.double())
    with pytest.raises(ValueError):
        m.run(x, state=torch.zeros((n_in + 1, 256), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, y=torch.zeros((n_in, 3), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        m.run(x, n_chan=3, row_map=[0, 1])
    with pytest.raises(ValueError):
        m.run(x, n_chan=17)
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    m.close()
    assert torch.cuda.current_device() == dev0


def test_memory_of_another_device_is_refused(duc):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    m = duc.Duc(du.taps_of(27, 1))
    x = torch.zeros((2, 128), dtype=torch.float32, device="cuda:1")
    with pytest.raises(ValueError):
        m.run(x)
    st = torch.zeros((2, 256), dtype=torch.float32, device="cuda:0")
    y = torch.zeros((2, 64), dtype=torch.float32, device="cuda:0")
    rc = duc.lib().uc_duc_run(m._h, C.c_void_p(x.data_ptr()), duc.IN_IQ, 2, 128, 2, 1, 64, 0, None, None, None, None, C.c_void_p(st.data_ptr()),
                              C.c_void_p(y.data_ptr()), duc.OUT_F32, 64, None, None)
    assert rc == -errno.EINVAL and b"not device memory of device 0" in duc.lib().uc_duc_last_error()
    m.close()


def test_four_unsynchronised_calls_on_one_stream(duc, ref):
    """The staging protocol: four calls with four different channel tables, enqueued back to back on one stream with nothing
    synchronised in between (two staging pairs: the third call waits for the first one's copy), give the four right results."""
    import torch
    case = du.CASES[4]                                                            # (5, 3, I/Q, 3 channels)
    c = ref[case]
    m = duc.Duc(c["sets"], 3)
    n = 500
    s = torch.cuda.Stream(device="cuda:0")
    x = c["x"][:, :2 * n]
    jobs = []
    with torch.cuda.stream(s):
        for k in range(4):
            ch = du.channels(31, 3, 2, seed=10 + k)
            got, st = m.run(x, 1000 * k + 1, 3, ch[2], ch[3], ch[0], ch[1], state=c["st0_dev"].clone())
            jobs.append((ch, got, st, 1000 * k + 1))
    s.synchronize()
    for ch, got, st, first in jobs:
        want, want_st, _ = duc.emulate32(c["sets"], c["x_host"][:, :2 * n], 3, first, 3, *ch, state=c["st0"])
        assert _same(got, want) and _same(st, want_st), first
    m.close()


def test_c_host_converts_rows_in_two_calls(duc, tmp_path):
    import re
    import subprocess
    from test_duc_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, equal = [int(v) for v in re.search(r"(\d+) int16 values in two calls, (\d+) equal", out.stdout).groups()]
    assert n == equal > 0 and "states equal" in out.stdout and "clip counts equal" in out.stdout


def test_code_object_shows_no_spill_no_scratch_and_the_stated_budget(duc, tmp_path, monkeypatch):
    from test_duc_cpu import code_objects
    code_objects(duc, tmp_path, monkeypatch)
