"""Large calls of the sibling libraries ("Large calls"): many rows and far rows.

MANY ROWS.  One call of R = 65 601 rows per library; row r carries row r mod 131 of a 131-row master, as do its set_index,
row_map, line, pair, job, step and phase.  The definition is evaluated for the 131 rows, by the rule the library's own GPU
test uses; on the device every row is compared with row r mod 131 by a gather; outputs lie in a guarded buffer; every row's
final state is compared too.  What each shape takes round a second time:
  iir     1026 row blocks of 64 lanes, one workgroup each, the last one with one live lane; call 1 (set_index alone) goes
          through the LDS tiles, 20 samples: one tile and one direct group; call 2 (row_map and set_index: 525 KB staged,
          all that two arrays of R words are) takes the direct path with rows read across 2^16
  mic     1026 row blocks as above, 20 samples: one tile and one direct group
  ddc     65 601 input rows: the state kernel's grid is capped at 65 536, its r += gridDim.x loop goes round twice for 65
          rows; 65 601 units over the 4-per-CU grid of the convert kernel; four staged arrays of R words, 1.05 MB
  duc     the same cap in its state kernel; 65 601 units over the convert kernel's grid; R channel records of 16 bytes,
          1.05 MB staged; floats and int16 with clip counts
  spec    65 601 frames, a run of consecutive units per workgroup of the occupancy-derived grid
  rate    R rows x 2 tiles (256 outputs and one) over the occupancy-derived grid, floats and int16
  retime  R lines x 2 tiles (260 outputs); the lines read rows across 2^16; 1.5 MB of line records staged
  array   R beams x 2 tiles (260 outputs), 130 701 taps that hear rows past 2^16; 2.6 MB of tap and beam records staged
  xcorr   R pairs x 257 lags = 16.9 M sums: launch_sum's grid of 65 536 x 256 threads goes round twice; 1.05 MB of pair records
  wcorr   the same cap in its sum kernel, at L = 128 and a guard of 128
  align   R pairs, four to a workgroup, over the occupancy-derived grid
  track   R pairs x 16 windows = 1 049 616 rows: the crest kernel's grid is capped at 2^20
  mf      R jobs of one segment, 8 taps, in chunks of consecutive units; 1.05 MB of job records staged
  scan    R arrays of 3 microphones, 2 beam groups each: 131 202 units; R rows over the best kernel's 8-per-CU grid
  link    R streams x 3 tiles over the 8-per-CU grid, 2.8 MB staged; pure noise in rows 0 .. 130 and 65 405 .. 65 600 against
          the model; uc_link_noise_words with 600 001 counters, more than its grid of 8 x 256 threads per CU holds
  scene   R microphones x 3 tiles, 3.4 MB of path and microphone records staged; the same rows of pure noise

FAR ROWS.  One test per row matrix that has a stride argument: three rows 2^31 + 24 elements apart, and 2^31 + 25, in an
arena whose first row starts 2^31 + 8 elements in (tests/large_util.py; tests/test_large_cpu.py proves that a row offset
cut to 32 bits lands inside the arena).  Matrices of 8-byte elements (the double correlations and powers, mf's complex
outputs) have two rows.  The arena is one byte pattern; the expected result is the same call on compact matrices, bit for
bit, itself held to the definition; afterwards, the rows put back, every byte of the arena is the pattern.  Matrices
without a stride argument are not covered: the states of iir, mic, ddc and duc, the records of spec, track, mf and scan.

Nothing here has a tolerance of its own: bits, or the bound that the library's own GPU test states and derives.  Every
test prints its figures before it asserts (pytest -s)."""
import numpy as np
import pytest

import large_util as lu

pytestmark = pytest.mark.gpu

R, P = lu.ROWS, lu.PERIOD
GUARD = -7654321.0
IGUARD = -1234567
GIB = 2 ** 30


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def idx(torch):
    """r mod 131 on the device"""
    return torch.from_numpy(lu.residues()).to("cuda:0")


def _arena(torch, elem_size):
    need = lu.arena_bytes(elem_size) + 4 * GIB
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        reason = "far rows of %d-byte elements: %.1f GiB free, the arena and 4 GiB are %.1f GiB" % (elem_size, free / GIB, need / GIB)
        print(reason)
        pytest.skip(reason)
    return lu.Arena(torch, elem_size)


@pytest.fixture(scope="module")
def arena4(torch):
    a = _arena(torch, 4)
    yield a
    a.free()


@pytest.fixture(scope="module")
def arena2(torch):
    a = _arena(torch, 2)
    yield a
    a.free()


def _ints(t, torch):
    """the bits of a tensor of 4-byte (or 2-byte) elements"""
    return t if t.dtype in (torch.int32, torch.int16) else t.view(torch.int32)


def _guarded(nr, n, torch, dtype=None, device="cuda:0"):
    """an output matrix of nr rows of n elements inside a buffer of guard values: behind every row and around the matrix"""
    dtype = dtype or torch.float32
    st = (n + 7) // 8 * 8 + 8
    guard = {torch.float32: GUARD, torch.float64: GUARD, torch.int32: IGUARD, torch.int16: -12345}[dtype]
    big = torch.full((nr * st + 32,), guard, dtype=dtype, device=device)
    return big, big[8:8 + nr * st].view(nr, st)[:, :n]


def _untouched(big, out):
    """with the expected rows overwritten by the guard, the whole buffer is the guard"""
    g = big[0].clone()
    out.fill_(g)
    return bool((big == g).all())


def _rows_equal(name, got, want, idx, torch):
    """got [R, n] on the device, want [131, n] on the host (same element size): every row of a residue class equals the
    class's first (a gather on the device), and the first 131 equal the definition"""
    g = _ints(got, torch)
    w = np.ascontiguousarray(want)
    w = w.view({2: np.int16, 4: np.int32}[w.dtype.itemsize]).reshape(P, -1)
    first = g[:P].contiguous()
    same = bool(torch.equal(g, first[idx]))
    head = np.array_equal(first.cpu().numpy().reshape(P, -1), w)
    print("%s: %d rows of %d words; classes identical: %s; 131 rows equal the definition: %s" % (name, g.shape[0], w.shape[1], same, head))
    assert same and head, name


def _far(name, arena, torch, dtype, n, stride):
    """the arena, filled, and a far matrix in it"""
    arena.fill()
    m = arena.matrix(dtype, n, stride)
    assert m.stride(0) == stride and m.data_ptr() == arena.buf.data_ptr() + lu.MARGIN * arena.elem_size
    return m


def _far_in(arena, m, rows, torch):
    for r in range(m.shape[0]):
        m[r].copy_(rows[r])


def _far_equal(m, want, torch):
    return all(bool(torch.equal(_ints(m[r], torch), _ints(want[r], torch))) for r in range(m.shape[0]))


def _clean(name, arena, m, stride):
    arena.erase(m)
    bad = arena.dirty()
    print("%s, stride 2^31 + %d: %d of %d arena bytes are not the pattern" % (name, stride - 2 ** 31, bad, arena.bytes))
    assert bad == 0, (name, stride)


STRIDES = (lu.STRIDE, lu.STRIDE + 1)


# ------------------------------------------------------------------------------------------------------------------- iir

class _Iir:
    N = 20

    def __init__(self, torch):
        from uchirp import iir
        self.m = iir
        rng = np.random.default_rng(501)
        self.sets = np.stack([iir.bandpass_sections(78125.0, lo, hi, 2) for lo, hi in ((16000.0, 17500.0), (17500.0, 19000.0), (16000.0, 19000.0), (2000.0, 3000.0))])
        x = (rng.standard_normal((P, self.N)) * 20000.0).astype(np.float32)
        x[0] = 0.0
        x[0, 0] = 1e-34                                            # its response runs through the denormals
        x[1, 0] = -0.0
        x[2, [0, 5, 17]] = [np.nan, np.inf, -np.inf]
        st = (rng.standard_normal((P, 16)) * 1000.0).astype(np.float32)
        st[0] = 0.0
        st[3] = (rng.standard_normal(16) * 1e-40).astype(np.float32)
        self.x, self.st, self.set = x, st, rng.integers(0, 4, size=P)
        self.want = np.zeros((P, self.N), np.float32)
        self.want_st = np.zeros((P, 16), np.float32)
        for k in range(4):
            rows = np.nonzero(self.set == k)[0]
            self.want[rows], self.want_st[rows] = iir.emulate32(self.sets[k], x[rows], st[rows])
        assert np.isfinite(self.want).all()
        self.obj = iir.Iir(self.sets)
        self.x_dev, self.st_dev = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(st).to("cuda:0")


def test_many_rows_iir(torch, idx):
    c = _Iir(torch)
    res = lu.residues()
    x = c.x_dev[idx]
    for name, row_map in (("iir, set_index (tiles)", None), ("iir, row_map and set_index (direct)", lu.shuffled_map())):
        state = c.st_dev[idx].clone()
        big, out = _guarded(R, c.N, torch)
        c.obj.run(x, state=state, out=out, row_map=row_map, set_index=c.set[res])
        torch.cuda.synchronize()
        _rows_equal(name, out, c.want, idx, torch)
        _rows_equal(name + ", states", state, c.want_st, idx, torch)
        assert _untouched(big, out), name
    c.obj.close()


def _iir_compact(c, torch):
    x3, st3 = c.x_dev[3:6].contiguous(), c.st_dev[3:6].contiguous()            # (row 3: denormal state)
    state = st3.clone()
    out, _ = c.obj.run(x3, state=state, set_index=c.set[3:6])
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c.want[3:6].view(np.uint32))
    assert np.array_equal(state.cpu().numpy().view(np.uint32), c.want_st[3:6].view(np.uint32))
    return x3, st3, out, state


def test_far_rows_iir_in(torch, arena4):
    c = _Iir(torch)
    x3, st3, want, want_st = _iir_compact(c, torch)
    for stride in STRIDES:
        far = _far("iir in", arena4, torch, torch.float32, c.N, stride)
        _far_in(arena4, far, x3, torch)
        state = st3.clone()
        big, out = _guarded(3, c.N, torch)
        c.obj.run(far, state=state, out=out, set_index=c.set[3:6])
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        assert _untouched(big, out)
        _clean("iir in", arena4, far, stride)
    c.obj.close()


def test_far_rows_iir_out(torch, arena4):
    c = _Iir(torch)
    x3, st3, want, want_st = _iir_compact(c, torch)
    for stride in STRIDES:
        far = _far("iir out", arena4, torch, torch.float32, c.N, stride)
        state = st3.clone()
        c.obj.run(x3, state=state, out=far, set_index=c.set[3:6])
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        _clean("iir out", arena4, far, stride)
    c.obj.close()


# ------------------------------------------------------------------------------------------------------------------- mic

class _Mic:
    N = 20

    def __init__(self, torch):
        from uchirp import mic
        self.m = mic
        rng = np.random.default_rng(502)
        x = (rng.uniform(-1.0, 1.0, (P, self.N)) * mic.Q_MAX).astype(np.float32)
        x[0] = 0.0
        x[1] = float(mic.Q_MAX)
        x[2, [0, 5, 17]] = [np.nan, np.inf, -np.inf]
        # states that a microphone reaches: those behind 8 earlier samples
        _, st = mic.model(mic.quantise_model((rng.uniform(-1.0, 1.0, (P, 8)) * mic.Q_MAX).astype(np.float32)))
        st[0] = 0
        self.x, self.st = x, st
        self.want, self.want_st = mic.model(mic.quantise_model(x), st)
        assert (self.want[0] == mic.SILENCE).all() and len(set(self.want.reshape(-1).tolist())) > 1000
        self.obj = mic.Mic(1.0, 0)
        self.x_dev, self.st_dev = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(st).to("cuda:0")


def test_many_rows_mic(torch, idx):
    c = _Mic(torch)
    x = c.x_dev[idx]
    state = c.st_dev[idx].clone()
    big, out = _guarded(R, c.N, torch, torch.int32)
    c.obj.modulate(x, state=state, out=out)
    torch.cuda.synchronize()
    _rows_equal("mic", out, c.want.view(np.int32), idx, torch)
    _rows_equal("mic, states", state, c.want_st, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _mic_compact(c, torch):
    x3, st3 = c.x_dev[2:5].contiguous(), c.st_dev[2:5].contiguous()
    state = st3.clone()
    out, _ = c.obj.modulate(x3, state=state)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c.want[2:5]) and np.array_equal(state.cpu().numpy(), c.want_st[2:5])
    return x3, st3, out, state


def test_far_rows_mic_in(torch, arena4):
    c = _Mic(torch)
    x3, st3, want, want_st = _mic_compact(c, torch)
    for stride in STRIDES:
        far = _far("mic in", arena4, torch, torch.float32, c.N, stride)
        _far_in(arena4, far, x3, torch)
        state = st3.clone()
        big, out = _guarded(3, c.N, torch, torch.int32)
        c.obj.modulate(far, state=state, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(state, want_st), stride
        assert _untouched(big, out)
        _clean("mic in", arena4, far, stride)
    c.obj.close()


def test_far_rows_mic_out(torch, arena4):
    c = _Mic(torch)
    x3, st3, want, want_st = _mic_compact(c, torch)
    for stride in STRIDES:
        far = _far("mic out", arena4, torch, torch.int32, c.N, stride)
        state = st3.clone()
        c.obj.modulate(x3, state=state, out=far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch) and torch.equal(state, want_st), stride
        _clean("mic out", arena4, far, stride)
    c.obj.close()


# ------------------------------------------------------------------------------------------------------------------- ddc

class _Ddc:
    N, DECIM, FIRST = 67, 3, 2 ** 32 - 20                          # (the phase's index wraps inside the row)

    def __init__(self, torch):
        from uchirp import ddc
        self.m = ddc
        rng = np.random.default_rng(503)
        self.taps = np.stack([ddc.lpf_taps(78125.0, 3000.0, n_taps=21), ddc.lpf_taps(78125.0, 5000.0, n_taps=21, window="hann")])
        x = (rng.standard_normal((P, self.N)) * 20000.0).astype(np.float32)
        x[0] = 0.0
        x[0, 40] = 1e-39
        x[1, [0, 5, 17]] = [np.nan, np.inf, -np.inf]
        st = (rng.standard_normal((P, 128)) * 20000.0).astype(np.float32)
        st[0] = 0.0
        st[3] = (rng.standard_normal(128) * 1e-40).astype(np.float32)
        self.x, self.st = x, st
        self.set = rng.integers(0, 2, size=P)
        self.steps = rng.integers(0, 2 ** 32, size=P, dtype=np.uint64).astype(np.uint32)
        self.phases = rng.integers(0, 2 ** 32, size=P, dtype=np.uint64).astype(np.uint32)
        self.steps[4], self.phases[4] = 0, 0
        self.steps[5] = ddc.step_of(17500.0, 78125.0)
        self.count = ddc.outputs(self.FIRST, self.N, self.DECIM)[1]
        self.want = np.zeros((P, self.count), np.complex64)
        self.want_st = np.zeros((P, 128), np.float32)
        for k in range(2):
            rows = np.nonzero(self.set == k)[0]
            self.want[rows], self.want_st[rows] = ddc.emulate32(self.taps[k], x[rows], self.DECIM, self.FIRST, self.steps[rows], self.phases[rows], st[rows])
        self.want = np.ascontiguousarray(self.want).view(np.float32)         # [131, 2 count]: I, Q pairs
        self.obj = ddc.Ddc(self.taps, self.DECIM)
        self.x_dev, self.st_dev = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(st).to("cuda:0")

    def run(self, x, state, y, rows, row_map=None):
        self.obj.run(x, first=self.FIRST, steps=self.steps[rows], phases=self.phases[rows], row_map=row_map, set_index=self.set[rows].astype(np.uint32),
                     state=state, y=y)


def test_many_rows_ddc(torch, idx):
    c = _Ddc(torch)
    res = lu.residues()
    x = c.x_dev[idx]
    for name, row_map in (("ddc", None), ("ddc, row_map", lu.shuffled_map().astype(np.uint32))):
        state = c.st_dev[idx].clone()
        big, out = _guarded(R, 2 * c.count, torch)
        c.run(x, state, out, res, row_map)
        torch.cuda.synchronize()
        _rows_equal(name, out, c.want, idx, torch)
        _rows_equal(name + ", states", state, c.want_st, idx, torch)
        assert _untouched(big, out), name
    c.obj.close()


def _ddc_compact(c, torch):
    rows = np.arange(3, 6)
    x3, st3 = c.x_dev[3:6].contiguous(), c.st_dev[3:6].contiguous()
    state = st3.clone()
    out = torch.empty((3, 2 * c.count), dtype=torch.float32, device="cuda:0")
    c.run(x3, state, out, rows)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c.want[3:6].view(np.uint32))
    assert np.array_equal(state.cpu().numpy().view(np.uint32), c.want_st[3:6].view(np.uint32))
    return rows, x3, st3, out, state


def test_far_rows_ddc_in(torch, arena4):
    c = _Ddc(torch)
    rows, x3, st3, want, want_st = _ddc_compact(c, torch)
    for stride in STRIDES:
        far = _far("ddc in", arena4, torch, torch.float32, c.N, stride)
        _far_in(arena4, far, x3, torch)
        state = st3.clone()
        big, out = _guarded(3, 2 * c.count, torch)
        c.run(far, state, out, rows)
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        assert _untouched(big, out)
        _clean("ddc in", arena4, far, stride)
    c.obj.close()


def test_far_rows_ddc_out(torch, arena4):
    c = _Ddc(torch)
    rows, x3, st3, want, want_st = _ddc_compact(c, torch)
    for stride in STRIDES:
        far = _far("ddc out", arena4, torch, torch.float32, 2 * c.count, stride)
        state = st3.clone()
        c.run(x3, state, far, rows)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        _clean("ddc out", arena4, far, stride)
    c.obj.close()


# ------------------------------------------------------------------------------------------------------------------- duc

class _Duc:
    N, L, K, FIRST = 67, 3, 9, 2 ** 32 // 3 - 20                   # (the phase's index wraps inside the row)

    def __init__(self, torch):
        from uchirp import duc
        self.m = duc
        rng = np.random.default_rng(504)
        self.taps = np.stack([duc.interp_taps(self.L, self.K), duc.interp_taps(self.L, self.K, cutoff=0.3)])
        x = (rng.standard_normal((P, 2 * self.N)) * 12000.0).astype(np.float32)      # loud enough for int16 to clip now and then
        x[0] = 0.0
        x[0, 80] = 1e-39
        x[1, [0, 5, 17]] = [np.nan, np.inf, -np.inf]
        st = (rng.standard_normal((P, 256)) * 12000.0).astype(np.float32)
        st[0] = 0.0
        st[3] = (rng.standard_normal(256) * 1e-40).astype(np.float32)
        self.x, self.st = x, st
        self.set = rng.integers(0, 2, size=P).astype(np.uint32)
        self.steps = rng.integers(0, 2 ** 32, size=P, dtype=np.uint64).astype(np.uint32)
        self.phases = rng.integers(0, 2 ** 32, size=P, dtype=np.uint64).astype(np.uint32)
        self.steps[4], self.phases[4] = 0, 0
        self.steps[5] = duc.step_of(17500.0, 78125.0)
        self.count = self.N * self.L
        self.want, self.want_clip = {}, {}
        for fmt in ("f32", "i16"):
            self.want[fmt], self.want_st, self.want_clip[fmt] = duc.emulate32(self.taps, x, self.L, self.FIRST, 1, None, self.set, self.steps, self.phases, st, out=fmt)
        assert 0 < int(self.want_clip["i16"].sum()) < self.want["i16"].size
        self.obj = duc.Duc(self.taps, self.L)
        self.x_dev, self.st_dev = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(st).to("cuda:0")

    def run(self, x, state, y, rows, fmt, row_map=None, clip=None):
        self.obj.run(x, first=self.FIRST, steps=self.steps[rows], phases=self.phases[rows], row_map=row_map, set_index=self.set[rows], state=state,
                     out=fmt, y=y, clip=clip)


def test_many_rows_duc(torch, idx):
    c = _Duc(torch)
    res = lu.residues()
    x = c.x_dev[idx]
    for name, fmt, row_map in (("duc, floats", "f32", None), ("duc, int16, row_map", "i16", lu.shuffled_map().astype(np.uint32))):
        state = c.st_dev[idx].clone()
        dt = torch.float32 if fmt == "f32" else torch.int16
        big, out = _guarded(R, c.count, torch, dt)
        clip = torch.zeros(R, dtype=torch.int32, device="cuda:0")
        c.run(x, state, out, res, fmt, row_map, clip if fmt == "i16" else None)
        torch.cuda.synchronize()
        _rows_equal(name, out, c.want[fmt], idx, torch)
        _rows_equal(name + ", states", state, c.want_st, idx, torch)
        _rows_equal(name + ", clip counts", clip[:, None], c.want_clip[fmt].astype(np.int32)[:, None], idx, torch)
        assert _untouched(big, out), name
    c.obj.close()


def _duc_compact(c, torch, fmt):
    rows = np.arange(3, 6)
    x3, st3 = c.x_dev[3:6].contiguous(), c.st_dev[3:6].contiguous()
    state = st3.clone()
    out = torch.empty((3, c.count), dtype=torch.float32 if fmt == "f32" else torch.int16, device="cuda:0")
    c.run(x3, state, out, rows, fmt)
    torch.cuda.synchronize()
    w = c.want[fmt][3:6]
    assert np.array_equal(out.cpu().numpy().view(np.uint16), np.ascontiguousarray(w).view(np.uint16))
    assert np.array_equal(state.cpu().numpy().view(np.uint32), c.want_st[3:6].view(np.uint32))
    return rows, x3, st3, out, state


def test_far_rows_duc_in(torch, arena4):
    c = _Duc(torch)
    rows, x3, st3, want, want_st = _duc_compact(c, torch, "f32")
    for stride in STRIDES:
        far = _far("duc in", arena4, torch, torch.float32, 2 * c.N, stride)
        _far_in(arena4, far, x3, torch)
        state = st3.clone()
        big, out = _guarded(3, c.count, torch)
        c.run(far, state, out, rows, "f32")
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        assert _untouched(big, out)
        _clean("duc in", arena4, far, stride)
    c.obj.close()


def test_far_rows_duc_out_f32(torch, arena4):
    c = _Duc(torch)
    rows, x3, st3, want, want_st = _duc_compact(c, torch, "f32")
    for stride in STRIDES:
        far = _far("duc out, floats", arena4, torch, torch.float32, c.count, stride)
        state = st3.clone()
        c.run(x3, state, far, rows, "f32")
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        _clean("duc out, floats", arena4, far, stride)
    c.obj.close()


def test_far_rows_duc_out_i16(torch, arena2):
    c = _Duc(torch)
    rows, x3, st3, want, want_st = _duc_compact(c, torch, "i16")
    for stride in STRIDES:
        far = _far("duc out, int16", arena2, torch, torch.int16, c.count, stride)
        state = st3.clone()
        c.run(x3, state, far, rows, "i16")
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch) and torch.equal(_ints(state, torch), _ints(want_st, torch)), stride
        _clean("duc out, int16", arena2, far, stride)
    c.obj.close()


# ------------------------------------------------------------------------------------------------------------------ spec

class _Spec:
    N, SCALE = 2048, 2.0 / 2048

    def __init__(self, torch):
        from uchirp import spec
        self.m = spec
        rng = np.random.default_rng(505)
        x = (rng.standard_normal((P, self.N)) * 10.0 ** rng.uniform(0.0, 4.0, (P, 1))).astype(np.float32)
        x[0] = 0.0                                                  # a frame of zeros is zeros
        x[1] = (1000.0 * np.sin(2.0 * np.pi * 17000.0 * np.arange(self.N) / 78125.0)).astype(np.float32)
        self.x = x
        self.want = spec.model(x, scale=self.SCALE)                                                     # float64 [131, 1, 1025]
        self.bound = (spec.ERROR_C * 2.0 ** -24 * self.SCALE * spec.model(x, norm=True))[:, :, None]    # test_gpu_spec.py's _bound
        self.obj = spec.Analyser(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def held(self, got, peaks, rows):
        """the rule of tests/test_gpu_spec.py: every value inside the error form's bound of the float64 model, the record
        the first arg-max of the stored row"""
        g = got.cpu().numpy()
        pk = self.m.peaks_of(peaks)
        err = np.abs(g - self.want[rows])
        ok = bool(np.all(err <= self.bound[rows]))
        first = all((pk[m, 0]["value"], pk[m, 0]["bin"]) == (g[m, 0].max(), int(np.argmax(g[m, 0]))) for m in range(g.shape[0]))
        with np.errstate(divide="ignore", invalid="ignore"):
            print("spec: worst error / bound %.3f; records are the first arg-max: %s" % (np.nanmax(err / self.bound[rows]), first))
        return ok and first and not g[rows.index(0)].any() if 0 in rows else ok and first


def _frames(t):
    """rows [n, bins] as [n, 1, bins]: one frame a row, the frames as far apart as the rows (what out_stride states)"""
    return t.as_strided((t.shape[0], 1, t.shape[1]), (t.stride(0), t.stride(0), 1))


def test_many_rows_spec(torch, idx):
    """65 601 frames over the occupancy-derived grid: every workgroup walks a run of units; out [R, 1, 1025] is 269 MB"""
    c = _Spec(torch)
    x = c.x_dev[idx]
    big, flat = _guarded(R, 1025, torch)
    out = _frames(flat)
    got, rec = c.obj.spectra(x, scale=c.SCALE, out=out, peaks=True)
    torch.cuda.synchronize()
    assert got.data_ptr() == flat.data_ptr()
    assert c.held(got[:P], rec[:P], list(range(P)))
    first = _ints(flat, torch)[:P].contiguous()
    same = bool(torch.equal(_ints(flat, torch), first[idx])) and bool(torch.equal(rec, rec[:P].contiguous()[idx]))
    print("spec: %d rows; classes identical (values and records): %s" % (R, same))
    assert same
    assert _untouched(big, flat)
    c.obj.close()


def _spec_compact(c, torch):
    x3 = c.x_dev[0:3].contiguous()
    out, rec = c.obj.spectra(x3, scale=c.SCALE, peaks=True)
    torch.cuda.synchronize()
    assert c.held(out, rec, [0, 1, 2])
    return x3, out, rec


def test_far_rows_spec_in(torch, arena4):
    c = _Spec(torch)
    x3, want, want_rec = _spec_compact(c, torch)
    for stride in STRIDES:
        far = _far("spec in", arena4, torch, torch.float32, c.N, stride)
        _far_in(arena4, far, x3, torch)
        big, flat = _guarded(3, 1025, torch)
        _, rec = c.obj.spectra(far, scale=c.SCALE, out=_frames(flat), peaks=True)
        torch.cuda.synchronize()
        assert torch.equal(_ints(flat, torch), _ints(want[:, 0], torch)) and torch.equal(rec, want_rec), stride
        assert _untouched(big, flat)
        _clean("spec in", arena4, far, stride)
    c.obj.close()


def test_far_rows_spec_out_stride(torch, arena4):
    """out_stride lies between frames: three rows of one frame each, 2^31 + 24 floats apart"""
    c = _Spec(torch)
    x3, want, want_rec = _spec_compact(c, torch)
    for stride in STRIDES:
        far = _far("spec out", arena4, torch, torch.float32, 1025, stride)
        _, rec = c.obj.spectra(x3, scale=c.SCALE, out=_frames(far), peaks=True)
        torch.cuda.synchronize()
        assert _far_equal(far, want[:, 0], torch) and torch.equal(rec, want_rec), stride
        _clean("spec out", arena4, far, stride)
    c.obj.close()


# ------------------------------------------------------------------------------------------------------------------ rate

class _Rate:
    UP, DOWN, HALF = 3125, 1764, 24                                # 44 100 Hz -> 78 125 Hz

    def __init__(self, torch, fmt):
        from uchirp import rate
        self.m = rate
        self.obj = rate.Converter(0, self.UP, self.DOWN, self.HALF)
        info = self.obj.info
        self.n_out = rate.tile_outputs(info) + 1                   # one tile of outputs and one
        self.n_in = rate.span(info, 0, self.n_out)[1] + 3          # every output's taps lie in the row, or in front of sample 0
        rng = np.random.default_rng(506)
        x = rng.standard_normal((P, self.n_in)) * 8000.0
        x[0] = 0.0
        self.x = np.rint(np.clip(x, -32768, 32767)).astype(np.int16) if fmt == "i16" else x.astype(np.float32)
        kw = dict(n_out=self.n_out)
        self.want = rate.model(self.x, self.UP, self.DOWN, self.HALF, **kw)
        # the bound of tests/test_gpu_rate.py's _ratio: one rounding per coefficient and per step of the chain
        self.bound = (info.taps + 1) * 2.0 ** -24 * rate.model(self.x, self.UP, self.DOWN, self.HALF, magnitude=True, **kw)
        self.x_dev = torch.from_numpy(self.x).to("cuda:0")

    def held(self, got, rows):
        g = got.cpu().numpy().astype(np.float64)
        err, b = np.abs(g - self.want[rows]), self.bound[rows]
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
        print("rate: worst |gpu - model| / bound %.3f, peak %.0f" % (r.max(), np.abs(self.want[rows]).max()))
        return bool(r.max() <= 1.0) and np.abs(self.want[rows]).max() > 8000.0


@pytest.mark.parametrize("fmt", ("f32", "i16"))
def test_many_rows_rate(torch, idx, fmt):
    """R rows x 2 tiles of outputs (one whole, one of a single output) over the occupancy-derived grid"""
    c = _Rate(torch, fmt)
    x = c.x_dev[idx]
    big, out = _guarded(R, c.n_out, torch)
    c.obj.convert(x, out=out)
    torch.cuda.synchronize()
    assert c.held(out[:P], np.arange(P))
    first = _ints(out, torch)[:P].contiguous()
    same = bool(torch.equal(_ints(out, torch), first[idx]))
    print("rate, %s: %d rows of %d outputs; classes identical: %s" % (fmt, R, c.n_out, same))
    assert same
    assert _untouched(big, out)
    c.obj.close()


def _rate_compact(c, torch):
    x3 = c.x_dev[1:4].contiguous()
    out = c.obj.convert(x3, n_out=c.n_out)
    torch.cuda.synchronize()
    assert c.held(out, np.arange(1, 4))
    return x3, out


def test_far_rows_rate_in_f32(torch, arena4):
    c = _Rate(torch, "f32")
    x3, want = _rate_compact(c, torch)
    for stride in STRIDES:
        far = _far("rate in, floats", arena4, torch, torch.float32, c.n_in, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, c.n_out, torch)
        c.obj.convert(far, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)), stride
        assert _untouched(big, out)
        _clean("rate in, floats", arena4, far, stride)
    c.obj.close()


def test_far_rows_rate_in_i16(torch, arena2):
    c = _Rate(torch, "i16")
    x3, want = _rate_compact(c, torch)
    for stride in STRIDES:
        far = _far("rate in, int16", arena2, torch, torch.int16, c.n_in, stride)
        _far_in(arena2, far, x3, torch)
        big, out = _guarded(3, c.n_out, torch)
        c.obj.convert(far, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)), stride
        assert _untouched(big, out)
        _clean("rate in, int16", arena2, far, stride)
    c.obj.close()


def test_far_rows_rate_out(torch, arena4):
    c = _Rate(torch, "f32")
    x3, want = _rate_compact(c, torch)
    for stride in STRIDES:
        far = _far("rate out", arena4, torch, torch.float32, c.n_out, stride)
        c.obj.convert(x3, out=far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("rate out", arena4, far, stride)
    c.obj.close()


def _within(name, got, want, bound, mag):
    """the rule of tests/test_gpu_retime.py and tests/test_gpu_array.py: |gpu - model| <= bound wherever there is a bound,
    equal where there is none"""
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: worst |gpu - model| / bound %.4f, peak %.0f, samples with a signal %.2f" % (name, ratio.max(), np.abs(want).max(), (mag > 0).mean()))
    return bool(ratio.max() <= 1.0) and np.abs(want).max() > 1000.0 and (mag > 0).mean() > 0.5


def _classes(name, out, idx, torch):
    first = _ints(out, torch)[:P].contiguous()
    same = bool(torch.equal(_ints(out, torch), first[idx]))
    print("%s: %d rows of %d; classes identical: %s" % (name, out.shape[0], out.shape[1], same))
    return same


# ---------------------------------------------------------------------------------------------------------------- retime

class _Retime:
    N_IN, N_OUT = 300, 260                                         # 260 outputs: a tile of 256 and four

    def __init__(self, torch):
        from uchirp import retime
        self.m = retime
        rng = np.random.default_rng(507)
        x = (rng.standard_normal((P, self.N_IN)) * 2000.0).astype(np.float32)
        x[0] = 0.0
        self.x = x
        self.delay = rng.uniform(-20.0, 20.0, P)
        self.delay[1], self.delay[2] = 5.0, -3.0                   # whole delays: shifted copies
        self.slope = rng.choice([0.0, 60e-6, -150e-6, 2.0 ** -9, -2.0 ** -9], P)
        self.slope[1] = self.slope[2] = 0.0
        lines = [(j, self.delay[j], self.slope[j]) for j in range(P)]
        self.want = retime.model(x, lines, n_out=self.N_OUT, table=retime.table)
        self.mag = retime.model(x, lines, n_out=self.N_OUT, table=retime.table, magnitude=True)
        self.bound = 17.0 * 2.0 ** -24 * self.mag                  # tests/test_gpu_retime.py
        self.obj = retime.Retimer(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def lines(self, mics, classes):
        a = np.zeros(len(mics), self.m.LINE_DTYPE)
        a["mic"], a["delay_samples"], a["slope"] = mics, self.delay[classes], self.slope[classes]
        return a

    def held(self, name, got, rows):
        ok = _within(name, got, self.want[rows], self.bound[rows], self.mag[rows])
        g = got.cpu().numpy()
        copies = all(np.array_equal(g[k, 20:220], self.x[r, 20 + d:220 + d]) for k, r in enumerate(rows) for d in ((5,) if r == 1 else (-3,) if r == 2 else ()))
        return ok and copies


def test_many_rows_retime(torch, idx):
    """R lines x 2 tiles over the occupancy-derived grid; line r reads microphone row_map[r] of R input rows, across 2^16;
    R line records of 24 bytes: 1.5 MB staged"""
    c = _Retime(torch)
    x = c.x_dev[idx]
    lines = c.lines(lu.shuffled_map(), lu.residues())
    big, out = _guarded(R, c.N_OUT, torch)
    c.obj.rows_packed(x, lines, n_out=c.N_OUT, out=out)
    torch.cuda.synchronize()
    assert c.held("retime", out[:P], np.arange(P))
    assert _classes("retime", out, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _retime_compact(c, torch):
    x3 = c.x_dev[1:4].contiguous()
    lines = c.lines(np.arange(3), np.arange(1, 4))
    out = c.obj.rows_packed(x3, lines, n_out=c.N_OUT)
    torch.cuda.synchronize()
    assert c.held("retime, compact", out, np.arange(1, 4))
    return x3, lines, out


def test_far_rows_retime_in(torch, arena4):
    c = _Retime(torch)
    x3, lines, want = _retime_compact(c, torch)
    for stride in STRIDES:
        far = _far("retime in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, c.N_OUT, torch)
        c.obj.rows_packed(far, lines, n_out=c.N_OUT, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)), stride
        assert _untouched(big, out)
        _clean("retime in", arena4, far, stride)
    c.obj.close()


def test_far_rows_retime_out(torch, arena4):
    c = _Retime(torch)
    x3, lines, want = _retime_compact(c, torch)
    for stride in STRIDES:
        far = _far("retime out", arena4, torch, torch.float32, c.N_OUT, stride)
        c.obj.rows_packed(x3, lines, n_out=c.N_OUT, out=far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("retime out", arena4, far, stride)
    c.obj.close()


# ----------------------------------------------------------------------------------------------------------------- array

class _Array:
    N_IN, N_OUT = 300, 260

    def __init__(self, torch):
        from uchirp import array
        self.m = array
        rng = np.random.default_rng(508)
        x = (rng.standard_normal((P, self.N_IN)) * 2000.0).astype(np.float32)
        x[0] = 0.0
        self.x = x
        self.k = 1 + np.arange(P) % 3                              # taps of beam j; tap t hears microphone (j + 7 t) mod 131
        self.delay = rng.uniform(-20.0, 20.0, (P, 3))
        self.delay[3, 0] = 4.0
        self.weight = rng.uniform(0.2, 1.0, (P, 3)).astype(np.float32)
        self.weight[3, 0] = 1.0                                    # beam 3: one whole tap of weight 1, a shifted copy
        beams = [[((j + 7 * t) % P, self.weight[j, t], self.delay[j, t]) for t in range(self.k[j])] for j in range(P)]
        self.want = array.model(x, beams, n_out=self.N_OUT, coef=array.coefficients)
        self.mag = array.magnitude(x, beams, n_out=self.N_OUT, coef=array.coefficients)
        self.bound = (16.0 + self.k[:, None]) * 2.0 ** -24 * self.mag       # tests/test_gpu_array.py
        self.obj = array.Array(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def packed(self, classes, mic_of):
        """the host arrays of beams of the classes `classes`; mic_of(t): the input row of every beam's tap t"""
        k = self.k[classes]
        beams = np.zeros(len(classes), self.m.BEAM_DTYPE)
        beams["n_taps"] = k
        beams["first_tap"] = np.cumsum(k) - k
        taps = np.zeros(int(k.sum()), self.m.TAP_DTYPE)
        for t in range(3):
            sel = k > t
            at = beams["first_tap"][sel] + t
            taps["mic"][at] = mic_of(t)[sel]
            taps["delay_samples"][at] = self.delay[classes[sel], t]
            taps["weight"][at] = self.weight[classes[sel], t]
        return taps, beams

    def held(self, name, got, rows):
        ok = _within(name, got, self.want[rows], self.bound[rows], self.mag[rows])
        g = got.cpu().numpy()
        copies = all(np.array_equal(g[k, :200], self.x[3, 4:204]) for k, r in enumerate(rows) if r == 3)
        return ok and copies


def test_many_rows_array(torch, idx):
    """R beams x 2 tiles over the occupancy-derived grid; beam r's taps hear rows of its own block of 131 among R input rows,
    so rows past 2^16; 130 701 tap records of 16 bytes and R beam records of 8: 2.6 MB staged"""
    c = _Array(torch)
    x = c.x_dev[idx]
    r = np.arange(R)
    res = lu.residues()

    def mic_of(t):
        m = r // P * P + (res + 7 * t) % P
        return np.where(m >= R, m - P, m)

    taps, beams = c.packed(res, mic_of)
    assert len(taps) * 16 + len(beams) * 8 > 2 ** 20 and taps["mic"].max() >= 2 ** 16
    big, out = _guarded(R, c.N_OUT, torch)
    c.obj.combine_packed(x, taps, beams, n_out=c.N_OUT, out=out)
    torch.cuda.synchronize()
    assert c.held("array", out[:P], np.arange(P))
    assert _classes("array", out, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _array_compact(c, torch):
    """three beams of 1, 2 and 3 taps over three input rows (rows 3 .. 5 of the master), held to the model"""
    array = c.m
    h = c.x[3:6]
    lists = [[(0, 1.0, 4.0)], [(1, c.weight[4, 0], c.delay[4, 0]), (2, c.weight[4, 1], c.delay[4, 1])],
             [(2, c.weight[5, 0], c.delay[5, 0]), (0, c.weight[5, 1], c.delay[5, 1]), (1, c.weight[5, 2], c.delay[5, 2])]]
    taps, beams = array.pack(lists)
    x3 = c.x_dev[3:6].contiguous()
    out = c.obj.combine_packed(x3, taps, beams, n_out=c.N_OUT)
    torch.cuda.synchronize()
    want = array.model(h, lists, n_out=c.N_OUT, coef=array.coefficients)
    mag = array.magnitude(h, lists, n_out=c.N_OUT, coef=array.coefficients)
    assert _within("array, compact", out, want, (16.0 + np.array([[1.0], [2.0], [3.0]])) * 2.0 ** -24 * mag, mag)
    assert np.array_equal(out.cpu().numpy()[0, :200], h[0, 4:204])
    return x3, taps, beams, out


def test_far_rows_array_in(torch, arena4):
    c = _Array(torch)
    x3, taps, beams, want = _array_compact(c, torch)
    for stride in STRIDES:
        far = _far("array in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, c.N_OUT, torch)
        c.obj.combine_packed(far, taps, beams, n_out=c.N_OUT, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_ints(out, torch), _ints(want, torch)), stride
        assert _untouched(big, out)
        _clean("array in", arena4, far, stride)
    c.obj.close()


def test_far_rows_array_out(torch, arena4):
    c = _Array(torch)
    x3, taps, beams, want = _array_compact(c, torch)
    for stride in STRIDES:
        far = _far("array out", arena4, torch, torch.float32, c.N_OUT, stride)
        c.obj.combine_packed(x3, taps, beams, n_out=c.N_OUT, out=far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("array out", arena4, far, stride)
    c.obj.close()


# ----------------------------------------------------------------------------------------------------------------- xcorr

@pytest.fixture(scope="module")
def arena8(torch):
    a = _arena(torch, 8)
    yield a
    a.free()


def _longs(t, torch):
    return t.view(torch.int64)


def _emulation_bar(name, g, want, E, emu, error_c):
    """the rule of tests/test_gpu_xcorr.py, test_gpu_wcorr.py and test_gpu_track.py: |gpu - model| / (2^-24 E) at most four
    times the float32 emulation's on the same inputs and at most the header's ERROR_C; a reference of zeros leaves no room.
    g, want, emu [..., lags]; E [...]"""
    zero = E == 0
    unit = 2.0 ** -24 * E[~zero][:, None]
    rg, re = float((np.abs(g - want)[~zero] / unit).max()), float((np.abs(emu - want)[~zero] / unit).max())
    print("%s: |gpu - model| / (2^-24 E) %.3f, emulation %.3f, bar %.3f, ERROR_C %d" % (name, rg, re, 4.0 * re, error_c))
    return bool((g[zero] == 0).all()) and rg <= 4.0 * re and rg <= error_c


def _periodic_pairs(dtype):
    """R pairs (ref, mic) of R input rows: pair r is the master's pair (j, (j + 5) mod 131), j = r mod 131, both rows taken
    through the shuffled map, so that low pairs read rows past 2^16 and the other way round"""
    m = lu.shuffled_map()
    r, res = np.arange(R), lu.residues()
    # the partner in the same block of 131, or in the block in front where this one has no such row
    mic = r // P * P + (res + 5) % P
    mic = np.where(mic >= R, mic - P, mic)
    pairs = np.zeros(R, dtype)
    pairs["ref"], pairs["mic"] = m, m[mic]
    assert ((pairs["mic"] % P) == (res + 5) % P).all() and ((pairs["ref"] % P) == res).all() and pairs["ref"][:P].max() >= 2 ** 16
    return pairs


def _classes8(name, out, idx, torch):
    first = _longs(out, torch)[:P].contiguous()
    same = bool(torch.equal(_longs(out, torch), first[idx]))
    print("%s: %d rows of %d doubles; classes identical: %s" % (name, out.shape[0], out.shape[1], same))
    return same


class _Xcorr:
    N_IN, FIRST, N, L = 700, 40, 600, 128                          # one segment; R x 257 lags > 65 536 x 256

    def __init__(self, torch):
        from uchirp import xcorr
        self.m = xcorr
        rng = np.random.default_rng(509)
        x = (rng.standard_normal((P, self.N_IN)) * 1500.0).astype(np.float32)
        x[0] = 0.0
        x[7] = np.roll(x[2], 33)                                   # pair (2, 7): a peak at lag +33
        self.x = x
        self.pairs = [(j, (j + 5) % P) for j in range(P)]
        args = (x, self.pairs, self.FIRST, self.N, self.L)
        self.want, self.E, self.emu = xcorr.model(*args), xcorr.model(*args, magnitude=True), xcorr.emulate32(*args)
        self.obj = xcorr.Xcorr(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def held(self, name, got, rows):
        """the rule of tests/test_gpu_xcorr.py: |gpu - model| / (2^-24 E) at most four times the emulation's on the same
        inputs and at most UC_XCORR_ERROR_C; a reference of zeros leaves no room"""
        return _emulation_bar(name, got.cpu().numpy(), self.want[rows], self.E[rows], self.emu[rows], self.m.ERROR_C)


def test_many_rows_xcorr(torch, idx):
    """R pairs x 257 lags = 16.9 M sums: launch_sum's grid of 65 536 x 256 threads goes round a second time; R units over
    the occupancy-derived grid; pair records of 16 bytes, 1.05 MB staged; both rows of a pair lie across 2^16"""
    c = _Xcorr(torch)
    assert R * (2 * c.L + 1) > 65536 * 256
    x = c.x_dev[idx]
    pairs = _periodic_pairs(c.m.PAIR_DTYPE)
    lags = 2 * c.L + 1
    big, out = _guarded(R, lags, torch, torch.float64)
    c.obj.correlate(x, pairs, first=c.FIRST, n=c.N, max_lag=c.L, out=out)
    torch.cuda.synchronize()
    assert c.held("xcorr", out[:P], np.arange(P))
    assert int(np.argmax(out[2].cpu().numpy())) == c.L + 33
    assert _classes8("xcorr", out, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _xcorr_compact(c, torch):
    rows = [2, 7, 12]
    x3 = c.x_dev[rows].contiguous()
    pairs = [(0, 1), (1, 2), (2, 0)]
    out = c.obj.correlate(x3, pairs, first=c.FIRST, n=c.N, max_lag=c.L)
    torch.cuda.synchronize()
    args = (c.x[rows], pairs, c.FIRST, c.N, c.L)
    want, E, emu = c.m.model(*args), c.m.model(*args, magnitude=True), c.m.emulate32(*args)
    unit = 2.0 ** -24 * E[:, None]
    rg, re = float((np.abs(out.cpu().numpy() - want) / unit).max()), float((np.abs(emu - want) / unit).max())
    print("xcorr, compact: |gpu - model| / (2^-24 E) %.3f, emulation %.3f" % (rg, re))
    assert rg <= 4.0 * re and rg <= c.m.ERROR_C
    return x3, pairs, out


def test_far_rows_xcorr_in(torch, arena4):
    c = _Xcorr(torch)
    x3, pairs, want = _xcorr_compact(c, torch)
    for stride in STRIDES:
        far = _far("xcorr in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, 2 * c.L + 1, torch, torch.float64)
        c.obj.correlate(far, pairs, first=c.FIRST, n=c.N, max_lag=c.L, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_longs(out, torch), _longs(want, torch)), stride
        assert _untouched(big, out)
        _clean("xcorr in", arena4, far, stride)
    c.obj.close()


def test_far_rows_xcorr_corr_stride(torch, arena8):
    """two rows of doubles 2^31 + 24 apart: row 1 at 16 GiB"""
    c = _Xcorr(torch)
    x3, pairs, want = _xcorr_compact(c, torch)
    for stride in STRIDES:
        far = _far("xcorr corr", arena8, torch, torch.float64, 2 * c.L + 1, stride)
        c.obj.correlate(x3, pairs[:2], first=c.FIRST, n=c.N, max_lag=c.L, out=far)
        torch.cuda.synchronize()
        assert all(bool(torch.equal(_longs(far[r], torch), _longs(want[r], torch))) for r in range(2)), stride
        _clean("xcorr corr", arena8, far, stride)
    c.obj.close()


# ----------------------------------------------------------------------------------------------------------------- align

class _Align:
    N_IN, FIRST, N, L = 700, 50, 600, 48                           # one segment of 4096

    def __init__(self, torch):
        from uchirp import align
        self.m = align
        rng = np.random.default_rng(510)
        x = (rng.standard_normal((P, self.N_IN)) * 1500.0).astype(np.float32)
        x[0] = 0.0
        x[7] = np.roll(x[2], 33)                                   # pair (2, 7): a peak at lag +33
        self.x = x
        self.pairs = [(j, (j + 5) % P) for j in range(P)]
        self.want = align.model(x, self.pairs, self.FIRST, self.N, self.L)
        self.mag = align.model(x, self.pairs, self.FIRST, self.N, self.L, magnitude=True)
        self.obj = align.Aligner(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def held(self, name, got, want, mag):
        """the rule of tests/test_gpu_align.py's _ratio: |gpu - model| <= ROUNDINGS 2^-24 sum |x x|, equal where that is 0"""
        bound = self.m.ROUNDINGS * 2.0 ** -24 * mag
        err = np.abs(got.cpu().numpy() - want)
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        print("%s: worst |gpu - model| / bound %.4f" % (name, ratio))
        return bool((err[bound == 0] == 0).all()) and ratio <= 1.0


def test_many_rows_align(torch, idx):
    """R pairs, four to a workgroup, over the occupancy-derived grid; pair records of 16 bytes, 1.05 MB staged; both rows of a
    pair lie across 2^16"""
    c = _Align(torch)
    x = c.x_dev[idx]
    pairs = _periodic_pairs(c.m.PAIR_DTYPE)
    big, out = _guarded(R, 2 * c.L + 1, torch, torch.float64)
    c.obj.correlate(x, pairs, first=c.FIRST, n=c.N, max_lag=c.L, out=out)
    torch.cuda.synchronize()
    assert c.held("align", out[:P], c.want, c.mag)
    assert int(np.argmax(out[2].cpu().numpy())) == c.L + 33
    assert _classes8("align", out, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _align_compact(c, torch):
    rows = [2, 7, 12]
    x3 = c.x_dev[rows].contiguous()
    pairs = [(0, 1), (1, 2), (2, 0)]
    out = c.obj.correlate(x3, pairs, first=c.FIRST, n=c.N, max_lag=c.L)
    torch.cuda.synchronize()
    assert c.held("align, compact", out, c.m.model(c.x[rows], pairs, c.FIRST, c.N, c.L), c.m.model(c.x[rows], pairs, c.FIRST, c.N, c.L, magnitude=True))
    return x3, pairs, out


def test_far_rows_align_in(torch, arena4):
    c = _Align(torch)
    x3, pairs, want = _align_compact(c, torch)
    for stride in STRIDES:
        far = _far("align in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, 2 * c.L + 1, torch, torch.float64)
        c.obj.correlate(far, pairs, first=c.FIRST, n=c.N, max_lag=c.L, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_longs(out, torch), _longs(want, torch)), stride
        assert _untouched(big, out)
        _clean("align in", arena4, far, stride)
    c.obj.close()


def test_far_rows_align_corr_stride(torch, arena8):
    """two rows of doubles 2^31 + 24 apart: row 1 at 16 GiB"""
    c = _Align(torch)
    x3, pairs, want = _align_compact(c, torch)
    for stride in STRIDES:
        far = _far("align corr", arena8, torch, torch.float64, 2 * c.L + 1, stride)
        c.obj.correlate(x3, pairs[:2], first=c.FIRST, n=c.N, max_lag=c.L, out=far)
        torch.cuda.synchronize()
        assert all(bool(torch.equal(_longs(far[r], torch), _longs(want[r], torch))) for r in range(2)), stride
        _clean("align corr", arena8, far, stride)
    c.obj.close()


# ----------------------------------------------------------------------------------------------------------------- wcorr

class _Wcorr:
    N_IN, FIRST, N, L, G = 700, 40, 600, 128, 128                  # one segment at L' = 256; R x 257 lags > 65 536 x 256

    def __init__(self, torch):
        from uchirp import wcorr
        self.m = wcorr
        rng = np.random.default_rng(511)
        x = (rng.standard_normal((P, self.N_IN)) * 1500.0).astype(np.float32)
        x[0] = 0.0
        self.x = x
        self.pairs = [(j, (j + 5) % P) for j in range(P)]
        self.w = wcorr.band_weights(78125.0, 16000.0, 19000.0, 1000.0)[0]
        self.want, self.E, self.emu = self.reference(x, self.pairs)
        self.obj = wcorr.Wcorr(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def reference(self, x, pairs):
        args = (x, pairs, self.FIRST, self.N, self.L, self.G, self.w)
        return self.m.model(*args), self.m.model(*args, magnitude=True), self.m.emulate32(*args)

    def run(self, x, pairs, out=None):
        return self.obj.windows(x, pairs, self.FIRST, self.N, self.N, 1, self.L, self.G, self.w, out=out)


def test_many_rows_wcorr(torch, idx):
    """R pairs x 257 lags = 16.9 M sums: the grid of 65 536 x 256 threads of the sum kernel goes round a second time; R units
    over the occupancy-derived grid; pair records of 16 bytes, 1.05 MB staged; both rows of a pair lie across 2^16"""
    c = _Wcorr(torch)
    assert R * (2 * c.L + 1) > 65536 * 256
    x = c.x_dev[idx]
    big, out = _guarded(R, 2 * c.L + 1, torch, torch.float64)
    c.run(x, _periodic_pairs(c.m.PAIR_DTYPE), out.unsqueeze(1))
    torch.cuda.synchronize()
    assert _emulation_bar("wcorr", out[:P].cpu().numpy(), c.want, c.E, c.emu, c.m.ERROR_C)
    assert _classes8("wcorr", out, idx, torch)
    assert _untouched(big, out)
    c.obj.close()


def _wcorr_compact(c, torch):
    rows = [2, 7, 12]
    x3 = c.x_dev[rows].contiguous()
    pairs = [(0, 1), (1, 2), (2, 0)]
    out = c.run(x3, pairs)[:, 0]
    torch.cuda.synchronize()
    assert _emulation_bar("wcorr, compact", out.cpu().numpy(), *c.reference(c.x[rows], pairs), c.m.ERROR_C)
    return x3, pairs, out


def test_far_rows_wcorr_in(torch, arena4):
    c = _Wcorr(torch)
    x3, pairs, want = _wcorr_compact(c, torch)
    for stride in STRIDES:
        far = _far("wcorr in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        big, out = _guarded(3, 2 * c.L + 1, torch, torch.float64)
        c.run(far, pairs, out.unsqueeze(1))
        torch.cuda.synchronize()
        assert torch.equal(_longs(out, torch), _longs(want, torch)), stride
        assert _untouched(big, out)
        _clean("wcorr in", arena4, far, stride)
    c.obj.close()


def test_far_rows_wcorr_corr_stride(torch, arena8):
    """two rows of doubles 2^31 + 24 apart (two pairs of one window): row 1 at 16 GiB"""
    c = _Wcorr(torch)
    x3, pairs, want = _wcorr_compact(c, torch)
    for stride in STRIDES:
        far = _far("wcorr corr", arena8, torch, torch.float64, 2 * c.L + 1, stride)
        c.run(x3, pairs[:2], far.unsqueeze(1))
        torch.cuda.synchronize()
        assert all(bool(torch.equal(_longs(far[r], torch), _longs(want[r], torch))) for r in range(2)), stride
        _clean("wcorr corr", arena8, far, stride)
    c.obj.close()


# ----------------------------------------------------------------------------------------------------------------- track

class _Track:
    N_IN, FIRST, WLEN, HOP, NW, L = 620, 20, 120, 30, 16, 16       # R x 16 windows > 2^20: the crest kernel's grid cap

    def __init__(self, torch):
        from uchirp import track, xcorr
        self.m, self.xcorr = track, xcorr
        rng = np.random.default_rng(512)
        x = (rng.standard_normal((P, self.N_IN)) * 1500.0).astype(np.float32)
        x[0] = 0.0
        x[7] = np.roll(x[2], 9)                                    # pair (2, 7): a crest at lag +9 in every window
        self.x = x
        self.pairs = [(j, (j + 5) % P) for j in range(P)]
        self.want, self.E, self.emu = self.reference(x, self.pairs)
        self.obj = track.Tracker(0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def reference(self, x, pairs):
        args = (x, pairs, self.FIRST, self.WLEN, self.HOP, self.NW, self.L)
        emu = np.stack([self.xcorr.emulate32(x, pairs, self.FIRST + w * self.HOP, self.WLEN, self.L) for w in range(self.NW)], axis=1)
        return self.m.windows_model(*args), self.m.windows_model(*args, magnitude=True), emu

    def run(self, x, pairs, corr=True, nw=None):
        return self.obj.windows(x, pairs, self.FIRST, self.WLEN, self.HOP, self.NW if nw is None else nw, self.L, corr=corr)

    def crests_held(self, crest, corr):
        """tests/test_gpu_track.py: the crest records equal `select_model` of the call's own doubles"""
        cr, co = self.m.crests(crest), corr.cpu().numpy()
        return all(cr[p, w].tobytes() == self.m.select_model(co[p, w]).tobytes() for p in range(cr.shape[0]) for w in range(cr.shape[1]))


def test_many_rows_track(torch, idx):
    """R pairs x 16 windows = 1 049 616 rows: the crest kernel's grid is capped at 2^20 and its row += gridDim.x loop goes round
    twice for 1040 rows; as many units over the occupancy-derived grid of the correlation kernel; pair records of 16 bytes,
    1.05 MB staged, 139 MB of unit sums"""
    c = _Track(torch)
    assert R * c.NW > 2 ** 20
    x = c.x_dev[idx]
    lags = 2 * c.L + 1
    big, flat = _guarded(R * c.NW, lags, torch, torch.float64)
    corr = flat.as_strided((R, c.NW, lags), (c.NW * flat.stride(0), flat.stride(0), 1))
    crest, _ = c.run(x, _periodic_pairs(c.m.PAIR_DTYPE), corr)
    torch.cuda.synchronize()
    assert _emulation_bar("track", corr[:P].cpu().numpy(), c.want, c.E, c.emu, c.m.ERROR_C)
    assert c.crests_held(crest[:P], corr[:P])
    assert (c.m.finish(c.m.crests(crest[2:3]), c.L)["lag"] == 9).all()
    first = _longs(corr, torch)[:P].contiguous()
    same = bool(torch.equal(_longs(corr, torch), first[idx])) and bool(torch.equal(crest, crest[:P].contiguous()[idx]))
    print("track: %d pairs x %d windows; classes identical (correlations and crest records): %s" % (R, c.NW, same))
    assert same
    assert _untouched(big, flat)
    c.obj.close()


def _track_compact(c, torch):
    rows = [2, 7, 12]
    x3 = c.x_dev[rows].contiguous()
    pairs = [(0, 1), (1, 2), (2, 0)]
    crest, corr = c.run(x3, pairs)
    torch.cuda.synchronize()
    assert _emulation_bar("track, compact", corr.cpu().numpy(), *c.reference(c.x[rows], pairs), c.m.ERROR_C)
    assert c.crests_held(crest, corr)
    return x3, pairs, crest, corr


def test_far_rows_track_in(torch, arena4):
    c = _Track(torch)
    x3, pairs, want_crest, want = _track_compact(c, torch)
    for stride in STRIDES:
        far = _far("track in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x3, torch)
        crest, corr = c.run(far, pairs)
        torch.cuda.synchronize()
        assert torch.equal(_longs(corr, torch), _longs(want, torch)) and torch.equal(crest, want_crest), stride
        _clean("track in", arena4, far, stride)
    c.obj.close()


def test_far_rows_track_corr_stride(torch, arena8):
    """two rows of doubles 2^31 + 24 apart (the two first windows of one pair): row 1 at 16 GiB"""
    c = _Track(torch)
    x3, pairs, want_crest, want = _track_compact(c, torch)
    for stride in STRIDES:
        far = _far("track corr", arena8, torch, torch.float64, 2 * c.L + 1, stride)
        crest, _ = c.run(x3, pairs[:1], far.unsqueeze(0), nw=2)
        torch.cuda.synchronize()
        assert all(bool(torch.equal(_longs(far[w], torch), _longs(want[0, w], torch))) for w in range(2)), stride
        assert torch.equal(crest, want_crest[:1, :2]), stride
        _clean("track corr", arena8, far, stride)
    c.obj.close()


# -------------------------------------------------------------------------------------------------------------------- mf

class _Mf:
    N, T, POS0 = 300, 8, 2 ** 40 + 5                               # one segment of 2039 outputs, 8 taps

    def __init__(self, torch):
        from uchirp import mf
        self.m = mf
        rng = np.random.default_rng(513)
        x = (rng.standard_normal((P, self.N)) * 1500.0).astype(np.float32)
        x[0] = 0.0
        self.x = x
        self.taps = np.stack([mf.matched(np.sign(rng.standard_normal(self.T))), (rng.standard_normal(self.T) + 1j * rng.standard_normal(self.T)) / 4.0])
        self.set = rng.integers(0, 2, size=P)
        jobs = [(j, self.set[j]) for j in range(P)]
        self.want = mf.model(x, self.taps, jobs)
        self.bound = mf.ERROR_C * 2.0 ** -24 * mf.bound(x, self.taps, jobs, self.POS0)     # tests/test_gpu_mf.py
        assert mf.plan(self.T, self.POS0, 0, self.N)[2] == 1
        self.obj = mf.Mf(self.taps, 0)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def held(self, name, y, rows):
        err = np.abs(y.cpu().numpy() - self.want[rows])
        b = self.bound[rows]
        print("%s: worst |gpu - model| / (ERROR_C 2^-24 ||a_k|| ||h||) %.3f" % (name, (err[b > 0] / b[b > 0]).max()))
        return bool((err <= b).all()) and np.abs(self.want[rows]).max() > 1000.0


def test_many_rows_mf(torch, idx):
    """R jobs of one segment over the occupancy-derived grid in chunks of consecutive units; job r reads row row_map[r]
    across 2^16; R job records of 16 bytes, 1.05 MB staged.  The arrival records have no stride: their classes are
    compared, their definition is tests/test_gpu_mf.py's"""
    c = _Mf(torch)
    x = c.x_dev[idx]
    jobs = np.zeros(R, c.m.JOB_DTYPE)
    jobs["row"], jobs["set"] = lu.shuffled_map(), c.set[lu.residues()]
    big, flat = _guarded(R, 2 * c.N, torch)                        # complex64 rows as pairs of floats, on 8 bytes
    y = torch.view_as_complex(flat.as_strided((R, c.N, 2), (flat.stride(0), 2, 1)))
    _, rec = c.obj.run(x, jobs, pos0=c.POS0, y=y)
    torch.cuda.synchronize()
    assert c.held("mf", y[:P], np.arange(P))
    assert _classes("mf", flat, idx, torch)
    assert bool(torch.equal(rec, rec[:P].contiguous()[idx]))
    assert _untouched(big, flat)
    c.obj.close()


def _mf_compact(c, torch):
    x3 = c.x_dev[1:4].contiguous()
    jobs = [(k, c.set[1 + k]) for k in range(3)]
    y, rec = c.obj.run(x3, jobs, pos0=c.POS0)
    torch.cuda.synchronize()
    assert c.held("mf, compact", y, np.arange(1, 4))
    return x3, jobs, y, rec


def test_far_rows_mf_in(torch, arena4):
    c = _Mf(torch)
    x3, jobs, want, want_rec = _mf_compact(c, torch)
    for stride in STRIDES:
        far = _far("mf in", arena4, torch, torch.float32, c.N, stride)
        _far_in(arena4, far, x3, torch)
        y, rec = c.obj.run(far, jobs, pos0=c.POS0)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(y).view(torch.int32), torch.view_as_real(want).view(torch.int32)) and torch.equal(rec, want_rec), stride
        _clean("mf in", arena4, far, stride)
    c.obj.close()


def test_far_rows_mf_out(torch, arena8):
    """two rows of complex64 (8-byte elements) 2^31 + 24 apart: row 1 at 16 GiB"""
    c = _Mf(torch)
    x3, jobs, want, want_rec = _mf_compact(c, torch)
    for stride in STRIDES:
        far = _far("mf out", arena8, torch, torch.complex64, c.N, stride)
        _, rec = c.obj.run(x3, jobs[:2], pos0=c.POS0, y=far)
        torch.cuda.synchronize()
        assert all(bool(torch.equal(torch.view_as_real(far[r]).view(torch.int32), torch.view_as_real(want[r]).view(torch.int32))) for r in range(2)), stride
        assert torch.equal(rec, want_rec[:2]), stride
        _clean("mf out", arena8, far, stride)
    c.obj.close()


# -------------------------------------------------------------------------------------------------------- link and scene

NOISY_ROWS = np.concatenate([np.arange(0, P), np.arange(2 ** 16 - P, 2 ** 16), np.arange(2 ** 16, R)])
SEED = 0x1234567890ABCDEF
FS = 78125.0
SQRT2 = 2 ** 0.5
FIRST = 2547                                                       # the signal calls begin here: behind the frames' silent first symbol


def _noise_held(name, z, link, n):
    """tests/test_gpu_link.py's noise rule on the rows of NOISY_ROWS of a render of pure noise at sigma 1: within 1e-5 of the
    model's normals of (seed, row index, sample), relative in the tail u0 < 2^-20"""
    worst_abs = worst_rel = 0.0
    for k, r in enumerate(NOISY_ROWS):
        m, u = link.normals(SEED, int(r), 0, n)
        tail = u < 2.0 ** -20
        err = np.abs(z[k] - m)
        worst_abs = max(worst_abs, float(err[~tail].max()))
        if tail.any():
            worst_rel = max(worst_rel, float((err[tail] / np.maximum(np.abs(m[tail]), 1e-300)).max()))
    print("%s: rows 0 .. 130, 65 405 .. 65 600 of pure noise: max |z - model| %.3g, max relative error in the tail %.3g" % (name, worst_abs, worst_rel))
    return worst_abs <= 1e-5 and worst_rel <= 1e-5


class _Link:
    N = 2148                                                       # two tiles of quads and a ragged end

    def __init__(self, torch):
        from uchirp import link
        self.m = link
        rng = np.random.default_rng(514)
        self.texts = ["".join(chr(int(ch)) for ch in rng.integers(32, 127, size=int(rng.integers(0, 4)))) for _ in range(P)]
        self.amp = rng.choice([500.0, 2000.0, 8000.0], size=P)
        self.amp[0] = 0.0
        self.lead = rng.uniform(0.0, 500.0, size=P)
        self.ppm = rng.uniform(-200.0, 200.0, size=P)
        _, p = link.pack(self.texts, self.lead, self.amp, 0.0, self.ppm)
        self.want = np.stack([link.signal(self.texts[s], float(p["lead_samples"][s]), float(p["amplitude"][s]), float(p["ppm"][s]), self.N, FS, FIRST)
                              for s in range(P)])
        self.ulp = np.spacing((p["amplitude"] * np.float32(SQRT2)).astype(np.float32)).astype(np.float64)[:, None]
        self.obj = link.Link(0)

    def held(self, name, got, rows):
        """tests/test_gpu_link.py: the float signal within 8 ulp of A sqrt 2 of the model"""
        w = np.abs(got.cpu().numpy().astype(np.float64) - self.want[rows]) / self.ulp[rows]
        print("%s: max error %.3f ulp of A sqrt 2, peak %.0f" % (name, w.max(), np.abs(self.want[rows]).max()))
        return bool(w.max() <= 8.0) and np.abs(self.want[rows]).max() > 500.0

    def run(self, classes, out=None, dtype=None):
        kw = {} if dtype is None else dict(dtype=dtype)
        return self.obj.transmit([self.texts[j] for j in classes], self.lead[classes], self.amp[classes], 0.0, ppm=self.ppm[classes],
                                 n_samples=self.N, first_sample=FIRST, out=out, **kw)


def test_many_rows_link(torch, idx):
    """R streams x 3 tiles over the 8-per-CU grid; R stream records of 40 bytes and R texts: 2.8 MB staged.  The noise is a
    function of the stream's index: the periodic call has sigma 0; a second call renders pure noise in every stream, and
    rows 0 .. 130 and 65 405 .. 65 600 are held to the model's normals.  uc_link_noise_words with 600 001 counters: more than
    the 8-per-CU grid of 256 threads holds at once (524 288 on 256 CUs), so its loop goes round twice"""
    c = _Link(torch)
    big, out = _guarded(R, c.N, torch)
    c.run(lu.residues(), out)
    torch.cuda.synchronize()
    assert c.held("link", out[:P], np.arange(P))
    assert _classes("link", out, idx, torch)
    assert _untouched(big, out)
    z = c.obj.transmit([""] * R, 0.0, 0.0, 1.0, n_samples=c.N, seed=SEED)
    rows = torch.from_numpy(NOISY_ROWS).to("cuda:0")
    assert _noise_held("link", z[rows].cpu().numpy().astype(np.float64), c.m, c.N)
    n = 600001
    words = c.obj.noise_words(SEED, R - 1, 2 ** 40 - 7, n).cpu().numpy().view(np.uint32)
    assert np.array_equal(words, c.m.noise_words(SEED, R - 1, 2 ** 40 - 7, n))
    c.obj.close()


def _link_compact(c, torch):
    classes = np.arange(1, 4)
    out = c.run(classes)
    torch.cuda.synchronize()
    assert c.held("link, compact", out, classes)
    return classes, out


def test_far_rows_link_out_f32(torch, arena4):
    c = _Link(torch)
    classes, want = _link_compact(c, torch)
    for stride in STRIDES:
        far = _far("link out, floats", arena4, torch, torch.float32, c.N, stride)
        c.run(classes, far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("link out, floats", arena4, far, stride)
    c.obj.close()


def test_far_rows_link_out_i16(torch, arena2):
    c = _Link(torch)
    classes, f = _link_compact(c, torch)
    want = c.run(classes, dtype=torch.int16)
    assert np.array_equal(want.cpu().numpy(), c.m.convert(f.cpu().numpy(), c.m.DTYPE_I16))      # the formats are one signal
    for stride in STRIDES:
        far = _far("link out, int16", arena2, torch, torch.int16, c.N, stride)
        c.run(classes, far, dtype=torch.int16)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("link out, int16", arena2, far, stride)
    c.obj.close()


class _Scene:
    N = 2148

    def __init__(self, torch):
        from uchirp import link, scene
        self.m, self.link = scene, link
        rng = np.random.default_rng(515)
        self.texts = ["".join(chr(int(ch)) for ch in rng.integers(32, 127, size=int(rng.integers(1, 4)))) for _ in range(8)]
        self.mics = []
        for j in range(P):
            k = j % 4                                              # 0 .. 3 paths; microphone 0 hears nothing
            self.mics.append((0.0, [(int(rng.integers(0, 8)), float(rng.choice([-600.0, 500.0, 2000.0])), float(rng.uniform(0.0, 500.0)),
                                     float(rng.uniform(-200.0, 200.0))) for _ in range(k)]))
        self.want = scene.model(self.texts, self.mics, n_samples=self.N, first_sample=FIRST)
        # tests/test_gpu_scene.py: 8 ulp of |g| sqrt 2 per path and half an ulp of the sum of the peaks per addition
        self.bound = np.array([sum(8 * float(np.spacing(np.float32(abs(g) * SQRT2))) for _, g, _, _ in pl) +
                               max(len(pl) - 1, 0) * 0.5 * float(np.spacing(np.float32(sum(abs(g) for _, g, _, _ in pl) * SQRT2))) for _, pl in self.mics])[:, None]
        self.obj = scene.Scene(0)

    def held(self, name, got, rows):
        err = np.abs(got.cpu().numpy().astype(np.float64) - self.want[rows])
        b = self.bound[rows]
        quiet = b[:, 0] == 0
        ratio = (err[~quiet] / b[~quiet]).max()
        print("%s: worst |gpu - model| / bound %.4f, peak %.0f" % (name, ratio, np.abs(self.want[rows]).max()))
        return bool(ratio <= 1.0) and not err[quiet].any() and np.abs(self.want[rows]).max() > 2000.0

    def packed(self, classes):
        return self.m.pack(self.texts, [self.mics[j] for j in classes])


def test_many_rows_scene(torch, idx):
    """R microphones x 3 tiles over the occupancy-derived grid; 98 k path records of 24 bytes and R microphone records of 16:
    3.4 MB staged.  The noise is a function of the microphone's index: the periodic call has sigma 0; a second call renders R
    microphones without paths at sigma 1, which are the link's streams of that index bit for bit (tests/test_gpu_scene.py),
    and rows 0 .. 130 and 65 405 .. 65 600 are held to the model's normals"""
    c = _Scene(torch)
    big, out = _guarded(R, c.N, torch)
    c.obj.render_packed(*c.packed(lu.residues()), n_samples=c.N, first_sample=FIRST, out=out)
    torch.cuda.synchronize()
    assert c.held("scene", out[:P], np.arange(P))
    assert _classes("scene", out, idx, torch)
    assert _untouched(big, out)
    z = c.obj.render(c.texts, [(1.0, [])] * R, n_samples=c.N, seed=SEED)
    ln = c.link.Link(0)
    same = bool(torch.equal(_ints(z, torch), _ints(ln.transmit([""] * R, 0.0, 0.0, 1.0, n_samples=c.N, seed=SEED), torch)))
    print("scene: R microphones without paths equal the link's noise streams bit for bit: %s" % same)
    assert same
    rows = torch.from_numpy(NOISY_ROWS).to("cuda:0")
    assert _noise_held("scene", z[rows].cpu().numpy().astype(np.float64), c.link, c.N)
    ln.close()
    c.obj.close()


class _Scan:
    N_IN, FIRST, WLEN, MICS = 200, 40, 100, 3

    def __init__(self, torch):
        from uchirp import scan
        self.m = scan
        rng = np.random.default_rng(516)
        x = (rng.standard_normal((P * self.MICS, self.N_IN)) * 1500.0).astype(np.float32)
        x[0:3] = 0.0                                               # array 0 hears nothing
        self.x = x
        self.mics, self.weights = [0, 1, 2], [1.0 / 3] * 3
        self.cand = np.array([[0.0, 0.0, 0.0], [0.0, 8.5, 15.0], [0.0, 16.75, 30.5], [0.0, 25.0, 46.0], [30.5, 16.75, 0.0], [3.0, 0.0, 7.0]])
        self.want = scan.definition(x, self.mics, self.weights, self.cand, self.FIRST, self.WLEN, n_arrays=P, array_rows=self.MICS)   # [131, 1, 6]
        self.best = scan.best_model(self.want)
        assert not self.want[0].any() and len(set(self.best["beam"].reshape(-1).tolist())) > 2
        self.obj = scan.Scanner(0)
        self.obj.set_beams(self.mics, self.weights, self.cand)
        self.x_dev = torch.from_numpy(x).to("cuda:0")

    def held(self, name, power, rec, classes):
        """tests/test_gpu_scan.py: the powers are the plain-C definition's bit for bit, the best records the model's"""
        g = power.cpu().numpy().reshape(len(classes), 1, -1)
        same = np.array_equal(g.view(np.uint64), self.want[classes].view(np.uint64))
        best = self.m.best_of(rec).tobytes() == np.ascontiguousarray(self.best[classes]).tobytes()
        print("%s: %d powers equal the definition's: %s; best records equal the model's: %s" % (name, g.size, same, best))
        return same and best


def test_many_rows_scan(torch, idx):
    """R arrays of three microphones (196 803 input rows) x 1 window x 2 beam groups = 131 202 units over the occupancy-derived
    grid; R rows of powers over the best kernel's 8-per-CU grid.  The steering set is the object's: nothing is staged"""
    c = _Scan(torch)
    x = c.x_dev.view(P, c.MICS, c.N_IN)[idx].reshape(R * c.MICS, c.N_IN)
    nb = len(c.cand)
    big, out = _guarded(R, nb, torch, torch.float64)
    _, rec = c.obj.power(x, c.FIRST, c.WLEN, n_arrays=R, array_rows=c.MICS, power=out.unsqueeze(1))
    torch.cuda.synchronize()
    assert c.held("scan", out[:P], rec[:P], np.arange(P))
    assert _classes8("scan", out, idx, torch) and bool(torch.equal(rec, rec[:P].contiguous()[idx]))
    assert _untouched(big, out)
    c.obj.close()


def _scan_compact(c, torch):
    classes = np.arange(1, 3)
    x6 = c.x_dev[3:9].contiguous()
    power, rec = c.obj.power(x6, c.FIRST, c.WLEN, n_arrays=2, array_rows=c.MICS)
    torch.cuda.synchronize()
    assert c.held("scan, compact", power, rec, classes)
    return x6, power, rec


def test_far_rows_scan_in(torch, arena4):
    """one array whose three microphones lie 2^31 + 24 floats apart"""
    c = _Scan(torch)
    x6, want, want_rec = _scan_compact(c, torch)
    for stride in STRIDES:
        far = _far("scan in", arena4, torch, torch.float32, c.N_IN, stride)
        _far_in(arena4, far, x6[:3], torch)
        power, rec = c.obj.power(far, c.FIRST, c.WLEN, n_arrays=1, array_rows=c.MICS)
        torch.cuda.synchronize()
        assert torch.equal(_longs(power, torch), _longs(want[:1], torch)) and torch.equal(rec, want_rec[:1]), stride
        _clean("scan in", arena4, far, stride)
    c.obj.close()


def test_far_rows_scan_power_stride(torch, arena8):
    """two rows of doubles 2^31 + 24 apart (two arrays of one window): row 1 at 16 GiB"""
    c = _Scan(torch)
    x6, want, want_rec = _scan_compact(c, torch)
    for stride in STRIDES:
        far = _far("scan power", arena8, torch, torch.float64, len(c.cand), stride)
        _, rec = c.obj.power(x6, c.FIRST, c.WLEN, n_arrays=2, array_rows=c.MICS, power=far.unsqueeze(1))
        torch.cuda.synchronize()
        assert all(bool(torch.equal(_longs(far[r], torch), _longs(want[r, 0], torch))) for r in range(2)) and torch.equal(rec, want_rec), stride
        _clean("scan power", arena8, far, stride)
    c.obj.close()


def test_far_rows_scene_out(torch, arena4):
    c = _Scene(torch)
    classes = np.arange(1, 4)                                      # 1, 2 and 3 paths
    want = c.obj.render_packed(*c.packed(classes), n_samples=c.N, first_sample=FIRST)
    torch.cuda.synchronize()
    assert c.held("scene, compact", want, classes)
    for stride in STRIDES:
        far = _far("scene out", arena4, torch, torch.float32, c.N, stride)
        c.obj.render_packed(*c.packed(classes), n_samples=c.N, first_sample=FIRST, out=far)
        torch.cuda.synchronize()
        assert _far_equal(far, want, torch), stride
        _clean("scene out", arena4, far, stride)
    c.obj.close()
