"""The beam scanner on the GPU (uc_scan_power, uchirp/scan.py): every power against the definition in plain C
(uc_scan_power_row) bit for bit -- window lengths around the step of 256, the tile of 1024 and the segment of 4096, 1 .. 32
taps, beam counts around the wave's four and the group's sixteen, floats and words, rows on 16 bytes and one word off, delays
that take the staged and the direct path in one set -- and against the array combiner's own samples squared and added in numpy
float32; grids, arrays, cuts into calls, overlapping and gapped windows, in_first past 2^40 and the beams' order change no
bit; the best records; the contract of the calls; the C host; the code object; and the -12 dB experiment end to end into the
receiver.  Nothing here has a tolerance of its own: the GPU's bits are the definition's.  Every test prints its figures
before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import scan_util as su

pytestmark = pytest.mark.gpu

WINDOWS = (1, 3, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4100)
HANGING = ((su.IN_FIRST - 100, 257), (su.IN_FIRST + su.N_IN - 100, 300))     # (first, window_len): over the rows' first and last sample
FORMATS = ("f32", "i32")
GUARD = -7654321.0


@pytest.fixture(scope="module")
def scan():
    from uchirp import scan as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ref(scan):
    """The rows of tests/scan_util.py per format, on the host and on the device, and per (tap count, format) the
    definition's powers: the 9 base beams over every window of WINDOWS and HANGING, and all 65 beams over 257 samples; made
    once and never written."""
    import torch
    f, w = su.rows()
    out = {"host": {"f32": f, "i32": w}, "dev": {"f32": torch.from_numpy(f).to("cuda:0"), "i32": torch.from_numpy(w).to("cuda:0")}}
    for nt in su.TAP_COUNTS:
        mics, wt, d = su.steering(nt)
        q = scan.quantise_model(d)
        out[nt] = (mics, wt, d)
        for fmt in FORMATS:
            x = out["host"][fmt]
            sweep = {(su.FIRST, wl): np.array([scan.power_row(x, mics, wt, q[b], su.FIRST, wl, su.IN_FIRST) for b in range(su.N_BASE)]) for wl in WINDOWS}
            for first, wl in HANGING:
                sweep[(first, wl)] = np.array([scan.power_row(x, mics, wt, q[b], first, wl, su.IN_FIRST) for b in range(su.N_BASE)])
            every = np.array([scan.power_row(x, mics, wt, q[b], su.FIRST, 257, su.IN_FIRST) for b in range(65)])
            # (over the rows' last sample the beam with the delay of 5000 samples hears nothing: its power is +0.0)
            assert all(np.isfinite(v).all() and (v >= 0).all() and ((v > 0).all() or k[0] != su.FIRST) for k, v in sweep.items())
            out[(nt, fmt)] = {"sweep": sweep, "all": every}
    return out


def _layouts(x, torch):
    """x twice: rows on 16 bytes (a stride that is a multiple of 4, larger than the rows), and rows one word off 16 bytes"""
    nr, n = x.shape
    stride = (n + 3) // 4 * 4 + 8
    for name, off, st in (("on 16 bytes", 4, stride), ("one word off", 1, stride + 1)):
        big = torch.full((nr * st + 8,), 0x7FC00000 if x.dtype == torch.int32 else float("nan"), dtype=x.dtype, device=x.device)
        view = big[off:off + nr * st].view(nr, st)[:, :n]
        view.copy_(x)
        assert view.data_ptr() % 16 == (4 * off) % 16
        yield name, view


def _same(t, want):
    return np.array_equal(su.bits(t.cpu().numpy().reshape(-1)), su.bits(np.asarray(want).reshape(-1)))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_taps", su.TAP_COUNTS)
def test_powers_equal_the_definition_bit_for_bit(scan, ref, n_taps, fmt):
    import torch
    mics, wt, d = ref[n_taps]
    r = ref[(n_taps, fmt)]
    sc = scan.Scanner()
    sc.set_beams(mics, wt, d[:su.N_BASE])
    direct = sc.direct_beams()
    print("%d taps, %s: %d of %d base beams take the direct path" % (n_taps, fmt, direct, su.N_BASE))
    assert 1 <= direct < su.N_BASE                                   # one set, both kernel paths (beam 3 holds a delay of 5000 samples)
    calls = 0
    for name, x in _layouts(ref["dev"][fmt], torch):
        for (first, wl), want in r["sweep"].items():
            p, rec = sc.power(x, first, wl, in_first=su.IN_FIRST)
            assert p.shape == (1, 1, su.N_BASE) and p.dtype == torch.float64
            assert _same(p, want), (name, first, wl, p.cpu().numpy(), want)
            best = scan.best_of(rec)
            assert best.shape == (1, 1) and best[0, 0] == scan.best_model(want), (name, first, wl)
            calls += 1
    # beam counts around the wave's 4 and the group's 16: the first n beams of the same 65
    x = ref["dev"][fmt]
    for n in su.BEAM_COUNTS:
        sc.set_beams(mics, wt, d[:n])
        p, _ = sc.power(x, su.FIRST, 257, in_first=su.IN_FIRST)
        assert _same(p, r["all"][:n]), n
        calls += 1
    assert 2 <= sc.direct_beams() < 65                               # (65 beams: beam 40 holds -3000 too)
    print("%d taps, %s: %d calls, every power equal" % (n_taps, fmt, calls))
    sc.close()


def _sum_squares32(y):
    """The definition's sum of squares of float32 samples y [n] in numpy float32, operation for operation."""
    total = 0.0
    for seg in range(0, y.size, 4096):
        part = np.zeros(4096, np.float32)
        chunk = y[seg:seg + 4096]
        part[:chunk.size] = chunk                                    # (a sample behind the end adds +0.0: the same bits as not adding)
        lanes = part.reshape(16, 64, 4).transpose(1, 0, 2).reshape(64, 64)   # chain l: its samples ascending
        acc = np.zeros(64, np.float32)
        for t in range(64):
            s = lanes[:, t] * lanes[:, t]
            acc = acc + s
        for h in (32, 16, 8, 4, 2, 1):
            acc[:h] = acc[:h] + acc[h:2 * h]
        total = total + float(acc[0])
    return total


@pytest.mark.parametrize("n_taps", (2, 32))
def test_powers_equal_the_array_combiner_s_samples_squared_and_added(scan, ref, n_taps):
    from uchirp import array
    mics, wt, d = ref[n_taps]
    q = scan.quantise_model(d[:su.N_BASE])
    x = ref["dev"]["f32"]
    beams = scan.beams_of(np.arange(su.N_BASE), d[:su.N_BASE], mics, wt)
    ar = array.Array()
    for wl in (257, 4097):
        y = ar.combine(x, beams, in_first=su.IN_FIRST, out_first=su.FIRST, n_out=wl).cpu().numpy()
        got = np.array([_sum_squares32(row) for row in y])
        want = ref[(n_taps, "f32")]["sweep"][(su.FIRST, wl)]
        print("%d taps, window %d: %d of %d powers of the combiner's samples equal the scan's" % (n_taps, wl, int((su.bits(got) == su.bits(want)).sum()), su.N_BASE))
        assert np.array_equal(su.bits(got), su.bits(want)), (wl, q[0])
    ar.close()


def test_grids_arrays_cuts_and_orders_give_the_same_bits(scan, ref, uc_tuning, monkeypatch):
    import torch
    nt = 8
    mics, wt, d = ref[nt]
    d = d[:21]
    f = ref["host"]["f32"]
    # three arrays of 8 rows (two more than the taps use): array 0 is the rows of scan_util, 1 and 2 are other noise
    rng = np.random.default_rng(77)
    x3h = (rng.standard_normal((24, su.N_IN)) * 20000.0).astype(np.float32)
    x3h[:su.ARRAY_ROWS] = f
    x3 = torch.from_numpy(x3h).to("cuda:0")
    first, wl, hop, nw = su.FIRST, 300, 130, 4                       # overlapping windows
    sc = scan.Scanner()
    sc.set_beams(mics, wt, d)
    assert 1 <= sc.direct_beams() < 21
    whole, rec = sc.power(x3, first, wl, hop=hop, n_windows=nw, n_arrays=3, array_rows=8, in_first=su.IN_FIRST)
    want = np.stack([scan.definition(x3h[8 * a:8 * a + 8], mics, wt, d, first, wl, hop, nw, in_first=su.IN_FIRST)[0] for a in range(3)])
    assert _same(whole, want)
    assert np.array_equal(scan.best_of(rec), scan.best_model(want))
    # one array alone; one call per window; gapped windows; in_first past 2^40; beams in another order
    one, _ = sc.power(x3[:8], first, wl, hop=hop, n_windows=nw, n_arrays=1, array_rows=8, in_first=su.IN_FIRST)
    assert _same(one, want[:1])
    one6, _ = sc.power(x3[:6], first, wl, hop=hop, n_windows=nw, in_first=su.IN_FIRST)
    assert _same(one6, want[:1])
    for w in range(nw):
        p, _ = sc.power(x3, first + w * hop, wl, n_arrays=3, array_rows=8, in_first=su.IN_FIRST)
        assert _same(p[:, 0], want[:, w]), w
    gapped, _ = sc.power(x3, first, 130, hop=260, n_windows=2, n_arrays=3, array_rows=8, in_first=su.IN_FIRST)
    short = np.stack([scan.definition(x3h[8 * a:8 * a + 8], mics, wt, d, first, 130, 260, 2, in_first=su.IN_FIRST)[0] for a in range(3)])
    assert _same(gapped, short)
    far = (1 << 44) + 12345
    moved, _ = sc.power(x3, far + (first - su.IN_FIRST), wl, hop=hop, n_windows=nw, n_arrays=3, array_rows=8, in_first=far)
    assert _same(moved, want)
    perm = np.random.default_rng(5).permutation(21)
    sc.set_beams(mics, wt, d[perm])
    shuffled, _ = sc.power(x3, first, wl, hop=hop, n_windows=nw, n_arrays=3, array_rows=8, in_first=su.IN_FIRST)
    assert _same(shuffled, want[:, :, perm])
    sc.close()
    # launch geometry: 1 .. 5 workgroups walk the 3 x 4 x 2 units (UC_SCAN_GRID, read under UC_TUNING=1 when the object is created)
    for grid in (1, 2, 3, 4, 5):
        monkeypatch.setenv("UC_SCAN_GRID", str(grid))
        s2 = scan.Scanner()
        s2.set_beams(mics, wt, d)
        got, rec2 = s2.power(x3, first, wl, hop=hop, n_windows=nw, n_arrays=3, array_rows=8, in_first=su.IN_FIRST)
        assert _same(got, want) and np.array_equal(scan.best_of(rec2), scan.best_model(want)), grid
        s2.close()
    monkeypatch.delenv("UC_SCAN_GRID")
    print("3 arrays x 4 overlapping windows x 21 beams: one array, single windows, gapped windows, in_first 2^44, shuffled beams and grids 1 .. 5 give the same bits")


def test_best_records_ties_nan_and_absent_outputs(scan, ref):
    import torch
    nt = 2
    mics, wt, d = ref[nt]
    f = ref["host"]["f32"]
    # the strongest of the first 20 beams gets a twin three places on: two equal greatest powers, the lower index wins
    p0 = ref[(nt, "f32")]["all"]
    top = int(np.argmax(p0[:20]))
    d20 = d[:20].copy()
    twin = (top + 3) % 20
    lo, hi = min(top, twin), max(top, twin)
    d20[twin] = d20[top]
    sc = scan.Scanner()
    sc.set_beams(mics, wt, d20)
    x = ref["dev"]["f32"]
    p, rec = sc.power(x, su.FIRST, 257, in_first=su.IN_FIRST)
    ph = p.cpu().numpy()[0, 0]
    best = scan.best_of(rec)[0, 0]
    print("twins %d and %d: powers %r %r, best %r" % (lo, hi, ph[lo], ph[hi], best))
    assert su.bits(ph[lo]) == su.bits(ph[hi]) == su.bits(p0[top]) and int(best["beam"]) == lo and best["flags"] == 0 and su.bits(best["power"]) == su.bits(p0[top])
    # a NaN in array 1 of 2: exactly its windows that reach it are flagged (taps read -7 .. +8 around the shifted sample)
    xh = np.concatenate([f, f]).copy()
    at = 1000
    xh[su.ARRAY_ROWS + int(mics[0]), at] = np.nan
    x2 = torch.from_numpy(xh).to("cuda:0")
    sc.set_beams(mics, wt, d[:5])
    wl, nw = 64, 24
    first = su.IN_FIRST + 200
    p, rec = sc.power(x2, first, wl, n_windows=nw, n_arrays=2, in_first=su.IN_FIRST)
    want = np.stack([scan.definition(xh[6 * a:6 * a + 6], mics, wt, d[:5], first, wl, None, nw, in_first=su.IN_FIRST)[0] for a in range(2)])
    best = scan.best_of(rec)
    flagged = np.nonzero(best["flags"][1])[0].tolist()
    print("NaN at element %d of array 1: windows %s flagged" % (at, flagged))
    assert _same(p, want) and np.array_equal(best, scan.best_model(want))
    assert (best["flags"][0] == 0).all() and 1 <= len(flagged) < nw and (best["beam"][1][flagged] == 0).all() and (best["power"][1][flagged] == 0.0).all()
    # power_dev NULL: the records alone; best_dev NULL: the powers alone
    none, rec2 = sc.power(x2, first, wl, n_windows=nw, n_arrays=2, power=False, in_first=su.IN_FIRST)
    assert none is None and np.array_equal(scan.best_of(rec2), best)
    p3, rec3 = sc.power(x2, first, wl, n_windows=nw, n_arrays=2, best=False, in_first=su.IN_FIRST)
    assert rec3 is None and _same(p3, want)
    # a strided power_dev among guard words
    big = torch.full((2 * nw * 9 + 4,), GUARD, dtype=torch.float64, device="cuda:0")
    view = big[2:2 + 2 * nw * 9].view(2, nw, 9)[:, :, :5]
    got, _ = sc.power(x2, first, wl, n_windows=nw, n_arrays=2, power=view, in_first=su.IN_FIRST)
    assert got.data_ptr() == view.data_ptr() and _same(view, want)
    view.fill_(GUARD)
    assert float(big.min()) == GUARD == float(big.max())
    sc.close()


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


def test_contract(scan, ref, other_device):
    import torch
    L = scan.lib()
    nt, fmt = 2, "f32"
    mics, wt, d = ref[nt]
    d = np.ascontiguousarray(d[:su.N_BASE])
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    sc = scan.Scanner()
    sc.set_beams(mics, wt, d)
    assert torch.cuda.current_device() == dev0
    x = ref["dev"][fmt]
    nr, n = x.shape
    wl = 257
    want = ref[(nt, fmt)]["sweep"][(su.FIRST, wl)]
    nb = su.N_BASE
    out = torch.full((nb + 3,), GUARD, dtype=torch.float64, device="cuda:0")
    rec = torch.zeros((4,), dtype=torch.int32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=scan.DTYPE_F32, n_rows=nr, in_first=su.IN_FIRST, n_in=n, in_stride=0, n_arrays=1, array_rows=nr,
             first=su.FIRST, window_len=wl, hop=wl, n_windows=1, power_ptr=out.data_ptr(), power_stride=0, best_ptr=rec.data_ptr()):
        rc = L.uc_scan_power(sc._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_rows, in_first, n_in, in_stride, n_arrays, array_rows, first,
                             window_len, hop, n_windows, C.c_void_p(power_ptr), power_stride, C.c_void_p(best_ptr), stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(64, np.float64)
    refusals = [("in NULL", dict(in_ptr=None)), ("both outputs NULL", dict(power_ptr=None, best_ptr=None)),
                ("no rows", dict(n_rows=0)), ("no samples", dict(n_in=0)), ("no arrays", dict(n_arrays=0)), ("no array rows", dict(array_rows=0)),
                ("no window", dict(window_len=0)), ("no hop", dict(hop=0)), ("no windows", dict(n_windows=0)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("more array rows than rows", dict(n_arrays=2)), ("a mic of the set beyond array_rows", dict(array_rows=1)),
                ("in_stride < n_in", dict(in_stride=n - 1)), ("power_stride < n_beams", dict(power_stride=nb - 1)),
                ("in_stride > 2^40", dict(in_stride=2 ** 40 + 1)), ("power_stride > 2^40", dict(power_stride=2 ** 40 + 1)),
                ("in_first > 2^52", dict(in_first=2 ** 52 + 1)), ("first > 2^52", dict(first=2 ** 52 + 1)), ("window_len > 2^40", dict(window_len=2 ** 40 + 1)),
                ("hop > 2^40", dict(hop=2 ** 40 + 1)), ("windows beyond 2^53", dict(hop=2 ** 40, n_windows=2 ** 14)),
                ("more than 2^32 - 1 triples", dict(n_windows=2 ** 32 // nb + 1, hop=1)),
                ("in not on 4 bytes", dict(in_ptr=x.data_ptr() + 2)), ("power not on 8 bytes", dict(power_ptr=out.data_ptr() + 4)),
                ("best not on 8 bytes", dict(best_ptr=rec.data_ptr() + 4)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("power: host memory", dict(power_ptr=host.ctypes.data)),
                ("best: host memory", dict(best_ptr=host.ctypes.data)),
                ("power overlaps in", dict(power_ptr=x.data_ptr() + 8)), ("best overlaps in", dict(best_ptr=x.data_ptr() + 4 * (nr * n - 2))),
                ("best overlaps power", dict(best_ptr=out.data_ptr() + 8 * (nb - 1)))]
    if two:
        far = torch.zeros((nr, n), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far.data_ptr())), ("power: memory of another device", dict(power_ptr=far.data_ptr())),
                     ("best: memory of another device", dict(best_ptr=far.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_scan_last_error(), name
        torch.cuda.synchronize()
        assert float(out.min()) == GUARD == float(out.max()) and int(rec.abs().max()) == 0, name       # nothing was enqueued
        assert call() == 0, name                                                                      # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same(out[:nb], want) and float(out[nb:].min()) == GUARD and scan.best_of(rec.view(1, 1, 4))[0, 0] == scan.best_model(want), name
        out.fill_(GUARD)
        rec.zero_()
    print("contract: %d refused calls, a valid call behind each gives the definition's bits" % len(refusals))
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    # set_beams is all or nothing: a refused upload leaves the set as it was
    u32, f32, f64 = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    m32 = np.ascontiguousarray(mics, np.uint32)
    other = np.ascontiguousarray(d[::-1])
    poisoned = other.copy()
    poisoned[-1, -1] = np.nan
    far_d = other.copy()
    far_d[0, 0] = 2.0 ** 20 + 1.0
    bad_w = wt.copy()
    bad_w[1] = np.inf
    mp, wp = m32.ctypes.data_as(u32), wt.ctypes.data_as(f32)
    for name, args in (("NaN in the last delay", (mp, wp, nt, poisoned.ctypes.data_as(f64), nb, 0)), ("a delay beyond 2^20", (mp, wp, nt, far_d.ctypes.data_as(f64), nb, 0)),
                       ("a weight that is not finite", (mp, bad_w.ctypes.data_as(f32), nt, other.ctypes.data_as(f64), nb, 0)),
                       ("no taps", (mp, wp, 0, other.ctypes.data_as(f64), nb, 0)), ("33 taps", (mp, wp, 33, other.ctypes.data_as(f64), nb, 0)),
                       ("no beams", (mp, wp, nt, other.ctypes.data_as(f64), 0, 0)), ("2^20 + 1 beams", (mp, wp, nt, other.ctypes.data_as(f64), 2 ** 20 + 1, 0)),
                       ("delay_stride < n_taps", (mp, wp, nt, other.ctypes.data_as(f64), nb, nt - 1)),
                       ("mics NULL", (None, wp, nt, other.ctypes.data_as(f64), nb, 0)), ("weights NULL", (mp, None, nt, other.ctypes.data_as(f64), nb, 0)),
                       ("delays NULL", (mp, wp, nt, None, nb, 0))):
        assert L.uc_scan_set_beams(sc._h, *args) == -errno.EINVAL and L.uc_scan_last_error(), name
        assert torch.cuda.current_device() == dev0
        assert call() == 0
        torch.cuda.synchronize()
        assert _same(out[:nb], want), name
        out.fill_(GUARD)
    # set_beams replaced between calls: the same candidates in reverse order
    assert L.uc_scan_set_beams(sc._h, mp, wp, nt, other.ctypes.data_as(f64), nb, 0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert _same(out[:nb], want[::-1])
    out.fill_(GUARD)
    rec.zero_()
    # an object without a set refuses to run; with a set it runs
    h2 = C.c_void_p()
    assert L.uc_scan_create(0, C.byref(h2)) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == -errno.EINVAL and b"no steering set" in L.uc_scan_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == GUARD == float(out.max())
    assert L.uc_scan_set_beams(h2, mp, wp, nt, d.ctypes.data_as(f64), nb, 0) == 0 and torch.cuda.current_device() == dev0
    assert call(h_=h2) == 0
    torch.cuda.synchronize()
    assert _same(out[:nb], want)
    L.uc_scan_destroy(h2)
    h2 = C.c_void_p()
    assert L.uc_scan_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_scan_create(0, None) == -errno.EINVAL
    if two:
        # an object on the other device: its own memory runs, device 0's is refused
        s1 = scan.Scanner(device=1)
        s1.set_beams(mics, wt, d)
        got, _ = s1.power(x.to("cuda:1"), su.FIRST, wl, in_first=su.IN_FIRST)
        torch.cuda.synchronize(1)
        assert _same(got, want) and torch.cuda.current_device() == dev0
        with pytest.raises(scan.ScanError):
            s1.power(x, su.FIRST, wl, in_first=su.IN_FIRST)
        s1.close()
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        sc.power(x.double(), su.FIRST, wl)
    with pytest.raises(ValueError):
        sc.power(x, su.FIRST, wl, power=torch.zeros((1, 1, nb + 1), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        sc.power(x, su.FIRST, wl, power=False, best=False)
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    sc.close()
    assert torch.cuda.current_device() == dev0


def test_c_host_scans_and_reads_the_records(scan, tmp_path):
    import re
    import subprocess
    from test_scan_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, equal = [int(v) for v in re.search(r"(\d+) powers in one call, (\d+) equal", out.stdout).groups()]
    assert n == 10 == equal and out.stdout.count("best beam 2, flags 0") == 2


def test_code_object_shows_no_spill_and_no_scratch(scan, tmp_path, monkeypatch):
    from test_scan_cpu import code_objects
    code_objects(scan, tmp_path, monkeypatch)


QUIET_BEFORE, PAST_THE_END = 30, 4           # blocks, for the receiver alone: of noise in front of the recording, of the scene behind it


def test_end_to_end_scan_steered_beams_at_minus_12_db(scan):
    """The CPU test's 16 arrays (tests/test_scan_cpu.py proves them on the float64 models) rendered by Scene.render, 24 blocks,
    scanned in ONE call over the 181 directions, window [2048, n - 2048): the records are the definition's, the chosen
    directions meet the CPU test's caps, and the beams of `beams_of` go through Array.combine and the SYNC_CPLX receiver.

    The records are the definition's: they are the best of the GPU's own powers, and the powers of every array's chosen beam and
    of its two neighbours equal uc_scan_power_row's bit for bit (all 16 x 181 through the plain-C row function take half a
    minute).

    What the receiver is given.  "Hi" at lead 300 occupies samples 2347 .. 51453: it ends in block 26, behind the 24 blocks of
    the recording, and the receiver replays the firmware's main loop, which has to see blocks of noise before it synchronises on
    a transmission.  Handed the 24 blocks as they are it decodes NOTHING, whatever the steering and the SNR (measured:
    scan-steered 0 / 16, truth-steered 0 / 16, microphone 0 alone 0 / 16; with noise in front but cut at 24 blocks 0 / 16 too;
    the whole transmission without noise in front 0 / 16).  So for the receiver alone the SAME scenes are rendered 4 blocks
    further (same seeds: the first 24 blocks are the recording, sample for sample, which is asserted) and get 30 blocks in front
    of the same microphones' noise with the transmitter silent (same sigma, seeds 1200 + a).  The scan sees the 24 blocks only,
    and the three things decoded -- scan-steered beams, truth-steered beams, microphone 0 -- are combined from the same
    continued rows.
    Measured on the MI355X: see DESIGN.md section 22."""
    import torch
    import uchirp
    from uchirp import array, scene
    exp = su.experiment()
    na, nm = su.N_ARRAYS, su.N_MICS
    sn = scene.Scene()
    x = torch.cat([sn.render(["Hi"], exp["scenes"][a], n_samples=su.N, seed=200 + a) for a in range(na)])
    further = torch.cat([sn.render(["Hi"], exp["scenes"][a], n_samples=su.N + PAST_THE_END * 2048, seed=200 + a) for a in range(na)])
    assert torch.equal(further[:, :su.N], x)
    mics, wt = np.arange(nm), np.full(nm, 1.0 / nm, np.float32)
    sc = scan.Scanner()
    sc.set_beams(mics, wt, exp["candidates"])
    assert sc.direct_beams() == 0
    p, rec = sc.power(x, su.W_FIRST, su.W_LEN, n_arrays=na)
    ph, best = p.cpu().numpy(), scan.best_of(rec)
    assert np.array_equal(best, scan.best_model(ph)) and (best["flags"] == 0).all()
    chosen = best["beam"][:, 0].astype(np.int64)
    xh = x.cpu().numpy()
    q = scan.quantise_model(exp["candidates"])
    checked = 0
    for a in range(na):
        for b in (chosen[a] - 1, chosen[a], chosen[a] + 1):
            if 0 <= b < q.shape[0]:
                assert su.bits(scan.power_row(xh[nm * a:nm * a + nm], mics, wt, q[b], su.W_FIRST, su.W_LEN)) == su.bits(ph[a, 0, b]), (a, b)
                checked += 1
    deg, samples = su.judge(exp, chosen)
    print("scan on the GPU: directions %s; worst direction error %.2f deg, worst delay error %.4f samples; %d powers equal uc_scan_power_row's"
          % (su.CANDIDATES_DEG[chosen].astype(int).tolist(), deg, samples, checked))
    assert deg <= su.CAP_DEG and samples <= su.CAP_SAMPLES
    # for the receiver: noise in front, the scene up to the end of the transmission behind
    quiet = torch.cat([sn.render(["Hi"], [(s, [(tx, 0.0, ld, ppm) for (tx, g, ld, ppm) in paths]) for (s, paths) in exp["scenes"][a]],
                                 n_samples=QUIET_BEFORE * 2048, seed=1200 + a) for a in range(na)])
    xl = torch.cat([quiet, further], dim=1).contiguous()
    ar = array.Array()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=2048 / su.FS)
    scan_beams = scan.beams_of(best[:, 0], exp["candidates"], mics, wt, array_rows=nm)
    true_beams = [[(nm * a + m, 1.0 / nm, float(dl)) for m, dl in enumerate(exp["true_delays"][a])] for a in range(na)]
    got_scan, _ = eng.receive_many(ar.combine(xl, scan_beams), want_trace=False)
    got_true, _ = eng.receive_many(ar.combine(xl, true_beams), want_trace=False)
    alone, _ = eng.receive_many(xl[0::nm], want_trace=False)
    ok_scan, ok_true, ok_alone = (sum(1 for g in got if "Hi" in g) for got in (got_scan, got_true, alone))
    print("-12 dB, %d arrays of %d: scan-steered beams decode %d / %d, truth-steered %d / %d, microphone 0 alone %d / %d"
          % (na, nm, ok_scan, na, ok_true, na, ok_alone, na))
    eng.close()
    ar.close()
    sc.close()
    sn.close()
    assert ok_scan >= ok_true - 1, (ok_scan, ok_true)
    assert ok_scan > ok_alone, (ok_scan, ok_alone)
