"""The retimer on the GPU (uc_retime_rows, uchirp/retime.py): shifted copies and the array combiner's taps bit for bit, random
and crafted lines against the float64 model (retime.model with the library's own table), bit-identity under every way of
cutting the work, guards, the contract of the call, and end to end through the scene renderer, the combiner, the wide-lag
correlator and the receivers of libuchirp.so.

Bound of the model test: an output is 16 blended coefficients, one product and 15 fused multiply-adds.  The model keeps
c = T[q] + mu D[q] unrounded; the device rounds each c once (half an ulp, 2^-24 relative, of a c whose product with x is one
term of sum |c x|) and each of the 16 steps of the chain once (half an ulp of a partial sum that sum |c x| bounds), so
|gpu - model| <= 17 * 2^-24 * sum |c x| per sample.  It is not tuned to what the kernel gives.  Every test prints its
figures before it asserts (pytest -s).  Recorded figures: DESIGN.md section 14."""
import ctypes as C
import errno

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
NM, NS = 5, 3 * 1024 + 37
SLOPES = (0.0, 2.0 ** -32, -2.0 ** -32, 40e-6, -40e-6, 1e-3, -1e-3, 2.0 ** -9, -2.0 ** -9)


@pytest.fixture(scope="module")
def retime():
    from uchirp import retime as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def array():
    from uchirp import array as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def scene():
    from uchirp import scene as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def rows():
    """5 rows x (3 * 1024 + 37) samples, as floats and as integer words that are mostly no floats (device tensors and host
    copies after the cast); made once and never written."""
    import torch
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((NM, NS)) * 1000.0).astype(np.float32)
    w = rng.integers(-2 ** 27, 2 ** 27, size=(NM, NS)).astype(np.int32)
    w[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    return {"f32": (torch.from_numpy(f).to("cuda:0"), f), "i32": (torch.from_numpy(w).to("cuda:0"), w.astype(np.float32))}


def _bits(t):
    import torch
    return t.view(torch.int32)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _shifted(row, d):
    """row[j + d] with zeros shifted in"""
    want = np.zeros(len(row), np.float32)
    src = np.arange(len(row)) + d
    ok = (src >= 0) & (src < len(row))
    want[ok] = row[src[ok]]
    return want


def _line_fx(mic, lead_fx, drift_fx):
    """a line from the two integers: both quotients are exact doubles, so the library gets the integers back"""
    assert abs(lead_fx) < 2 ** 53 and abs(drift_fx) <= 2 ** 23
    return (mic, lead_fx / 2.0 ** 32, drift_fx / 2.0 ** 32)


def _crafted(retime):
    """Lines whose position steps at chosen outputs: the whole part I - j at output `at` (and with it q wraps between 255
    and 0), or the table row q alone; `at` inside a lane's four outputs (4 l + 1 .. 3), between two lanes, at a wave's first
    sample and at a tile's."""
    lines, what = [], []
    for slope in (40e-6, -40e-6, 1e-3, -1e-3, 2.0 ** -9, -2.0 ** -9):
        drift_fx = retime.fixed_model(0.0, slope)[1]
        for at in (1066, 1067, 1065, 1068, 2000, 512, 1024, 2048, 2304, 3, 3107):
            for unit, k in ((2 ** 32, 11), (2 ** 32, -4), (2 ** 24, 5 * 256 + 77), (2 ** 24, -3 * 256 + 254)):
                # rising: off(at - 1) < k unit <= off(at); falling: off(at) < k unit <= off(at - 1)
                lead_fx = k * unit - at * drift_fx if drift_fx > 0 else k * unit - (at - 1) * drift_fx
                lines.append(_line_fx(len(lines) % NM, lead_fx, drift_fx))
                what.append((at, unit))
    return lines, what


def test_crafted_lines_step_where_they_should(retime):
    lines, what = _crafted(retime)
    for (mic, d, s), (at, unit) in zip(lines, what):
        I, q, mu = retime.positions(d, s, 0, NS)
        j = np.arange(NS)
        if unit == 2 ** 32:
            assert (I - j)[at] != (I - j)[at - 1] and abs(int(q[at]) - int(q[at - 1])) == 255, (d, s, at)
        else:
            assert q[at] != q[at - 1] and (I - j)[at] == (I - j)[at - 1], (d, s, at)
        assert retime.fixed(d, s) == retime.fixed_model(d, s)


def test_integer_delays_are_shifted_copies(retime, rows):
    rt = retime.Retimer()
    delays = (0, 5, -3, 1500, -2049, NS + 3, -NS - 9)
    lines = [(m, float(d), 0.0) for d in delays for m in (0, 2, NM - 1)]
    for name, (dev, host) in rows.items():
        got = rt.rows(dev, lines).cpu().numpy()
        want = np.stack([_shifted(host[m], int(d)) for (m, d, _) in lines])
        print("copy, %s: %d of %d elements differ from the shifted input" % (name, int((got != want).sum()), got.size))
        assert got.dtype == np.float32 and np.array_equal(got, want), name
        assert np.count_nonzero(want[3 * 3]) > 1000 and not want[-1].any() and not want[-4].any()


def test_fractions_of_256_equal_the_array_combiner(retime, array, rows):
    rt, ar = retime.Retimer(), array.Array()
    lines = [(q % NM, float((q * 7) % 41 - 20) + q / 256.0, 0.0) for q in range(256)]
    lines += [(1, 1500.0 + 3.0 / 256.0, 0.0), (3, -1400.0 - 3.0 / 256.0, 0.0), (0, float(NS) + 0.5, 0.0), (4, -float(NS) - 8.5, 0.0)]
    beams = [[(m, 1.0, d)] for (m, d, _) in lines]
    for name, (dev, host) in rows.items():
        got, want = rt.rows(dev, lines), ar.combine(dev, beams)
        differ = int((_bits(got) != _bits(want)).sum())
        print("k + q / 256, %s: %d of %d elements differ in a bit from Array.combine of one weight-1 tap" % (name, differ, got.numel()))
        assert differ == 0 and float(want.abs().max()) > 1000.0, name


def test_random_and_crafted_lines_within_the_bound_of_the_model(retime, rows):
    rng = np.random.default_rng(64)
    lines = []
    for i in range(64):
        s = SLOPES[i % len(SLOPES)]
        d = float(rng.uniform(-3000.0, 3000.0)) if i % 3 else float(rng.uniform(-40.0, 40.0))
        lines.append((int(rng.integers(0, NM)), d, s))
    crafted, _ = _crafted(retime)
    lines += crafted
    assert set(s for (_, _, s) in lines[:64]) == set(SLOPES)
    rt = retime.Retimer()
    for name, (dev, host) in rows.items():
        got = rt.rows(dev, lines).cpu().numpy().astype(np.float64)
        want = retime.model(host, lines, table=retime.table)
        mag = retime.model(host, lines, table=retime.table, magnitude=True)
        bound = 17.0 * 2.0 ** -24 * mag
        err = np.abs(got - want)
        assert np.abs(want).max() > 1000.0 and (mag > 0).mean() > 0.5
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        w = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print("%d lines, %s: worst |gpu - model| / bound %.4f (line %d %r, sample %d, error %.4g, bound %.4g); median over the samples "
              "with a signal %.4f" % (len(lines), name, ratio[w], w[0], lines[w[0]], w[1], err[w], bound[w], np.median(ratio[bound > 0])))
        assert ratio.max() <= 1.0, (name, w, ratio[w])


def _mixed_lines(retime, rng, count, span, grain=1):
    """lines over every slope; with grain > 1 lead_fx is a multiple of it (delays that stay exact doubles when shifted)"""
    crafted, _ = _crafted(retime)
    out = []
    for i in range(count):
        drift_fx = retime.fixed_model(0.0, SLOPES[i % len(SLOPES)])[1]
        lead_fx = int(rng.integers(-int(span * 2 ** 32), int(span * 2 ** 32))) // grain * grain
        out.append(_line_fx(int(rng.integers(0, NM)), lead_fx, drift_fx))
    if grain == 1:
        out += crafted[::7]
    return out


@pytest.mark.parametrize("fmt", ["f32", "i32"])
def test_chunks_windows_grids_orders_and_strides_are_bit_identical(retime, rows, uc_tuning, monkeypatch, fmt):
    import torch
    x, h = rows[fmt]
    rng = np.random.default_rng(3)
    rt = retime.Retimer()
    for span, halo in ((3000.0, 3008 + 16), (40.0, 48 + 16)):        # |slope| * NS <= 6.1 samples more than the delay
        lines = _mixed_lines(retime, rng, 18, span)
        packed = retime.pack(lines)
        nl = len(lines)
        whole = rt.rows_packed(x, packed)
        assert float(whole.abs().max()) > 100.0 and whole.dtype == torch.float32
        # the output range cut into calls: 1001 samples (no multiple of four: rows start unaligned, lanes hang over the end), one block
        for step in (1001, N):
            y = torch.zeros_like(whole)
            for a in range(0, NS, step):
                b = min(a + step, NS)
                rt.rows_packed(x, packed, out_first=a, out=y[:, a:b])
            assert _same_bits(y, whole), (span, step)
        # the input handed over as the window [a - halo, b + halo) of the buffer (clipped to it)
        y = torch.zeros_like(whole)
        for a in range(0, NS, 1001):
            b = min(a + 1001, NS)
            lo, hi = max(0, a - halo), min(NS, b + halo)
            rt.rows_packed(x[:, lo:hi], packed, in_first=lo, out_first=a, out=y[:, a:b])
        assert _same_bits(y, whole), span
        # launch geometry: 1 .. 5 workgroups (UC_RETIME_GRID, read under UC_TUNING=1 when the object is created)
        for grid in range(1, 6):
            monkeypatch.setenv("UC_RETIME_GRID", str(grid))
            r2 = retime.Retimer()
            assert _same_bits(r2.rows_packed(x, packed), whole), (span, grid)
            r2.close()
        monkeypatch.delenv("UC_RETIME_GRID")
        # calls in a row (both staging slots, the host array reused and overwritten at once), lines in another order, a line alone
        order = rng.permutation(nl)
        outs = []
        buf = packed.copy()
        for sel in (order, order[::-1], np.array([nl // 2]), np.arange(nl)):
            buf[:len(sel)] = packed[sel]
            outs.append((sel, rt.rows_packed(x, buf[:len(sel)])))
            buf["delay_samples"] = 0.25
        torch.cuda.synchronize()
        for sel, y in outs:
            assert _same_bits(y, whole[torch.from_numpy(np.ascontiguousarray(sel)).to("cuda:0")]), (span, len(sel))
        # strided rows on both sides (odd pitches: rows that are not 16-byte aligned)
        xs = torch.zeros((NM, NS + 131), dtype=x.dtype, device="cuda:0")[:, 3:3 + NS]
        xs.copy_(x)
        ys = torch.full((nl, NS + 57), 7.0, dtype=torch.float32, device="cuda:0")
        rt.rows_packed(xs, packed, out=ys[:, 1:1 + NS])
        assert _same_bits(ys[:, 1:1 + NS], whole), span
        assert float(ys[:, 0].min()) == 7.0 == float(ys[:, 0].max()) and float(ys[:, 1 + NS:].min()) == 7.0 == float(ys[:, 1 + NS:].max())


@pytest.mark.parametrize("fmt", ["f32", "i32"])
def test_sample_numbers_near_2_to_the_38_give_the_same_bits(retime, rows, fmt):
    """Output and input start at 2^38 - 4096 and every lead is moved by -first * drift_fx, in integers: the same positions
    in the rows, so the same bits.  lead_fx is kept a multiple of 4096 so that the moved delay is still an exact double."""
    x, h = rows[fmt]
    rng = np.random.default_rng(38)
    first = 2 ** 38 - 4096
    rt = retime.Retimer()
    base = _mixed_lines(retime, rng, 18, 3000.0, grain=4096)
    moved = []
    for (m, d, s) in base:
        lead_fx, drift_fx = retime.fixed_model(d, s)
        far = lead_fx - first * drift_fx
        assert far % 4096 == 0 and abs(far) <= 2 ** 62                            # an exact double, a delay within 2^30
        moved.append((m, float(far) / 2.0 ** 32, s))
        assert retime.fixed(*moved[-1][1:]) == (far, drift_fx)
    whole = rt.rows(x, base)
    got = rt.rows(x, moved, in_first=first, out_first=first)
    assert float(whole.abs().max()) > 100.0 and _same_bits(got, whole)
    tail = rt.rows(x, moved, in_first=first, out_first=first + 1001, n_out=NS - 1001)
    assert _same_bits(tail, whole[:, 1001:])
    # the last sample number there is: out_first + n_out = 2^38
    end = rt.rows(x, moved, in_first=first, out_first=2 ** 38 - 5, n_out=5)
    want = retime.model(h, moved, in_first=first, out_first=2 ** 38 - 5, n_out=5, table=retime.table)
    mag = retime.model(h, moved, in_first=first, out_first=2 ** 38 - 5, n_out=5, table=retime.table, magnitude=True)
    assert (np.abs(end.cpu().numpy() - want) <= 17.0 * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("fmt", ["f32", "i32"])
def test_guards_gaps_and_ends(retime, rows, fmt):
    import torch
    x, h = rows[fmt]
    rng = np.random.default_rng(8)
    lines = _mixed_lines(retime, rng, 18, 3000.0) + [(0, -20.0, 0.0), (4, 25.5, 2.0 ** -9), (2, float(NS) + 9.0, 0.0), (1, -float(NS) - 8.0, 40e-6)]
    nl = len(lines)
    rt = retime.Retimer()
    whole = rt.rows(x, lines)
    # input rows with gaps of NaN (integer words: of the largest word, 2.1e9 after the cast) between them and around them;
    # output rows with guard values around them
    pitch = NS + 131
    big = torch.full((NM + 2, pitch), float("nan") if fmt == "f32" else 2 ** 31 - 1, dtype=x.dtype, device="cuda:0")
    xs = big[1:1 + NM, 67:67 + NS]
    xs.copy_(x)
    ys = torch.full((nl + 2, NS + 57), 7.0, dtype=torch.float32, device="cuda:0")
    rt.rows(xs, lines, out=ys[1:1 + nl, 5:5 + NS])
    got = ys[1:1 + nl, 5:5 + NS]
    assert not bool(torch.isnan(got).any())
    assert _same_bits(got, whole)
    ys[1:1 + nl, 5:5 + NS] = 7.0
    assert float(ys.min()) == 7.0 == float(ys.max())
    # positions off either end read zeros: where all 16 samples lie outside the row the output is zero, and nothing else is
    g = whole.cpu().numpy()
    for r, (m, d, s) in enumerate(lines):
        I, _, _ = retime.positions(d, s, 0, NS)
        outside = (I + 8 < 0) | (I - 7 >= NS)
        assert not g[r][outside].any(), r
    assert not g[-1].any() and not g[-2].any() and np.count_nonzero(g[-4]) > NS - 40
    assert np.array_equal(g[-4], _shifted(h[0], -20))                        # delay -20: 20 zeros, then the row


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


def test_contract(retime, rows, other_device):
    import torch
    L = retime.lib()
    x, h = rows["f32"]
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    rt = retime.Retimer(0)
    assert torch.cuda.current_device() == dev0
    lines = [(0, 2.25, 40e-6), (4, -7.5, -1e-3), (2, 100.0, 0.0)]
    packed = retime.pack(lines)
    want = rt.rows(x, lines)
    torch.cuda.synchronize()
    out = torch.full((3, NS), 7.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=retime.DTYPE_F32, n_mics=NM, in_first=0, n_in=NS, in_stride=0, ln=packed, n_lines=3,
             out_ptr=out.data_ptr(), out_first=0, n_out=NS, out_stride=0):
        rc = L.uc_retime_rows(rt._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_mics, in_first, n_in, in_stride,
                              ln.ctypes.data_as(C.c_void_p) if ln is not None else None, n_lines, C.c_void_p(out_ptr), out_first, n_out,
                              out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    def changed(field, i, v):
        b = packed.copy()
        b[field][i] = v
        return b

    host = np.zeros(NM * NS, np.float32)
    refusals = [("mic >= n_mics", dict(ln=changed("mic", 1, NM))), ("mic >= n_mics (fewer microphones)", dict(n_mics=4)),
                ("delay inf", dict(ln=changed("delay_samples", 0, np.inf))), ("delay nan", dict(ln=changed("delay_samples", 2, np.nan))),
                ("slope nan", dict(ln=changed("slope", 1, np.nan))), ("slope inf", dict(ln=changed("slope", 2, -np.inf))),
                ("|delay| > 2^30", dict(ln=changed("delay_samples", 0, 2.0 ** 30 + 1.0))),
                ("|delay| > 2^30, negative", dict(ln=changed("delay_samples", 0, -2.0 ** 30 - 1.0))),
                ("|slope| > 2^-9", dict(ln=changed("slope", 0, float(np.nextafter(2.0 ** -9, 1.0))))),
                ("|slope| > 2^-9, negative", dict(ln=changed("slope", 2, -float(np.nextafter(2.0 ** -9, 1.0))))),
                ("reserved != 0", dict(ln=changed("reserved", 1, 1))),
                ("out_first + n_out > 2^38", dict(out_first=2 ** 38 - NS + 1)), ("out_first > 2^38", dict(out_first=2 ** 38 + 1)),
                ("out_first + n_out wraps", dict(out_first=2 ** 64 - 5)),
                ("in_stride < n_in", dict(in_stride=NS - 1)), ("out_stride < n_out", dict(out_stride=NS - 1)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("no microphones", dict(n_mics=0)), ("no input samples", dict(n_in=0)), ("no lines", dict(n_lines=0)),
                ("no output samples", dict(n_out=0)),
                ("lines NULL", dict(ln=None)), ("in NULL", dict(in_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * NS)),
                ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (NM * NS - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (3 * NS - 1)))]
    if two:
        far_in = torch.zeros((NM, NS), dtype=torch.float32, device="cuda:1")
        far_out = torch.zeros((3, NS), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far_in.data_ptr())), ("out: memory of another device", dict(out_ptr=far_out.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_retime_last_error(), name
        torch.cuda.synchronize()
        assert float(out.min()) == 7.0 == float(out.max()), name          # nothing was enqueued
        assert call() == 0, name                                          # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same_bits(out, want), name
        out.fill_(7.0)
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    assert call(out_first=2 ** 38 - NS) == 0                              # the last range there is
    h2 = C.c_void_p()
    assert L.uc_retime_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_retime_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    rt.close()
    assert torch.cuda.current_device() == dev0


# ---- end to end: arrays of 8 microphones with clocks of their own, rendered by the scene renderer

def _texts(rng, count, lo, hi):
    return ["".join(chr(int(c)) for c in rng.integers(32, 127, size=int(rng.integers(lo, hi + 1)))) for _ in range(count)]


def _clocked(rng, n_arrays, n_mics, amp, snr_db):
    texts = _texts(rng, n_arrays, 2, 6)
    lead = rng.integers(25, 46, size=n_arrays) * float(N) + rng.uniform(0.0, N, size=n_arrays)
    lead = lead[:, None] + rng.uniform(0.0, 40.0, size=(n_arrays, n_mics))
    ppm = rng.uniform(-50.0, 50.0, size=(n_arrays, n_mics)).astype(np.float32).astype(np.float64)      # struct uc_scene_path holds a float
    sigma = amp / 10.0 ** (snr_db / 20.0)

    def mics(with_ppm):
        return [(sigma, [(a, amp, float(lead[a, m]), float(ppm[a, m]) if with_ppm else 0.0)]) for a in range(n_arrays) for m in range(n_mics)]

    return texts, lead, ppm, mics


def _decoded(texts, got):
    return sum(1 for t, g in zip(texts, got) if t in g)


def _sum_beams(n_arrays, n_mics):
    return [[(a * n_mics + m, 1.0 / n_mics, 0.0) for m in range(n_mics)] for a in range(n_arrays)]


def test_known_lines_restore_the_beams_of_drifting_microphones(retime, array, scene, uchirp):
    """-12 dB, 16 arrays of 8 microphones, ppm uniform in +-50.  Rows retimed by `undo` of the scene's own leads and ppm and
    summed with weight 1 / 8 decode at least as many texts as the twin scene with every ppm = 0, steered by its true
    delays, minus 1 of 16; the same drifting rows steered by the leads alone decode strictly fewer."""
    na, nm, nb = 16, 8, 104
    rng = np.random.default_rng(12)
    texts, lead, ppm, mics = _clocked(rng, na, nm, 2000.0, -12.0)
    sc, ar, rt = scene.Scene(), array.Array(), retime.Retimer()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    steered = [[(a * nm + m, w, d) for (m, w, d) in array.steer(lead[a])] for a in range(na)]
    twin = sc.render(texts, mics(False), n_samples=nb * N, seed=41)
    got_twin, _ = eng.receive_many(ar.combine(twin, steered), want_trace=False)
    del twin
    x = sc.render(texts, mics(True), n_samples=nb * N, seed=41)
    lines = [(a * nm + m,) + retime.undo(lead[a, m], ppm[a, m], lead[a].min(), 0.0) for a in range(na) for m in range(nm)]
    y = rt.rows(x, lines)
    got, _ = eng.receive_many(ar.combine(y, _sum_beams(na, nm)), want_trace=False)
    control, _ = eng.receive_many(ar.combine(x, steered), want_trace=False)
    ok, ok_twin, ok_control = _decoded(texts, got), _decoded(texts, got_twin), _decoded(texts, control)
    print("known lines, -12 dB, %d arrays of %d, ppm in +-50: retimed and summed decode %d / %d; the twin scene without clock offsets, "
          "true-steered, %d / %d; the drifting rows steered by the leads alone %d / %d" % (na, nm, ok, na, ok_twin, na, ok_control, na))
    assert ok >= ok_twin - 1, (ok, ok_twin)
    assert ok_control < ok, (ok_control, ok)


def test_estimated_lines_match_the_model_and_decode_the_same_texts(retime, array, scene, uchirp):
    """+14 dB, 8 arrays of 8 microphones, ppm uniform in +-50: the lines `drift` fits from the wide-lag correlator's windows
    (lags -128 .. 128) have slopes within 1 ppm of the scene's own and within 0.01 ppm of `drift_model`'s, and the sum of the
    rows retimed by them decodes, array by array, the text that the sum retimed by the known lines decodes."""
    from uchirp import xcorr
    na, nm, nb = 8, 8, 104
    rng = np.random.default_rng(15)
    texts, lead, ppm, mics = _clocked(rng, na, nm, 2000.0, 14.0)
    sc, ar, rt = scene.Scene(), array.Array(), retime.Retimer()
    eng = uchirp.Engine(uchirp.SYNC_CPLX, time_frame=N / FS)
    x = sc.render(texts, mics(True), n_samples=nb * N, seed=43)
    arrays = [[a * nm + m for m in range(nm)] for a in range(na)]
    xc = xcorr.Xcorr()
    lines, fits = retime.drift(x, arrays, xc, max_lag=128, retimer=rt)
    lines_model, _ = retime.drift_model(x.cpu().numpy(), arrays, max_lag=64, table=retime.table)
    worst_truth = worst_model = 0.0
    for a in range(na):
        for m in range(1, nm):
            i = a * nm + m
            _, s = retime.undo(lead[a, m], ppm[a, m], lead[a, 0], ppm[a, 0])
            assert lines[i][0] == i == lines_model[i][0]
            worst_truth = max(worst_truth, abs(lines[i][2] - s) * 1e6)
            worst_model = max(worst_model, abs(lines[i][2] - lines_model[i][2]) * 1e6)
    print("estimated lines, +14 dB, %d arrays of %d: worst |slope - truth| %.4f ppm, worst |slope - drift_model| %.5f ppm; fewest windows "
          "kept %d of %d" % (na, nm, worst_truth, worst_model, min(f["kept"] for f in fits if f), fits[1]["windows"]))
    assert worst_truth <= 1.0, worst_truth
    assert worst_model <= 0.01, worst_model
    known = [(a * nm + m,) + retime.undo(lead[a, m], ppm[a, m], lead[a, 0], ppm[a, 0]) for a in range(na) for m in range(nm)]
    got, _ = eng.receive_many(ar.combine(rt.rows(x, lines), _sum_beams(na, nm)), want_trace=False)
    want, _ = eng.receive_many(ar.combine(rt.rows(x, known), _sum_beams(na, nm)), want_trace=False)
    print("  texts from the estimated lines %r\n  texts from the known lines     %r\n  sent %r" % (got, want, texts))
    assert _decoded(texts, want) >= na - 1
    assert list(got) == list(want)
