"""The band-weighted correlator on the GPU (uc_wcorr_windows, uchirp/wcorr.py): with weights of one, bit for bit the
correlations of `Xcorr.correlate` per window (at guard g: the central lags of that correlator at L + g); with weights,
within the header's error form of the float64 model, exact under a power-of-two scale and zero under weights of zero; the
same bits under every way of dealing the work; the delays of 32 pairs at 0 dB equal to the model's; the estimator under
`retime.drift`; the contract of the call; and a plain C host.  Every test prints its figures before it asserts (pytest -s).

Inputs (tests/wcorr_util.py): 4 rows of 3 x 2048 + 37 samples, the smallest rows at which a full group and one more sample
fit at L' >= 253."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

import wcorr_util as wu
from test_wcorr_cpu import _same_bits, build_host

pytestmark = pytest.mark.gpu

NM, NS, PAIRS = wu.NM, wu.NS, wu.PAIRS
FILL = -7.5


@pytest.fixture(scope="module")
def wcorr():
    from uchirp import wcorr as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def xcorr():
    from uchirp import xcorr as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def mics():
    """the rows of wcorr_util.mics() as (device tensor, host array) per format; made once and never written"""
    import torch
    return {k: (torch.from_numpy(np.array(v)).to("cuda:0"), v) for k, v in wu.mics().items()}


def _guarded(torch, n_pairs, nw, lags):
    """a correlation buffer with three fill values behind every row: (the view to hand over, the whole buffer)"""
    whole = torch.full((n_pairs, nw, lags + 3), FILL, dtype=torch.float64, device="cuda:0")
    return whole[:, :, :lags], whole


@pytest.mark.parametrize("L,g", wu.LAG_GUARD)
def test_ones_are_xcorr_per_window_and_weights_meet_the_error_form(wcorr, xcorr, mics, L, g):
    """Over every case of the list: weights NULL and an explicit table of ones give the central 2 L + 1 lags of
    `Xcorr.correlate` at L + g per window, bit for bit, into a strided buffer whose fill values stay; for one case per
    window_len (and the last), every weight table of the list within the error form of `windows_model`."""
    import torch
    wc, xc = wcorr.Wcorr(), xcorr.Xcorr()
    lags, Lp = 2 * L + 1, L + g
    cases = wu.cases(Lp)
    ones = np.ones(wcorr.BINS, np.float32)
    tables = wu.weight_tables()
    worst, checked, seen_wl = 0.0, 0, set()
    for name in ("f32", "i32"):
        dev, host = mics[name]
        xs = torch.zeros((NM, NS + 131), dtype=dev.dtype, device="cuda:0")[:, 3:3 + NS]      # strided rows with an odd pitch
        xs.copy_(dev)
        for i, (first, wl, hop, nw) in enumerate(cases):
            src = xs if i % 4 == 3 else dev
            want = torch.stack([xc.correlate(dev, PAIRS, first=first + w * hop, n=wl, max_lag=Lp) for w in range(nw)], dim=1)[:, :, g:g + lags]
            for weights in (None, ones):
                view, whole = _guarded(torch, len(PAIRS), nw, lags)
                assert wc.windows(src, PAIRS, first, wl, hop, nw, L, g, weights, out=view) is view
                assert torch.equal(view, want), (name, L, g, first, wl, hop, nw, weights is None)
                assert bool((whole[:, :, lags:] == FILL).all()), (name, L, g, first, wl, hop, nw)
            if (name, wl) not in seen_wl or (first, wl, hop, nw) == cases[-1]:
                seen_wl.add((name, wl))
                E = wcorr.windows_model(host, PAIRS, first, wl, hop, nw, L, g, magnitude=True)
                for tname, w in tables:
                    got = wc.windows(src, PAIRS, first, wl, hop, nw, L, g, w).cpu().numpy()
                    model = wcorr.windows_model(host, PAIRS, first, wl, hop, nw, L, g, w)
                    ratio = wu.error_ratio(got, model, E, float(np.abs(w).max()))
                    worst = max(worst, ratio)
                    checked += 1
                    assert ratio <= wcorr.ERROR_C, (name, L, g, first, wl, hop, nw, tname, ratio)
    print("L %3d guard %3d: %d cases x 2 formats x {NULL, ones} bit-equal to Xcorr.correlate at L + guard per window; %d weighted calls, worst "
          "|gpu - model| / (2^-24 max|w| E) %.3f (bar %d)" % (L, g, len(cases), checked, worst, wcorr.ERROR_C))
    assert checked >= 2 * 5 * len(tables)
    wc.close()
    xc.close()


def test_case_list_covers_what_the_issue_names():
    for L, g in wu.LAG_GUARD:
        S = 2048 - 2 * (L + g)
        cases = wu.cases(L + g)
        wls = {c[1] for c in cases}
        assert {1, S - 1, S, S + 1, 2048} <= wls and ((4 * S in wls and 4 * S + 1 in wls) == (4 * S + 1 <= NS))
        assert {c[3] for c in cases} == {1, 2, 3, 7}
        for wl in wls - {1}:
            hops = {c[2] for c in cases if c[1] == wl}
            assert {1, wl} <= hops and (wl <= 3 or wl - 3 in hops) and wl + 5 in hops, (L, g, wl, hops)
        assert any(c[0] == 0 for c in cases) and any(c[0] % 2 == 1 for c in cases)
        assert any(c[0] + (c[3] - 1) * c[2] + c[1] == NS and c[0] > 0 for c in cases)
    assert 4097 in {c[1] for c in wu.cases(512)} and 4 * 1024 + 1 in {c[1] for c in wu.cases(512)} and 4 * 1536 + 1 not in {c[1] for c in wu.cases(192)}


def test_tracker_gives_the_same_bits_at_guard_0(wcorr, mics):
    from uchirp import track
    wc, tr = wcorr.Wcorr(), track.Tracker()
    import torch
    for name, L, first, wl, hop, nw in (("f32", 200, 3, 1649, 700, 7), ("i32", 512, 1, 4097, 1000, 3)):
        dev, _ = mics[name]
        assert torch.equal(wc.windows(dev, PAIRS, first, wl, hop, nw, L, 0), tr.windows(dev, PAIRS, first, wl, hop, nw, L, corr=True, crest=False))
    wc.close()
    tr.close()


def test_scaled_weights_scale_exactly_zero_weights_give_zero_and_impulses_give_h(wcorr, mics):
    import torch
    wc = wcorr.Wcorr()
    tables = wu.weight_tables()
    for name, L, g, first, wl, hop, nw in (("f32", 128, 128, 3, 4 * 1536 + 1, 1, 2), ("i32", 200, 56, 1, 1537, 700, 7), ("f32", 512, 0, 0, 4097, 1000, 3)):
        dev, _ = mics[name]
        for tname, w in tables[:3]:
            full = wc.windows(dev, PAIRS, first, wl, hop, nw, L, g, w)
            small = wc.windows(dev, PAIRS, first, wl, hop, nw, L, g, w * np.float32(0.125))
            assert bool(full.abs().max() > 0) and torch.equal(small, full * 0.125), (name, L, g, tname)
        zero = wc.windows(dev, PAIRS, first, wl, hop, nw, L, g, np.zeros(wcorr.BINS, np.float32))
        assert bool((zero == 0).all()) and not bool(torch.signbit(zero).any()), (name, L, g)        # +0.0
    # rows with one non-zero sample each: value_ref * value_mic * h[(l - d) mod 2048]
    x, places = wu.impulses()
    dev = torch.from_numpy(np.array(x)).to("cuda:0")
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (0, 0)]
    worst = 0.0
    for tname, w in tables:
        h = np.fft.irfft(w.astype(np.float64), 2048)
        for L, g in ((64, 128), (512, 0), (300, 100)):
            got = wc.correlate(dev, pairs, 0, None, L, g, w).cpu().numpy()
            model = wcorr.model(x, pairs, 0, None, L, g, w)
            E = wcorr.model(x, pairs, 0, None, L, g, w, magnitude=True)
            for i, (ref, mic) in enumerate(pairs):
                d = places[mic][0] - places[ref][0]
                want = places[ref][1] * places[mic][1] * h[(np.arange(-L, L + 1) - d) % 2048]
                assert np.abs(model[i] - want).max() <= 1e-12 * abs(places[ref][1] * places[mic][1]) * np.abs(w).max()
            ratio = wu.error_ratio(got, model, E, float(np.abs(w).max()))
            worst = max(worst, ratio)
            assert ratio <= wcorr.ERROR_C, (tname, L, g, ratio)
    print("impulse rows, %d weight tables: worst |gpu - model| / (2^-24 max|w| E) %.3f (bar %d)" % (len(tables), worst, wcorr.ERROR_C))
    wc.close()


def test_the_same_bits_however_the_work_is_dealt(wcorr, mics, monkeypatch):
    """Grids of 1-5 workgroups and the default, calls in a row with both staging slots and another weight table in
    between, the pairs in another order, a pair alone, a window alone."""
    import torch
    wc = wcorr.Wcorr()
    band, rnd = wu.weight_tables()[0][1], wu.weight_tables()[1][1]
    for name, L, g, first, wl, hop, nw, w in (("f32", 200, 56, 3, 1537, 700, 7, band), ("i32", 384, 128, 1, 4097, 1000, 3, rnd),
                                              ("i32", 64, 128, 0, 2048, 2048, 3, band), ("f32", 1, 0, 5, 2045, 1, 7, rnd), ("f32", 128, 128, 0, 4 * 1536 + 1, 7, 1, None)):
        dev, _ = mics[name]
        lags = 2 * L + 1
        corr0 = wc.windows(dev, PAIRS, first, wl, hop, nw, L, g, w)
        other = wc.windows(dev, PAIRS, first, wl, hop, nw, L, g, rnd if w is band else band)
        assert not torch.equal(other, corr0)
        for grid in (1, 2, 3, 4, 5):
            monkeypatch.setenv("UC_TUNING", "1")
            monkeypatch.setenv("UC_WCORR_GRID", str(grid))
            tg = wcorr.Wcorr()
            monkeypatch.delenv("UC_TUNING")
            monkeypatch.delenv("UC_WCORR_GRID")
            for turn in range(4):                                            # both staging slots, other weights in between
                view, whole = _guarded(torch, len(PAIRS), nw, lags)
                if turn == 2:
                    assert torch.equal(tg.windows(dev, PAIRS, first, wl, hop, nw, L, g, rnd if w is band else band, out=view), other)
                else:
                    assert torch.equal(tg.windows(dev, PAIRS, first, wl, hop, nw, L, g, w, out=view), corr0), (name, L, g, grid, turn)
                assert bool((whole[:, :, lags:] == FILL).all())
            tg.close()
        order = [4, 0, 5, 2, 1, 3]
        assert torch.equal(wc.windows(dev, [PAIRS[i] for i in order], first, wl, hop, nw, L, g, w), corr0[order])
        for i in (0, 1, 5):
            assert torch.equal(wc.windows(dev, [PAIRS[i]], first, wl, hop, nw, L, g, w)[0], corr0[i])
        for k in range(nw):
            assert torch.equal(wc.windows(dev, PAIRS, first + k * hop, wl, hop, 1, L, g, w)[:, 0], corr0[:, k])
            assert torch.equal(wc.correlate(dev, PAIRS, first + k * hop, wl, L, g, w), corr0[:, k])
    wc.close()


def test_delays_of_32_pairs_at_0_db_are_the_models(wcorr):
    """`uc_wcorr_peak` of the GPU's doubles against `peak_model` of `model`: the same lag and |delay difference| <= 1e-6
    samples in every one of the 32 pairs (tests/test_wcorr_cpu.py shows that their runner-up stays below 0.99)."""
    import torch
    x, pairs, truth = wu.delay_pairs(32, 0.0, 1000)
    w = wu.band()
    wc = wcorr.Wcorr()
    got = wc.correlate(torch.from_numpy(np.array(x)).to("cuda:0"), pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, wu.DELAY_L, wu.DELAY_GUARD, w).cpu().numpy()
    model = wcorr.model(x, pairs, wu.DELAY_FIRST, wu.DELAY_WINDOW, wu.DELAY_L, wu.DELAY_GUARD, w)
    worst = 0.0
    for i in range(32):
        a, b = wcorr.peak(got[i]), wcorr.peak_model(model[i])
        worst = max(worst, abs(a["delay_samples"] - b["delay_samples"]))
        assert a["lag"] == b["lag"] and a["flags"] == b["flags"] == 0, (i, a, b)
    print("32 pairs at 0 dB: worst |delay(gpu) - delay(model)| %.3g samples; worst |delay - truth| %.3f"
          % (worst, max(abs(wcorr.peak(got[i])["delay_samples"] - truth[i]) for i in range(32))))
    assert worst <= 1e-6
    wc.close()


def test_estimator_is_correlate_and_peak_and_drift_runs_over_it(wcorr, mics):
    import torch
    from uchirp import link, retime
    dev, _ = mics["f32"]
    wc = wcorr.Wcorr()
    w = wu.band()
    est = wc.estimator(w, 128)
    arrays = [[0, 1, 2], [3, 0]]
    delays, peaks = est.delays(dev, arrays, first=5, n=4096, max_lag=64)
    rows = wc.correlate(dev, [(0, 1), (0, 2), (3, 0)], 5, 4096, 64, 128, w).cpu().numpy()
    want = [wcorr.peak(r) for r in rows]
    assert delays == [[0.0, want[0]["delay_samples"], want[1]["delay_samples"]], [0.0, want[2]["delay_samples"]]]
    assert peaks[0][0] is None and peaks[1][0] is None and _same_bits(peaks[0][2], want[1]) and _same_bits(peaks[1][1], want[2])
    # two microphones with clocks of their own at +14 dB: `retime.drift` over the estimator returns a line per row
    nb, amp = 24, 2000.0
    x = link.model([wu.TEXT] * 2, [3000.0, 3011.5], amp, amp / 10.0 ** (14.0 / 20.0), [0.0, 40.0], n_samples=nb * 2048, seed=3).astype(np.float32)
    lines, fits = retime.drift(torch.from_numpy(x).to("cuda:0"), [[0, 1]], est, max_lag=64)
    print("drift over the weighted estimator: lines %r" % (lines,))
    assert len(lines) == 2 and lines[0][0] == 0 and lines[1][0] == 1 and fits[0] is None and fits[1]["kept"] >= 4
    assert abs(lines[1][2] * 1e6 + 40.0) <= 2.0                                  # the microphone's clock runs 40 ppm fast
    beams, d2, _ = wcorr.steer(dev, arrays, est, first=5, n=4096, max_lag=64)
    assert d2 == delays and len(beams) == 2 and len(beams[0]) == 3
    wc.close()


def test_contract_of_the_call(wcorr, mics):
    """Every refused argument list returns -EINVAL with a text and enqueues nothing; the next good call gives the right
    bits; the caller's device and the object survive."""
    import torch
    L = wcorr.lib()
    wc = wcorr.Wcorr()
    dev, _ = mics["f32"]
    dev0 = torch.cuda.current_device()
    band = wu.band()
    good = dict(first=3, window_len=1537, hop=700, n_windows=3, max_lag=200, guard=56, weights=band)
    corr0 = wc.windows(dev, PAIRS, **good)
    torch.cuda.synchronize()
    pairs = np.zeros(2, wcorr.PAIR_DTYPE)
    pairs["mic"] = 1
    lags, nw = 401, 3
    corr = torch.full((2 * nw * lags + 64,), FILL, dtype=torch.float64, device="cuda:0")
    host = np.zeros(1 << 16, np.float64)
    other = torch.zeros(8, dtype=torch.float64)                                  # host memory
    wbuf = np.array(band)

    def call(h=wc._h, x=dev.data_ptr(), dtype=1, n_mics=NM, n_in=NS, in_stride=NS, pr=pairs.ctypes.data, n_pairs=2, first=3, wl=1537, hop=700,
             n_windows=nw, lag=200, guard=56, w=wbuf.ctypes.data, co=corr.data_ptr(), cs=0):
        return L.uc_wcorr_windows(h, x, dtype, n_mics, n_in, in_stride, pr, n_pairs, first, wl, hop, n_windows, lag, guard, w, co, cs, None)

    bad_pairs = pairs.copy()
    bad_pairs[1]["ref"] = NM
    bad_w = [wbuf.copy() for _ in range(3)]
    bad_w[0][0], bad_w[1][512], bad_w[2][1024] = np.nan, np.inf, -np.inf
    refused = [
        ("wcorr NULL", dict(h=None)), ("in NULL", dict(x=None)), ("corr NULL", dict(co=None)), ("pairs NULL", dict(pr=None)),
        ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)), ("no microphones", dict(n_mics=0)), ("no pairs", dict(n_pairs=0)),
        ("no windows", dict(n_windows=0)), ("n_in 0", dict(n_in=0)), ("window_len 0", dict(wl=0)), ("hop 0", dict(hop=0)),
        ("first past n_in", dict(first=NS + 1)), ("a window past n_in", dict(first=NS - 1537 - 1400 + 1)), ("hop too long", dict(hop=2400)),
        ("windows past n_in", dict(n_windows=8)), ("max_lag 0", dict(lag=0)), ("max_lag 513", dict(lag=513, guard=0)),
        ("max_lag + guard 513", dict(guard=313)), ("guard 2^32 - 1", dict(guard=2 ** 32 - 1)), ("a weight is NaN", dict(w=bad_w[0].ctypes.data)),
        ("a weight is infinite", dict(w=bad_w[1].ctypes.data)), ("the last weight is infinite", dict(w=bad_w[2].ctypes.data)),
        ("corr_stride < lags", dict(cs=400)), ("in_stride < n_in", dict(in_stride=NS - 1)), ("a pair's row >= n_mics", dict(pr=bad_pairs.ctypes.data)),
        ("n_mics too small for the pairs", dict(n_mics=1)), ("in_dev on the host", dict(x=host.ctypes.data)),
        ("corr_dev on the host", dict(co=other.data_ptr())), ("corr_dev overlaps in_dev", dict(co=dev.data_ptr() + 64)),
    ]
    for name, kw in refused:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc, L.uc_wcorr_last_error())
        assert L.uc_wcorr_last_error(), name
        assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    assert bool((corr == FILL).all())                                            # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    got = corr[:2 * nw * lags].reshape(2, nw, lags)
    assert torch.equal(got[0], corr0[0]) and torch.equal(got[1], corr0[0]) and bool((corr[2 * nw * lags:] == FILL).all())
    assert torch.equal(wc.windows(dev, PAIRS, **good), corr0)
    with pytest.raises(ValueError):
        wc.windows(dev, PAIRS, 0, 100, 0, 1, 8)
    with pytest.raises(ValueError):
        wc.windows(dev, PAIRS, 0, 100, 100, 1, 8, 0, np.ones(1024, np.float32))
    with pytest.raises(wcorr.WcorrError):
        wc.windows(dev, PAIRS, 0, 100, 100, 1, 400, 113)
    assert torch.equal(wc.windows(dev, PAIRS, **good), corr0)
    h2 = C.c_void_p()
    assert L.uc_wcorr_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_wcorr_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    wc.close()


def test_c_host_finds_the_delay_of_10_25_samples_at_minus_12_db(wcorr, tmp_path):
    import re
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [(float(a), float(b)) for a, b in re.findall(r"window +\d+: delay +(-?[0-9.]+) weighted, +(-?[0-9.]+) plain", out.stdout)]
    assert len(got) == 26
    weighted = sum(abs(a - 10.25) <= 1.0 for a, _ in got)
    plain = sum(abs(b - 10.25) <= 1.0 for _, b in got)
    print("windows within 1 sample of 10.25: %d weighted, %d plain" % (weighted, plain))
    assert weighted >= 8 and weighted >= plain
