"""The delay tracker on the GPU (uc_track_windows, uchirp/track.py): the correlations of every window bit for bit those
of `Xcorr.correlate` called per window, and within the header's error form of the float64 model; the same bits under every
way of dealing the work; crest records equal to `select_model` of the call's own correlations and finished records equal
to `xcorr.peak` of them; crafted correlations through the crest kernel alone; `track.drift` against `retime.drift` end to
end; the contract of the call; and a plain C host.  Every test prints its figures before it asserts (pytest -s).

Inputs: 4 rows of 3 x 2048 + 37 samples, the smallest rows at which a full group and one more sample fit at L >= 253."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

from test_track_cpu import build_host, crafted_rows, same_bits

pytestmark = pytest.mark.gpu

N = 2048
FS = 78125.0
NM = 4
NS = 3 * 2048 + 37
PAIRS = [(0, 1), (2, 2), (3, 0), (1, 0), (3, 3), (2, 1)]
LAGS = (1, 64, 65, 200, 511, 512)
GUARD = -7.5


@pytest.fixture(scope="module")
def track():
    from uchirp import track as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def xcorr():
    from uchirp import xcorr as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def mics(track):
    """4 microphones x (3 x 2048 + 37) samples: a message of amplitude 2000 at a lead of its own per microphone, plus noise
    (device tensor and host copy), and int32 words most of which are no floats (word 0 of every row is 0); made once and
    never written."""
    import torch
    from uchirp import scene
    rng = np.random.default_rng(26)
    lead = rng.uniform(0.0, 600.0, size=NM)
    x = scene.Scene().render(["Hi"], [(300.0, [(0, 2000.0, float(lead[m]), 0.0)]) for m in range(NM)], n_samples=NS, seed=8)
    h = x.cpu().numpy()
    assert np.abs(h).max() > 2000.0
    words = rng.integers(-2 ** 27, 2 ** 27, size=(NM, NS)).astype(np.int32)
    words[:, :8] = [0, 1, -1, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 77]
    return {"f32": (x, h), "i32": (torch.from_numpy(words).to("cuda:0"), words)}


def _cases(L):
    """(first, window_len, hop, n_windows): every window_len of the issue's list that fits, with every hop and every count
    of windows that fit, `first` taking 0, an odd value and the value at which the last window ends at n_in in turn"""
    S = 2048 - 2 * L
    out, turn = [], 0
    for wl in (1, S - 1, S, S + 1, 2048, 4 * S, 4 * S + 1):
        if wl > NS:
            continue
        for hop in (1, wl - 3, wl, wl + 5):
            if hop < 1:
                continue
            for nw in (1, 2, 3, 7):
                span = (nw - 1) * hop + wl
                if span > NS:
                    continue
                room = NS - span
                first = (0, min(room, 701) | 1 if room else 0, room)[turn % 3]
                if first > room:
                    first = room
                turn += 1
                out.append((first, wl, hop, nw))
    return out


def _guarded(torch, n_pairs, nw, lags):
    """a correlation buffer with three guard values behind every row: (the view to hand over, the whole buffer)"""
    whole = torch.full((n_pairs, nw, lags + 3), GUARD, dtype=torch.float64, device="cuda:0")
    return whole[:, :, :lags], whole


def _check_crests(track, xcorr, crest, corr, L, counts):
    """slots == select_model of the call's own doubles; finished records == xcorr.peak of them (or the row is excluded by
    the header's rule, which is counted)"""
    fin = track.finish(crest, L)
    for p in range(corr.shape[0]):
        for w in range(corr.shape[1]):
            want = track.select_model(corr[p, w])
            assert crest[p, w].tobytes() == want.tobytes(), (L, p, w, crest[p, w], want)
            counts["rows"] += 1
            counts["many"] += int(want["n_candidates"]) > track.SLOTS
            if track.excluded(corr[p, w], crest[p, w]):
                counts["excluded"] += 1
                continue
            assert same_bits(fin[p, w], xcorr.peak(corr[p, w])), (L, p, w)


@pytest.mark.parametrize("L", LAGS)
def test_windows_are_xcorr_per_window_and_crests_are_the_model(track, xcorr, mics, L):
    """Checks 1 and 3 of the issue over every case: correlations bit-equal to `Xcorr.correlate` per window on the same
    buffer, guard values untouched; for one case per window_len the error form against `windows_model`, and the crest
    records against `select_model` and `xcorr.peak`."""
    import torch
    tr, xc = track.Tracker(), xcorr.Xcorr()
    lags = 2 * L + 1
    cases = _cases(L)
    counts = {"rows": 0, "many": 0, "excluded": 0}
    worst = 0.0
    seen_wl = set()
    for name in ("f32", "i32"):
        dev, host = mics[name]
        xs = torch.zeros((NM, NS + 131), dtype=dev.dtype, device="cuda:0")[:, 3:3 + NS]      # strided rows with an odd pitch
        xs.copy_(dev)
        for i, (first, wl, hop, nw) in enumerate(cases):
            src = xs if i % 4 == 3 else dev
            view, whole = _guarded(torch, len(PAIRS), nw, lags)
            crest, corr = tr.windows(src, PAIRS, first, wl, hop, nw, L, corr=view)
            assert corr is view
            want = torch.stack([xc.correlate(dev, PAIRS, first=first + w * hop, n=wl, max_lag=L) for w in range(nw)], dim=1)
            assert torch.equal(view, want), (name, L, first, wl, hop, nw)
            assert bool((whole[:, :, lags:] == GUARD).all()), (name, L, first, wl, hop, nw)
            if (name, wl) not in seen_wl or (first, wl, hop, nw) == cases[-1]:
                seen_wl.add((name, wl))
                got = view.cpu().numpy()
                model = track.windows_model(host, PAIRS, first, wl, hop, nw, L)
                E = track.windows_model(host, PAIRS, first, wl, hop, nw, L, magnitude=True)
                zero = E == 0
                assert (got[zero] == 0).all()
                if not zero.all():
                    ratio = float((np.abs(got - model)[~zero] / (2.0 ** -24 * E[~zero, None])).max())
                    worst = max(worst, ratio)
                    assert ratio <= track.ERROR_C, (name, L, first, wl, hop, nw, ratio)
                _check_crests(track, xcorr, track.crests(crest), got, L, counts)
    print("L %3d: %d cases x 2 formats bit-equal to Xcorr.correlate per window; worst |gpu - model| / (2^-24 E) %.3f (bar %d); %d crest "
          "records equal select_model, %d of them from more than %d candidates, %d excluded"
          % (L, len(cases), worst, track.ERROR_C, counts["rows"], counts["many"], track.SLOTS, counts["excluded"]))
    assert counts["excluded"] == 0 and counts["rows"] >= 60
    tr.close()
    xc.close()


def test_case_list_covers_what_the_issue_names():
    for L in LAGS:
        S = 2048 - 2 * L
        cases = _cases(L)
        wls = {c[1] for c in cases}
        assert {1, S - 1, S, S + 1, 2048} <= wls and ((4 * S in wls and 4 * S + 1 in wls) == (4 * S + 1 <= NS))
        assert {c[3] for c in cases} == {1, 2, 3, 7}
        for wl in wls - {1}:
            hops = {c[2] for c in cases if c[1] == wl}
            assert {1, wl} <= hops and (wl <= 3 or wl - 3 in hops) and wl + 5 in hops, (L, wl, hops)
        assert any(c[0] == 0 for c in cases) and any(c[0] % 2 == 1 for c in cases)
        assert any(c[0] + (c[3] - 1) * c[2] + c[1] == NS and c[0] > 0 for c in cases)
        assert any(c[3] > 1 and c[2] < c[1] for c in cases) and any(c[3] > 1 and c[2] > c[1] for c in cases)
    assert 4097 in {c[1] for c in _cases(512)} and 4105 in {c[1] for c in _cases(511)}


def test_the_same_bits_however_the_work_is_dealt(track, mics, monkeypatch):
    """Check 2: grids of 1-5 workgroups and the default, calls in a row, the pairs in another order, a pair alone, a window
    alone, corr_dev NULL against given; a reference window of zeros."""
    import torch
    tr = track.Tracker()
    for name, L, first, wl, hop, nw in (("f32", 200, 3, 1649, 700, 7), ("i32", 512, 1, 4097, 1000, 3), ("i32", 64, 0, 2048, 2048, 3),
                                        ("f32", 1, 5, 2045, 1, 7)):
        dev, _ = mics[name]
        lags = 2 * L + 1
        crest0, corr0 = tr.windows(dev, PAIRS, first, wl, hop, nw, L, corr=True)
        for g in (1, 2, 3, 4, 5):
            monkeypatch.setenv("UC_TUNING", "1")
            monkeypatch.setenv("UC_TRACK_GRID", str(g))
            tg = track.Tracker()
            monkeypatch.delenv("UC_TUNING")
            monkeypatch.delenv("UC_TRACK_GRID")
            for _ in range(3):                                               # both staging slots, and the first one again
                view, whole = _guarded(torch, len(PAIRS), nw, lags)
                crest = tg.windows(dev, PAIRS, first, wl, hop, nw, L, corr=view)[0]
                assert torch.equal(view, corr0) and torch.equal(crest, crest0), (name, L, g)
                assert bool((whole[:, :, lags:] == GUARD).all())
            tg.close()
        order = [4, 0, 5, 2, 1, 3]
        crest, corr = tr.windows(dev, [PAIRS[i] for i in order], first, wl, hop, nw, L, corr=True)
        assert torch.equal(corr, corr0[order]) and torch.equal(crest, crest0[order])
        for i in (0, 1, 5):
            crest, corr = tr.windows(dev, [PAIRS[i]], first, wl, hop, nw, L, corr=True)
            assert torch.equal(corr[0], corr0[i]) and torch.equal(crest[0], crest0[i])
        for w in range(nw):
            crest, corr = tr.windows(dev, PAIRS, first + w * hop, wl, hop, 1, L, corr=True)
            assert torch.equal(corr[:, 0], corr0[:, w]) and torch.equal(crest[:, 0], crest0[:, w])
        assert torch.equal(tr.windows(dev, PAIRS, first, wl, hop, nw, L), crest0)                       # corr_dev NULL
        assert torch.equal(tr.windows(dev, PAIRS, first, wl, hop, nw, L, corr=True, crest=False), corr0)   # crest_dev NULL
    words, _ = mics["i32"]
    crest, corr = tr.windows(words, PAIRS, 0, 1, 1, 1, 512, corr=True)        # word 0 of every row is 0
    rec = track.crests(crest)
    assert bool((corr == 0).all()) and (rec["flags"] == track.NO_PEAK | track.AT_EDGE).all() and (rec["n_candidates"] == 0).all()
    assert (rec["slot"]["k"] == -1).all() and (rec["slot"]["r"] == 0).all()
    assert (track.finish(rec, 512)["flags"] == track.NO_PEAK | track.AT_EDGE).all()
    tr.close()


def test_crafted_correlations_through_the_crest_kernel(track, xcorr, mics, monkeypatch):
    """Check 3, third item: under UC_TUNING=1 and UC_TRACK_CRESTS_OF_CORR=1 a tracker READS corr_dev and runs the crest kernel
    alone.  Rows without a candidate, with one, with the best at either end, with the largest sample at an edge, with c
    outside (-1, 1), with exact ties, with more than four candidates, with values that are not finite."""
    import torch
    monkeypatch.setenv("UC_TUNING", "1")
    monkeypatch.setenv("UC_TRACK_CRESTS_OF_CORR", "1")
    tr = track.Tracker()
    monkeypatch.delenv("UC_TUNING")
    monkeypatch.delenv("UC_TRACK_CRESTS_OF_CORR")
    dev, _ = mics["f32"]
    rows = crafted_rows()
    base = dict(rows)["more than four candidates"]
    for at, v in ((0, np.nan), (80, np.inf), (17, -np.inf), (63, np.nan), (64, np.inf)):
        bad = base.copy()
        bad[at] = v
        rows.append(("not finite at %d" % at, bad))
    w = 2.0 * np.pi / 4.46
    k = np.arange(-512, 513, dtype=np.float64)
    rows.append(("no candidate, the largest sample inside", -1.0 - np.arange(-40.0, 41.0) ** 2))
    rows.append(("1025 lags, crests of one height class", 1e9 * np.cos(w * (k - 0.37)) * (1.0 + 1e-9 * k)))
    rows.append(("1025 lags, an envelope", 1e9 * np.cos(w * (k + 401.2)) * np.exp(-0.5 * ((k + 401.2) / 11.0) ** 2)))
    flags = set()
    many = 0
    for name, row in rows:
        L = (len(row) - 1) // 2
        corr = torch.from_numpy(np.ascontiguousarray(row, np.float64)).to("cuda:0").reshape(1, 1, -1)
        keep = corr.clone()
        rec = track.crests(tr.windows(dev, [(0, 1)], 0, 16, 16, 1, L, corr=corr)[0])[0, 0]
        assert torch.equal(corr.view(torch.int64), keep.view(torch.int64)), name          # read, not written
        want = track.select_model(row)
        assert rec.tobytes() == want.tobytes(), (name, rec, want)
        flags.add(int(rec["flags"]))
        many += int(rec["n_candidates"]) > track.SLOTS
        if rec["flags"] & track.NOT_FINITE:
            with pytest.raises(track.TrackError):
                track.finish(rec, L)
        else:
            assert not track.excluded(row, rec), name
            assert same_bits(track.finish(rec, L), xcorr.peak(row)), name
    print("%d crafted rows through the crest kernel: flags seen %r, %d rows with more than %d candidates" % (len(rows), sorted(flags), many, track.SLOTS))
    assert {0, track.NO_PEAK, track.AT_EDGE, track.NO_PEAK | track.AT_EDGE, track.NOT_FINITE} <= flags and many >= 10
    # several rows in one call: [2 pairs, 3 windows] of strided rows
    six = np.stack([r for n, r in rows if len(r) == 81][:6]).reshape(2, 3, 81)
    whole = torch.full((2, 3, 90), GUARD, dtype=torch.float64, device="cuda:0")
    whole[:, :, :81] = torch.from_numpy(six).to("cuda:0")
    rec = track.crests(tr.windows(dev, [(0, 1), (2, 3)], 0, 16, 16, 3, 40, corr=whole[:, :, :81])[0])
    for p in range(2):
        for w_ in range(3):
            assert rec[p, w_].tobytes() == track.select_model(six[p, w_]).tobytes()
    tr.close()


def test_drift_with_one_call_per_pass_gives_the_lines_of_the_loop(track, xcorr):
    """Check 4.  2 arrays of 4 at +14 dB, 104 blocks, ppm uniform in +-50, leads within +-30 samples: `track.drift` returns
    exactly the lines (and fits) of `retime.drift` over `Xcorr`, both at L = 128; and both meet the bars of DESIGN.md section
    14 against the scene's truth: every slope within 1 ppm, every delay at the transmission's centre within 0.01 samples."""
    from uchirp import link, retime, scene
    na, nm, nb, amp = 2, 4, 104, 2000.0
    rng = np.random.default_rng(16)
    text = "Hello, World"
    lead = 4000.0 + 500.0 * np.arange(na)[:, None] + rng.uniform(-30.0, 30.0, size=(na, nm))
    ppm = rng.uniform(-50.0, 50.0, size=(na, nm)).astype(np.float32).astype(np.float64)          # struct uc_scene_path holds a float
    sigma = amp / 10.0 ** (14.0 / 20.0)
    x = scene.Scene().render([text] * na, [(sigma, [(a, amp, float(lead[a, m]), float(ppm[a, m]))]) for a in range(na) for m in range(nm)],
                             n_samples=nb * N, seed=44)
    arrays = [[a * nm + m for m in range(nm)] for a in range(na)]
    rt, xc, tr = retime.Retimer(), xcorr.Xcorr(), track.Tracker()
    lines, fits = track.drift(x, arrays, tr, max_lag=128, retimer=rt)
    lines_loop, fits_loop = retime.drift(x, arrays, xc, max_lag=128, retimer=rt)
    worst = {"track": [0.0, 0.0], "loop": [0.0, 0.0]}
    for a in range(na):
        sounding = np.nonzero(link.signal(text, lead[a, 0], amp, ppm[a, 0], nb * N, FS))[0]
        centre = 0.5 * (sounding[0] + sounding[-1])
        for m in range(1, nm):
            i = a * nm + m
            d, s = retime.undo(lead[a, m], ppm[a, m], lead[a, 0], ppm[a, 0])
            for key, ln in (("track", lines[i]), ("loop", lines_loop[i])):
                worst[key][0] = max(worst[key][0], abs(ln[2] - s) * 1e6)
                worst[key][1] = max(worst[key][1], abs((ln[1] + ln[2] * centre) - (d + s * centre)))
    print("drift, +14 dB, %d arrays of %d, L = 128, %d windows: one tracker call per pass: worst |slope - truth| %.4f ppm, worst |delay - truth| "
          "at the centre %.4f samples; the loop over Xcorr.delays: %.4f ppm, %.4f samples; fewest windows kept %d"
          % (na, nm, fits[1]["windows"], worst["track"][0], worst["track"][1], worst["loop"][0], worst["loop"][1],
             min(f["kept"] for f in fits if f)))
    assert lines == lines_loop, (lines, lines_loop)
    assert fits == fits_loop
    for key in ("track", "loop"):
        assert worst[key][0] <= 1.0 and worst[key][1] <= 0.01, (key, worst[key])
    for o in (rt, xc, tr):
        o.close()


def test_contract_of_the_call(track, mics):
    """Check 5: every refused argument returns -EINVAL with a text and enqueues nothing; the next good call gives the right
    bits; the caller's device and the object survive."""
    import torch
    L = track.lib()
    tr = track.Tracker()
    dev, _ = mics["f32"]
    dev0 = torch.cuda.current_device()
    good = dict(first=3, window_len=1649, hop=700, n_windows=3, max_lag=200)
    crest0, corr0 = tr.windows(dev, PAIRS, corr=True, **good)
    torch.cuda.synchronize()
    pairs = np.zeros(2, track.PAIR_DTYPE)
    pairs["mic"] = 1
    lags, nw = 401, 3
    corr = torch.full((2 * nw * lags + 64,), GUARD, dtype=torch.float64, device="cuda:0")
    crest = torch.zeros((2 * nw * track.CREST_BYTES + 64,), dtype=torch.uint8, device="cuda:0")
    host = np.zeros(1 << 16, np.float64)
    other = torch.zeros(8, dtype=torch.float64)                                  # host memory

    def call(h=tr._h, x=dev.data_ptr(), dtype=1, n_mics=NM, n_in=NS, in_stride=NS, pr=pairs.ctypes.data, n_pairs=2, first=3, wl=1649, hop=700,
             n_windows=nw, lag=200, co=corr.data_ptr(), cs=0, cr=crest.data_ptr()):
        return L.uc_track_windows(h, x, dtype, n_mics, n_in, in_stride, pr, n_pairs, first, wl, hop, n_windows, lag, co, cs, cr, None)

    bad_pairs = pairs.copy()
    bad_pairs[1]["ref"] = NM
    refused = [
        ("track NULL", dict(h=None)), ("in NULL", dict(x=None)), ("both outputs NULL", dict(co=None, cr=None)), ("pairs NULL", dict(pr=None)),
        ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)), ("no microphones", dict(n_mics=0)), ("no pairs", dict(n_pairs=0)),
        ("no windows", dict(n_windows=0)), ("n_in 0", dict(n_in=0)), ("window_len 0", dict(wl=0)), ("hop 0", dict(hop=0)),
        ("first past n_in", dict(first=NS + 1)), ("a window past n_in", dict(first=NS - 1649 - 1400 + 1)), ("hop too long", dict(hop=2300)),
        ("windows past n_in", dict(n_windows=8, co=None)), ("max_lag 0", dict(lag=0)), ("max_lag 513", dict(lag=513)),
        ("corr_stride < lags", dict(cs=400)), ("in_stride < n_in", dict(in_stride=NS - 1)), ("a pair's row >= n_mics", dict(pr=bad_pairs.ctypes.data)),
        ("n_mics too small for the pairs", dict(n_mics=1)), ("in_dev on the host", dict(x=host.ctypes.data)),
        ("corr_dev on the host", dict(co=other.data_ptr())), ("crest_dev on the host", dict(cr=host.ctypes.data)),
        ("corr_dev overlaps in_dev", dict(co=dev.data_ptr() + 64)), ("crest_dev overlaps in_dev", dict(cr=dev.data_ptr() + 4 * NS)),
        ("crest_dev overlaps corr_dev", dict(cr=corr.data_ptr() + 8 * 100)),
        ("crest_dev overlaps a strided corr_dev", dict(co=corr.data_ptr(), cs=lags + 10, cr=corr.data_ptr() + 8 * (2 * nw * lags + 20))),
    ]
    for name, kw in refused:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc, L.uc_track_last_error())
        assert L.uc_track_last_error(), name
        assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    assert bool((corr == GUARD).all()) and bool((crest == 0).all())                # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    got = corr[:2 * nw * lags].reshape(2, nw, lags)
    assert torch.equal(got[0], corr0[0]) and torch.equal(got[1], corr0[0]) and bool((corr[2 * nw * lags:] == GUARD).all())
    assert torch.equal(crest[:2 * nw * track.CREST_BYTES].reshape(2, nw, -1)[1], crest0[0]) and bool((crest[2 * nw * track.CREST_BYTES:] == 0).all())
    crest1, corr1 = tr.windows(dev, PAIRS, corr=True, **good)
    assert torch.equal(corr1, corr0) and torch.equal(crest1, crest0)
    with pytest.raises(ValueError):
        tr.windows(dev, PAIRS, 0, 100, 0, 1, 8)
    with pytest.raises(ValueError):
        tr.windows(dev, PAIRS, 0, 100, 100, 1, 8, crest=False)
    with pytest.raises(track.TrackError):
        tr.windows(dev, PAIRS, 0, 100, 100, 1, 513)
    h2 = C.c_void_p()
    assert L.uc_track_create(torch.cuda.device_count(), C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_track_create(0, None) == -errno.EINVAL
    assert torch.cuda.current_device() == dev0
    tr.close()


def test_delays_have_the_shape_of_xcorr_delays_per_window(track, xcorr, mics):
    dev, _ = mics["f32"]
    tr, xc = track.Tracker(), xcorr.Xcorr()
    arrays = [[0, 1, 2], [3, 0]]
    delays, peaks = tr.delays(dev, arrays, first=5, window_len=2048, hop=1500, n_windows=3, max_lag=300)
    for w in range(3):
        d, p = xc.delays(dev, arrays, first=5 + 1500 * w, n=2048, max_lag=300)
        for a in range(2):
            assert [delays[a][m][w] for m in range(len(arrays[a]))] == d[a]
            assert peaks[a][0] is None and p[a][0] is None
            for m in range(1, len(arrays[a])):
                assert same_bits(peaks[a][m][w], p[a][m])
    rec = tr.peaks(dev, [(0, 1)], 5, 2048, 1500, 3, 300)
    assert rec.shape == (1, 3) and rec.dtype == track.PEAK_DTYPE and rec["delay_samples"][0, 1] == delays[0][1][1]
    tr.close()
    xc.close()


def test_c_host_tracks_a_delay_of_97_5_samples(track, tmp_path):
    import re
    exe = build_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [(float(d), int(f)) for d, f in re.findall(r"window +\d+: delay +(-?[0-9.]+) .*flags (\d+)", out.stdout)]
    assert len(got) == 26
    near = [d for d, f in got if f == 0 and abs(d - 97.5) <= 0.05]
    assert len(near) >= 8, got
