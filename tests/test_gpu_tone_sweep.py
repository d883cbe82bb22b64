"""Tone sweeps: a peak through every window bin of every band and I/Q frame-kernel build.

The parity tests feed the frame kernels the modem's own chirps, so the maximum sits on the same two or three bins of
the window in every frame and every other bin only ever has to stay below it.  Here every bin of both windows is, in
some frame, the CLEAR maximum (tests/tone_sweep_util.py; proven on the float64 oracle alone by
tests/test_tone_sweep_cpu.py), so that the bin's own lane, twiddle and place in the first-max search decide a record.

Per case, float32 samples and int32 DFSDM words:
  1. the usual bars on every history (tests/parity_util.py): magnitudes within MAG_TOL x the frame's window maximum,
     every index mismatch a proven near-tie -- check_history as it stands for the real transforms (RX_REAL,
     DECHIRP_DOWN: both windows hold the tone); for the one-sided spectra of SYNC_CPLX and I/Q the near-tie is
     measured in the same unit as the magnitudes, MAG_TOL x the frame's largest window magnitude
     (tone_sweep_util.prove_near_ties: the window across DC from a clean tone holds leakage 1e-6 of it);
  2. wherever the oracle's window winner is clear (second <= 0.99 x first, in a window that holds signal:
     tone_sweep_util.SIGNAL) the GPU's max_freq_left / max_freq_right is the oracle's EXACTLY, and max_freq too where
     the two window maxima differ by more than 1 % (both sides are within MAG_TOL = 2e-5 of the maximum: an error
     inside the bar cannot overturn a lead of 500 bars);
  3. every bin of the coverage set is reached by such an exact comparison (counted);
  4. the same batch with the frames in a fixed permutation: bit-identical records, frame by frame.  DECHIRP_DOWN
     transforms frames (2u, 2u + 1) in one complex FFT and a frame's float32 round-off depends on its partner
     (include/uchirp.h; tests/test_gpu_parity.py::test_dechirp_down_frame_pairs_...): there the PAIRS are permuted for
     the bit comparison, and a permutation of the frames -- other partners -- goes through 1 - 3 again;
  5. the same batch under UC_GRID=1 with groups of 2 (one workgroup walks every ring slot): the same bits.

The band kernel is swept at the seams of its window search too (tone_sweep_util.SEAM_WIDTHS: the widths at which bin bandwidth2
changes its owner), float32 at every width and int32 where the owner changes; test_edge_frames_at_the_seams adds the all-zero
and all-NaN frames there, whose answer is the edge-bin owner's alone.

The parametrize ids name the kernel instantiation a case reaches (csrc/uc_band_kernel.hip: UC_DISPATCH,
csrc/uc_iq_kernel.hip: UC_IQ_DISPATCH); the geometry that selects it is asserted.  `pytest -s` prints the figures."""
import numpy as np
import pytest

from oracle import uco
from parity_util import MAG_TOL, check_history, check_magnitudes, clear_symbols, window_scale
import tone_sweep_util as tsu

pytestmark = pytest.mark.gpu

VARIANT = {"rx_real": uco.RX_REAL, "sync_cplx": uco.SYNC_CPLX, "dechirp_down": uco.DECHIRP_DOWN, "iq": uco.IQ}
MFMA = {"UC_IQ_FIR": "mfma"}

# (id = the instantiation reached, case, environment under UC_TUNING=1, stride or None)
BUILDS = [
    # band kernel, batch build <MODE, DTYPE, WAVES>: every occupancy UC_BAND_WAVES offers
    ("band<RxReal,W2>", "rx_real-literal", {"UC_BAND_WAVES": "2"}, None),
    ("band<RxReal,W3>", "rx_real-literal", {"UC_BAND_WAVES": "3"}, None),
    ("band<RxReal,W4>", "rx_real-literal", {"UC_BAND_WAVES": "4"}, None),
    ("band<RxReal,W3>-matched", "rx_real-matched", {}, None),
    ("band<Cplx,W2>", "sync_cplx-literal", {"UC_BAND_WAVES": "2"}, None),
    ("band<Cplx,W3>", "sync_cplx-literal", {"UC_BAND_WAVES": "3"}, None),
    ("band<Cplx,W4>", "sync_cplx-literal", {"UC_BAND_WAVES": "4"}, None),
    ("band<Cplx,W2>-matched", "sync_cplx-matched", {}, None),
    ("band<Pair,W3>", "dechirp_down-default", {}, None),
    # band kernel, overlap build <.., kFramesOverlap>: any stride < 2048
    ("band<RxReal,W3,Overlap>", "rx_real-literal", {}, 2047),
    ("band<Cplx,W2,Overlap>", "sync_cplx-literal", {}, 2047),
    # band kernel, WIDE build <MODE, DTYPE, 2, WIDE>
    ("band<RxReal,W2,WIDE>-294", "rx_real-wide294", {}, None),
    ("band<RxReal,W2,WIDE>-318", "rx_real-wide318", {}, None),
    ("band<Cplx,W2,WIDE>-294", "sync_cplx-wide294", {}, None),
    ("band<Cplx,W2,WIDE>-318", "sync_cplx-wide318", {}, None),
    ("band<Pair,W2,WIDE>-240", "dechirp_down-wide240", {}, None),
    ("band<Pair,W2,WIDE>-312", "dechirp_down-wide312", {}, None),
    # iq_kernel<DTYPE, BB> (n 2048) and iq1024_kernel<DTYPE, BB, FIRM>
    ("iq<BB0>", "iq2048-bb0", {}, None),
    ("iq<BB1>", "iq2048-bb1", {}, None),
    ("iq<BB2>", "iq2048-bb2", {}, None),
    ("iq1024<BB0,FIRM0>", "iq1024-bb0", {}, None),
    ("iq1024<BB1,FIRM0>", "iq1024-bb1", {}, None),
    ("iq1024<BB2,FIRM0>", "iq1024-bb2", {}, None),
    ("iq1024<BB0,FIRM1>", "iq1024-bb0", MFMA, None),
    ("iq1024<BB1,FIRM1>", "iq1024-bb1", MFMA, None),
    ("iq1024<BB1,FIRM1>-narrow", "iq1024-bb2", MFMA, None),     # with the flag set the narrow geometry goes to <.., 1, 1> too
]
# band kernel at the seams of its window search (tone_sweep_util.SEAM_WIDTHS): the widths at which bin bandwidth2 changes its
# owner, wave 1 loses its common bins, the third round of the WIDE build gets its first bin
_DEFAULT = {"rx_real": "band<RxReal,W3>-w%d", "sync_cplx": "band<Cplx,W2>-w%d", "dechirp_down": "band<Pair,W3>-w%d"}
_WIDE = {"rx_real": "band<RxReal,W2,WIDE>-%d", "sync_cplx": "band<Cplx,W2,WIDE>-%d", "dechirp_down": "band<Pair,W2,WIDE>-%d"}
SEAM_BUILDS = [((_WIDE if w > 191 else _DEFAULT)[kind] % w, tsu.seam_name(kind, w), {}, None)
               for kind, widths in tsu.SEAM_WIDTHS.items() for w in widths]
BUILDS += SEAM_BUILDS
SEAM_INT32 = (64, 128, 192, 256)        # the word type changes the load alone: int32 where the owner of bin bandwidth2 changes
SWEEPS = [pytest.param(*b, dtype, id="%s-%s" % (b[0], dtype)) for b in BUILDS for dtype in ("float32", "int32")
          if dtype == "float32" or b not in SEAM_BUILDS or tsu.CASES[b[1]][3]["bw2"] in SEAM_INT32]


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


def _engine(uchirp, monkeypatch, name, dtype, env):
    variant, cfg = tsu.config(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = uchirp.Engine(variant, mag_mean=1000.0 * (256 if dtype == "int32" else 1), **cfg)
    for k in env:
        monkeypatch.delenv(k)
    return e


def _assert_geometry(e, o, name, env, stride):
    """The numbers the dispatchers select the instantiation by."""
    kind, cfg, recipe, geo = tsu.CASES[name]
    assert (e.n, e.bandwidth, e.bandwidth2, e.idx_left_zero) == (o.n, o.bandwidth, o.bandwidth2, o.idx_left_zero)
    assert e.bandwidth2 == geo["bw2"]
    if kind == "iq":
        assert e.n == cfg["n"] and e.halo == tsu.HALO
        if recipe == "iq_bb":
            narrow = e.bandwidth2 <= (32 if e.n == 1024 else 64)
            assert narrow == name.endswith("bb2") and e.spf == 2
        else:
            assert e.spf == 1
    else:
        assert e.n == 2048
        assert (e.bandwidth2 > 191) == ("wide" in name)
        assert stride is None or (stride < 2048 and e.bandwidth2 <= 191 and kind != "dechirp_down" and not env)


def _against_the_oracle(sw, gs, gst, label):
    """1 - 3 of the module's docstring; prints the figures before it asserts."""
    o, rst = sw.o, sw.records
    worst = 0.0
    for h in range(o.spf):
        scale = window_scale(rst[:, h])
        for fld in ("mag_max", "mag_max_left", "mag_max_right"):
            worst = max(worst, float(np.max(np.abs(gst[:, h][fld].astype(np.float64) - rst[:, h][fld].astype(np.float64)) / scale)))
    hit, count, bad = set(), 0, []
    for h in range(o.spf):
        hh, c, b = tsu.exact_comparisons(sw, gst[:, h], h)
        hit |= hh
        count += c
        bad += b
    cov = sw.coverage()
    print("%-44s %5d frames  worst |gpu - oracle| / (MAG_TOL x window max) %.3f  exact comparisons %5d on %3d of %3d window "
          "bins, %d wrong" % (label, sw.n_frames, worst / MAG_TOL, count, len(hit), len(sw.whole()), len(bad)), end="")
    ties = 0
    try:
        for h in range(o.spf):
            if sw.real_spectrum:       # both windows hold the tone: parity_util's rule as it stands
                ties += check_history(o, sw.frame, gst[:, h], rst[:, h], h, "%s hist%d" % (label, h), raw_idx=sw.raw_idx)
            else:
                check_magnitudes(gst[:, h], rst[:, h], "%s hist%d" % (label, h))
                ties += tsu.prove_near_ties(sw, gst[:, h], h, MAG_TOL, "%s hist%d" % (label, h))
            assert np.array_equal(gst[:, h]["mag_mean"], rst[:, h]["mag_mean"])
    finally:
        print("  near-ties proven %d" % ties)
    assert not bad, "%s: %d exact comparisons fail, first (history, frame, field, gpu, oracle): %r" % (label, len(bad), bad[:8])
    assert hit == cov and count >= len(cov)
    if sw.firmware:
        assert len(cov) >= 0.85 * len(sw.whole())
    else:
        assert cov == sw.whole()
    if o.spf == 2:
        clear = clear_symbols(rst)
        assert np.array_equal(gs[clear], sw.symbols[clear]), label
    else:
        assert (gs == 0xFF).all()


@pytest.mark.parametrize("build,name,env,stride,dtype", SWEEPS)
def test_tone_sweep(uchirp, monkeypatch, uc_tuning, build, name, env, stride, dtype):
    sw, _ = tsu.sweep(name, dtype, stride)
    o = sw.o
    if stride is not None:
        assert o.table(uco.TABLE_HANN)[0] == 0.0      # the sample two overlapping frames share counts for nothing
    e = _engine(uchirp, monkeypatch, name, dtype, env)
    _assert_geometry(e, o, name, env, stride)
    paired = tsu.CASES[name][0] == "dechirp_down"
    label = "%s %s %s" % (build, name, dtype)
    gs, gst = e.process(sw.buf, n_frames=sw.n_frames, stride=sw.stride)
    _against_the_oracle(sw, gs, gst, label)
    # 4. a fixed permutation of the frames (DECHIRP_DOWN: of the pairs): bit-identical records, frame by frame
    _, pbuf, nf, st, _, order = tsu.batch(name, dtype, stride, "pairs" if paired else "frames")
    ps, pst = e.process(pbuf, n_frames=nf, stride=st)
    assert (order != np.arange(nf)).mean() > 0.9
    assert np.array_equal(ps, gs[order]), label
    assert np.array_equal(pst.view(np.uint32), gst[order].view(np.uint32)), label
    if paired:      # other partners in the shared transform: the oracle's bars and the exact rule again
        swp, _ = tsu.sweep(name, dtype, stride, "frames")
        qs, qst = e.process(swp.buf, n_frames=swp.n_frames, stride=swp.stride)
        _against_the_oracle(swp, qs, qst, label + " (other partners)")
    # 5. one workgroup, groups of 2: every ring slot, the hand-out over many groups -- the same bits
    e1 = _engine(uchirp, monkeypatch, name, dtype, dict(env, UC_GRID="1", UC_BAND_GROUP="2", UC_IQ_GROUP="2"))
    ts, tst = e1.process(sw.buf, n_frames=sw.n_frames, stride=sw.stride)
    assert np.array_equal(ts, gs), label
    assert np.array_equal(tst.view(np.uint32), gst.view(np.uint32)), label
    e.close()
    e1.close()


def _loudest_left_edge(sw):
    """The frame of a sweep whose tone is the clear winner on the left window's FIRST element (bin bandwidth2) and largest there."""
    edge = sw.windows["left"][0]
    on = [f for f in range(sw.n_frames) for h in range(sw.o.spf) if sw.clear["left"][h, f] and sw.win["left"][h, f] == edge]
    assert on
    return max(on, key=lambda f: float(sw.records[f]["mag_max_left"].max()))


@pytest.mark.parametrize("env", [{}, {"UC_GRID": "1", "UC_BAND_GROUP": "2"}], ids=["default", "grid1-group2"])
@pytest.mark.parametrize("build,name", [(b[0], b[1]) for b in SEAM_BUILDS], ids=[b[0] for b in SEAM_BUILDS])
def test_edge_frames_at_the_seams(uchirp, monkeypatch, uc_tuning, build, name, env):
    """All-zero and all-NaN frames at every seam width, by the rule of test_gpu_wide.py::test_wide_edge_frames_and_peaks_in_every_
    round: magnitudes and snr equal to the oracle's or both NaN, the three indices and the symbol equal.  In a zero frame every
    bin ties and arm_max_f32 keeps the FIRST element of each window: bin 0 on the right, bin bandwidth2 on the left -- the answer
    of the one thread that owns that bin, whichever wave and slot the width puts it in.

    Frames 0, 1 zero, 2 NaN, 3 zero, 4 noise, 5 zero; behind them the sweep's loudest tone on bin bandwidth2, a zero frame, and
    one more zero frame: with groups of 2 the ring slots alternate, so that this last one sits in the slot the loud frame wrote
    last.  DECHIRP_DOWN transforms frames (2u, 2u + 1) together: the loud frame, the zero frame and the one more are pairs of
    their own there, and only zero frames whose partner is zero are compared."""
    sw, _ = tsu.sweep(name)
    o, n = sw.o, sw.o.n
    paired = tsu.CASES[name][0] == "dechirp_down"
    loud = sw.frame(_loudest_left_edge(sw)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    x = [zero, zero, np.full(n, np.nan, np.float32), zero,
         (1000.0 * np.random.default_rng(1).standard_normal(n)).astype(np.float32), zero]
    if paired:
        x += [loud, loud, zero, zero, zero, zero]
        check = (0, 1, 8, 9, 10, 11)
    else:
        x += [loud, zero, zero]
        check = (0, 1, 2, 3, 5, 7, 8)
    x = np.stack(x)
    e = _engine(uchirp, monkeypatch, name, "float32", env)
    _assert_geometry(e, o, name, {}, None)
    rs, rst = o.process(x)
    gs, gst = e.process(x)
    loud_at = 6
    assert rst[loud_at]["mag_max_left"].max() > 1e4      # what a stale edge word would hold
    for f in check:
        for h in range(o.spf):
            if not np.isnan(x[f]).any():                 # the oracle's answer is the first element of each window
                assert rst[f, h]["mag_max"] == 0.0 and rst[f, h]["max_freq_right"] == sw.record_of_bin("right", 0)
                assert rst[f, h]["max_freq_left"] == sw.record_of_bin("left", sw.windows["left"][0])
            for fld in ("mag_max", "mag_max_left", "mag_max_right", "snr"):
                a, b = float(gst[f, h][fld]), float(rst[f, h][fld])
                assert (np.isnan(a) and np.isnan(b)) or a == b, (build, f, h, fld, a, b)
            for fld in ("max_freq", "max_freq_left", "max_freq_right"):
                assert gst[f, h][fld] == rst[f, h][fld], (build, f, h, fld, int(gst[f, h][fld]), int(rst[f, h][fld]))
        assert gs[f] == rs[f], (build, f)
    print("%-32s %-12s %d frames: %d zero / NaN frames x %d histories equal the oracle's in 7 fields and the symbol; the loud frame's "
          "left edge %.4g" % (build, "+".join("%s=%s" % kv for kv in env.items()) or "default", len(x), len(check), o.spf,
                              float(rst[loud_at]["mag_max_left"].max())))
    e.close()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("build,name,env", [("iq1024<BB1,FIRM0>", "iq1024-bb1", {}), ("iq<BB1>", "iq2048-bb1", {}),
                                            ("iq1024<BB1,FIRM1>", "iq1024-bb1", MFMA)],
                         ids=["iq1024<BB1,FIRM0>", "iq<BB1>", "iq1024<BB1,FIRM1>"])
def test_noisy_stream_on_the_least_compared_builds(uchirp, monkeypatch, uc_tuning, build, name, env, dtype):
    """The 200-frame -10 dB stream of test_baseband_noisy_stream_matches_oracle_and_decodes in the geometry just past
    the narrow builds (BB = 1) and with the FIR on the matrix pipe (FIRM = 1): the same assertions."""
    n_frames = 200
    x, bits, o = tsu.noisy_stream(name, dtype, n_frames)
    e = _engine(uchirp, monkeypatch, name, dtype, env)
    _assert_geometry(e, o, name, env, None)
    n, k = o.n, (256 if dtype == "int32" else 1)
    mm = (np.random.default_rng(n).uniform(500.0, 2000.0, size=(n_frames, 2)) * k).astype(np.float32)
    for mag_mean in (None, mm):
        rs, rst = o.process(x, halo=tsu.HALO, n_frames=n_frames, mag_mean=mag_mean)
        gs, gst = e.process(x, n_frames=n_frames, mag_mean=mag_mean)
        clear = clear_symbols(rst)
        worst = max(float(np.max(np.abs(gst[:, h][fld].astype(np.float64) - rst[:, h][fld].astype(np.float64)) / window_scale(rst[:, h])))
                    for h in (0, 1) for fld in ("mag_max", "mag_max_left", "mag_max_right"))
        print("%-44s %5d frames  worst |gpu - oracle| / (MAG_TOL x window max) %.3f  clear symbols %d, decoded %.3f"
              % ("%s %s %s noisy%s" % (build, name, dtype, "" if mag_mean is None else " per-frame floor"), n_frames,
                 worst / MAG_TOL, clear.sum(), (gs == bits).mean()), end="")
        ties = 0
        try:
            assert clear.mean() >= 0.995
            assert np.array_equal(gs[clear], rs[clear])
            if mag_mean is None:
                assert (gs == bits).mean() > (0.995 if n == 2048 else 0.97), (gs == bits).mean()
            for h in (0, 1):
                ties += check_history(o, lambda f: x[f * n: f * n + n + tsu.HALO], gst[:, h], rst[:, h], h,
                                      "%s noisy hist%d" % (build, h), spectrum_kw={"halo": tsu.HALO})
                np.testing.assert_array_equal(gst[:, h]["mag_mean"], rst[:, h]["mag_mean"])
                snr_err = np.abs(gst[:, h]["snr"].astype(np.float64) - rst[:, h]["snr"]) / np.maximum(np.abs(rst[:, h]["snr"]), 1.0)
                assert snr_err.max() < 1e-4
            assert ties <= 0.02 * n_frames
        finally:
            print("  near-ties proven %d" % ties)
    e.close()
