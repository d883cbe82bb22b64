"""Pulse sweeps: the clear maximum through every output index of compress_kernel (both slots of a frame pair) and through
every offset of a stream_kernel block; the ragged last block; non-finite samples in a stream.

The parity tests of these two kernels (test_gpu_parity.py::test_compress_variant_fft_h_ifft, test_gpu_scale.py,
test_stream.py) leave it to random numbers which output wins a frame or a block.  Here the inputs of
tests/pulse_sweep_util.py make every one of them the CLEAR winner somewhere (proven on the float64 oracle alone by
tests/test_pulse_sweep_cpu.py), so that its own thread, slot t, last-pass twiddle and place in the first-maximum search
decide a record.

compress (Engine(COMPRESS, mag_mean=1.0), float32 frames and int32 words), on every batch:
  1. mag_max within MAG_TOL x |the oracle's| on every frame (an all-zero frame: x its partner's, include/uchirp.h);
  2. on every clear frame (second-largest output <= 0.99 x the largest) every index field IS the oracle's;
  3. on the rest an index mismatch must be a near-tie within MAG_TOL x |max| in the oracle's own output;
  4. symbols all SYM_NONE; the index sets reached by 2. are counted per pair slot.
stream (D 4 / 8 / 16, float32 and int32; D 8 under FLAG_STREAM_UP):
  5. peaks.offset IS the oracle's in every clear block (second <= 0.995 x first), which is every aimed block;
  6. peaks.value and all of `compressed` within STREAM_TOL x the stream's largest oracle value; any other offset
     mismatch a near-tie by test_stream.py's rule.
`pytest -s` prints the figures before anything is asserted."""
import numpy as np
import pytest

from oracle import uco
from parity_util import MAG_TOL
from test_stream import STREAM_TOL
from test_gpu_decision import snr_of
import pulse_sweep_util as psu

pytestmark = pytest.mark.gpu

INDEX_FIELDS = ("max_freq", "max_freq_left", "max_freq_right")


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


def _engine(uchirp, monkeypatch, variant, env, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = uchirp.Engine(variant, **kw)
    for k in env:
        monkeypatch.delenv(k)
    return e


# ------------------------------------------------------------------------------------------------ compress

def _compress_against_the_oracle(uchirp, acc, order, gs, gst, label, paired=True):
    """1 - 4 of the module's docstring on the batch of a layout -> (indices exact-compared in slot a, in slot b)."""
    order = np.asarray(order)
    g, r = gst[:, 0], acc.records(order)
    nf = len(order)
    assert g.shape == r.shape == (nf,)
    rmax = np.abs(r["mag_max"].astype(np.float64))
    scale = rmax.copy()
    if paired:      # an all-zero frame's round-off is its partner's (one complex transform per pair)
        partner = np.arange(nf) ^ 1
        partner[partner >= nf] = nf - 1
        scale = np.where(order == psu.ZERO, rmax[partner], scale)
    scale = np.maximum(scale, 1e-30)
    err = np.abs(g["mag_max"].astype(np.float64) - r["mag_max"].astype(np.float64)) / scale
    real = order != psu.ZERO
    clear = np.zeros(nf, bool)
    clear[real] = acc.clear[order[real]]
    wrong = np.zeros(nf, bool)
    for fld in INDEX_FIELDS:
        wrong |= g[fld] != r[fld]
    bad = np.nonzero(wrong & clear)[0]
    ha, hb = psu.slot_hits(acc, order, paired)
    print("%-46s %5d frames  worst |gpu - oracle| / (MAG_TOL x |max|) %.3f  exact comparisons %5d, %d wrong; indices reached in "
          "slot a %4d, slot b %4d" % (label, nf, err.max() / MAG_TOL, int(clear.sum()), bad.size, len(ha), len(hb)), end="")
    ties = 0
    try:
        for f in np.nonzero(wrong & ~clear)[0]:     # every other mismatch: a near-tie in the oracle's own output
            y = acc.spectrum(order[f])
            assert g["max_freq"][f] == g["max_freq_right"][f] and g["max_freq_left"][f] == 0, (label, f)
            assert 0 <= g["max_freq"][f] < psu.N, (label, f)
            assert y.max() - y[g["max_freq"][f]] <= MAG_TOL * abs(y.max()), \
                "%s frame %d: GPU index %d is not a near-tie (%.6g vs max %.6g)" % (label, f, g["max_freq"][f], y[g["max_freq"][f]], y.max())
            ties += 1
    finally:
        print("  near-ties proven %d" % ties)
    assert err.max() <= MAG_TOL, "%s: mag_max rel err %.3g on frame %d" % (label, err.max(), int(np.argmax(err)))
    assert bad.size == 0, "%s: %d exact comparisons fail, first (frame, gpu, oracle): %r" % (
        label, bad.size, [(int(f), int(g["max_freq"][f]), int(r["max_freq"][f])) for f in bad[:8]])
    for fld in ("mag_max_left",):
        assert not g[fld].any(), label
    assert np.array_equal(g["mag_max_right"].view(np.uint32), g["mag_max"].view(np.uint32)), label
    assert (gs == uchirp.SYM_NONE).all(), label
    return ha, hb


def _same_bits(a, b, label):
    assert np.array_equal(a[0], b[0]), label
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), label


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_compress_every_index_wins_in_both_pair_slots(uchirp, dtype):
    """The batch as it stands, and with one all-zero frame in front (16 385 frames: every frame changes slot and partner,
    the last pair is ragged): every output index is the exact-compared winner in slot a and in slot b."""
    acc = psu.compress_account(dtype)
    e = uchirp.Engine(uchirp.COMPRESS, mag_mean=1.0)
    base, shifted = psu.layout("base"), psu.layout("zero_front")
    a0, b0 = _compress_against_the_oracle(uchirp, acc, base, *e.process(acc.frames), "compress %s" % dtype)
    gs, gst = e.process(acc.batch(shifted))
    a1, b1 = _compress_against_the_oracle(uchirp, acc, shifted, gs, gst, "compress %s, zero frame in front" % dtype)
    # (the zero frame rides with frame 0: its outputs are that frame's round-off, within the bar of 0 -- include/uchirp.h)
    assert len(shifted) % 2 == 1 and abs(float(gst[0, 0]["mag_max"])) <= MAG_TOL * abs(float(gst[1, 0]["mag_max"]))
    print("  every index the exact-compared winner: slot a %d, slot b %d of 2048" % (len(a0 | a1), len(b0 | b1)))
    assert len(a0 | a1) == psu.N and len(b0 | b1) == psu.N
    e.close()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_compress_permuted_pairs_and_other_partners(uchirp, dtype):
    """A permutation of whole pairs: the unpermuted run's records, bit for bit, frame by frame.  A permutation of the
    frames (other partners in the shared transform): the oracle's bars and the exact rule again."""
    acc = psu.compress_account(dtype)
    e = uchirp.Engine(uchirp.COMPRESS, mag_mean=1.0)
    gs, gst = e.process(acc.frames)
    order = psu.layout("pairs")
    ps, pst = e.process(acc.batch(order))
    _same_bits((ps, pst), (gs[order], gst[order]), "compress %s permuted pairs" % dtype)
    order = psu.layout("frames")
    qs, qst = e.process(acc.batch(order))
    ha, hb = _compress_against_the_oracle(uchirp, acc, order, qs, qst, "compress %s, other partners" % dtype)
    assert len(ha | hb) == psu.N
    e.close()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_compress_launch_shapes_and_unpaired(uchirp, monkeypatch, uc_tuning, dtype):
    """One workgroup with chunks of 2 pairs and three workgroups under the static deal: the bits of the default launch.
    FLAG_NO_FRAME_PAIRS (every frame alone in its transform): the oracle's bars, exact max_freq on clear frames."""
    acc = psu.compress_account(dtype)
    e = uchirp.Engine(uchirp.COMPRESS, mag_mean=1.0)
    ref = e.process(acc.frames)
    for env in ({"UC_GRID": "1", "UC_COMPRESS_CHUNK": "2"}, {"UC_GRID": "3", "UC_STATIC_DEAL": "1"}):
        e1 = _engine(uchirp, monkeypatch, uchirp.COMPRESS, env, mag_mean=1.0)
        _same_bits(e1.process(acc.frames), ref, "compress %s %r" % (dtype, env))
        e1.close()
    eu = uchirp.Engine(uchirp.COMPRESS, mag_mean=1.0, flags=uchirp.FLAG_NO_FRAME_PAIRS)
    for kind in ("base", "zero_front"):
        order = psu.layout(kind)
        us, ust = eu.process(acc.batch(order))
        ha, hb = _compress_against_the_oracle(uchirp, acc, order, us, ust, "compress %s unpaired %s" % (dtype, kind), paired=False)
        assert len(ha) == psu.N and not hb
        if kind == "zero_front":        # alone in its transform the zero frame is exact: every output ties at 0, the first wins
            assert ust[0, 0]["mag_max"] == 0.0 and ust[0, 0]["max_freq"] == 0 and ust[0, 0]["snr"] == -1.0
    eu.close()
    e.close()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_compress_decision_fields_are_the_kernels_own_numbers(uchirp, dtype):
    """Per-frame noise floors, the two floats of a frame distinct: stats.mag_mean is the first of the two, and snr is
    (mag_max - mag_mean) / mag_mean in float32 from the kernel's OWN mag_max, bit for bit on every frame -- paired and
    unpaired, with the ragged last frame of 16 385."""
    acc = psu.compress_account(dtype)
    order = psu.layout("zero_front")
    x = acc.batch(order)
    mm = psu.distinct_mag_mean(len(order), 256.0 if dtype == "int32" else 1.0)
    for flags, label in ((0, "paired"), (uchirp.FLAG_NO_FRAME_PAIRS, "unpaired")):
        e = uchirp.Engine(uchirp.COMPRESS, mag_mean=1.0, flags=flags)
        for cnt in (len(order), len(order) - 1):
            gs, gst = e.process(x[:cnt], mag_mean=mm[:cnt])
            g = gst[:, 0]
            want = snr_of(g["mag_max"], mm[:cnt, 0])
            same = want.view(np.uint32) == g["snr"].view(np.uint32)
            floor = np.array_equal(g["mag_mean"].view(np.uint32), mm[:cnt, 0].view(np.uint32))
            print("compress %s %s %d frames: mag_mean == the frame's first float: %s; snr == (mag_max - mag_mean) / mag_mean in "
                  "float32 on %d of %d frames; snr %.3g .. %.3g" % (dtype, label, cnt, floor, int(same.sum()), cnt, g["snr"].min(),
                                                                    g["snr"].max()))
            assert floor
            assert same.all(), np.nonzero(~same)[0][:8]
            assert (gs == uchirp.SYM_NONE).all()
            # ... and the floor does not touch the search
            ref = acc.records(order[:cnt])
            c = np.zeros(cnt, bool)
            c[1:] = acc.clear[order[1:cnt]]
            assert np.array_equal(g["max_freq"][c], ref["max_freq"][c])
        e.close()


# ------------------------------------------------------------------------------------------------ stream

def _stream_against_the_oracle(acc, cg, pg, label):
    """5 - 6 of the module's docstring; prints the figures before it asserts -> offsets reached by exact comparisons."""
    cr, pr, hop = acc.comp, acc.peaks, acc.hop
    assert cg.shape == cr.shape and pg.shape == pr.shape, label
    scale = acc.scale
    err = float(np.abs(cg.astype(np.float64) - cr.astype(np.float64)).max()) / scale
    perr = float(np.abs(pg["value"].astype(np.float64) - pr["value"].astype(np.float64)).max()) / scale
    off_ok = pg["offset"] < np.array([acc.valid(b) for b in range(acc.n_blocks)])
    wrong = pg["offset"] != pr["offset"]
    bad = np.nonzero(wrong & acc.clear)[0]
    hit = set(int(v) for v in pr["offset"][acc.clear & ~wrong])
    # the stored outputs are v_sqrt_f32 (1 ulp), the record's value sqrtf: printed, not asserted
    own = cg[np.arange(acc.n_blocks)[off_ok] * hop + pg["offset"][off_ok]]
    ulp = int((own.view(np.uint32) != pg["value"][off_ok].view(np.uint32)).sum())
    print("%-34s %5d blocks  worst |gpu - oracle| / (STREAM_TOL x stream max): compressed %.3f, peaks %.3f  exact comparisons %5d "
          "on %4d of %4d offsets, %d wrong; record != stored output on %d blocks" % (label, acc.n_blocks, err / STREAM_TOL, perr / STREAM_TOL,
                                                                                    int(acc.clear.sum()), len(hit), hop, bad.size, ulp), end="")
    ties = 0
    try:
        assert off_ok.all(), "%s: offsets outside their block in blocks %r" % (label, np.nonzero(~off_ok)[0][:8])
        for b in np.nonzero(wrong & ~acc.clear)[0]:       # legal only as a near-tie of the oracle's own block maximum
            assert cr[b * hop + pg["offset"][b]] >= pr["value"][b] - STREAM_TOL * scale, \
                "%s: block %d peak offset %d is not a near-tie" % (label, b, pg["offset"][b])
            ties += 1
    finally:
        print("  near-ties proven %d" % ties)
    assert err <= STREAM_TOL, "%s: |gpu - oracle| = %.3g of the stream's peak" % (label, err)
    assert perr <= STREAM_TOL, "%s: peak values, |gpu - oracle| = %.3g of the stream's peak" % (label, perr)
    assert bad.size == 0, "%s: %d exact comparisons fail, first (block, gpu, oracle): %r" % (
        label, bad.size, [(int(b), int(pg["offset"][b]), int(pr["offset"][b])) for b in bad[:8]])
    return hit


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("case", list(psu.STREAM_CASES))
def test_stream_every_offset_is_the_peak_of_a_block(uchirp, monkeypatch, uc_tuning, case, dtype):
    o, x, aimed = psu.sweep_stream(case, dtype)
    acc = psu.StreamAccount(o, x)
    kw = psu.STREAM_CASES[case]
    e = uchirp.Engine(uchirp.STREAM, **kw)
    assert e.stream_geometry(x.size) == o.stream_geometry(x.size)
    cg, pg = e.process_stream(x)
    hit = _stream_against_the_oracle(acc, cg, pg, "stream %s %s" % (case, dtype))
    assert acc.clear[1:].all() and hit >= set(range(acc.hop))
    assert np.array_equal(pg["offset"][1:], aimed[1:])
    if case == "D8" and dtype == "float32":      # other grids, chunk sizes and the static deal: the same bytes
        for env in ({"UC_GRID": "1", "UC_STREAM_CHUNK": "1"}, {"UC_GRID": "3", "UC_STREAM_CHUNK": "4"},
                    {"UC_GRID": "3", "UC_STATIC_DEAL": "1"}):
            e1 = _engine(uchirp, monkeypatch, uchirp.STREAM, env, **kw)
            c1, p1 = e1.process_stream(x)
            assert np.array_equal(c1.view(np.uint32), cg.view(np.uint32)), env
            assert np.array_equal(p1.view(np.uint8), pg.view(np.uint8)), env
            e1.close()
    e.close()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_stream_ragged_last_block_keeps_its_peak_in_front_of_valid(uchirp, dtype):
    """The largest value of the last block lies BEHIND `valid` (a symbol cut off by the end of the stream; the kernel's
    out-of-range loads read zeros): only the range check of the search keeps it from winning.  The record is the
    oracle's for the stream as it is; `compressed` has exactly n_out values, the words behind them stay untouched."""
    import torch
    dev = torch.device("cuda:0")
    e = uchirp.Engine(uchirp.STREAM)
    guard = 4096
    for v in psu.RAGGED_VALID:
        o, x, _, valid = psu.ragged_stream(v, dtype)
        acc = psu.StreamAccount(o, x)
        cg, pg = e.process_stream(x)
        _stream_against_the_oracle(acc, cg, pg, "ragged valid %d %s" % (valid, dtype))
        assert pg["offset"][2] < valid
        if acc.clear[2]:
            assert pg["offset"][2] == acc.peaks["offset"][2]
        # device buffers with guard words behind n_out outputs and n_blocks records
        cbuf = torch.full((acc.n_out + guard,), -7.0, dtype=torch.float32, device=dev)
        pbuf = torch.full((acc.n_blocks + 8, 2), -7, dtype=torch.int32, device=dev)
        e.process_stream(torch.from_numpy(x).to(dev), compressed_out=cbuf, peaks_out=pbuf)
        torch.cuda.synchronize()
        ch, ph = cbuf.cpu().numpy(), pbuf.cpu().numpy()
        assert np.array_equal(ch[:acc.n_out].view(np.uint32), cg.view(np.uint32))
        assert (ch[acc.n_out:] == -7.0).all() and (ph[acc.n_blocks:] == -7).all(), valid
        assert np.array_equal(ph[:acc.n_blocks].copy().view(uchirp.PEAK_DTYPE).reshape(-1), pg)
    e.close()


@pytest.mark.parametrize("decim", [8, 16])
def test_stream_non_finite_samples(uchirp, decim):
    """include/uchirp.h at uc_process_stream: a NaN / Inf sample makes every output non-finite in each overlap-save block
    that reads it and no other; a record's offset is always below the block's number of outputs; a block with no output
    that compares reports (NaN, 0), arm_max_f32's answer for a block whose first element is NaN.  The oracle's
    time-domain sum turns about L outputs NaN instead of whole blocks: the documented difference, asserted as such.
    (Before the fix the all-NaN block's record was (NaN, 0x7fffffff): a host that reads compressed[b hop + offset] left
    its buffer.)"""
    o = uco.Oracle(uco.STREAM, decim=decim)
    e = uchirp.Engine(uchirp.STREAM, decim=decim)
    x = psu.noise_stream(o)
    halo, n_out, n_blocks, hop = o.stream_geometry(x.size)
    L = psu.N // decim
    pos = psu.nonfinite_positions(o, x.size)
    cases = [(k, np.nan) for k in (pos if decim == 8 else ("block3", "overlap34", "halo"))] + [("block3", np.inf)]
    valid = np.minimum(hop, n_out - np.arange(n_blocks) * hop)
    for name, val in cases:
        s = pos[name]
        hot = psu.blocks_reading(o, x.size, s)
        y, z = x.copy(), x.copy()
        y[s], z[s] = val, 0.0
        cg, pg = e.process_stream(y)
        c0, p0 = e.process_stream(z)
        cr, pr = o.process_stream(y)
        acc0 = psu.StreamAccount(o, z)
        label = "decim %d %s at %s (sample %d, blocks %s)" % (decim, "NaN" if np.isnan(val) else "+Inf", name, s, hot)
        blk = np.arange(n_out) // hop
        in_hot = np.isin(blk, hot)
        print("%s: GPU non-finite outputs %d (the blocks' %d), NaN %d; the oracle's %d (L = %d); records of those blocks %r"
              % (label, int((~np.isfinite(cg)).sum()), int(in_hot.sum()), int(np.isnan(cg).sum()), int((~np.isfinite(cr)).sum()), L,
                 [(float(pg["value"][b]), int(pg["offset"][b])) for b in hot]))
        assert (pg["offset"] < valid).all(), (label, pg["offset"])
        assert not np.isfinite(cg[in_hot]).any(), label
        for b in hot:
            if np.isnan(val):
                assert np.isnan(cg[blk == b]).all(), label
                assert np.isnan(pg["value"][b]) and pg["offset"][b] == 0, (label, pg[b])
            else:
                assert not np.isfinite(pg["value"][b]), (label, pg[b])
        # every other block: the bits of the same stream with 0.0 at that sample, and the oracle's within the bar
        cold = ~np.isin(np.arange(n_blocks), hot)
        assert np.array_equal(cg[~in_hot].view(np.uint32), c0[~in_hot].view(np.uint32)), label
        assert np.array_equal(pg[cold].view(np.uint8), p0[cold].view(np.uint8)), label
        _stream_against_the_oracle(acc0, c0, p0, "  the same with 0.0 there")
        # the documented difference: the oracle's non-finite outputs lie inside those blocks, about L of them, and
        # everything else of the oracle is what it gives with 0.0 there only outside those blocks
        bad_r = ~np.isfinite(cr)
        assert set((np.nonzero(bad_r)[0] // hop).tolist()) <= set(hot) and bad_r.sum() <= L + 26 // decim + 1 < in_hot.sum(), label
        assert np.abs(cr[~in_hot].astype(np.float64) - cg[~in_hot]).max() <= STREAM_TOL * acc0.scale, label
    e.close()
