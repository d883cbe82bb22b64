"""Oracle-only proof that the pulse sweeps of tests/pulse_sweep_util.py do what tests/test_gpu_pulse_sweep.py relies on:

  * compress: every output index 0 .. 2047 is the arg-max of at least one CLEAR frame (second-largest output <= 0.99 x
    the largest in the float64 oracle), for float32 frames and for int32 words; with the all-zero frame in front every
    index has been that in slot a AND in slot b of a frame pair;
  * stream: every offset 0 .. hop - 1 is the peak of a clear block (second <= 0.995 x first), hit exactly where it was
    aimed, in every case the GPU test runs;
  * ragged last block: in the stream extended with zeros the block's largest value at o >= valid is >= 1.01 x its
    largest at o < valid, and the oracle's record of the stream as it is lies below `valid`;
  * non-finite samples: the blocks that read a sample (include/uchirp.h) are the blocks in which the oracle's
    time-domain sum has a NaN output.

0.99, 0.995 and 1.01 are conditions on the INPUTS; no kernel is compared here.  No GPU."""
import numpy as np
import pytest

from oracle import uco
import pulse_sweep_util as psu


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_every_output_index_is_the_clear_maximum_of_some_frame_in_both_slots(dtype):
    acc = psu.compress_account(dtype)
    nf = psu.PHASES * psu.N
    assert acc.frames.shape == (nf, psu.N) and acc.frames.dtype == np.dtype(dtype)
    cov = acc.coverage()
    per_phase = [len(set(acc.win[ph * psu.N:(ph + 1) * psu.N][acc.clear[ph * psu.N:(ph + 1) * psu.N]].tolist()))
                 for ph in range(psu.PHASES)]
    best = np.full(psu.N, np.inf)
    np.minimum.at(best, acc.win, acc.ratio)
    print("compress %s: %d frames, %d clear; %d of 2048 output indices are the clear maximum of a frame (phase by phase: %s); "
          "worst index has a frame at second / first = %.4f" % (dtype, nf, int(acc.clear.sum()), len(cov), per_phase, best.max()))
    assert cov == set(range(psu.N)), sorted(set(range(psu.N)) - cov)
    # the oracle's record agrees with its own output wherever the frame is clear: the exact rule compares records
    c = acc.clear
    assert np.array_equal(acc.rec["max_freq"][c], acc.win[c])
    assert np.array_equal(acc.rec["max_freq_right"][c], acc.win[c]) and not acc.rec["max_freq_left"].any()
    # slots: as built, and with one all-zero frame in front (16 385 frames: a ragged last pair)
    a0, b0 = psu.slot_hits(acc, psu.layout("base"))
    a1, b1 = psu.slot_hits(acc, psu.layout("zero_front"))
    assert len(psu.layout("zero_front")) == nf + 1 and psu.layout("zero_front")[0] == psu.ZERO
    assert a0 == b1 and b0 == a1                     # every frame changes slot
    print("  slot a / slot b: as built %d / %d, zero frame in front %d / %d, together %d / %d"
          % (len(a0), len(b0), len(a1), len(b1), len(a0 | a1), len(b0 | b1)))
    assert len(a0 | a1) == psu.N and len(b0 | b1) == psu.N
    # without pairing every frame rides in slot a
    au, bu = psu.slot_hits(acc, psu.layout("base"), paired=False)
    assert len(au) == psu.N and not bu
    # the all-zero frame: every output ties at 0, the first wins
    assert acc.zero_rec["mag_max"] == 0.0 and acc.zero_rec["max_freq"] == 0


def test_layouts_are_permutations_that_keep_or_change_partners():
    nf = psu.PHASES * psu.N
    base = psu.layout("base")
    p = psu.layout("pairs")
    assert sorted(p) == list(range(nf)) and (p != base).mean() > 0.9
    assert (p[0::2] % 2 == 0).all() and (p[1::2] == p[0::2] + 1).all()
    q = psu.layout("frames")
    assert sorted(q) == list(range(nf))
    assert ((q[0::2] >> 1) != (q[1::2] >> 1)).mean() > 0.99          # other partners
    mm = psu.distinct_mag_mean(7)
    assert mm.shape == (7, 2) and mm.dtype == np.float32 and (mm[:, 0] != mm[:, 1]).all()


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("case", list(psu.STREAM_CASES))
def test_every_offset_of_a_block_is_the_clear_peak_of_some_block(case, dtype):
    o, x, aimed = psu.sweep_stream(case, dtype)
    acc = psu.StreamAccount(o, x)
    hop, D = acc.hop, int(o.cfg.decim)
    assert hop == {4: 1537, 8: 1793, 16: 1921}[D] and acc.n_blocks == hop + 1 and acc.n_out == (hop + 1) * hop
    assert x.size == acc.halo + (hop + 1) * hop * D
    hit = set(int(v) for v in acc.peaks["offset"][acc.clear])
    print("stream %s %s: %d samples, %d blocks of %d, %d clear; %d of %d offsets are the peak of a clear block; second / first "
          "%.4f .. %.4f over the aimed blocks; block peaks %.4f .. 1 of the stream's largest"
          % (case, dtype, x.size, acc.n_blocks, hop, int(acc.clear.sum()), len(hit), hop, acc.ratio[1:].min(), acc.ratio[1:].max(),
             acc.peaks["value"][1:].min() / acc.scale))
    assert acc.clear[1:].all(), np.nonzero(~acc.clear[1:])[0][:8] + 1
    assert np.array_equal(acc.peaks["offset"][1:], aimed[1:])        # hit exactly where it was aimed
    assert set(int(v) for v in acc.peaks["offset"][1:]) == set(range(hop))
    # the bar relative to the stream's largest value is each block's own scale within a few per cent
    assert acc.peaks["value"][1:].min() >= 0.95 * acc.scale


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("valid", psu.RAGGED_VALID)
def test_ragged_last_block_has_its_maximum_behind_valid(valid, dtype):
    o, x, ext, valid = psu.ragged_stream(valid, dtype)
    acc, full = psu.StreamAccount(o, x), psu.StreamAccount(o, ext)
    hop = acc.hop
    assert acc.n_blocks == 3 and acc.valid(2) == valid and full.valid(2) == hop and 1 <= valid < hop
    assert np.array_equal(full.comp[:acc.n_out], acc.comp)          # causal: the outputs that exist do not see the extension
    seg = full.comp[2 * hop:3 * hop].astype(np.float64)
    front, behind = seg[:valid].max(), seg[valid:].max()
    print("ragged valid %4d %s: largest behind valid %.1f at offset %d = %.4f x the largest in front (%.1f at %d); valid part "
          "clear: %s" % (valid, dtype, behind, valid + int(np.argmax(seg[valid:])), behind / front, front, int(np.argmax(seg[:valid])),
                         bool(acc.clear[2])))
    assert behind >= psu.BEHIND * front and front > 0
    assert full.peaks["offset"][2] >= valid                          # a search without the range check would report this
    assert acc.peaks["offset"][2] < valid and acc.peaks["offset"][2] == int(np.argmax(seg[:valid]))


@pytest.mark.parametrize("decim", [8, 16])
def test_blocks_that_read_a_sample_are_the_blocks_the_oracle_turns_nan(decim):
    o = uco.Oracle(uco.STREAM, decim=decim)
    x = psu.noise_stream(o)
    halo, n_out, n_blocks, hop = o.stream_geometry(x.size)
    L = psu.N // decim
    assert n_blocks == 7 and n_out % hop == 13
    clean, _ = o.process_stream(x)
    for name, s in psu.nonfinite_positions(o, x.size).items():
        y = x.copy()
        y[s] = np.nan
        comp, peaks = o.process_stream(y)
        bad = np.nonzero(np.isnan(comp))[0]
        blocks = sorted(set((bad // hop).tolist()))
        want = psu.blocks_reading(o, x.size, s)
        print("decim %d NaN at %s (sample %d): blocks that read it %s; the oracle's time-domain sum has %d NaN outputs (L = %d) in "
              "blocks %s" % (decim, name, s, want, bad.size, L, blocks))
        assert blocks == want
        assert bad.size <= L + 26 // decim + 1 and (name == "halo" or bad.size >= L)
        ok = ~np.isnan(comp)
        assert np.array_equal(comp[ok], clean[ok])
    want = {k: psu.blocks_reading(o, x.size, s) for k, s in psu.nonfinite_positions(o, x.size).items()}
    assert want == {"block3": [3], "overlap34": [3, 4], "last-of-3-alone": [3], "first-of-overlap34": [3, 4],
                    "last-of-overlap34": [3, 4], "first-of-4-alone": [4], "halo": [0]}
