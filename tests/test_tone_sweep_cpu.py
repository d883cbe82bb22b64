"""Oracle-only proof that the tone sweeps of tests/tone_sweep_util.py do what tests/test_gpu_tone_sweep.py relies on:
every bin of both search windows is, in at least one frame, the CLEAR winner of its window in the float64 oracle
spectrum (second-largest bin <= 0.99 x the largest) -- so that the GPU test, which compares indices exactly on clear
winners, reaches every bin.  No GPU here."""
import numpy as np
import pytest

from oracle import uco
from parity_util import clear_symbols
import tone_sweep_util as tsu

FIRMWARE_CAP = 0.85      # the FIR's pass band does not reach the ends of the firmware's windows


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("name", list(tsu.CASES))
def test_every_window_bin_is_a_clear_winner_in_some_frame(name, dtype):
    sw, _ = tsu.sweep(name, dtype)
    o = sw.o
    kind, _, recipe, geo = tsu.CASES[name]
    assert o.bandwidth2 == geo["bw2"]
    whole = sw.whole()
    cov = sw.coverage()
    worst = max(float(sw.ratio[s][sw.clear[s]].max()) for s in sw.windows)
    print("%s %s: %d frames, %d of %d window bins are a clear winner, worst clear second/first %.3f"
          % (name, dtype, sw.n_frames, len(cov & whole), len(whole), worst))
    assert cov <= whole
    if recipe == "iq_fw":
        print("  left out: %s" % sorted(whole - cov))
        assert len(cov) >= FIRMWARE_CAP * len(whole)
    else:
        assert cov == whole, sorted(whole - cov)
        # ... and in EVERY history (the up and the down frames of the recipe serve one each)
        per = sw.coverage(per_history=True)
        for h in range(o.spf):
            assert {(s, k) for (hh, s, k) in per if hh == h} == whole, h
    # the oracle's records agree with its spectrum wherever the winner is clear: the exact rule compares records
    for h in range(o.spf):
        for s in sw.windows:
            for f in np.nonzero(sw.clear[s][h])[0]:
                assert sw.records[f, h]["max_freq_" + s] == sw.record_of_bin(s, sw.win[s][h, f]), (h, s, f)


@pytest.mark.parametrize("name", [k for k, v in tsu.CASES.items() if v[2] != "iq_fw"])
def test_off_window_frames_exist_and_their_winners_lie_inside(name):
    sw, order = tsu.sweep(name)
    o = sw.o
    _, bs = tsu.build_frames(name, o)
    bw2 = o.bandwidth2
    off = np.nonzero(np.abs(bs) >= bw2)[0]
    assert {int(abs(b)) for b in bs[off]} >= {bw2, bw2 + 1}
    if bs.min() < 0:
        assert {int(b) for b in bs[off]} >= {-bw2, -bw2 - 1, bw2, bw2 + 1}
    for f in off:
        for h in range(o.spf):
            for s, (a, b) in sw.windows.items():
                assert a <= sw.win[s][h, f] < b


@pytest.mark.parametrize("name", ["rx_real-literal", "sync_cplx-literal"])
def test_overlap_layout_keeps_every_frame_a_clean_tone(name):
    """Stride 2047: the shared sample is the later frame's sample 0, which the periodic Hann weights with 0 -- the
    oracle's account of the overlapped batch is that of the separate frames."""
    sw, _ = tsu.sweep(name)
    ov, _ = tsu.sweep(name, stride=2047)
    assert sw.o.table(uco.TABLE_HANN)[0] == 0.0
    assert ov.stride == 2047 and ov.buf.size == (ov.n_frames - 1) * 2047 + 2048
    assert ov.coverage(per_history=True) == sw.coverage(per_history=True)
    for s in sw.windows:
        assert np.array_equal(ov.win[s], sw.win[s]) and np.array_equal(ov.clear[s], sw.clear[s])
    for fld in ("max_freq", "max_freq_left", "max_freq_right"):
        assert np.array_equal(ov.records[fld], sw.records[fld])


def test_permutations_are_permutations_and_keep_pairs():
    p = tsu.permutation(641)
    assert sorted(p) == list(range(641)) and (p != np.arange(641)).mean() > 0.9
    q = tsu.permutation(163, keep_pairs=True)
    assert sorted(q) == list(range(163)) and q[-1] == 162
    assert (q[0:162:2] % 2 == 0).all() and (q[1:162:2] == q[0:162:2] + 1).all() and (q[:162] != np.arange(162)).mean() > 0.9


@pytest.mark.parametrize("name", ["iq1024-bb1", "iq2048-bb1"])
def test_noisy_stream_of_the_wider_base_band_decodes_on_the_oracle(name):
    """The 200-frame -10 dB stream the GPU test feeds the BB = 1 and FIRM = 1 builds: the oracle decodes it as well
    as the stream of BASELINE configs[2] (tests/test_gpu_iq_baseband.py), so the GPU test's decode claim has room."""
    x, bits, o = tsu.noisy_stream(name)
    rs, rst = o.process(x, halo=tsu.HALO, n_frames=len(bits))
    rate, clear = (rs == bits).mean(), clear_symbols(rst)
    print("%s: oracle decodes %.3f of 200 frames at -10 dB, %d clear decisions" % (name, rate, clear.sum()))
    assert rate > (0.995 if o.n == 2048 else 0.97) and clear.mean() >= 0.995
