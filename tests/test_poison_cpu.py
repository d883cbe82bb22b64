"""The masks of tests/poison_util.py, proved without a GPU: for every case and position the float64 model of the library is
evaluated on the clean rows and on rows whose sample q is moved by a finite amount.  The outputs that differ are exactly
`reads` (the MUST zone), except where the term's other factor is exactly zero -- and those are listed by the case
(`zero_terms`), not ignored.  MAY never overlaps MUST, and every position hits the zones it is there for."""
import numpy as np
import pytest

import poison_util as pu

CASES = pu.all_cases()

# what the issue asks of the cases: none is dropped
EXPECTED = {"xcorr-L64", "xcorr-L512", "xcorr-clip", "align-L5", "align-L64", "mf-c32-pos0", "mf-c32-far", "mf-f32-far",
            "spec-hop100-all", "spec-hop100-ac-sub", "spec-hop400-ac-all", "spec-hop400-sub",
            "rate-3125-1764", "rate-5-13", "array-3x600", "retime-3x600",
            "track-hop1024", "track-hop3000", "mf-f32-pos0",
            "wcorr-ones-hop1024", "wcorr-band-hop1024", "wcorr-band-hop3000", "wcorr-zero-hop3000"}
# the only cases with a term whose other factor is exactly zero: a reference sample at the row's end, whose microphone
# window the row clips (outside the row a microphone reads +0)
# ... and a frame's sample 0 under the periodic Hann window, whose first coefficient is exactly zero
ZERO_TERMS = {("xcorr-clip", "ref 0"), ("xcorr-clip", "ref last")}
# (at hop 100 the sample behind frame 5's last one, 750, is frame 8's sample 0)
ZERO_TERMS |= {("spec-hop100-%s" % n, label) for n in ("all", "ac-sub") for label in ("frame 5 first", "frame 5 last+1")}
ZERO_TERMS |= {("spec-hop400-%s" % n, "frame 1 first") for n in ("ac-all", "sub")}
# ... and the fifteen zero coefficients of a tap with an integer delay (microphone 2 has no other tap; microphone 0 has one)
ZERO_TERMS |= {("array-3x600", label) for label in ("int support 0", "int support 15", "int centre", "first output support 0",
                                                     "last output support 15")}
ZERO_TERMS |= {("retime-3x600", "int centre")}          # (the same, for the line with slope 0 and a whole delay)


# rate: how many of a position's terms have a zero coefficient.  3125 / 1764: the table holds up * T entries for a prototype
# of N_h = 2 half q + 1 values, so up T - N_h = 3124 of them are zeros, all at tap T - 1 (the oldest sample); a sample is
# under tap T - 1 of ceil(up / down) = 2 outputs (the row's last sample of none that the row's outputs include).
# 5 / 13: up T = N_h, no padding; but sample 0 sits at the prototype's index c + 13 m for output m, a zero of the sinc
# for every output that reads it but output 0.
RATE_ZERO_TERMS = {"rate-3125-1764": {"k-T": 2, "k-T+1": 2, "k": 2, "k+1": 2, "row 0": 2, "row last": 0},
                   "rate-5-13": {"k-T": 0, "k-T+1": 0, "k": 0, "k+1": 0, "row 0": 24, "row last": 0}}


def test_rate_zero_taps():
    from uchirp import rate
    for c in CASES:
        if c.lib == "rate":
            tab = rate.table(c.info)                          # uc_rate_table: [up, T]
            n_h = 2 * c.HALF * max(c.info.up, c.info.down) + 1
            behind = np.arange(c.info.up)[:, None] + np.arange(c.T)[None, :] * c.info.up >= n_h
            assert (tab[behind] == 0).all() and behind[:, :-1].sum() == 0 and behind.sum() == c.info.up * c.T - n_h
            assert behind.sum() == {"rate-3125-1764": 3124, "rate-5-13": 0}[c.name]
            assert set(RATE_ZERO_TERMS[c.name]) == {p.label for p in c.positions}
            # the edges of the middle output, from uc_rate_step
            by = {p.label: p for p in c.positions}
            want = {"k-T": False, "k-T+1": True, "k": True, "k+1": False}
            for label, inside in want.items():
                assert c.reads(by[label])["out"][0, c.mid] == inside, (c.name, label)


def test_no_case_is_dropped():
    assert {c.name for c in CASES} == EXPECTED
    assert {c.lib for c in CASES} == set(pu.LIBRARIES)
    for c in CASES:
        labels = [(p.label, p.part) for p in c.positions]
        assert len(labels) == len(set(labels)) and len(labels) >= 4, c.name
        for p in c.positions:
            assert 0 <= p.q < c.rows.shape[1] and 0 <= p.row < c.rows.shape[0], (c.name, p.label)
        wants = [frozenset(p.want) for p in c.positions]
        assert any("must" in w for w in wants), c.name
        assert any("may" in w for w in wants) == (c.lib in pu.HAVE_MAY), c.name
        # (an mf row ends inside its last window, xcorr-clip reads its rows whole, and frames every 100 samples leave no
        # gap: no sample lies outside every zone)
        if c.lib not in ("mf", "rate") and c.name != "xcorr-clip" and not c.name.startswith("spec-hop100"):
            assert frozenset() in wants, c.name
    assert pu.GRIDS == (None, 1, 2) and len(pu.POISONS) == 3


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_masks_are_the_models_reach(case):
    clean = case.model(case.rows)
    for pos in case.positions:
        got = case.model(pu.moved(case.rows, pos))
        must, may, zero = case.reads(pos), case.may(pos), case.zero_terms(pos)
        for name, ref in clean.items():
            differs = got[name] != ref
            m, z = must[name], zero[name]
            assert m.shape == ref.shape == may[name].shape, (case.name, pos.label, name)
            assert not (differs & ~m).any(), (case.name, pos.label, name, "an output outside MUST changed")
            assert not (z & ~m).any()
            if case.lib == "wcorr":      # which terms have a zero coefficient is the weights' matter: test_wcorr_zero_terms
                pass
            elif case.lib == "rate":
                assert z.sum() == RATE_ZERO_TERMS[case.name][pos.label], (case.name, pos.label, "zero terms are listed")
            else:
                assert z.any() == ((case.name, pos.label) in ZERO_TERMS), (case.name, pos.label, "zero terms are listed")
            assert np.array_equal(differs, m & ~z), (case.name, pos.label, name, np.argwhere(differs != (m & ~z))[:8])
        for name in must:
            assert not (must[name] & may[name]).any(), (case.name, pos.label, name)
        hit_must = any(v.any() for v in must.values())
        hit_may = any(v.any() for v in may.values())
        assert hit_must == ("must" in pos.want), (case.name, pos.label, pos.part, "MUST", hit_must)
        assert hit_may == ("may" in pos.want), (case.name, pos.label, pos.part, "MAY", hit_may)


def test_array_support_edges():
    """array: the sixteen samples under a tap, from uc_array_tap_coefficients' shift"""
    c = next(c for c in CASES if c.lib == "array")
    by = {p.label: p for p in c.positions}
    j = c.J - c.OUT_FIRST
    for label, inside in (("frac support-1", False), ("frac support 0", True), ("frac support 15", True), ("frac support 16", False)):
        assert c.reads(by[label])["out"][1, j] == inside, label   # (beam 2 has a tap of microphone 1 too, at another delay)
        assert not c.reads(by[label])["out"][0].any()           # beam 0 has no tap of microphone 1
    assert c.reads(by["first output support 0"])["out"][2].sum() == 1 and c.reads(by["first output support 0"])["out"][2, 0]
    assert c.reads(by["last output support 15"])["out"][2].sum() == 1 and c.reads(by["last output support 15"])["out"][2, -1]
    assert c.reads(by["int centre"])["out"][0].sum() == 16 and c.zero_terms(by["int centre"])["out"][0].sum() == 15


def test_retime_support_edges():
    """retime: the sixteen samples under output J of the line with slope +2^-9, from uc_retime_fixed's integers"""
    c = next(c for c in CASES if c.lib == "retime")
    by = {p.label: p for p in c.positions}
    j = c.J - c.OUT_FIRST
    for label, inside in (("support-1", False), ("support 0", True), ("support 15", True), ("support 16", False)):
        assert c.reads(by[label])["out"][1, j] == inside, label
    assert c.reads(by["first output support 0"])["out"][2, 0] and c.reads(by["last output support 15"])["out"][2, -1]
    # the slope moves the support against the output: one sample more than the 399 steps of the outputs
    assert c.steps[1][0][-1] - c.steps[1][0][0] == 400


def test_wcorr_zero_terms():
    """wcorr: the definition is total, so a sample of a window's segments has a term in every stored lag.  Band weights leave
    no coefficient exactly zero; weights of zero leave none that is not; with weights of ones the impulse response is the
    unit impulse and the terms left are uc_xcorr_correlate's at L + guard.  The guard widens the microphone's range."""
    for c in CASES:
        if c.lib == "wcorr":
            by = {p.label: p for p in c.positions}
            for pos in c.positions:
                m, z = c.reads(pos)["corr"], c.zero_terms(pos)["corr"]
                assert m.all(axis=2).sum() == m.any(axis=2).sum()              # whole (pair, window)s
                if c.kind == "band":
                    assert not z.any()
                elif c.kind == "zero":
                    assert np.array_equal(z, m)
                else:
                    assert not (z & ~m).any() and np.array_equal(m & ~z, c._xcorr_reach(pos) & ~z)
            # a microphone sample that only the guard's lags read: in window 0 all the same
            assert c.reads(by["mic in the guard alone"])["corr"][0, 0].all()
            assert not c.reads(by["mic before window 0"])["corr"].any()
            # window 1's own edges, guard included
            assert not c.reads(by["mic first-L-g-1"])["corr"][0, 1].any() and c.reads(by["mic first-L-g"])["corr"][0, 1].all()
            assert c.reads(by["mic first+n+L+g-1"])["corr"][0, 1].all() and not c.reads(by["mic first+n+L+g"])["corr"][0, 1].any()
            if c.kind == "ones":
                assert c.zero_terms(by["mic in the guard alone"])["corr"][0, 0].all()    # no stored lag of the plain sums reads it


def test_align_bound_is_the_kernels_pass():
    """the MAY stretch of align: the last segment's 300 samples take two passes of 256, so 212 padded lanes"""
    for c in CASES:
        if c.lib == "align":
            assert c.n_up - c.n == 212
            inside = next(p for p in c.positions if p.label == "mic pad last")
            outside = next(p for p in c.positions if p.label == "mic pad end")
            assert outside.q == inside.q + 1
            m = c.may(inside)["corr"]
            assert m[0].sum() == 1 and m[0, -1] and m[1].sum() == 1 and m[1, -1]      # lag +L alone, in both pairs


def test_mf_window_edges():
    """mf: the window of the middle segment is base - T .. base + S; its first and last element are read by no sum of the
    segment (MAY), one element further out the segment is untouched"""
    for c in CASES:
        if c.lib == "mf":
            by = {(p.label, p.part): p for p in c.positions}
            part = c.positions[0].part
            for label, touched in (("base-T-1", False), ("base-T", True), ("base+S", True), ("base+S+1", False)):
                p = by[(label, part)]
                assert c.may(p)["rec"][:, 1].all() == touched and not c.reads(p)["rec"][:, 1].any(), (c.name, label)
            assert c.reads(by[("base-T+1", part)])["rec"][:, 1].all() and c.reads(by[("base+S-1", part)])["rec"][:, 1].all()
