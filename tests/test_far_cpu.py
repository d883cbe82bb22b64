"""CPU tests of the link simulator's and the scene renderer's arithmetic far from sample 0 (tests/far_util.py holds the
exact reference and the cases): the float64 model (uchirp.link.signal, which uchirp.scene.model is built from) against the
definition in rational arithmetic, the host function uc_link_frame_origin against fractions, and the record of what the
arithmetic it replaced did at the same cases.

The bar for the model, 0.01 float ulp of A sqrt 2: its time is one product and one sum on numbers under 2 s, its phase a
few operations on numbers under 500 turns, each rounded to 2^-53 relative: about 1e-13 turns, 4e-5 ulp of float at the
peak; 0.01 leaves a factor of 100 and is still 800 times under the kernels' bound of 8.  Every test prints its figures
before it asserts (pytest -s)."""
import ctypes as C
import errno
from fractions import Fraction as F

import numpy as np
import pytest

import far_util as fu

BAR = 0.01


@pytest.fixture(scope="module")
def link():
    from uchirp import link as m
    return m


@pytest.fixture(scope="module")
def built(link):
    link.build()
    link.lib()
    return link


def _streams(c):
    return zip(c["texts"], c["lead"], c["amp"], c["ppm"])


class _Exact:
    """The exact reference at the chosen samples of every stream of every case: computed once, never written to."""

    def __init__(self):
        self.cases = fu.link_cases()
        self.rows = []
        for c in self.cases:
            rows = []
            for text, lead, amp, ppm in _streams(c):
                js = fu.chosen(text, lead, ppm, c["first_sample"], c["n_samples"])
                x, on = fu.exact_signal(text, lead, amp, ppm, js)
                x.setflags(write=False)
                on.setflags(write=False)
                rows.append((np.array(js, np.int64), x, on))
            self.rows.append(rows)


@pytest.fixture(scope="module")
def exact():
    return _Exact()


def _worst(link, c, rows, time=None):
    """worst |model - exact| in float ulp of A sqrt 2 over a case's streams; the silence and the sounding range are compared
    exactly.  `time`: another time to feed the law (the old arithmetic), else link.signal itself."""
    worst = 0.0
    for (text, lead, amp, ppm), (js, x, on) in zip(_streams(c), rows):
        if time is None:
            m = link.signal(text, lead, float(amp), float(ppm), c["n_samples"], fu.FS, c["first_sample"])[js - c["first_sample"]]
            assert np.array_equal(m != 0.0, on), (fu.case_name(c), text)          # silent exactly where the definition is
            assert on.any() and not on[0] and not on[-1]                           # the whole frame lies inside the call
        else:
            m = link.law(text, time(lead, ppm, js), float(amp))
        worst = max(worst, float(np.abs(m - x).max() / fu.ulp_of_peak(amp)))
    return worst


def test_exact_reference_is_the_model_near_zero(link):
    """Three frames with lead < 2^20, where the model's arithmetic was never in doubt."""
    rng = np.random.default_rng(20)
    for text, lead, amp, ppm in (("Hi", 0.375, 20000.0, 0.0), ("a", float(rng.uniform(0, 2 ** 20)), 500.0, 200.0),
                                 ("xyz", 46 * 2048 + 0.625, 8000.0, -35.0)):
        first = max(0, int(lead) - 3000)
        n = 50 * 2048
        js = np.array(fu.chosen(text, lead, ppm, first, n), np.int64)
        x, on = fu.exact_signal(text, lead, amp, ppm, js)
        m = link.signal(text, lead, amp, ppm, n, fu.FS, first)[js - first]
        w = float(np.abs(m - x).max() / fu.ulp_of_peak(amp))
        print("near zero: lead %.3f, ppm %+.0f: %d samples (%d sounding), max |model - exact| %.2e ulp of A sqrt 2" % (lead, ppm, js.size, on.sum(), w))
        assert on.sum() > 100 and np.array_equal(m != 0.0, on)
        assert w <= BAR


def test_no_listed_case_has_a_sample_at_a_symbol_boundary():
    """Input check on the reference alone: 1e-11 s clear of every boundary, the symbol index is no matter of rounding (the
    fixed arithmetic's time error is 1e-15 s; the 1e-10 s guard of the definition is ten times this margin)."""
    worst = min(min(fu.seam_margin(text, lead, ppm) for text, lead, _, ppm in _streams(c)) for c in fu.link_cases())
    print("seams: the nearest sample lies %.3e s from a symbol boundary" % float(worst))
    assert worst >= F(1, 10 ** 11)


def test_model_is_the_definition_at_every_far_case(link, exact):
    for c, rows in zip(exact.cases, exact.rows):
        w = _worst(link, c, rows)
        print("model, first_sample %-10s: max |model - exact| %.2e ulp of A sqrt 2 over %d samples" % (fu.case_name(c), w, sum(r[0].size for r in rows)))
        assert w <= BAR, fu.case_name(c)


def test_old_arithmetic_leaves_the_bound_far_out(link, exact):
    """The record of why frame_time changed: the law fed with the time as it was taken before, one double fma of
    j * rate - lead_s (far_util.old_time, a restatement on the CPU; it asserts nothing about the library)."""
    got = {}
    for c, rows in zip(exact.cases, exact.rows):
        got[fu.case_name(c)] = w = _worst(link, c, rows, time=fu.old_time)
        print("old arithmetic, first_sample %-10s: max |law(old time) - exact| %.3g ulp of A sqrt 2" % (fu.case_name(c), w))
    assert got["2^36"] > 8.0 and got["2^40"] > 8.0 and got["2^40+3"] > 8.0
    assert got["2^31-2048"] <= 8.0              # (and it was sound where its tests were)


def test_frame_origin_against_fractions(built, exact):
    link = built
    leads = [(float(lead), float(ppm)) for c in exact.cases for _, lead, _, ppm in _streams(c)]
    leads += [(0.0, 0.0), (0.375, 200.0), (-1234.5, -35.0), (2.0 ** 53, 200.0), (-2.0 ** 53, -200.0), (2.5, 0.0), (3.5, 0.0),
              (1e300, 35.0), (-1e300, 0.0), (5.0, -1e6), (0.0, -1e6)]
    worst = 0.0
    for lead, ppm in leads:
        o, t0, rate = link.frame_origin(lead, ppm, fu.FS)
        mo, mt0, mrate = link.origin_model(lead, ppm, fu.FS)
        assert o == mo and rate == mrate, (lead, ppm)
        if abs(lead) <= 2.0 ** 53 and abs(ppm) <= 200.0:
            # the rational value of t0 for this origin, and that the origin is the sample nearest to the frame's beginning
            stretch = 1 + F(ppm) / 10 ** 6
            want = (o * stretch - F(lead)) / F(fu.FS)
            if abs(F(lead) / stretch) <= 2 ** 53:                           # (beyond: held to +-2^53, t0 takes the rest)
                assert abs(o - F(lead) / stretch) <= F(3, 2), (lead, ppm)   # (the double quotient is an ulp off at 2^53)
            else:
                assert abs(o) == 2 ** 53
            err = abs(F(t0) - want) / F(float(np.spacing(abs(float(want))))) if want else abs(F(t0))
            worst = max(worst, float(err))
            assert t0 == mt0 or err <= 2, (lead, ppm, t0, mt0)
    print("frame_origin: %d leads, t0 within %.2f ulp of the rational value" % (len(leads), worst))
    assert worst <= 2.0
    assert link.frame_origin(2.5, 0.0)[0] == 2 and link.frame_origin(3.5, 0.0)[0] == 4          # ties to even
    assert link.frame_origin(1e300, 35.0)[0] == 2 ** 53 and link.frame_origin(-1e300, 0.0)[0] == -2 ** 53
    # the shift property at the host: ppm 0, one integer added to the lead moves the origin by it and leaves t0 alone
    for lead in (100.0625, 77.5, 12345.9375):
        o, t0, _ = link.frame_origin(lead, 0.0)
        for s in (2 ** 32, 2 ** 40 + 1, 2 ** 48):
            assert link.frame_origin(lead + s, 0.0)[:2] == (o + s, t0) or (lead == 77.5 and s & 1)
    # refusals
    L, out = link.lib(), link.LinkOrigin()
    for args in ((float("nan"), 0.0, fu.FS), (float("inf"), 0.0, fu.FS), (0.0, float("nan"), fu.FS), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0),
                 (0.0, 0.0, float("inf"))):
        assert L.uc_link_frame_origin(*args, C.byref(out)) == -errno.EINVAL, args
        assert L.uc_link_last_error()
    assert L.uc_link_frame_origin(0.0, 0.0, fu.FS, None) == -errno.EINVAL
    assert C.sizeof(link.LinkOrigin) == 24
    assert link.MAX_FIRST_SAMPLE == 2 ** 52 and link.MAX_SAMPLES == 2 ** 40
