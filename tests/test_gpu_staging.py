"""The staging protocol of the sibling libraries on the GPU (csrc/uc_host.hpp: two pinned + device pairs used in turn, the
`copied` and `done` events, a pair that grows while its last kernel may still read it): four calls back to back on one
non-default stream, with NO synchronisation between them, into four outputs of their own, each bit for bit what the same
call gives alone on a fresh object with a synchronise behind it.

The argument tables hold 3, 600, 3 and 2000 records: slot 0 stays at its first 4096 bytes and is staged again while call 0
may still be in flight; slot 1 takes the 600 records and has to grow for the 2000 while the kernel of call 1 may still read
it (the unit sums of align, xcorr and track grow with it).  Inputs: 8 rows x 4096 samples, max_lag 8, one window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NM, NS, L = 8, 4096, 8
SIZES = (3, 600, 3, 2000)


@pytest.fixture(scope="module")
def rows():
    """8 rows x 4096 samples on the device; made once and never written."""
    import torch
    x = torch.from_numpy((np.random.default_rng(31).standard_normal((NM, NS)) * 1000.0).astype(np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    return x


def _pairs(n, rng):
    return [(int(a), int(b)) for a, b in rng.integers(0, NM, size=(n, 2))]


def _beams(n, rng):
    """n taps in beams of at most 25"""
    taps = [(int(rng.integers(0, NM)), float(rng.uniform(-1.0, 1.0)), float(rng.uniform(-20.0, 20.0))) for _ in range(n)]
    return [taps[i:i + 25] for i in range(0, n, 25)]


def _lines(n, rng):
    return [(int(rng.integers(0, NM)), float(rng.uniform(-20.0, 20.0)), float(rng.uniform(-1e-4, 1e-4))) for _ in range(n)]


def _case(name):
    """(make the object, the table of n records, the call: the tuple of tensors it writes)"""
    if name == "array":
        from uchirp import array
        return array.Array, _beams, lambda o, x, t: (o.combine(x, t),)
    if name == "align":
        from uchirp import align
        return align.Aligner, _pairs, lambda o, x, t: (o.correlate(x, t, max_lag=L),)
    if name == "xcorr":
        from uchirp import xcorr
        return xcorr.Xcorr, _pairs, lambda o, x, t: (o.correlate(x, t, max_lag=L),)
    if name == "retime":
        from uchirp import retime
        return retime.Retimer, _lines, lambda o, x, t: (o.rows(x, t),)
    from uchirp import track
    return track.Tracker, _pairs, lambda o, x, t: o.windows(x, t, window_len=NS, n_windows=1, max_lag=L, corr=True)


@pytest.mark.parametrize("name", ["array", "align", "xcorr", "retime", "track"])
def test_back_to_back_calls_equal_the_calls_alone(name, rows):
    import torch
    make, table, call = _case(name)
    tables = [table(n, np.random.default_rng(100 + i)) for i, n in enumerate(SIZES)]
    stream = torch.cuda.Stream()
    obj = make()
    with torch.cuda.stream(stream):
        outs = [call(obj, rows, t) for t in tables]          # four calls, nothing waits in between
    stream.synchronize()
    got = [[o.cpu().numpy().tobytes() for o in out] for out in outs]
    obj.close()
    want = []
    for t in tables:
        alone = make()
        with torch.cuda.stream(stream):
            out = call(alone, rows, t)
        stream.synchronize()
        want.append([o.cpu().numpy().tobytes() for o in out])
        alone.close()
    for i, (g, w) in enumerate(zip(got, want)):
        same = [a == b for a, b in zip(g, w)]
        print("%s: call %d, %d records, %s bytes written: %s" % (name, i, SIZES[i], [len(b) for b in w], "same bits" if all(same) else "DIFFERENT"))
        assert all(len(b) > 0 and any(b) for b in w), "call %d wrote nothing" % i
    assert got == want
