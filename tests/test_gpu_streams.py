"""The host-side ordering of the sibling libraries (csrc/uc_host.hpp) where one stream cannot show it: calls of one object on
TWO streams, setters and destroy while a call is still pending.  tests/test_gpu_staging.py runs five libraries on one stream,
where `hipStreamWaitEvent(hs, sl->done)` of stage_copy is a no-op; here

  (a) the seven staging libraries it lacks run its recipe (tables of 3, 600, 3 and 2000 records back to back on one stream);
      iir, ddc and duc stage only when a call names host arrays, so calls without any are put between the staged ones;
  (b) all twelve staging libraries run calls 0 and 3 on stream A and calls 1 and 2 on stream B while A is held: call 2 takes
      the slot (and the unit sums) of call 0, whose kernel has not even started;
  (c) the six setters are called from the host while a run on the held stream A is pending;
  (d) all sixteen objects are closed while their only call is pending on the held stream A.

The hold is torch.cuda._sleep on A, sized from the device's clock rate for roughly 20 ms, with an event behind it.  Every
case asserts that the event has NOT happened after the last host call that must not block ("hold too short" otherwise: no
case passes with a hold that had ended), prints the hold's measured length and asserts that it stayed under 200 ms.

Every call writes outputs (and, for iir, ddc and duc, a state) of its own; the inputs are 8 rows x 4096 samples, never
written.  The reference of every call is the same call alone on a fresh object with a synchronise behind it, bit for bit."""
import numpy as np
import pytest

from test_gpu_staging import L, NM, NS, SIZES, _beams, _lines, _pairs, rows  # noqa: F401  (rows: the module's fixture)

pytestmark = pytest.mark.gpu

HOLD_MS = 20.0
HOLD_MAX_MS = 200.0
STAGING = ["link", "scene", "array", "align", "xcorr", "wcorr", "retime", "track", "mf", "iir", "ddc", "duc"]
UNSTAGED = ["rate", "spec", "mic", "scan"]
SETTERS = ["spec", "mf", "ddc", "duc", "iir", "scan"]
N_SETS = 4


# ------------------------------------------------------------------------------------------------------------- the tables

def _streams(n, rng):
    """link: n streams (texts, lead_samples, amplitude, sigma, ppm)"""
    return (["Hi"] * n, rng.uniform(0.0, 500.0, n), rng.uniform(500.0, 2000.0, n), rng.uniform(1.0, 50.0, n), rng.uniform(-100.0, 100.0, n))


def _mics(n, rng):
    """scene: n paths in microphones of at most 16 (the library's cap on a microphone's paths)"""
    paths = [(0, float(rng.uniform(500.0, 2000.0)), float(rng.uniform(0.0, 500.0)), float(rng.uniform(-100.0, 100.0))) for _ in range(n)]
    return [(float(rng.uniform(1.0, 50.0)), paths[i:i + 16]) for i in range(0, n, 16)]


def _weighted(n, rng):
    """wcorr: n pairs and the 1025 weights"""
    return _pairs(n, rng), rng.uniform(0.5, 1.5, 1025).astype(np.float32)


def _jobs(n, rng):
    """mf: n (row, set) jobs"""
    return [(int(r), int(s)) for r, s in zip(rng.integers(0, NM, n), rng.integers(0, N_SETS, n))]


def _channels(n, rng):
    """iir, ddc, duc: n output rows (iir reads the first two arrays only)"""
    return dict(row_map=rng.integers(0, NM, n).astype(np.uint32), set_index=rng.integers(0, N_SETS, n).astype(np.uint32),
                steps=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), phases=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))


def _next_row(r):
    return (int(r) + 1) % NM


# a table of the same length that differs from t in EVERY record and is as valid: the rows move on by one (mod 8), the
# parameters of link and scene by a fixed amount inside their ranges
_OTHER = {
    "pairs": lambda t: [(_next_row(a), b) for a, b in t],
    "beams": lambda t: [[(_next_row(m), w, d) for m, w, d in beam] for beam in t],
    "lines": lambda t: [(_next_row(m), d, p) for m, d, p in t],
    "streams": lambda t: (t[0], t[1] + 1.5, t[2] * 0.75, t[3], t[4]),
    "mics": lambda t: [(s, [(tx, g * 0.75, ld + 1.5, p) for tx, g, ld, p in paths]) for s, paths in t],
    "weighted": lambda t: ([(_next_row(a), b) for a, b in t[0]], t[1]),
    "jobs": lambda t: [(_next_row(r), s) for r, s in t],
    "channels": lambda t: dict(t, row_map=((t["row_map"] + 1) % NM).astype(np.uint32)),
}


# ---------------------------------------------------------------------------------------------------------- the libraries

def _sets(name, which):
    """the coefficient set S1 (which = 0) or S2 (1) of a library with a setter: same shapes, other values throughout"""
    rng = np.random.default_rng(700 + which)
    if name == "spec":
        return rng.uniform(0.5, 1.0, 2048).astype(np.float32)
    if name == "mf":
        return (rng.standard_normal((N_SETS, 33)) + 1j * rng.standard_normal((N_SETS, 33))).astype(np.complex64)
    if name == "iir":
        from uchirp import iir
        return np.stack([iir.dc_block_sections(44100.0, c, order=4) for c in rng.uniform(50.0, 5000.0, N_SETS)])
    if name == "ddc":
        return rng.uniform(-0.1, 0.1, (N_SETS, 21)).astype(np.float32)
    if name == "duc":
        return rng.uniform(-0.5, 0.5, (N_SETS, 9 * 2)).astype(np.float32)
    return [0, 2, 5, 7], rng.uniform(0.1, 0.5, 4).astype(np.float32), rng.uniform(-20.0, 20.0, (40, 4))       # scan: 40 beams of 4 taps


class _Lib:
    """One library: `make(which)` a fresh object (with the set S1 or S2, if it has a setter), `set(obj, which)` its setter,
    `table(n, rng)` / `other(t)` its argument table, `call(obj, x, t)` the tuple of tensors one call writes (t None: the call
    that names no host array), `refused(obj, x)` a call that the library must refuse with -EINVAL."""

    def __init__(self, name):
        import importlib
        self.name = name
        self.mod = m = importlib.import_module("uchirp." + name)
        self.set = None
        kind = None
        if name == "link":
            kind, self.table = "streams", _streams
            self.make = lambda which=0: m.Link()
            self.call = lambda o, x, t: (o.transmit(*t, n_samples=NS, seed=5),)
            self.refused = lambda o, x: o.transmit(["Hi"], 0.0, 1000.0, -1.0, n_samples=NS)
        elif name == "scene":
            kind, self.table = "mics", _mics
            self.make = lambda which=0: m.Scene()
            self.call = lambda o, x, t: (o.render(["Hi"], t, n_samples=NS, seed=5),)
            self.refused = lambda o, x: o.render(["Hi"], [(-1.0, [(0, 1000.0, 0.0, 0.0)])], n_samples=NS)
        elif name == "array":
            kind, self.table = "beams", _beams
            self.make = lambda which=0: m.Array()
            self.call = lambda o, x, t: (o.combine(x, t),)
            self.refused = lambda o, x: o.combine(x, [[(NM, 1.0, 0.0)]])
        elif name in ("align", "xcorr"):
            kind, self.table = "pairs", _pairs
            self.make = lambda which=0: (m.Aligner if name == "align" else m.Xcorr)()
            self.call = lambda o, x, t: (o.correlate(x, t, max_lag=L),)
            self.refused = lambda o, x: o.correlate(x, [(NM, 0)], max_lag=L)
        elif name == "wcorr":
            kind, self.table = "weighted", _weighted
            self.make = lambda which=0: m.Wcorr()
            self.call = lambda o, x, t: (o.correlate(x, t[0], max_lag=L, weights=t[1]),)
            self.refused = lambda o, x: o.correlate(x, [(NM, 0)], max_lag=L)
        elif name == "retime":
            kind, self.table = "lines", _lines
            self.make = lambda which=0: m.Retimer()
            self.call = lambda o, x, t: (o.rows(x, t),)
            self.refused = lambda o, x: o.rows(x, [(NM, 0.0, 0.0)])
        elif name == "track":
            kind, self.table = "pairs", _pairs
            self.make = lambda which=0: m.Tracker()
            self.call = lambda o, x, t: o.windows(x, t, window_len=NS, n_windows=1, max_lag=L, corr=True)
            self.refused = lambda o, x: o.windows(x, [(NM, 0)], window_len=NS, n_windows=1, max_lag=L, corr=True)
        elif name == "mf":
            kind, self.table = "jobs", _jobs
            self.make = lambda which=0: m.Mf(_sets(name, which))
            self.set = lambda o, which: o.set_templates(_sets(name, which))
            # (a setter case compares the outputs alone: half of a record's words are counts that no template moves)
            self.call = lambda o, x, t: o.run(x, t, out="real") if t is not None else (o.run(x, out="real", records=False)[0],)
            self.refused = lambda o, x: o.run(x, [(NM, 0)], out="real")
        elif name == "iir":
            kind, self.table = "channels", _channels
            self.make = lambda which=0: m.Iir(_sets(name, which))
            self.set = lambda o, which: o.set_sections(_sets(name, which))
            self.call = lambda o, x, t: o.run(x, row_map=t["row_map"], set_index=t["set_index"]) if t is not None else o.run(x)
            self.refused = lambda o, x: o.run(x, row_map=[NM])
        elif name == "ddc":
            kind, self.table = "channels", _channels
            self.make = lambda which=0: m.Ddc(_sets(name, which), 3)
            self.set = lambda o, which: o.set_taps(_sets(name, which), 3)
            # (without steps the carrier stands still and every Q is 0 under any taps: the call without host arrays stores I alone)
            self.call = lambda o, x, t: o.run(x, **t) if t is not None else o.run(x, out="i")
            self.refused = lambda o, x: o.run(x, row_map=[NM])
        elif name == "duc":
            # (the 4096 floats of a row are 2048 I, Q pairs)
            kind, self.table = "channels", _channels
            self.make = lambda which=0: m.Duc(_sets(name, which), 2)
            self.set = lambda o, which: o.set_taps(_sets(name, which), 2)
            self.call = lambda o, x, t: o.run(x, **t) if t is not None else o.run(x)
            self.refused = lambda o, x: o.run(x, row_map=[NM])
        elif name == "rate":
            self.make = lambda which=0: m.Converter(0, 3, 2)
            self.call = lambda o, x, t: (o.convert(x),)
        elif name == "spec":
            def make(which=0):
                o = m.Analyser()
                o.set_window(_sets(name, which))
                return o
            self.make = make
            self.set = lambda o, which: o.set_window(_sets(name, which))
            self.call = lambda o, x, t: (o.spectra(x, hop=512),)
        elif name == "mic":
            self.make = lambda which=0: m.Mic(1.0)
            self.call = lambda o, x, t: o.modulate(x)
        else:
            def make(which=0):
                o = m.Scanner()
                o.set_beams(*_sets(name, which))
                return o
            self.make = make
            self.set = lambda o, which: o.set_beams(*_sets(name, which))
            self.call = lambda o, x, t: o.power(x, 64, 1000, n_windows=3)
        self.other = _OTHER.get(kind)
        self.error = next(v for k, v in vars(m).items() if k.endswith("Error") and isinstance(v, type) and v.__module__ == m.__name__)


# ---------------------------------------------------------------------------------------------------------------- helpers

def _bits(out):
    return [o.cpu().numpy().tobytes() for o in out]


def _alone(lib, x, t, stream, which=0, arrays=False):
    """the call alone on a fresh object with a synchronise behind it: the bytes of every tensor it writes (with `arrays`
    the host copies themselves, in front of the bytes)"""
    import torch
    obj = lib.make(which)
    with torch.cuda.stream(stream):
        out = lib.call(obj, x, t)
    stream.synchronize()
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in out]
    want = [h.tobytes() for h in host]
    obj.close()
    assert all(len(b) > 0 and any(b) for b in want), "%s: the call alone wrote nothing" % lib.name
    return (host, want) if arrays else want


def _clock_khz():
    """The device's clock rate in kHz, the unit torch.cuda._sleep counts in: torch's device properties where they carry it,
    else hipDeviceAttributeClockRate asked of the HIP runtime the process already has (through a library of ours that
    links it)."""
    import ctypes as C
    import torch
    khz = getattr(torch.cuda.get_device_properties(0), "clock_rate", None)
    if not khz:
        from uchirp import spec
        value = C.c_int(0)
        rc = spec.lib().hipDeviceGetAttribute(C.byref(value), 5, 0)      # 5: hipDeviceAttributeClockRate
        assert rc == 0 and value.value > 0, "hipDeviceGetAttribute: rc %d, %d kHz" % (rc, value.value)
        khz = value.value
    return int(khz)


class _Hold:
    """Stream A kept busy for roughly HOLD_MS: everything enqueued on A behind it is pending while `pending()` is true."""

    def __init__(self, stream):
        import torch
        self.stream = stream
        khz = _clock_khz()                                               # cycles per millisecond
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.t0.record()
            torch.cuda._sleep(int(khz * HOLD_MS))
            self.t1.record()

    def must_be_pending(self, where):
        assert not self.t1.query(), "hold too short: it had ended %s" % where

    def finish(self, name):
        """with everything synchronised: the measured length, which must not look like a hang"""
        ms = self.t0.elapsed_time(self.t1)
        print("%s: the hold on stream A lasted %.2f ms" % (name, ms))
        assert ms < HOLD_MAX_MS, "the hold lasted %.1f ms" % ms


def _report(name, labels, got, want):
    for label, g, w in zip(labels, got, want):
        print("%s: %s, %s bytes written: %s" % (name, label, [len(b) for b in w], "same bits" if g == w else "DIFFERENT"))
    assert got == want


# ------------------------------------------------------------------------------------------------- (a) one stream, 7 more

@pytest.mark.parametrize("name", ["link", "scene", "wcorr", "mf", "iir", "ddc", "duc"])
def test_back_to_back_calls_of_the_other_staging_libraries(name, rows):
    """The recipe of test_gpu_staging.py: slot 0 is staged again while call 0 may be in flight, slot 1 grows for the 2000
    records while the kernel of call 1 may still read it.  (Every size is the recipe's.  wcorr stages its 1025 weights with
    the pairs, 4100 bytes, so its slots start at 8192 bytes, not 4096: slot 1 takes 16384 for the 600 pairs and grows to
    65536 for the 2000.)  iir, ddc and duc: a call that names no host array stands between the staged ones, in front and
    behind; only a staged call may move on to the other slot, or the 2000 records would land in slot 0."""
    import torch
    lib = _Lib(name)
    tables = [lib.table(n, np.random.default_rng(100 + i)) for i, n in enumerate(SIZES)]
    labels = ["call %d, %d records" % (i, n) for i, n in enumerate(SIZES)]
    if name in ("iir", "ddc", "duc"):
        tables = [None, tables[0], None, tables[1], tables[2], None, None, tables[3], None]
        labels = ["call %d, %s" % (i, "no host array" if t is None else "%d records" % len(t["row_map"])) for i, t in enumerate(tables)]
    stream = torch.cuda.Stream()
    want = [_alone(lib, rows, t, stream) for t in tables]
    obj = lib.make()
    with torch.cuda.stream(stream):
        outs = [lib.call(obj, rows, t) for t in tables]          # nothing waits in between
    stream.synchronize()
    got = [_bits(out) for out in outs]
    obj.close()
    _report(name, labels, got, want)


# ------------------------------------------------------------------------------------------------------- (b) two streams

@pytest.mark.parametrize("name", STAGING)
def test_calls_on_two_streams_equal_the_calls_alone(name, rows):
    """Call 0 (A, slot 0, 2000 records: the most work the rows give, pending behind the hold), call 1 (B, slot 1, 3 records),
    a refused call (enqueues nothing, leaves the slot), call 2 (B, slot 0 again, with a table that differs from call 0's in
    every record; its host side waits in stage_begin until call 0's copy has run, that is until the hold ends, and its copy
    waits on B for call 0's kernel on A), call 3 (A, slot 1, 600 records: the slot grows).  Both tables of slot 0 are valid
    for both calls, so a broken order can only give wrong numbers."""
    import torch
    lib = _Lib(name)
    t0 = lib.table(SIZES[3], np.random.default_rng(200))
    tables = [t0, lib.table(SIZES[0], np.random.default_rng(201)), lib.other(t0), lib.table(SIZES[1], np.random.default_rng(203))]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    want = [_alone(lib, rows, t, a) for t in tables]
    assert want[0] != want[2], "the two tables of slot 0 give the same outputs"
    obj = lib.make()
    hold = _Hold(a)
    with torch.cuda.stream(a):
        out0 = lib.call(obj, rows, tables[0])
    with torch.cuda.stream(b):
        out1 = lib.call(obj, rows, tables[1])
        hold.must_be_pending("after call 1")
        with pytest.raises(lib.error, match=r"rc=-22"):
            lib.refused(obj, rows)
        out2 = lib.call(obj, rows, tables[2])                    # blocks the host until the hold ends: the design
    with torch.cuda.stream(a):
        out3 = lib.call(obj, rows, tables[3])
    a.synchronize()
    b.synchronize()
    hold.finish(name)
    got = [_bits(out) for out in (out0, out1, out2, out3)]
    obj.close()
    _report(name, ["call 0 on A", "call 1 on B", "call 2 on B", "call 3 on A"], got, want)


# --------------------------------------------------------------------------------------------------------- (c) the setters

@pytest.mark.parametrize("name", SETTERS)
def test_setter_waits_for_the_runs_pending_on_another_stream(name, rows):
    """Run 1 (A, set S1, pending behind the hold), run 2 (B, S1, finished), the setter with S2, run 3 (B, S2).  Nothing of
    run 2 or run 3 is ordered behind run 1: only the setter's own wait keeps S2 away from it.  The outputs under S1 and S2
    differ in every element of the first tensor a call writes (asserted), so a run that read the other set, or half of
    each, cannot pass."""
    import torch
    lib = _Lib(name)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    (host1, want1), (host2, want2) = _alone(lib, rows, None, a, 0, arrays=True), _alone(lib, rows, None, a, 1, arrays=True)
    assert host1[0].shape == host2[0].shape and (host1[0] != host2[0]).all(), "S1 and S2 agree in %d of %d elements" % (
        int((host1[0] == host2[0]).sum()), host1[0].size)
    obj = lib.make(0)
    hold = _Hold(a)
    with torch.cuda.stream(a):
        out1 = lib.call(obj, rows, None)
    with torch.cuda.stream(b):
        out2 = lib.call(obj, rows, None)
    b.synchronize()
    hold.must_be_pending("in front of the setter")
    lib.set(obj, 1)                                              # may block until the hold ends
    with torch.cuda.stream(b):
        out3 = lib.call(obj, rows, None)
    a.synchronize()
    b.synchronize()
    hold.finish(name)
    got = [_bits(out) for out in (out1, out2, out3)]
    obj.close()
    _report(name, ["run 1 on A under S1", "run 2 on B under S1", "run 3 on B under S2"], got, [want1, want1, want2])


# ----------------------------------------------------------------------------------------------------------- (d) destroy

@pytest.mark.parametrize("name", STAGING + UNSTAGED)
def test_close_waits_for_the_call_pending(name, rows):
    """One call on the held stream A, then close() at once: destroy frees what the pending call reads (the staging pair, the
    unit sums, the tables and coefficient sets), so it has to wait for it.  (The microphone model owns no device memory and
    does not wait.)"""
    import torch
    lib = _Lib(name)
    table = lib.table(SIZES[1], np.random.default_rng(300)) if name in STAGING else None
    a = torch.cuda.Stream()
    want = _alone(lib, rows, table, a)
    obj = lib.make()
    hold = _Hold(a)
    with torch.cuda.stream(a):
        out = lib.call(obj, rows, table)
    hold.must_be_pending("after the call")
    obj.close()
    a.synchronize()
    hold.finish(name)
    _report(name, ["the call on A"], [_bits(out)], [want])
