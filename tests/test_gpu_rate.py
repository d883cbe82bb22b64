"""The rate converter on the GPU (uc_rate_convert, uchirp/rate.py): every ratio and both formats against the float64 model,
the table bit for bit through combs of ones, bit-identity under every way of cutting the work, guards, the contract of the
call, and end to end into the receivers of libuchirp.so, recorded and live.

Bound of the model test: an output is T float coefficients, one product and T - 1 fused multiply-adds.  The model keeps h in
float64; the device rounds each coefficient once (half an ulp, 2^-24 relative, of an h whose product with x is one term of
sum |h x|) and each of the T steps of the chain once (half an ulp of a partial sum that sum |h x| bounds), so
|gpu - model| <= (T + 1) * 2^-24 * sum |h x| per sample.  It is not tuned to what the kernel gives.  Every test prints its
figures before it asserts (pytest -s)."""
import ctypes as C
import errno

import numpy as np
import pytest

import rate_util as ru

pytestmark = pytest.mark.gpu

N = 2048
NR, NS = 5, 1500
# (up, down, half, taps)
RATIOS = ((3125, 1764, 24, 49), (625, 384, 24, 49), (625, 768, 24, 59), (3, 2, 24, 49), (2, 3, 24, 73), (7, 5, 4, 9), (5, 13, 24, 125))


@pytest.fixture(scope="module")
def rate():
    from uchirp import rate as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def rows():
    """5 rows x 1500 samples, as floats and as PCM words (device tensors and host copies); made once and never written."""
    import torch
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((NR, NS)) * 1000.0).astype(np.float32)
    w = rng.integers(-2 ** 15, 2 ** 15, size=(NR, NS)).astype(np.int16)
    w[:, :6] = [0, 1, -1, 2 ** 15 - 1, -2 ** 15, 77]
    return {"f32": (torch.from_numpy(f).to("cuda:0"), f), "i16": (torch.from_numpy(w).to("cuda:0"), w)}


def _bits(t):
    import torch
    return t.view(torch.int32)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _ratio(rate, got, x, up, down, half, taps, **kw):
    """worst |gpu - model| / bound over one call's outputs"""
    want = rate.model(x, up, down, half, **kw)
    mag = rate.model(x, up, down, half, magnitude=True, **kw)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = (taps + 1) * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - want)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0, float(np.abs(want).max()) if want.size else 0.0


@pytest.mark.parametrize("up,down,half,taps", RATIOS)
def test_every_ratio_within_the_bound_of_the_model(rate, rows, up, down, half, taps):
    import torch
    cv = rate.Converter(0, up, down, half)
    assert cv.info.taps == taps
    worst = 0.0
    for name, (dev, host) in rows.items():
        # whole rows from sample 0
        r, peak = _ratio(rate, cv.convert(dev).cpu().numpy(), host, up, down, half, taps)
        assert peak > 100.0
        worst = max(worst, r)
        # rows that start at an odd sample; outputs from before the rows' first contribution to behind their last
        in_first = 2001
        c = cv.info.centre                                                 # k(m) = (m down + c) div up
        m_lo, m_hi = -(-(in_first * up - c) // down) - 10, -(-((in_first + NS + taps - 1) * up - c) // down) + 10
        kw = dict(in_first=in_first, out_first=m_lo, n_out=m_hi - m_lo)
        got = cv.convert(dev, **kw).cpu().numpy()
        assert not got[:, :5].any() and not got[:, -5:].any() and np.abs(got).max() > 100.0
        worst = max(worst, _ratio(rate, got, host, up, down, half, taps, **kw)[0])
        # one, T - 1 and T input samples; one output sample
        for n_in in (1, taps - 1, taps):
            kw = dict(in_first=in_first, out_first=m_lo, n_out=(n_in + 2 * taps) * up // down + 20)
            got = cv.convert(dev[:, 40:40 + n_in], **kw).cpu().numpy()
            assert got.any()
            worst = max(worst, _ratio(rate, got, host[:, 40:40 + n_in], up, down, half, taps, **kw)[0])
        for m in (0, 1, 700, NS * up // down - 1):
            got = cv.convert(dev, out_first=m, n_out=1).cpu().numpy()
            worst = max(worst, _ratio(rate, got, host, up, down, half, taps, out_first=m, n_out=1)[0])
        # strided rows on both sides (odd pitches)
        xs = torch.zeros((NR, NS + 131), dtype=dev.dtype, device="cuda:0")[:, 3:3 + NS]
        xs.copy_(dev)
        n_out = rate.count(cv.info, NS)
        ys = torch.full((NR, n_out + 57), 7.0, dtype=torch.float32, device="cuda:0")
        cv.convert(xs, out=ys[:, 1:1 + n_out])
        worst = max(worst, _ratio(rate, ys[:, 1:1 + n_out].cpu().numpy(), host, up, down, half, taps)[0])
    print("%d / %d, half %d, T = %d: worst |gpu - model| / bound %.4f over both formats and every shape" % (up, down, half, taps, worst))
    assert worst <= 1.0, worst
    cv.close()


def test_combs_of_ones_read_every_table_entry_exactly(rate):
    """Row r is 1 at the samples i with i mod T = r: under every output lies exactly one 1, at tap j = (k - r) mod T, so the
    output IS the float C[p][j] (every other product is an exact zero).  Outputs of one whole period and T rows cover every
    (p, j) of the 3125 x 49 table."""
    import torch
    cv = rate.Converter.for_rates(44100)
    i = cv.info
    up, down, T = i.up, i.down, i.taps
    assert (up, down, T) == (3125, 1764, 49)
    out_first, n_out = up, up + 75                                       # behind the first T samples: no tap reads in front of sample 0
    lo, hi = rate.span(i, out_first, n_out)
    assert lo >= 0
    comb = (np.arange(hi)[None, :] % T == np.arange(T)[:, None]).astype(np.int16)
    got = cv.convert(torch.from_numpy(comb).to("cuda:0"), out_first=out_first, n_out=n_out).cpu().numpy()
    table = rate.table(i)
    m = np.arange(out_first, out_first + n_out, dtype=np.int64)
    k, p = np.divmod(m * down + i.centre, up)
    j = (k[None, :] - np.arange(T)[:, None]) % T                          # [row, output]
    want = table[p[None, :], j]
    differ = int((got != want).sum())                                     # as floats: a zero entry may come out as -0.0f
    seen = np.zeros((up, T), bool)
    seen[np.broadcast_to(p[None, :], j.shape), j] = True
    print("combs: %d outputs, %d differ from their table entry; %d of %d entries read" % (got.size, differ, int(seen.sum()), seen.size))
    assert seen.all() and differ == 0 and np.array_equal(got, want)
    cv.close()


@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("up,down,half", [(3125, 1764, 24), (625, 768, 24), (5, 13, 24)])
def test_cuts_grids_calls_rows_and_far_samples_give_the_same_bits(rate, rows, uc_tuning, monkeypatch, fmt, up, down, half):
    import torch
    x, _ = rows[fmt]
    cv = rate.Converter(0, up, down, half)
    i = cv.info
    n_out = rate.count(i, NS) + 40
    whole = cv.convert(x, n_out=n_out)
    assert float(whole.abs().max()) > 100.0 and whole.dtype == torch.float32 and tuple(whole.shape) == (NR, n_out)
    tile = rate.tile_outputs(i)
    assert n_out > tile + 1
    # the output range cut into two calls, and into calls of 65 samples
    for cut in (1, 63, 64, 65, tile - 1, tile, tile + 1):
        y = torch.zeros_like(whole)
        cv.convert(x, out_first=0, out=y[:, :cut])
        cv.convert(x, out_first=cut, out=y[:, cut:])
        assert _same_bits(y, whole), cut
    y = torch.zeros_like(whole)
    for a in range(0, n_out, 65):
        b = min(a + 65, n_out)
        lo, hi = rate.span(i, a, b - a)                                    # the input handed over as the window that `span` names
        lo = min(max(lo, 0), NS - 1)                                       # (behind the rows: their last sample, which nothing reads)
        cv.convert(x[:, lo:max(min(hi, NS), lo + 1)], in_first=lo, out_first=a, out=y[:, a:b])
    assert _same_bits(y, whole)
    # launch geometry: 1 .. 5 workgroups (UC_RATE_GRID, read under UC_TUNING=1 when the object is created)
    for grid in range(1, 6):
        monkeypatch.setenv("UC_RATE_GRID", str(grid))
        c2 = rate.Converter(0, up, down, half)
        assert _same_bits(c2.convert(x, n_out=n_out), whole), grid
        c2.close()
    monkeypatch.delenv("UC_RATE_GRID")
    # calls in a row, not synchronised in between; rows as a sub-matrix (another row block, another pairing of the rows)
    outs = [cv.convert(x, n_out=n_out) for _ in range(3)]
    sub = cv.convert(x[1:4], n_out=n_out)
    last = cv.convert(x[4:5], n_out=n_out)
    torch.cuda.synchronize()
    assert all(_same_bits(o, whole) for o in outs) and _same_bits(sub, whole[1:4]) and _same_bits(last, whole[4:5])
    # 21 rows: two row blocks, the second with 5 rows
    many = cv.convert(x.repeat(5, 1)[:21].contiguous(), n_out=n_out)
    assert _same_bits(many, whole.repeat(5, 1)[:21])
    # whole periods further on: out_first + a up with in_first + a down are the same positions; the a that puts the range's
    # end within one period of 2^38
    a = (2 ** 38 - n_out) // i.up
    assert 2 ** 38 - i.up < a * i.up + n_out <= 2 ** 38
    far = cv.convert(x, in_first=a * i.down, out_first=a * i.up, n_out=n_out)
    assert _same_bits(far, whole)
    end = cv.convert(x, in_first=2 ** 38 * i.down // i.up - NS + 3, out_first=2 ** 38 - 5, n_out=5)      # the last samples there are
    assert end.shape == (NR, 5)
    cv.close()


@pytest.mark.parametrize("fmt", ["f32", "i16"])
def test_guards_gaps_and_ends(rate, rows, fmt):
    import torch
    x, h = rows[fmt]
    cv = rate.Converter.for_rates(48000)
    n_out = rate.count(cv.info, NS) + 100
    whole = cv.convert(x, n_out=n_out)
    # input rows with gaps of NaN (PCM: of the largest word) between them and around them; output rows with guard values
    big = torch.full((NR + 2, NS + 131), float("nan") if fmt == "f32" else 2 ** 15 - 1, dtype=x.dtype, device="cuda:0")
    xs = big[1:1 + NR, 67:67 + NS]
    xs.copy_(x)
    ys = torch.full((NR + 2, n_out + 57), 7.0, dtype=torch.float32, device="cuda:0")
    cv.convert(xs, out=ys[1:1 + NR, 5:5 + n_out])
    got = ys[1:1 + NR, 5:5 + n_out]
    assert not bool(torch.isnan(got).any()) and _same_bits(got, whole)
    ys[1:1 + NR, 5:5 + n_out] = 7.0
    assert float(ys.min()) == 7.0 == float(ys.max())
    # outputs whose T samples all lie behind the row are zero
    lo = np.array([rate.span(cv.info, m, 1)[0] for m in range(n_out - 100, n_out)])
    g = whole.cpu().numpy()[:, n_out - 100:]
    assert (lo >= NS).sum() >= 20 and not g[:, lo >= NS].any() and g[:, lo < NS - 1].any()
    cv.close()


@pytest.fixture
def other_device():
    """The calling thread's current device while the object lives on device 0: device 1 where the machine has one, so that
    an entry point that left the object's device current would be seen."""
    import torch
    before = torch.cuda.current_device()
    cur = 1 if torch.cuda.device_count() > 1 else 0
    torch.cuda.set_device(cur)
    yield cur
    torch.cuda.set_device(before)


def test_contract(rate, rows, other_device):
    import torch
    L = rate.lib()
    x, h = rows["f32"]
    dev0 = other_device
    two = torch.cuda.device_count() >= 2
    if not two:
        print("contract: one GPU visible: the two-GPU branch (current device != the object's, memory of another device) did not run")
    cv = rate.Converter(0, 3, 2)
    assert torch.cuda.current_device() == dev0
    no = rate.count(cv.info, NS)
    want = cv.convert(x)
    torch.cuda.synchronize()
    out = torch.full((NR, no), 7.0, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)

    def call(h_=None, in_ptr=x.data_ptr(), dtype=rate.DTYPE_F32, n_rows=NR, in_first=0, n_in=NS, in_stride=0, out_ptr=out.data_ptr(),
             out_first=0, n_out=no, out_stride=0):
        rc = L.uc_rate_convert(cv._h if h_ is None else h_, C.c_void_p(in_ptr), dtype, n_rows, in_first, n_in, in_stride,
                               C.c_void_p(out_ptr), out_first, n_out, out_stride, stream)
        assert torch.cuda.current_device() == dev0
        return rc

    host = np.zeros(NR * no, np.float32)
    refusals = [("out_first + n_out > 2^38", dict(out_first=2 ** 38 - no + 1)), ("out_first > 2^38", dict(out_first=2 ** 38 + 1)),
                ("out_first + n_out wraps", dict(out_first=2 ** 64 - 5)),
                ("in_stride < n_in", dict(in_stride=NS - 1)), ("out_stride < n_out", dict(out_stride=no - 1)),
                ("dtype 2", dict(dtype=2)), ("dtype -1", dict(dtype=-1)),
                ("no rows", dict(n_rows=0)), ("no input samples", dict(n_in=0)), ("no output samples", dict(n_out=0)),
                ("in NULL", dict(in_ptr=None)), ("out NULL", dict(out_ptr=None)),
                ("in: host memory", dict(in_ptr=host.ctypes.data)), ("out: host memory", dict(out_ptr=host.ctypes.data)),
                ("out overlaps in", dict(out_ptr=x.data_ptr() + 4 * NS)),
                ("out overlaps the end of in", dict(out_ptr=x.data_ptr() + 4 * (NR * NS - 1))),
                ("in overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (NR * no - 1))),
                ("in (as PCM) overlaps the end of out", dict(in_ptr=out.data_ptr() + 4 * (NR * no - 1), dtype=rate.DTYPE_I16))]
    if two:
        far_in = torch.zeros((NR, NS), dtype=torch.float32, device="cuda:1")
        far_out = torch.zeros((NR, no), dtype=torch.float32, device="cuda:1")
        refusals += [("in: memory of another device", dict(in_ptr=far_in.data_ptr())), ("out: memory of another device", dict(out_ptr=far_out.data_ptr()))]
    for name, kw in refusals:
        rc = call(**kw)
        assert rc == -errno.EINVAL, (name, rc)
        assert L.uc_rate_last_error(), name
        torch.cuda.synchronize()
        assert float(out.min()) == 7.0 == float(out.max()), name          # nothing was enqueued
        assert call() == 0, name                                          # and the object is as usable as before
        torch.cuda.synchronize()
        assert _same_bits(out, want), name
        out.fill_(7.0)
    assert call(h_=C.c_void_p(None)) == -errno.EINVAL
    assert call(out_first=2 ** 38 - no) == 0                              # the last range there is
    h2 = C.c_void_p()
    assert L.uc_rate_create(torch.cuda.device_count(), 3, 2, 24, 9.0, C.byref(h2)) == -errno.ENODEV and not h2.value
    assert L.uc_rate_create(0, 3, 2, 24, 9.0, None) == -errno.EINVAL
    for bad in ((5, 5, 24, 9.0), (0, 2, 24, 9.0), (3, 2, 3, 9.0), (3, 2, 24, float("nan")), (1, 16, 4, 9.0), (4097, 4096, 24, 9.0)):
        assert L.uc_rate_create(0, *bad, C.byref(h2)) == -errno.EINVAL and not h2.value, bad
    assert torch.cuda.current_device() == dev0
    torch.cuda.synchronize()
    cv.close()
    assert torch.cuda.current_device() == dev0


def test_c_host_reads_the_table_through_one_sounding_sample(rate, tmp_path):
    import re
    import subprocess
    from test_rate_cpu import build_host
    out = subprocess.run([build_host(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    n, sounding, equal = [int(v) for v in re.search(r"(\d+) outputs, (\d+) under the sample that sounds, (\d+) equal", out.stdout).groups()]
    assert n == 3125 == equal and 80 <= sounding <= 90


# ---- end to end: sound-card recordings into the receivers

def test_fifteen_recordings_decode_after_the_conversion_on_the_gpu(rate, uchirp):
    """The 15 int16 recordings of tests/test_rate_cpu.py (three rates, five texts each), converted in three calls, one per
    rate, the rows of a rate padded with silence to one length; then times 0.1 into the same noise and through
    uc_receive_streams, SYNC_CPLX: every text is the one sent."""
    import torch
    texts, skews = ru.texts(), ru.skews()
    eng = uchirp.Engine(uchirp.SYNC_CPLX)
    index, sent, streams = 0, [], []
    for fs in ru.RATES:
        cv = rate.Converter.for_rates(fs)
        pcm = [ru.pcm(t, fs) for t in texts[fs]]
        block = np.zeros((len(pcm), max(len(w) for w in pcm)), np.int16)
        for r, w in enumerate(pcm):
            block[r, :len(w)] = w
        y = cv.convert(torch.from_numpy(block).to("cuda:0")).cpu().numpy()
        for r, (t, w, skew) in enumerate(zip(texts[fs], pcm, skews[fs])):
            streams.append(ru.in_noise(y[r, :rate.count(cv.info, len(w))], skew, index))
            sent.append(t)
            index += 1
        cv.close()
    nb = max(len(s) for s in streams)
    x = np.zeros((len(streams), nb), np.float32)
    rng = np.random.default_rng(77)
    for r, s in enumerate(streams):
        x[r, :len(s)] = s
        x[r, len(s):] = ru.SIGMA * rng.standard_normal(nb - len(s))      # the shorter recordings go on as noise
    got, _ = eng.receive_many(torch.from_numpy(x).to("cuda:0"), want_trace=False)
    for t, g in zip(sent, got):
        print("sent %r, decoded %r" % (t, g))
    assert len(sent) == 15 and [g for g in got] == [t + "\n" for t in sent]
    eng.close()


def test_live_blocks_converted_into_the_ring_equal_the_recorded_run(rate, uchirp):
    """One 44.1 kHz recording (the waveform at a tenth of full scale in noise of sigma 5, as int16, behind the 30 blocks of
    noise a receiver needs to settle) converted block by block,
    out_first = 2048 b, from the input window `span` names, straight into the two ring buffers that live.next reads: text
    and traces equal those of the recorded run over the recording converted in one call."""
    import torch
    text = "Live @ 44.1k"
    rng = np.random.default_rng(9)
    w = ru.pcm(text, 44100)
    lead = 35000 + 333
    rec = ru.SIGMA * rng.standard_normal(lead + len(w) + 35000)
    rec[lead:lead + len(w)] += ru.GAIN * w
    rec = np.rint(rec).astype(np.int16)[None, :]
    xd = torch.from_numpy(rec).to("cuda:0")
    cv = rate.Converter.for_rates(44100)
    nb = rate.count(cv.info, rec.shape[1]) // N
    whole = cv.convert(xd, n_out=nb * N)
    eng = uchirp.Engine(uchirp.SYNC_CPLX)
    text_g, tr_g = eng.receive(whole.reshape(-1).contiguous())
    print("recorded run: %r over %d blocks" % (text_g, nb))
    assert text_g == text + "\n" and len(tr_g) == nb
    live = eng.live(1)
    live.keep_previous(True)
    ring = [torch.zeros((1, N), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    got, traces = "", []
    for b in range(nb):
        lo, hi = rate.span(cv.info, b * N, N)
        lo, hi = max(lo, 0), min(hi, rec.shape[1])
        cv.convert(xd[:, lo:hi], in_first=lo, out_first=b * N, out=ring[b % 2])
        t, tr = live.next(ring[b % 2])
        got += t[0]
        traces.append(tr[0])
    assert got == text_g
    assert np.array_equal(np.concatenate(traces).view(np.uint8), tr_g.view(np.uint8))
    live.close()
    eng.close()
    cv.close()
