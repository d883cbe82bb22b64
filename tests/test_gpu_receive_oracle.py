"""The default paths of the many-stream receiver against the oracle DIRECTLY: uco.Oracle(variant).receive(x, precision=F64,
busy=..., margins=True), the literal sequential main loop (receiver/Src/main.c:417-554), stream by stream.

tests/test_gpu_receive_many.py and tests/test_gpu_wide.py tie these paths bit for bit to the one-launch recorded call of the same
library, under the poison switch; only that call met the oracle, with a busy mask and below the stepping thresholds.  Here the
shipped configuration (UC_RX_POISON off, no knob unless a leg says so) meets the oracle itself, and no leg compares GPU with GPU:

  a. recorded calls served block by block by the shipped gate (1024 SYNC_CPLX streams; 8192 RX_REAL streams);
  b. the same path forced at 64 streams (UC_RX_STEP_MIN=1), float32 and int32 words;
  c. live receivers, one block per call, default contract -- the walk over the offsets the need word allows -- without and with
     busy masks;
  d. the same with uc_rx_state_keep_previous on a ring of two device buffers;
  e. the lane-per-stream replay kernel (more than 16 384 streams): one recorded call (stepped) and live, one block per call;
  f. the wide ROWS build (bandwidth2 = 294): recorded, live, live with kept chunks;
  g. a negative control: with every need word forced to the IDLE turn-0 set (UC_RX_NEED_FORCE=0x052, the pricing switch: wrong
     results by design) the same judge reports `bad` for the live leg and for the knob-less recorded call of (a) -- which therefore
     took the stepped path -- and nothing for 1023 streams, served in one launch, where need words are not used.

Inputs: receive_oracle_util.transmissions(), 1024 random transmissions of seed 2601; tests/test_receive_oracle_inputs.py pins on
the CPU that the float32 oracle equals the float64 oracle on every one of them, so the cap below is the receiver's alone.
Verdict of a leg (receive_oracle_util.judge, the rule of the 1000-transmission test): text, trace length and FIELDS equal the
oracle's, else the first differing block is judged by the oracle's own margin; `bad == 0 and soft <= 3` per distinct source
stream; on matching streams snr_up AND snr_down of the tracking blocks within rtol 1e-4 / atol 1e-3 of the oracle's.

Not here: the PDM live path (tests/test_dfsdm.py) and graph-replayed steps (the graph tests of tests/test_gpu_receive_many.py)."""
import functools

import numpy as np
import pytest

from oracle import uco
import receive_oracle_util as u
from receive_oracle_util import N, BLOCKS

pytestmark = pytest.mark.gpu

VARIANTS = [uco.SYNC_CPLX, uco.RX_REAL]
STEP_MIN = {uco.SYNC_CPLX: 1024, uco.RX_REAL: 8192}      # uc_receive_streams' shipped gate of the stepped path (uc_api_rx.cpp)
WAVE_STREAMS = 16384                                     # above: the lane-per-stream replay kernel (uc_rx_kernel.hip)
KNOBS = ("UC_TUNING", "UC_RX_POISON", "UC_RX_STEP_MIN", "UC_RX_NEED_FORCE", "UC_GRID", "UC_BAND_GROUP", "UC_STATIC_DEAL")


@pytest.fixture(scope="module")
def uchirp():
    import uchirp as m
    m.lib()
    return m


@pytest.fixture
def shipped(monkeypatch):
    """No experiment switch: what a context reads at creation is the shipped configuration."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@functools.lru_cache(maxsize=None)
def _reference(variant):
    """The float64 oracle over the 1024 streams, no busy mask: computed once, shared by the legs, never written to."""
    return u.oracle_many(variant, u.transmissions()[0])


@pytest.fixture(scope="module")
def xd512():
    """The first 512 streams on the device, shared by the live legs."""
    import torch
    xd = torch.tensor(u.transmissions()[0][:512], device="cuda:0")
    yield xd
    del xd
    torch.cuda.empty_cache()


def _verdict(res, sources=None, decoded=True):
    assert res["bad"] == 0 and res["soft"] <= 3, res
    assert res["snr_ok"] and res["snr_blocks"] > 0, res
    if sources is not None:
        assert res["sources"] == sources, res
    if decoded:
        assert res["decoded"] >= u.decoded_floor(res["sources"]), res


def _live(e, xd, blocks, busy=None, kept=False):
    """One block per call of live.next on device chunks -> [(stream, text, trace)].  kept: uc_rx_state_keep_previous, the
    chunks lie in a ring of two device buffers; else the chunk is read where it lies in xd (rows further apart than a chunk)."""
    import torch
    ns = int(xd.shape[0])
    live = e.live(ns)
    live.keep_previous(kept)
    ring = [torch.zeros((ns, N), dtype=xd.dtype, device=xd.device) for _ in range(2)] if kept else None
    texts, traces = [""] * ns, [[] for _ in range(ns)]
    for b in range(blocks):
        chunk = xd[:, b * N:(b + 1) * N]
        if kept:
            ring[b % 2].copy_(chunk)
            chunk = ring[b % 2]
        t, tr = live.next(chunk, busy=None if busy is None else np.ascontiguousarray(busy[:, b:b + 1]))
        for s in range(ns):
            texts[s] += t[s]
            traces[s].append(tr[s])
    live.close()
    return [(s, texts[s], np.concatenate(traces[s])) for s in range(ns)]


def _live_lanes(uchirp, e, xd, blocks, lanes):
    """One block per call with every buffer on the device (live.next_into), the outputs of `lanes` only brought to the host:
    -> [(lane, text, trace)]."""
    import torch
    dev = xd.device
    ns = int(xd.shape[0])
    pick = torch.as_tensor(list(lanes), device=dev)
    live = e.live(ns)
    text = torch.zeros((ns, 8), dtype=torch.uint8, device=dev)
    ntext = torch.zeros(ns, dtype=torch.int32, device=dev)
    trace = torch.zeros((ns, 1, uchirp.RX_EVENT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    ntrace = torch.zeros(ns, dtype=torch.int32, device=dev)
    nt, tt, ntr, trc = [], [], [], []
    for b in range(blocks):
        live.next_into(xd[:, b * N:(b + 1) * N], text, ntext, trace=trace, n_trace=ntrace)
        nt.append(ntext[pick].cpu().numpy())
        tt.append(text[pick].cpu().numpy())
        ntr.append(ntrace[pick].cpu().numpy())
        trc.append(trace[pick].cpu().numpy().reshape(len(pick), -1).view(uchirp.RX_EVENT_DTYPE)[:, 0])
    live.close()
    nt, tt, ntr, trc = np.stack(nt), np.stack(tt), np.stack(ntr), np.stack(trc)
    assert nt.max() <= 8 and ntr.max() <= 1
    out = []
    for k, lane in enumerate(lanes):
        txt = b"".join(bytes(tt[b, k, :nt[b, k]]) for b in np.nonzero(nt[:, k])[0])
        out.append((lane, txt.decode("latin-1"), trc[ntr[:, k] > 0, k]))
    return out


# ---- a. recorded, stepped by the shipped gate -----------------------------------------------------------------------------------

def test_recorded_sync_cplx_streams_served_block_by_block_by_default(uchirp, shipped):
    x, msgs = u.transmissions()
    busy = None
    assert x.shape[0] >= STEP_MIN[uco.SYNC_CPLX] and x.shape[1] // N > 1 and busy is None        # the stepped path's gate
    e = uchirp.Engine(uco.SYNC_CPLX)
    texts, traces = e.receive_many(x, busy=busy)
    e.close()
    res = u.judge("a. recorded SYNC_CPLX, 1024 streams (stepped)", zip(range(x.shape[0]), texts, traces), _reference(uco.SYNC_CPLX), msgs)
    _verdict(res, sources=1024)


def test_recorded_rx_real_streams_served_block_by_block_by_default(uchirp, shipped):
    import torch
    x, msgs = u.transmissions()
    many = torch.tensor(x, device="cuda:0").repeat(8, 1)
    busy = None
    assert many.shape[0] == 8192 >= STEP_MIN[uco.RX_REAL] and many.shape[1] // N > 1 and busy is None
    e = uchirp.Engine(uco.RX_REAL)
    texts, traces = e.receive_many(many, busy=busy)
    e.close()
    del many
    torch.cuda.empty_cache()
    res = u.judge("a. recorded RX_REAL, 8192 streams = 8 x 1024 (stepped)", ((k % 1024, texts[k], traces[k]) for k in range(8192)),
                  _reference(uco.RX_REAL), msgs)
    assert res["streams"] == 8192
    _verdict(res, sources=1024)


# ---- b. recorded, stepping forced at a small shape ------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_recorded_streams_stepped_at_a_small_shape(uchirp, shipped, variant):
    shipped.setenv("UC_TUNING", "1")
    shipped.setenv("UC_RX_STEP_MIN", "1")
    x, msgs = u.transmissions()
    x = x[:64]
    e = uchirp.Engine(variant)
    texts, traces = e.receive_many(x)
    res = u.judge("b. stepped (UC_RX_STEP_MIN=1) variant %d float32, 64 streams" % variant, zip(range(64), texts, traces),
                  _reference(variant), msgs)
    _verdict(res, sources=64)
    xi = u.words(x)
    texts, traces = e.receive_many(xi)
    e.close()
    res = u.judge("b. stepped (UC_RX_STEP_MIN=1) variant %d int32 words, 64 streams" % variant, zip(range(64), texts, traces),
                  u.oracle_many(variant, xi), msgs)
    _verdict(res, sources=64)


# ---- c. live, one block per call, default contract ------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_live_streams_one_block_per_call(uchirp, shipped, xd512, variant):
    _, msgs = u.transmissions()
    e = uchirp.Engine(variant)
    got = _live(e, xd512, BLOCKS)
    e.close()
    res = u.judge("c. live, one block per call, variant %d, 512 streams" % variant, got, _reference(variant), msgs)
    _verdict(res, sources=512)


@pytest.mark.parametrize("variant", VARIANTS)
def test_live_streams_one_block_per_call_with_busy_masks(uchirp, shipped, xd512, variant):
    x, msgs = u.transmissions()
    busy = u.busy_masks()[:256]
    assert busy.shape == (256, BLOCKS) and 64 <= int(busy.any(axis=1).sum()) <= 192          # about half of the streams drop blocks
    e = uchirp.Engine(variant)
    got = _live(e, xd512[:256], BLOCKS, busy=busy)
    e.close()
    ref = u.oracle_many(variant, x[:256], busy=busy)
    assert all(len(r[1]) == int((busy[s] == 0).sum()) for s, r in enumerate(ref))
    res = u.judge("c. live, one block per call, busy masks, variant %d, 256 streams" % variant, got, ref, msgs)
    _verdict(res, sources=256, decoded=False)


# ---- d. live, kept chunks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_live_streams_one_block_per_call_with_kept_chunks(uchirp, shipped, xd512, variant):
    _, msgs = u.transmissions()
    e = uchirp.Engine(variant)
    got = _live(e, xd512, BLOCKS, kept=True)
    e.close()
    res = u.judge("d. live, kept chunks (ring of two), variant %d, 512 streams" % variant, got, _reference(variant), msgs)
    _verdict(res, sources=512)


# ---- e. lane-per-stream replay --------------------------------------------------------------------------------------------------

def test_lane_per_stream_replay_recorded_and_live(uchirp, shipped, xd512):
    import torch
    _, msgs = u.transmissions()
    many = xd512.repeat(33, 1)
    ns = int(many.shape[0])
    assert ns == 16896 > WAVE_STREAMS and ns >= STEP_MIN[uco.RX_REAL]
    lanes = list(range(0, ns, 13))                       # 13 and 512 are coprime: every source stream is met
    assert len({k % 512 for k in lanes}) == 512
    e = uchirp.Engine(uco.RX_REAL)
    texts, traces = e.receive_many(many)
    res = u.judge("e. lane-per-stream replay, recorded (stepped), RX_REAL, every 13th of 16896 streams",
                  ((k % 512, texts[k], traces[k]) for k in lanes), _reference(uco.RX_REAL), msgs)
    assert res["streams"] == len(lanes)
    _verdict(res, sources=512)
    del texts, traces
    got = _live_lanes(uchirp, e, many, BLOCKS, lanes)
    e.close()
    del many
    torch.cuda.empty_cache()
    res = u.judge("e. lane-per-stream replay, live one block per call, RX_REAL, every 13th of 16896 streams",
                  ((k % 512, t, tr) for k, t, tr in got), _reference(uco.RX_REAL), msgs)
    _verdict(res, sources=512)


# ---- f. wide windows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_wide_windows_recorded_live_and_kept(uchirp, shipped, variant):
    """(tests/test_receive_oracle_inputs.py: on these 64 streams the float32 oracle equals the float64 oracle, 0 soft, 0 bad.)"""
    import torch
    x, msgs = u.wide_transmissions()
    ref = u.oracle_many(variant, x, **u.WIDE_KW)
    e = uchirp.Engine(variant, **u.WIDE_KW)
    assert e.bandwidth2 == 294
    texts, traces = e.receive_many(x)
    res = u.judge("f. wide windows, recorded, variant %d, 64 streams" % variant, zip(range(len(texts)), texts, traces), ref, msgs)
    _verdict(res, sources=u.WIDE_STREAMS)
    xd = torch.tensor(x, device="cuda:0")
    for kept in (False, True):
        got = _live(e, xd, u.WIDE_BLOCKS, kept=kept)
        res = u.judge("f. wide windows, live one block per call%s, variant %d, 64 streams" % (", kept chunks" if kept else "", variant),
                      got, ref, msgs)
        _verdict(res, sources=u.WIDE_STREAMS)
    e.close()


# ---- g. negative control --------------------------------------------------------------------------------------------------------

def test_forced_need_words_are_seen_by_these_legs(uchirp, shipped, xd512):
    """UC_RX_NEED_FORCE=0x052: every need word is the IDLE turn-0 set with the DOWN statistics off (bit 6 stays set, as the ROWS save
    path requires) -- a fast path that is WRONG and faults nothing.  The judge of the legs above must say so wherever need words are
    used, and only there."""
    shipped.setenv("UC_TUNING", "1")
    shipped.setenv("UC_RX_NEED_FORCE", "0x052")
    x, msgs = u.transmissions()
    ref = _reference(uco.SYNC_CPLX)
    e = uchirp.Engine(uco.SYNC_CPLX)
    got = _live(e, xd512[:64], BLOCKS)
    live = u.judge("g. control, live one block per call, 64 SYNC_CPLX streams, need words forced", got, ref, msgs)
    texts, traces = e.receive_many(x)
    stepped = u.judge("g. control, recorded 1024 SYNC_CPLX streams (no stepping knob), need words forced",
                      zip(range(1024), texts, traces), ref, msgs)
    texts, traces = e.receive_many(x[:1023])
    single = u.judge("g. control, recorded 1023 SYNC_CPLX streams (one launch), need words forced", zip(range(1023), texts, traces),
                     ref, msgs)
    e.close()
    print("g. control: bad live %d, stepped %d, one launch %d" % (live["bad"], stepped["bad"], single["bad"]))
    assert live["bad"] > 0
    assert stepped["bad"] > 0
    _verdict(single, sources=1023)
