"""The condition the caps of tests/test_gpu_receive_oracle.py rest on, checked without a GPU: on the very inputs of those legs the
float32 oracle, judged against the float64 oracle by the legs' own rule (receive_oracle_util.judge: classify_divergence on the
first differing block), stays inside `bad == 0 and soft <= 3`, the float64 oracle decodes at least 1000 of the 1024 messages
(the same share of the wide inputs), its traces visit all four states, and float32 round-off stays inside the snr bar.
A receiver that computes in float32 as the reference does therefore has the whole cap for itself: the cap is no artefact of the
reference or of these inputs."""
import numpy as np
import pytest

from oracle import uco
import receive_oracle_util as u


def _check(label, variant, x, msgs, **kw):
    r64 = u.oracle_many(variant, x, **kw)
    r32 = u.oracle_many(variant, x, precision=uco.F32, **kw)
    res = u.judge(label, ((s, r32[s][0], r32[s][1]) for s in range(x.shape[0])), r64, msgs)
    states = np.unique(np.concatenate([r[1]["state_before"] for r in r64]))
    print("%s: states visited %s" % (label, states.tolist()))
    assert res["bad"] == 0 and res["soft"] <= 3
    assert res["decoded"] >= u.decoded_floor(x.shape[0])
    assert states.tolist() == [0, 1, 2, 3]
    assert res["snr_ok"] and res["snr_blocks"] > 0          # (the worst ratio is printed: well under 1 % of the bar)


@pytest.mark.parametrize("variant", [uco.RX_REAL, uco.SYNC_CPLX])
def test_float32_oracle_equals_float64_oracle_on_the_1024_streams(variant):
    x, msgs = u.transmissions()
    assert x.shape == (u.STREAMS, u.BLOCKS * u.N)
    _check("seed %d variant %d, F32 oracle against F64 oracle" % (u.SEED, variant), variant, x, msgs)


@pytest.mark.parametrize("variant", [uco.RX_REAL, uco.SYNC_CPLX])
def test_float32_oracle_equals_float64_oracle_on_the_wide_streams(variant):
    x, msgs = u.wide_transmissions()
    o = uco.Oracle(variant, **u.WIDE_KW)
    assert o.bandwidth2 == 294
    _check("wide windows variant %d, F32 oracle against F64 oracle" % variant, variant, x, msgs, **u.WIDE_KW)
