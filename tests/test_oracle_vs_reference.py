"""Cross-check of the oracle against the reference's own outputs on random streams.

The inputs are rebuilt from seeds (tests/golden_util.py); what the reference made of them is stored
in tests/golden/reference_cases.npz (tests/golden/make_golden_reference.py runs the reference)."""
import datetime

import numpy as np
import pytest


def _check(pre, bufs, tss, kw, spec):
    from oracle import analyze_oracle as oracle
    from tests import golden_util as gu

    z = gu.reference_cases()
    assert gu.iq_sha256(bufs) == str(z[f"{pre}/iq_sha256"]), f"regenerated IQ of {pre} differs from the bytes the reference saw"
    oa = oracle.OracleAnalyzer(device="0", **kw)
    n = 0
    for b, (buf, ts) in enumerate(zip(bufs, tss)):
        every, kept = oa.process(buf, ts)
        tab = gu.signals_table(every, ts.replace(tzinfo=datetime.timezone.utc))
        assert np.array_equal(tab, z[f"{pre}/b{b}/table"], equal_nan=True)
        kept_ids = {id(s) for s in kept}
        assert [id(s) in kept_ids for s in every] == list(z[f"{pre}/b{b}/kept"])
        if spec:
            assert oa.spec_last.shape == tuple(z[f"{pre}/b{b}/spec_shape"])
            assert gu.spec_sha256(oa.spec_last) == str(z[f"{pre}/b{b}/spec_sha256"])
        n += len(every)
    return n


@pytest.mark.parametrize("seed", range(6))
def test_random_streams_match_reference(seed):
    from tests import golden_util as gu

    bufs, tss, kw = gu.reference_stream_case(seed)
    assert _check(f"stream/{seed}", bufs, tss, kw, spec=True) > 0


@pytest.mark.parametrize("floor_db", [-2.0, 2.0, 8.0])
def test_noise_floor_around_the_threshold_matches_reference(floor_db):
    """The regime in which decisions sit on the noise itself: the reference's default geometry and thresholds (300 kS/s,
    nperseg 256, -90 dBW, 5 dB SNR, 8 - 40 ms) with the noise floor 2 dB under, 2 dB over and 8 dB over the absolute
    threshold -- over it the SNR test alone decides.  Oracle and reference must agree exactly (same float32 powers)."""
    from tests import golden_util as gu

    bufs, tss, kw = gu.reference_noise_floor_case(floor_db)
    n = _check(f"floor/{floor_db}", bufs, tss, kw, spec=False)
    assert n > 5, n
