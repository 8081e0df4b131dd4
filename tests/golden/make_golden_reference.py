#!/usr/bin/env python3
"""Generate tests/golden/reference_cases.npz by running the REFERENCE on the inputs of
tests/test_oracle_vs_reference.py and test_match.py::test_oracle_against_imported_reference_on_fresh_streams.

The inputs are rebuilt from seeds by the builders in tests/golden_util.py (the tests rebuild them the
same way; a SHA-256 of the IQ bytes pins them); the file holds only what the reference made of them:

* ``stream/<seed>/...`` and ``floor/<floor_db>/...``: per buffer every Signal field before the
  shadow filter (the 8-column table of golden_util.signals_table), the shadow verdicts and, for the
  random streams, a SHA-256 of the spectrogram's values (golden_util.spec_sha256);
* ``match/<trial>/...``: the matcher's consumed groups in queue order and the groups still open at the
  end (ts and duration in microseconds, frequency, per-device avgs with a presence mask).

The reference's ``radiotracking.analyze`` imports ``rtlsdr`` and ``radiotracking.match`` imports
``cbor2`` / ``paho.mqtt.client``; stand-in modules are injected for the imports only (make_golden.py,
make_golden_match.py).

Usage:  TZ=UTC python tests/golden/make_golden_reference.py REFERENCE_CHECKOUT
"""
import datetime
import json
import os
import sys
import time
import types

os.environ["TZ"] = "UTC"
time.tzset()

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main(reference):
    sys.path.insert(0, REPO)
    sys.path.insert(0, reference)
    for name in ("cbor2", "paho", "paho.mqtt", "paho.mqtt.client"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from tests import golden_util as gu
    from tests.golden import make_golden as mg  # (injects the rtlsdr stub, imports radiotracking.analyze)

    import radiotracking
    import radiotracking.match as ref_match
    from pyradiotracking_amd.match import datetime_to_us

    out = {}
    cases = [("stream", seed, gu.reference_stream_case(seed), True) for seed in range(6)]
    cases += [("floor", floor_db, gu.reference_noise_floor_case(floor_db), False) for floor_db in (-2.0, 2.0, 8.0)]
    for kind, key, (bufs, tss, kw), with_spec in cases:
        pre = f"{kind}/{key}"
        out[f"{pre}/iq_sha256"] = np.array(gu.iq_sha256(bufs))
        for b, exp in enumerate(mg.run_reference_buffers(mg.make_reference(**kw), bufs, tss)):
            out[f"{pre}/b{b}/table"] = exp["table"]
            out[f"{pre}/b{b}/kept"] = exp["kept"]
            if with_spec:
                out[f"{pre}/b{b}/spec_sha256"] = np.array(gu.spec_sha256(exp["spec"]))
                out[f"{pre}/b{b}/spec_shape"] = np.array(exp["spec"].shape, dtype=np.int64)

    class Sink:
        def __init__(self):
            self.items = []

        def put(self, x):
            self.items.append(x)

    us = datetime.timedelta(microseconds=1)
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    for trial, (devices, params, signals) in enumerate(gu.matcher_trials()):
        sink = Sink()
        ref = ref_match.SignalMatcher(device=devices, signal_queue=sink, **params)
        for dev, ts_us, freq, dur_us, avg in signals:
            ref.add(radiotracking.Signal(dev, epoch + ts_us * us, freq, dur_us * us, avg + 3, avg, 1.0, -100.0, 10.0))
        for what, groups in (("consumed", sink.items), ("pending", ref._matched)):
            arrs = gu.matched_groups_arrays([(g.ts, g.frequency, g.duration, g._avgs) for g in groups], len(devices), datetime_to_us)
            for k, v in arrs.items():
                out[f"match/{trial}/{what}/{k}"] = v
    out["index_json"] = np.array(json.dumps({"streams": list(range(6)), "floors": [-2.0, 2.0, 8.0], "match_trials": trial + 1}))
    path = os.path.join(HERE, "reference_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "radiotracking")):
        raise SystemExit("usage: make_golden_reference.py REFERENCE_CHECKOUT (the directory holding radiotracking/)")
    main(os.path.abspath(sys.argv[1]))
