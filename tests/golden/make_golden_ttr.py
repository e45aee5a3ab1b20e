#!/usr/bin/env python3
"""Generate tests/golden/ttr.npz by running the UNMODIFIED reference's postTimeStepTTR (Helper/post_ttr.py:8).

Build-container only, like make_golden_query.py (same loader: oracle/_harness/ref_loader.py).  Run as

    python tests/golden/make_golden_ttr.py

Everything written is DATA: seeded inputs, the fields the reference returned for them, and a record of whether its
update branch (a second call on the Bundle the first returned) raised.  Only the initialisation branch can be pinned:
the first call on a Bundle without a `ttr` field.  Cases: a vector, a column and a 2-D array; values below, above and
exactly at zero; an initial time that is not zero.
"""
import io
import json
import os
import sys
import contextlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_harness"))
import ref_loader  # noqa: E402

ref_loader.load()

from LevelSetPy.Utilities import Bundle  # noqa: E402
from LevelSetPy.Helper.post_ttr import postTimeStepTTR  # noqa: E402

CASES = {"vec": ((957,), 0.0), "col": ((203, 1), 0.375), "arr": ((33, 29), -1.25)}


def main():
    out, raised = {}, {}
    rng = np.random.default_rng(20260301)
    for name, (shape, t0) in CASES.items():
        y = rng.standard_normal(shape)
        y.reshape(-1)[::7] = 0.0                               # nodes exactly at the level
        with contextlib.redirect_stdout(io.StringIO()):
            yOut, sd = postTimeStepTTR(t0, y.copy(), Bundle({}))
        assert np.array_equal(np.asarray(yOut), y)
        out[name + "_y"], out[name + "_t"] = y, np.float64(t0)
        out[name + "_ttr"] = np.asarray(sd.ttr, dtype=np.float64)
        out[name + "_lastY"] = np.asarray(sd.ttrLastY, dtype=np.float64)
        out[name + "_lastT"] = np.float64(sd.ttrLastT)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                postTimeStepTTR(t0 + 0.5, y - 0.3, sd)
            raised[name] = None
        except Exception as e:                  # noqa: BLE001  (whatever the reference raises is the record)
            raised[name] = "%s: %s" % (type(e).__name__, str(e)[:120])
        print("%-4s %-10s init pinned; update %s" % (name, shape, raised[name] or "ran"))
    out["raised_json"] = np.array(json.dumps(raised))
    path = os.path.join(HERE, "ttr.npz")
    np.savez_compressed(path, **out)
    print("wrote ttr.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
