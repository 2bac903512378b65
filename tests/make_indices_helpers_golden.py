#!/usr/bin/env python3
"""Makes tests/golden/indices_helpers.npz by running the REFERENCE's own selection / fusion helpers (imported in place through
oracle.gen_golden.import_reference(); nothing of it is copied) on a small seeded dictionary.  Not collected by pytest.  It needs
the reference tree where oracle.gen_golden.import_reference() looks for it, and writes with the NumPy that is installed (the
fixture records its version):

    python tests/make_indices_helpers_golden.py

The file holds the input dictionary, a JSON manifest of the calls (arguments, result layout, exception type and text) and
every result array.  tests/indices_helpers_cases.py replays the manifest on the mirror.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from indices_helpers_cases import CALLS, flatten, input_dict  # noqa: E402

THRESHOLDS = (0.01, 0.1)


def main():
    from oracle.gen_golden import import_reference
    ref_idx, _, _ = import_reference()
    arrays, manifest = {}, []
    D, seg = input_dict()
    for k, v in flatten(D).items():
        arrays["in/" + k] = v
    arrays["in_seg"] = seg
    # no variance within a factor of two of a threshold the cases use: summation order cannot decide a case
    for k, v in flatten(D).items():
        var = float(np.var(v))
        for t in THRESHOLDS:
            assert var == 0.0 or var > 2 * t or var < t / 2, (k, var, t)
        print(f"{k:28s} {str(v.dtype):8s} var {var:.3e}")
    for i, (fn, args, kwargs) in enumerate(CALLS):
        a = [seg if x == "<seg>" else (D if x == "<D>" else x) for x in args]
        entry = {"fn": fn, "args": args, "kwargs": kwargs}
        try:
            res = getattr(ref_idx, fn)(*a, **kwargs)
        except Exception as e:  # noqa: BLE001
            entry["raises"] = [type(e).__name__, str(e)]
        else:
            flat = flatten(res)
            entry["result"] = [[k, str(v.dtype), list(v.shape)] for k, v in flat.items()]
            entry["kind"] = type(res).__name__
            for k, v in flat.items():
                arrays[f"out{i}/{k}"] = v
        manifest.append(entry)
        print(i, fn, entry.get("raises") or entry["result"])
    arrays["manifest"] = np.array(json.dumps(manifest, ensure_ascii=False))
    arrays["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "golden", "indices_helpers.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
