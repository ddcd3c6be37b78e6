"""Generates tests/golden/ref_*.npz from oracle/_ref/libref.so -- the reference's own registration / feature classes
compiled verbatim from /root/reference (oracle/ref_shim).  Only runs where /root/reference is present; the committed
files let the oracle be checked against the compiled reference anywhere (tests/test_ref_pin.py).
Run from the repo root:  python tests/golden/make_ref_golden.py [name ...]
(no names: every scenario of refpin.pinned_scenarios(), every feature case of refpin.pinned_feature_cases() and "small_functions";
a feature case is named "features:<case>")
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import refpin  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    names = sys.argv[1:] or (refpin.pinned_scenarios() + ["features:" + c for c in refpin.pinned_feature_cases()] + ["small_functions"])
    for name in names:
        if name == "small_functions":
            out = refpin.run_small_functions_ref(*refpin.small_function_cases())
            np.savez_compressed(os.path.join(HERE, "ref_small_functions.npz"), **{k: np.asarray(v) for k, v in out.items()})
            print(name, {k: np.shape(v) for k, v in out.items()})
        elif name.startswith("features:"):
            case = name[len("features:"):]
            out = refpin.run_features_subprocess(case)
            np.savez_compressed(os.path.join(HERE, f"ref_features_{case}.npz"), **refpin.features_to_golden(out))
            print("features", case, {k: v.shape for k, v in out.items() if isinstance(v, np.ndarray) and k in ("ordered", "corner", "planar")})
        else:
            out = refpin.run_ref_subprocess(name)
            np.savez_compressed(os.path.join(HERE, f"ref_{name}.npz"), **refpin.to_golden(out))
            print(name, "frames", out["n_frames"], "ok", [out[k]["ok"] for k in range(out["n_frames"])], "iters", [out[k]["iters"] for k in range(out["n_frames"])])
