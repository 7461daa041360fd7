#!/usr/bin/env python
"""Generate tests/golden/resident_sv_bits.npz: the outputs of the resident SV kernel, to the bit.

Run once on an MI355X with the library of the commit whose bits are to be kept, loaded through
PF_LIB, and give that commit's id:

    PF_LIB=/path/to/libpf_hip.so python tests/golden/make_golden_resident_bits.py --commit ID [--out FILE]

The runs are those of tests/resident_bits_cases.py.  Per run the file holds every step's mean, Neff,
log normaliser and resample flag in full, and the final particles, weights and log-weights as SHA-256
digests of their bytes (in full for the first run), which keeps the file small; equal digests are
equal bits.  tests/test_gpu_resident_bits.py runs the same cases on the library in the tree.
"""

from __future__ import annotations

import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from tests import resident_bits_cases as RB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "resident_sv_bits.npz"))
    args = ap.parse_args()
    store = {"commit": np.array(args.commit)}
    for name in RB.CASES:
        out = RB.run_case(name, os.environ.__setitem__)
        assert out["flags"].any() and np.all(np.isfinite(out["means"])), name
        for f in RB.FIELDS + ("resident",):
            store[f"{name}/{f}"] = out[f]
        for f in ("x", "w", "lw"):
            store[f"{name}/{f}_sha256"] = np.array(RB.digest(out[f]))
        if name == "base":
            store["base/x"], store["base/w"], store["base/lw"] = out["x"], out["w"], out["lw"]
        print(name, "resamples", int(out["flags"].sum()), "resident", bool(out["resident"]), flush=True)
    np.savez_compressed(args.out, **store)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
