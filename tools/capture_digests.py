"""Writes a digest fixture under tests/golden/: the SHA-256 of what a test module's digest function returns for every case of its
bit-equality test, from ANOTHER build of the library (the commit a rewrite of those kernels is held to).  Needs the GPU.

    python tools/capture_digests.py PARENT.so --commit <hash of the commit PARENT.so was built from> \
        [--digests tests.test_hip_resampling:sample_pdf_digests --out tests/golden/resample_digests.json]
    python tools/capture_digests.py PARENT.so --commit <hash> --digests tests.test_hip_shape_corners:generic_digests \
        --out tests/golden/generic_digests.json
    python tools/capture_digests.py PARENT.so --commit <hash> --digests tests.test_hip_march_split:march_digests \
        --out tests/golden/march_digests.json

The cases, their inputs and the launches are the test module's own (test_sample_pdf_bits_match_recorded / test_generic_bits_match_recorded /
test_march_bits_match_recorded call the same function).  Every case is captured twice; the file is written only if the two captures agree (the kernels have no atomics:
a difference is a finding)."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", help="the build of libegonerf_hip.so to record")
    ap.add_argument("--commit", required=True, help="the commit that build was compiled from (stored in the file)")
    ap.add_argument("--digests", default="tests.test_hip_resampling:sample_pdf_digests", help="module:function that returns case -> digests")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "resample_digests.json"))
    a = ap.parse_args()
    os.environ["EGO_ALLOW_STALE_LIB"] = "1"   # the recorded build is not the tree's
    from egonerf_amd import _lib
    _lib.LIB = os.path.abspath(a.lib)
    module, function = a.digests.split(":")
    digests = getattr(importlib.import_module(module), function)
    first, second = digests(), digests()
    differs = [k for k in first if first[k] != second[k]]
    if differs:
        print("two captures of the same build differ (the kernels are not deterministic):", differs)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"commit": a.commit, "digests": first}, open(a.out, "w"), indent=1)
    print(a.out, len(first), "cases, two captures agree; library", _lib.LIB)
    return 0


if __name__ == "__main__":
    sys.exit(main())
