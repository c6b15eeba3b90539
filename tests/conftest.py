import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs the HIP library through the C-ABI)")
    config.addinivalue_line("markers", "slow: long soak (tens of minutes of CPU oracle time); runs only when the -m expression names it, e.g. -m 'gpu and slow'")


def pytest_collection_modifyitems(config, items):
    """`slow` tests are opt-in: the driver's plain `-m gpu` run must stay within minutes, so they are skipped unless the marker expression
    itself mentions `slow` (or EGO_RUN_SLOW=1)."""
    if "slow" in (config.getoption("markexpr") or "") or os.environ.get("EGO_RUN_SLOW") == "1":
        return
    skip = pytest.mark.skip(reason="slow soak: select with -m 'gpu and slow'")
    for it in items:
        if "slow" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session", autouse=True)
def _library_is_current():
    """egonerf_amd._lib.load() refuses a binary that was not built from the sources next to it; (re)build before the first test
    instead of failing every test after a kernel edit (a no-op when libegonerf_hip.so.hash matches; hipcc cross-compiles without
    a GPU in ~10 s)."""
    from egonerf_amd.build import build_library
    build_library(force=False)


class _SplitNpz:
    """A fixture stored as <name>.npz plus <name>.part2.npz, ... (oracle/capture_golden.py: save_split keeps every committed file
    under 1 MiB), read like one np.load result: `.files` in order, `fx[key]`, `key in fx`."""

    def __init__(self, paths):
        import numpy as np
        self._parts = [np.load(p) for p in paths]
        self._where = {k: z for z in self._parts for k in z.files}
        self.files = [k for z in self._parts for k in z.files]

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def keys(self):
        return list(self.files)


@pytest.fixture(scope="session")
def golden():
    import glob
    import numpy as np

    cache = {}

    def load(name):
        if name not in cache:
            path = os.path.join(GOLDEN, name + ".npz")
            parts = sorted(glob.glob(os.path.join(GOLDEN, name + ".part*.npz")), key=lambda p: int(p.rsplit(".part", 1)[1][:-4]))
            cache[name] = _SplitNpz([path] + parts) if parts else np.load(path)
        return cache[name]

    return load
