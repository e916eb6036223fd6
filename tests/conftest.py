import gc
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(autouse=True)
def _collect_garbage_before_gpu_tests(request):
    """A model dropped by an earlier test keeps its training engine, and that engine's captured hipGraphs, in reference cycles
    (engine <-> its linears, captured step <-> its saved activations) that only the cyclic collector frees.  Left to the
    collector's own timing, it may run inside a later test's stream capture, on the thread that captures, and destroy those
    graphs there -- HIP calls a capture does not permit, and the process aborts.  Collected here, before the next test starts."""
    if request.node.get_closest_marker("gpu") is not None:
        gc.collect()


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")
