"""The pipeline-against-serial-order tests of tests/test_fec_overlap_gpu.py, the very same test functions, collected a second time against the
HOST TWIN (tests/emu). Launches run in place there, so nothing overlaps; what the twin proves without a GPU is the pipeline's bookkeeping: which set
of buffers a batch lives in, the start state guessed across a batch boundary and its check, the discard of a batch issued on a wrong premise,
the even batch split. Streams and batches are smaller than on the device (the twin runs the 64 lanes of a wave as fibers)."""
import importlib.util
import os

import pytest

from tests import test_fec_overlap_gpu as OV
from tests.emu import build as emu_build
from tests.emu import fake_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    return fake_torch


@pytest.fixture(scope="module")
def capi():
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no host clang++ to build the twin with")
    lib = emu_build.build()
    spec = importlib.util.spec_from_file_location("capi_host_twin_overlap", os.path.join(ROOT, "satdump_amd", "capi.py"))
    m = importlib.util.module_from_spec(spec)
    old = os.environ.get("SDHIP_LIB")
    os.environ["SDHIP_LIB"] = lib
    os.environ["SDHIP_TESTING_TWIN"] = "1"  # capi refuses the twin without it
    try:
        spec.loader.exec_module(m)
        m.lib()
    finally:
        del os.environ["SDHIP_TESTING_TWIN"]
        if old is None:
            del os.environ["SDHIP_LIB"]
        else:
            os.environ["SDHIP_LIB"] = old
    assert m.LIB_PATH == lib
    return m


@pytest.fixture(autouse=True)
def _twin_sizes(monkeypatch):
    monkeypatch.setitem(OV.SIZES, "frames", 150)
    monkeypatch.setitem(OV.SIZES, "batch", 5)


for _name in dir(OV):
    if _name.startswith("test_") and _name not in globals():
        globals()[_name] = getattr(OV, _name)
