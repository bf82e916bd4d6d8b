"""The tests of the path-history forward pass (tests/test_vit2h_step_gpu.py), the very same test functions, collected a second time
against the HOST TWIN (tests/emu) the way tests/test_fec_gpu_on_twin_cpu.py collects the FEC parity tests: v2h_step's packed 16-bit
arithmetic, the tags and the lane roles are integer code the twin runs as it stands."""
import importlib.util
import os

import pytest

from oracle import pyref
from tests import test_vit2h_step_gpu as V
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
    spec = importlib.util.spec_from_file_location("capi_host_twin_vit2h", os.path.join(ROOT, "satdump_amd", "capi.py"))
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


@pytest.fixture(scope="module")
def orc():
    return pyref.best()


for _name in dir(V):
    if _name.startswith("test_") and _name not in globals():
        globals()[_name] = getattr(V, _name)
