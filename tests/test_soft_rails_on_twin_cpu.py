"""The int8-rail tests (tests/test_soft_rails_gpu.py), the very same test functions, collected a second time against the HOST TWIN (tests/emu) the way
tests/test_vit2h_step_on_twin_cpu.py collects the path-history tests: every -128 rule is integer code in a fetch path, which the twin runs as it stands."""
import importlib.util
import os

import pytest

from oracle import pyref
from tests import test_soft_rails_gpu as R
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
    spec = importlib.util.spec_from_file_location("capi_host_twin_rails", os.path.join(ROOT, "satdump_amd", "capi.py"))
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


# (the m2x case is eleven minutes of emulated Viterbi blocks behind the de-interleaver's 2.6 M samples of lead-in, with or without rails: SDHIP_TWIN_FULL=1 collects
# it here, as it was run for the sabotage of m2x_clamp; otherwise it stays with the GPU suite)
_LEFT_TO_THE_GPU = () if os.environ.get("SDHIP_TWIN_FULL") else ("test_lrpt_m2x_rails",)

for _name in dir(R):
    if _name.startswith("test_") and _name not in globals() and _name not in _LEFT_TO_THE_GPU:
        globals()[_name] = getattr(R, _name)
