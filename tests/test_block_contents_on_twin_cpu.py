"""The block-contents tests (tests/test_block_contents_gpu.py), the very same test functions, collected a second time against the HOST TWIN (tests/emu) the way
tests/test_soft_rails_on_twin_cpu.py collects the rails tests: the allocator, its pool, its counters and the fill are host code, which the twin runs as it
stands, and every kernel that reads a block before writing it reads the same bytes there."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import pyref
from tests import test_block_contents_gpu as B
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
    spec = importlib.util.spec_from_file_location("capi_host_twin_blocks", os.path.join(ROOT, "satdump_amd", "capi.py"))
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


class _NumpyMem:
    """satdump_amd.dvbs2's memory adapter on host arrays (the twin's 'device' pointers are host pointers)"""

    @staticmethod
    def alloc(n, dtype):
        return np.zeros(int(n), dtype=dtype)

    @staticmethod
    def from_host(a):
        return np.ascontiguousarray(a).copy()

    @staticmethod
    def ptr(h):
        return h.ctypes.data

    @staticmethod
    def to_host(h, n=None):
        return (h if n is None else h[:n]).copy()


@pytest.fixture(scope="module")
def mem():
    return _NumpyMem


ctx = B.ctx

# the m2x case is eleven minutes of emulated Viterbi blocks on the twin, filled or not (tests/test_soft_rails_on_twin_cpu.py): SDHIP_TWIN_FULL=1 collects it here,
# otherwise it stays with the GPU suite
_LEFT_TO_THE_GPU = () if os.environ.get("SDHIP_TWIN_FULL") else ("lrpt_m2x",)


@pytest.mark.parametrize("fill", [255, 127])
@pytest.mark.parametrize("family", [f for f in B.FILLED if f not in _LEFT_TO_THE_GPU])
def test_filled_blocks(ctx, family, fill):
    B.test_filled_blocks(ctx, family, fill)


for _name in dir(B):
    if _name.startswith("test_") and _name not in globals():
        globals()[_name] = getattr(B, _name)
