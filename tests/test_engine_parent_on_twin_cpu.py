"""tests/test_engine_parent_gpu.py, the very same test function, collected a second time against the HOST TWIN of the engine (tests/emu) and the fixtures recorded
through it on the parent commit (tests/golden/engine_parent/twin_*.npz: the twin's sqrtf is not v_sqrt_f32, so they are a set of their own). Runs in the CPU
suite (-m "not gpu"): the twin compiles satdump_amd/csrc/demod_engine.hip itself, so this proves that the refactored host code computes and launches what the
parent's did; the GPU build stays with -m gpu."""
import pytest

from tests import engine_parent_util as U
from tests import test_engine_parent_gpu as G
from tests.emu import fake_torch
from tests.test_afc_variants_on_twin_cpu import _plain
from tests.test_engine_parent_gpu import inputs  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def torch_cuda():
    return fake_torch


@pytest.fixture(scope="module")
def capi():
    m = U.twin_capi()
    if m is None:
        pytest.skip("no host clang++ to build the twin with")
    return m


@pytest.fixture(autouse=True)
def _twin_fixtures(monkeypatch):
    monkeypatch.setattr(G, "BACKEND", "twin")


test_engine_equals_the_parent = _plain(G.test_engine_equals_the_parent)
