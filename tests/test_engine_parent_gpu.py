"""The engine's host scaffold -- one helper per rule of the schedule "lane per chunk, judge the hand-offs, re-run what failed" instead of a copy per stage --
computes what the copies computed and launches what they launched: every case of tests/engine_parent_util.py against the fixtures
tests/golden/engine_parent/gpu_*.npz, recorded on the parent commit on the GPU (tools/gen_engine_parent_golden.py). Per call of every stream: soft symbols,
float symbols (or output samples), the six chunk counters and the launches of every kernel. The fixtures' counters say that the lanes ran and that no boundary
was let through unverified (except in `noise`, where some must be), so a run that skipped the lanes cannot pass. Run with -m gpu."""
import numpy as np
import pytest

from oracle import pyref
from tests import engine_parent_util as U
from tests.test_demod_gpu import capi, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BACKEND = "gpu"


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(name):
        key = (U.CASES[name]["stream"],) + tuple(bool(U.CASES[name].get(k)) for k in ("step", "dc", "noise", "scale"))
        if key not in cache:
            cache[key] = U.signal(name)
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("name", list(U.CASES))
def test_engine_equals_the_parent(torch_cuda, capi, inputs, name):
    want = U.load(BACKEND, name)
    U.check_conditions(name, want)  # the fixture itself: forced == 0 (noise: > 0), the lanes ran, qpsk_own_warmup re-ran chunks
    rec = U.run_case(torch_cuda, capi, name, inputs(name))
    U.compare(rec, want, name)
    if U.CASES[name].get("exact"):
        # exact mode behind the one dc_block(): bit for bit the reference chain, as test_afc_variants_gpu.py::test_exact_mode_equals_the_oracle holds it
        ref = pyref.best().psk_demod(pyref.demod_cfg(samplerate=6e6, symbolrate=2333333, constellation=pyref.QPSK, rrc_alpha=0.5, pll_bw=0.003, dc_block=1,
                                                     post_costas_dc=1), inputs(name))
        assert np.array_equal(rec["_soft"], ref["soft"])
        assert np.array_equal(rec["_syms"].view(np.uint32), ref["syms"].view(np.uint32))
