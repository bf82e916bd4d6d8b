"""The AGC's uniform options as variants of the launch (k_afc<ORDER, AFC_*>, AgcStageT<.., AGC_MAG_*>, the gain cap as one minimum against a bound) compute what
the code in front of them computed, BYTE FOR BYTE: every case of tests/afc_variants_util.py against the fixtures tests/golden/afc_parent/gpu_*.npz, recorded on
the parent commit on the GPU (tools/gen_afc_parent_golden.py). The streams are the smallest that run one full cooperative wave of k_afc beside the per-lane
path (76 / 75 chunks of 2048 samples, sample counts a multiple of 8 and not); the counters in the fixtures say that every chunk boundary was verified, none let
through (forced == 0), so a run that skipped the lanes cannot pass. Run with -m gpu."""
import numpy as np
import pytest

from oracle import pyref
from tests import afc_variants_util as U
from tests.test_demod_gpu import capi, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
PSK = [n for n, c in U.CASES.items() if c["kind"] == "psk"]
AGC = [n for n, c in U.CASES.items() if c["kind"] == "agc"]


@pytest.fixture(scope="module")
def inputs():
    return {n: U.signal(c) for n, c in U.CASES.items()}


@pytest.mark.parametrize("name", PSK)
def test_psk_demod_equals_the_parent(torch_cuda, capi, inputs, name):
    """BPSK and QPSK through psk_demod (the fused AGC + 31-tap filter + Costas lanes, cooperative and per-lane), the 33-tap chain (AGC lanes, filter and loop as
    stages of their own) and exact mode: soft symbols, float symbols and chunk counters."""
    want = U.load(BACKEND, name)
    assert want["counters"][U.COUNTERS.index("chunks_forced")] == 0
    if not U.CASES[name]["cfg"].get("exact"):
        assert want["counters"][U.COUNTERS.index("chunks")] >= 2 * 75  # the lanes ran: 75 chunks or more in each of the stages that count them
    U.compare(U.run_case(torch_cuda, capi, name, inputs[name]), want, name)


@pytest.mark.parametrize("name", ["qpsk", "bpsk_ragged"])
def test_per_lane_path_equals_the_parent(torch_cuda, capi, inputs, name, monkeypatch):
    """SDHIP_COOP=0: every chunk on the per-lane path of the same instances. It computed the cooperative path's bytes before
    (test_cooperative_lanes_equal_the_per_lane_streams) and must still: the same fixtures."""
    monkeypatch.setenv("SDHIP_COOP", "0")
    U.compare(U.run_case(torch_cuda, capi, name, inputs[name]), U.load(BACKEND, name), name)


@pytest.mark.parametrize("name", AGC)
def test_agc_blocks_equal_the_parent(torch_cuda, capi, inputs, name):
    """The ndsp AGC blocks in the chunk-parallel mode's arithmetic: |input| (agc_fast_cc, input_mag on) and |output| (agc_cc), no cap (max_gain 0), the default
    cap, and a cap low enough to hold the gain on the quiet half of the stream -- which the output itself shows: a sample that left at the cap is x * cap."""
    case, x = U.CASES[name], inputs[name]
    rec = U.run_case(torch_cuda, capi, name, x)
    f = U.clamp_fraction(x, rec["_out"], U.LOW_CAP)
    if case.get("capped"):
        assert 0.2 < f < 0.8, f"the cap of {U.LOW_CAP} engaged on {f:.3f} of the samples"
    else:
        assert f < 0.01
        g = np.abs(rec["_out"].view(np.complex64)[len(x) // 4: len(x) // 2]) / np.maximum(np.abs(x[len(x) // 4: len(x) // 2]), 1e-20)
        assert np.median(g) > 1.5 * U.LOW_CAP  # without the cap the gain on the quiet half stands well above it
    U.compare(rec, U.load(BACKEND, name), name)


def test_exact_mode_equals_the_oracle(torch_cuda, capi, inputs):
    """exact = 1 on the same stream: bit for bit the reference chain, as tests/test_demod_gpu.py::test_exact_mode_bit_identical holds it."""
    name = "qpsk_exact"
    x = inputs[name]
    want = pyref.best().psk_demod(pyref.demod_cfg(samplerate=6e6, symbolrate=2333333, constellation=pyref.QPSK, rrc_alpha=0.5, pll_bw=0.003), x)
    rec = U.run_case(torch_cuda, capi, name, x)
    assert np.array_equal(rec["_soft"], want["soft"])
    assert np.array_equal(rec["_syms"].view(np.uint32), want["syms"].view(np.uint32))
