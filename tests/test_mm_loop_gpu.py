"""k_mm's unrolled fast paths (the default) against its one-symbol loop (SDHIP_MM_LOOP=0) on the device: the same steps in the same order, so the
int8 symbols, the float symbols and the boundary statistics must be byte for byte the same (tests/test_mm_loop_on_twin_cpu.py is the host twin's
version). MetOp, GOES and NPP find ~6.2, ~4.9 and 8 symbols in a 16-sample feed, so lanes leave the three-step pass after each of its steps; chunk
lengths that are multiples of neither 16 nor 24 and short warm-ups make re-run lanes stop at checkpoints. Both the Q8 instances (soft symbols
only) and the float instances (float symbols asked for) run."""
import numpy as np
import pytest

from tests.test_mm_feed_gpu import KW, _run, _signal

pytestmark = pytest.mark.gpu

CASES = [
    # case, frames, engine config, environment
    ("metop", 600, {}, {}),
    ("metop", 120, dict(chunk_len=4120), {"SDHIP_W_MM": "512"}),
    ("goes", 200, {}, {"SDHIP_MM_Q8": "1"}),
    ("goes", 60, dict(chunk_len=4120), {"SDHIP_W_MM": "512"}),
    ("npp", 200, {}, {}),
    ("npp", 100, dict(chunk_len=2056), {"SDHIP_W_MM": "256"}),
]


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("case,frames,extra,env", CASES, ids=[f"{c[0]}-{c[2].get('chunk_len', 'default')}-{i}" for i, c in enumerate(CASES)])
def test_unrolled_loop_bit_identical_on_device(monkeypatch, case, frames, extra, env, floats):
    import torch
    from satdump_amd import capi
    x = _signal(case, frames)
    n = len(x)
    bounds = [0, n // 3 + 5, (2 * n) // 3 + 101, n]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for loop in ("0", "1"):
        monkeypatch.setenv("SDHIP_MM_LOOP", loop)
        out[loop] = _run(torch, capi, KW[case], x, bounds, floats, **extra)
    a, b = out["0"], out["1"]
    assert a[2]["chunks"] > 30
    if "chunk_len" in extra:
        assert a[2]["chunks_fixed"] > 0  # re-run lanes were on the path
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2]
