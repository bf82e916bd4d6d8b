"""k_mm's unrolled fast paths (the default) against its one-symbol loop (SDHIP_MM_LOOP=0) on the host twin: the fast paths run three symbols per
pass through mm_sym, the delay line passed round three register pairs instead of rotated, and put the MmState order back once per feed -- the same
steps in the same order, so the int8 rows, the float symbols, the symbol counts, the boundary verdicts and the re-runs (checkpoint merges included)
must come out byte for byte the same.

A lane leaves the unrolled loop after the first, second or third step of a pass, depending on how many symbols it finds in a feed: ~6.2 at MetOp's
2.57 samples per symbol, ~4.9 at GOES' 3.24, 8 at NPP's 2, so every exit occurs. Chunk lengths that are multiples of neither 16 nor 24 put the
checkpoints at varying places in a feed; short warm-ups make many boundaries fail, so re-run lanes start from exact states and stop at checkpoints.
Both the Q8 instances (no float symbols asked for) and the float instances (the parity legs) run."""
import numpy as np
import pytest

from tests.test_demod_emu_cpu import _case, _run, twin  # noqa: F401  (twin: fixture, the host twin's binding)
from tests.test_mm_feed_on_twin_cpu import _run_soft_only, _stats

CASES = [
    # case, frames, chunk length (samples), environment, re-runs expected
    ("metop", 40, 4120, {"SDHIP_W_MM": "512"}, True),
    ("metop", 40, 8200, {}, False),
    ("goes", 24, 4120, {"SDHIP_W_MM": "512", "SDHIP_MM_Q8": "1"}, True),
    ("npp", 40, 2056, {"SDHIP_W_MM": "256"}, True),
    ("npp", 40, 4120, {"SDHIP_W_MM": "512", "SDHIP_FAST_MATH": "0"}, True),
]


@pytest.mark.parametrize("case,frames,chunk,env,reruns", CASES, ids=[f"{c[0]}-L{c[2]}-{i}" for i, c in enumerate(CASES)])
def test_unrolled_loop_bit_identical_to_one_symbol_loop(twin, monkeypatch, case, frames, chunk, env, reruns):  # noqa: F811
    plain, x, ocfg, kw, ofec = _case(case, frames)
    n = len(x)
    bounds = [0, n // 3 + 5, (2 * n) // 3 + 101, n]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for loop in ("0", "1"):
        monkeypatch.setenv("SDHIP_MM_LOOP", loop)
        soft, syms, st = _run(twin, kw, x, chunks=bounds, chunk_len=chunk)
        soft_q8, st_q8 = _run_soft_only(twin, kw, x, bounds, chunk_len=chunk)
        out[loop] = (soft, syms, _stats(st), soft_q8, _stats(st_q8))
    a, b = out["0"], out["1"]
    assert a[2]["chunks"] > 30
    if reruns:  # re-run lanes (exact start states, early exit at the checkpoints) were on the path
        assert a[2]["chunks_fixed"] > 0 and a[4]["chunks_fixed"] > 0
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2]
    assert np.array_equal(a[3], b[3])
    assert a[4] == b[4]
    assert np.array_equal(a[0], a[3])


def test_loop_switch_refuses_other_values(twin, monkeypatch):  # noqa: F811
    plain, x, ocfg, kw, ofec = _case("metop", 4)
    monkeypatch.setenv("SDHIP_MM_LOOP", "2")
    with pytest.raises(Exception, match="SDHIP_MM_LOOP"):
        _run(twin, kw, x[:200000], chunk_len=4096)
