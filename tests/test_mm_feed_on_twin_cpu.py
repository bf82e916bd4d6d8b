"""k_mm's 16-sample feeds (the default) against its 8-sample feeds (SDHIP_MM_FEED=8) on the host twin: the symbol loop runs once per feed
instead of once per 8-sample block, with the same iterations in the same order -- so the int8 rows, the float symbols, the symbol counts,
the boundary verdicts and the re-runs (checkpoint merges included) must come out byte for byte the same.

Chunk lengths that are not multiples of 16 put the checkpoints in either half of a feed; short warm-ups make many boundaries fail, so
re-run lanes start from exact states and stop at checkpoints; several calls put chunk 0 (the carried state) and the last chunk's tail
and look-ahead on the path. Both the Q8 instances (no float symbols asked for) and the float instances (the parity legs) run."""
import numpy as np
import pytest

from tests.test_demod_emu_cpu import _case, _run, twin  # noqa: F401  (twin: fixture, the host twin's binding)

STAT_FIELDS = ["samples_in", "symbols_out", "buffer_size", "chunks", "chunks_fixed", "chunks_rotated", "chunks_inexact", "chunks_forced"]


def _run_soft_only(twin, kw, x, chunks, **extra):  # noqa: F811
    """_run without float symbols: the clock recovery stores the int8 symbols itself (k_mm<.., Q8>)."""
    import ctypes as C
    cfg = twin.demod_cfg(**kw, **extra)
    dem = twin.PskDemod(cfg)
    x = np.ascontiguousarray(x)
    soft = []
    for a, b in zip(chunks[:-1], chunks[1:]):
        n = b - a
        o_soft = np.zeros(2 * n + 64, dtype=np.int8)
        ns = dem.process_dev(x.ctypes.data_as(C.c_void_p).value + 8 * a, n, twin.FMT_CF32, o_soft.ctypes.data_as(C.c_void_p).value, 2 * n + 64)
        soft.append(o_soft[:ns].copy())
    st = dem.stats()
    dem.close()
    return np.concatenate(soft), st


def _stats(st):
    return {f: getattr(st, f) for f in STAT_FIELDS}


CASES = [
    # case, frames, chunk length (samples), environment, re-runs expected
    ("metop", 40, 4104, {"SDHIP_W_MM": "512"}, True),
    ("metop", 40, 8200, {}, False),
    ("goes", 24, 4104, {"SDHIP_W_MM": "512", "SDHIP_MM_Q8": "1"}, True),
    ("npp", 40, 2056, {"SDHIP_W_MM": "256"}, True),
    ("npp", 40, 4096, {"SDHIP_W_MM": "512", "SDHIP_FAST_MATH": "0"}, True),
]


@pytest.mark.parametrize("case,frames,chunk,env,reruns", CASES, ids=[f"{c[0]}-L{c[2]}-{i}" for i, c in enumerate(CASES)])
def test_feed16_bit_identical_to_feed8(twin, monkeypatch, case, frames, chunk, env, reruns):  # noqa: F811
    plain, x, ocfg, kw, ofec = _case(case, frames)
    n = len(x)
    bounds = [0, n // 3 + 5, (2 * n) // 3 + 101, n]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for feed in ("8", "16"):
        monkeypatch.setenv("SDHIP_MM_FEED", feed)
        soft, syms, st = _run(twin, kw, x, chunks=bounds, chunk_len=chunk)
        soft_q8, st_q8 = _run_soft_only(twin, kw, x, bounds, chunk_len=chunk)
        out[feed] = (soft, syms, _stats(st), soft_q8, _stats(st_q8))
    a, b = out["8"], out["16"]
    assert a[2]["chunks"] > 30
    if reruns:  # re-run lanes (exact start states, early exit at the checkpoints) were on the path
        assert a[2]["chunks_fixed"] > 0 and a[4]["chunks_fixed"] > 0
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2]
    assert np.array_equal(a[3], b[3])
    assert a[4] == b[4]
    # the Q8 rows and the float rows quantised by k_quantize are the same soft stream
    assert np.array_equal(a[0], a[3])


def test_feed_switch_refuses_other_widths(twin, monkeypatch):  # noqa: F811
    plain, x, ocfg, kw, ofec = _case("metop", 4)
    monkeypatch.setenv("SDHIP_MM_FEED", "32")
    with pytest.raises(Exception, match="SDHIP_MM_FEED"):
        _run(twin, kw, x[:200000], chunk_len=4096)
