"""k_mm's 16-sample feeds (the default) against its 8-sample feeds (SDHIP_MM_FEED=8) on the device: same iterations in the same order, so the
int8 symbols, the float symbols and the boundary statistics must be byte for byte the same (tests/test_mm_feed_on_twin_cpu.py is the host twin's
version). Both the Q8 instances (soft symbols only) and the float instances (float symbols asked for) run; short warm-ups make re-run lanes
stop at checkpoints."""
import numpy as np
import pytest

from satdump_amd import synth
from tests import util

pytestmark = pytest.mark.gpu

KW = {
    "metop": dict(samplerate=6e6, symbolrate=2333333, constellation="qpsk", rrc_alpha=0.5, pll_bw=0.003),
    "goes": dict(samplerate=3e6, symbolrate=927000, constellation="bpsk", rrc_alpha=0.5, pll_bw=0.02, max_sps=3.0),
    "npp": dict(samplerate=30e6, symbolrate=15e6, constellation="qpsk", rrc_alpha=0.5, pll_bw=0.002),
}
STAT_FIELDS = ["samples_in", "symbols_out", "buffer_size", "chunks", "chunks_fixed", "chunks_rotated", "chunks_inexact", "chunks_forced"]


def _signal(case, nframes):
    spec, cadus, plain, syms = {"metop": util.metop_case, "goes": util.goes_case, "npp": util.npp_case}[case](nframes=nframes)
    x, _ = synth.modulate(syms, spec)
    return x


def _run(torch, capi, kw, x, bounds, floats, **extra):
    dem = capi.PskDemod(capi.demod_cfg(**kw, **extra))
    d_x = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    soft, syms = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        n = b - a
        d_soft = torch.zeros(2 * n + 64, dtype=torch.int8, device="cuda")
        d_syms = torch.zeros(2 * (n + 64), dtype=torch.float32, device="cuda")
        if floats:
            ns = dem.process_dev(d_x.data_ptr() + 8 * a, n, capi.FMT_CF32, d_soft.data_ptr(), 2 * n + 64, d_syms.data_ptr(), n + 64)
        else:
            ns = dem.process_dev(d_x.data_ptr() + 8 * a, n, capi.FMT_CF32, d_soft.data_ptr(), 2 * n + 64)
        soft.append(d_soft[:ns].cpu().numpy())
        syms.append(d_syms.cpu().numpy())
    st = dem.stats()
    dem.close()
    return np.concatenate(soft), np.concatenate(syms), {f: getattr(st, f) for f in STAT_FIELDS}


CASES = [
    # case, frames, engine config, environment
    ("metop", 600, {}, {}),
    ("metop", 120, dict(chunk_len=4104), {"SDHIP_W_MM": "512"}),
    ("goes", 200, {}, {"SDHIP_MM_Q8": "1"}),
    ("goes", 60, dict(chunk_len=4104), {"SDHIP_W_MM": "512"}),
    ("npp", 200, {}, {}),
    ("npp", 100, dict(chunk_len=2056), {"SDHIP_W_MM": "256"}),
]


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("case,frames,extra,env", CASES, ids=[f"{c[0]}-{c[2].get('chunk_len', 'default')}-{i}" for i, c in enumerate(CASES)])
def test_feed16_bit_identical_to_feed8_on_device(monkeypatch, case, frames, extra, env, floats):
    import torch
    from satdump_amd import capi
    x = _signal(case, frames)
    n = len(x)
    bounds = [0, n // 3 + 5, (2 * n) // 3 + 101, n]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for feed in ("8", "16"):
        monkeypatch.setenv("SDHIP_MM_FEED", feed)
        out[feed] = _run(torch, capi, KW[case], x, bounds, floats, **extra)
    a, b = out["8"], out["16"]
    assert a[2]["chunks"] > 30
    if "chunk_len" in extra:
        assert a[2]["chunks_fixed"] > 0  # re-run lanes were on the path
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2]
