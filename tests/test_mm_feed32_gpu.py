"""k_mm's 32-sample feeds (SDHIP_MM_FEED32=1; the default of a main launch of at most four blocks per CU) against its 16- and 8-sample feeds, in one
process: the same iterations in the same order, so the int8 soft stream, the float symbols, the demodulator's counters and the per-call results of a
stream cut into calls must be byte for byte the same at every width. tests/test_mm_feed32_on_twin_cpu.py collects these functions a second time
against the host twin.

What a 32-sample feed can get wrong where a 16-sample one cannot, and the shapes that put it on the path:
  * a checkpoint (every 1024 samples of a chunk) ends one of FOUR blocks of a feed: chunk lengths 2056, 2072 and 4104 (multiples of 8, not of 32: chunk k
    starts 8 k, 24 k, 8 k samples off the 32-sample grid, so the chunk starts, ends and checkpoints of a stream fall at each of the four offsets). The
    engine rounds the clock recovery's warm-up up to 256 samples, so the offsets come from the chunk length alone;
  * the ring holds a feed and the window in front of it: 2.0, 2.571 and 3.236 samples per symbol, and 8.571, where a 16-sample feed holds one or two
    symbols and a 32-sample one three or four;
  * re-run lanes (16-sample feeds, exact start states) meet the checkpoints a 32-wide main launch left: short warm-ups and a hand-off window of 2e-4
    samples (SDHIP_MM_TOL_MICRO) make most boundaries fail at first sight;
  * calls cut at bounds that are no multiple of 32, one of 20 samples and one of 13 -- shorter than a feed.
BPSK and QPSK, int8 rows (no float symbols asked for, or SDHIP_MM_Q8=1) and float rows, the fast arithmetic and the exact one (SDHIP_FAST_MATH=0).
Each stream is 170 003 samples: 41 to 83 chunks. The last tests ask the launch counts (SDHIP_DEBUG names the width of the main launches there) which
width ran. Run with -m gpu."""
import functools

import numpy as np
import pytest

from satdump_amd import synth
from tests.test_demod_gpu import capi, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N = 170003
STAT_FIELDS = ["samples_in", "symbols_out", "buffer_size", "chunks", "chunks_fixed", "chunks_rotated", "chunks_inexact", "chunks_forced"]
SIGNALS = {
    "qpsk2.0": dict(cfg=dict(samplerate=30e6, symbolrate=15e6, constellation="qpsk", rrc_alpha=0.5, pll_bw=0.002), amplitude=0.4, cfo_hz=20000.0, esn0_db=8.0, seed=4),
    "qpsk2.571": dict(cfg=dict(samplerate=6e6, symbolrate=2333333, constellation="qpsk", rrc_alpha=0.5, pll_bw=0.003), amplitude=0.25, cfo_hz=3000.0, esn0_db=10.0, seed=1),
    "bpsk3.236": dict(cfg=dict(samplerate=3e6, symbolrate=927000, constellation="bpsk", rrc_alpha=0.5, pll_bw=0.02), amplitude=0.5, cfo_hz=1000.0, esn0_db=7.0, seed=2),
    "qpsk8.571": dict(cfg=dict(samplerate=6e6, symbolrate=700000, constellation="qpsk", rrc_alpha=0.5, pll_bw=0.003, max_sps=10.0), amplitude=0.3, cfo_hz=500.0,
                      esn0_db=12.0, seed=7),
}
FEED_NAME = "k_mm (main launches over %d-sample feeds, included in k_mm)"


@functools.lru_cache(maxsize=None)
def _signal(name):
    """random symbols through satdump_amd.synth, computed once per process and never written to"""
    s = SIGNALS[name]
    cfg = s["cfg"]
    rng = np.random.default_rng(s["seed"])
    nsym = int(N / (cfg["samplerate"] / cfg["symbolrate"])) + 64
    if cfg["constellation"] == "bpsk":
        a = (rng.integers(0, 2, nsym) * 2.0 - 1.0).astype(np.complex128)
    else:
        a = ((rng.integers(0, 2, nsym) * 2.0 - 1.0) + 1j * (rng.integers(0, 2, nsym) * 2.0 - 1.0)) / np.sqrt(2.0)
    spec = synth.SynthSpec(constellation=cfg["constellation"], samplerate=cfg["samplerate"], symbolrate=cfg["symbolrate"], rrc_alpha=cfg["rrc_alpha"],
                           amplitude=s["amplitude"], cfo_hz=s["cfo_hz"], esn0_db=s["esn0_db"], seed=s["seed"], timing_offset=0.3)
    x, _ = synth.modulate(a, spec)
    assert len(x) >= N
    return np.ascontiguousarray(x[:N], dtype=np.complex64)


def _run(torch, capi, cfg, x, bounds, floats, **extra):  # noqa: F811
    """one stream through one handle, call by call: the int8 symbols and the float symbols of every call, and the counters at the end"""
    dem = capi.PskDemod(capi.demod_cfg(**cfg, **extra))
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
    return soft, syms, {f: getattr(st, f) for f in STAT_FIELDS}


def _same(a, b, what):
    assert len(a[0]) == len(b[0])
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(u, v), f"{what}: int8 symbols of call {i}"
    for i, (u, v) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), f"{what}: float symbols of call {i}"
    assert a[2] == b[2], what


def _ask(monkeypatch, width):
    """the switches that ask for a width: SDHIP_MM_FEED names 8 or 16 (and refuses anything else, as it did before there was a third width), SDHIP_MM_FEED32=1
    widens the main launches to 32; None: neither is set, the launch's size decides between 16 and 32"""
    monkeypatch.delenv("SDHIP_MM_FEED", raising=False)
    monkeypatch.delenv("SDHIP_MM_FEED32", raising=False)
    if width == "32":
        monkeypatch.setenv("SDHIP_MM_FEED32", "1")
    elif width is not None:
        monkeypatch.setenv("SDHIP_MM_FEED", width)


def _three_widths(monkeypatch, torch, capi, name, bounds, floats, env, **extra):  # noqa: F811
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for feed in ("8", "16", "32"):
        _ask(monkeypatch, feed)
        out[feed] = _run(torch, capi, SIGNALS[name]["cfg"], _signal(name), bounds, floats, **extra)
    _same(out["8"], out["32"], "32 against 8")
    _same(out["16"], out["32"], "32 against 16")
    return out["32"]


CASES = [
    # signal, chunk length, environment
    ("qpsk2.571", 2056, {"SDHIP_W_MM": "512"}),
    ("qpsk2.571", 2072, {"SDHIP_W_MM": "512", "SDHIP_FAST_MATH": "0"}),
    ("qpsk2.0", 2056, {"SDHIP_W_MM": "256"}),
    ("qpsk2.0", 2072, {"SDHIP_W_MM": "256", "SDHIP_FAST_MATH": "0"}),
    ("bpsk3.236", 2056, {"SDHIP_W_MM": "512"}),
    ("bpsk3.236", 2072, {"SDHIP_W_MM": "512", "SDHIP_MM_Q8": "1", "SDHIP_FAST_MATH": "0"}),
    ("qpsk8.571", 2056, {"SDHIP_W_MM": "1024"}),
]


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("name,chunk,env", CASES, ids=[f"{c[0]}-L{c[1]}-{'exact' if 'SDHIP_FAST_MATH' in c[2] else 'fast'}" for c in CASES])
def test_feed32_bit_identical_to_feed16_and_feed8(monkeypatch, torch_cuda, capi, name, chunk, env, floats):  # noqa: F811
    r = _three_widths(monkeypatch, torch_cuda, capi, name, [0, N], floats, env, chunk_len=chunk)
    assert 40 <= N // chunk <= 100 and r[2]["chunks"] >= N // chunk  # (the counter adds the chunks of every lane stage of the chain)
    assert r[2]["symbols_out"] > 0.9 * N / (SIGNALS[name]["cfg"]["samplerate"] / SIGNALS[name]["cfg"]["symbolrate"])


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("name,chunk", [("qpsk2.571", 2056), ("bpsk3.236", 2072), ("qpsk8.571", 2056)])
def test_feed32_streams_cut_into_calls(monkeypatch, torch_cuda, capi, name, chunk, floats):  # noqa: F811
    """bounds that are no multiple of 32 (nor of 8), a first call of 20 samples and one of 13 in the middle: shorter than a feed"""
    bounds = [0, 20, 50025, 50038, 100141, N]
    r = _three_widths(monkeypatch, torch_cuda, capi, name, bounds, floats, {"SDHIP_W_MM": "512"}, chunk_len=chunk)
    assert len(r[0][-1]) > 0 and len(r[0][3]) > 0 and r[2]["samples_in"] == N


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("name,chunk,fast", [("qpsk2.571", 4104, "1"), ("qpsk2.0", 4104, "0"), ("bpsk3.236", 2056, "1")])
def test_feed32_failed_handoffs_and_checkpoints(monkeypatch, torch_cuda, capi, name, chunk, fast, floats):  # noqa: F811
    """a warm-up of 256 samples and a hand-off window of 2e-4 samples: boundaries fail at first sight, their chunks run again (16-sample feeds, exact start
    states) and stop where they meet a checkpoint of the 32-wide main launch -- a checkpoint that ends the first, second, third or last block of a feed"""
    env = {"SDHIP_W_MM": "256", "SDHIP_MM_TOL_MICRO": "200", "SDHIP_FAST_MATH": fast}
    r = _three_widths(monkeypatch, torch_cuda, capi, name, [0, 70011, N], floats, env, chunk_len=chunk)
    assert r[2]["chunks_fixed"] > 0  # re-run lanes were on the path


def _widths_run(capi, fn):  # noqa: F811
    """the launches of the main launches' three width names (SDHIP_DEBUG) over fn()"""
    capi.prof_enable(True)
    try:
        capi.prof_reset()
        fn()
        prof = capi.prof_get()
    finally:
        capi.prof_reset()
        capi.prof_enable(False)
    assert prof["k_mm"][1] > 0
    return {w: prof.get(FEED_NAME % w, (0.0, 0))[1] for w in (8, 16, 32)}


@pytest.mark.parametrize("floats", [False, True], ids=["q8", "float"])
@pytest.mark.parametrize("fast", ["1", "0"], ids=["fast", "exact"])
def test_the_width_asked_for_is_the_width_that_ran(monkeypatch, torch_cuda, capi, fast, floats):  # noqa: F811
    """all four 32-wide instances (int8 and float rows, fast and exact arithmetic), the switches at each of their values, the fall-back, and what they refuse"""
    monkeypatch.setenv("SDHIP_DEBUG", "1")
    monkeypatch.setenv("SDHIP_W_MM", "512")
    monkeypatch.setenv("SDHIP_FAST_MATH", fast)
    name = "qpsk2.571"
    run = lambda: _run(torch_cuda, capi, SIGNALS[name]["cfg"], _signal(name), [0, N], floats, chunk_len=2056)  # noqa: E731
    for feed, want in (("8", 8), ("16", 16), ("32", 32), (None, 32)):  # (83 chunks are two blocks: the default is 32 on any device)
        _ask(monkeypatch, feed)
        got = _widths_run(capi, run)
        assert got[want] > 0 and all(got[w] == 0 for w in got if w != want), (feed, got)
    # SDHIP_MM_FEED32=0 keeps a launch that would take 32 at 16; =1 widens an explicit 16 as well
    monkeypatch.setenv("SDHIP_MM_FEED32", "0")
    got = _widths_run(capi, run)
    assert got[16] > 0 and got[8] == 0 and got[32] == 0, got
    monkeypatch.setenv("SDHIP_MM_FEED32", "1")
    monkeypatch.setenv("SDHIP_MM_FEED", "16")
    got = _widths_run(capi, run)
    assert got[32] > 0 and got[8] == 0 and got[16] == 0, got
    # the 32-wide instances are the unrolled ones: SDHIP_MM_LOOP=0 keeps 16
    _ask(monkeypatch, "32")
    monkeypatch.setenv("SDHIP_MM_LOOP", "0")
    got = _widths_run(capi, run)
    assert got[16] > 0 and got[8] == 0 and got[32] == 0, got
    monkeypatch.delenv("SDHIP_MM_LOOP")
    # what the switches refuse: a width SDHIP_MM_FEED does not name (32 among them), a value of SDHIP_MM_FEED32 other than 0 or 1, 8 and 32 at once
    for env in ({"SDHIP_MM_FEED": "24"}, {"SDHIP_MM_FEED": "32"}, {"SDHIP_MM_FEED32": "2"}, {"SDHIP_MM_FEED": "8", "SDHIP_MM_FEED32": "1"}):
        _ask(monkeypatch, None)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(Exception, match="SDHIP_MM_FEED"):
            run()


def _cus(torch):
    try:
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except AttributeError:  # the host twin's stand-in runtime reports 8
        return 8


def test_a_launch_of_more_than_four_blocks_per_cu_keeps_16(monkeypatch, torch_cuda, capi):  # noqa: F811
    """the occupancy rule of the default: 64-sample chunks of the clock recovery alone (SDHIP_CHUNK_MM), a few more of them than 4 x 64 x CUs lanes -- the default
    is 16 there, 32 when asked for, and 32 by default on a stream of a quarter of the length; same bytes"""
    monkeypatch.setenv("SDHIP_DEBUG", "1")
    monkeypatch.setenv("SDHIP_W_MM", "256")
    monkeypatch.setenv("SDHIP_CHUNK_MM", "64")
    name = "qpsk2.571"
    lanes = 4 * 64 * _cus(torch_cuda) + 130
    reps = (64 * lanes + 256) // N + 1
    x = np.tile(_signal(name), reps)[: 64 * lanes + 256]
    out = {}

    def run(key, xs):
        out[key] = _run(torch_cuda, capi, SIGNALS[name]["cfg"], xs, [0, len(xs)], False)
    _ask(monkeypatch, None)
    got = _widths_run(capi, lambda: run("default", x))
    assert got[16] > 0 and got[32] == 0 and got[8] == 0, got
    got = _widths_run(capi, lambda: run("short", x[: len(x) // 4]))
    assert got[32] > 0 and got[16] == 0 and got[8] == 0, got
    _ask(monkeypatch, "32")
    got = _widths_run(capi, lambda: run("32", x))
    assert got[32] > 0 and got[16] == 0 and got[8] == 0, got
    _same(out["default"], out["32"], "32 against the default of a large launch")
