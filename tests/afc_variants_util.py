"""Shared by tools/gen_afc_parent_golden.py (which records) and tests/test_afc_variants_{gpu,on_twin_cpu}.py (which compare): the cases under which the AGC
recurrence's uniform options -- magnitude of the input or of the output, gain cap or none -- and the lane stages built on it (k_afc, k_chunks<AgcStage>, the
31-tap and the other filters) are pinned to what the parent of the k_afc variant work computed, byte for byte. Not a test module.

Every stream is the smallest that still enters the cooperative path of k_afc and the per-lane path beside it: chunks of 2048 samples, 76 / 75 of them (one full
wave of ordinary chunks 1 .. 64, chunk 0 and a ragged tail per lane), once with a sample count that is a multiple of 8 and once with one that is not."""
import ctypes as C
import hashlib
import os

import numpy as np

from satdump_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "afc_parent")
CHUNK, WARMUP = 2048, 512
N_ALIGNED = 75 * CHUNK + 1232  # 76 chunks; a multiple of 8
N_RAGGED = 74 * CHUNK + 1237   # 75 chunks; not a multiple of 8 (nor of 2)
HEAD = 4096                    # leading values kept beside the hash, to say WHERE a mismatch begins
LOW_CAP = 2.0                  # the capped AGC cases: below the ~4 the loop settles at on the quiet half of their input, above the ~1 of the loud half

# Es/N0, amplitude and offsets of bench.py's WORKLOADS (goes_hrit: bpsk 7 dB; metop_ahrpt: qpsk 10 dB)
_QPSK = dict(constellation="qpsk", samplerate=6e6, symbolrate=2333333, rrc_alpha=0.5, pll_bw=0.003)
_BPSK = dict(constellation="bpsk", samplerate=6e6, symbolrate=2333333, rrc_alpha=0.5, pll_bw=0.02)
_CH_Q = dict(esn0_db=10.0, amplitude=0.25, cfo_hz=5000.0, seed=31)
_CH_B = dict(esn0_db=7.0, amplitude=0.5, cfo_hz=1000.0, seed=32)

# name -> what runs. kind "psk": capi.PskDemod over the whole stream in one call (soft symbols, float symbols, chunk counters);
# kind "agc": one ndsp AGC block (agc_cc: |output|; agc_fast_cc: |input| times the gain), its output samples
CASES = {
    "qpsk": dict(kind="psk", cfg=_QPSK, chan=_CH_Q, n=N_ALIGNED),
    "qpsk_ragged": dict(kind="psk", cfg=_QPSK, chan=_CH_Q, n=N_RAGGED),
    "bpsk": dict(kind="psk", cfg=_BPSK, chan=_CH_B, n=N_ALIGNED),
    "bpsk_ragged": dict(kind="psk", cfg=_BPSK, chan=_CH_B, n=N_RAGGED),
    # a filter that is not the 31-tap one: the AGC lanes alone (k_chunks<AgcStage>), the filter and the Costas loop as stages of their own
    "qpsk_rrc33": dict(kind="psk", cfg=dict(_QPSK, rrc_taps=33), chan=_CH_Q, n=N_ALIGNED),
    "qpsk_exact": dict(kind="psk", cfg=dict(_QPSK, exact=1), chan=_CH_Q, n=N_ALIGNED, oracle=True),
    "agc_fast": dict(kind="agc", block="agc_fast_cc", keys=dict(rate=1e-2, reference=1.0, max_gain=65536.0), chan=_CH_Q, n=N_RAGGED),
    "agc_nocap": dict(kind="agc", block="agc_cc", keys=dict(rate=1e-2, reference=1.0, max_gain=0.0), chan=_CH_Q, n=N_ALIGNED),
    "agc_fast_nocap": dict(kind="agc", block="agc_fast_cc", keys=dict(rate=1e-2, reference=1.0, max_gain=0.0), chan=_CH_Q, n=N_ALIGNED),
    "agc_lowcap": dict(kind="agc", block="agc_cc", keys=dict(rate=1e-2, reference=1.0, max_gain=LOW_CAP), chan=_CH_Q, n=N_RAGGED, capped=True),
    "agc_fast_lowcap": dict(kind="agc", block="agc_fast_cc", keys=dict(rate=1e-2, reference=1.0, max_gain=LOW_CAP), chan=_CH_Q, n=N_ALIGNED, capped=True),
}


def signal(case: dict) -> np.ndarray:
    """The case's input: random symbols through satdump_amd.synth. The AGC cases get a level step in the middle (x 4), so that a low cap holds the gain on the
    quiet half and lets it go on the loud one."""
    cfg, ch, n = case.get("cfg", _QPSK), case["chan"], case["n"]
    rng = np.random.default_rng(ch["seed"])
    nsym = int(n / (cfg["samplerate"] / cfg["symbolrate"])) + 64
    if cfg["constellation"] == "bpsk":
        a = (rng.integers(0, 2, nsym) * 2.0 - 1.0).astype(np.complex128)
    else:
        a = ((rng.integers(0, 2, nsym) * 2.0 - 1.0) + 1j * (rng.integers(0, 2, nsym) * 2.0 - 1.0)) / np.sqrt(2.0)
    spec = synth.SynthSpec(constellation=cfg["constellation"], samplerate=cfg["samplerate"], symbolrate=cfg["symbolrate"], rrc_alpha=cfg["rrc_alpha"],
                           amplitude=ch["amplitude"], cfo_hz=ch["cfo_hz"], esn0_db=ch["esn0_db"], seed=ch["seed"], timing_offset=0.3)
    x, _ = synth.modulate(a, spec)
    assert len(x) >= n
    x = np.ascontiguousarray(x[:n], dtype=np.complex64)
    if case["kind"] == "agc":
        x[n // 2:] *= np.float32(4.0)
    return x


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _counters(st) -> np.ndarray:
    return np.array([st.chunks, st.chunks_fixed, st.chunks_rotated, st.chunks_inexact, st.chunks_forced, st.symbols_out], dtype=np.int64)


COUNTERS = ("chunks", "chunks_fixed", "chunks_rotated", "chunks_inexact", "chunks_forced", "symbols_out")


def run_case(torch, capi, name: str, x: np.ndarray | None = None) -> dict:
    """Run one case on whatever `capi` is bound to (the library on the GPU with torch, the host twin with tests/emu/fake_torch). Returns the record a fixture
    holds: hashes of the whole outputs, their first HEAD values, the chunk counters."""
    case = CASES[name]
    x = signal(case) if x is None else x
    n = len(x)
    rec = {"input_sha": np.array(sha(x))}
    if case["kind"] == "psk":
        # (this geometry meets every condition of launch_afc's cooperative path: chunk, both warm-ups and the estimator window multiples of 16 samples, 66 chunks
        # or more; SDHIP_COOP=0 in the environment sends every chunk down the per-lane path instead, which computes the same bytes)
        dem = capi.PskDemod(capi.demod_cfg(**case["cfg"], chunk_len=CHUNK, warmup=WARMUP))
        d_x = torch.from_numpy(np.ascontiguousarray(x.view(np.float32))).cuda()
        d_soft = torch.zeros(2 * n + 64, dtype=torch.int8, device="cuda")
        d_syms = torch.zeros(2 * (n + 64), dtype=torch.float32, device="cuda")
        ns = dem.process_dev(d_x.data_ptr(), n, capi.FMT_CF32, d_soft.data_ptr(), 2 * n + 64, d_syms.data_ptr(), n + 64)
        nsym = ns if case["cfg"]["constellation"] == "bpsk" else ns // 2
        soft = d_soft[:ns].cpu().numpy()
        syms = d_syms[: 2 * nsym].cpu().numpy()
        rec.update(soft_sha=np.array(sha(soft)), syms_sha=np.array(sha(syms)), soft_len=np.array(len(soft)), soft_head=soft[:HEAD].copy(),
                   syms_head=syms[:HEAD].view(np.uint32).copy(), counters=_counters(dem.stats()))
        rec["_soft"], rec["_syms"] = soft, syms  # whole outputs for the caller (not stored)
    else:
        from satdump_amd import ndsp
        blk = ndsp.SingleBlock(case["block"], capi_mod=capi)
        for k, v in case["keys"].items():
            assert blk.set_cfg(k, v) == ndsp.RES_OK
        blk._cfg.chunk_len = CHUNK  # (start gains by the affine scan, as the block runs by default: no warm-up to set)
        d_x = torch.from_numpy(np.ascontiguousarray(x.view(np.float32))).cuda()
        d_y = torch.zeros(2 * (n + 64), dtype=torch.float32, device="cuda")
        nout = blk.work_dev(d_x.data_ptr(), n, d_y.data_ptr(), n + 64)
        assert nout == n
        y = d_y[: 2 * n].cpu().numpy()
        rec.update(out_sha=np.array(sha(y)), out_head=y[:HEAD].view(np.uint32).copy(), counters=_counters(blk.stats()))
        rec["_out"] = y
        blk.stop()
    return rec


def twin_capi():
    """satdump_amd/capi.py bound to the host twin (tests/emu), as tests/test_demod_gpu_on_twin_cpu.py binds it; None where the host clang++ is missing."""
    import importlib.util
    from tests.emu import build as emu_build
    if not os.path.exists(emu_build.CLANG):
        return None
    lib = emu_build.build()
    spec = importlib.util.spec_from_file_location("capi_host_twin_afc", os.path.join(ROOT, "satdump_amd", "capi.py"))
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


def clamp_fraction(x: np.ndarray, y: np.ndarray, cap: float) -> float:
    """Share of the AGC block's samples that left with the gain AT the cap: the block writes x * gain, so those are exactly x * cap in float."""
    xf = x.view(np.float32)
    ok = xf != 0
    return float(np.mean((xf * np.float32(cap))[ok] == y[ok]))


def load(backend: str, name: str) -> dict:
    with np.load(os.path.join(GOLDEN, f"{backend}_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def compare(rec: dict, want: dict, name: str) -> None:
    """Byte for byte: lengths, counters, the leading values (for a readable first difference), then the hashes of the whole outputs."""
    assert str(rec["input_sha"]) == str(want["input_sha"]), f"{name}: the synthesised input differs from the one the fixture was recorded on"
    assert np.array_equal(rec["counters"], want["counters"]), f"{name}: counters {dict(zip(COUNTERS, rec['counters']))} != {dict(zip(COUNTERS, want['counters']))}"
    for k in sorted(want):
        if k.endswith("_head"):
            d = np.flatnonzero(rec[k] != want[k])
            assert len(d) == 0, f"{name}: {k} differs first at value {d[0]} ({len(d)} of {len(want[k])})"
    for k in sorted(want):
        if k.endswith("_sha") or k.endswith("_len"):
            assert str(rec[k]) == str(want[k]), f"{name}: {k} {rec[k]} != {want[k]}"
