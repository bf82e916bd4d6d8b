"""GPU parity tests of fsk_demod / sdpsk_demod (run with -m gpu; tests/test_fsk_on_twin_cpu.py collects the same functions against the host twin).
Every call goes through the C ABI. The reference's behaviour reaches these tests as data: tests/golden/fsk/*.npz, recorded by tools/gen_fsk_golden.py from
the reference's own blocks (cs16 input, parameters, soft bytes, float symbols, every stage's output for its first 8192 samples).

exact = 1 must reproduce the fixtures BIT FOR BIT; the chunk-parallel mode is held to the symbol count and to a measured share of float symbols within
1e-5 of the fixture's (test_chunk_parallel_mode)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from satdump_amd import synth

gpu = pytest.mark.gpu  # every test but test_defaults needs the device
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsk")
CASES = ["fsk_a", "fsk_b", "sdpsk_c"]
CHUNK = 4096
# end-to-end operating point: tools/gen_fsk_golden.py (E2E) checked on the CPU that the reference chain + the oracle's simple decoder recover frames 1 .. 11 here
E2E = dict(samplerate=6e6, symbolrate=2.35e6, h=0.5, bt=0.5, esn0_db=14.0, cfo_hz=20e3, seed=5, rrc_alpha=0.35)
# share of float symbols within 1e-5 of the fixture's, chunk-parallel mode, chunk_len 4096 -- MEASURED (test_chunk_parallel_mode's docstring), per case the lower of
# the host twin's and the GPU's value over the one-call and the three-call run, minus the spread between the three cases
MEASURED = {"fsk_a": 0.9948, "fsk_b": 0.9990, "sdpsk_c": 0.9936}
FLOOR = {k: v - (max(MEASURED.values()) - min(MEASURED.values())) for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def capi():
    from satdump_amd import capi as c
    c.lib()
    return c


_cache = {}


def _golden(name):
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        g = {k: z[k] for k in z.files}
        g["params"] = json.loads(bytes(g["params"]).decode())
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()  # (a copy: the fixtures' arrays are read-only)


def _handle(capi, g, **extra):
    return capi.FskDemod(capi.fsk_cfg(g["params"]["kind"], **g["params"]["cfg"], **extra))


def _run(torch, capi, g, bounds=None, **extra):
    """The fixture's cs16 input through a fresh handle, in the calls `bounds` cuts it into: (soft, syms, stats of the last call, chunks summed over the calls)."""
    dem = _handle(capi, g, **extra)
    cs16 = g["cs16"]
    n = len(cs16) // 2
    d_x = _dev(torch, cs16)
    soft, syms, chunks = [], [], 0
    bounds = bounds or [0, n]
    for a, b in zip(bounds[:-1], bounds[1:]):
        m = b - a
        d_soft = torch.zeros(m + 64, dtype=torch.int8, device="cuda")
        d_syms = torch.zeros(m + 64, dtype=torch.float32, device="cuda")
        ns = dem.process_dev(d_x.data_ptr() + 4 * a, m, capi.FMT_CS16, d_soft.data_ptr(), m + 64, d_syms.data_ptr(), m + 64)
        soft.append(d_soft[:ns].cpu().numpy())
        syms.append(d_syms[:ns].cpu().numpy())
        st = dem.stats()
        chunks += st.chunks
    return np.concatenate(soft), np.concatenate(syms), dem.stats(), chunks


def _op(torch, capi, kind, params, x, cont=0, complex_in=False):
    n = len(x) // 2 if complex_in else len(x)
    d_x = _dev(torch, x)
    d_y = torch.zeros(n + 64, dtype=torch.float32, device="cuda")
    p = np.asarray(list(params) + [cont], dtype=np.float32)
    nout = capi.lib().sdhip_op_block(0, kind, p.ctypes.data_as(C.c_void_p), C.c_void_p(d_x.data_ptr()), n, C.c_void_p(d_y.data_ptr()), n + 64)
    assert nout >= 0, capi.last_error()
    return d_y[:nout].cpu().numpy()


def _blocks(g):
    """(kind, params, input, complex input?, expected output) of the five real-valued blocks on one fixture's stage records"""
    c, info = g["params"]["cfg"], g["info"]
    fsk = g["params"]["kind"] == "fsk"
    dc_out = g["st_dc"]
    fir_in = g["st_agc2"] if fsk else dc_out
    out = [(11, [1.0], g["st_agc"], True, g["st_quad"]), (12, [], g["st_quad"], False, dc_out)]
    if fsk:
        out.append((13, [0.1, 0.5, 1.0, 65535.0], dc_out, False, g["st_agc2"]))
    box = int(info[3]) if c.get("basic_shaping") else 0
    out.append((14, [float(info[1]), c["symbolrate"], c.get("rrc_alpha", 0.5), 31, box], fir_in, False, g["st_fir"]))
    out.append((15, [float(info[0]), 1.7e-2 ** 2 / 4.0, 0.5, 1.7e-2, 0.005], g["st_fir"], False, g["st_mm"]))
    return out


def test_defaults(capi):
    """sdhip_fsk_cfg_default = the module headers' values (module_fsk_demod.h:25-31, module_sdpsk_demod.h:23-29 and the constructors). Needs no device."""
    for kind in ("fsk", "sdpsk"):
        c, x = capi.fsk_cfg(kind)
        assert x.kind == capi.REAL_KINDS[kind] and x.basic_shaping == 0
        assert c.rrc_taps == 31 and c.clock_mu == 0.5 and c.clock_omega_relative_limit == np.float32(0.005)
        assert c.clock_gain_mu == np.float32(1.7e-2) and c.clock_gain_omega == np.float32(1.7e-2 ** 2 / 4.0)
        assert c.agc_rate == np.float32(1e-2) and c.dc_block == 0 and c.iq_swap == 0 and c.exact == 0
        assert (c.min_sps, c.max_sps) == ((np.float32(1.0), np.float32(10.0)) if kind == "sdpsk" else (np.float32(1.1), np.float32(4.0)))


@gpu
@pytest.mark.parametrize("case", CASES)
def test_single_blocks_bit_exact(torch_cuda, capi, case):
    """Each real-valued block of sdhip_op_block (kinds 11 .. 15) reproduces the fixture's stage output bit for bit, the stream run in one call and in two calls
    cut at an odd index."""
    g = _golden(case)
    for kind, params, x, cplx, want in _blocks(g):
        n = len(x) // 2 if cplx else len(x)
        got = _op(torch_cuda, capi, kind, params, x, complex_in=cplx)
        assert len(got) == len(want), (kind, len(got), len(want))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"kind {kind}"
        cut = 3001
        a = _op(torch_cuda, capi, kind, params, x[: (2 * cut if cplx else cut)], complex_in=cplx)
        b = _op(torch_cuda, capi, kind, params, x[(2 * cut if cplx else cut):], cont=1, complex_in=cplx)
        got2 = np.concatenate([a, b])
        assert n > cut and len(got2) == len(want) and np.array_equal(got2.view(np.uint32), want.view(np.uint32)), f"kind {kind} in two calls"


@gpu
@pytest.mark.parametrize("case", CASES)
def test_exact_mode_bit_identical(torch_cuda, capi, case):
    """exact = 1: soft bytes and float symbols bit-identical to the fixture, in one call and in three calls cut at n // 3 and n // 3 + 12345."""
    g = _golden(case)
    n = len(g["cs16"]) // 2
    for bounds in (None, [0, n // 3, n // 3 + 12345, n]):
        soft, syms, st, _ = _run(torch_cuda, capi, g, bounds, exact=1)
        assert st.final_sps == g["info"][0] and st.buffer_size == int(g["info"][2])
        assert len(syms) == len(g["syms"])
        assert np.array_equal(syms.view(np.uint32), g["syms"].view(np.uint32))
        assert np.array_equal(soft, g["soft"])


def _share(syms, ref):
    scale = np.sqrt(np.mean(ref.astype(np.float64) ** 2))
    return float(np.mean(np.abs(syms.astype(np.float64) - ref) / scale <= 1e-5))


@gpu
@pytest.mark.parametrize("case", CASES)
def test_chunk_parallel_mode(torch_cuda, capi, case):
    """The product mode (chunk_len 4096: over twenty lanes per stage) against the fixture, in one call and in three calls: the same NUMBER of symbols (no symbol
    dropped or doubled at a hand-off), stats.chunks > 20, and the share of float symbols within 1e-5 (of the symbols' rms) of the fixture's at or above FLOOR.

    Measured shares (one call / three calls):
        host twin   fsk_a 0.9969 / 0.9948   fsk_b 0.9990 / 0.9990   sdpsk_c 0.9936 / 0.9998
        MI355X      fsk_a 0.9969 / 0.9948   fsk_b 0.9990 / 0.9990   sdpsk_c 0.9936 / 0.9998   (the same figures: every stage's arithmetic is the reference's,
                    operation for operation, on either; the schedule is the same)
    MEASURED holds the lower value per case; the floor is that minus the spread between the cases (0.9990 - 0.9936 = 0.54 point).
    The rest is the floor of any time-parallel schedule of this loop, as for the PSK chain (99.13 - 99.61 %): the clock recovery feeds back through the arm index
    rint(mu * 128), two trajectories on the same samples hover a fraction of an arm apart and pick neighbouring arms on a fraction of a percent of the symbols."""
    g = _golden(case)
    n = len(g["cs16"]) // 2
    for bounds in (None, [0, n // 3, n // 3 + 12345, n]):
        soft, syms, st, chunks = _run(torch_cuda, capi, g, bounds, chunk_len=CHUNK)
        assert len(syms) == len(g["syms"]) and len(soft) == len(g["soft"])
        assert chunks > 20
        share = _share(syms, g["syms"])
        print(f"{case} {'one call' if bounds is None else 'three calls'}: share within 1e-5 = {share:.4f} (floor {FLOOR[case]:.4f}), chunks {chunks}")
        assert share >= FLOOR[case], f"{share:.4f} of the symbols within 1e-5, floor {FLOOR[case]:.4f}"


@gpu
@pytest.mark.parametrize("case", ["fsk_a", "sdpsk_c"])
def test_host_push_pull_path(torch_cuda, capi, case):
    """sdhip_demod_push / flush / pull (what the modules call) give the bytes sdhip_demod_process_dev gives."""
    g = _golden(case)
    cs16 = g["cs16"]
    n = len(cs16) // 2
    for exact in (1, 0):
        dem = _handle(capi, g, exact=exact, chunk_len=0 if exact else CHUNK)
        for a, b in zip([0, 7, 7, 30000, 30001], [7, 7, 30000, 30001, n]):
            dem.push(cs16[2 * a: 2 * b], capi.FMT_CS16)
        dem.flush()
        soft = dem.pull()
        want, _, _, _ = _run(torch_cuda, capi, g, None, exact=exact, chunk_len=0 if exact else CHUNK)
        assert np.array_equal(soft, want)
        if exact:
            assert np.array_equal(soft, g["soft"])


@gpu
def test_empty_and_tiny_calls(torch_cuda, capi):
    """0, 1 and ntaps - 1 samples between normal calls: exact mode still equals the one-call output."""
    g = _golden("fsk_a")
    n = len(g["cs16"]) // 2
    nt = int(g["info"][3])
    bounds = [0, 0, 1, 20000, 20000, 20001, 20001 + nt - 1, 60000, 60000 + nt - 1, n - 1, n, n]
    soft, syms, _, _ = _run(torch_cuda, capi, g, bounds, exact=1)
    assert np.array_equal(syms.view(np.uint32), g["syms"].view(np.uint32)) and np.array_equal(soft, g["soft"])


@gpu
def test_end_to_end_cadus(torch_cuda, capi):
    """Baseband -> CADUs with no CPU module in between: 12 unrandomised CADUs, NRZ-L, as GFSK at case A's rates -> the FSK handle (exact AND chunk-parallel)
    -> FecDecoder(SDHIP_DEC_SIMPLE_PSK, cadu_size 8192, RS223 I = 4). At least 10 CADUs, each byte-identical to a transmitted one; both modes the same list."""
    cadus = synth.make_cadus(12, seed=E2E["seed"], derand=False)
    bits = np.concatenate([np.unpackbits(cadus.reshape(-1)), np.random.default_rng(E2E["seed"]).integers(0, 2, 8192).astype(np.uint8)])  # (+ a frame of idle bits)
    x = synth.modulate_fsk(bits, E2E["samplerate"], E2E["symbolrate"], h=E2E["h"], bt=E2E["bt"], esn0_db=E2E["esn0_db"], cfo_hz=E2E["cfo_hz"], seed=E2E["seed"])
    n = len(x)
    d_x = _dev(torch_cuda, x.view(np.float32))
    lists = []
    for exact in (1, 0):
        dem = capi.FskDemod(capi.fsk_cfg("fsk", samplerate=E2E["samplerate"], symbolrate=E2E["symbolrate"], rrc_alpha=E2E["rrc_alpha"], exact=exact,
                                         chunk_len=0 if exact else CHUNK))
        d_soft = torch_cuda.zeros(n + 64, dtype=torch_cuda.int8, device="cuda")
        ns = dem.process_dev(d_x.data_ptr(), n, capi.FMT_CF32, d_soft.data_ptr(), n + 64)
        dec = capi.FecDecoder(capi.fec_cfg(decoder=capi.DEC_SIMPLE_PSK, constellation="bpsk", cadu_size=8192, derandomize=0, rs_i=4, rs_type=capi.RS223, rs_usecheck=1))
        dec.push(d_soft[:ns].cpu().numpy())
        got = dec.pull()
        assert len(got) >= 10
        for f in got:
            assert (cadus == f).all(1).any(), "a decoded CADU is none of the transmitted ones"
        lists.append(got)
    assert lists[0].shape == lists[1].shape and np.array_equal(lists[0], lists[1])


@gpu
def test_noise_only_input(torch_cuda, capi):
    """Noise alone, 200 k samples: the call returns, the symbol count is within 1 % of n / final_sps, and boundaries were let through unlocked."""
    n = 200_000
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(2 * n) * 0.3).astype(np.float32)
    dem = capi.FskDemod(capi.fsk_cfg("fsk", samplerate=6e6, symbolrate=2.35e6, rrc_alpha=0.35, chunk_len=CHUNK))
    d_x = _dev(torch_cuda, x)
    d_soft = torch_cuda.zeros(n + 64, dtype=torch_cuda.int8, device="cuda")
    ns = dem.process_dev(d_x.data_ptr(), n, capi.FMT_CF32, d_soft.data_ptr(), n + 64)
    st = dem.stats()
    assert abs(ns - n / st.final_sps) < 0.01 * n / st.final_sps
    assert st.chunks_forced > 0


@gpu
def test_refusals(capi):
    """rrc_alpha is mandatory unless basic_shaping is set; basic_shaping is fsk_demod's key."""
    with pytest.raises(capi.SdhipError, match="RRC Alpha"):
        capi.FskDemod(capi.fsk_cfg("fsk", samplerate=6e6, symbolrate=2.35e6))
    with pytest.raises(capi.SdhipError, match="basic_shaping"):
        capi.FskDemod(capi.fsk_cfg("sdpsk", samplerate=6000.0, symbolrate=1200.0, rrc_alpha=0.4, basic_shaping=1))
