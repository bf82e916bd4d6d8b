#!/usr/bin/env python3
"""tools/gen_fsk_golden.py -- records what the reference's fsk_demod / sdpsk_demod compute as fixtures under tests/golden/fsk/.

Needs the reference tree (REF, default /root/reference) and g++; the GPU tests that read the fixtures need neither. The driver
tools/fsk_golden_driver.cpp is compiled with the reference's own block sources, included and compiled where they lie, into a TEMPORARY directory with
the oracle's recorded flags (-O2 -ffp-contract=off, ref_shim/); nothing compiled stays behind.

Three cases of 98 304 input samples (tests/golden/fsk/INDEX.txt lists them). Each .npz holds
    cs16                      the input, interleaved int16 (the chain reads x * (1 / 32767), as the modules' cs16 reader does)
    params                    JSON: the keys of the configuration and the channel that made the input
    info                      float32 {final_sps, final_samplerate, d_buffer_size, filter taps}
    soft, syms                one int8 / one float32 per symbol, whole stream
    st_agc, st_quad, st_dc, st_agc2 (fsk), st_fir     the output of every stage for its first 8192 samples
    st_mm                     the symbols MMClockRecoveryBlock<float> emits for the first 8192 samples of st_fir (the block run on them alone)
The generator also runs every chain with the input cut at odd places and insists that the reference's output does not depend on the cut, and it checks the
end-to-end test's operating point (tests/test_fsk_gpu.py::test_end_to_end_cadus): the reference chain followed by the oracle's simple decoder recovers every
frame behind the first two."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satdump_amd import capi, synth  # noqa: E402

REF_CPP = ["common/dsp/block.cpp", "common/dsp/buffer.cpp", "common/dsp/utils/agc.cpp", "common/dsp/utils/correct_iq.cpp", "common/dsp/filter/fir.cpp",
           "common/dsp/filter/firdes.cpp", "common/dsp/clock_recovery/clock_recovery_mm.cpp", "common/dsp/resamp/polyphase_bank.cpp",
           "common/dsp/resamp/rational_resampler.cpp", "common/dsp/window/window.cpp", "common/dsp/resamp/smart_resampler.cpp", "common/dsp/resamp/power_decim.cpp",
           "common/dsp/filter/decimating_fir.cpp", "common/dsp/demod/quadrature_demod.cpp", "common/dsp/utils/fast_trig.cpp"]
N = 98304
STAGE = 8192
E2E = dict(samplerate=6e6, symbolrate=2.35e6, h=0.5, bt=0.5, esn0_db=14.0, cfo_hz=20e3, seed=5, rrc_alpha=0.35)  # tests/test_fsk_gpu.py uses the same values

CASES = {
    "fsk_a": dict(kind="fsk", cfg=dict(samplerate=6e6, symbolrate=2.35e6, rrc_alpha=0.35), chan=dict(h=0.5, bt=0.5, esn0_db=14.0, cfo_hz=20e3, seed=11)),
    "fsk_b": dict(kind="fsk", cfg=dict(samplerate=3e6, symbolrate=600e3, basic_shaping=1, dc_block=1), chan=dict(h=0.7, bt=None, esn0_db=16.0, cfo_hz=5e3, seed=12)),
    "sdpsk_c": dict(kind="sdpsk", cfg=dict(samplerate=6000.0, symbolrate=1200.0, rrc_alpha=0.4), chan=dict(esn0_db=16.0, cfo_hz=10.0, seed=13)),
}


def build_driver(ref: str, tmp: str) -> C.CDLL:
    sc = os.path.join(ref, "src-core")
    flags = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-DSOURCE_PATH_SIZE=0", "-I" + os.path.join(ROOT, "ref_shim"), "-I" + sc, "-w", "-fno-access-control"]
    lib = os.path.join(tmp, "libfskref.so")
    subprocess.check_call(["g++"] + flags + ["-shared", "-o", lib, os.path.join(ROOT, "tools", "fsk_golden_driver.cpp")] + [os.path.join(sc, f) for f in REF_CPP] +
                          ["-lpthread", "-lm"])
    L = C.CDLL(lib)
    L.fskref_run.restype = C.c_int64
    L.fskref_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.fskref_mm.restype = C.c_int64
    L.fskref_mm.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    return L


def run_chain(L, cfg, ext, x: np.ndarray, cuts=(), stages=False):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n = len(x)
    soft = np.zeros(n + 64, dtype=np.int8)
    syms = np.zeros(n + 64, dtype=np.float32)
    info = np.zeros(4, dtype=np.float32)
    cu = np.asarray(sorted(cuts), dtype=np.int64)
    st = [np.zeros(2 * STAGE if s == 0 else STAGE, dtype=np.float32) for s in range(6)]
    ptrs = (C.c_void_p * 6)(*[a.ctypes.data for a in st])
    st_n = np.zeros(6, dtype=np.int64)
    ns = L.fskref_run(C.byref(cfg), C.byref(ext), x.ctypes.data, n, cu.ctypes.data if len(cu) else None, len(cu), soft.ctypes.data, syms.ctypes.data, n + 64,
                      ptrs if stages else None, STAGE, st_n.ctypes.data, info.ctypes.data)
    st = [a[: int(k)] for a, k in zip(st, st_n)]
    assert ns >= 0, "fskref_run failed"
    return dict(soft=soft[:ns].copy(), syms=syms[:ns].copy(), info=info, stages=st)


def make_input(name, case):
    c, ch = case["cfg"], case["chan"]
    nbits = int(N / (c["samplerate"] / c["symbolrate"])) + 8
    bits = np.random.default_rng(ch["seed"]).integers(0, 2, nbits).astype(np.uint8)
    if case["kind"] == "fsk":
        x = synth.modulate_fsk(bits, c["samplerate"], c["symbolrate"], h=ch["h"], bt=ch["bt"], esn0_db=ch["esn0_db"], cfo_hz=ch["cfo_hz"], seed=ch["seed"])
    else:
        x = synth.modulate_sdpsk(bits, c["samplerate"], c["symbolrate"], rrc_alpha=c["rrc_alpha"], esn0_db=ch["esn0_db"], cfo_hz=ch["cfo_hz"], seed=ch["seed"])
    assert len(x) >= N, (name, len(x))
    return synth.to_cs16(x[:N])


def cs16_to_cf32(cs16: np.ndarray) -> np.ndarray:
    return (cs16.astype(np.float32) * np.float32(1.0 / 32767.0)).view(np.complex64)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fsk"))
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    index = ["# produced by tools/gen_fsk_golden.py from the reference's own block sources (fsk_demod / sdpsk_demod); name, size, key:sha256[:12]"]
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(args.ref, tmp)
        for name, case in CASES.items():
            cfg, ext = capi.fsk_cfg(case["kind"], **case["cfg"])
            cs16 = make_input(name, case)
            x = cs16_to_cf32(cs16)
            whole = run_chain(L, cfg, ext, x, stages=True)
            for cuts in ([N // 3, N // 3 + 12345], [1, 7, 4099, 33333, 33334, 70001, N - 1], list(range(5, N, 7777))):
                cut = run_chain(L, cfg, ext, x, cuts=cuts)
                assert np.array_equal(cut["soft"], whole["soft"]) and np.array_equal(cut["syms"].view(np.uint32), whole["syms"].view(np.uint32)), \
                    f"{name}: the reference's output DEPENDS on how the input is cut ({cuts[:3]}...): a finding for DESIGN.md"
            st = whole["stages"]
            fir = st[4]
            mm = np.zeros(len(fir) + 8, dtype=np.float32)
            nmm = L.fskref_mm(whole["info"][0], cfg.clock_gain_omega, cfg.clock_mu, cfg.clock_gain_mu, cfg.clock_omega_relative_limit, fir.ctypes.data, len(fir), mm.ctypes.data,
                              len(mm))
            assert nmm > 0 and np.array_equal(mm[:nmm].view(np.uint32), whole["syms"][:nmm].view(np.uint32)), "the block alone and in the chain disagree"
            arrays = dict(cs16=cs16, params=np.frombuffer(json.dumps(dict(kind=case["kind"], cfg=case["cfg"], chan=case["chan"], n=N)).encode(), dtype=np.uint8),
                          info=whole["info"], soft=whole["soft"], syms=whole["syms"], st_agc=st[0], st_quad=st[1], st_dc=st[2], st_fir=fir, st_mm=mm[:nmm].copy())
            if case["kind"] == "fsk":
                arrays["st_agc2"] = st[3]
            path = os.path.join(args.out, name + ".npz")
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            assert size < 1048576, (name, size)
            index.append(f"{name}.npz {size:9d} B  " + " ".join(f"{k}:{sha(v)}" for k, v in sorted(arrays.items())))
            clipped = int(np.sum(np.abs(whole["soft"].astype(np.int32)) == 127))
            print(f"{name}: {len(whole['soft'])} symbols, final_sps {whole['info'][0]:.4f}, {int(whole['info'][3])} taps, {clipped} clamped, {size} B; cuts leave the output unchanged")
        if not args.skip_e2e:
            from oracle import pyref
            cadus = synth.make_cadus(12, seed=E2E["seed"], derand=False)
            bits = np.concatenate([np.unpackbits(cadus.reshape(-1)), np.random.default_rng(E2E["seed"]).integers(0, 2, 8192).astype(np.uint8)])  # (+ a frame of idle bits)
            x = synth.modulate_fsk(bits, E2E["samplerate"], E2E["symbolrate"], h=E2E["h"], bt=E2E["bt"], esn0_db=E2E["esn0_db"], cfo_hz=E2E["cfo_hz"], seed=E2E["seed"])
            cfg, ext = capi.fsk_cfg("fsk", samplerate=E2E["samplerate"], symbolrate=E2E["symbolrate"], rrc_alpha=E2E["rrc_alpha"])
            r = run_chain(L, cfg, ext, x)
            got = pyref.best().simple_decode(pyref.fec_cfg(decoder=2, constellation=pyref.BPSK, cadu_size=8192, derandomize=0, rs_i=4, rs_type=1, rs_usecheck=1), r["soft"])["cadu"]
            ids = [int(np.flatnonzero((cadus == g).all(1))[0]) if (cadus == g).all(1).any() else -1 for g in got]
            print(f"end to end at Es/N0 {E2E['esn0_db']} dB: reference chain + simple decoder -> frames {ids}")
            assert set(range(2, 12)) <= set(ids), "the end-to-end operating point does not recover every frame behind the first two"
    with open(os.path.join(args.out, "INDEX.txt"), "w") as f:
        f.write("\n".join(index) + "\n")


if __name__ == "__main__":
    main()
