#!/usr/bin/env python3
"""ccsds_turbo_decoder on one MI355X, soft symbols resident in HBM, at the two settings of the Stereo pipelines (turbo_rate 1/6 and 1/2, turbo_base 1115, 20 and 1
iterations): frames/s of sdhip_ccsds_turbo_process_dev over a synthetic locked stream of 4096 frames (HIP events around the call alone, two warm-up calls, the
median of five; a handle is a stream, so one per call, created outside the timed window), and the kernels' own times inside one more such call from the library's
per-kernel HIP events (sdhip_prof_*), taken in a call of their own. Also measures contract 4 of the module's tests: max |ours - fixture| / max(1, |fixture|) of the
a-priori arrays over the two BCJR fixtures. Writes profiles/ccsds_turbo_bench.json.

The stream is made here, by an encoder written from CCSDS 131.0-B (the constituent code of section 6.3 and the library's own interleaver table): 8 distinct frames
with a valid CRC, tiled, +-40 with AWGN. The run asserts that every frame comes out, which also proves that encoder against the decoder.

The baseline is the reference module's own loop on one CPU thread of ANOTHER HOST (where the reference tree is; the GPU machine has none): `--cpu-baseline`
compiles tools/ccsds_turbo_golden_driver.cpp the way tools/gen_ccsds_turbo_golden.py does, runs it on the first frames of the SAME streams and merges its frames/s.
usage: tools/bench_ccsds_turbo.py [--frames 4096] [--reps 5] | --cpu-baseline [--cpu-frames 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "ccsds_turbo_bench.json")
SETTINGS = {"stereo_r16_i20": ("1/6", 1115, 20), "stereo_r12_i1": ("1/2", 1115, 1)}
DISTINCT = 8
AMP = 40.0
SIGMA = {"1/2": 22.0, "1/6": 40.0}
ASM_HEX = {"1/2": "034776C7272895B0", "1/6": "25D5C0CE8990F6C9461BF79CDA2A3F31766F0936B9E40863"}
G0, G1, G2, G3 = 0x13, 0x1B, 0x15, 0x1F
UPPER = {"1/2": (G0, G1), "1/6": (G0, G1, G2, G3)}
LOWER = {"1/2": (G1,), "1/6": (G1, G3)}


def crc16(data: bytes) -> int:
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def soft_pn() -> np.ndarray:
    reg, out = 0xFF, []
    for _ in range(255):
        out.append(reg & 1)
        fb = (reg ^ (reg >> 3) ^ (reg >> 5) ^ (reg >> 7)) & 1
        reg = (reg >> 1) | (fb << 7)
    return np.array(out, dtype=np.uint8)


def constituent(bits, polys) -> np.ndarray:
    """the 16-state recursive encoder (feedback 10011), terminated in four steps: [len(bits) + 4][len(polys)] output bits; G0's own output is the input bit"""
    out = np.zeros((len(bits) + 4, len(polys)), np.uint8)
    s = 0
    for i in range(len(bits) + 4):
        old = ((s >> 1) ^ s) & 1
        u = int(bits[i]) if i < len(bits) else old  # termination: the input cancels the feedback
        fb = old ^ u
        for j, p in enumerate(polys):
            o = ((p >> 4) & 1) & fb
            for k in range(4):
                o ^= ((p >> (3 - k)) & 1) & ((s >> (3 - k)) & 1)
            out[i, j] = o
        s = (s >> 1) | (fb << 3)
    assert s == 0
    return out


def encode(rate: str, frame: np.ndarray, pi: np.ndarray) -> np.ndarray:
    bits = np.unpackbits(frame)
    up, lo = constituent(bits, UPPER[rate]), constituent(bits[pi], LOWER[rate])
    if rate == "1/2":  # the systematic bit, then the upper parity in even steps and the lower one in odd steps
        odd = (np.arange(len(up)) & 1).astype(bool)
        return np.stack([up[:, 0], np.where(odd, lo[:, 0], up[:, 1])], axis=1).reshape(-1)
    return np.concatenate([up, lo], axis=1).reshape(-1)


def make_stream(rate: str, base: int, pi: np.ndarray) -> np.ndarray:
    """DISTINCT frames of ASM + randomised codeword as int8 soft bytes"""
    rng = np.random.default_rng(13900 + base + len(ASM_HEX[rate]))
    asm = np.array([(int(ch, 16) >> (3 - k)) & 1 for ch in ASM_HEX[rate] for k in range(4)], dtype=np.uint8)
    out = []
    for _ in range(DISTINCT):
        body = rng.integers(0, 256, base - 2).astype(np.uint8)
        c = crc16(body.tobytes())
        cw = encode(rate, np.concatenate([body, np.array([c >> 8, c & 0xFF], np.uint8)]), pi)
        out.append(np.concatenate([asm, cw ^ np.resize(soft_pn(), len(cw))]))
    v = np.concatenate(out).astype(np.float64) * 2.0 - 1.0
    return np.clip(np.rint(v * AMP + SIGMA[rate] * rng.standard_normal(len(v))), -127, 127).astype(np.int8)


def merge(update: dict):
    cur = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            cur = json.load(f)
    for k, v in update.items():
        if isinstance(v, dict) and isinstance(cur.get(k), dict):
            cur[k].update(v)
        else:
            cur[k] = v
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
        f.write("\n")
    return cur


def interleaver(base: int) -> np.ndarray:
    """CCSDS 131.0-B section 6.3 (the library's table is tested against the reference's; this one is the bench's own, so that --cpu-baseline needs no device library)"""
    p = [31, 37, 43, 47, 53, 59, 61, 67]
    out = np.zeros(8 * base, np.int64)
    for s in range(1, 8 * base + 1):
        m = (s - 1) % 2
        i = (s - 1) // (2 * base)
        j = (s - 1) // 2 - i * base
        t = (19 * i + 1) % 4
        c = (p[t % 8] * j + 21 * m) % base
        out[s - 1] = 2 * (t + c * 4 + 1) - m - 1
    return out


def cpu_baseline(args) -> dict:
    import gen_ccsds_turbo_golden as gen
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(args.ref, tmp)
        for key, (rate, base, iters) in SETTINGS.items():
            soft = make_stream(rate, base, interleaver(base))
            F = len(soft) // DISTINCT
            soft = soft[: args.cpu_frames * F]
            p = dict(turbo_rate=rate, turbo_base=base, turbo_iters=iters)
            t0 = time.perf_counter()
            r = gen.run_module(L, p, soft)
            dt = time.perf_counter() - t0
            assert len(r["offset"]) == args.cpu_frames and r["crc_ok"].all() and not r["pos"].any(), (key, r["pos"], r["crc_ok"])
            res[key] = {"value": round(args.cpu_frames / dt, 3), "unit": "frames/s", "seconds_per_frame": round(dt / args.cpu_frames, 3), "cores": 1, "kind": "reference", "frames": args.cpu_frames,
                        "host": "another host than the GPU figure's: the machine the fixtures are generated on, one thread",
                        "sample": f"the module's loop (correlator, derand_ccsds_soft, CCSDSTurbo::decode, {iters} iterations, CRC) on the same stream's first frames"}
    return {"cpu_baseline": res}


def event_ms(torch, fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def bcjr_error(torch, capi) -> dict:
    u = np.load(os.path.join(ROOT, "tests", "golden", "turbo", "turbo_unit.npz"))
    L = 223 * 8
    out = {}
    for tag, rate in (("bcjr_r12", "1/2"), ("bcjr_r16", "1/6")):
        for code, stream, start, want in ((0, u[tag + "_stream0"], np.full((2, L), np.log(0.5)), u[tag + "_after_upper"]), (1, u[tag + "_stream1"], u[tag + "_lower_in"], u[tag + "_after_lower"])):
            d_s, d_m = torch.from_numpy(np.array(stream)).cuda(), torch.from_numpy(np.array(start)).cuda()
            assert capi.lib().sdhip_op_ccsds_turbo_bcjr(0, capi.CCSDS_TURBO_RATES[rate], 223, code, d_s.data_ptr(), 1, d_m.data_ptr()) == 0, capi.last_error()
            got = d_m.cpu().numpy()
            out[f"{tag}_code{code}"] = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    out["max"] = max(out.values())
    return out


def bcjr_late_error(torch, capi) -> dict:
    """the same measure over the late-iteration passes of turbo_iter_r*.npz (the iteration before a frame's first clean one, and iteration 8), teacher-forced"""
    out = {}
    for tag, rate in (("r12", "1/2"), ("r13", "1/3"), ("r14", "1/4"), ("r16", "1/6")):
        g = np.load(os.path.join(ROOT, "tests", "golden", "turbo", f"turbo_iter_{tag}.npz"))
        p, worst = g["passes"], 0.0
        for x in range(2):
            for code, stream, start, want in ((0, g["stream0"], p[x, 0], p[x, 1]), (1, g["stream1"], p[x, 2], p[x, 3])):
                d_s, d_m = torch.from_numpy(np.array(stream)).cuda(), torch.from_numpy(np.array(start)).cuda()
                assert capi.lib().sdhip_op_ccsds_turbo_bcjr(0, capi.CCSDS_TURBO_RATES[rate], 223, code, d_s.data_ptr(), 1, d_m.data_ptr()) == 0, capi.last_error()
                worst = max(worst, float(np.max(np.abs(d_m.cpu().numpy() - want) / np.maximum(1.0, np.abs(want)))))
        out["turbo_iter_" + tag] = worst
    out["max"] = max(out.values())
    return out


def gpu(args) -> dict:
    import torch
    assert torch.cuda.is_available(), "tools/bench_ccsds_turbo.py measures on the GPU: no device, no figure"
    torch.zeros(1, device="cuda")
    from satdump_amd import capi
    L = capi.lib()
    L.sdhip_pool_enable(1)
    res = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "reps": args.reps, "warmup": args.warmup, "bcjr_message_error": bcjr_error(torch, capi),
           "bcjr_late_message_error": bcjr_late_error(torch, capi)}
    for key, (rate, base, iters) in SETTINGS.items():
        soft = make_stream(rate, base, capi.ccsds_turbo_interleaver(base).astype(np.int64))
        tiles = max(1, args.frames // DISTINCT)
        d_soft = torch.from_numpy(soft).cuda().repeat(tiles)
        n = int(d_soft.numel())
        nfr = tiles * DISTINCT
        d_out = torch.zeros((nfr + 8) * (base + 4), dtype=torch.uint8, device="cuda")
        cfg = capi.ccsds_turbo_cfg(rate=rate, base=base, iterations=iters)
        handles = [capi.CcsdsTurbo(cfg) for _ in range(args.warmup + args.reps + 1)]
        frames_out = []

        def module():
            frames_out.append(handles.pop().process_dev(d_soft.data_ptr(), n, d_out.data_ptr(), nfr + 8))

        for _ in range(args.warmup):
            module()
        ms = event_ms(torch, module, args.reps)
        med = float(np.median(ms))
        r = {"rate": rate, "base": base, "iterations": iters, "frames": nfr, "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
             "frames_per_s": round(nfr / med * 1e3, 1), "mbit_per_s": round(nfr * base * 8 / med * 1e3 / 1e6, 2)}
        capi.prof_enable(True)
        capi.prof_reset()
        module()
        torch.cuda.synchronize()
        r["kernels_ms"] = {k: round(v[0], 3) for k, v in sorted(capi.prof_get().items(), key=lambda kv: -kv[1][0])}
        r["kernel_launches"] = {k: int(v[1]) for k, v in capi.prof_get().items()}
        capi.prof_enable(False)
        assert all(k == nfr for k in frames_out), (frames_out, nfr)  # every frame decoded and its CRC held
        first = d_out[: base + 4].cpu().numpy()
        assert bytes(first[:4]) == bytes([0x1A, 0xCF, 0xFC, 0x1D])
        r["frames_out"] = int(frames_out[-1])
        r["workload"] = f"{nfr} frames of {n // nfr} soft bytes, +-{AMP:g} with sigma {SIGMA[rate]:g}, in lock"
        res[key] = r
        print(key, json.dumps(r), flush=True)
        del d_soft, d_out
    return {"gpu": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=3)
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=None, help="write the result here instead of merging it into profiles/ccsds_turbo_bench.json")
    args = ap.parse_args()
    r = cpu_baseline(args) if args.cpu_baseline else gpu(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        r = merge(r)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
