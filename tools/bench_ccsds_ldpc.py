#!/usr/bin/env python3
"""ccsds_ldpc_decoder ("ldpc_rate": "7/8", QPSK, direct output, 10 iterations) on one MI355X, soft symbols resident in HBM: frames/s and Mbit/s of
sdhip_ccsds_ldpc_process_dev over a synthetic locked stream (HIP events around the call alone: the handles are created before the timed window, one per call,
since a handle is a stream), and the kernels' own times inside such a call from the library's per-kernel HIP events (sdhip_prof_*: k_cl_correlate, the chain,
k_cl_decode), taken in a run of their own. Writes profiles/ccsds_ldpc_bench.json.

The baseline is the reference module's own loop on one CPU thread, not an earlier state of this code: `--cpu-baseline` (needs the reference tree and g++, no
device) compiles tools/ccsds_ldpc_golden_driver.cpp the way tools/gen_ccsds_ldpc_golden.py does, runs it on a prefix of the SAME stream and merges its frames/s
into the JSON file. The stream is made from a seed (64 distinct frames, tiled: neither side cares that frames repeat), so both runs see the same bytes.
usage: tools/bench_ccsds_ldpc.py [--frames 16384] [--reps 5] | --cpu-baseline [--cpu-frames 512]"""
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
OUT = os.path.join(ROOT, "profiles", "ccsds_ldpc_bench.json")
F, DATA = 8192, 7136
BASE = 64


def make_stream(frames: int, sigma: float):
    """(the 64 distinct frames as one int8 array, tiles): a locked QPSK stream, +-48 with AWGN of `sigma` (the fixtures' 20 makes the module slide on a few
    per cent of its reads -- its 32-bit ASM against 8160 x 4 candidates --, 16 leaves some ten hard-decision errors a frame and the stream in lock)"""
    import gen_ccsds_ldpc_golden as gen
    enc = gen.Encoder()
    rng = np.random.default_rng(7899)
    v = np.concatenate([gen.wire_frame(enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)), True) for _ in range(BASE)]).astype(np.float64) * 2.0 - 1.0
    return gen.quantise(v * gen.AMP + sigma * rng.standard_normal(len(v))), max(1, frames // BASE)


def merge(update: dict):
    cur = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            cur = json.load(f)
    cur.update(update)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
        f.write("\n")
    return cur


def cpu_baseline(args) -> dict:
    import gen_ccsds_ldpc_golden as gen
    base, _ = make_stream(BASE, args.sigma)
    soft = np.tile(base, max(1, args.cpu_frames // BASE))
    nfr = len(soft) // F
    p = dict(constellation=gen.QPSK, derandomize=1, iterations=10, internal_stream=0)
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build_driver(args.ref, tmp)
        gen.run_module(L, p, soft[: 8 * F])  # warm-up
        t0 = time.perf_counter()
        r = gen.run_module(L, p, soft)
        dt = time.perf_counter() - t0
    nfr_in, nfr = nfr, len(r["offset"])  # (a 32-bit ASM: now and then 30 data symbols in a row look more like it than the noisy ASM does, and the module slides)
    assert nfr >= nfr_in * 0.97, (nfr, nfr_in)
    return {"cpu_baseline": {"value": round(nfr / dt, 1), "unit": "frames/s", "mbit_per_s": round(nfr * DATA / dt / 1e6, 2), "cores": 1, "kind": "reference", "frames": nfr, "sigma": args.sigma, "slides": int((r["locked"] == 0).sum()),
                             "sample": "the module's loop (CorrelatorGeneric, rotate_soft, derand_ccsds_soft, CCSDSLDPC over LDPCDecoderGeneric, 10 iterations) on one thread"}}


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


def gpu(args) -> dict:
    import torch
    assert torch.cuda.is_available(), "tools/bench_ccsds_ldpc.py measures on the GPU: no device, no figure"
    torch.zeros(1, device="cuda")
    from satdump_amd import capi
    base, tiles = make_stream(args.frames, args.sigma)
    d_soft = torch.from_numpy(base).cuda().repeat(tiles)
    n = int(d_soft.numel())
    nfr = n // F
    d_out = torch.zeros((nfr + 8) * 1024, dtype=torch.uint8, device="cuda")
    L = capi.lib()
    L.sdhip_pool_enable(1)
    cfg = capi.ccsds_ldpc_cfg(constellation="qpsk", rate="7/8", iterations=10)
    frames_out = []
    handles = [capi.CcsdsLdpc(cfg) for _ in range(args.warmup + args.reps + 1)]  # a handle is a stream: one per call, created outside the timed window

    def module():
        frames_out.append(handles.pop().process_dev(d_soft.data_ptr(), n, d_out.data_ptr(), nfr + 8))

    for _ in range(args.warmup):
        module()
    ms = event_ms(torch, module, args.reps)
    med = float(np.median(ms))
    res = {"module": {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "frames_per_s": round(nfr / med * 1e3, 1),
                      "mbit_per_s": round(nfr * DATA / med * 1e3 / 1e6, 1)}}
    # the kernels' own times inside one more such call (per-kernel events slow the host side: not part of the figure above)
    capi.prof_enable(True)
    capi.prof_reset()
    module()
    torch.cuda.synchronize()
    res["kernels_ms"] = {k: round(v[0], 3) for k, v in sorted(capi.prof_get().items(), key=lambda kv: -kv[1][0])}
    res["kernel_launches"] = {k: int(v[1]) for k, v in capi.prof_get().items()}
    capi.prof_enable(False)
    assert nfr * 0.97 <= frames_out[-1] <= nfr, (frames_out[-1], nfr)  # (the module slides now and then even in lock: see cpu_baseline)
    first = d_out[: 1024].cpu().numpy()
    assert bytes(first[:4]) == bytes([0x1D, 0xFC, 0xCF, 0x1A])
    dec = capi.CcsdsLdpc(cfg)
    levels = dec.levels()
    dec.close()
    return {"gpu": {"device": torch.cuda.get_device_name(0), "frames": nfr, "frames_out": int(frames_out[-1]), "sigma": args.sigma, "reps": args.reps, "warmup": args.warmup, "iterations": 10, "levels": levels, **res,
                    "workload": f"{nfr} QPSK frames of 8192 soft bytes, +-48 with sigma {args.sigma}, derandomised, direct output"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=16.0)
    ap.add_argument("--key", default=None, help="store the result under this key instead of gpu / cpu_baseline")
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=512)
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=None, help="write the result here instead of merging it into profiles/ccsds_ldpc_bench.json")
    args = ap.parse_args()
    r = cpu_baseline(args) if args.cpu_baseline else gpu(args)
    if args.key:
        r = {args.key: next(iter(r.values()))}
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
