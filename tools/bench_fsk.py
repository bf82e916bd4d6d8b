#!/usr/bin/env python3
"""fsk_demod on one MI355X, samples resident in HBM: complex samples/s of the chunk-parallel handle (sdhip_fsk_demod_create, sdhip_demod_process_dev) on the
parameters of case A of tests/golden/fsk (6 Msps, 2.35 Msym/s GFSK, rrc_alpha 0.35, 20 kHz offset), 2^26 samples per call; one warm-up call, then the median of
five timed calls, and the share of every kernel from HIP events. The result line is printed and written to profiles/.
usage: tools/bench_fsk.py [--samples 67108864] [--steps 5] [--out profiles/fsk_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsk_bench.json"))
    return ap.parse_args(argv)


def run(args) -> dict:
    import torch
    torch.zeros(1, device="cuda")
    from satdump_amd import capi, synth

    # one block of 2^18 symbols, tiled in HBM (the phase is continuous inside a block; a tile seam is one phase step the loops ride through)
    bits = np.random.default_rng(11).integers(0, 2, 1 << 18).astype(np.uint8)
    blk = synth.modulate_fsk(bits, 6e6, 2.35e6, h=0.5, bt=0.5, esn0_db=14.0, cfo_hz=20e3, seed=11)
    reps = max(1, args.samples // len(blk))
    n = reps * len(blk)
    d_x = torch.from_numpy(blk.view(np.float32)).cuda().repeat(reps)
    d_soft = torch.zeros(n // 2 + 64, dtype=torch.int8, device="cuda")
    dem = capi.FskDemod(capi.fsk_cfg("fsk", samplerate=6e6, symbolrate=2.35e6, rrc_alpha=0.35))

    def step():
        return dem.process_dev(d_x.data_ptr(), n, capi.FMT_CF32, d_soft.data_ptr(), n // 2 + 64)

    ns = 0
    for _ in range(args.warmup):
        ns = step()
    first = dem.stats()
    capi.prof_enable(True)
    capi.prof_reset()
    times = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.time()
        ns = step()
        torch.cuda.synchronize()
        times.append(time.time() - t0)
    prof = capi.prof_get()
    capi.prof_enable(False)
    dt = float(np.median(times))
    total = sum(v[0] for v in prof.values()) or 1.0
    kern = {k: {"ms_per_step": round(v[0] / args.steps, 3), "share": round(v[0] / total, 4)} for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])[:10]}
    st = dem.stats()
    return {"metric": "fsk_demod complex samples/s, chunk-parallel mode, samples resident in HBM", "value": round(n / dt / 1e6, 1), "unit": "Msamples/s",
            "ms_per_step": round(dt * 1e3, 3), "steps_ms": [round(t * 1e3, 3) for t in times],
            "config": {"workload": f"GFSK 6 Msps / 2.35 Msym/s, h 0.5, BT 0.5, Es/N0 14 dB, 20 kHz offset, {n} samples per call, module defaults (rrc 0.35 / 31 taps, clock 1.7e-2)"},
            "symbols_per_call": int(ns), "kernels": kern,
            "first_call_chunks": {"chunks": first.chunks, "re_run": first.chunks_fixed, "accepted_by_tolerance": first.chunks_inexact, "let_through": first.chunks_forced},
            "steady_chunks": {"chunks": st.chunks, "re_run": st.chunks_fixed, "accepted_by_tolerance": st.chunks_inexact, "let_through": st.chunks_forced}}


def main():
    args = parse()
    res = run(args)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
