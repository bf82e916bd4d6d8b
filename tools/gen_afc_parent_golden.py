#!/usr/bin/env python3
"""tools/gen_afc_parent_golden.py -- records what the engine computes for the cases of tests/afc_variants_util.py as fixtures under tests/golden/afc_parent/.

The fixtures pin the outputs of the commit in front of the k_afc variant work (41e933d): run this on THAT build, once on the GPU (--backend gpu, the library
under satdump_amd/lib) and once on the CPU through the host twin (--backend twin, tests/emu; its sqrtf is not v_sqrt_f32, so the two sets differ from each
other). Later builds must reproduce both byte for byte (tests/test_afc_variants_gpu.py, tests/test_afc_variants_on_twin_cpu.py). Do not re-record on a later
build to make a test pass: a difference is a change of arithmetic.

Each <backend>_<case>.npz holds the sha256 of the whole outputs (int8 soft symbols and float symbols, or the AGC block's samples), their first 4096 values, the
sha256 of the input and the DemodStats chunk counters {chunks, fixed, rotated, inexact, forced, symbols_out}. The recorder insists on what the tests rely on:
no chunk let through unverified (forced == 0), the low cap engaged on part of its stream and the uncapped gain above it there."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import afc_variants_util as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["gpu", "twin"], required=True)
    ap.add_argument("--out", default=U.GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with the fixtures instead of writing them")
    a = ap.parse_args()
    if a.backend == "gpu":
        import torch
        from satdump_amd import capi
        capi.lib()
    else:
        from tests.emu import fake_torch as torch
        capi = U.twin_capi()
        assert capi is not None, "no host clang++ to build the twin with"
    os.makedirs(a.out, exist_ok=True)
    bad = 0
    for name, case in U.CASES.items():
        x = U.signal(case)
        rec = U.run_case(torch, capi, name, x)
        c = dict(zip(U.COUNTERS, rec["counters"].tolist()))
        print(f"{a.backend}_{name}: n {len(x)} {c}", flush=True)
        assert c["chunks_forced"] == 0, "a chunk was let through unverified: not a fixture"
        if case["kind"] == "psk" and not case["cfg"].get("exact"):
            assert c["chunks"] >= 2 * 75
        if case["kind"] == "agc":
            f = U.clamp_fraction(x, rec["_out"], U.LOW_CAP)
            print(f"    share of samples leaving at gain {U.LOW_CAP}: {f:.3f}", flush=True)
            assert (0.2 < f < 0.8) if case.get("capped") else f < 0.01
        keep = {k: v for k, v in rec.items() if not k.startswith("_")}
        if a.check:
            try:
                U.compare(rec, U.load(a.backend, name), name)
            except AssertionError as e:
                bad += 1
                print("    MISMATCH:", e, flush=True)
        else:
            np.savez_compressed(os.path.join(a.out, f"{a.backend}_{name}.npz"), **keep)
    if not a.check:
        lines = ["# produced by tools/gen_afc_parent_golden.py on commit 41e933d (the parent of the k_afc variant work); name, size, key:sha256[:12] of the stored array"]
        for f in sorted(os.listdir(a.out)):
            if f.endswith(".npz"):
                with np.load(os.path.join(a.out, f)) as z:
                    keys = " ".join(f"{k}:{hashlib.sha256(np.ascontiguousarray(z[k]).tobytes()).hexdigest()[:12]}" for k in sorted(z.files))
                lines.append(f"{f}    {os.path.getsize(os.path.join(a.out, f))} B  {keys}")
        open(os.path.join(a.out, "INDEX.txt"), "w").write("\n".join(lines) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
