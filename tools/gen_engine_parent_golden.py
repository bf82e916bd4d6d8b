#!/usr/bin/env python3
"""tools/gen_engine_parent_golden.py -- records what the engine computes for the cases of tests/engine_parent_util.py as fixtures under tests/golden/engine_parent/.

The fixtures pin the outputs AND the kernel launch counts of the commit in front of the host-scaffold refactor of demod_engine.hip (966c66d): run this on THAT
build, once on the GPU (--backend gpu, the library under satdump_amd/lib) and once on the CPU through the host twin (--backend twin, tests/emu; its sqrtf is not
v_sqrt_f32, so the two sets differ from each other). Later builds must reproduce both byte for byte (tests/test_engine_parent_gpu.py,
tests/test_engine_parent_on_twin_cpu.py). Do not re-record on a later build to make a test pass: a difference is a change of behaviour.

Each <backend>_<case>.npz holds, per call c<i> of the stream: the sha256 of the input, of the soft symbols and of the float symbols (or output samples), their
lengths, the DemodStats chunk counters {chunks, fixed, rotated, inexact, forced, symbols_out} and the launches of every kernel (names + counts, from
sdhip_prof_get); beside them the first 4096 values of the whole stream's outputs. The recorder insists on what the tests rely on
(engine_parent_util.check_conditions): no chunk let through unverified except in `noise`, the lanes ran, a re-run in `qpsk_own_warmup`."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import engine_parent_util as U  # noqa: E402


def write_index(out):
    lines = ["# produced by tools/gen_engine_parent_golden.py on commit 966c66d (the parent of the engine's host-scaffold refactor); name, size, sha256[:12] of the file's "
             "arrays taken together. Both backends report launch counts: every fixture holds them."]
    for f in sorted(os.listdir(out)):
        if f.endswith(".npz"):
            h = hashlib.sha256()
            with np.load(os.path.join(out, f)) as z:
                for k in sorted(z.files):
                    h.update(k.encode() + np.ascontiguousarray(z[k]).tobytes())
            lines.append(f"{f}    {os.path.getsize(os.path.join(out, f))} B  {h.hexdigest()[:12]}")
    open(os.path.join(out, "INDEX.txt"), "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["gpu", "twin", "index"], required=True, help="index: only rewrite INDEX.txt from the fixtures that are there")
    ap.add_argument("--out", default=U.GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with the fixtures instead of writing them")
    ap.add_argument("--cases", default="", help="comma-separated subset (default: all)")
    a = ap.parse_args()
    if a.backend == "index":
        return write_index(a.out)
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
    for name in (a.cases.split(",") if a.cases else U.CASES):
        x = U.signal(name)
        rec = U.run_case(torch, capi, name, x)
        print(f"{a.backend}_{name}: {U.counters(rec)}", flush=True)
        print(f"    launches of call 0: {U.launches(rec, 0)}", flush=True)
        try:
            U.check_conditions(name, rec)
            if a.check:
                U.compare(rec, U.load(a.backend, name), name)
        except AssertionError as e:
            bad += 1
            print("    FAILED:", e, flush=True)
            continue
        if not a.check:
            np.savez_compressed(os.path.join(a.out, f"{a.backend}_{name}.npz"), **{k: v for k, v in rec.items() if not k.startswith("_")})
    if not a.check:
        write_index(a.out)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
