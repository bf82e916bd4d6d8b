#!/usr/bin/env python3
"""What a rocprofv3 --kernel-trace of bench.py says about the FEC handle's batch pipeline (SDHIP_FEC_OVERLAP):

  tools/fec_overlap_trace.py <..._kernel_trace.csv> [--steps N]

Per pair of consecutive Viterbi forward passes (k_vit2h_acs) with no demodulator kernel between them -- two batches of one step --:
  gap      end of the first forward pass -> start of the second: the kernels behind a forward pass and the host round trips among them.
           Serial order: this is the hideable budget H. Pipelined: what is left of it.
  under    kernels that start inside the second forward pass's span, by name, with their summed duration
  tb_after whether the second forward pass starts before the first batch's traceback (k_vit2h_tb) has ended
and the forward pass's duration per launch, first batch of a step against the later ones (the later ones share the chip when pipelined).
Sums are per step (pairs / steps seen: a step = a run of forward passes between demodulator kernels). Prints one JSON object."""
import argparse
import csv
import json
import re
import statistics as st
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--last-steps", type=int, default=20, help="only the last N steps of the trace (the timed ones)")
    a = ap.parse_args()
    rows = []
    with open(a.trace, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name") or r.get("kernel_name") or ""
            s, e = int(r.get("Start_Timestamp") or r["start_timestamp"]), int(r.get("End_Timestamp") or r["end_timestamp"])
            m = re.search(r"(k_[A-Za-z0-9_]+)", name)
            rows.append((s, e, m.group(1) if m else name[:40]))
    rows.sort()
    is_demod = lambda n: n.startswith(("k_afc", "k_mm", "k_chunk"))  # the demodulator handle's kernels: a new step has begun
    acs = [i for i, r in enumerate(rows) if r[2].startswith("k_vit2h_acs")]
    steps, cur = [], []
    for k, i in enumerate(acs):
        if cur and any(is_demod(rows[x][2]) for x in range(cur[-1] + 1, i)):
            steps.append(cur)
            cur = []
        cur.append(i)
    if cur:
        steps.append(cur)
    steps = steps[-a.last_steps:]
    gaps, under, tb_after, first_ms, later_ms, pairs = [], {}, 0, [], [], 0
    for sp in steps:
        first_ms.append((rows[sp[0]][1] - rows[sp[0]][0]) / 1e6)
        g_step = 0.0
        for p, q in zip(sp[:-1], sp[1:]):
            pairs += 1
            later_ms.append((rows[q][1] - rows[q][0]) / 1e6)
            g_step += max(0, rows[q][0] - rows[p][1]) / 1e6
            tb = next((rows[x] for x in range(p + 1, len(rows)) if rows[x][2].startswith("k_vit2h_tb")), None)
            if tb and rows[q][0] < tb[1]:
                tb_after += 1
            for x in range(q + 1, len(rows)):
                if rows[x][0] >= rows[q][1]:
                    break
                u = under.setdefault(rows[x][2], [0, 0.0])
                u[0] += 1
                u[1] += (rows[x][1] - rows[x][0]) / 1e6
        gaps.append(g_step)
    n = max(1, len(steps))
    out = {
        "steps": len(steps), "forward_passes_per_step": st.mean(len(s) for s in steps) if steps else 0, "pairs": pairs,
        "gap_ms_per_step": {"mean": st.mean(gaps) if gaps else 0, "min": min(gaps, default=0), "max": max(gaps, default=0)},
        "second_forward_pass_starts_before_first_traceback_ends": f"{tb_after} of {pairs}",
        "kernels_started_under_a_later_forward_pass_per_step": {k: {"launches": v[0] / n, "ms": round(v[1] / n, 3)} for k, v in sorted(under.items(), key=lambda kv: -kv[1][1])},
        "forward_pass_ms_per_launch": {"first_batch_of_a_step": st.mean(first_ms) if first_ms else 0, "later_batches": st.mean(later_ms) if later_ms else 0},
        "forward_pass_ms_per_step": (sum(first_ms) + sum(later_ms)) / n,
    }
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
