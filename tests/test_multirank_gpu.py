"""N>1 path on the real engines: two ranks SHARE the one GPU of the test box (SDHIP_BENCH_SHARE_GPU=1, gloo for the tiny
boundary exchange), each cold-starts the HIP demodulator + decoder on its chunk of ONE recording, rank 0 stitches from the
boundary frames. The stitched CADU list must equal what a single rank decodes from the very same recording
(bench.py --gpus 1 --blocks 2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(cmd, env_extra, timeout=900):
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


@pytest.mark.parametrize("workload,frames", [("goes_hrit", 309), ("npp_hrd", 240), ("metop_ahrpt", 252)])
def test_two_ranks_shard_one_recording_on_the_engines(tmp_path, workload, frames):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    # one pass, no warm-up pass: the single-rank run then is ALSO a cold start at sample 0 (with a warm-up pass its engines would
    # carry their lock over from the end of the periodic recording and decode the very first frames too)
    common = ["--full", "--workload", workload, "--frames", str(frames), "--steps", "1", "--warmup", "0", "--cpu-samples", "0"]  # --full: the check and --dump
    one = _run([sys.executable, "bench.py", "--gpus", "1", "--blocks", "2", "--dump", str(tmp_path / "one")] + common, {})
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                "bench.py", "--gpus", "2", "--dump", str(tmp_path / "two")] + common, {"SDHIP_BENCH_SHARE_GPU": "1"})
    assert two["n_gpus"] == 2 and "ONE recording" in two["config"]["sharding"]
    want = np.load(str(tmp_path / "one.rank0.npy"))
    meta = json.load(open(str(tmp_path / "two.json")))
    parts = [np.load(str(tmp_path / f"two.rank{r}.npy"))[d:] for r, d in enumerate(meta["drops"])]
    got = np.concatenate(parts, axis=0)
    assert meta["drops"][0] == 0 and meta["drops"][1] >= 1  # the overlap really was decoded twice
    assert two["check"]["stitched"] == len(got)
    # The single rank's list, WHOLE frames -- sync marker and RS parity included, MetOp (rs_usecheck off) too. Round 4: every rank finds where its soft stream
    # continues its predecessor's (sdhip_shard_align on a few KB of boundary symbols) and starts its decoder on the single stream's Viterbi block grid, so the
    # N decoders decode the very blocks one decoder decodes. The decoders work in whole Viterbi buffers, so the remainder that stays
    # undecoded at the very end of the recording can differ: one frame more or less at the END, none anywhere else.
    m = min(len(got), len(want))
    assert abs(len(got) - len(want)) <= 1 and np.array_equal(got[:m], want[:m]), (got.shape, want.shape, np.flatnonzero((got[:m] != want[:m]).any(axis=1))[:8])
    assert len(got) >= 2 * frames - 4
    assert two["check"]["payload_matching_transmitted"] == two["check"]["cadus_last_step_all_ranks"]
    assert one["check"]["payload_matching_transmitted"] == one["check"]["cadus_last_step"]

    # ---- and against the single-stream REFERENCE decode of the very same recording, full frames, sync marker included
    import bench
    from oracle import pyref
    from satdump_amd import synth
    wl = bench.WORKLOADS[workload]
    rec = synth.Recording(synth.SynthSpec(**wl["spec"]), frames, blocks=2)
    x = rec.synth_range(0, rec.n_samples)
    _, refc, _, _ = bench.ref_decode(pyref.best(), wl, x, want_syms=False)
    k = min(len(got), len(refc))
    assert abs(len(got) - len(refc)) <= 1 and k >= 2 * frames - 4
    # whole frames against the reference too: rank 1 decodes the single stream's blocks from soft symbols that are another trajectory of the same loops on the
    # same samples (+-1 int8 LSB on ~0.1 % of them) -- the Viterbi decoder does not see that
    assert np.array_equal(got[:k], refc[:k]), np.flatnonzero((got[:k] != refc[:k]).any(axis=1))[:8]
