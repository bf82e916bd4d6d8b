"""ccsds_ldpc_decoder_hip through the drop-in boundary on the GPU: tests/minihost (a host built from the reference's own headers) loads the plugin and runs the
module file -> file on the streams of tests/golden/ldpc, for both output branches. (The minihost's stand-in list has no entry for the stock id
ccsds_ldpc_decoder, so the `_hip` id is addressed directly.) The file written must be the fixture's bytes and the statistics the module's.

The minihost and the plugin are compiled against the reference's headers: where the reference tree is absent they cannot exist and the tests skip; where it is
present and they are missing, the build is broken and the tests fail."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import test_ccsds_ldpc_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "minihost", "_build", "minihost")
PLUGIN = os.path.join(ROOT, "plugin", "_build", "libsdhip_support.so")
LIB = os.path.join(ROOT, "satdump_amd", "lib", "libsdhip.so")
NAMES = {0: "bpsk", 2: "qpsk", 3: "oqpsk"}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    if not (os.path.exists(HOST) and os.path.exists(PLUGIN)):
        assert not os.path.isdir(os.environ.get("REF", "/root/reference")), "the reference tree is here but the minihost / plugin were not built"
        pytest.skip("no reference tree, no prebuilt minihost / plugin")
    return HOST


def _run(host, job, tmp_path):
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    p = subprocess.run([host, LIB, PLUGIN, "run", str(jp)], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _params(g):
    p = g["params"]
    out = {"constellation": NAMES[p["constellation"]], "ldpc_rate": "7/8", "ldpc_iterations": p["iterations"], "derandomize": bool(p["derandomize"])}
    if p["internal_stream"]:
        out.update(internal_stream=True, internal_cadu_size=p["internal_cadu_size"], internal_asm="%08x" % p["internal_asm"])
    return out


@pytest.mark.parametrize("case,ccsds", [("r78_qpsk_direct", True), ("r78_oqpsk_internal", True), ("r78_bpsk", False)])
def test_module_file_to_file(host, tmp_path, case, ccsds):
    g = G._golden(case)
    inp = tmp_path / "in.soft"
    np.asarray(g["soft"]).tofile(str(inp))
    params = _params(g)
    if not ccsds:
        params["ccsds"] = False
    job = {"mode": "file", "input": str(inp), "output_hint": str(tmp_path / case), "demod": {"module": "ccsds_ldpc_decoder_hip", "parameters": params}}
    rep = _run(host, job, tmp_path)
    assert rep["demod_class"] == "ccsds_ldpc_decoder_hip"
    assert rep["soft"].endswith(".cadu" if ccsds else ".frm")
    want, state = G._expected(g)
    got = np.fromfile(rep["soft"], dtype=np.uint8)
    assert len(got) == len(want) and np.array_equal(got, want)
    st = rep["demod_stats"]
    assert st["correlator_lock"] == bool(g["stats"][0]) and st["ldpc_corr"] == int(g["stats"][1])
    assert np.float32(st["correlator_corr"]).view(np.uint32) == np.asarray(g["stat_cor"]).view(np.uint32)[0]
    assert st["lock_state"] == ("SYNCED" if g["stats"][0] else "NOSYNC")
    if state is not None:
        assert st["deframer_state"] == {2: "NOSYNC", 6: "SYNCING", 12: "SYNCED"}[state] and st["deframer_lock"] == (state == 12)


def test_uncovered_parameter_sets_are_refused(host, tmp_path):
    """the `_hip` id refuses what the device path does not cover (under SDHIP_OVERRIDE=1 the stock id keeps the CPU module for these)"""
    g = G._golden("r78_qpsk_direct")
    inp = tmp_path / "in.soft"
    np.asarray(g["soft"])[:8192].tofile(str(inp))
    for over in ({"ldpc_rate": "1/2", "ldpc_block_size": 1024}, {"ldpc2": True}, {"internal_stream": True, "internal_cadu_size": 8275}):
        job = {"mode": "file", "input": str(inp), "output_hint": str(tmp_path / "x"), "instantiate_only": True,
               "demod": {"module": "ccsds_ldpc_decoder_hip", "parameters": dict(_params(g), **over)}}
        jp = tmp_path / "job.json"
        jp.write_text(json.dumps(job))
        p = subprocess.run([host, LIB, PLUGIN, "run", str(jp)], capture_output=True, text=True, env=dict(os.environ), timeout=120)
        assert p.returncode != 0 and "ccsds_ldpc_decoder_hip" in (p.stdout + p.stderr), (over, p.stdout[-500:], p.stderr[-500:])
