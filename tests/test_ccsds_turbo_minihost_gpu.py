"""ccsds_turbo_decoder_hip through the drop-in boundary on the GPU: tests/minihost (a host built from the reference's own headers) loads the plugin and runs the
module file -> file on a stream of tests/golden/turbo. (The minihost's stand-in list has no entry for the stock id ccsds_turbo_decoder, so the `_hip` id is
addressed directly.) The .cadu written must be the fixture's bytes, byte for byte, and the statistics the module's.

The minihost and the plugin are compiled against the reference's headers: where the reference tree is absent they cannot exist and the tests skip; where it is
present and they are missing, the build is broken and the tests fail."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import test_ccsds_turbo_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "minihost", "_build", "minihost")
PLUGIN = os.path.join(ROOT, "plugin", "_build", "libsdhip_support.so")
LIB = os.path.join(ROOT, "satdump_amd", "lib", "libsdhip.so")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    if not (os.path.exists(HOST) and os.path.exists(PLUGIN)):
        assert not os.path.isdir(os.environ.get("REF", "/root/reference")), "the reference tree is here but the minihost / plugin were not built"
        pytest.skip("no reference tree, no prebuilt minihost / plugin")
    return HOST


def _job(g, inp, hint, **over):
    p = g["params"]
    params = dict({"turbo_rate": p["turbo_rate"], "turbo_base": p["turbo_base"], "turbo_iters": p["turbo_iters"]}, **over)
    return {"mode": "file", "input": str(inp), "output_hint": str(hint), "demod": {"module": "ccsds_turbo_decoder_hip", "parameters": params}}


@pytest.mark.parametrize("case", ["r12_b223", "r16_b223"])
def test_module_file_to_file(host, tmp_path, case):
    g = G._golden(case)
    inp = tmp_path / "in.soft"
    np.asarray(g["soft"]).tofile(str(inp))
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(_job(g, inp, tmp_path / case)))
    p = subprocess.run([host, LIB, PLUGIN, "run", str(jp)], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["demod_class"] == "ccsds_turbo_decoder_hip"
    assert rep["soft"].endswith(".cadu")
    want = np.asarray(g["out"])
    got = np.fromfile(rep["soft"], dtype=np.uint8)
    assert len(got) == len(want) and np.array_equal(got, want)
    st = rep["demod_stats"]
    assert st["correlator_lock"] == bool(g["stats"][0]) and st["crc_lock"] == bool(g["stats"][1])
    assert np.float32(st["correlator_corr"]).view(np.uint32) == np.asarray(g["stat_cor"]).view(np.uint32)[0]
    assert st["lock_state"] == ("SYNCED" if g["stats"][0] else "NOSYNC")


def test_bad_parameter_sets_are_refused(host, tmp_path):
    """the module's own exceptions for its three mandatory keys, and hip_devices (under SDHIP_OVERRIDE=1 the stock id keeps the CPU module for it)"""
    g = G._golden("r12_b223")
    inp = tmp_path / "in.soft"
    np.asarray(g["soft"])[:4096].tofile(str(inp))
    for over, msg in (({"turbo_rate": "1/5"}, "Invalid Turbo Rate"), ({"turbo_base": 224}, "Turbo Base must be"), ({"hip_devices": [0, 1]}, "ccsds_turbo_decoder_hip")):
        job = dict(_job(g, inp, tmp_path / "x", **over), instantiate_only=True)
        jp = tmp_path / "job.json"
        jp.write_text(json.dumps(job))
        p = subprocess.run([host, LIB, PLUGIN, "run", str(jp)], capture_output=True, text=True, env=dict(os.environ), timeout=120)
        assert p.returncode != 0 and msg in (p.stdout + p.stderr), (over, p.stdout[-500:], p.stderr[-500:])
