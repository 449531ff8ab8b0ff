"""Engine#defineMont, customMontLadderBatch, customMontValidateBatch, customMontDeriveBatch and their
Async forms through the N-API addon (tools/check_custom_mont_engine.js): every case of
tests/golden/custom_mont.json, on the CPU unit-test build of the device code and on the device."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _run(lib):
    assert shutil.which("node") is not None, "node is needed for the N-API leg (a missing tool is no reason to skip)"
    from elliptic_amd.js import build as jb
    jb.build()
    env = dict(os.environ)
    if lib:
        env["ELLGPU_LIB"] = lib
        env["ELLGPU_WIDE_GRID"] = "0"
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_mont_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "custom_mont.json")) as f:
        gold = json.load(f)
    # every case six times (ladder, validate, derive x the synchronous and the Promise form) and four
    # refusals per curve
    want = sum(6 * (len(c["cases"]) if "cases" in c else sum(len(r["z0"]) for r in c["rows"])) + 4 for c in gold)
    assert res["ok"] and res["curves"] == 5 and res["checked"] == want and want >= 6000
    return res


def test_engine_custom_mont_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_custom_mont_device():
    _run(None)
