"""Engine#customSignBatch, customSignDetBatch and their Async forms through the N-API addon
(tools/check_custom_sign_engine.js): every case of tests/golden/custom_sign.json, on the CPU
unit-test build of the device code and on the device."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _run(lib):
    if shutil.which("node") is None:
        pytest.skip("node not available")
    from elliptic_amd.js import build as jb
    jb.build()
    env = dict(os.environ)
    if lib:
        env["ELLGPU_LIB"] = lib
        env["ELLGPU_WIDE_GRID"] = "0"
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_sign_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "custom_sign.json")) as f:
        cases = sum(len(c["det"]) + len(c["sup"]) for c in json.load(f))
    # every case twice (the synchronous and the Promise form) and one refusal per domain
    assert res["ok"] and res["curves"] == 6 and cases >= 200 and res["checked"] == 2 * cases + 6
    return res


def test_engine_custom_sign_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_custom_sign_device():
    _run(None)
