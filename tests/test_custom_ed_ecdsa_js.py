"""Engine#defineEdwardsDomain, customEdVerifyBatch, customEdSignBatch, customEdSignDetBatch and their
Async forms through the N-API addon (tools/check_custom_ed_ecdsa_engine.js): every case of
tests/golden/custom_ed_ecdsa.json, on the CPU unit-test build of the device code and on the device."""
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
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_ed_ecdsa_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "custom_ed_ecdsa.json")) as f:
        gold = json.load(f)
    # every case twice (the synchronous and the Promise form) and, per domain, fourteen refusals and
    # the product that the domain id and the plain id must share
    want = sum(2 * (len(d["verify"]) + len(d["det"]) + len(d["sup"])) + 15 for d in gold)
    assert res["ok"] and res["domains"] == 4 and res["checked"] == want and want >= 500
    return res


def test_engine_custom_ed_ecdsa_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_custom_ed_ecdsa_device():
    _run(None)
