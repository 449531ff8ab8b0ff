"""Engine#defineBase, releaseBase, baseInfo, mulBaseBatch, mulBase2Batch and their Async forms through
the N-API addon (tools/check_fixed_base_engine.js): every case of tests/golden/fixed_base.json, on
the CPU unit-test build of the device code and on the device; the result's size follows the curve's
width."""
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
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_fixed_base_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "fixed_base.json")) as f:
        gold = json.load(f)
    # every case twice (the synchronous and the Promise form); four refusals per curve, one more per
    # refused base
    want = sum(2 * (sum(len(m) for m in c["mul"]) + len(c["pairs"])) for c in gold)
    assert res["ok"] and res["curves"] == 9 and res["checked"] == want and want >= 4000
    assert res["refused"] == sum(4 + len(c.get("refused", [])) for c in gold)
    return res


def test_engine_fixed_base_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_fixed_base_device():
    _run(None)
