"""Engine#customEdDecompressBatch, customEdDecodePointBatch, customEdValidateBatch, customEdDeriveBatch,
customEdDeriveWireBatch, customEdEncodePointBatch and their Async forms through the N-API addon
(tools/check_custom_ed_engine.js): every case of tests/golden/custom_ed.json, on the CPU unit-test
build of the device code and on the device."""
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
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_ed_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "custom_ed.json")) as f:
        gold = json.load(f)
    # every case twice (the synchronous and the Promise form) -- validate and encode cases four times
    # (with and without the order; compact and full) -- and, per curve, seven refusals and, where the
    # curve has encode cases, the refused width
    want = 0
    for c in gold:
        if "rows" in c:
            want += 2 * 4 * len(c["rows"]) + 7
        else:
            twice = sum(c2["op"] in ("validate", "encode") for c2 in c["cases"])
            want += 2 * (len(c["cases"]) + twice) + 8
    assert res["ok"] and res["curves"] == 9 and res["checked"] == want and want >= 1800
    return res


def test_engine_custom_ed_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_custom_ed_device():
    _run(None)
