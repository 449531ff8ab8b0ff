"""Engine#customDeriveBatch, customDeriveWireBatch, customValidateBatch, customEncodePointBatch and
their Async forms through the N-API addon (tools/check_custom_ecdh_engine.js): every case of
tests/golden/custom_ecdh.json, on the CPU unit-test build of the device code and on the device."""
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
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_ecdh_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "custom_ecdh.json")) as f:
        gold = json.load(f)
    # derive and derive_wire twice (the synchronous and the Promise form), validate and encode four
    # times (x with / without the order test, x full / compact), validate once more on the plain id,
    # and four refusals per domain (the order test on the plain id, three wrong coordBytes)
    want = sum(2 * len(c["derive"]) + 2 * len(c["derive_wire"]) + 5 * len(c["validate"]) + 4 * len(c["encode"]) + 4
               for c in gold)
    assert res["ok"] and res["curves"] == 6 and res["checked"] == want and want >= 1200
    return res


def test_engine_custom_ecdh_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_custom_ecdh_device():
    _run(None)
