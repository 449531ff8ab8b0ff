"""Engine#eddsaVerifyBaseBatch and its Async form through the N-API addon
(tools/check_eddsa_verify_base_engine.js): every case of tests/golden/eddsa_verify_base.json for every
key and for the generator alias, and the refusals, on the CPU unit-test build of the device code and on
the device."""
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
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_eddsa_verify_base_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "eddsa_verify_base.json")) as f:
        gold = json.load(f)
    # every case twice (the synchronous and the Promise form), the first key's once more through the
    # alias; five refusals
    want = 2 * (sum(len(cs) for cs in gold["cases"]) + len(gold["cases"][0]))
    assert res["ok"] and res["keys"] == 8 and res["checked"] == want and want >= 2 * 9 * 16
    assert res["refused"] == 5
    return res


def test_engine_eddsa_verify_base_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_eddsa_verify_base_device():
    _run(None)
