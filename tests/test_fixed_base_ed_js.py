"""Engine#defineEdBase, then baseInfo, mulBaseBatch, mulBase2Batch, their Async forms and releaseBase
on its handles through the N-API addon (tools/check_fixed_base_ed_engine.js): the recorded answers of
tests/golden/fixed_base_ed.json for four bases per curve and the pairs among them, on the CPU
unit-test build of the device code and on the device."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
BASES = (0, 2, 3, 5)


def _run(lib):
    assert shutil.which("node") is not None, "node is needed for the N-API leg (a missing tool is no reason to skip)"
    from elliptic_amd.js import build as jb
    jb.build()
    env = dict(os.environ)
    if lib:
        env["ELLGPU_LIB"] = lib
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_fixed_base_ed_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, "tests", "golden", "fixed_base_ed.json")) as f:
        gold = json.load(f)
    # every case twice (the synchronous and the Promise form); five refusals per curve and one at the end
    want = sum(2 * (sum(len(c["mul"][b]) for b in BASES) + sum(1 for q in c["pairs"] if q[0] in BASES and q[1] in BASES))
               for c in gold)
    assert res["ok"] and res["curves"] == 4 and res["checked"] == want and want >= 1400
    assert res["refused"] == 5 * len(gold) + 1
    return res


def test_engine_fixed_base_ed_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_fixed_base_ed_device():
    _run(None)
