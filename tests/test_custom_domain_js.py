"""Engine#defineShortDomain through the N-API addon (tools/check_custom_domain_engine.js): the
domains of tests/golden/custom_ecdsa.json through ecdsaVerifyBatch, mulBatch(id, k, null) and
mulAddBatch(id, k1, null, ...), on the CPU unit-test build of the device code and on the device."""
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
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_domain_engine.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["curves"] == 5 and res["checked"] > 300 and res["refused"] > 0
    return res


def test_engine_domain_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_engine_domain_device():
    _run(None)


def _install_check(lib, custom=True):
    """tools/check_custom_ecdsa.js: install() on ECDSA over user-defined domains against an
    unpatched copy of the reference"""
    if shutil.which("node") is None:
        pytest.skip("node not available")
    from oracle import make_ref
    ref = make_ref.present()
    if ref is None:
        pytest.skip("no copy of the reference in oracle/_ref (made by build())")
    from elliptic_amd.js import build as jb
    jb.build()
    env = dict(os.environ, ELLIPTIC_REFERENCE=ref, ELLGPU_CUSTOM="1" if custom else "0")
    if lib:
        env["ELLGPU_LIB"] = lib
        env["ELLGPU_WIDE_GRID"] = "0"
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "check_custom_ecdsa.js")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["checked"] > 1000
    return res


def test_install_custom_ecdsa_hostsim():
    from hostsim.build import build as build_hostsim
    res = _install_check(build_hostsim())
    assert res["custom"] and res["offCurve"] > 0


def test_install_custom_ecdsa_off_hostsim():
    from hostsim.build import build as build_hostsim
    assert _install_check(build_hostsim(), custom=False)["gpuCalls"] == 0


@pytest.mark.gpu
def test_install_custom_ecdsa_device():
    res = _install_check(None)
    print(json.dumps(res))
