"""The N-API addon form by form (tools/record_addon_forms.js --compare): for every export that takes operand
Buffers, a valid two-item call, the same call through callAsync where the operation has an id, the
mul* calls with caller-supplied result Buffers, and the refusals with their exact messages, equal
tests/golden/addon_forms.json -- recorded from the addon in which every operation was written out by hand,
before it became one descriptor per operation.  On the CPU unit-test build of the device code and on the
device: the two builds agree byte for byte, so one fixture serves both."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# callAsync's ids keep their meaning: direct callers of callAsync pass them
OPS = ["mulFixed", "mulVar", "mulAdd2", "ecdsaVerify", "x25519", "ecdsaSignDet", "ecdsaRecover", "ecdsaVerifyWire",
       "decodePoints", "customVerifyWire", "customRecover", "customSign", "customSignDet", "customDerive",
       "customDeriveWire", "customValidate", "customEncodePoints", "customMontLadder", "customMontValidate",
       "customMontDerive", "customEdDecompress", "customEdDecodePoints", "customEdValidate", "customEdDerive",
       "customEdDeriveWire", "customEdEncodePoints", "customEdVerify", "customEdSign", "customEdSignDet", "mulBase",
       "mulBase2", "ecdsaVerifyBase", "eddsaVerifyBase"]


def _run(lib):
    assert shutil.which("node") is not None, "node is needed for the N-API leg (a missing tool is no reason to skip)"
    from elliptic_amd.js import build as jb
    jb.build()
    env = dict(os.environ)
    if lib:
        env["ELLGPU_LIB"] = lib
    else:
        env.pop("ELLGPU_LIB", None)
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "record_addon_forms.js"), "--compare"], env=env,
                       capture_output=True, text=True, timeout=900)
    res = json.loads(p.stdout.strip().splitlines()[-1]) if p.stdout.strip() else {}
    assert p.returncode == 0 and res.get("ok"), json.dumps(res.get("differences", res), indent=1)[:6000] + p.stderr[-3000:]
    with open(os.path.join(ROOT, "tests", "golden", "addon_forms.json")) as f:
        gold = json.load(f)["calls"]
    # every recorded call was made again, every operation with an id also through callAsync
    assert res["calls"] == len(gold) >= 56
    assert res["promiseForms"] == sum(1 for e in gold.values() if "async" in e) >= 39
    assert res["changedCalls"] == sum(len(e["refusals"]) + len(e.get("asyncRefusals", {})) for e in gold.values()) >= 800
    assert res["ops"] == {name: i for i, name in enumerate(OPS)}
    return res


def test_addon_forms_hostsim():
    from hostsim.build import build as build_hostsim
    _run(build_hostsim())


@pytest.mark.gpu
def test_addon_forms_device():
    _run(None)


def test_fixture_covers_every_batch_export_and_id():
    with open(os.path.join(ROOT, "tests", "golden", "addon_forms.json")) as f:
        gold = json.load(f)["calls"]
    with open(os.path.join(ROOT, "elliptic_amd", "js", "ellgpu_napi.c")) as f:
        src = f.read()
    table = src[src.index("static const op_desc ops[]"):src.index("#define N_OPS")]
    exports = re.findall(r'^  \{"(\w+)", -?\d+, "', table, re.M)          # rows with a synchronous export
    assert len(exports) >= 33
    recorded = {k.split(":")[0] for k in gold}
    assert sorted(set(exports) - recorded) == []
    ids = {int(k.split(":")[1].split("/")[0]) for k in gold if k.startswith("customEcdh:")}
    assert ids == set(range(13, 26))
    # every entry records the synchronous result and a Promise-form one that equals it
    for k, e in gold.items():
        assert "names" in e["sync"] or "bare" in e["sync"], k
        if "async" in e:
            assert e["async"] == e["sync"], k


def test_index_js_names_its_op_ids():
    with open(os.path.join(ROOT, "elliptic_amd", "js", "index.js")) as f:
        src = f.read()
    assert len(re.findall(r"_async\(this\.OPS\.\w+,", src)) >= 33
    assert re.findall(r"_async\(\s*\d", src) == [] and re.findall(r"customEcdh\(this\.ctx,\s*\d", src) == []
