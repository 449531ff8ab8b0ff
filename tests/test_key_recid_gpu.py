"""The recovery id of a signature under a known key in one pass (ellgpu_ecdsa_recid), on the device:
the reference's recorded answers (tests/golden/key_recid.json) through host memory and device
tensors, and per curve one 257-item batch whose expected bytes are the Python-integer model's
(tests/key_recid_checks.py), run at the sizes at which k1 G + k2 P changes its kernel form -- the
larger sizes draw their items from that batch in a shuffled order, so the model is computed once."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_recid_checks as KR  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257, 641, 4099]


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import elliptic_amd
    c = elliptic_amd.Context(0)
    yield c
    c.close()


def _sized(name, n):
    bt = KR.random_batch(name, 257)
    assert KR.meets_conditions(bt)
    return bt.first(n) if n <= bt.n else bt.tiled(n)


def _thresholds():
    """the batch sizes at which Engine::form_for and the row layer's gate change the kernel form, as
    Engine::init_tuning derives them from the device's compute units"""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    wave_round = cu * 4 * 64
    return {"coop_grid": cu * 16 // 3, "row_from": cu * 5 // 2, "row_grid": cu * 18, "parted_grid": wave_round // 2,
            "small_grid": 3 * wave_round}


@pytest.mark.parametrize("name", KR.PRESETS)
def test_golden(ctx, name):
    spec = KR.spec_of(name)
    for shuffled in (False, True):
        for bt in KR.fixture_batches(spec, shuffled):
            a = KR.check(ctx, name, bt, "host")
            b = KR.check(ctx, name, bt, "dev_torch")
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            if not shuffled:
                KR.check_recover_agrees(ctx, name, bt)
                if name in ("secp256k1", "p256", "p384") and bt.h.shape[1] == spec["B"]:
                    KR.check_verify_agrees(ctx, name, bt)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["secp256k1", "p256"])
def test_sizes(ctx, name, n):
    bt = _sized(name, n)
    KR.check(ctx, name, bt, "dev_torch")
    KR.check(ctx, name, bt, "host")


def test_every_form_of_the_endomorphism_curve(ctx):
    """one n above each threshold form_for knows on secp256k1: a wave per part, a row per item, a
    lane per part, and the full grid above the largest of them"""
    t = _thresholds()
    for n in sorted({t["row_from"] + 1, t["coop_grid"] + 1, t["row_grid"] + 1, t["parted_grid"] + 1, t["small_grid"] + 1}):
        KR.check(ctx, "secp256k1", _sized("secp256k1", n), "dev_torch")


def test_above_the_row_layer_of_p256(ctx):
    t = _thresholds()
    for n in (t["coop_grid"], t["coop_grid"] + 1, t["small_grid"] + 1):
        KR.check(ctx, "p256", _sized("p256", n), "dev_torch")


@pytest.mark.parametrize("name,n", [("p384", 1), ("p384", 65), ("p384", 257), ("p521", 1), ("p521", 65), ("p521", 257),
                                    ("p192", 65), ("p224", 65)])
def test_other_curves(ctx, name, n):
    bt = KR.random_batch(name, 257 if name in ("p384", "p521") else 65)
    assert KR.meets_conditions(bt)
    KR.check(ctx, name, bt.first(n), "dev_torch")
    KR.check(ctx, name, bt.first(n), "host")


@pytest.mark.parametrize("name", ["secp256k1", "p256", "p384"])
def test_cross_checks(ctx, name):
    bt = KR.random_batch(name, 257)
    KR.check_recover_agrees(ctx, name, bt)
    KR.check_verify_agrees(ctx, name, bt)
    KR.check_no_poison(ctx, name, bt, "dev_torch")


def test_overlapping_device_operands_are_refused(ctx):
    import torch
    from elliptic_amd import _lib
    bt = _sized("secp256k1", 64)
    h, r, s, pub = (torch.from_numpy(a).cuda() for a in (bt.h, bt.r, bt.s, bt.pub))
    buf = torch.zeros(64 * 64 + 128, dtype=torch.uint8, device="cuda")
    pub2 = buf[:64 * 64].view(64, 64)
    pub2.copy_(pub)
    rec, st = (torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(2))
    for out in ((buf[64 * 64 - 1:64 * 64 + 63], st), (rec, buf[64 * 64 - 1:64 * 64 + 63]), (rec[:64], rec[:64])):
        with pytest.raises(_lib.EllgpuError) as e:
            ctx.ecdsa_recid("secp256k1", h, r, s, pub2, out=out)
        assert e.value.code == -2 and "overlap" in str(e.value)
    ctx.ecdsa_recid("secp256k1", h, r, s, pub2, out=(buf[64 * 64:64 * 64 + 64], st))
    torch.cuda.synchronize()
    assert (buf[64 * 64:64 * 64 + 64].cpu().numpy() == bt.recid).all() and (st.cpu().numpy() == bt.status).all()
    with pytest.raises(ValueError):
        ctx.ecdsa_recid("secp256k1", h, r, s, pub)                      # device tensors need out=
    with pytest.raises(ValueError):
        ctx.ecdsa_recid("secp256k1", h, r, s[:, :31], pub, out=(rec, st))


def test_three_items_per_inversion():
    """a fresh process with ELLGPU_PREP_K=3 ELLGPU_NORM_K=3 on secp256k1 at n = 257: groups of three
    with a status-3 item first, in the middle and last"""
    KR.run_child(["dev_torch", 257, "secp256k1"], KR.K3_ENV)
