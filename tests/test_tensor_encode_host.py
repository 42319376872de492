"""GPU Huffman emission without a GPU: the model of the kernels' decomposition (tests/emit_model.py) against mjw_emit on adversarial
data units, TensorEncoder's argument errors (raised before any device call) and the lazy torch import."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import emit_model as em
import helpers


def plan_for(ica, w, h, c, q):
    import ctypes as C
    p = ica.binding.WritePlan()
    L = ica.lib()
    L.mjw_plan_init.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    assert L.mjw_plan_init(C.byref(p), w, h, c, q)
    return p


def check(ica, plan, du, tile, stats=None):
    want = ica.emit_jpeg(plan, du)
    T = em.tables_from_header(want[:em.HDR])
    got = em.emit_entropy(T, du, plan.du_per_mcu, tile=tile, stats=stats)
    assert want[-2:] == b"\xff\xd9"
    assert got == want[em.HDR:-2]


@pytest.mark.parametrize("q,w,h", [(90, 64, 48), (95, 40, 24), (30, 16, 16), (100, 8, 8)])
@pytest.mark.parametrize("tile", [128, 5, 2, 1])
def test_model_equals_mjw_emit_on_adversarial_units(ica, q, w, h, tile):
    rng = np.random.default_rng(q * 1000 + w + tile)
    plan = plan_for(ica, w, h, 3, q)
    du = em.adversarial_units(rng, plan.mcu_x * plan.mcu_y, plan.du_per_mcu)
    d = em.dc_diffs(du, plan.du_per_mcu)
    assert d.max() <= 2047 and d.min() >= -2047 and np.abs(du[:, 1:]).max() <= 1023
    if plan.mcu_x * plan.mcu_y >= 4:
        assert d.max() == 2047 and d.min() == -2047
    check(ica, plan, du, tile)


def test_model_zero_runs_eob_and_all_zero_units(ica):
    """runs of 15, 16, 17, 31, 32 and 48 zeros before a value; coefficient 63 set (no EOB); all-zero units"""
    plan = plan_for(ica, 16, 16, 3, 90)  # one 4:2:0 MCU: 6 units
    for run in (15, 16, 17, 31, 32, 48):
        du = np.zeros((6, 64), np.int16)
        du[0, 1 + run] = 5
        du[1, 1 + run] = -1023
        du[2, 63] = 1
        du[3, 1 + run] = 1
        du[3, 63] = -7
        du[4, 1 + run] = 1023  # chroma
        check(ica, plan, du, 128)
        check(ica, plan, du, 1)
    check(ica, plan, np.zeros((6, 64), np.int16), 1)


def test_model_tile_boundary_on_an_ff_byte_and_ff_dense_streams(ica):
    """tiles of one unit over 0xFF-dense units: some byte shared by two tiles is 0xFF (the stuffing of the shared byte)"""
    plan = plan_for(ica, 64, 64, 3, 90)
    rng = np.random.default_rng(5)
    seen = 0
    for it in range(40):
        du = np.stack([em._unit(rng, "ff") for _ in range(plan.mcu_x * plan.mcu_y * 6)])
        du[:, 0] = rng.integers(-1024, 1024, size=du.shape[0])
        stats = {}
        check(ica, plan, du, 1, stats)
        seen += stats.get("shared_ff", 0)
        if seen >= 3:
            break
    assert seen >= 3
    want = ica.emit_jpeg(plan, du)
    assert want.count(b"\xff\x00") > len(want) // 20


def test_model_every_bit_total_residue(ica):
    """bit totals (fill included) at every residue mod 8, multiples of 8 among them: the bits below the last byte are dropped"""
    rng = np.random.default_rng(11)
    plan = plan_for(ica, 8, 8, 3, 95)  # one 4:4:4 MCU: 3 units
    seen = set()
    for it in range(400):
        du = np.zeros((3, 64), np.int16)
        du[:, 0] = rng.integers(-300, 300, size=3)
        for u in range(3):
            k = rng.integers(1, 64, size=int(rng.integers(0, 6)))
            du[u, k] = rng.integers(-40, 41, size=len(k))
        stats = {}
        check(ica, plan, du, 1, stats)
        seen.add(stats["bits"] % 8)
        if len(seen) == 8:
            break
    assert seen == set(range(8))


def test_model_on_the_writers_own_units(ica, golden):
    """the small writer goldens' units (host transform) through the model at the kernels' tile size and at tiles of 3 units"""
    for nm in golden.enc_names:
        img, q = golden[nm + "/rgb"], int(golden[nm + "/q"][0])
        plan, du = ica.host_transform(img, q)
        for tile in (128, 3):
            T = em.tables_from_header(bytes(golden[nm + "/jpg"])[:em.HDR])
            assert em.emit_entropy(T, du, plan.du_per_mcu, tile=tile) == bytes(golden[nm + "/jpg"])[em.HDR:-2], (nm, tile)


def test_tensor_encoder_argument_errors_need_no_device(ica):
    with pytest.raises(ValueError):
        ica.TensorEncoder(device="cpu")
    enc = ica.TensorEncoder()
    a = torch.zeros((3, 16, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        enc.encode([a])  # a CPU tensor
    with pytest.raises(ValueError, match="uint8"):
        enc.encode([a.float()])
    with pytest.raises(ValueError, match="layout"):
        enc.encode([a], layout="NCHW")
    with pytest.raises(ValueError, match="channels"):
        enc.encode([torch.zeros((5, 16, 16), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="channels"):
        enc.encode([torch.zeros((16, 16, 5), dtype=torch.uint8)], layout="HWC")
    for q in (-1, 101, 90.0, True, None):
        with pytest.raises(ValueError, match="quality"):
            enc.encode([a], quality=q)
    with pytest.raises(ValueError, match="4-D"):
        enc.encode(torch.zeros((2, 3, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="stride"):
        enc.encode([torch.zeros((3, 16, 32), dtype=torch.uint8)[:, :, ::2]])
    with pytest.raises(ValueError, match="stride"):
        enc.encode([torch.zeros((16, 16, 3), dtype=torch.uint8).transpose(0, 1)], layout="HWC")
    assert enc.encode([]) == []
    assert enc._ctx is None and enc._enc is None  # nothing touched a device


def test_import_leaves_torch_out_for_the_encoder():
    code = "import sys, image_codecs_amd as ica; assert 'torch' not in sys.modules; ica.Encoder; assert 'torch' not in sys.modules; " \
           "ica.TensorEncoder; assert 'torch' in sys.modules; print('ok')"
    r = subprocess.run([sys.executable, "-c", code], cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
