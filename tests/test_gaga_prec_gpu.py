"""The GAGAvatar head with its upsampler in the bf16x3 mode, on the small head of tests/gaga_cases.py: ``render_clip`` stays one library
call and stays bit-identical to the chain of the package's own pieces (the rig of tests/test_gaga_gpu.py) with the chain's upsampler
in the same mode, and a switch between two clips keeps the library object and with it the forehead EMA state."""
import types

import pytest
import torch

import gaga_cases as gc
from test_gaga_gpu import Rig, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    r.want, r.want_state = r.chain(r.codes)      # the f32 chain (computed once, shared, read only)
    r.unet.set_precision("bf16x3")
    r.want3, _ = r.chain(r.codes)
    r.want3_second, _ = r.chain(r.codes, state=r.want_state)      # a second clip in bf16x3 that continues the first clip's EMA
    r.unet.set_precision("f32")
    return r


def _fresh(rig, mode):
    rig.head.set_slab(gc.SLAB)
    rig.head.set_avatar_id("a")
    rig.head.set_precision(mode)
    rig.head.reset_motion_state()
    return rig.head


def test_render_clip_equals_the_chain_in_bf16x3(rig):
    head = _fresh(rig, "bf16x3")
    assert head.precision == "bf16x3"
    got = head.render_clip(rig.codes, rig.flame, randomize_noise=False)
    assert torch.equal(_bits(got), _bits(rig.want3))
    assert not torch.equal(_bits(got), _bits(rig.want))
    diff = float((got.cpu() - rig.want).abs().max())
    print(f"max-abs difference between the f32 and the bf16x3 frames: {diff:.3e}")
    assert diff < 0.5 / 255      # (S = 16, synthetic weights: far below one 8-bit grey level)
    assert torch.equal(_bits(_fresh(rig, "f32").render_clip(rig.codes, rig.flame, randomize_noise=False)), _bits(rig.want))


def test_a_switch_between_clips_keeps_the_ema_state(rig):
    head = _fresh(rig, "f32")
    first = head.render_clip(rig.codes, rig.flame, randomize_noise=False)
    handle = head._h.value
    head.set_precision("bf16x3")
    second = head.render_clip(rig.codes, rig.flame, randomize_noise=False)
    assert head._h.value == handle, "the switch built a new library object"
    assert torch.equal(_bits(first), _bits(rig.want))
    assert torch.equal(_bits(second), _bits(rig.want3_second))
    assert not torch.equal(_bits(second), _bits(rig.want3)), "the state was reset"
    head.set_precision("f32")


def test_engine_takes_gaga_precision(rig):
    from artalk_amd.engine import ARTAvatarInferEngine
    _fresh(rig, "f32")
    eng = ARTAvatarInferEngine(load_gaga=True, gaga=rig.head, gaga_flame=rig.flame, model=types.SimpleNamespace(cfg=None), gaga_precision="bf16x3")
    assert rig.head.precision == "bf16x3"
    rig.head.reset_motion_state()
    torch.manual_seed(8)
    a = eng.rendering(None, rig.codes, shape_id="a")
    torch.manual_seed(8)
    rig.head.reset_motion_state()
    assert torch.equal(_bits(a), _bits(rig.head.render_clip(rig.codes, rig.flame)))
    with pytest.raises(ValueError):
        ARTAvatarInferEngine(gaga=rig.head, gaga_flame=rig.flame, model=types.SimpleNamespace(cfg=None), gaga_precision="fp16")
    rig.head.set_precision("f32")
