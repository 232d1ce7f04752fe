"""The Gaussian generators as a module (artalk_amd.gsgen.GSGenerators on artalk_gsgen_*) on the case table of tests/gsgen_cases.py,
against the fixtures made from the reference's own classes (tools/make_golden_gsgen.py), and wired into the GAGAvatar head.  Allowance
per attribute: max-abs error <= 4 x e32, e32 being the restatement in float32 against float64 on the CPU (never taken from the kernel),
with a floor of one float32 ulp of the attribute's largest value.  Run with -s for error / e32."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gaga_cases as gc
import gsgen_cases as cases
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import gsgen
from artalk_amd import styleunet as su
from artalk_amd.flame import FLAMEModel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(cases.CASES)
GUARD = 256
POISON = -7.25e9


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "gsgen_ref.npz"))


class Rig:
    def __init__(self, name):
        r = cases.reference_run(name)
        self.name, self.ref = name, r
        self.gen = gsgen.GSGenerators(*cases.CASES[name]).load_state_dict(r["sd"])
        self.f0, self.f1 = torch.from_numpy(r["f0"]).cuda(), torch.from_numpy(r["f1"]).cuda()
        self.tm = torch.from_numpy(r["tm"])
        self.shapecode = torch.linspace(-1, 1, 300)
        self.first = self.gen.build_avatar(self.f0, self.f1, self.tm, self.shapecode)      # computed once, shared, read only


_rigs = {}


@pytest.fixture
def rig(request):
    name = request.param
    if name not in _rigs:
        _rigs[name] = Rig(name)
    return _rigs[name]


by_case = pytest.mark.parametrize("rig", NAMES, indirect=True)


@by_case
def test_equals_golden(gold, rig):
    V = cases.CASES[rig.name][0]
    N = cases.n_gaussians(rig.name)
    for k, w in cases.ATTRS.items():
        got, want = rig.first[k], torch.from_numpy(gold[f"{rig.name}_{k}"])
        assert tuple(got.shape) == (N, w) and got.device.type == "cpu" and bool(torch.isfinite(got).all())
        err, e32, allowed = float((got.double() - want).abs().max()), rig.ref["e32"][k], rig.ref["allow"][k]
        print(f"case {rig.name} {k}: max-abs error {err:.3e}, e32 {e32:.3e}, error / e32 {err / max(e32, 1e-300):.2f}, allowed {allowed:.3e}")
        assert err <= allowed, f"case {rig.name} {k}: error {err:.3e} > allowed {allowed:.3e} (e32 {e32:.3e})"
    assert float(rig.first["xyz"][:V].abs().max()) == 0.0
    assert torch.equal(rig.first["transform_matrix"], rig.tm) and torch.equal(rig.first["shapecode"], rig.shapecode)
    gaga._check_avatar("generated", rig.first, V)


@by_case
def test_bits_repeat_on_any_stream_and_with_a_batch_axis(rig):
    again = rig.gen.build_avatar(rig.f0[None], rig.f1[None], rig.tm, rig.shapecode, device="cuda")
    assert all(again[k].is_cuda for k in cases.ATTRS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = rig.gen.build_avatar(rig.f0, rig.f1, rig.tm, rig.shapecode)
    torch.cuda.current_stream().wait_stream(side)
    for k in cases.ATTRS:
        assert torch.equal(_bits(again[k]), _bits(rig.first[k])), f"{k}: a second call gave other bits"
        assert torch.equal(_bits(other[k]), _bits(rig.first[k])), f"{k}: a side stream gave other bits"


@by_case
def test_exactly_n_rows_are_written(rig):
    N = cases.n_gaussians(rig.name)
    bufs = {k: torch.full((N * w + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda") for k, w in cases.ATTRS.items()}
    for k, w in cases.ATTRS.items():
        bufs[k][GUARD:GUARD + N * w] = float("nan")
    rc = capi.lib().artalk_gsgen_generate(rig.gen._h, capi.ptr(rig.f0), capi.ptr(rig.f1), capi.ptr(rig.tm.contiguous()),
                                          *[capi.ptr(bufs[k][GUARD:]) for k in cases.ATTRS], capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    for k, w in cases.ATTRS.items():
        whole = bufs[k].cpu()
        assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + N * w:] == POISON).all()), f"{k}: written outside its N rows"
        assert torch.equal(_bits(whole[GUARD:GUARD + N * w].reshape(N, w)), _bits(rig.first[k])), f"{k}: a row was left unwritten"


@by_case
def test_a_second_avatar_leaves_no_trace(rig):
    f0b, f1b = rig.f0.flip(1) * 0.7, rig.f1.flip(0) * 1.3
    tmb = torch.from_numpy(cases.transform_matrix("ABCD"[("ABCD".index(rig.name) + 1) % 4]))
    second = rig.gen.build_avatar(f0b, f1b, tmb, rig.shapecode)
    back = rig.gen.build_avatar(rig.f0, rig.f1, rig.tm, rig.shapecode)
    fresh = gsgen.GSGenerators(*cases.CASES[rig.name]).load_state_dict(rig.ref["sd"]).build_avatar(f0b, f1b, tmb, rig.shapecode)
    for k in cases.ATTRS:
        assert torch.equal(_bits(second[k]), _bits(fresh[k])), f"{k}: the second avatar differs from a fresh object's"
        assert torch.equal(_bits(back[k]), _bits(rig.first[k]))
    assert not torch.equal(second["colors"], rig.first["colors"]) and not torch.equal(second["xyz"], rig.first["xyz"])


def test_refusals_on_a_real_object():
    name = "A"
    if name not in _rigs:
        _rigs[name] = Rig(name)
    rig = _rigs[name]
    L = capi.lib()
    x = torch.zeros(50, 16)
    assert L.artalk_gsgen_set_tensor(rig.gen._h, b"head_base", capi.ptr(x), 2, (C.c_int64 * 2)(50, 16)) == capi.ESTATE
    assert L.artalk_gsgen_finalize(rig.gen._h) == capi.ESTATE
    fin = C.c_int32()
    assert L.artalk_gsgen_dims(rig.gen._h, None, None, None, None, None, C.byref(fin)) == (rig.gen.device.index or 0) and fin.value == 1
    with pytest.raises(ValueError, match="f_feature0 must be"):
        rig.gen.build_avatar(rig.f0[:, :5], rig.f1, rig.tm, rig.shapecode)
    with pytest.raises(ValueError, match="f_feature1 must be"):
        rig.gen.build_avatar(rig.f0, rig.f1[:-1], rig.tm, rig.shapecode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rig.gen.build_avatar(rig.f0.cpu(), rig.f1, rig.tm, rig.shapecode)
    bad = rig.tm.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        rig.gen.build_avatar(rig.f0, rig.f1, bad, rig.shapecode)
    with pytest.raises(RuntimeError, match="before load_state_dict"):
        gsgen.GSGenerators(*cases.CASES[name]).build_avatar(rig.f0, rig.f1, rig.tm, rig.shapecode)
    rig.gen.set_timing(True)
    timed = rig.gen.build_avatar(rig.f0, rig.f1, rig.tm, rig.shapecode)
    conv_ms, total_ms = rig.gen.timing()
    rig.gen.set_timing(False)
    assert 0.0 < conv_ms <= total_ms and all(torch.equal(_bits(timed[k]), _bits(rig.first[k])) for k in cases.ATTRS)


def test_wired_into_the_head():
    """build_avatar -> GAGAvatar.add_avatar -> render_clip on the small head of tests/gaga_cases.py (64 vertices, P = 6, 136 Gaussians):
    the frames of a head constructed directly from the same dict, bit for bit, also after switching to another avatar and back."""
    dims = (gc.V, 16, 16, 16, 6)
    assert dims[0] + 2 * dims[4] ** 2 == gc.N
    gen = gsgen.GSGenerators(*dims).load_state_dict(gsgen.synth_state_dict(*dims, seed=5))
    g = torch.Generator().manual_seed(12)
    f0, f1 = torch.randn(1, 16, 6, 6, generator=g).cuda(), torch.randn(1, 16, generator=g).cuda()
    other = gc.avatar()
    made = gen.build_avatar(f0, f1, other["transform_matrix"], other["shapecode"])
    flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=gc.flame_asset())
    sd = su.synth_state_dict(gc.S)
    codes = gc.motion_codes().cuda()
    direct = gaga.GAGAvatar({"made": made}, sd, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
    want = direct.render_clip(codes, flame, randomize_noise=False)
    head = gaga.GAGAvatar({"other": other}, sd, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
    head.set_avatar_id("other")
    base = head.render_clip(codes, flame, randomize_noise=False)
    head.add_avatar("made", made)
    head.set_avatar_id("made")
    head.reset_motion_state()
    got = head.render_clip(codes, flame, randomize_noise=False)
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(base)), "the generated avatar draws what the other one draws"
    head.set_avatar_id("other")
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(codes, flame, randomize_noise=False)), _bits(base))
    head.set_avatar_id("made")
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(codes, flame, randomize_noise=False)), _bits(want))
    # replacing the tracked avatar takes effect on the next clip
    head.add_avatar("made", other)
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(codes, flame, randomize_noise=False)), _bits(base))
