"""DINOBase on the device against the fixtures made from the reference's own module (tools/make_golden_dino.py): the feature plane and
the global vector of cases A, B and C within max(4 x e32, 1 ulp), e32 being the case's float32 restatement against float64 on the CPU
(tests/dino_cases.py); for case A also the four taps and the four layer_rn outputs.  Then what must be bit-identical: two calls, a side
stream, a second object; and the whole identity chain - prepare_image -> forward -> GSGenerators.build_avatar -> add_avatar ->
render_clip - against GAGAvatar.from_checkpoint with the same synthetic dicts.  Run with -s for error / e32."""
import os

import numpy as np
import pytest
import torch

import dino_cases as cases
import gaga_cases as gc
from artalk_amd import dino, gaga, gsgen
from artalk_amd import styleunet as su
from artalk_amd.flame import FLAMEModel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "dino_ref.npz")), np.load(os.path.join(GOLD, "dino_ref_taps.npz"))


_models = {}


def _model(name):
    if name not in _models:
        r = cases.reference_run(name)
        _models[name] = dino.DINOBase(*r["dims"]).load_state_dict(r["sd"])
    return _models[name]


def _check(name, key, got, want, r):
    err = float((got.detach().cpu().double() - torch.from_numpy(np.asarray(want))).abs().max())
    e32, allow = r["e32"][key], r["allow"][key]
    print(f"case {name} {key}: error {err:.2e}, e32 {e32:.2e}, error / e32 {err / e32:.2f}, allowance {allow:.2e}")
    assert err <= allow


@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_the_reference(name, gold):
    r, m = cases.reference_run(name), _model(name)
    f0, f1 = m.forward(torch.from_numpy(r["image"]).cuda()[None])
    od, D, _, _, g = r["dims"]
    assert tuple(f0.shape) == (1, od, 8 * g, 8 * g) and tuple(f1.shape) == (1, D)
    _check(name, "plane", f0[0], gold[0][f"{name}_plane"], r)
    _check(name, "glob", f1[0], gold[0][f"{name}_glob"], r)
    if name == "A":
        stride = int(gold[1]["rn0_channel_stride"])
        for i in range(4):
            _check(name, f"tap{i}", m.read(f"tap{i}"), gold[1][f"A_tap{i}"], r)
            rn = m.read(f"rn{i}")
            _check(name, f"rn{i}", rn[..., ::stride] if i == 0 else rn, gold[1][f"A_rn{i}"], r)
        # the global vector is the first PATCH token of the last tap
        assert torch.equal(f1[0], m.read("tap3")[0, 0])


def test_calls_streams_and_objects_give_the_same_bits():
    r, m = cases.reference_run("C"), _model("C")
    img = torch.from_numpy(r["image"]).cuda()
    a0, a1 = m.forward(img)
    b0, b1 = m.forward(img)      # the object re-used
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c0, c1 = m.forward(img)
    side.synchronize()
    assert torch.equal(a0, c0) and torch.equal(a1, c1)
    other = dino.DINOBase(*r["dims"]).load_state_dict(r["sd"])
    d0, d1 = other.forward(img[None])
    assert torch.equal(a0, d0) and torch.equal(a1, d1)
    # timing on changes nothing and fills every stage
    m.set_timing(True)
    e0, _ = m.forward(img)
    stages, total = m.timing()
    m.set_timing(False)
    assert torch.equal(a0, e0) and total > 0 and all(v > 0 for v in stages.values()) and sum(stages.values()) <= total * 1.05


def test_prepare_image_and_refusals():
    r, m = cases.reference_run("A"), _model("A")
    S = m.image_size
    big = torch.rand(3, 2 * S + 3, 3 * S + 1, generator=torch.Generator().manual_seed(2))
    want = torch.nn.functional.interpolate(big.double()[None], (S, S), mode="bilinear", align_corners=False, antialias=True)
    want32 = torch.nn.functional.interpolate(big[None], (S, S), mode="bilinear", align_corners=False, antialias=True)
    allow = cases.allowance(float((want32.double() - want).abs().max()), 1.0)
    for src in (big, big.cuda(), big[None]):      # host, device, with the batch axis
        got = m.prepare_image(src)
        assert tuple(got.shape) == (1, 3, S, S) and got.is_cuda
        assert float((got.cpu().double() - want).abs().max()) <= allow
    assert torch.equal(m.prepare_image(torch.from_numpy(r["image"]))[0].cpu(), torch.from_numpy(r["image"]))      # the same size: the identity
    with pytest.raises(ValueError, match="interpolated"):
        m.prepare_image(big, size=S + 14)
    with pytest.raises(ValueError, match="square"):
        m.forward(torch.zeros(3, S, S + 14, device="cuda"))
    with pytest.raises(ValueError, match="interpolated"):
        m.forward(torch.zeros(3, S + 14, S + 14, device="cuda"))
    with pytest.raises(ValueError, match="one image"):
        m.forward(torch.zeros(2, 3, S, S, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward(torch.zeros(3, S, S))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        dino.DINOBase(*r["dims"]).forward(torch.zeros(3, S, S, device="cuda"))


# ---- the identity chain at case A's dims, the small StyleUNet and FLAME model of the head's tests
class Chain:
    def __init__(self):
        r = cases.reference_run("A")
        od, D, depth, heads, g = r["dims"]
        self.flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=gc.flame_asset())
        gs_dims = (gc.V, 16, D, od, 8 * g)
        self.ckpt = {"base_model." + k: v for k, v in r["sd"].items()}
        self.ckpt.update(gsgen.synth_state_dict(*gs_dims, seed=1))
        self.unet_sd = su.synth_state_dict(gc.S)
        self.ckpt.update({"upsampler." + k: v for k, v in self.unet_sd.items()})
        self.ckpt["percep_loss.net.weight"] = torch.zeros(3)
        big = torch.rand(3, 97, 83, generator=torch.Generator().manual_seed(5))
        self.tracked = {n: {"image": img, "transform_matrix": torch.from_numpy(_tm(n)), "shapecode": gc.avatar(seed=s)["shapecode"].tolist()}
                        for n, img, s in (("a", big, 2), ("b", torch.from_numpy(r["image"]), 3))}
        self.dino = _model("A")
        self.gen = gsgen.GSGenerators(*gs_dims).load_state_dict(self.ckpt)
        self.codes = gc.motion_codes().cuda()

    def by_hand(self, name):
        e = self.tracked[name]
        f0, f1 = self.dino.forward(self.dino.prepare_image(e["image"]))
        return self.gen.build_avatar(f0, f1, e["transform_matrix"], torch.tensor(e["shapecode"]))


def _tm(name):
    import gsgen_cases
    return gsgen_cases.transform_matrix("A" if name == "a" else "B")


@pytest.fixture(scope="module")
def chain():
    return Chain()


def test_from_checkpoint_equals_the_chain_of_public_calls(chain):
    mark = gc.water_mark()
    av = chain.by_hand("a")
    assert av["xyz"].shape[0] == gc.V + 2 * chain.dino.plane ** 2
    hand = gaga.GAGAvatar({"x": gc.avatar()}, chain.unet_sd, water_mark=mark, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
    hand.add_avatar("a", av)
    hand.set_avatar_id("a")
    want = hand.render_clip(chain.codes, chain.flame, randomize_noise=False)
    head = gaga.GAGAvatar.from_checkpoint(chain.ckpt, chain.tracked, water_mark=mark, flame=chain.flame, forehead_indices=gc.FOREHEAD)
    assert head.image_size == gc.S and head.n_dynamic == gc.V and head.flame_model is chain.flame and not head.all_gagavatar_id
    head.set_avatar_id("a")
    got = head.render_clip(chain.codes, head.flame_model, randomize_noise=False)
    assert got.shape == (gc.T_CLIP, 3, gc.S, gc.S) and float(got.std()) > 0.01
    assert torch.equal(got, want)
    for k in gaga.AVATAR_FIELDS:
        assert torch.equal(head.all_gagavatar_id["a"][k], av[k])


def test_identities_are_generated_once_each(chain, monkeypatch):
    head = gaga.GAGAvatar.from_checkpoint(chain.ckpt, chain.tracked, flame=chain.flame, forehead_indices=gc.FOREHEAD)
    made = []
    orig = head._generate
    monkeypatch.setattr(head, "_generate", lambda name: (made.append(name), orig(name))[1])
    head.set_avatar_id("a")
    a = head.render_clip(chain.codes, chain.flame, randomize_noise=False)
    head.set_avatar_id("b")      # a second identity: generated now
    b = head.render_clip(chain.codes, chain.flame, randomize_noise=False)
    assert made == ["a", "b"] and not torch.equal(a, b)
    bh = chain.by_hand("b")
    assert all(torch.equal(head.all_gagavatar_id["b"][k], bh[k]) for k in gaga.AVATAR_FIELDS)
    kept = head.all_gagavatar_id["a"]
    head.set_avatar_id("a")      # back to the first: its Gaussians are reused
    assert made == ["a", "b"] and head.all_gagavatar_id["a"] is kept
    with pytest.raises(KeyError):
        head.set_avatar_id("nobody.jpg")
    # a new photo under a known name is generated afresh; under a new name it is added
    head.add_avatar_image("a", chain.tracked["b"]["image"], chain.tracked["b"]["transform_matrix"], chain.tracked["b"]["shapecode"])
    head.set_avatar_id("a")
    assert made == ["a", "b", "a"] and all(torch.equal(head.all_gagavatar_id["a"][k], bh[k]) for k in gaga.AVATAR_FIELDS)
    with pytest.raises(RuntimeError, match="from_checkpoint"):
        gaga.GAGAvatar({"x": gc.avatar()}, chain.unet_sd, image_size=gc.S, n_dynamic=gc.V).add_avatar_image("y", None, None, None)


def test_engine_builds_the_head_from_the_checkpoint(chain, tmp_path):
    import types
    from artalk_amd.engine import ARTAvatarInferEngine
    torch.save({"model": chain.ckpt}, tmp_path / "GAGAvatar.pt")
    eng = ARTAvatarInferEngine(load_gaga=True, gaga_ckpt=str(tmp_path / "GAGAvatar.pt"), gaga_tracked=chain.tracked, gaga_flame=chain.flame,
                               model=types.SimpleNamespace(cfg=None))
    got = eng.rendering(None, chain.codes, shape_id="b")
    assert got.shape == (gc.T_CLIP, 3, gc.S, gc.S) and 0.0 <= float(got.min()) and float(got.max()) <= 1.0 and float(got.std()) > 0.01
