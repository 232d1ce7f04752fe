"""The FLAME cases of tests/flame_cases.py on the CPU: no device, the reference alone.
  * the extended oracle (all five joints, any dtype) is pinned to the reference's own lbs() by tests/golden/flame_lbs_joints.npz;
  * every case keeps the reference inside its own conditions: float64 finite, float32 within a few units of float32 rounding of it;
  * the all-joints case tells a kernel that mishandles one joint from a right one by more than 1000 bars;
  * every repeated batch says which reference row each of its frames is.
tests/test_flame_joints_gpu.py runs the same table on the device."""
import os

import numpy as np
import pytest
import torch

import flame_cases as fc
from artalk_amd.flame import synthetic_flame_asset
from conftest import GOLDEN
from flame_oracle import flame_buffers, flame_forward, full_pose_of, lbs

# e32 of a case may be at most this many units of 2^-23 * max|v|.  The float32 path rounds through six stages - two sums of up to 400
# products whose terms are a tenth of |v|, the joint regression, Rodrigues' formula, the chain of 3x4 products, the blend of the five
# transforms and the final 3x4 product - of one to two such units each when they add up; beyond that the reference itself is unstable
# at the input and can set no bar.  (Measured: 0.8 .. 4.2 units over the table.)
E32_MAX_UNITS = 16.0


def _joints_golden():
    g = np.load(os.path.join(GOLDEN, "flame_lbs_joints.npz"))
    fp = torch.from_numpy(g["full_pose"])
    return g, dict(shape_params=torch.from_numpy(g["shape"]), expression_params=torch.from_numpy(g["exp"]),
                   pose_params=torch.cat([fp[:, 0:3], fp[:, 6:9]], 1), neck_pose=fp[:, 3:6], eye_pose_params=fp[:, 9:15])


def test_oracle_all_joints_matches_reference_lbs():
    g, kw = _joints_golden()
    assert g["full_pose"].shape == (4, 15) and (g["full_pose"] != 0).all()
    asset = synthetic_flame_asset()
    v32 = flame_forward(asset, **kw)
    assert v32.dtype == torch.float32 and v32.shape == (4, 5023, 3)
    assert np.abs(v32[:, ::37].numpy() - g["verts_sub"]).max() < 1e-6              # the bar of the existing pin (tests/test_flame.py)
    assert abs(v32.double().sum().item() - float(g["verts_sum"])) < 1e-3
    v64 = flame_forward(asset, dtype=torch.float64, **kw)
    assert v64.dtype == torch.float64
    e32 = (v32.double() - v64).abs().max().item()
    assert 0 < e32 < 1e-6
    assert np.abs(v64[:, ::37].numpy() - g["verts_sub"].astype(np.float64)).max() <= 4 * e32


def test_oracle_defaults_are_the_rest_pose_of_neck_and_eyes():
    """the callers of before (global and jaw pose only) get what they got: zeros for the neck and the eyes, float32"""
    g = np.load(os.path.join(GOLDEN, "flame_lbs.npz"))
    shape, m = torch.from_numpy(g["shape"]), torch.from_numpy(g["motion"])
    asset = synthetic_flame_asset()
    a = flame_forward(asset, shape, m[:, :100], m[:, 100:])
    b = flame_forward(asset, shape, m[:, :100], m[:, 100:], neck_pose=torch.zeros(1, 3), eye_pose_params=torch.zeros(6, 6), dtype=torch.float32)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    # other numbers of shape and expression directions than 300 / 100
    c = flame_forward(asset, shape[:, :7], m[:, :5], m[:, 100:], n_shape=7, n_exp=5)
    bf = flame_buffers(asset, 7, 5)
    assert bf["shapedirs"].shape == (5023, 3, 12)
    assert torch.equal(bf["shapedirs"][:, :, 7:], asset["flame_model"]["shapedirs"][:, :, 300:305])
    assert torch.equal(c, lbs(torch.cat([shape[:, :7], m[:, :5]], 1), full_pose_of(m[:, 100:]), bf["v_template"], bf["shapedirs"], bf["posedirs"],
                              bf["J_regressor"], bf["parents"], bf["lbs_weights"]))


def test_table_covers_what_it_names():
    names = set(fc.BY_NAME)
    assert {"joints-all", "angles", "scale5", "V5024-T1153"} | {"joints-only-" + j for j in fc.JOINTS} <= names
    assert {f"T{T}" for T in (1, 32, 33, 64, 65, 129, 1153)} <= names
    assert {f"V{V}-T{T}" for V in (1, 4, 255, 256, 257, 5024) for T in (5, 33)} <= names
    assert {f"K{k}-T{T}" for k in ("100+50", "300+84", "1+31") for T in (5, 33)} <= names
    for c in fc.ALL:
        x = fc.make_inputs(c)
        full = full_pose_of(x.pose, x.neck, x.eyes).reshape(c.D, 5, 3)
        if c.kind == "all":
            assert (full != 0).all() and len(torch.unique(full)) == full.numel(), c.name        # distinct per joint and frame
        elif c.kind.startswith("only"):
            j = int(c.kind[4:])
            rest = [k for k in range(5) if k != j]
            assert (full[:, j] != 0).all() and (full[:, rest] == 0).all(), c.name
    a = full_pose_of(*fc.make_inputs(fc.BY_NAME["angles"])[2:5]).reshape(len(fc.ANGLE_ROWS), 5, 3)
    assert torch.allclose(a[0].norm(dim=1), torch.tensor([3.1, np.pi, 2.0, 1.0, 6.0]), rtol=1e-6)
    assert (a[fc.ZERO_ROW] == 0).all() and (a[2] == np.float32(1e-8)).all() and (a[6] != 0).sum() == 1 and a[6, 2, 1] == np.float32(1e-4)
    for r, s in ((3, 1e-7), (4, 1e-5), (5, 1e-3)):
        assert 0 < a[r].abs().min() and 0.3 * s < a[r].abs().max() < 5 * s
    # the input that is no case: a joint of exactly (-1e-8, -1e-8, -1e-8) is NaN in the reference itself
    for c in fc.ALL:
        full = full_pose_of(*fc.make_inputs(c)[2:5]).reshape(-1, 3)
        assert not (full == np.float32(-1e-8)).all(dim=1).any(), c.name


@pytest.mark.parametrize("c", fc.ALL, ids=fc.case_id)
def test_reference_stays_inside_its_conditions(c):
    r = fc.reference(c)
    assert r.want64.dtype == torch.float64 and r.want64.shape == (c.D, c.V, 3)
    assert torch.isfinite(r.want64).all()
    assert np.isfinite(r.e32) and r.e32 <= E32_MAX_UNITS * 2.0 ** -23 * r.vmax, (c.name, r.e32, r.vmax)
    assert r.bar == 4 * max(r.e32, 2.0 ** -23 * r.vmax) and 0.05 * c.scale < r.vmax < 2 * c.scale


def test_zero_pose_row_is_the_blend_of_v_shaped():
    c = fc.BY_NAME["angles"]
    r = fc.reference(c)
    blend = fc.zero_pose_blend(c)[fc.ZERO_ROW]
    assert (r.want64[fc.ZERO_ROW] - blend).abs().max().item() < 1e-15
    w = fc.asset(c.V)["flame_model"]["weights"].double().sum(dim=1)
    assert 0 < (w - 1).abs().max().item() < 2.0 ** -21            # the weights sum to 1 to float32 only: the blend is not v_shaped itself


def test_lbs_wrong_without_a_defect_is_the_oracle():
    c = fc.BY_NAME["joints-all"]
    assert torch.equal(fc.wrong_forward(c, None), fc.reference(c).want64)
    assert torch.equal(fc.wrong_forward(c, None, torch.float32), fc.oracle(c, torch.float32))


@pytest.mark.parametrize("wrong", fc.WRONG)
def test_all_joints_case_discriminates(wrong):
    c = fc.BY_NAME["joints-all"]
    r = fc.reference(c)
    moved = (fc.wrong_forward(c, wrong) - r.want64).abs().max().item()
    print(f"{wrong}: moves a vertex by {moved:.3g} = {moved / r.bar:.3g} bars")
    assert moved > 1000 * r.bar


@pytest.mark.parametrize("c", [c for c in fc.ALL if c.D < c.T], ids=fc.case_id)
def test_periodic_case_maps_every_frame_to_a_reference_row(c):
    x = fc.make_inputs(c)
    assert x.rows.shape == (c.T,) and x.rows.dtype == torch.int64
    assert x.rows.min() == 0 and x.rows.max() == c.D - 1 and len(torch.unique(x.rows)) == c.D        # every distinct frame is used
    assert torch.equal(x.rows, torch.arange(c.T) % c.D)
    assert all(t.shape[0] == c.D for t in x[:5])
    assert len(torch.unique(x.exp, dim=0)) == c.D and len(torch.unique(torch.cat([x.pose, x.neck, x.eyes], 1), dim=0)) == c.D
