"""FLAMEModel.forward on the device against the float64 oracle: all five joints, the angle edges, and the launch edges in T, V and K
of the path get_flame_verts -> FLAMEModel.forward -> artalk_flame_verts (two fp32 GEMMs, flame_joints / flame_pose / flame_skin).
The cases and their references are those of tests/flame_cases.py (tests/test_flame_cases_cpu.py checks the table without a device).

The bar of a case: |got - want64| <= 4 * max(e32, 2^-23 * max|want64|), e32 = max|oracle32 - oracle64| on the same inputs, computed
here - the reference's own float32 error, never the kernel's.  Every output frame is compared with its reference row.

Measured on an MI355X, ratio = max|got - want64| / e32 (the bar is 4, or more where e32 < 2^-23 * max|want64|):
  case                       max|got - want64|   e32        ratio   share of the bar
  joints-all                    3.079e-07      2.547e-07   1.21    0.30
  joints-only-global            3.722e-07      2.718e-07   1.37    0.34
  joints-only-neck              3.390e-07      2.932e-07   1.16    0.29
  joints-only-jaw               3.629e-07      2.395e-07   1.51    0.38
  joints-only-eye_l             4.135e-07      2.490e-07   1.66    0.42
  joints-only-eye_r             3.364e-07      2.244e-07   1.50    0.37
  angles                        3.548e-07      2.238e-07   1.59    0.40
  T1                            1.593e-07      1.023e-07   1.56    0.39
  T32                           3.239e-07      2.179e-07   1.49    0.37
  T33                           3.179e-07      2.413e-07   1.32    0.33
  T64                           2.893e-07      2.216e-07   1.30    0.33
  T65                           3.176e-07      2.319e-07   1.37    0.34
  T129                          3.232e-07      2.857e-07   1.13    0.28
  T1153                         3.605e-07      3.168e-07   1.14    0.28
  V1-T5                         8.830e-08      3.091e-08   2.86    0.63
  V1-T33                        1.464e-07      4.889e-08   2.99    0.75
  V4-T5                         1.161e-07      9.376e-08   1.24    0.31
  V4-T33                        1.036e-07      7.600e-08   1.36    0.34
  V255-T5                       1.980e-07      1.656e-07   1.20    0.30
  V255-T33                      2.815e-07      1.679e-07   1.68    0.42
  V256-T5                       3.018e-07      1.284e-07   2.35    0.59
  V256-T33                      2.252e-07      1.537e-07   1.47    0.37
  V257-T5                       2.283e-07      1.681e-07   1.36    0.34
  V257-T33                      2.501e-07      1.693e-07   1.48    0.37
  V5024-T5                      3.178e-07      1.911e-07   1.66    0.42
  V5024-T33                     3.749e-07      2.222e-07   1.69    0.42
  V5024-T1153                   3.718e-07      2.433e-07   1.53    0.38
  K100+50-T5                    1.447e-07      1.231e-07   1.18    0.29
  K100+50-T33                   1.494e-07      1.944e-07   0.77    0.19
  K300+84-T5                    2.888e-07      1.936e-07   1.49    0.37
  K300+84-T33                   3.267e-07      2.644e-07   1.24    0.31
  K1+31-T5                      8.887e-08      9.549e-08   0.93    0.23
  K1+31-T33                     1.074e-07      1.059e-07   1.01    0.25
  scale5                        1.677e-06      1.015e-06   1.65    0.41
  regrow T6                     3.232e-07      2.857e-07   1.13    0.28
  regrow T129                   3.232e-07      2.857e-07   1.13    0.28
  regrow T6 again               3.232e-07      2.857e-07   1.13    0.28
  pose_params=None              3.409e-07      2.566e-07   1.33    0.33
  expression_params=None        3.454e-07      1.609e-07   2.15    0.54
  3-component pose              3.621e-07      2.662e-07   1.36    0.34
  eye_pose_params given         3.237e-07      2.948e-07   1.10    0.27
  eye_pose_params=None          3.196e-07      2.141e-07   1.49    0.37
  device                        3.079e-07      2.547e-07   1.21    0.30
  non-contiguous host           3.079e-07      2.547e-07   1.21    0.30
  non-contiguous device         3.079e-07      2.547e-07   1.21    0.30
  side stream                   3.079e-07      2.547e-07   1.21    0.30
  verts_sclae                   1.677e-06      1.015e-06   1.65    0.41
  get_flame_verts               3.486e-07      2.575e-07   1.35    0.34
  get_flame_verts with_global    3.196e-07      2.141e-07   1.49    0.37
  get_flame_verts 3-d           3.196e-07      2.141e-07   1.49    0.37
No case exceeds 4; the largest ratio, 2.99 at V = 1, is 0.75 of its bar (e32 there is below 2^-23 * max|want64|).  The file takes 3.5 s.
"""
import functools

import numpy as np
import pytest
import torch

import flame_cases as fc
from flame_oracle import flame_forward

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(V=5023, n_shape=300, n_exp=100, scale=1.0):
    from artalk_amd.flame import FLAMEModel
    return FLAMEModel(n_shape=n_shape, n_exp=n_exp, scale=scale, no_lmks=True, flame_ckpt=fc.asset(V))


def _model_of(c):
    return _model(c.V, c.n_shape, c.n_exp, c.scale)


def _kwargs(c, rows=None):
    """the arguments of forward for a case (frames ``rows`` of the distinct ones; default: the case's own T frames) and the neck pose"""
    x = fc.make_inputs(c)
    r = x.rows if rows is None else rows
    return dict(shape_params=x.shape[r], expression_params=x.exp[r], pose_params=x.pose[r], eye_pose_params=x.eyes[r]), x.neck[r]


def _call(fm, kw, neck=None, **more):
    """forward with ``fm.neck_pose`` set for the call, as the reference's buffer would be; the result on the host"""
    if neck is not None:
        fm.neck_pose = neck
    try:
        out = fm(**kw, **more)
    finally:
        fm.neck_pose = torch.zeros(1, 3)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu()


def _err(got, want64, rows):
    """max |got[t] - want64[rows[t]]| over every frame t"""
    assert got.shape == (len(rows),) + tuple(want64.shape[1:]), (got.shape, want64.shape)
    assert torch.isfinite(got).all()
    err = 0.0
    for d in range(want64.shape[0]):
        sel = got[rows == d]
        if len(sel):
            err = max(err, (sel.double() - want64[d]).abs().max().item())
    return err


def _hold(tag, got, ref, rows, factor=fc.BAR_FACTOR):
    err = _err(got, ref.want64, rows)
    bar = factor * max(ref.e32, 2.0 ** -23 * ref.vmax)
    print(f"RATIO {tag}: err {err:.3e} e32 {ref.e32:.3e} ratio {err / ref.e32:.2f} of-bar {err / bar:.2f}")
    assert err <= bar, f"{tag}: max|got - want64| = {err:.3e} > bar {bar:.3e} (e32 {ref.e32:.3e}, ratio {err / ref.e32:.2f})"
    return err


@functools.lru_cache(maxsize=None)
def _got(c):
    kw, neck = _kwargs(c)
    return _call(_model_of(c), kw, neck)


# T1153: gemm_config takes the 128x128 BK16 kernel from 1024 tiles of 128x128 on; M = 1153 -> ceil(1153 / 128) = 10 row tiles,
# N = 3 * 5023 = 15069 (and 3 * 5024 = 15072) -> ceil(N / 128) = 118 column tiles, 10 * 118 = 1180 >= 1024 (T = 1152: 9 * 118 = 1062 too,
# but 1153 also leaves a last row tile of one row).  T <= 32: 32x128 tiles; 33 .. : 64x64 tiles.
@pytest.mark.parametrize("c", fc.ALL, ids=fc.case_id)
def test_case_meets_the_reference_bar(c):
    if c.T == 1153:
        assert -(-c.T // 128) * -(-c.V * 3 // 128) == 10 * 118 >= 1024
    _hold(c.name, _got(c), fc.reference(c), fc.make_inputs(c).rows)


def test_zero_pose_row_is_the_float64_blend_of_v_shaped():
    c = fc.BY_NAME["angles"]
    ref = fc.reference(c)
    got = _got(c)[fc.ZERO_ROW]
    assert (got.double() - fc.zero_pose_blend(c)[fc.ZERO_ROW]).abs().max().item() <= ref.bar


def test_workspace_regrown_and_reused():
    """one handle at T = 6, 129, 6: the second call regrows the workspace, the third runs over the larger buffers"""
    from artalk_amd.flame import FLAMEModel
    c = fc.BY_NAME["T129"]
    ref = fc.reference(c)
    fm = FLAMEModel(n_shape=300, n_exp=100, scale=1.0, no_lmks=True, flame_ckpt=fc.asset(c.V))
    rows6, rows129 = torch.arange(6) % c.D, fc.make_inputs(c).rows
    a = _call(fm, *_kwargs(c, rows=rows6))
    b = _call(fm, *_kwargs(c, rows=rows129))
    d = _call(fm, *_kwargs(c, rows=rows6))
    assert np.array_equal(a.numpy(), d.numpy())
    for tag, got, rows in (("regrow T6", a, rows6), ("regrow T129", b, rows129), ("regrow T6 again", d, rows6)):
        _hold(tag, got, ref, rows)


def test_frame_of_a_batch_equals_the_call_on_that_frame():
    """T = 8 and T = 1 both run 32x128 GEMM tiles, every other kernel works per frame: bit for bit"""
    c = fc.BY_NAME["joints-all"]
    batch = _got(c)
    for t in (0, 3, 7):
        one = _call(_model_of(c), *_kwargs(c, rows=torch.tensor([t])))
        assert np.array_equal(one[0].numpy(), batch[t].numpy()), t


def _wide(t, dev=None):
    """t as a column slice of a wider tensor"""
    w = torch.cat([torch.full((t.shape[0], 3), 7.0), t, torch.full((t.shape[0], 5), -7.0)], dim=1)
    if dev is not None:
        w = w.to(dev)
    v = w[:, 3:3 + t.shape[1]]
    assert not v.is_contiguous() or t.shape[0] == 1
    return v


def test_forward_argument_forms():
    """FLAME.py:127-149 on the frames of the all-joints case; what names the same values gives the same bits"""
    c = fc.BY_NAME["joints-all"]
    fm, x, ref, asset = _model_of(c), fc.make_inputs(c), fc.reference(c), fc.asset(c.V)
    kw, neck = _kwargs(c)
    plain = _got(c)

    def oracle_ref(**o):
        w64 = flame_forward(asset, dtype=torch.float64, **o)
        e32 = (flame_forward(asset, **o).double() - w64).abs().max().item()
        return fc.Ref(w64, e32, w64.abs().max().item(), None)
    rows = torch.arange(c.T)
    z6 = torch.zeros(c.T, 6)
    # pose_params=None: the rest pose of global and jaw (neck and eyes still given)
    got = _call(fm, dict(kw, pose_params=None), neck)
    _hold("pose_params=None", got, oracle_ref(shape_params=x.shape, expression_params=x.exp, pose_params=z6, neck_pose=x.neck, eye_pose_params=x.eyes), rows)
    # expression_params=None: zeros
    got = _call(fm, dict(kw, expression_params=None), neck)
    _hold("expression_params=None", got, oracle_ref(shape_params=x.shape, expression_params=torch.zeros(c.T, c.n_exp), pose_params=x.pose,
                                                     neck_pose=x.neck, eye_pose_params=x.eyes), rows)
    # 3-component pose: the jaw alone, the global rotation zero
    got = _call(fm, dict(kw, pose_params=x.pose[:, 3:]), neck)
    _hold("3-component pose", got, oracle_ref(shape_params=x.shape, expression_params=x.exp, pose_params=torch.cat([torch.zeros(c.T, 3), x.pose[:, 3:]], 1),
                                               neck_pose=x.neck, eye_pose_params=x.eyes), rows)
    # eye_pose_params given / left out, the neck buffer at its default
    got = _call(fm, kw)
    _hold("eye_pose_params given", got, oracle_ref(shape_params=x.shape, expression_params=x.exp, pose_params=x.pose, eye_pose_params=x.eyes), rows)
    got = _call(fm, dict(kw, eye_pose_params=None))
    _hold("eye_pose_params=None", got, oracle_ref(shape_params=x.shape, expression_params=x.exp, pose_params=x.pose), rows)
    # inputs on the device, and as column slices of wider tensors on the host and on the device
    dev = fm.device
    forms = {"device": ({k: v.to(dev) for k, v in kw.items()}, neck.to(dev)),
             "non-contiguous host": ({k: _wide(v) for k, v in kw.items()}, _wide(neck)),
             "non-contiguous device": ({k: _wide(v, dev) for k, v in kw.items()}, _wide(neck, dev))}
    for tag, (k2, n2) in forms.items():
        got = _call(fm, k2, n2)
        _hold(tag, got, ref, rows)
        assert np.array_equal(got.numpy(), plain.numpy()), tag
    # under a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _call(fm, {k: v.to(dev) for k, v in kw.items()}, neck.to(dev))
    torch.cuda.current_stream().wait_stream(side)
    _hold("side stream", got, ref, rows)
    assert np.array_equal(got.numpy(), plain.numpy())


def test_verts_sclae_is_ignored_without_landmarks():
    """FLAME.py:148-149: with no_lmks=True the reference returns vertices * self.scale before it looks at verts_sclae"""
    c = fc.BY_NAME["scale5"]
    fm = _model_of(c)
    assert fm.scale == 5.0
    kw, neck = _kwargs(c)
    plain = _got(c)
    for s in (2.0, 0.0, torch.tensor(3.0)):
        got = _call(fm, kw, neck, verts_sclae=s)
        assert np.array_equal(got.numpy(), plain.numpy()), s
    _hold("verts_sclae", got, fc.reference(c), fc.make_inputs(c).rows)
    from artalk_amd.flame import FLAMEModel
    fm0 = FLAMEModel(n_shape=300, n_exp=100, scale=0.0, no_lmks=True, flame_ckpt=fc.asset(c.V))      # (the old code divided by scale)
    got = _call(fm0, kw, neck, verts_sclae=2.0)
    assert (got == 0).all()


def test_get_flame_verts_forms():
    """model.py get_flame_verts (bitwise_vae.py:43-57): with_global=False zeroes the global rotation; 3-dimensional shape_params loop
    over the leading dimension"""
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.model import _BasicVAE
    c = fc.BY_NAME["joints-all"]
    vae, fm, x, asset = _BasicVAE(ARTalkConfig.tiny()), _model_of(c), fc.make_inputs(c), fc.asset(c.V)
    motion = torch.cat([x.exp, x.pose], dim=1)               # (8, 106)

    def oracle_ref(pose):
        w64 = flame_forward(asset, x.shape, x.exp, pose, dtype=torch.float64)
        e32 = (flame_forward(asset, x.shape, x.exp, pose).double() - w64).abs().max().item()
        return fc.Ref(w64, e32, w64.abs().max().item(), None)
    rows = torch.arange(c.T)
    no_global = torch.cat([torch.zeros(c.T, 3), x.pose[:, 3:]], 1)
    got = vae.get_flame_verts(fm, x.shape, motion).cpu()
    _hold("get_flame_verts", got, oracle_ref(no_global), rows)
    got = vae.get_flame_verts(fm, x.shape, motion, with_global=True).cpu()
    _hold("get_flame_verts with_global", got, oracle_ref(x.pose), rows)
    got3 = vae.get_flame_verts(fm, x.shape.reshape(2, 4, -1), motion.reshape(2, 4, -1), with_global=True).cpu()
    assert got3.shape == (2, 4, c.V, 3)
    _hold("get_flame_verts 3-d", got3.reshape(8, c.V, 3), oracle_ref(x.pose), rows)
    with pytest.raises(ValueError):
        vae.get_flame_verts(fm, x.shape[0], motion[0])
