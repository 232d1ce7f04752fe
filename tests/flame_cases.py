"""The FLAME vertex-path cases shared by tests/test_flame_cases_cpu.py (the reference alone) and tests/test_flame_joints_gpu.py
(FLAMEModel.forward on the device): one table, the inputs of every case, and its float32 / float64 reference, computed once per
process and handed out read-only.  torch on the CPU only; nothing here touches a device.

A case is (name, V, n_shape, n_exp, T, D, kind, scale):
  V        vertices of synthetic_flame_asset(n_verts=V)
  T, D     frames of the call and DISTINCT frames among them: frames are independent, so a long batch repeats D distinct frames and
           frame t is held to reference row ``rows[t] = t % D`` (make_inputs returns the map; D = T where nothing repeats)
  kind     "all": the five joints (global, neck, jaw, left eye, right eye) at 0.3 * randn, distinct per joint and frame;
           "only0" .. "only4": that joint alone, the others exactly zero; "angles": the rows of ANGLE_ROWS

The bar of a case is BAR_FACTOR * max(e32, 2^-23 * max|want64|) with e32 = max|oracle32 - oracle64| on the case's own inputs: the
reference's float32 error, never the kernel's.

One input is no case, on purpose: a joint whose three components all equal exactly -1e-8 makes ``rot_vecs + 1e-8`` the zero vector in
float32, the reference's batch_rodrigues then divides 0 by 0 and returns NaN, and flame_pose_kernel computes the same 0 / 0."""
import functools
import math
from collections import namedtuple

import torch

from artalk_amd.flame import synthetic_flame_asset
from flame_oracle import batch_rigid_transform, batch_rodrigues, flame_buffers, flame_forward, full_pose_of

JOINTS = ("global", "neck", "jaw", "eye_l", "eye_r")
BAR_FACTOR = 4.0          # the project's precedent: the render tests hold the device to 4 x the float32-numpy error
ANGLE_ROWS = ("large: 3.1, pi, 2, 1, 6 rad", "zero", "every component +1e-8", "1e-7 * randn", "1e-5 * randn", "1e-3 * randn", "one component 1e-4")
ZERO_ROW = 1

Case = namedtuple("Case", "name V n_shape n_exp T D kind scale")
Inputs = namedtuple("Inputs", "shape exp pose neck eyes rows")       # D distinct frames each, and rows (T,): frame -> distinct frame
Ref = namedtuple("Ref", "want64 e32 vmax bar")


def _c(name, T, V=5023, n_shape=300, n_exp=100, D=None, kind="all", scale=1.0):
    return Case(name, V, n_shape, n_exp, T, min(T, 8) if D is None else D, kind, scale)


JOINT_CASES = [_c("joints-all", 8)] + [_c("joints-only-" + JOINTS[j], 8, kind=f"only{j}") for j in range(5)]
ANGLE_CASES = [_c("angles", len(ANGLE_ROWS), kind="angles")]
# gemm_config: 32x128 tiles at T <= 32, 64x64 above, 128x128 BK16 from 1024 tiles of 128x128 on: ceil(1153/128) * ceil(15069/128) = 10 * 118
T_CASES = [_c(f"T{T}", T, D=37 if T > 129 else None) for T in (1, 32, 33, 64, 65, 129, 1153)]
# 256 vertices per skin workgroup and per stride of the joint regressor; V = 4: N = 12, below any tile; V = 5024: N % 4 == 0, the 16-byte
# epilogue, which reads the broadcast (ldr = 0) residual of the shape GEMM as vectors: at T = 5, 33, 1153 in all three tile configurations
V_CASES = [_c(f"V{V}-T{T}", T, V=V) for V in (1, 4, 255, 256, 257, 5024) for T in (5, 33)] + [_c("V5024-T1153", 1153, V=5024, D=37)]
# NB = 150 -> K padded to 160; NB = 384: no padding, the whole-array upload of artalk_flame_create; NB = 32: one K step
K_CASES = [_c(f"K{ns}+{ne}-T{T}", T, n_shape=ns, n_exp=ne) for ns, ne in ((100, 50), (300, 84), (1, 31)) for T in (5, 33)]
SCALE_CASES = [_c("scale5", 8, scale=5.0)]
ALL = JOINT_CASES + ANGLE_CASES + T_CASES + V_CASES + K_CASES + SCALE_CASES
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)


def case_id(c):
    return c.name


@functools.lru_cache(maxsize=None)
def asset(V):
    return synthetic_flame_asset(n_verts=V)


def _unit(g, n):
    a = torch.randn(n, 3, generator=g)
    return a / a.norm(dim=1, keepdim=True)


def _angle_rows(g):
    """(7, 15) axis-angles, joint-major: the rows of ANGLE_ROWS"""
    p = torch.zeros(len(ANGLE_ROWS), 5, 3)
    p[0] = _unit(g, 5) * torch.tensor([3.1, math.pi, 2.0, 1.0, 6.0])[:, None]
    p[2] = 1e-8
    for r, s in ((3, 1e-7), (4, 1e-5), (5, 1e-3)):
        p[r] = s * torch.randn(5, 3, generator=g)
    p[6, 2, 1] = 1e-4
    return p.reshape(len(ANGLE_ROWS), 15)


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """The D distinct frames of a case (float32) and the frame -> distinct frame map.  The same bits in every process."""
    g = torch.Generator().manual_seed(2000 + ALL.index(c))
    shape = 0.5 * torch.randn(c.D, c.n_shape, generator=g)
    shape[0] = 0.0                                            # the engine's default shape code
    exp = torch.randn(c.D, c.n_exp, generator=g)
    if c.kind == "angles":
        full = _angle_rows(g)
    else:
        full = 0.3 * torch.randn(c.D, 15, generator=g)
        if c.kind.startswith("only"):
            keep = torch.zeros(5, 3)
            keep[int(c.kind[4:])] = 1.0
            full = full * keep.reshape(1, 15)
    rows = torch.arange(c.T) % c.D
    pose = torch.cat([full[:, 0:3], full[:, 6:9]], dim=1).contiguous()
    return Inputs(shape, exp, pose, full[:, 3:6].contiguous(), full[:, 9:15].contiguous(), rows)


def oracle(c, dtype):
    x = make_inputs(c)
    return flame_forward(asset(c.V), x.shape, x.exp, x.pose, n_shape=c.n_shape, n_exp=c.n_exp, scale=c.scale, neck_pose=x.neck,
                         eye_pose_params=x.eyes, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(c):
    """want64 (D, V, 3) float64, the float32 reference's own error against it, max|want64| and the bar of the case.  Shared: do not write to it."""
    w64 = oracle(c, torch.float64)
    e32 = (oracle(c, torch.float32).double() - w64).abs().max().item()
    vmax = w64.abs().max().item()
    return Ref(w64, e32, vmax, BAR_FACTOR * max(e32, 2.0 ** -23 * vmax))


# ---- wrong versions of the float64 oracle: what a kernel that mishandles a joint would compute
WRONG = ("neck rotation dropped", "left eye rotation dropped", "right eye rotation dropped", "eyes parented to joint 0",
         "jaw rotation transposed", "pose-feature blocks of neck and jaw swapped", "A_j without the - G_j.R J_j term")


def lbs_wrong(wrong, betas, pose, b):
    """oracle ``lbs`` step for step, with one defect (``wrong`` in WRONG; None: no defect, bit for bit ``lbs``)"""
    assert wrong is None or wrong in WRONG
    B, dt = betas.shape[0], betas.dtype
    v_shaped = b["v_template"][None] + torch.einsum("bl,mkl->bmk", betas, b["shapedirs"])
    J = torch.einsum("bik,ji->bjk", v_shaped, b["J_regressor"])
    rot = batch_rodrigues(pose.view(-1, 3)).view(B, -1, 3, 3)
    if wrong == WRONG[4]:
        rot = rot.clone()
        rot[:, 2] = rot[:, 2].transpose(1, 2).clone()
    feat = rot[:, 1:] - torch.eye(3, dtype=dt)
    if wrong == WRONG[5]:
        feat = feat[:, [1, 0, 2, 3]]
    v_posed = torch.matmul(feat.reshape(B, -1), b["posedirs"]).view(B, -1, 3) + v_shaped
    parents = b["parents"].clone()
    if wrong == WRONG[3]:
        parents[3:] = 0
    if wrong in WRONG[:3]:            # the joint stays in the pose features and leaves the chain G_j = G_parent . T_j only
        rot = rot.clone()
        rot[:, (1, 3, 4)[WRONG.index(wrong)]] = torch.eye(3, dtype=dt)
    posed, A = batch_rigid_transform(rot, J, parents)
    if wrong == WRONG[6]:
        A = A.clone()
        A[:, :, :3, 3] = posed        # = G_j: the translation of the chain itself
    T = torch.matmul(b["lbs_weights"][None].expand(B, -1, -1), A.view(B, 5, 16)).view(B, -1, 4, 4)
    homo = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=dt)], dim=2)
    return torch.matmul(T, homo[..., None])[:, :, :3, 0]


def wrong_forward(c, wrong, dtype=torch.float64):
    x = make_inputs(c)
    b = flame_buffers(asset(c.V), c.n_shape, c.n_exp, dtype)
    betas = torch.cat([x.shape.to(dtype), x.exp.to(dtype)], dim=1)
    return lbs_wrong(wrong, betas, full_pose_of(x.pose, x.neck, x.eyes, dtype), b) * c.scale


def zero_pose_blend(c):
    """What a frame of exactly zero pose is, in float64: every A_j is the identity, so the vertex is (sum_j w_vj) * v_shaped - not
    v_shaped itself, for the synthetic weights sum to 1 only to float32."""
    x = make_inputs(c)
    b = flame_buffers(asset(c.V), c.n_shape, c.n_exp, torch.float64)
    betas = torch.cat([x.shape.double(), x.exp.double()], dim=1)
    v_shaped = b["v_template"][None] + torch.einsum("bl,mkl->bmk", betas, b["shapedirs"])
    return b["lbs_weights"].sum(dim=1)[None, :, None] * v_shaped * c.scale

