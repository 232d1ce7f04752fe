"""The GAGAvatar head's host and element-wise definitions ("GAGAvatar head") restated for the tests.  The reference's
``app/GAGAvatar/models.py`` imports pytorch3d and torchvision at its top and cannot be imported here, so this is a restatement:

  cameras      numpy, ``dtype`` float64 (the oracle) or float32 (the yardstick e32).  It takes pytorch3d's route - axis-angle ->
               quaternion -> matrix - where the library evaluates Rodrigues' formula, so the two share no arithmetic.
  ema, blend   the reference's statements (models.py:120-125, :131-138) in float32, once in numpy and once in torch on the CPU.
``Variant`` swaps in deliberately wrong readings of the camera definition (the CPU tests show that the oracle tells them apart)."""
from dataclasses import dataclass

import numpy as np
import torch

FOCAL, Z_NEAR, Z_FAR = 12.0, 0.01, 100.0


@dataclass(frozen=True)
class Variant:
    flip: bool = True                 # w = (-r0, r1, -r2)
    transpose: bool = True            # the inverse of R . D
    diag_left: bool = True            # D on the left of R^T
    own_translation: bool = True      # the avatar's translation (the reference's initial_trans = (0, 0, 5000 / 512) is dead)


def axis_angle_to_matrix(w, dtype):
    """pytorch3d.transforms.axis_angle_to_matrix for one vector: through the unit quaternion."""
    f = dtype
    w = np.asarray(w, dtype=f)
    angle = np.sqrt((w * w).sum(dtype=f))
    half = angle * f(0.5)
    if abs(float(angle)) < 1e-6:
        s = f(0.5) - angle * angle / f(48)
    else:
        s = np.sin(half) / angle
    r, (i, j, k) = np.cos(half), w * s
    two_s = f(2) / (r * r + i * i + j * j + k * k)
    one = f(1)
    return np.array([[one - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
                     [two_s * (i * j + k * r), one - two_s * (i * i + k * k), two_s * (j * k - i * r)],
                     [two_s * (i * k - j * r), two_s * (j * k + i * r), one - two_s * (i * i + j * j)]], dtype=f)


def cameras(rot_codes, transform_matrix, dtype=np.float64, v=Variant()):
    """rot_codes (T, 3) float32 values, transform_matrix (3, 4) -> (view (T, 4, 4), proj (T, 4, 4), cam (T, 3, 4)) in ``dtype``."""
    f = dtype
    codes = np.asarray(rot_codes, dtype=np.float32).reshape(-1, 3)
    tm = np.asarray(transform_matrix, dtype=np.float32).astype(f)
    D = np.diag(np.array([-1, 1, -1], dtype=f))
    K = np.zeros((4, 4), dtype=f)      # the projection of artalk_amd.splat.build_camera_matrices, transposed for row vectors
    K[0, 0] = K[1, 1] = f(1.0 / np.tan(np.arctan(1.0 / FOCAL)))
    K[2, 2] = f(Z_FAR / (Z_FAR - Z_NEAR))
    K[3, 2] = f(-(Z_FAR * Z_NEAR) / (Z_FAR - Z_NEAR))
    K[2, 3] = f(1)
    views, projs, cams = [], [], []
    for r in codes:
        w = r.astype(f) * (np.array([-1, 1, -1], dtype=f) if v.flip else f(1))
        R = axis_angle_to_matrix(w, f)
        Rt = R.T if v.transpose else R
        M = D @ Rt if v.diag_left else Rt @ D
        t = tm[:, 3] if v.own_translation else np.array([0, 0, 5000.0 / 512], dtype=f)
        cam = np.concatenate([M, t[:, None]], axis=1).astype(f)
        V = np.zeros((4, 4), dtype=f)
        V[:3, :3] = cam[:, :3]
        V[3, :3] = cam[:, 3]
        V[3, 3] = 1
        V[:, :2] *= f(-1)
        views.append(V); projs.append((V @ K).astype(f)); cams.append(cam)
    return np.stack(views), np.stack(projs), np.stack(cams)


# hand-computed [:3, :3] blocks for a quarter turn about each axis of the code (exact in exact arithmetic)
QUARTER_TURNS = {
    0: np.array([[-1, 0, 0], [0, 0, -1], [0, -1, 0]], dtype=np.float64),
    1: np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], dtype=np.float64),
    2: np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1]], dtype=np.float64),
}


def ema_numpy(points, state=None):
    """points (T, K, 3) float32 -> (smoothed points, final state): models.py:120-125 frame by frame in float32 numpy."""
    p = np.array(points, dtype=np.float32, copy=True)
    a, b = np.float32(0.98), np.float32(0.02)
    s = None if state is None else np.array(state, dtype=np.float32, copy=True)
    for t in range(p.shape[0]):
        if s is None:
            s = p[t].copy()
        else:
            s = a * s + b * p[t]
            p[t] = s
    return p, s


def ema_torch(verts, index, state=None):
    """verts (T, V, 3) float32 CPU tensor -> (verts with the listed rows smoothed, final state (1, K, 3)): the recurrence in torch's
    own arithmetic, one frame at a time."""
    out = verts.clone()
    idx = torch.as_tensor(index, dtype=torch.long)
    s = None if state is None else state.clone()
    for t in range(out.shape[0]):
        cur = out[t:t + 1, idx]
        if s is None:
            s = cur
        else:
            s = 0.98 * s + 0.02 * cur
            out[t:t + 1, idx] = s
    return out, s


def ema_fma_numpy(points, state=None):
    """The same recurrence with the sum contracted to one rounding (what an FMA gives): the variant the bit-equality test excludes."""
    p = np.array(points, dtype=np.float32, copy=True)
    s = None if state is None else np.array(state, dtype=np.float32, copy=True)
    for t in range(p.shape[0]):
        if s is None:
            s = p[t].copy()
        else:
            prod = (np.float32(0.02) * p[t]).astype(np.float64)      # rounded product, then a * s + prod rounded once
            s = (np.float64(np.float32(0.98)) * s.astype(np.float64) + prod).astype(np.float32)
            p[t] = s
    return p, s


def finish_torch(image, water_mark=None):
    """image (F, 3, S, S), water_mark (4, h, w) or None, float32 CPU tensors: clamp, then the blend on the bottom-right patch."""
    image = image.clone().clamp(0, 1)
    if water_mark is None:
        return image
    h, w = water_mark.shape[-2:]
    a = water_mark[3:4] * 0.8
    image[..., -h:, -w:] = image[..., -h:, -w:] * (1 - a) + water_mark[:3] * a
    return image


def finish_numpy(image, water_mark=None):
    img = np.clip(np.asarray(image, dtype=np.float32), np.float32(0), np.float32(1))
    if water_mark is None:
        return img
    wm = np.asarray(water_mark, dtype=np.float32)
    h, w = wm.shape[1:]
    a = wm[3:4] * np.float32(0.8)
    img[..., -h:, -w:] = img[..., -h:, -w:] * (np.float32(1) - a) + wm[:3] * a
    return img
