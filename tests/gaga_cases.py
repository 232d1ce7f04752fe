"""Case tables of the GAGAvatar head's tests (tests/test_gaga_cpu.py, test_gaga_ops_gpu.py, test_gaga_gpu.py) and the small synthetic head
they share: S = 16, a 64-vertex FLAME asset at scale 5, N = 64 + 2 x 6^2 Gaussians, 8 forehead vertices, a 5 x 8 watermark."""
import math

import numpy as np
import torch

PI32 = float(np.float32(math.pi))
HALF_PI32 = float(np.float32(math.pi / 2))

# ---- cameras: named head-rotation codes (float32 values)
CAMERA_CASES = {
    "zero": [0.0, 0.0, 0.0],
    "tiny": [6e-8, -6e-8, 5.2e-8],                      # |w| = 1e-7: the small-angle branch
    "quarter_0": [HALF_PI32, 0.0, 0.0],
    "quarter_1": [0.0, HALF_PI32, 0.0],
    "quarter_2": [0.0, 0.0, HALF_PI32],
    "near_pi": [1.9, -2.1, 1.35],                       # |w| = 3.139
    "near_pi_axis": [0.0, PI32 - 1e-3, 0.0],
    "typical": [0.11, -0.23, 0.04],
}
TRANSFORM = [[0.98, -0.05, 0.17, 0.031], [0.06, 0.99, -0.02, -0.114], [-0.16, 0.03, 0.97, 9.61]]      # an avatar's own [R | t]


def random_codes(seed=3, n=16):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 3)) * np.array([0.4, 0.6, 0.3])).astype(np.float32)


# ---- single ops
FLAME_INPUT_CASES = [(T, stride, NB) for T in (1, 3) for stride, NB in ((106, 100), (131, 400), (112, 100), (106, 400))]
FOREHEAD_CASES = [(K, T, preset) for K in (1, 68) for T in (1, 2, 7, 8, 9, 17) for preset in (False, True)]
MEANS_CASES = [(F, V, N) for F in (1, 3) for V, N in ((64, 64), (64, 136), (5, 300))]
FINISH_S = 16
FINISH_MARKS = [(5, 8), (16, 16), None]

# ---- the small head
S, V, N_STATIC, T_CLIP, SLAB = 16, 64, 72, 5, 2
N = V + N_STATIC
FOREHEAD = [3, 17, 18, 40, 41, 42, 60, 63]
MARK = (5, 8)
TRANSLATION = (0.0, 0.0, 5000.0 / 512)


def flame_asset():
    from artalk_amd.flame import synthetic_flame_asset
    return synthetic_flame_asset(n_verts=V)


def motion_codes(T=T_CLIP, seed=11):
    """(T, 106) float32: expression and jaw at the scale of real clips, a head rotation that moves the camera visibly."""
    g = np.random.default_rng(seed)
    m = np.zeros((T, 106), dtype=np.float32)
    m[:, :100] = 0.8 * g.standard_normal((T, 100))
    m[:, 100:103] = 0.15 * g.standard_normal((T, 3))
    m[:, 103:106] = np.abs(0.1 * g.standard_normal((T, 3)))
    return torch.from_numpy(m)


def water_mark(h=MARK[0], w=MARK[1], seed=5):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.random((4, h, w), dtype=np.float32))


def avatar(seed=2, n=N):
    """An identity's Gaussians: the V dynamic ones (their xyz rows are placeholders the head ignores) and two 6 x 6 planes of static
    ones around the head, sized so that a 16 x 16 image at focal 12 from (0, 0, 5000 / 512) is well covered."""
    g = np.random.default_rng(seed)
    xyz = np.full((n, 3), 1e6, dtype=np.float32)      # a dynamic row that was read would land far outside the image
    u = np.linspace(-0.62, 0.62, 6, dtype=np.float32)
    gx, gy = np.meshgrid(u, u)
    for i, z in enumerate((0.12, -0.15)):
        lo = V + 36 * i
        xyz[lo:lo + 36] = np.stack([gx.ravel(), gy.ravel(), np.full(36, z, dtype=np.float32)], axis=1)
    xyz[V:] += 0.02 * g.standard_normal((n - V, 3)).astype(np.float32)
    colors = (0.5 * g.standard_normal((n, 32))).astype(np.float32)
    colors[:, :3] = 1.0 / (1.0 + np.exp(-2.0 * colors[:, :3]))
    q = g.standard_normal((n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    tm = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.array(TRANSLATION)[:, None]], axis=1).astype(np.float32)
    return {"xyz": torch.from_numpy(xyz), "colors": torch.from_numpy(colors),
            "opacities": torch.from_numpy(g.uniform(0.35, 0.95, (n, 1)).astype(np.float32)),
            "scales": torch.from_numpy(g.uniform(0.07, 0.16, (n, 3)).astype(np.float32)),
            "rotations": torch.from_numpy(q),
            "shapecode": torch.from_numpy((0.5 * g.standard_normal(300)).astype(np.float32)),
            "transform_matrix": torch.from_numpy(tm)}
