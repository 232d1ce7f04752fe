"""Seeded cases for the Gaussian splat rasteriser's tests (tests/splat_ref.py is the oracle).

A Gaussian's preprocess decisions are discontinuous: the radius is a ceil, the tile rectangle an int(), the near cull a comparison.
``random_case`` re-draws every Gaussian that sits within rounding of one of them - 3 sqrt(lambda) within 1e-4 of an integer, a
rectangle bound within 1e-4 px of a tile edge, t.z within 1e-6 of 0.2 - so that float32 and float64 decide alike and ``radii`` can be
compared for equality on every Gaussian.  What is left is per pixel (alpha against 1/255, the stop test, depth ties) and is handled by
the oracle's margins.  Everything is float32 (what the device is given); the camera comes from ``splat_ref.build_camera``.
"""
import functools

import numpy as np

from splat_ref import NUM_CHANNELS, ambiguous, build_camera, preprocess, splat_ref

AMBIGUOUS_CAP = 0.01      # share of the pixels the ambiguity mask may take (a condition of every case in TABLE)


def camera(focal_x=2.0, focal_y=2.0, distance=3.0, yaw_deg=0.0, pitch_deg=0.0):
    """[R | t] looking at the origin from `distance`, turned by yaw and pitch -> dict(V, P float32, tanfovx, tanfovy, cam_matrix)."""
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    M = np.concatenate([ry @ rx, np.array([[0.0], [0.0], [distance]])], axis=1)
    V, P = build_camera(M, focal_x, focal_y)
    return dict(V=V.astype(np.float32), P=P.astype(np.float32), tanfovx=1.0 / focal_x, tanfovy=1.0 / focal_y, cam_matrix=M.astype(np.float32))


def near_threshold(pre):
    """(N,) bool: Gaussians whose preprocess decision is within rounding of a threshold (see the module text)."""
    r3 = pre["r3"]
    with np.errstate(invalid="ignore"):
        near = np.abs(r3 - np.round(r3)) < 1e-4
        for v in (pre["lo"], pre["hi"]):
            px = v * 16.0
            near |= (np.abs(px - 16.0 * np.round(px / 16.0)) < 1e-4).any(axis=1)
        near |= np.abs(pre["tz"] - 0.2) < 1e-6
        near |= ~np.isfinite(r3)
    return near


def _draw(g, n, spread, scale_lo, scale_hi, depth_spread, opac_hi=1.0):
    means = np.stack([g.uniform(-spread, spread, n), g.uniform(-spread, spread, n), g.uniform(-depth_spread, depth_spread, n)], axis=1)
    scales = np.exp(g.uniform(np.log(scale_lo), np.log(scale_hi), (n, 3)))
    rots = g.standard_normal((n, 4))
    rots /= np.linalg.norm(rots, axis=1, keepdims=True) * g.uniform(0.9, 1.1, (n, 1))      # used as given: not quite unit
    opac = g.uniform(0.05 * opac_hi, opac_hi, n)
    colors = g.uniform(-1.0, 1.6, (n, NUM_CHANNELS))
    return [a.astype(np.float32) for a in (means, colors, opac, scales, rots)]


def random_case(seed, N, H, W, cam=None, spread=1.6, scale_lo=0.02, scale_hi=0.25, depth_spread=1.0, scale_modifier=1.0, bg=None,
                opac_hi=1.0):
    cam = cam or camera()
    g = np.random.default_rng(seed)
    arrs = _draw(g, N, spread, scale_lo, scale_hi, depth_spread, opac_hi)
    for _ in range(50):
        means, colors, opac, scales, rots = arrs
        pre = preprocess(means, opac, scales, rots, cam["V"], cam["P"], cam["tanfovx"], cam["tanfovy"], H, W, scale_modifier)
        bad = np.nonzero(near_threshold(pre))[0]
        if bad.size == 0:
            break
        fresh = _draw(g, bad.size, spread, scale_lo, scale_hi, depth_spread, opac_hi)
        for a, fr in zip(arrs, fresh):
            a[bad] = fr
    else:
        raise AssertionError("the re-draw did not settle")
    return dict(means=means, colors=colors, opacities=opac, scales=scales, rotations=rots, H=H, W=W, scale_modifier=scale_modifier,
                bg=None if bg is None else np.asarray(bg, dtype=np.float32), **cam)


def bg_ramp():
    return np.linspace(-0.5, 1.0, NUM_CHANNELS).astype(np.float32)



def opaque_stack():
    """Broad Gaussians one behind the other over the image centre: there alphas of about 0.9 and 0.92 leave T = 0.008, and the third, at
    the cap of 0.99, would leave 8e-5: the walk stops before it with a visible share (0.008 of its colour) at stake.  In front of them
    a small opaque Gaussian whose centre falls exactly on pixel (10, 20): opacity 1 there, so the cap binds.  Small ones around it; the
    1 / 255 skip trims every small footprint."""
    means = [[0.0, 0.0, -0.4 + 0.2 * k] for k in range(5)] + [[-0.28125, 0.34375, -1.0], [0.6, -0.5, -0.8], [-0.7, 0.4, -0.9], [0.2, 0.7, -0.7]]
    scales = [1.0] * 5 + [0.15, 0.12, 0.1, 0.15]
    op = [0.9, 0.92, 1.0, 0.99, 0.9, 1.0, 0.7, 0.6, 0.8]
    return hand_case(means, op, np.array(scales)[:, None], 32, 32, bg=np.full(NUM_CHANNELS, 0.5))


def culled_and_drawn():
    """Gaussians 0..5 are not drawn - inside the near limit (t.z = 0.1 and 0.19), behind the camera,
    and off screen to the right, the left and below - and 6..8 are."""
    means = [[0.0, 0.0, -2.9], [0.1, 0.0, -2.81], [0.0, 0.1, -5.0], [-9.0, 0.0, 0.0], [9.0, 0.2, 0.5], [0.0, 12.0, 0.0],
             [0.3, 0.2, 0.0], [-0.4, -0.3, 0.4], [0.0, 0.5, -0.6]]
    return hand_case(means, 0.8, 0.08, 40, 56, bg=bg_ramp())


def all_culled():
    c = culled_and_drawn()
    return dict(c, **{k: c[k][:6] for k in ("means", "colors", "opacities", "scales", "rotations")})


def equal_depths():
    """Gaussians 0 and 1 share centre and depth and differ in colour and shape; 2 and 3 share a depth at different places and overlap."""
    means = [[0.1, -0.1, 0.2], [0.1, -0.1, 0.2], [-0.5, 0.3, -0.3], [-0.3, 0.35, -0.3]]
    return hand_case(means, [0.8, 0.6, 0.7, 0.9], np.array([[0.3, 0.12, 0.2], [0.15, 0.3, 0.2], [0.2, 0.2, 0.2], [0.25, 0.1, 0.2]]), 40, 56)


def swapped(c, i, j):
    """The same case with Gaussians i and j in each other's places."""
    out = dict(c)
    for k in ("means", "colors", "opacities", "scales", "rotations"):
        a = c[k].copy()
        a[[i, j]] = a[[j, i]]
        out[k] = a
    return out


# name -> how to build it; every one of them is checked against AMBIGUOUS_CAP and for float32 / float64 agreement in test_splat_cpu.py
TABLE = {
    "n300_40x56": lambda: random_case(11, 300, 40, 56),
    "n1500_40x56": lambda: random_case(12, 1500, 40, 56),
    "n300_33x17": lambda: random_case(13, 300, 33, 17),
    "n1500_33x17": lambda: random_case(24, 1500, 33, 17),      # (561 pixels: seeds 14 and 54 have 6 ambiguous ones, 1.07 %, and are not used)
    "n255": lambda: random_case(15, 255, 40, 56),
    "n256": lambda: random_case(16, 256, 40, 56),
    "n257": lambda: random_case(17, 257, 40, 56),
    "bg_scale_modifier": lambda: random_case(18, 300, 40, 56, scale_modifier=1.7, bg=bg_ramp()),
    "turned_camera": lambda: random_case(19, 300, 40, 56, cam=camera(2.5, 1.5, 3.0, yaw_deg=25.0, pitch_deg=-10.0)),
    "n1": lambda: hand_case([[0.2, -0.1, 0.0]], 0.8, np.array([[0.3, 0.1, 0.2]]), 40, 56, rotations=[[0.9, 0.2, -0.3, 0.25]]),
    # 600 faint Gaussians within +-6.4 px of the centre of a 48 x 48 image: all of them in tile (1, 1), three LDS batches, nobody stops
    "one_tile_600": lambda: random_case(20, 600, 48, 48, spread=0.4, scale_lo=0.01, scale_hi=0.04, opac_hi=0.3),
    "opaque_stack": opaque_stack,
    "whole_image": lambda: hand_case([[0.1, 0.05, 0.0]], 0.7, 2.0, 40, 56, bg=bg_ramp()),
    "culled_and_drawn": culled_and_drawn,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return TABLE[name]()


def run_ref(c, dtype=np.float64, variant=None, **over):
    k = dict(c, **over)
    return splat_ref(k["means"], k["colors"], k["opacities"], k["scales"], k["rotations"], k["V"], k["P"], k["tanfovx"], k["tanfovy"],
                     k["H"], k["W"], bg=k["bg"], scale_modifier=k["scale_modifier"], dtype=dtype, variant=variant)


@functools.lru_cache(maxsize=None)
def case_refs(name):
    """(float64 oracle, float32 yardstick) of a TABLE case, computed once per session and left unchanged."""
    c = case(name)
    return run_ref(c), run_ref(c, dtype=np.float32)


def hand_case(means, opacities, scales, H, W, colors=None, rotations=None, cam=None, bg=None, scale_modifier=1.0):
    """A case written out by hand: identity rotations and channel ramps unless given."""
    cam = cam or camera()
    means = np.asarray(means, dtype=np.float32).reshape(-1, 3)
    n = means.shape[0]
    if colors is None:
        colors = 0.2 + 0.8 * np.cos(np.arange(n)[:, None] * 0.7 + np.arange(NUM_CHANNELS)[None, :] * 0.3)
    if rotations is None:
        rotations = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    return dict(means=means, colors=np.asarray(colors, dtype=np.float32).reshape(n, NUM_CHANNELS),
                opacities=np.broadcast_to(np.asarray(opacities, dtype=np.float32), (n,)).copy(),
                scales=np.broadcast_to(np.asarray(scales, dtype=np.float32), (n, 3)).copy(),
                rotations=np.asarray(rotations, dtype=np.float32), H=H, W=W, scale_modifier=scale_modifier,
                bg=None if bg is None else np.asarray(bg, dtype=np.float32), **cam)


def share_and_yardstick(r64, r32, **amb):
    """(ambiguous mask, its share, max-abs float32-numpy error over the unambiguous pixels)."""
    amb_mask = ambiguous(r64, **amb)
    ok = ~amb_mask
    yard = float(np.abs(r32["image"].astype(np.float64) - r64["image"])[:, ok].max()) if ok.any() else 0.0
    return amb_mask, float(amb_mask.mean()), yard
