"""The case table of the 8-bit frame tests (tests/test_frames_cpu.py, test_frames_ops_gpu.py): shapes at which the kernels of
``csrc/frames.hip`` change path - frame sizes that are no multiple of four bytes (3 x 5 rgb24 is 45 bytes, 2 x 2 yuv420p is 6), so later
frames start misaligned; W % 4 == 2; more than one workgroup - each filled in four ways."""
import numpy as np

HAND_COLOURS = {      # name: ((r, g, b) in [0, 1], (Y, U, V)), the values DESIGN.md works out by hand
    "black": ((0.0, 0.0, 0.0), (16, 128, 128)),
    "white": ((1.0, 1.0, 1.0), (235, 128, 128)),
    "red": ((1.0, 0.0, 0.0), (82, 90, 240)),
    "green": ((0.0, 1.0, 0.0), (144, 54, 34)),
    "blue": ((0.0, 0.0, 1.0), (41, 240, 110)),
}

RGB24_SHAPES = [(1, 1, 1), (3, 3, 5), (2, 7, 13), (2, 2, 6), (1, 4, 10), (1, 16, 16), (2, 34, 66)]
YUV420P_SHAPES = [(3, 2, 2), (3, 2, 6), (2, 6, 2), (1, 4, 10), (1, 16, 16), (2, 34, 66)]
FILLS = ("table", "random", "colours", "blocks")
CASES = [(fmt, shape, fill) for fmt, shapes in (("rgb24", RGB24_SHAPES), ("yuv420p", YUV420P_SHAPES)) for shape in shapes for fill in FILLS]
OFFSET_CASES = [("rgb24", (2, 7, 13), "random"), ("yuv420p", (2, 34, 66), "random")]      # the source starts one float past a 16-byte boundary


def case_id(case):
    fmt, (F, H, W), fill = case
    return f"{fmt}-{F}x{H}x{W}-{fill}"


def levels():
    """float32(k / 255) for k = 0 .. 255: the values an 8-bit image becomes when the reference divides it by 255"""
    return (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)


def value_table():
    """Every level, its float32 neighbours below and above, 0 and 1 themselves, values outside [0, 1], both infinities and NaN."""
    lv = levels()
    below, above = np.nextafter(lv, np.float32(-np.inf)), np.nextafter(lv, np.float32(np.inf))
    extra = np.array([0.0, 1.0, -0.0, -1e-7, -0.25, -3.0, 1.0 + 2.0 ** -23, 1.5, 2.0, 300.0, -1e30, 1e30, np.inf, -np.inf, np.nan],
                     dtype=np.float32)
    return np.concatenate([np.stack([below, lv, above], axis=1).reshape(-1), extra]).astype(np.float32)


def make(shape, fill, seed=0):
    """-> float32 (F, 3, H, W)"""
    F, H, W = shape
    n = F * 3 * H * W
    g = np.random.default_rng(1000 * seed + 31 * F + 7 * H + W)
    if fill == "table":
        t = value_table()
        # consecutive elements walk the table; a small shape starts where the table turns from levels to the values out of range
        start = (len(t) - min(n, len(t))) if n < len(t) else 0
        return t[(start + np.arange(n)) % len(t)].reshape(F, 3, H, W).copy()
    if fill == "random":
        return g.random((F, 3, H, W), dtype=np.float32)
    if fill == "colours":      # pixel p of frame f shows hand colour (p + f) % 5
        rgb = np.array([c[0] for c in HAND_COLOURS.values()], dtype=np.float32)
        which = (np.arange(H * W)[None, :] + np.arange(F)[:, None]) % len(rgb)
        return np.ascontiguousarray(rgb[which].reshape(F, H, W, 3).transpose(0, 3, 1, 2))
    if fill == "blocks":       # exact levels, independent per pixel: the four pixels of a 2 x 2 block differ and their sums take every residue mod 4
        return levels()[g.integers(0, 256, size=(F, 3, H, W))]
    raise KeyError(fill)


def solid(rgb, H=2, W=2):
    """one frame of one colour"""
    return np.ascontiguousarray(np.broadcast_to(np.array(rgb, dtype=np.float32)[None, :, None, None], (1, 3, H, W)))
