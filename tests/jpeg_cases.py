"""The JPEG case table, shared by tests/test_jpeg_cpu.py (the restatement against Pillow) and tests/test_jpeg_ops_gpu.py (the kernels against
the restatement).  Small shapes that reach every branch of the definition in DESIGN.md section 5, "JPEG out".  A case is
``(name, subsampling, quality)``; ``frames(name)`` gives its rgb24 frames ``(F, H, W, 3)`` uint8 (read only)."""
import functools

import numpy as np

BOTH = ("420", "444")
Q3 = (50, 90, 100)


def _smooth(H, W, seed=0):
    """A smooth colourful picture with a hard edge in it: what a rendered frame looks like to a codec."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = 128 + 100 * np.sin(0.21 * x + 0.1 * seed) * np.cos(0.13 * y)
    g = 128 + 90 * np.cos(0.17 * y + 0.05 * x + seed)
    b = np.where((x + 2 * y + 3 * seed) % 19 < 9, 40.0, 215.0)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def _blocks(H, W):
    y, x = np.mgrid[0:H, 0:W]
    v = (((y // 8) + (x // 8)) % 2 * 255).astype(np.uint8)
    return np.stack([v, v, v], -1)


def _checker(H, W):
    y, x = np.mgrid[0:H, 0:W]
    v = (((y + x) % 2) * 255).astype(np.uint8)
    return np.stack([v, v, v], -1)


def _cosine(H, W):
    y, x = np.mgrid[0:H, 0:W]
    v = 128 + 40 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    v = np.round(v).astype(np.uint8)
    return np.stack([v, v, v], -1)


def _flat(H, W):
    return np.broadcast_to(np.array([200, 120, 30], np.uint8), (H, W, 3)).copy()


def _noise(H, W, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


PICTURES = {
    "1x1": lambda: _smooth(1, 1, 3)[None],
    "8x8": lambda: _smooth(8, 8, 1)[None],
    "16x16": lambda: _smooth(16, 16, 2)[None],
    "17x23": lambda: _smooth(17, 23, 4)[None],
    "24x40": lambda: _smooth(24, 40, 5)[None],
    "blocks16x64": lambda: _blocks(16, 64)[None],
    "checker16x32": lambda: _checker(16, 32)[None],
    "cosine16x24": lambda: _cosine(16, 24)[None],
    "flat24x24": lambda: _flat(24, 24)[None],
    "noise32x48": lambda: _noise(32, 48)[None],
    "rows136x16": lambda: _smooth(136, 16, 6)[None],
    "rows272x16": lambda: _smooth(272, 16, 7)[None],
    "three48x64": lambda: np.stack([_smooth(48, 64, 8), _noise(48, 64, 9), _flat(48, 64)]),
}


@functools.lru_cache(maxsize=None)
def frames(name):
    x = np.ascontiguousarray(PICTURES[name]())
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3
    x.setflags(write=False)
    return x


CASES = (
    [(n, s, q) for n in ("1x1", "8x8", "16x16", "17x23", "24x40", "flat24x24") for s in BOTH for q in Q3]
    + [("blocks16x64", s, 100) for s in BOTH]
    + [("checker16x32", "444", 100)]
    + [("cosine16x24", "444", q) for q in (90, 100)]
    + [("noise32x48", s, 100) for s in BOTH]
    + [("rows136x16", "444", 90), ("rows272x16", "420", 90)]
    + [("three48x64", s, 90) for s in BOTH]
)
NOISE = ("noise32x48", "three48x64")      # pictures with a noise frame: the default cap is not promised to hold them


def case_id(case):
    return f"{case[0]}-{case[1]}-q{case[2]}"
