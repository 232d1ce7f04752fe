"""The definition of the 8-bit frames ("Frames out") restated in numpy: float32 for the one multiplication, integers
for everything after it.  ``rgb24`` and ``yuv420p`` give the bytes the kernels of ``csrc/frames.hip`` must give; the ``reading`` argument
selects one of the wrong readings tests/test_frames_cpu.py tells apart from the right one."""
import numpy as np

READINGS = ("round", "noclamp", "fullrange", "topleft", "mean_floor", "bgr", "uv_swapped", "nv12")


def quantise(x, reading=None):
    """float32 array -> uint8: (uint8)(clamp(x, 0, 1) * 255.0f), truncation, NaN -> 0.  (-> int64 internally; uint8 at the end.)"""
    x = np.asarray(x, dtype=np.float32)
    if reading == "noclamp":      # the reference itself: out-of-range values wrap (what is not finite is taken as 0 here)
        p = (x * np.float32(255.0)).astype(np.float32)
        p = np.where(np.isfinite(p), p, np.float32(0.0))
        return np.mod(np.trunc(p.astype(np.float64)), 256.0).astype(np.int64).astype(np.uint8)      # (exact: integers in float64)
    c = np.where(np.isnan(x), np.float32(0.0), np.minimum(np.maximum(x, np.float32(0.0)), np.float32(1.0))).astype(np.float32)
    p = (c * np.float32(255.0)).astype(np.float32)      # rounded once to float32
    if reading == "round":
        return np.floor(p.astype(np.float64) + 0.5).astype(np.int64).astype(np.uint8)
    return np.trunc(p).astype(np.int64).astype(np.uint8)


def rgb24(x, reading=None):
    """x (F, 3, H, W) float32 -> (F, H, W, 3) uint8"""
    q = quantise(x, reading)
    if reading == "bgr":
        q = q[:, ::-1]
    return np.ascontiguousarray(q.transpose(0, 2, 3, 1))


def yuv_from_rgb8(R, G, B, reading=None):
    """int64 arrays of 0..255 -> (Y, U, V) int64, BT.601 limited range, >> arithmetic (numpy's >> on int64 is)"""
    if reading == "fullrange":
        Y = (77 * R + 150 * G + 29 * B + 128) >> 8
        U = ((-43 * R - 85 * G + 128 * B + 128) >> 8) + 128
        V = ((128 * R - 107 * G - 21 * B + 128) >> 8) + 128
        return Y, np.clip(U, 0, 255), np.clip(V, 0, 255)
    Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    U = ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128
    V = ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128
    return Y, U, V


def yuv420p(x, reading=None):
    """x (F, 3, H, W) float32, H and W even -> (F, H * 3 // 2, W) uint8: per frame Y [H][W], U [H/2][W/2], V [H/2][W/2], contiguous"""
    q = quantise(x, reading).astype(np.int64)
    if reading == "bgr":
        q = q[:, ::-1]
    F, _, H, W = q.shape
    assert H % 2 == 0 and W % 2 == 0
    Y = yuv_from_rgb8(q[:, 0], q[:, 1], q[:, 2], reading)[0]
    blocks = q.reshape(F, 3, H // 2, 2, W // 2, 2)
    if reading == "topleft":
        m = blocks[:, :, :, 0, :, 0]
    else:
        m = (blocks.sum(axis=(3, 5)) + (0 if reading == "mean_floor" else 2)) >> 2
    _, U, V = yuv_from_rgb8(m[:, 0], m[:, 1], m[:, 2], reading)
    if reading == "uv_swapped":
        U, V = V, U
    for plane in (Y, U, V):
        assert plane.min(initial=0) >= 0 and plane.max(initial=0) <= 255
    if reading == "nv12":
        chroma = np.stack([U, V], axis=-1).reshape(F, -1)
    else:
        chroma = np.concatenate([U.reshape(F, -1), V.reshape(F, -1)], axis=1)
    out = np.concatenate([Y.reshape(F, -1), chroma], axis=1).astype(np.uint8)
    return np.ascontiguousarray(out.reshape(F, H * 3 // 2, W))


def pack(x, format, reading=None):
    return {"rgb24": rgb24, "yuv420p": yuv420p}[format](x, reading)
