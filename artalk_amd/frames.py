"""Frames out: fp32 planar frames ``(F, 3, H, W)`` in [0, 1] on the device -> the 8-bit frames a video encoder takes, and a ``.y4m`` file
any encoder reads ("Frames out"; the kernels: ``csrc/frames.hip``).

``"rgb24"``: uint8 ``(F, H, W, 3)``, ``(x * 255.0).astype(np.uint8)`` of the clamped frame, what ``av.VideoFrame.from_ndarray(frame,
format="rgb24")`` takes.  ``"yuv420p"``: uint8 ``(F, H * 3 // 2, W)``, per frame the Y plane, then U and V at half size (I420), BT.601
limited range in integers from the quantised R, G, B.  Writing and reading Y4M is host only; there is no PyAV code here."""
from __future__ import annotations

import re

import torch

from . import capi

FORMATS = {"rgb24": capi.FRAMES_RGB24, "yuv420p": capi.FRAMES_YUV420P}


def format_code(format):
    try:
        return FORMATS[format]
    except (KeyError, TypeError):
        raise ValueError(f"unknown frame format {format!r}: one of {sorted(FORMATS)}") from None


def frame_bytes(format, H, W):
    """Bytes of one H x W frame in ``format`` (``artalk_frames_bytes``)."""
    n = int(capi.lib().artalk_frames_bytes(format_code(format), int(H), int(W)))
    if n < 0:
        raise ValueError(f"no {format} frame of {H} x {W}: H and W must be in 1..16384" + (" and even" if format == "yuv420p" else ""))
    return n


def frame_shape(format, F, H, W):
    """Shape of the uint8 tensor that holds F frames."""
    frame_bytes(format, H, W)
    return (F, H, W, 3) if format == "rgb24" else (F, H * 3 // 2, W)


@torch.no_grad()
def pack_frames(x, format):
    """x: a CUDA float32 ``(F, 3, H, W)`` tensor -> uint8 ``(F, H, W, 3)`` (``"rgb24"``) or ``(F, H * 3 // 2, W)`` (``"yuv420p"``) on the
    same device, from one kernel launch on the current stream.  A non-contiguous x is made contiguous first; a contiguous view goes in
    as it is, whatever its storage offset."""
    code = format_code(format)
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError("pack_frames takes a float32 (F, 3, H, W) tensor")
    if not x.is_cuda:
        raise RuntimeError("pack_frames runs on the GPU: x must be a CUDA tensor (there is no CPU fallback)")
    F, _, H, W = (int(v) for v in x.shape)
    x = x.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    L = capi.lib()
    with torch.cuda.device(x.device):
        out = torch.empty(frame_shape(format, F, H, W), dtype=torch.uint8, device=x.device)
        rc = L.artalk_frames_pack(capi.ptr(x), F, H, W, code, capi.ptr(out), capi.current_stream_ptr())
    if rc == capi.EINVAL:
        raise ValueError("artalk_frames_pack refused: " + L.artalk_frames_last_error().decode())
    if rc != capi.OK:
        raise RuntimeError("artalk_frames_pack failed: " + L.artalk_frames_last_error().decode())
    return out


def _host_yuv(yuv, size):
    if not isinstance(yuv, torch.Tensor):
        yuv = torch.as_tensor(yuv)
    if yuv.dtype != torch.uint8 or yuv.dim() != 3:
        raise ValueError("write_y4m takes a uint8 (F, H * 3 // 2, W) tensor of yuv420p frames")
    W = int(yuv.shape[2])
    if int(yuv.shape[1]) % 3 != 0:
        raise ValueError(f"{int(yuv.shape[1])} rows are not H * 3 // 2 of any H")
    H = int(yuv.shape[1]) // 3 * 2
    if size is not None and (int(size[0]), int(size[1])) != (H, W):
        raise ValueError(f"the frames are {H} x {W}, not size = {tuple(size)}")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"yuv420p needs an even H and W (got {H} x {W})")
    return yuv.cpu().contiguous(), H, W


def write_y4m(path, yuv, fps=25, size=None):
    """Writes yuv420p frames ``(F, H * 3 // 2, W)`` (a uint8 tensor, device or host) as a YUV4MPEG2 file: the header line, then per frame
    ``FRAME`` and the I420 bytes.  ``size=(H, W)`` is checked against the tensor when given.  ``ffmpeg -i clip.y4m`` encodes the file."""
    yuv, H, W = _host_yuv(yuv, size)
    fps = int(fps)
    if fps < 1:
        raise ValueError("fps must be a positive integer")
    data = yuv.numpy()
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F{fps}:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode("ascii"))
        for frame in data:
            f.write(b"FRAME\n")
            f.write(frame.tobytes())


def read_y4m(path):
    """-> (yuv uint8 (F, H * 3 // 2, W) on the host, fps, (H, W)) of a file ``write_y4m`` wrote (4:2:0, integer frame rate)."""
    with open(path, "rb") as f:
        header = f.readline()
        m = re.fullmatch(rb"YUV4MPEG2 W(\d+) H(\d+) F(\d+):1 (?:.* )?C420\w*(?: .*)?\n", header)
        if not m:
            raise ValueError(f"{path}: not a 4:2:0 YUV4MPEG2 file with an integer frame rate: {header[:80]!r}")
        W, H, fps = int(m.group(1)), int(m.group(2)), int(m.group(3))
        n = H * W * 3 // 2
        frames = []
        while True:
            line = f.readline()
            if not line:
                break
            if not line.startswith(b"FRAME"):
                raise ValueError(f"{path}: expected FRAME, found {line[:20]!r}")
            raw = f.read(n)
            if len(raw) != n:
                raise ValueError(f"{path}: frame {len(frames)} is cut short")
            frames.append(torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(H * 3 // 2, W))
    yuv = torch.stack(frames) if frames else torch.empty(0, H * 3 // 2, W, dtype=torch.uint8)
    return yuv, fps, (H, W)
