"""Frames out: fp32 planar frames ``(F, 3, H, W)`` in [0, 1] on the device -> the 8-bit frames a video encoder takes, and a ``.y4m`` file
any encoder reads ("Frames out"; the kernels: ``csrc/frames.hip``).

``"rgb24"``: uint8 ``(F, H, W, 3)``, ``(x * 255.0).astype(np.uint8)`` of the clamped frame, what ``av.VideoFrame.from_ndarray(frame,
format="rgb24")`` takes.  ``"yuv420p"``: uint8 ``(F, H * 3 // 2, W)``, per frame the Y plane, then U and V at half size (I420), BT.601
limited range in integers from the quantised R, G, B.  Writing and reading Y4M is host only; there is no PyAV code here.

JPEG out ("JPEG out"; the kernels: ``csrc/jpeg.hip``): ``encode_jpeg`` turns rgb24 frames into one baseline JPEG
stream per frame on the device, ``(data (F, cap), sizes (F,))``; ``split_jpeg`` / ``write_mjpeg`` / ``read_mjpeg`` are the host side of a
Motion-JPEG sender.  "jpeg" is not a frame format of ``format_code``: a stream has no fixed size."""
from __future__ import annotations

import ctypes as C
import re

import torch

from . import capi

FORMATS = {"rgb24": capi.FRAMES_RGB24, "yuv420p": capi.FRAMES_YUV420P}
SUBSAMPLINGS = {"420": capi.JPEG_420, "444": capi.JPEG_444}
JPEG_HEADER_BYTES = capi.JPEG_HEADER_BYTES


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


# ---- JPEG out ----
def subsampling_code(subsampling):
    try:
        return SUBSAMPLINGS[subsampling]
    except (KeyError, TypeError):
        raise ValueError(f"unknown subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}") from None


def _jpeg_size(n, H, W):
    if n < 0:
        raise ValueError(f"no JPEG of {H} x {W}: H and W must be in 1..16384")
    return n


def jpeg_default_cap(H, W):
    """The slot ``encode_jpeg`` gives a frame when the caller names none: H W 3 + 1024 bytes (``artalk_jpeg_default_cap``)."""
    return _jpeg_size(int(capi.lib().artalk_jpeg_default_cap(int(H), int(W))), H, W)


def jpeg_bound(H, W, subsampling="420"):
    """A slot no H x W picture overflows (``artalk_jpeg_bound``)."""
    return _jpeg_size(int(capi.lib().artalk_jpeg_bound(int(H), int(W), subsampling_code(subsampling))), H, W)


def jpeg_header(H, W, quality=90, subsampling="420"):
    """The 629 bytes every stream of this size, quality and subsampling starts with (``artalk_jpeg_header``, host only)."""
    buf = (C.c_uint8 * JPEG_HEADER_BYTES)()
    n = capi.lib().artalk_jpeg_header(int(H), int(W), int(quality), subsampling_code(subsampling), buf, JPEG_HEADER_BYTES)
    if n != JPEG_HEADER_BYTES:
        raise ValueError("artalk_jpeg_header refused: " + capi.lib().artalk_jpeg_last_error(None).decode())
    return bytes(buf)


def jpeg_options(jpeg):
    """The ``jpeg=dict(quality=, subsampling=, cap=)`` option of the render calls -> (quality, subsampling, cap), checked."""
    opts = dict(jpeg or {})
    unknown = sorted(set(opts) - {"quality", "subsampling", "cap"})
    if unknown:
        raise ValueError(f"jpeg= takes quality, subsampling and cap, not {unknown}")
    quality, subsampling, cap = int(opts.get("quality", 90)), opts.get("subsampling", "420"), opts.get("cap")
    subsampling_code(subsampling)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality must be in 1..100 (got {quality})")
    if cap is not None and int(cap) < JPEG_HEADER_BYTES + 2:
        raise ValueError(f"cap must be at least the header and EOI, {JPEG_HEADER_BYTES + 2} bytes (got {cap})")
    return quality, subsampling, None if cap is None else int(cap)


class JpegEncoder:
    """A baseline JPEG encoder on one device (``artalk_jpeg_*``): it owns the scratch its two kernels write and the uploaded header of
    every size it has seen.  ``encode`` enqueues on the current stream and never waits for the device, except to grow scratch."""

    def __init__(self, quality=90, subsampling="420", device="cuda"):
        self.quality, self.subsampling, _ = jpeg_options(dict(quality=quality, subsampling=subsampling))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("JpegEncoder runs on the GPU: device must be a CUDA device (there is no CPU fallback)")
        self._h = None

    def _handle(self):
        if self._h is None:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", idx)
            h = C.c_void_p()
            if capi.lib().artalk_jpeg_create(int(idx), C.byref(h)) != capi.OK:
                raise RuntimeError("artalk_jpeg_create failed: " + capi.lib().artalk_jpeg_last_error(None).decode())
            self._h = h
        return self._h

    def set_timing(self, enable=True):
        """Time the two launches of every call (``artalk_jpeg_set_timing``); a timed ``encode`` waits for its last launch."""
        capi.lib().artalk_jpeg_set_timing(self._handle(), int(bool(enable)))
        return self

    def launch_ms(self):
        """(rows kernel ms, pack kernel ms) of the last timed ``encode`` (``artalk_jpeg_get_timing``)."""
        ms = (C.c_double * 2)()
        capi.lib().artalk_jpeg_get_timing(self._handle(), ms, 2)
        return tuple(ms)

    def close(self):
        if self._h is not None:
            capi.lib().artalk_jpeg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @torch.no_grad()
    def encode(self, x, cap=None, host=False, out=None):
        """x: uint8 ``(F, H, W, 3)`` rgb24 frames on the encoder's device, or float32 ``(F, 3, H, W)`` frames, which go through
        ``pack_frames(x, "rgb24")`` first -> ``(data uint8 (F, cap), sizes int64 (F,))``: frame f's stream is ``data[f, :sizes[f]]``; a
        frame that does not fit ``cap`` (default ``jpeg_default_cap``) has ``sizes[f] = -(the bytes it needs)``.  ``out=(data, sizes)``:
        contiguous device tensors of these shapes to fill instead of new ones.  ``host=True`` returns pinned CPU tensors, filled on the
        current stream: synchronise it before reading them."""
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3:
            x = pack_frames(x, "rgb24")
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError("encode_jpeg takes a uint8 (F, H, W, 3) tensor of rgb24 frames or a float32 (F, 3, H, W) one")
        if not x.is_cuda:
            raise RuntimeError("encode_jpeg runs on the GPU: x must be a CUDA tensor (there is no CPU fallback)")
        F, H, W, _ = (int(v) for v in x.shape)
        cap = jpeg_default_cap(H, W) if cap is None else int(cap)
        if cap < JPEG_HEADER_BYTES + 2:
            raise ValueError(f"cap must be at least the header and EOI, {JPEG_HEADER_BYTES + 2} bytes (got {cap})")
        x = x.detach()
        if not x.is_contiguous():
            x = x.contiguous()
        h = self._handle()
        if x.device != self.device:
            raise RuntimeError(f"x lives on {x.device}, the encoder on {self.device}")
        L = capi.lib()
        with torch.cuda.device(x.device):
            if out is None:
                data = torch.empty((F, cap), dtype=torch.uint8, device=x.device)
                sizes = torch.empty((F,), dtype=torch.int64, device=x.device)
            else:
                data, sizes = out
                if (data.dtype != torch.uint8 or tuple(data.shape) != (F, cap) or sizes.dtype != torch.int64 or tuple(sizes.shape) != (F,)
                        or not data.is_contiguous() or not sizes.is_contiguous() or data.device != x.device or sizes.device != x.device):
                    raise ValueError(f"out must be contiguous (uint8 ({F}, {cap}), int64 ({F},)) tensors on {x.device}")
            rc = L.artalk_jpeg_encode(h, capi.ptr(x), F, H, W, self.quality, subsampling_code(self.subsampling), capi.ptr(data), cap,
                                      capi.ptr(sizes), capi.current_stream_ptr())
            if rc == capi.EINVAL:
                raise ValueError("artalk_jpeg_encode refused: " + L.artalk_jpeg_last_error(h).decode())
            if rc != capi.OK:
                raise RuntimeError("artalk_jpeg_encode failed: " + L.artalk_jpeg_last_error(h).decode())
            if host:
                data_host = torch.empty((F, cap), dtype=torch.uint8, pin_memory=True)
                sizes_host = torch.empty((F,), dtype=torch.int64, pin_memory=True)
                data_host.copy_(data, non_blocking=True)
                sizes_host.copy_(sizes, non_blocking=True)
                return data_host, sizes_host
        return data, sizes


_encoders = {}


def jpeg_encoder(device, quality=90, subsampling="420"):
    """The shared encoder of a device, quality and subsampling: made on first use, kept for the life of the process."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (int(idx), int(quality), subsampling)
    if key not in _encoders:
        _encoders[key] = JpegEncoder(quality, subsampling, torch.device("cuda", idx))
    return _encoders[key]


def encode_jpeg(x, quality=90, subsampling="420", cap=None, host=False):
    """``JpegEncoder.encode`` with the shared encoder of x's device: uint8 ``(F, H, W, 3)`` or float32 ``(F, 3, H, W)`` on the GPU ->
    ``(data uint8 (F, cap), sizes int64 (F,))``."""
    quality, subsampling, cap = jpeg_options(dict(quality=quality, subsampling=subsampling, cap=cap))
    if not isinstance(x, torch.Tensor):
        raise ValueError("encode_jpeg takes a uint8 (F, H, W, 3) tensor of rgb24 frames or a float32 (F, 3, H, W) one")
    if not x.is_cuda:
        raise RuntimeError("encode_jpeg runs on the GPU: x must be a CUDA tensor (there is no CPU fallback)")
    return jpeg_encoder(x.device, quality, subsampling).encode(x, cap=cap, host=host)


def _host_bytes(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().contiguous().numpy()
    import numpy as np
    return np.ascontiguousarray(t)


def split_jpeg(data, sizes):
    """``(data (F, cap), sizes (F,))`` of ``encode_jpeg`` (tensors or arrays, device or host) -> the F streams as ``bytes``.  A negative
    size - a frame that did not fit its slot - raises ``ValueError`` naming the frame and the bytes it needs."""
    data, sizes = _host_bytes(data), _host_bytes(sizes)
    if data.ndim != 2 or sizes.ndim != 1 or data.shape[0] != sizes.shape[0]:
        raise ValueError("split_jpeg takes data (F, cap) and sizes (F,)")
    cap = int(data.shape[1])
    out = []
    for f, n in enumerate(int(v) for v in sizes):
        if n < 0:
            raise ValueError(f"frame {f} did not fit its slot of {cap} bytes: it needs {-n} (jpeg_bound gives a cap that always fits)")
        if n > cap:
            raise ValueError(f"frame {f}: size {n} exceeds the slot of {cap} bytes")
        out.append(data[f, :n].tobytes())
    return out


def write_mjpeg(path, data, sizes):
    """Writes the frames back to back: a raw Motion-JPEG file (``ffmpeg -f mjpeg -framerate 25 -i clip.mjpeg``).  Returns the number of
    frames written."""
    frames = split_jpeg(data, sizes)
    with open(path, "wb") as f:
        for b in frames:
            f.write(b)
    return len(frames)


def _next_jpeg(buf, at, path):
    """The end of the JPEG that starts at buf[at]: walks the marker segments up to SOS, then the scan up to EOI."""
    if buf[at:at + 2] != b"\xff\xd8":
        raise ValueError(f"{path}: expected SOI at byte {at}, found {bytes(buf[at:at + 2])!r}")
    i = at + 2
    while True:      # the segments before the scan carry their length
        if i + 4 > len(buf) or buf[i] != 0xFF:
            raise ValueError(f"{path}: the frame at byte {at} is cut short or damaged at byte {i}")
        marker, i = buf[i + 1], i + 2 + int.from_bytes(buf[i + 2:i + 4], "big")
        if marker == 0xDA:
            break
    while True:      # in the scan 0xFF is followed by 0x00 (stuffing) or 0xD0..0xD7 (restart), until EOI
        i = buf.find(b"\xff", i)
        if i < 0 or i + 1 >= len(buf):
            raise ValueError(f"{path}: the frame at byte {at} has no EOI")
        if buf[i + 1] == 0xD9:
            return i + 2
        i += 2 if buf[i + 1] == 0x00 or 0xD0 <= buf[i + 1] <= 0xD7 else 1


def read_mjpeg(path):
    """-> the frames of a file ``write_mjpeg`` wrote, as ``bytes``: split at SOI / EOI (byte stuffing keeps both out of a scan)."""
    with open(path, "rb") as f:
        buf = f.read()
    frames, at = [], 0
    while at < len(buf):
        end = _next_jpeg(buf, at, path)
        frames.append(buf[at:end])
        at = end
    return frames
