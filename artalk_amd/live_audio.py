"""Live audio in: raw PCM packets of any size -> the model's 16 kHz mono blocks, per stream, on the device ("Live
audio in"; the kernels and the object: ``csrc/pcm.hip``).

A live sender hands over interleaved 16-bit (or float) PCM at 48 or 44.1 kHz in packets of 10 - 20 ms.  ``LiveAudio`` resamples them as
they come - a streaming form of ``audio.resample_mean_16k`` whose 16 kHz samples are bit for bit those of the whole-clip call on the
concatenated signal, whatever the packet sizes - and collects them per stream in a ring from which ``take`` cuts the 64 000-sample
blocks ``stream_step`` takes.  One kernel launch per ``push`` for all listed streams, whatever their rates; no call waits for the device;
every count (frames in, samples written and taken) is host arithmetic.

    live = LiveAudio()
    a = live.open(48000, channels=2, dtype="s16")
    live.push([a], [packet_bytes])                    # as often as packets come
    if live.ready(a): chunks, n_valid = live.take([a])  # (1, 64000) on the device, [64000]
    live.end([a])                                     # the sender hung up: the tail becomes available, then live.drained(a)

The arithmetic (``plan``, ``final_groups``, ``emitted``, ``total_outputs``) is stated here in plain Python as well: the tests hold the
library's to it.  The library is the product path: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import audio, capi

DTYPES = {"s16": (capi.PCM_S16, 2, np.dtype("<i2"), torch.int16), "f32": (capi.PCM_F32, 4, np.dtype("<f4"), torch.float32)}
TARGET_RATE = 16000


# ------------------------------------------------------------------------------------------------ arithmetic (host only)
def final_groups(n_in, orig, width):
    """Groups of ``new`` outputs that are final after ``n_in`` frames: group j reads frames up to j orig + width + orig - 1."""
    return 0 if n_in < width else (n_in - width) // orig


def emitted(n_in, orig, new, width):
    """16 kHz samples a stream holds after ``n_in`` frames, before its end."""
    return new * final_groups(n_in, orig, width)


def total_outputs(n, orig, new):
    """ceil(new n / orig): the samples of a whole signal of n frames (``resample_mean_16k``'s length)."""
    return -((-n * new) // orig)


def plan(n_before, frames, end, orig, new, width):
    """What a push of ``frames`` frames (``end``: the end of the signal) does to a stream that has taken ``n_before`` frames, as
    ``artalk_op_pcm_plan`` states it: a dict of n_out, lead, carry_n, carry_from, carry_out_n, groups.  The launch's span is the carry
    (``carry_n`` frames: every frame from j_next orig - width on) followed by the packet; span frame v stands for signal frame
    v + j_next orig - width, and the first ``lead`` span frames lie before the signal's first."""
    j0 = final_groups(n_before, orig, width)
    a0 = j0 * orig - width
    lead, carry_n = max(0, -a0), n_before - max(a0, 0)
    if end:
        n_out = total_outputs(n_before, orig, new) - j0 * new
        return dict(n_out=n_out, lead=lead, carry_n=carry_n, carry_from=lead, carry_out_n=0, groups=-(-n_out // new))
    n_after = n_before + frames
    j1 = final_groups(n_after, orig, width)
    keep = max(j1 * orig - width, 0)
    return dict(n_out=(j1 - j0) * new, lead=lead, carry_n=carry_n, carry_from=keep - a0, carry_out_n=n_after - keep, groups=j1 - j0)


def rate_geometry(sample_rate):
    """(orig, new, width) of a sample rate, refused with ``ValueError`` when the streaming kernel does not take it.  16 kHz is the
    channel mean alone: one tap of 1.0."""
    sample_rate = int(sample_rate)
    if sample_rate < 1:
        raise ValueError(f"sample_rate must be positive (got {sample_rate})")
    if sample_rate == TARGET_RATE:
        return 1, 1, 0
    orig, new, ntaps = audio.tap_table_geometry(sample_rate, TARGET_RATE)
    if ntaps > capi.PCM_MAX_TAPS or new * ntaps > audio.MAX_TAP_TABLE:
        raise ValueError(f"resampling {sample_rate} Hz to {TARGET_RATE} Hz reduces to {orig}:{new} with {ntaps} taps a phase (limit "
                         f"{capi.PCM_MAX_TAPS}) and a table of {new * ntaps} elements (limit {audio.MAX_TAP_TABLE}); resample to a rate with a "
                         "larger common divisor first")
    return orig, new, (ntaps - orig) // 2


def rate_taps(sample_rate):
    """(taps float32 (new, 2 width + orig) on the host, orig, new, width): built exactly as the whole-clip path builds them."""
    orig, new, width = rate_geometry(sample_rate)
    if int(sample_rate) == TARGET_RATE:
        return torch.ones(1, 1, dtype=torch.float32), 1, 1, 0
    taps, w, o, n = audio.sinc_resample_kernel(int(sample_rate), TARGET_RATE)
    assert (o, n, w) == (orig, new, width)
    return taps, orig, new, width


def check_format(channels, dtype):
    if dtype not in DTYPES:
        raise ValueError(f"unknown sample format {dtype!r}: one of {sorted(DTYPES)}")
    if not 1 <= int(channels) <= capi.PCM_MAX_CHANNELS:
        raise ValueError(f"channels must be in 1..{capi.PCM_MAX_CHANNELS} (got {channels})")


class AudioStream:
    """One stream of ``LiveAudio.open``: ``id`` (the library's, never reused), ``sample_rate``, ``channels``, ``dtype``, ``closed``."""

    def __init__(self, owner, sid, sample_rate, channels, dtype):
        self._owner = owner
        self.id, self.sample_rate, self.channels, self.dtype = int(sid), int(sample_rate), int(channels), dtype
        self.closed = False

    def close(self):
        if not self.closed:
            self._owner.close(self)

    def __repr__(self):
        return f"AudioStream(id={self.id}, {self.sample_rate} Hz, {self.channels} ch, {self.dtype}, closed={self.closed})"


class LiveAudio:
    def __init__(self, device="cuda", block=64000, ring_blocks=3, max_streams=64):
        """``block``: samples of one ``take`` row (the model's 4 s); ``ring_blocks`` (>= 2): blocks a stream's ring holds - a push whose
        samples would not fit what ``take`` has left free is refused; ``max_streams``: streams open at a time."""
        block, ring_blocks, max_streams = int(block), int(ring_blocks), int(max_streams)
        if block < 1 or ring_blocks < 2 or not 1 <= max_streams <= 4096 or block * ring_blocks >= 1 << 30:
            raise ValueError("LiveAudio needs block >= 1, ring_blocks >= 2, max_streams in 1..4096 and a ring below 2^30 samples")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("LiveAudio runs on the GPU: device must be a CUDA device (there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.block, self.ring_blocks = block, ring_blocks
        self._h = C.c_void_p()
        self._rates = set()
        rc = capi.lib().artalk_pcm_create(self.device.index, block, ring_blocks, max_streams, C.byref(self._h))
        if rc != capi.OK:
            self._h = C.c_void_p()
            raise RuntimeError("artalk_pcm_create failed: " + capi.lib().artalk_pcm_last_error(None).decode())

    def __del__(self):
        try:
            h, self._h = getattr(self, "_h", None), None
            if h:
                capi.lib().artalk_pcm_destroy(h)
        except Exception:
            pass

    def _raise(self, what, rc):
        msg = f"{what}: " + capi.lib().artalk_pcm_last_error(self._h).decode()
        raise (ValueError if rc == capi.EINVAL else RuntimeError)(msg)

    def _ids(self, streams):
        streams = list(streams)
        for st in streams:
            if not isinstance(st, AudioStream) or st._owner is not self:
                raise ValueError(f"{st!r} is not a stream of this LiveAudio")
        return streams, (C.c_int64 * len(streams))(*[st.id for st in streams])

    # ------------------------------------------------------------------------------------------------ streams
    def open(self, sample_rate, channels=1, dtype="s16"):
        """A new stream of interleaved ``dtype`` samples (``"s16"``: little-endian int16, value / 32768; ``"f32"``) with ``channels``
        channels at ``sample_rate``.  A rate's tap table is built and uploaded the first time the rate is opened."""
        check_format(channels, dtype)
        sample_rate = int(sample_rate)
        L = capi.lib()
        if sample_rate not in self._rates:
            taps, orig, new, width = rate_taps(sample_rate)      # (ValueError before the device is touched)
            rc = L.artalk_pcm_set_rate(self._h, sample_rate, capi.ptr(taps), orig, new, width)
            if rc != capi.OK:
                self._raise("artalk_pcm_set_rate", rc)
            self._rates.add(sample_rate)
        sid = C.c_int64(0)
        rc = L.artalk_pcm_open(self._h, sample_rate, int(channels), DTYPES[dtype][0], C.byref(sid))
        if rc != capi.OK:
            self._raise("artalk_pcm_open", rc)
        return AudioStream(self, sid.value, sample_rate, channels, dtype)

    def close(self, st):
        if st.closed:
            return
        rc = capi.lib().artalk_pcm_close(self._h, st.id)
        st.closed = True
        if rc != capi.OK:
            self._raise("artalk_pcm_close", rc)

    # ------------------------------------------------------------------------------------------------ packets in
    @staticmethod
    def _packet(st, pkt):
        """-> (object to keep alive, address, frames, on the device)"""
        code, nbytes, np_dtype, t_dtype = DTYPES[st.dtype]
        frame_bytes = nbytes * st.channels
        if isinstance(pkt, (bytes, bytearray, memoryview)):
            pkt = bytes(pkt)
            if len(pkt) % frame_bytes:
                raise ValueError(f"a packet of {len(pkt)} bytes is no whole number of {st.channels}-channel {st.dtype} frames")
            return pkt, C.cast(C.c_char_p(pkt), C.c_void_p).value, len(pkt) // frame_bytes, False
        if isinstance(pkt, np.ndarray):
            if pkt.dtype != np_dtype:
                raise ValueError(f"a {st.dtype} stream takes {np_dtype} arrays (got {pkt.dtype})")
            pkt = torch.from_numpy(np.ascontiguousarray(pkt))
        if not isinstance(pkt, torch.Tensor):
            raise ValueError(f"a packet is bytes, a numpy array or a tensor (got {type(pkt).__name__})")
        if pkt.dtype != t_dtype:
            raise ValueError(f"a {st.dtype} stream takes {t_dtype} tensors (got {pkt.dtype})")
        if pkt.dim() == 1 and st.channels == 1:
            pkt = pkt[:, None]
        if pkt.dim() != 2 or pkt.shape[1] != st.channels:
            raise ValueError(f"a packet has the shape (frames, {st.channels}) (got {tuple(pkt.shape)})")
        pkt = pkt.detach().contiguous()
        return pkt, pkt.data_ptr() if pkt.shape[0] else 0, int(pkt.shape[0]), pkt.is_cuda

    def push(self, streams, packets):
        """One packet per listed stream: ``bytes``, a numpy array or a CPU or CUDA tensor of shape ``(frames, channels)`` in the stream's
        format (mono: ``(frames,)`` as well), of any length, 0 included.  One kernel launch on the current stream for all of them.
        Host packets are copied before the call returns; CUDA tensors are read in place by the launch.  One call takes host packets or
        device packets, not both.  ``ValueError`` / ``RuntimeError`` with nothing changed: a stream that is closed, listed twice or has
        ended, a push whose samples would not fit the ring's free space."""
        streams, ids = self._ids(streams)
        packets = list(packets)
        if len(packets) != len(streams) or not streams:
            raise ValueError(f"push takes one packet per stream (got {len(packets)} for {len(streams)}), at least one")
        got = [self._packet(st, pkt) for st, pkt in zip(streams, packets)]
        on_device = {g[3] for g in got if g[2] > 0}
        if len(on_device) > 1:
            raise ValueError("one push takes host packets or device packets, not both")
        dev = bool(on_device and on_device.pop())
        n = len(streams)
        data = (C.c_void_p * n)(*[g[1] if g[2] else None for g in got])
        frames = (C.c_int64 * n)(*[g[2] for g in got])
        with torch.cuda.device(self.device):
            for g in got:
                if dev and g[2] and g[0].device != self.device:
                    raise ValueError(f"a device packet lives on {g[0].device}, not on {self.device}")
            rc = capi.lib().artalk_pcm_push(self._h, ids, n, data, frames, int(dev), capi.current_stream_ptr())
            if dev and rc == capi.OK:
                for g in got:
                    if g[2]:
                        g[0].record_stream(torch.cuda.current_stream())      # the launch reads the packet in place
        if rc != capi.OK:
            self._raise("artalk_pcm_push refused" if rc != capi.EHIP else "artalk_pcm_push failed", rc)

    def end(self, streams):
        """The listed streams' signals end here: the samples that were waiting for frames that will not come are written (one launch),
        and ``take`` then serves the rest, the last row short."""
        streams, ids = self._ids(streams)
        with torch.cuda.device(self.device):
            rc = capi.lib().artalk_pcm_end(self._h, ids, len(streams), capi.current_stream_ptr())
        if rc != capi.OK:
            self._raise("artalk_pcm_end refused" if rc != capi.EHIP else "artalk_pcm_end failed", rc)

    # ------------------------------------------------------------------------------------------------ blocks out
    def _available(self, st):
        n, ended = C.c_int64(0), C.c_int(0)
        rc = capi.lib().artalk_pcm_available(self._h, st.id, C.byref(n), C.byref(ended))
        if rc != capi.OK:
            self._raise("artalk_pcm_available", rc)
        return int(n.value), bool(ended.value)

    def available(self, st):
        """16 kHz samples written and not yet taken (host arithmetic: nothing waits for the device)."""
        return self._available(st)[0]

    def ended(self, st):
        return self._available(st)[1]

    def ready(self, st):
        """``take`` would serve this stream: it holds a full block, or it has ended and holds at least one sample."""
        n, ended = self._available(st)
        return n >= self.block or (ended and n >= 1)

    def drained(self, st):
        """The stream has ended and every sample has been taken."""
        n, ended = self._available(st)
        return ended and n == 0

    def next_valid(self, streams):
        """The ``n_valid`` that ``take(streams)`` is going to report, without taking anything."""
        out = []
        for st in streams:
            n, ended = self._available(st)
            if not (n >= self.block or (ended and n >= 1)):
                raise RuntimeError(f"stream {st.id} holds {n} samples: neither a block of {self.block} nor the rest of an ended stream")
            out.append(min(n, self.block))
        return out

    def take(self, streams):
        """The oldest block of each listed stream -> ``(chunks (n, block) float32 on the device, n_valid)``: row i is zero past its
        ``n_valid[i]`` real samples (``block``, or fewer on the last row of a stream that has ended).  One launch on the current
        stream.  A stream that is not ``ready`` is refused with nothing taken."""
        streams, ids = self._ids(streams)
        n = len(streams)
        if not n:
            raise ValueError("take lists at least one stream")
        n_valid = (C.c_int64 * n)()
        with torch.cuda.device(self.device):
            out = torch.empty(n, self.block, dtype=torch.float32, device=self.device)
            rc = capi.lib().artalk_pcm_take(self._h, ids, n, capi.ptr(out), out.stride(0), n_valid, capi.current_stream_ptr())
        if rc != capi.OK:
            self._raise("artalk_pcm_take refused" if rc != capi.EHIP else "artalk_pcm_take failed", rc)
        return out, [int(v) for v in n_valid]
