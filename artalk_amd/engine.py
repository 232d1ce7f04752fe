"""Host-side mirror of the reference's ``ARTAvatarInferEngine`` (``inference.py:18-95``) for the audio->motion path.

Same constructor arguments, attributes and methods as the reference class, so code written against it (the CLI
at ``inference.py:225-237``, the Gradio handler at ``:99-125``) keeps working for everything up to the FLAME
codes.  Rendering (``inference.py:59-87``: FLAME mesh / GAGAvatar, PyAV muxing) is downstream of the drop-in
boundary: ``rendering`` only forwards to what the caller plugs in - the FLAME model and the mesh renderer
(``artalk_amd.flame.FLAMEModel``, ``artalk_amd.render.RenderMesh``) or the GAGAvatar head with its scale-5 FLAME model
(``artalk_amd.gaga.GAGAvatar``), and with ``output=`` hands the frames over in 8 bits as an encoder takes them
(``artalk_amd.frames``); the identity side of GAGAvatar, encoding and muxing are out of scope.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List, Optional, Sequence

import torch

from . import capi
from .config import ARTalkConfig
from .model import BitwiseARModel


class ARTAvatarInferEngine:
    def __init__(self, load_gaga=False, fix_pose=False, clip_length=750, device="cuda",
                 ckpt_path="./assets/ARTalk_wav2vec.pt", config_path=None, state_dict=None, config=None, model=None,
                 calibration=None, precision=None, gaga=None, gaga_flame=None, gaga_precision=None, gaga_ckpt=None, gaga_tracked=None):
        """Arguments of the reference class, plus (all optional): ``state_dict`` / ``config`` instead of a checkpoint file, ``model``
        (an already loaded BitwiseARModel), and ``calibration`` - the f16x3 site scales to start from: a ``save_scales`` file or a
        ``{site: exponent}`` dict (``load_scales``), or a sequence of 16 kHz audio tensors to calibrate on once here (``calibrate``).
        None keeps the model's scales (a checkpoint with outlier activations then recalibrates on its first outlier batch).
        ``precision``: the GEMM arithmetic (``BitwiseARModel.set_precision``: 'f16x3', 'f32' or 'bf16'); None keeps the model's.
        ``gaga``: an ``artalk_amd.gaga.GAGAvatar`` or the path of an avatar pack (``GAGAvatar.load``), with ``gaga_flame``, an
        ``artalk_amd.flame.FLAMEModel`` built with ``scale=5.0``: the photoreal head behind ``rendering(shape_id=<avatar id>)``.
        Both can also be plugged into ``engine.GAGAvatar`` / ``engine.GAGAvatar_flame`` later, like ``flame_model``.
        ``gaga_precision``: the arithmetic of the head's upsampler convolutions (``GAGAvatar.set_precision``: 'f32', 'bf16x3' or
        'bf16'); None keeps the head's.
        ``gaga_ckpt`` / ``gaga_tracked`` instead of ``gaga``: the reference's two files, ``GAGAvatar.pt`` and ``tracked.pt``, each as a
        dict or as a path that ``torch.load(weights_only=True)`` can read (``GAGAvatar.from_checkpoint``): the avatars are then built
        on the device from their tracked photos."""
        if load_gaga and gaga is None and gaga_ckpt is None:
            raise NotImplementedError("load_gaga=True needs gaga=: an artalk_amd.gaga.GAGAvatar or the path of an avatar pack.  The "
                                      "reference builds its avatars with DINOv2 from torch.hub, which is not part of this package: "
                                      "export a pack on a machine that runs the reference (INTEGRATION.md section 1d)")
        self.device = device
        self.fix_pose = fix_pose
        self.clip_length = clip_length
        audio_encoder = "wav2vec"                                           # inference.py:23
        if model is not None:          # an already loaded BitwiseARModel (several engines may share the 2 GB of weights)
            state_dict, config = {}, model.cfg
        if state_dict is None:
            # FileNotFoundError for a missing checkpoint, like torch.load at inference.py:24
            state_dict = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        if config is None:
            if config_path is not None:
                configs = json.load(open(config_path))
            else:
                configs = ARTalkConfig.full().reference_dict()            # == assets/config.json
            configs["AR_CONFIG"]["AUDIO_ENCODER"] = audio_encoder
            config = ARTalkConfig.from_reference_dict(configs)
        if model is not None:
            self.ARTalk = model
        else:
            self.ARTalk = BitwiseARModel(config).eval().to(device)
            self.ARTalk.load_state_dict(state_dict, strict=True)
        if calibration is not None:
            if isinstance(calibration, (str, os.PathLike, dict)):
                self.ARTalk.load_scales(calibration)
            else:
                self.ARTalk.calibrate(list(calibration))
        if precision is not None:
            self.ARTalk.set_precision(precision)
        # renderer-side attributes of the reference object; filled by whoever owns the (out of scope) renderers
        self.flame_model = None
        self.mesh_renderer = None
        self.output_dir = "render_results/ARTAvatar_{}".format(audio_encoder)
        self.style_motion = None
        self.GAGAvatar = None
        self.GAGAvatar_flame = gaga_flame
        self.live_audio = None                                              # the audio front door, made by the first open_stream(audio=...)
        if gaga is not None:
            from .gaga import GAGAvatar
            self.GAGAvatar = gaga if isinstance(gaga, GAGAvatar) else GAGAvatar.load(gaga, device=device)
        elif gaga_ckpt is not None:
            from .gaga import GAGAvatar
            if gaga_tracked is None:
                raise ValueError("gaga_ckpt= needs gaga_tracked=: the tracked identities (tracked.pt), as a dict or a path")
            ckpt = self._load_plain(gaga_ckpt, "gaga_ckpt")
            if "model" in ckpt and "head_base" not in ckpt:
                ckpt = ckpt["model"]
            self.GAGAvatar = GAGAvatar.from_checkpoint(ckpt, self._load_plain(gaga_tracked, "gaga_tracked"), flame=gaga_flame, device=device)
        if self.GAGAvatar is not None and gaga_precision is not None:
            self.GAGAvatar.set_precision(gaga_precision)

    @staticmethod
    def _load_plain(what, name):
        """A dict as it is; a path through torch.load(weights_only=True).  A file that needs pickle is refused."""
        if isinstance(what, dict):
            return what
        import pickle
        try:
            got = torch.load(what, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as e:
            raise ValueError(f"{name}={what!r} cannot be read with weights_only=True (it needs pickle, which is not run here): load it "
                             f"yourself where you trust it and pass the dict ({str(e).splitlines()[0]})") from None
        if not isinstance(got, dict):
            raise ValueError(f"{name}={what!r} holds a {type(got).__name__}, not a dict")
        return got

    def set_style_motion(self, style_motion):
        if isinstance(style_motion, str):
            style_motion = torch.load("assets/style_motion/{}.pt".format(style_motion), map_location="cpu", weights_only=True)
        assert style_motion.shape == (50, 106), f"Invalid style_motion shape: {style_motion.shape}."
        self.style_motion = style_motion[None].to(self.device)

    # ------------------------------------------------------------------ inference.py:47-57
    def inference(self, audio, clip_length=None):
        audio_batch = {"audio": audio[None].to(self.device), "style_motion": self.style_motion}
        pred_motions = self.ARTalk.inference(audio_batch, with_gtmotion=False)[0]
        return self._postprocess(pred_motions, clip_length)

    def inference_batch(self, audios: Sequence[torch.Tensor], style_motions: Optional[Sequence[Optional[torch.Tensor]]] = None,
                        clip_length=None) -> List[torch.Tensor]:
        """Data-parallel form of ``inference``: B clips in one pass, each post-processed like a single clip."""
        if style_motions is None and self.style_motion is not None:
            style_motions = [self.style_motion[0]] * len(audios)
        preds = self.ARTalk.inference_batch(audios, style_motions)
        return [self._postprocess(p, clip_length) for p in preds]

    def _postprocess(self, pred_motions, clip_length=None):
        clip_length = clip_length if clip_length is not None else self.clip_length
        pred_motions = self.smooth_motion_savgol_device(pred_motions)[:clip_length]
        if self.fix_pose:
            pred_motions[..., 100:103] *= 0.0
        pred_motions[..., 104:] *= 0.0
        return pred_motions

    # ------------------------------------------------------------------ live streams (independent sessions)
    def open_stream(self, style_motion=None, shape_id=None, audio=None):
        """One live stream (``BitwiseARModel.open_session``) with the engine's style clip unless ``style_motion`` ((50, 106)) is given.
        Streams join and leave independently: ``stream_step`` takes any subset of them, ``stream.close()`` frees one.
        With a GAGAvatar head plugged in and a ``shape_id`` (an avatar id) the stream also gets a stream of the head
        (``GAGAvatar.open_stream``), kept under the session's id for ``stream_render``; ``close_stream`` closes both halves.
        ``audio=(sample_rate, channels, dtype)`` (``dtype``: "s16" or "f32") gives the stream an audio half as well, a stream of the
        engine's ``artalk_amd.live_audio.LiveAudio``: ``stream_feed`` takes its raw PCM packets and ``stream_step(streams)`` its blocks.
        A format the front door does not take raises ``ValueError`` before a session exists."""
        if style_motion is None and self.style_motion is not None:
            style_motion = self.style_motion[0]
        if audio is not None:
            from . import live_audio
            sample_rate, channels, dtype = audio
            live_audio.check_format(channels, dtype)
            live_audio.rate_geometry(sample_rate)
        head = getattr(self, "GAGAvatar", None)
        head_stream = head.open_stream(shape_id) if head is not None and shape_id is not None else None      # (KeyError before a session exists)
        audio_stream = self._front_door().open(sample_rate, channels, dtype) if audio is not None else None
        try:
            st = self.ARTalk.open_session(style_motion)
        except Exception:
            if audio_stream is not None:
                audio_stream.close()
            raise
        if head_stream is not None:
            self._head_streams()[st.id] = head_stream
        if audio_stream is not None:
            self._audio_streams()[st.id] = audio_stream
        return st

    def _front_door(self):
        """The engine's LiveAudio, made on first use with the model's block (64 000 samples)."""
        if getattr(self, "live_audio", None) is None:
            from .live_audio import LiveAudio
            self.live_audio = LiveAudio(device=self.device, block=self.ARTalk.cfg.samples_per_chunk)
        return self.live_audio

    def _audio_streams(self):
        if not hasattr(self, "_pcm_streams"):      # (engines assembled without __init__)
            self._pcm_streams = {}
        return self._pcm_streams

    def _audio_of(self, streams):
        books = self._audio_streams()
        for st in streams:
            if st.id not in books:
                raise ValueError(f"session {st.id} was opened without audio= (or closed): it has no audio half")
        return [books[st.id] for st in streams]

    def stream_feed(self, streams, packets):
        """Raw PCM in: one packet per listed stream (``bytes``, a numpy array, a CPU or CUDA tensor ``(frames, channels)`` in the
        format the stream was opened with, of any length), resampled to 16 kHz mono on the device by one launch for all of them
        (``LiveAudio.push``).  Nothing waits for the device."""
        self._front_door().push(self._audio_of(streams), packets)

    def stream_audio_end(self, streams):
        """The listed streams' senders have hung up (``LiveAudio.end``): what is left becomes ready, the last block short."""
        self._front_door().end(self._audio_of(streams))

    def stream_ready(self, streams):
        """The streams of ``streams``, in order, that ``stream_step(streams)`` can take a block from: a full 4 s, or the rest of a
        stream that has ended."""
        live = self._front_door()
        return [st for st, a in zip(streams, self._audio_of(streams)) if live.ready(a)]

    def stream_drained(self, st):
        """The stream's audio has ended and every block has been stepped: after its last ``stream_step`` the loop closes it - after a
        ``stream_flush`` when its last block was a full one, which ended nothing."""
        return self._front_door().drained(self._audio_of([st])[0])

    def _head_streams(self):
        if not hasattr(self, "_gaga_streams"):      # (engines assembled without __init__)
            self._gaga_streams = {}
        return self._gaga_streams

    def close_stream(self, st):
        """Closes a stream of ``open_stream``: its session and, if it has one, its stream of the head."""
        head_stream = self._head_streams().pop(st.id, None)
        if head_stream is not None:
            head_stream.close()
        audio_stream = self._audio_streams().pop(st.id, None)
        if audio_stream is not None:
            audio_stream.close()
        st.close()

    def stream_render(self, streams, frames, spans, output=None, host=False, order="time", jpeg=None):
        """Photoreal frames of what ``stream_step(smooth=True)`` or ``stream_flush`` returned for ``streams``: ``frames`` (n, R, 106) and
        ``spans[i] = (first, count)`` -> ``(images, index)`` from one ``GAGAvatar.render_streams`` call.  ``images`` holds
        ``sum(count)`` frames - (.., 3, S, S) in [0, 1], or with ``output="rgb24"`` / ``"yuv420p"`` the 8-bit frames of
        ``artalk_amd.frames`` (``host=True``: in pinned memory on the CPU) - in ``order`` ("time": frame k of every stream before frame
        k + 1 of any; "stream": stream by stream); ``index`` (CPU, int64) names every frame: (position in ``streams``, absolute frame
        number ``first + k``).  Every stream keeps its own forehead EMA across steps.  A stream opened without ``shape_id`` raises
        ``ValueError``.  ``output="jpeg"`` (``jpeg=dict(quality=, subsampling=, cap=)``): ``images`` is ``(data (.., cap), sizes)``, one
        baseline JPEG stream per frame (``artalk_amd.frames.encode_jpeg``) - with ``host=True`` what a Motion-JPEG sender puts on the
        wire after ``frames.split_jpeg``."""
        head, flame = getattr(self, "GAGAvatar", None), getattr(self, "GAGAvatar_flame", None)
        if head is None or flame is None:
            raise RuntimeError("stream_render needs the GAGAvatar head and its scale-5 FLAME model (engine.GAGAvatar, engine.GAGAvatar_flame)")
        books = self._head_streams()
        for st in streams:
            if st.id not in books:
                raise ValueError(f"session {st.id} was opened without shape_id (or closed): it has no stream of the head")
        if len(spans) != len(streams):
            raise ValueError(f"spans holds {len(spans)} entries, streams {len(streams)}")
        images, index = head.render_streams([books[st.id] for st in streams], frames, flame, counts=[int(c) for _, c in spans], order=order,
                                            out="float" if output is None else output, host=host, jpeg=jpeg)
        if index.shape[0]:
            index[:, 1] += torch.tensor([int(f) for f, _ in spans], dtype=torch.int64)[index[:, 0]]
        return images, index

    def stream_step(self, streams, chunks=None, n_valid=None, smooth=False):
        """Next 4 seconds of the listed streams: ``chunks`` (n, 64000) -> (n, 100, 106) (with ``n_valid`` also the valid frame counts,
        ``BitwiseARModel.step_sessions``), with ``fix_pose`` applied and dims 104: zeroed as ``inference`` does.  These are the raw codes:
        the Savitzky-Golay window of ``inference`` reaches 4 frames into the future, which a live block does not have yet.

        ``smooth=True`` returns what ``inference`` returns instead, 4 frames (160 ms) late: ``(frames (n, 104, 106), spans)``, where the
        first ``count`` rows of ``frames[i]`` are stream i's frames ``first .. first + count - 1`` of ``_postprocess`` of its whole clip,
        bit for bit, and ``spans[i] = (first, count)`` - 96 frames on a stream's first step, 100 afterwards, everything that is left on
        its last (``BitwiseARModel.smooth_sessions``; the filter's state, 9 raw frames, lives with the session).  With ``n_valid`` a
        stream whose chunk has fewer than 100 valid frames ends there; a row with ``n_valid <= 0`` flushes a stream that has not ended
        yet and is skipped (count 0) for one that has.  A stream that ends on a chunk boundary never says so: ``stream_flush`` ends it.
        A stream that would end shorter than 9 frames raises ``ValueError`` before anything runs, as ``inference`` does for such a clip -
        also a stream that was never stepped and is listed with ``n_valid <= 0``: that row is a flush of nothing.  A stream is
        smoothed from its first step on or not at all: one that was stepped with ``smooth=False`` before raises ``RuntimeError``
        (the smoother would filter across the gap).

        ``chunks=None``: every stream's next block comes from its audio half (``open_stream(audio=...)``, ``stream_feed``), and
        ``n_valid`` is always passed - 64 000 for a full block, fewer for the last block of a stream whose audio has ended - so the
        result has the ``n_valid`` form.  Every listed stream must be ready (``stream_ready``); the checks above run before a block
        leaves its ring."""
        take = None
        if chunks is None:
            if n_valid is not None:
                raise ValueError("n_valid comes from the audio half when chunks is None")
            for st in streams:
                if st.closed:
                    raise RuntimeError(f"session {st.id} is closed ({st.why}); open it again")
            take = self._audio_of(streams)
            n_valid = self._front_door().next_valid(take)
        if not smooth:
            if take is not None:
                chunks, n_valid = self._front_door().take(take)
            res = self.ARTalk.step_sessions(streams, chunks, n_valid=n_valid)
            pred = res[0] if n_valid is not None else res
            if self.fix_pose:
                pred[..., 100:103] *= 0.0
            pred[..., 104:] *= 0.0
            return (pred, res[1]) if n_valid is not None else pred
        m = self.ARTalk
        n = len(streams)
        if n_valid is None:
            plan = [(100, False)] * n
        else:      # the frame counts step_sessions is going to report, known before it runs
            plan = [(m.valid_frames(st.fed, int(nv)), True) if int(nv) <= 0 or m.valid_frames(st.fed, int(nv)) < 100 else (100, False)
                    for st, nv in zip(streams, n_valid)]
        rows = [i for i, (st, (nf, last)) in enumerate(zip(streams, plan)) if not (st.smooth_done and nf == 0)]
        for i in rows:
            self._check_smoothable(streams[i], *plan[i])
        if take is not None:
            chunks, n_valid = self._front_door().take(take)
        res = m.step_sessions(streams, chunks, n_valid=n_valid)
        pred = res[0] if n_valid is not None else res
        frames = torch.zeros(n, 104, pred.shape[-1], dtype=pred.dtype, device=pred.device)
        spans = [(st.frames_seen, 0) for st in streams]
        if rows:
            sub, sub_spans = m.smooth_sessions([streams[i] for i in rows], pred if len(rows) == n else pred[rows],
                                               [plan[i][0] for i in rows], [plan[i][1] for i in rows])
            if len(rows) == n:
                frames = sub
            else:
                frames[rows] = sub
            for i, sp in zip(rows, sub_spans):
                spans[i] = sp
        return self._zero_dims(frames), spans

    def stream_flush(self, streams):
        """End streams that stopped on a chunk boundary, where no short chunk told ``stream_step(smooth=True)`` so: the 4 frames the
        smoother still holds back, ``(frames (n, 4, 106), spans)``.  A stream that has ended already raises ``RuntimeError``."""
        for st in streams:
            self._check_smoothable(st, 0, True)
        frames, spans = self.ARTalk.smooth_sessions(streams, None, [0] * len(streams), [True] * len(streams))
        return self._zero_dims(frames)[:, :4], spans

    def _check_smoothable(self, st, nf, last):
        if st.smooth_done:
            raise RuntimeError(f"session {st.id} has been smoothed to its end; open a new stream")
        if st.frames_seen != 100 * st.steps:
            raise RuntimeError(f"session {st.id} was stepped without smooth=True before ({st.frames_seen} frames smoothed in "
                               f"{st.steps} steps): a stream is smoothed from its first step on")
        if last and st.frames_seen + nf < 9:      # scipy raises for mode='interp' when window_length exceeds the signal length
            raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")

    def _zero_dims(self, frames):
        """The rest of ``_postprocess``, after smoothing."""
        if self.fix_pose:
            frames[..., 100:103] *= 0.0
        frames[..., 104:] *= 0.0
        return frames

    def smooth_motion_savgol(self, motion_codes):
        """``smooth_motion_savgol`` (inference.py:89-95) without the host round trip: Savitzky-Golay (5, 2) on all dims,
        (9, 3) on dims 100:103 of the unsmoothed signal, scipy's mode='interp' edges, as a device kernel (artalk_savgol)."""
        T = motion_codes.shape[0]
        if T < 9:
            # scipy raises for mode='interp' when window_length (9 for the pose dims) exceeds the signal length
            raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
        x = motion_codes.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = capi.lib().artalk_savgol(self.ARTalk._h, capi.ptr(x), capi.ptr(out), int(T), capi.current_stream_ptr())
        if rc != capi.OK:
            raise RuntimeError("artalk_savgol failed: " + self.ARTalk._err())
        return out

    smooth_motion_savgol_device = smooth_motion_savgol

    def rendering(self, audio, pred_motions, shape_id="mesh", shape_code=None, save_name="ARTAvatar.mp4", *, output=None, jpeg=None):
        """Downstream of the boundary (inference.py:59-87).  Produces the vertices the reference's mesh branch would
        feed its renderer when a FLAME model has been plugged in.  With a renderer plugged into ``engine.mesh_renderer`` as well
        (``artalk_amd.render.RenderMesh``) it returns what the reference stacks into ``pred_images`` (inference.py:70-72, :83):
        a ``(T, 3, S, S)`` tensor in [0, 1], on the device and from one batched call over all frames (the reference renders frame by
        frame and moves each image to the host).

        ``output="rgb24"`` or ``"yuv420p"`` (keyword only) returns, on both branches, the frames as a video encoder takes them
        (``artalk_amd.frames``): uint8 ``(T, S, S, 3)`` or ``(T, S * 3 // 2, S)`` on the device, the reference's
        ``(x * 255).astype(np.uint8)`` hand-over (inference.py:83-86, app/utils_videos.py) without the host round trip;
        ``artalk_amd.frames.write_y4m`` writes the second as a file any encoder reads.  It needs images: with no renderer plugged in it
        raises ``ValueError``.  Muxing and the audio track (PyAV) are not part of this package.

        ``output="jpeg"`` (``jpeg=dict(quality=, subsampling=, cap=)``) returns ``(data uint8 (T, cap), sizes int64 (T,))`` on the device
        instead: one baseline JPEG stream per frame, ``artalk_amd.frames.encode_jpeg`` of the ``"rgb24"`` frames;
        ``artalk_amd.frames.write_mjpeg`` writes them as a Motion-JPEG file."""
        if output == "jpeg":
            from .frames import encode_jpeg, jpeg_options, pack_frames
            quality, subsampling, cap = jpeg_options(jpeg)      # ValueError for a bad option, before anything runs
        elif jpeg is not None:
            raise ValueError('jpeg= goes with output="jpeg"')
        elif output is not None:
            from .frames import format_code, pack_frames
            format_code(output)      # ValueError for an unknown format, before anything runs
        head = getattr(self, "GAGAvatar", None)      # (engines assembled without __init__ have no such attribute)
        if shape_id != "mesh" and head is not None:
            # inference.py:73-79 in one library call: (T, 3, S, S) in [0, 1] on the device
            flame = getattr(self, "GAGAvatar_flame", None)
            if flame is None:
                raise RuntimeError("plug an artalk_amd.flame.FLAMEModel built with scale=5.0 into engine.GAGAvatar_flame")
            head.set_avatar_id(shape_id)
            if output == "jpeg":
                return head.render_clip(pred_motions, flame, out="jpeg", jpeg=jpeg)
            return head.render_clip(pred_motions, flame) if output is None else head.render_clip(pred_motions, flame, out=output)
        if shape_id != "mesh" or self.flame_model is None:
            raise NotImplementedError("rendering is outside the audio->motion path; plug a FLAME model into "
                                      "engine.flame_model to get vertices (and an artalk_amd.render.RenderMesh into "
                                      "engine.mesh_renderer to get images), or pass pred_motions to the reference renderer")
        if output is not None and getattr(self, "mesh_renderer", None) is None:
            raise ValueError(f"output={output!r} needs images: plug an artalk_amd.render.RenderMesh into engine.mesh_renderer "
                             "(without a renderer the mesh branch returns vertices)")
        if shape_code is None:
            shape_code = audio.new_zeros(1, 300).to(self.device).expand(pred_motions.shape[0], -1)
        else:
            assert shape_code.dim() == 2, f"Invalid shape_code dim: {shape_code.dim()}."
            assert shape_code.shape[0] == 1, f"Invalid shape_code shape: {shape_code.shape}."
            shape_code = shape_code.to(self.device).expand(pred_motions.shape[0], -1)
        verts = self.ARTalk.basic_vae.get_flame_verts(self.flame_model, shape_code, pred_motions, with_global=True)
        renderer = getattr(self, "mesh_renderer", None)      # (engines assembled without __init__ have no such attribute)
        if renderer is None:
            return verts
        images = renderer(verts)[0] / 255.0
        if output == "jpeg":
            return encode_jpeg(pack_frames(images, "rgb24"), quality=quality, subsampling=subsampling, cap=cap)
        return images if output is None else pack_frames(images, output)      # the reference's / 255.0 * 255.0 round trip
