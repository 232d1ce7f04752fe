"""Device stand-in for the per-frame half of the reference's ``GAGAvatar`` (``app/GAGAvatar/models.py:63-138``): motion codes in,
photoreal RGB frames out, from one library call per clip on top of ``artalk_gaga_*`` (``include/artalk_hip.h``, ``csrc/gaga.hip``).
What is computed is written out in DESIGN.md section 5 ("GAGAvatar head").

The identity half (DINOv2 through ``torch.hub``, the DPT head, the three ``*GSGenerator``s) runs once per avatar: its result, the
avatar's Gaussians, comes in as data - a *pack* exported from a machine that runs the reference - or from
``artalk_amd.gsgen.GSGenerators.build_avatar`` through ``add_avatar``, or, with ``GAGAvatar.from_checkpoint``, is made here from the
identity's tracked photo by ``artalk_amd.dino.DINOBase`` and the generators the first time ``set_avatar_id`` names it.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import capi
from . import frames as _frames
from . import splat as _splat
from .styleunet import StyleUNet, noise_resolution

FORMAT = "artalk-gaga-avatars/1"
AVATAR_FIELDS = {"xyz": 3, "colors": 32, "opacities": 1, "scales": 3, "rotations": 4}      # per-Gaussian widths
PACK_FIELDS = ("format", "upsampler", "water_mark", "n_dynamic", "avatars")
FOCAL = 12.0
MOTION_DIM = 106


def camera_matrices(rot_codes, transform_matrix):
    """``artalk_gaga_cameras`` (host only): head-rotation codes (T, 3) and the avatar's (3, 4) ``transform_matrix`` -> (view (T, 4, 4),
    projection (T, 4, 4), cam (T, 3, 4)).  cam is the frame's ``t_transform``: ``transform_emoca_to_p3d(codes)[:, :3, :3]`` beside the
    avatar's own translation; view and projection are what ``artalk_amd.splat.build_camera_matrices(cam, 12, 12)`` makes of it.
    Evaluated in double and rounded once; ``rot_codes`` is not modified."""
    r = torch.as_tensor(rot_codes).detach().to(dtype=torch.float32, device="cpu").reshape(-1, 3).contiguous()
    tm = torch.as_tensor(transform_matrix).detach().to(dtype=torch.float32, device="cpu").contiguous()
    if tuple(tm.shape) != (3, 4):
        raise ValueError(f"transform_matrix must be (3, 4), got {tuple(tm.shape)}")
    T = int(r.shape[0])
    view, proj, cam = torch.empty(T, 4, 4), torch.empty(T, 4, 4), torch.empty(T, 3, 4)
    L = capi.lib()
    rc = L.artalk_gaga_cameras(capi.ptr(r), 3, T, capi.ptr(tm), capi.ptr(view), capi.ptr(proj), capi.ptr(cam))
    if rc != capi.OK:
        raise ValueError("artalk_gaga_cameras refused: " + L.artalk_gaga_last_error(None).decode())
    return view, proj, cam


def _check_avatar(name, av, n_dynamic):
    if not isinstance(av, dict):
        raise ValueError(f"avatar {name!r} must be a dict")
    for k in tuple(AVATAR_FIELDS) + ("shapecode", "transform_matrix"):
        if k not in av:
            raise ValueError(f"avatar {name!r} lacks {k!r}")
    N = None
    out = {}
    for k, width in AVATAR_FIELDS.items():
        t = torch.as_tensor(av[k]).detach().to(dtype=torch.float32, device="cpu")
        if t.dim() == 3 and t.shape[0] == 1:      # the reference keeps a batch axis of 1 on _gs_params
            t = t[0]
        t = t.reshape(t.shape[0], -1)
        if t.shape[1] != width:
            raise ValueError(f"avatar {name!r}: {k} must be (N, {width}), got {tuple(t.shape)}")
        if N is None:
            N = int(t.shape[0])
        if t.shape[0] != N:
            raise ValueError(f"avatar {name!r}: {k} holds {t.shape[0]} Gaussians, xyz {N}")
        out[k] = t.contiguous()
    if N < n_dynamic:
        raise ValueError(f"avatar {name!r} holds {N} Gaussians, fewer than the {n_dynamic} that ride on the vertices")
    out["shapecode"] = torch.as_tensor(av["shapecode"]).detach().to(dtype=torch.float32, device="cpu").reshape(-1).contiguous()
    tm = torch.as_tensor(av["transform_matrix"]).detach().to(dtype=torch.float32, device="cpu")
    if tuple(tm.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"avatar {name!r}: transform_matrix must be (3, 4), got {tuple(tm.shape)}")
    out["transform_matrix"] = tm.reshape(-1, tm.shape[-2], 4)[0][:3].contiguous()
    return out


class GagaStream:
    """One live stream of ``GAGAvatar.open_stream``: ``id`` (never reused), ``avatar_id``, ``closed``, and ``set_avatar(id)`` (the forehead
    EMA is kept, as the reference's ``set_avatar_id`` keeps it), ``reset()`` (the next frame is taken as it is) and ``close()``.  The
    stream's EMA state lives in the head's library object, in a row of its own; it is opened there by the first render that lists it."""

    def __init__(self, head, sid, avatar_id):
        self._head, self.id, self.avatar_id, self.closed = head, int(sid), avatar_id, False
        self._lib = None          # the library's stream id

    def set_avatar(self, avatar_id):
        self._check_open()
        self._head._known_avatar(avatar_id)
        self.avatar_id = avatar_id

    def reset(self):
        self._check_open()
        if self._lib is not None:
            if capi.lib().artalk_gaga_stream_reset(self._head._h, self._lib) != capi.OK:
                raise RuntimeError("artalk_gaga_stream_reset failed: " + self._head._err())

    def close(self):
        if self.closed:
            return
        if self._lib is not None and self._head._h is not None:
            if capi.lib().artalk_gaga_stream_close(self._head._h, self._lib) != capi.OK:
                raise RuntimeError("artalk_gaga_stream_close failed: " + self._head._err())
        self._lib, self.closed = None, True
        self._head._streams.pop(self.id, None)

    def _check_open(self):
        if self.closed:
            raise ValueError(f"stream {self.id} is closed")


class _JpegPieces:
    """The ``(data, sizes)`` result of a render call with ``out="jpeg"``, filled piece by piece: each piece of rgb24 frames is encoded on
    the current stream into its slots (``frames.JpegEncoder``); with ``host`` its slots and sizes are then copied to the pinned result on
    a copy stream, behind an event, while the caller renders the next piece."""

    def __init__(self, T, S, device, jpeg, host):
        quality, subsampling, cap = _frames.jpeg_options(jpeg)
        self.cap = _frames.jpeg_default_cap(S, S) if cap is None else cap
        self.encoder = _frames.jpeg_encoder(device, quality, subsampling)
        self.data = torch.empty((T, self.cap), dtype=torch.uint8, device=device)
        self.sizes = torch.empty((T,), dtype=torch.int64, device=device)
        self.host = bool(host)
        if self.host:
            self.data_host = torch.empty((T, self.cap), dtype=torch.uint8, pin_memory=True)
            self.sizes_host = torch.empty((T,), dtype=torch.int64, pin_memory=True)
            self.copy_stream = torch.cuda.Stream(device)

    def put(self, t0, rgb):
        t1 = t0 + int(rgb.shape[0])
        self.encoder.encode(rgb, cap=self.cap, out=(self.data[t0:t1], self.sizes[t0:t1]))
        if self.host:
            done = torch.cuda.Event()
            done.record()
            self.copy_stream.wait_event(done)
            with torch.cuda.stream(self.copy_stream):
                self.data_host[t0:t1].copy_(self.data[t0:t1], non_blocking=True)
                self.sizes_host[t0:t1].copy_(self.sizes[t0:t1], non_blocking=True)

    def finish(self):
        """(also after a failure: a copy may be in flight)"""
        if self.host:
            torch.cuda.current_stream().wait_stream(self.copy_stream)
            torch.cuda.current_stream().synchronize()

    def result(self):
        return (self.data_host, self.sizes_host) if self.host else (self.data, self.sizes)


class GAGAvatar:
    """``GAGAvatar(avatars, upsampler, water_mark=None, image_size=512, n_dynamic=5023, forehead_indices=None, device="cuda")``.

    ``avatars``: ``{id: {"xyz", "colors", "opacities", "scales", "rotations", "shapecode", "transform_matrix"}}`` - an identity's
    ``_gs_params`` after the reference's first ``forward_expression`` and its tracked ``shapecode`` / ``transform_matrix``.
    ``upsampler``: an ``artalk_amd.styleunet.StyleUNet`` or its state dict.  ``water_mark``: a ``(4, h, w)`` RGBA tensor in [0, 1]
    already at its final size (the reference resizes its logo to 82 x 256 with torchvision's antialiased resize: the exporter's job).
    ``forehead_indices``: None = the reference's 68 vertices when the FLAME model has more than 3913, else none.

    The device is first touched by ``render_clip``.  The forehead EMA state lives in the library object and survives clips and
    ``set_avatar_id``, as ``upper_points`` does in the reference; ``reset_motion_state`` (ours) unsets it."""

    def __init__(self, avatars, upsampler, water_mark=None, image_size=512, n_dynamic=5023, forehead_indices=None, device="cuda", _tracked=None):
        self.image_size, self.n_dynamic = int(image_size), int(n_dynamic)
        self.device = torch.device(device)
        # from_checkpoint: the identities still to be turned into Gaussians, and the two modules that do it
        self._tracked, self._dino, self._gsgen, self.flame_model = _tracked, None, None, None
        if not isinstance(avatars, dict) or not (avatars or _tracked):
            raise ValueError("avatars must be a non-empty dict")
        self.all_gagavatar_id = {k: _check_avatar(k, v, self.n_dynamic) for k, v in avatars.items()}
        if isinstance(upsampler, StyleUNet):
            if upsampler.out_size != self.image_size or upsampler.in_dim != 32 or upsampler.out_dim != 3:
                raise ValueError(f"the upsampler must map 32 channels to 3 at {self.image_size} x {self.image_size}")
            self.upsampler, self._upsampler_sd = upsampler, None
        else:
            self._upsampler_sd = dict(upsampler)
            self.upsampler = StyleUNet(self.image_size, self.image_size, 32, 3)
            self.upsampler.load_state_dict(self._upsampler_sd)      # names and shapes are checked here; the upload waits for the device
        if water_mark is not None:
            water_mark = torch.as_tensor(water_mark).detach().to(dtype=torch.float32, device="cpu").contiguous()
            if water_mark.dim() != 3 or water_mark.shape[0] != 4:
                raise ValueError(f"water_mark must be (4, h, w), got {tuple(water_mark.shape)}")
            if water_mark.shape[1] > self.image_size or water_mark.shape[2] > self.image_size:
                raise ValueError(f"a water_mark of {tuple(water_mark.shape[1:])} does not fit the {self.image_size} x {self.image_size} image")
        self._water_mark = water_mark
        if forehead_indices is not None:
            forehead_indices = [int(i) for i in forehead_indices]
            if len(set(forehead_indices)) != len(forehead_indices):
                raise ValueError("forehead_indices lists a vertex twice")
            if any(i < 0 or i >= self.n_dynamic for i in forehead_indices):
                raise ValueError(f"forehead_indices must lie in [0, {self.n_dynamic})")
        self.forehead_indices = forehead_indices
        self.cam_params = {"focal_x": FOCAL, "focal_y": FOCAL, "size": [self.image_size, self.image_size]}
        self._h = None
        self._flame = None          # the FLAMEModel the library object borrows
        self._tracked_name = None
        self._uploaded = None       # id of the avatar the library object holds
        self._index, self._borrowed = None, None
        self._slab = 0
        # live streams: open streams by id, avatar id -> pool slot, the slots whose upload is current, the pool's size on the device
        self._resident, self._streams, self._next_stream = 4, {}, 0
        self._slot_of, self._fresh, self._pool = {}, set(), None

    # ---- packs ----
    @classmethod
    def load(cls, path, device="cuda", forehead_indices=None):
        pack = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(pack, dict) or pack.get("format") != FORMAT:
            got = pack.get("format") if isinstance(pack, dict) else type(pack).__name__
            raise ValueError(f"{path}: not an avatar pack of format {FORMAT!r} (found {got!r})")
        missing = [k for k in PACK_FIELDS if k not in pack]
        if missing:
            raise ValueError(f"{path}: the pack lacks {', '.join(missing)}")
        wm = pack["water_mark"]
        size = int(pack.get("image_size", 512))
        return cls(pack["avatars"], pack["upsampler"], water_mark=wm, image_size=size, n_dynamic=int(pack["n_dynamic"]),
                   forehead_indices=forehead_indices, device=device)

    @classmethod
    def from_checkpoint(cls, model_state_dict, tracked, water_mark=None, flame=None, device="cuda", image_size=None, heads=None,
                        forehead_indices=None):
        """The whole head from the reference's two files (ours): ``model_state_dict`` is the ``model`` dict of ``GAGAvatar.pt``
        (``upsampler.*`` -> the StyleUNet, ``head_base`` / ``gs_generator_*`` -> ``GSGenerators``, ``base_model.*`` -> ``DINOBase``; the
        sizes are read off the tensors - ``image_size`` off the upsampler's largest noise buffer - and ``heads`` defaults to vit_dim / 64), ``tracked`` the dict of ``tracked.pt``:
        ``{id: {"image" (3, h, w) in [0, 1], "transform_matrix", "shapecode"}}``.  An identity is turned into Gaussians the first time
        ``set_avatar_id`` names it (the reference does so in its first ``forward_expression``) and kept.  ``flame``: the scale-5
        ``FLAMEModel``, kept in ``flame_model`` for whoever renders."""
        from .dino import DINOBase
        from .gsgen import GSGenerators
        sd = model_state_dict
        for k in ("head_base", "base_model.dino_model.pos_embed", "base_model.dino_model.cls_token", "base_model.output_conv.weight"):
            if k not in sd:
                raise ValueError(f"the checkpoint lacks {k!r}: pass the 'model' dict of GAGAvatar.pt")
        if not isinstance(tracked, dict) or not tracked:
            raise ValueError("tracked must be a non-empty dict")
        tr = {name: cls._check_tracked(name, e) for name, e in tracked.items()}
        vit_dim = int(sd["base_model.dino_model.cls_token"].shape[-1])
        tokens = int(sd["base_model.dino_model.pos_embed"].shape[-2])
        grid = int(round((tokens - 1) ** 0.5))
        if grid * grid + 1 != tokens:
            raise ValueError(f"pos_embed holds {tokens} positions, which is no square grid and a class token")
        depth = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("base_model.dino_model.blocks."))
        out_dim = int(sd["base_model.output_conv.weight"].shape[0])
        n_verts, head_dim = (int(v) for v in sd["head_base"].shape)
        if image_size is None:
            image_size = max([int(v.shape[-1]) for k, v in sd.items() if k.startswith("upsampler.") and ".noises.noise" in k] or [512])
        head = cls({}, {k[len("upsampler."):]: v for k, v in sd.items() if k.startswith("upsampler.")}, water_mark=water_mark,
                   image_size=image_size, n_dynamic=n_verts, forehead_indices=forehead_indices, device=device, _tracked=tr)
        head._dino = DINOBase(out_dim, vit_dim, depth, int(heads) if heads else vit_dim // 64, grid, device=device).load_state_dict(sd)
        head._gsgen = GSGenerators(n_verts, head_dim, vit_dim, out_dim, 8 * grid, device=device).load_state_dict(sd)
        head.flame_model = flame
        return head

    @staticmethod
    def _check_tracked(name, e):
        if not isinstance(e, dict):
            raise ValueError(f"tracked identity {name!r} must be a dict")
        for k in ("image", "transform_matrix", "shapecode"):
            if k not in e:
                raise ValueError(f"tracked identity {name!r} lacks {k!r}")
        img = torch.as_tensor(e["image"]).detach().float()      # the reference: torch.tensor(value).float() for what is no tensor
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"tracked identity {name!r}: image must be (3, h, w), got {tuple(img.shape)}")
        tm = torch.as_tensor(e["transform_matrix"]).detach().to(dtype=torch.float32, device="cpu")
        if tuple(tm.shape[-2:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"tracked identity {name!r}: transform_matrix must be (3, 4), got {tuple(tm.shape)}")
        return {"image": img, "transform_matrix": tm, "shapecode": torch.as_tensor(e["shapecode"]).detach().float().cpu()}

    def add_avatar_image(self, name, image, transform_matrix, shapecode):
        """Adds or replaces a tracked identity of a head built by ``from_checkpoint`` (ours); its Gaussians are made the next time
        ``set_avatar_id`` names it."""
        if self._dino is None:
            raise RuntimeError("this head holds finished avatars only: build it with GAGAvatar.from_checkpoint to add identities by image")
        self._tracked[name] = self._check_tracked(name, {"image": image, "transform_matrix": transform_matrix, "shapecode": shapecode})
        self.all_gagavatar_id.pop(name, None)
        if self._uploaded == name:
            self._uploaded = None
        self._fresh.discard(self._slot_of.get(name))

    def _generate(self, name):
        e = self._tracked[name]
        f0, f1 = self._dino.forward(self._dino.prepare_image(e["image"]))
        self.add_avatar(name, self._gsgen.build_avatar(f0, f1, e["transform_matrix"], e["shapecode"]))

    def _default_id(self):
        names = list(self.all_gagavatar_id) + [k for k in (self._tracked or {}) if k not in self.all_gagavatar_id]
        return "11.jpg" if "11.jpg" in names else names[0]

    def save(self, path):
        if self._upsampler_sd is None:
            raise RuntimeError("this head was built around a loaded StyleUNet: construct it from the state dict to save a pack")
        torch.save({"format": FORMAT, "upsampler": self._upsampler_sd, "water_mark": self._water_mark, "n_dynamic": self.n_dynamic,
                    "image_size": self.image_size, "avatars": self.all_gagavatar_id}, path)

    # ---- torch.nn.Module look-alikes ----
    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GAGAvatar runs on the GPU only (there is no CPU fallback)")
        if self._h is not None and (device.index or 0) != (self.device.index or 0):
            raise RuntimeError(f"the head lives on {self.device}: build a new one for {device}")
        self.device = device
        return self

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _release(self):
        if self._h is not None:
            capi.lib().artalk_gaga_destroy(self._h)
            self._h = None
        # the pool and the streams' states went with the object: slots are uploaded and streams opened again by the next render
        self._pool = None
        self._fresh.clear()
        for st in self._streams.values():
            st._lib = None

    def _err(self):
        return capi.lib().artalk_gaga_last_error(self._h).decode()

    # ---- the reference's methods ----
    def set_avatar_id(self, avatar_id):
        if avatar_id not in self.all_gagavatar_id and self._tracked and avatar_id in self._tracked:
            self._generate(avatar_id)
        self.all_gagavatar_id[avatar_id]      # KeyError for an unknown id, like the reference's dict lookup
        self._tracked_name = avatar_id

    def add_avatar(self, name, avatar):
        """Adds or replaces an identity (ours): ``avatar`` as in the constructor, for instance what
        ``artalk_amd.gsgen.GSGenerators.build_avatar`` returns.  Replacing the tracked identity takes effect on the next clip."""
        self.all_gagavatar_id[name] = _check_avatar(name, avatar, self.n_dynamic)
        if self._uploaded == name:
            self._uploaded = None
        self._fresh.discard(self._slot_of.get(name))      # a resident copy is stale: the next render that needs it uploads it again

    def reset_motion_state(self):
        """Unset the forehead EMA: the next frame is taken as it is, like the reference's very first frame."""
        if self._h is not None:
            rc = capi.lib().artalk_gaga_reset_state(self._h)
            if rc != capi.OK:
                raise RuntimeError("artalk_gaga_reset_state failed: " + self._err())

    def set_slab(self, frames):
        """Frames per pass over the head's scratch (0: the default, what fits 512 MiB); never more than the upsampler's slab in force.
        Returns the request before the device is touched, the value in force afterwards."""
        frames = int(frames)
        if frames < 0 or frames > 64:
            raise ValueError("slab must be in 0..64 frames (0: the default)")
        self._slab = frames
        if self._h is None:
            return frames
        return int(capi.lib().artalk_gaga_set_slab(self._h, frames))

    def set_precision(self, name):
        """The arithmetic of the upsampler's convolutions (``StyleUNet.set_precision``: 'f32', 'bf16x3' or 'bf16').  The upsampler's
        handle does not change, so the library object and with it the forehead EMA state survive a switch."""
        self.upsampler.set_precision(name)
        return self

    @property
    def precision(self):
        return self.upsampler.precision

    def build_forward_batch(self, motion_code, flame_model):
        """The reference's two-step form.  The batch here is a handle for ``forward_expression``: the motion rows (a copy: unlike the
        reference, ``motion_code`` is not modified), the FLAME model and ``t_transform`` (T, 3, 4), the per-frame cameras.  The vertices
        and the forehead EMA are produced inside the library call that ``forward_expression`` makes, so the EMA advances there."""
        if self._tracked_name is None:
            self.set_avatar_id(self._default_id())
        motion_code = self._check_motion(motion_code)
        tm = self.all_gagavatar_id[self._tracked_name]["transform_matrix"]
        return {"motion_code": motion_code.clone(), "flame_model": flame_model,
                "t_transform": camera_matrices(motion_code[:, 100:103].cpu(), tm)[2].to(motion_code.device)}

    def forward_expression(self, batch, randomize_noise=True, noise=None, out="float"):
        return self.render_clip(batch["motion_code"], batch["flame_model"], randomize_noise=randomize_noise, noise=noise, out=out)

    # ---- the fast path ----
    @staticmethod
    def _check_motion(motion_codes):
        if not isinstance(motion_codes, torch.Tensor) or motion_codes.dim() != 2 or motion_codes.shape[1] < MOTION_DIM:
            raise ValueError(f"motion_codes must be a (T, {MOTION_DIM}) tensor")
        if not motion_codes.is_cuda:
            raise RuntimeError("GAGAvatar runs on the GPU: motion_codes must be a CUDA tensor (there is no CPU fallback)")
        return motion_codes

    def _device_motion(self, m, dense):
        """What both render calls ask of their motion tensor beyond its shape: on the GPU and on the head's device.  Returns it detached,
        as float32 rows the library can walk - ``dense``: contiguous as a whole; else rows of stride 1 that do not overlap."""
        if not m.is_cuda:
            raise RuntimeError("GAGAvatar runs on the GPU: motion_codes must be a CUDA tensor (there is no CPU fallback)")
        if (m.device.index or 0) != (self.device.index if self.device.index is not None else torch.cuda.current_device()):
            raise RuntimeError(f"motion_codes lives on {m.device}, the head on {self.device}")
        m = m.detach()
        fits = m.is_contiguous() if dense else m.stride(1) == 1 and (m.shape[0] <= 1 or m.stride(0) >= m.shape[1])
        return m if m.dtype == torch.float32 and fits else m.float().contiguous()

    @staticmethod
    def _format(out, host):
        """The library's code of ``out`` (0: float frames), after the check that ``host=True`` goes with an 8-bit format."""
        if out != "float":
            return _frames.format_code(out)
        if host:
            raise ValueError('host=True needs out="rgb24" or out="yuv420p"')
        return 0

    def _result_buffers(self, out, T, device, host, host_buffer=None):
        """The tensors a render call fills -> (the float or uint8 device tensor, the pinned host tensor or None).  ``host_buffer``: the
        caller's pinned tensor, checked against the result's shape and used instead of a new one."""
        S = self.image_size
        if host_buffer is not None:
            want = tuple(_frames.frame_shape(out, T, S, S)) if host else None
            if (want is None or not isinstance(host_buffer, torch.Tensor) or host_buffer.dtype != torch.uint8 or tuple(host_buffer.shape) != want
                    or not host_buffer.is_contiguous() or not host_buffer.is_pinned()):
                raise ValueError(f"host_buffer goes with host=True and must be a contiguous pinned uint8 tensor of shape {want}")
        shape = (T, 3, S, S) if out == "float" else _frames.frame_shape(out, T, S, S)
        res = torch.empty(shape, dtype=torch.float32 if out == "float" else torch.uint8, device=device)
        if host and host_buffer is None:
            host_buffer = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        return res, host_buffer

    def _raise_rc(self, rc, name):
        if rc == capi.EINVAL:
            raise ValueError(name + " refused: " + self._err())
        if rc != capi.OK:
            raise RuntimeError(name + " failed: " + self._err())

    def _avatar_args(self, name, flame_model):
        """The avatar arguments of ``artalk_gaga_set_avatar`` and ``artalk_gaga_pool_set``: N and the seven pointers."""
        av = self.all_gagavatar_id[name]
        if av["shapecode"].numel() != flame_model.n_betas - 100:
            raise ValueError(f"avatar {name!r}: shapecode holds {av['shapecode'].numel()} values, the FLAME model "
                             f"takes {flame_model.n_betas - 100}")
        return (int(av["xyz"].shape[0]),) + tuple(capi.ptr(av[k]) for k in tuple(AVATAR_FIELDS) + ("shapecode", "transform_matrix"))

    def _ensure(self, flame_model, avatar=True):
        """The library object for this FLAME model and, with ``avatar``, the tracked identity uploaded as the classic path's avatar."""
        L = capi.lib()
        if self._h is not None:
            # the library object borrows three handles: another FLAME model, reloaded upsampler weights or released splat buffers
            # mean a new object (and a new EMA state)
            borrowed = (getattr(flame_model, "_h", None), self.upsampler._h, _splat._handles.get(self._index))
            if self._flame is not flame_model or [b.value if b is not None else None for b in borrowed] != self._borrowed:
                self._release()
        if self._h is None:
            if getattr(flame_model, "_h", None) is None:
                raise ValueError("flame_model must be an artalk_amd.flame.FLAMEModel")
            if abs(float(flame_model.scale) - 5.0) > 0:
                raise ValueError(f"the GAGAvatar head skins at scale 5 (models.py: FLAMEModel(scale=5.0)); this FLAME model has scale {flame_model.scale}")
            if flame_model.n_verts != self.n_dynamic:
                raise ValueError(f"the FLAME model has {flame_model.n_verts} vertices, the pack's avatars {self.n_dynamic} dynamic Gaussians")
            dev = self.device
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            with torch.cuda.device(idx):
                self.upsampler.to(torch.device("cuda", idx))
                if not self.upsampler._loaded:
                    raise RuntimeError("the upsampler has no weights: load_state_dict first")
                h = C.c_void_p()
                rc = L.artalk_gaga_create(int(idx), flame_model._h, _splat._handle(torch.device("cuda", idx)), self.upsampler._h,
                                          int(flame_model.n_verts), int(flame_model.n_betas), self.image_size, C.byref(h))
                if rc != capi.OK:
                    raise ValueError("artalk_gaga_create refused: " + L.artalk_gaga_last_error(None).decode())
                self._h, self._flame, self._uploaded, self._index = h, flame_model, None, int(idx)
                self._borrowed = [flame_model._h.value, self.upsampler._h.value, _splat._handles[int(idx)].value]
                if self.forehead_indices is not None:
                    arr = (C.c_int32 * max(len(self.forehead_indices), 1))(*self.forehead_indices)
                    if L.artalk_gaga_set_forehead(h, arr, len(self.forehead_indices)) != capi.OK:
                        raise ValueError("artalk_gaga_set_forehead refused: " + self._err())
                if self._water_mark is not None:
                    wm = self._water_mark
                    if L.artalk_gaga_set_watermark(h, capi.ptr(wm), int(wm.shape[1]), int(wm.shape[2])) != capi.OK:
                        raise ValueError("artalk_gaga_set_watermark refused: " + self._err())
                if L.artalk_gaga_set_slab(h, self._slab) < 0:
                    raise ValueError("artalk_gaga_set_slab refused: " + self._err())
        if not avatar:
            return
        if self._tracked_name is None:
            self.set_avatar_id(self._default_id())
        if self._uploaded != self._tracked_name:
            if L.artalk_gaga_set_avatar(self._h, *self._avatar_args(self._tracked_name, flame_model)) != capi.OK:
                raise ValueError("artalk_gaga_set_avatar refused: " + self._err())
            self._uploaded = self._tracked_name

    def _noise_args(self, T, noise, randomize_noise, device, slab=None):
        """The noise arguments of a render call over T frames in slabs of ``slab`` (default: ``render_clip``'s) -> (pointers, batch
        strides, the tensors to keep alive)."""
        nl = self.upsampler.num_layers
        if noise is None and randomize_noise:
            slab = self.slab_in_force() if slab is None else slab
            parts = [[torch.empty(min(slab, T - f0), 1, noise_resolution(i), noise_resolution(i), device=device).normal_()
                      for i in range(nl)] for f0 in range(0, T, slab)]
            noise = [torch.cat([p[i] for p in parts]) for i in range(nl)]
        if noise is None:
            return None, None, None
        if len(noise) != nl:
            raise ValueError(f"noise must hold {nl} tensors")
        keep = []
        for i, n in enumerate(noise):
            r = noise_resolution(i)
            if not n.is_cuda or tuple(n.shape[1:]) != (1, r, r) or n.shape[0] not in (1, T):
                raise ValueError(f"noise[{i}] must be a CUDA tensor of shape (1 or {T}, 1, {r}, {r})")
            keep.append(n.detach().float().contiguous())
        ptrs = (C.c_void_p * nl)(*[t.data_ptr() for t in keep])
        strides = (C.c_int64 * nl)(*[0 if t.shape[0] == 1 else t.shape[2] * t.shape[3] for t in keep])
        return ptrs, strides, keep

    def slab_in_force(self):
        return None if self._h is None else int(capi.lib().artalk_gaga_set_slab(self._h, self._slab))

    @torch.no_grad()
    def render_clip(self, motion_codes, flame_model, randomize_noise=True, noise=None, out="float", host=False, jpeg=None):
        """motion_codes (T, 106) on the device -> (T, 3, S, S) in [0, 1] on the device, from one library call.  ``flame_model``: an
        ``artalk_amd.flame.FLAMEModel`` built with ``scale=5.0``.  Unlike the reference, ``motion_codes`` is NOT modified (there
        ``transform_emoca_to_p3d`` flips the sign of columns 100 and 102 in place through a view).  ``randomize_noise=True`` draws the
        StyleGAN noise with torch's generator once per slab (the reference: once per frame); ``False`` uses the stored buffers;
        ``noise`` - per layer a device tensor (T or 1, 1, r, r) - overrides both.

        ``out="rgb24"`` or ``"yuv420p"`` returns the frames as a video encoder takes them instead (``artalk_amd.frames``): uint8
        ``(T, S, S, 3)`` or ``(T, S * 3 // 2, S)``, byte-equal to ``pack_frames(render_clip(...), out)``, from one
        ``artalk_gaga_render_u8`` call that never holds the fp32 clip.  With ``host=True`` the result is a pinned CPU tensor, filled slab
        by slab while the next slab renders; the method synchronises the current stream before it returns it.

        ``out="jpeg"`` returns ``(data uint8 (T, cap), sizes int64 (T,))`` instead, one baseline JPEG stream per frame
        (``artalk_amd.frames.encode_jpeg``; ``jpeg=dict(quality=, subsampling=, cap=)``, defaults 90, "420", ``jpeg_default_cap``),
        byte-equal to ``encode_jpeg(render_clip(..., out="rgb24"))``: the clip is rendered in pieces of the slab in force, each piece
        is encoded on the device and, with ``host=True``, copied to the pinned result while the next piece renders."""
        if out == "jpeg":
            return self._render_clip_jpeg(motion_codes, flame_model, randomize_noise, noise, host, jpeg)
        if jpeg is not None:
            raise ValueError('jpeg= goes with out="jpeg"')
        fmt = self._format(out, host)
        m = self._device_motion(self._check_motion(motion_codes), dense=False)
        T = int(m.shape[0])
        stride = int(m.stride(0)) if T > 1 else int(m.shape[1])
        L = capi.lib()
        with torch.cuda.device(m.device):
            res, res_host = self._result_buffers(out, T, m.device, host)
            self._ensure(flame_model)
            if T == 0:
                return res_host if host else res
            ptrs, strides, keep = self._noise_args(T, noise, randomize_noise, m.device)
            if out == "float":
                rc = L.artalk_gaga_render(self._h, capi.ptr(m), stride, T, ptrs, strides, int(self.upsampler.activation), capi.ptr(res),
                                          capi.current_stream_ptr())
            else:
                rc = L.artalk_gaga_render_u8(self._h, capi.ptr(m), stride, T, ptrs, strides, int(self.upsampler.activation), fmt,
                                             capi.ptr(res), capi.ptr(res_host), capi.current_stream_ptr())
                if host:
                    torch.cuda.current_stream().synchronize()      # (also after a failure: a copy may be in flight)
        self._raise_rc(rc, "artalk_gaga_render" if out == "float" else "artalk_gaga_render_u8")
        return res_host if host else res

    # ---- live streams: many independent streams through one head ("Live streams through the head") ----
    def set_resident(self, slots=4):
        """Avatars that stay on the device at once (default 4); every open stream's avatar needs a slot.  Set before the first stream
        is opened."""
        slots = int(slots)
        if slots < 1 or slots > 4096:
            raise ValueError("slots must be in 1..4096")
        if self._streams:
            raise RuntimeError(f"{len(self._streams)} streams are open: set_resident comes before the first open_stream")
        if slots != self._resident:
            self._resident = slots
            self._slot_of.clear()
            self._fresh.clear()
            self._pool = None      # the next render reserves the pool anew
        return self

    def _known_avatar(self, avatar_id):
        if avatar_id not in self.all_gagavatar_id and self._tracked and avatar_id in self._tracked:
            self._generate(avatar_id)
        self.all_gagavatar_id[avatar_id]      # KeyError for an unknown id, as set_avatar_id

    def open_stream(self, avatar_id):
        """A ``GagaStream`` on ``avatar_id``: a forehead EMA state of its own, unset.  A tracked identity is turned into Gaussians here,
        as ``set_avatar_id`` does; apart from that the device is first touched by ``render_streams``."""
        self._known_avatar(avatar_id)
        st = GagaStream(self, self._next_stream, avatar_id)
        self._next_stream += 1
        self._streams[st.id] = st
        return st

    def stream_slab_in_force(self):
        """Frames per slab of ``render_streams`` (``artalk_gaga_streams_slab``: sized for the pool's avatars, where ``slab_in_force`` is
        sized for the classic path's); None before the library object exists."""
        return None if self._h is None else int(capi.lib().artalk_gaga_streams_slab(self._h))

    def _plan_slots(self, streams):
        """Books only: gives every avatar the listed streams name a slot - a free one, else one whose avatar no open stream names - and
        returns [(avatar id, slot)] for the slots the next render has to upload (new, or stale after ``add_avatar``)."""
        named = []
        for st in self._streams.values():
            if st.avatar_id not in named:
                named.append(st.avatar_id)
        if len(named) > self._resident:
            raise RuntimeError(f"the open streams name {len(named)} distinct avatars, the head keeps {self._resident} resident "
                               f"(set_resident); close a stream or build the head with more slots")
        for st in streams:
            if st.avatar_id in self._slot_of:
                continue
            taken = set(self._slot_of.values())
            free = [k for k in range(self._resident) if k not in taken]
            if not free:      # room is needed: an avatar no open stream names leaves (there is one: named fits)
                idle = next(a for a in self._slot_of if a not in named)
                free = [self._slot_of.pop(idle)]
            self._slot_of[st.avatar_id] = free[0]
            self._fresh.discard(free[0])
        todo = []
        for st in streams:
            slot = self._slot_of[st.avatar_id]
            if slot not in self._fresh and (st.avatar_id, slot) not in todo:
                todo.append((st.avatar_id, slot))
        return todo

    @staticmethod
    def plan_frames(counts, order="time", firsts=None, rows_per_stream=None):
        """The frame lists of a ``render_streams`` call, a pure function: ``counts[i]`` frames of stream i starting at its row
        ``firsts[i]`` (default 0) -> ``(frame_row, frame_stream_index, frame_k)``, three lists of ``sum(counts)`` ints.  ``order="time"``:
        frame k of every listed stream that still has one, then k + 1 - what a live sender wants; ``"stream"``: each stream's frames
        together.  ``frame_row`` is ``firsts[i] + k``, the row within stream i's own block, plus ``i * rows_per_stream`` when the blocks
        lie one after the other in one array."""
        counts = [int(c) for c in counts]
        firsts = [0] * len(counts) if firsts is None else [int(f) for f in firsts]
        if len(firsts) != len(counts):
            raise ValueError(f"firsts holds {len(firsts)} entries, counts {len(counts)}")
        if any(c < 0 for c in counts) or any(f < 0 for f in firsts):
            raise ValueError("counts and firsts must not be negative")
        if order == "time":
            pairs = [(i, k) for k in range(max(counts, default=0)) for i, c in enumerate(counts) if k < c]
        elif order == "stream":
            pairs = [(i, k) for i, c in enumerate(counts) for k in range(c)]
        else:
            raise ValueError(f'order must be "time" or "stream", got {order!r}')
        per = 0 if rows_per_stream is None else int(rows_per_stream)
        return [i * per + firsts[i] + k for i, k in pairs], [i for i, _ in pairs], [k for _, k in pairs]

    @torch.no_grad()
    def render_streams(self, streams, motion_codes, flame_model, counts=None, firsts=None, order="time", randomize_noise=True, noise=None,
                       out="float", host=False, host_buffer=None, jpeg=None):
        """Frames of many streams from one library call (``artalk_gaga_render_streams``).  ``streams``: n open ``GagaStream``s, each at
        most once; ``motion_codes`` (n, R, 106) on the device - what ``stream_step(smooth=True)`` returns - with ``counts[i]`` valid rows
        from row ``firsts[i]`` (defaults: R and 0).  Returns ``(frames, index)``: ``frames`` (sum(counts), 3, S, S) in [0, 1], or with
        ``out="rgb24"`` / ``"yuv420p"`` the uint8 shapes of ``artalk_amd.frames`` (``host=True``: pinned, on the CPU), in the order
        ``plan_frames(counts, order)`` gives; ``index`` a CPU int64 tensor (sum(counts), 2) of (position in ``streams``, k).  Every
        frame equals the frame a head of its own would render for that stream: each stream's forehead EMA walks its own frames only.
        Noise as in ``render_clip`` (a per-frame ``noise`` follows the order of ``frames``).  ``host_buffer``: with ``host=True``, a
        pinned uint8 tensor of the result's shape to fill and return instead of a new one - it is filled slab by slab, so another
        thread of a live sender can take a slab's frames out of it while the later slabs still render.

        ``out="jpeg"``: ``((data, sizes), index)`` with one JPEG stream per frame as in ``render_clip`` (``jpeg=`` as there; no
        ``host_buffer``), the frames in the same order and byte-equal to ``encode_jpeg`` of the ``out="rgb24"`` frames."""
        if out == "jpeg":
            if host_buffer is not None:
                raise ValueError('host_buffer goes with out="rgb24" or out="yuv420p"')
            return self._render_streams_jpeg(streams, motion_codes, flame_model, counts, firsts, order, randomize_noise, noise, host, jpeg)
        if jpeg is not None:
            raise ValueError('jpeg= goes with out="jpeg"')
        fmt = self._format(out, host)
        streams = list(streams)
        for st in streams:
            if not isinstance(st, GagaStream) or st._head is not self:
                raise ValueError("streams must hold GagaStreams of this head (GAGAvatar.open_stream)")
            if st.closed:
                raise ValueError(f"stream {st.id} is closed")
        if len({st.id for st in streams}) != len(streams):
            raise ValueError("a stream is listed twice: one call walks each stream's frames once")
        m = motion_codes
        if not isinstance(m, torch.Tensor) or m.dim() != 3 or m.shape[2] < MOTION_DIM or m.shape[0] != len(streams):
            raise ValueError(f"motion_codes must be a ({len(streams)}, R, {MOTION_DIM}) tensor: one block of rows per listed stream")
        m = self._device_motion(m, dense=True)
        n, R = int(m.shape[0]), int(m.shape[1])
        counts = [R] * n if counts is None else [int(c) for c in counts]
        firsts = [0] * n if firsts is None else [int(f) for f in firsts]
        if len(counts) != n or len(firsts) != n:
            raise ValueError(f"counts and firsts must hold {n} entries each")
        rows, which, ks = self.plan_frames(counts, order, firsts, R)
        if any(f + c > R for f, c in zip(firsts, counts)):
            raise ValueError(f"a stream's rows firsts[i] .. firsts[i] + counts[i] must lie within its {R} rows")
        T, W = len(rows), int(m.shape[2])
        index = torch.tensor([which, ks], dtype=torch.int64).t().contiguous().reshape(T, 2)
        L = capi.lib()
        with torch.cuda.device(m.device):
            res, res_host = self._result_buffers(out, T, m.device, host, host_buffer)
            todo = self._plan_slots(streams)
            self._ensure(flame_model, avatar=False)
            h = self._h
            if self._pool is None and streams:
                N = int(self.all_gagavatar_id[streams[0].avatar_id]["xyz"].shape[0])
                rc = L.artalk_gaga_pool_reserve(h, self._resident, N)
                if rc != capi.OK:
                    raise (ValueError if rc == capi.EINVAL else RuntimeError)("artalk_gaga_pool_reserve failed: " + self._err())
                self._pool = (self._resident, N)
                self._fresh.clear()
                todo = self._plan_slots(streams)
            for name, slot in todo:
                if L.artalk_gaga_pool_set(h, slot, *self._avatar_args(name, flame_model)) != capi.OK:
                    raise ValueError(f"artalk_gaga_pool_set refused avatar {name!r}: " + self._err())
                self._fresh.add(slot)
            for st in streams:
                if st._lib is None:
                    sid = C.c_int32(-1)
                    if L.artalk_gaga_stream_open(h, C.byref(sid)) != capi.OK:
                        raise RuntimeError("artalk_gaga_stream_open failed: " + self._err())
                    st._lib = int(sid.value)
            if T == 0:
                return (res_host if host else res), index
            ptrs, strides, keep = self._noise_args(T, noise, randomize_noise, m.device, self.stream_slab_in_force())
            frame_row = (C.c_int64 * T)(*rows)
            frame_stream = (C.c_int32 * T)(*[streams[i]._lib for i in which])
            frame_slot = (C.c_int32 * T)(*[self._slot_of[streams[i].avatar_id] for i in which])
            rc = L.artalk_gaga_render_streams(h, capi.ptr(m), W, T, frame_row, frame_stream, frame_slot, ptrs, strides,
                                              int(self.upsampler.activation), fmt, capi.ptr(res) if fmt == 0 else None,
                                              None if fmt == 0 else capi.ptr(res), capi.ptr(res_host), capi.current_stream_ptr())
            if host:
                torch.cuda.current_stream().synchronize()      # (also after a failure: a copy may be in flight)
        self._raise_rc(rc, "artalk_gaga_render_streams")
        return (res_host if host else res), index

    # ---- JPEG out: the render calls in pieces of a slab, each piece encoded on the device ("JPEG out") ----
    def _noise_rows(self, noise, T, rows):
        """The given per-layer noise for the frames ``rows`` (a slice or an index tensor) of a call over T frames."""
        if noise is None:
            return None
        for i, n in enumerate(noise):
            if not isinstance(n, torch.Tensor) or n.dim() != 4 or n.shape[0] not in (1, T):
                raise ValueError(f"noise[{i}] must be a CUDA tensor of shape (1 or {T}, 1, r, r)")
        return [n if n.shape[0] == 1 else n[rows] for n in noise]

    def _render_clip_jpeg(self, motion_codes, flame_model, randomize_noise, noise, host, jpeg):
        m = self._device_motion(self._check_motion(motion_codes), dense=False)
        T = int(m.shape[0])
        with torch.cuda.device(m.device):
            pieces = _JpegPieces(T, self.image_size, m.device, jpeg, host)
            self._ensure(flame_model)
            slab = max(1, int(self.slab_in_force()))
            try:
                for t0 in range(0, T, slab):
                    t1 = min(T, t0 + slab)
                    rgb = self.render_clip(m[t0:t1], flame_model, randomize_noise=randomize_noise, noise=self._noise_rows(noise, T, slice(t0, t1)),
                                           out="rgb24")
                    pieces.put(t0, rgb)
            finally:
                pieces.finish()
        return pieces.result()

    def _render_streams_jpeg(self, streams, motion_codes, flame_model, counts, firsts, order, randomize_noise, noise, host, jpeg):
        streams = list(streams)
        m = motion_codes
        if not isinstance(m, torch.Tensor) or m.dim() != 3 or m.shape[2] < MOTION_DIM or m.shape[0] != len(streams):
            raise ValueError(f"motion_codes must be a ({len(streams)}, R, {MOTION_DIM}) tensor: one block of rows per listed stream")
        m = self._device_motion(m, dense=True)
        n, R = int(m.shape[0]), int(m.shape[1])
        counts = [R] * n if counts is None else [int(c) for c in counts]
        firsts = [0] * n if firsts is None else [int(f) for f in firsts]
        if len(counts) != n or len(firsts) != n:
            raise ValueError(f"counts and firsts must hold {n} entries each")
        rows, which, ks = self.plan_frames(counts, order, firsts, R)
        if any(f + c > R for f, c in zip(firsts, counts)):
            raise ValueError(f"a stream's rows firsts[i] .. firsts[i] + counts[i] must lie within its {R} rows")
        T = len(rows)
        index = torch.tensor([which, ks], dtype=torch.int64).t().contiguous().reshape(T, 2)
        with torch.cuda.device(m.device):
            pieces = _JpegPieces(T, self.image_size, m.device, jpeg, host)
            # a call over no frames checks the streams, reserves the pool and uploads the avatars: the slab in force is the pool's after it
            self.render_streams(streams, m, flame_model, counts=[0] * n, firsts=firsts, order=order, out="rgb24")
            slab = max(1, int(self.stream_slab_in_force()))
            try:
                for t0 in range(0, T, slab):
                    t1 = min(T, t0 + slab)
                    # the piece's frames of stream i are consecutive: k_lo[i] .. k_lo[i] + c[i] - 1
                    c, k_lo = [0] * n, [0] * n
                    for t in range(t0, t1):
                        if c[which[t]] == 0:
                            k_lo[which[t]] = ks[t]
                        c[which[t]] += 1
                    place = {(which[t], ks[t]): t - t0 for t in range(t0, t1)}
                    _, sub_which, sub_ks = self.plan_frames(c, order)
                    # frame q of the piece's own call is frame to[q] of the piece in this call's order
                    to = [place[(i, k_lo[i] + k)] for i, k in zip(sub_which, sub_ks)]
                    straight = to == list(range(t1 - t0))
                    to_dev = None if straight else torch.tensor(to, dtype=torch.int64, device=m.device)
                    sub_noise = self._noise_rows(noise, T, slice(t0, t1) if straight else to_dev + t0)
                    rgb, _ = self.render_streams(streams, m, flame_model, counts=c, firsts=[f + k for f, k in zip(firsts, k_lo)], order=order,
                                                 randomize_noise=randomize_noise, noise=sub_noise, out="rgb24")
                    if not straight:
                        rgb = torch.empty_like(rgb).index_copy_(0, to_dev, rgb)
                    pieces.put(t0, rgb)
            finally:
                pieces.finish()
        return pieces.result(), index
