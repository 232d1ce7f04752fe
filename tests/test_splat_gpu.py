"""Gaussian splat rasteriser on the GPU (artalk_splat_*, artalk_amd.splat) against the numpy restatement of its definition
(tests/splat_ref.py, float64).  ``radii`` must be equal for every Gaussian: the case generator (tests/splat_cases.py) keeps every
preprocess decision away from its threshold.  Images are compared on unambiguous pixels only (alpha margin >= 1e-4, stop margin >=
1e-3, no two contributing depths within 4 float32 units); per pixel and channel the allowed error is
    4 x max(float32-numpy error of the case, 2^-23 (sum |alpha T colour| + T |bg|))
- the factor 4 is the mesh renderer's margin, the second term one float32 unit of what is summed.  Run with -s for shares and errors;
the measured figures per case are in DESIGN.md section 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from artalk_amd import capi
from splat_cases import (AMBIGUOUS_CAP, TABLE, all_culled, bg_ramp, case, case_refs, equal_depths, near_threshold, run_ref, share_and_yardstick,
                         swapped)
from splat_ref import NUM_CHANNELS

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ATTRS = (("means", 3), ("colors", NUM_CHANNELS), ("opacities", 1), ("scales", 3), ("rotations", 4))


def _abi(frames, shared=(), pad=0, prefill=None, n_cams=None, h=None):
    """artalk_splat_render over `frames` (cases of one N, H, W, scale modifier and background; the camera may differ per frame).
    ``shared``: attributes passed once with stride 0 (taken from frame 0).  ``pad``: guard words after out and radii.  Returns
    (images (T, 32, H, W), radii (T, N), whole out buffer, whole radii buffer) as numpy arrays."""
    L = capi.lib()
    own = h is None
    if own:
        h = C.c_void_p()
        assert L.artalk_splat_create(0, C.byref(h)) == capi.OK
    try:
        c0, T = frames[0], len(frames)
        N, H, W = c0["means"].shape[0], c0["H"], c0["W"]
        args = []
        keep = []
        for name, width in ATTRS:
            if name in shared:
                t, stride = torch.from_numpy(np.ascontiguousarray(c0[name])).cuda(), 0
            else:
                t, stride = torch.from_numpy(np.stack([c[name] for c in frames])).cuda(), N * width
            keep.append(t)
            args += [capi.ptr(t), stride]
        n_cams = n_cams or (1 if T == 1 or all(c["V"] is c0["V"] for c in frames) else T)
        view = torch.from_numpy(np.stack([c["V"] for c in frames[:n_cams]]).astype(np.float32)).contiguous()
        proj = torch.from_numpy(np.stack([c["P"] for c in frames[:n_cams]]).astype(np.float32)).contiguous()
        bg = None if c0["bg"] is None else torch.from_numpy(c0["bg"]).cuda()
        n_out, n_rad = T * NUM_CHANNELS * H * W, T * N
        out = torch.full((n_out + pad,), float("nan") if prefill is None else prefill, dtype=torch.float32, device="cuda")
        radii = torch.full((n_rad + pad,), -77, dtype=torch.int32, device="cuda")
        rc = L.artalk_splat_render(h, N, T, H, W, *args, capi.ptr(view), capi.ptr(proj), n_cams, c0["tanfovx"], c0["tanfovy"],
                                   c0["scale_modifier"], capi.ptr(bg), capi.ptr(out), capi.ptr(radii), capi.current_stream_ptr())
        assert rc == capi.OK, L.artalk_splat_last_error(h).decode()
        torch.cuda.synchronize()
        o, r = out.cpu().numpy(), radii.cpu().numpy()
        return o[:n_out].reshape(T, NUM_CHANNELS, H, W), r[:n_rad].reshape(T, N), o, r
    finally:
        if own:
            L.artalk_splat_destroy(h)


def _check(tag, img, radii, r64, r32, cap=AMBIGUOUS_CAP, **amb):
    """The comparison every case shares.  Returns (ambiguous share, kernel error, float32 numpy error)."""
    assert img.shape == r64["image"].shape and img.dtype == np.float32 and radii.dtype == np.int32
    assert not near_threshold(r64["pre"]).any(), f"{tag}: a Gaussian sits within rounding of a preprocess threshold"
    wrong = np.nonzero(radii != r64["radii"])[0]
    assert wrong.size == 0, f"{tag}: radii differ for Gaussians {wrong[:8].tolist()}: {radii[wrong[:8]].tolist()} vs {r64['radii'][wrong[:8]].tolist()}"
    assert np.isfinite(img).all(), f"{tag}: {int((~np.isfinite(img)).sum())} values were not written (or are not finite)"
    mask, share, yard = share_and_yardstick(r64, r32, **amb)
    ok = ~mask
    allowed = FACTOR * np.maximum(yard, 2.0 ** -23 * r64["mag"])
    err = np.abs(img.astype(np.float64) - r64["image"])
    worst = float(err[:, ok].max()) if ok.any() else 0.0
    ratio = float((err / allowed)[:, ok].max()) if ok.any() else 0.0
    print(f"{tag}: ambiguous share {share:.3%} of {mask.size} pixels, max-abs error kernel {worst:.3e} / float32 numpy {yard:.3e}, "
          f"largest error / allowed {ratio:.3f}")
    if cap is not None:
        assert share <= cap, f"{tag}: the ambiguity mask covers {share:.3%} of the pixels"
    assert ok.any()
    bad = (err > allowed) & ok[None]
    assert not bad.any(), (f"{tag}: {int(bad.sum())} values on unambiguous pixels beyond {FACTOR:g} x max(float32 numpy error {yard:.3e}, one "
                           f"float32 unit of the sum); worst {worst:.3e}, first {np.argwhere(bad)[:4].tolist()}")
    return share, worst, yard


@pytest.mark.parametrize("name", sorted(TABLE))
def test_against_float64(name):
    """40 x 56 and 33 x 17 with 300 and 1 500 Gaussians, N = 1 / 255 / 256 / 257, 600 Gaussians in one tile (three LDS batches), an opaque
    stack that stops early, one Gaussian over the whole image, culled Gaussians beside drawn ones, a background with a scale modifier, a
    turned camera with tanfovx != tanfovy."""
    c = case(name)
    r64, r32 = case_refs(name)
    img, radii, _, _ = _abi([c])
    _check(name, img[0], radii[0], r64, r32)
    if name == "culled_and_drawn":
        assert radii[0][:6].tolist() == [0] * 6 and (radii[0][6:] > 0).all()
    if name == "opaque_stack":
        assert (r64["stop_margin"] < np.inf).mean() > 0.2      # the stop test is made on a good part of the image


def test_all_culled_is_the_background_exactly():
    c = all_culled()
    img, radii, _, _ = _abi([c])
    assert (radii == 0).all()
    assert np.array_equal(img[0], np.broadcast_to(bg_ramp()[:, None, None], img[0].shape))
    # N = 0 writes the background too, for every frame, and with no background that is zero
    empty = dict(c, **{k: c[k][:0] for k, _ in ATTRS})
    img0, radii0, _, _ = _abi([empty, empty])
    assert radii0.shape == (2, 0) and np.array_equal(img0[1], img[0]) and np.array_equal(img0[0], img[0])
    assert (_abi([dict(empty, bg=None)])[0] == 0.0).all()


def test_equal_depths_lower_index_first():
    c = equal_depths()
    r64, r32 = run_ref(c), run_ref(c, dtype=np.float32)
    d = r64["pre"]["depth"].astype(np.float32)
    assert d[0] == d[1] and d[2] == d[3]
    assert (r64["depth_gap"] == 0).sum() > 50      # many pixels blend two Gaussians of one depth
    img, radii, _, _ = _abi([c])
    _check("equal depths", img[0], radii[0], r64, r32, depth_ulps=-1)      # ties are decided by index: nothing ambiguous about them
    s = swapped(c, 0, 1)
    img_s, radii_s, _, _ = _abi([s])
    _check("equal depths, swapped", img_s[0], radii_s[0], run_ref(s), run_ref(s, dtype=np.float32), depth_ulps=-1)
    assert np.abs(img_s[0] - img[0]).max() > 1e-2, "the order of two Gaussians of equal depth does not change the image"


def test_nan_prefill_and_guard_words():
    PAD = 4096
    frames = [case("n300_33x17"), case("n300_33x17")]
    img, radii, out, rad = _abi(frames, pad=PAD)      # out is pre-filled with NaN, radii with -77
    assert np.isfinite(img).all() and (radii >= 0).all()
    assert np.isnan(out[-PAD:]).all() and (rad[-PAD:] == -77).all(), "guard words written"
    r64, r32 = case_refs("n300_33x17")
    _check("guarded, frame 1", img[1], radii[1], r64, r32)
    # the same with the whole-image Gaussian: every tile of every frame is walked
    c = case("whole_image")
    img, radii, out, rad = _abi([c, c, c], pad=PAD)
    assert np.isfinite(img).all() and np.isnan(out[-PAD:]).all() and (rad[-PAD:] == -77).all()
    _check("guarded whole image, frame 2", img[2], radii[2], *case_refs("whole_image"))


def test_determinism_batching_and_sharing():
    a, b, c = case("n1500_40x56"), case("n300_40x56"), case("one_tile_600")
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_splat_create(0, C.byref(h)) == capi.OK
    try:
        first = _abi([a], h=h)
        again = _abi([a], h=h)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        # T = 3 with three cameras and per-frame attributes against three one-frame calls (frames of one N: a, a swapped, a turned)
        turned = dict(a, **{k: case("turned_camera")[k] for k in ("V", "P")})
        frames = [a, swapped(a, 3, 700), turned]
        whole = _abi(frames, h=h)
        for t, f in enumerate(frames):
            one = _abi([f], h=h)
            assert np.array_equal(whole[0][t], one[0][0]) and np.array_equal(whole[1][t], one[1][0]), t
        assert not np.array_equal(whole[0][0], whole[0][2])
        # a smaller and a differently shaped call on the same handle, then the first again: the buffers carry nothing over
        _abi([b], h=h)
        _abi([c], h=h)
        assert np.array_equal(_abi([a], h=h)[0], first[0])
        # shared (stride 0) against replicated attributes, per-frame means
        moved = dict(a, means=(a["means"] + np.float32(0.01)).astype(np.float32))
        rep = _abi([a, moved], h=h)
        shr = _abi([a, moved], shared=("colors", "opacities", "scales", "rotations"), h=h)
        assert np.array_equal(rep[0], shr[0]) and np.array_equal(rep[1], shr[1])
        assert not np.array_equal(rep[0][0], rep[0][1])
        all_shared = _abi([a, a], shared=tuple(k for k, _ in ATTRS), h=h)
        assert np.array_equal(all_shared[0][0], first[0][0]) and np.array_equal(all_shared[0][1], first[0][0])
    finally:
        L.artalk_splat_destroy(h)


def test_unaligned_colours_take_the_same_values():
    """A colour pointer that is not 16-byte aligned goes through the dword staging path: same bits."""
    c = case("n300_40x56")
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_splat_create(0, C.byref(h)) == capi.OK
    try:
        want = _abi([c], h=h)[0]
        N, H, W = c["means"].shape[0], c["H"], c["W"]
        dev = {k: torch.from_numpy(c[k]).cuda() for k, _ in ATTRS}
        store = torch.zeros(N * NUM_CHANNELS + 1, dtype=torch.float32, device="cuda")
        store[1:] = dev["colors"].reshape(-1)
        assert store[1:].data_ptr() % 16 == 4
        out = torch.full((NUM_CHANNELS, H, W), float("nan"), dtype=torch.float32, device="cuda")
        radii = torch.empty(N, dtype=torch.int32, device="cuda")
        view, proj = torch.from_numpy(c["V"]).contiguous(), torch.from_numpy(c["P"]).contiguous()
        rc = L.artalk_splat_render(h, N, 1, H, W, capi.ptr(dev["means"]), 0, capi.ptr(store[1:]), 0, capi.ptr(dev["opacities"]), 0,
                                   capi.ptr(dev["scales"]), 0, capi.ptr(dev["rotations"]), 0, capi.ptr(view), capi.ptr(proj), 1, c["tanfovx"],
                                   c["tanfovy"], 1.0, None, capi.ptr(out), capi.ptr(radii), capi.current_stream_ptr())
        assert rc == capi.OK, L.artalk_splat_last_error(h).decode()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0])
    finally:
        L.artalk_splat_destroy(h)


def test_rasterizer_and_render_gaussian_end_to_end():
    from artalk_amd.splat import GaussianRasterizationSettings, GaussianRasterizer, build_camera_matrices, render_gaussian
    c = case("turned_camera")
    focal_x, focal_y = 1.0 / c["tanfovx"], 1.0 / c["tanfovy"]
    cam = torch.from_numpy(c["cam_matrix"])[None]
    view, proj, pos = build_camera_matrices(cam, focal_x, focal_y)
    # the oracle on the matrices the Python layer hands over (float32 torch arithmetic; the case was drawn with float64 ones)
    o = dict(c, V=view[0].numpy(), P=proj[0].numpy())
    r64, r32 = run_ref(o), run_ref(o, dtype=np.float32)
    dev = {k: torch.from_numpy(c[k]).cuda() for k, _ in ATTRS}
    rs = GaussianRasterizationSettings(image_height=c["H"], image_width=c["W"], tanfovx=c["tanfovx"], tanfovy=c["tanfovy"],
                                       bg=torch.zeros(1, NUM_CHANNELS).cuda(), scale_modifier=1.0, viewmatrix=view[0].cuda(),
                                       projmatrix=proj[0].cuda(), sh_degree=0, campos=pos[0].cuda(), prefiltered=False, debug=False)
    colour, radii = GaussianRasterizer(raster_settings=rs)(
        means3D=dev["means"], means2D=torch.zeros_like(dev["means"]), shs=None, colors_precomp=dev["colors"],
        opacities=dev["opacities"][:, None], scales=dev["scales"], rotations=dev["rotations"], cov3D_precomp=None)
    assert colour.shape == (NUM_CHANNELS, c["H"], c["W"]) and colour.is_cuda and radii.shape == (300,) and radii.dtype == torch.int32
    _check("GaussianRasterizer", colour.cpu().numpy(), radii.cpu().numpy(), r64, r32)
    # render_gaussian: a batch of two, the second with moved points; the background's row 0 serves both frames
    moved = (c["means"] + np.float32(0.03)).astype(np.float32)      # (0.02 would put one Gaussian within 1e-4 of a radius step)
    gs = dict(xyz=torch.from_numpy(np.stack([c["means"], moved])).cuda(), colors=dev["colors"][None].repeat(2, 1, 1),
              opacities=dev["opacities"][None, :, None].repeat(2, 1, 1), scales=dev["scales"][None].repeat(2, 1, 1),
              rotations=dev["rotations"][None].repeat(2, 1, 1))
    bg = torch.stack([torch.from_numpy(bg_ramp()), torch.zeros(NUM_CHANNELS)]).cuda()
    res = render_gaussian(gs, cam.repeat(2, 1, 1).cuda(), dict(focal_x=focal_x, focal_y=focal_y, size=(c["H"], c["W"])), bg_color=bg)
    assert res["images"].shape == (2, NUM_CHANNELS, c["H"], c["W"]) and res["radii"].shape == (2, 300)
    assert res["viewspace_points"].shape == (2, 300, 3) and not res["viewspace_points"].any()
    for t, means in enumerate((c["means"], moved)):
        ot = dict(o, means=means, bg=bg_ramp())
        _check(f"render_gaussian frame {t}", res["images"][t].cpu().numpy(), res["radii"][t].cpu().numpy(), run_ref(ot),
               run_ref(ot, dtype=np.float32))
    # no background: the frame of the rasteriser call above, bit for bit
    plain = render_gaussian(gs, cam.repeat(2, 1, 1).cuda(), dict(focal_x=focal_x, focal_y=focal_y, size=(c["H"], c["W"])))
    assert torch.equal(plain["images"][0], colour) and torch.equal(plain["radii"][0], radii)
