"""The kernels live streams add to the GAGAvatar head, one launch each (artalk_op_gaga_forehead_streams / _flame_inputs_sets / _means_sets)
and the rasteriser's pool form (artalk_splat_render_sets).  All of them move fp32 values or repeat arithmetic an existing kernel does, so
every comparison is exact: bit-equal to the torch CPU statement of tests/gaga_ref.py, or to the existing entry point frame by frame."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gaga_cases as gc
import gaga_ref as ref
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import splat

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7.25e9
I32 = dict(dtype=torch.int32, device="cuda")


def _guarded(n, fill=float("nan")):
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf


def _take(buf, n, what):
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), f"the kernel wrote outside {what}"
    return whole[GUARD:GUARD + n]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- forehead_streams
ROWS = 5                       # rows of the state pool; row 0 and row 4 are NaN guard rows no stream may touch
POOL_ROW = (3, 1, 2)           # stream e's row: neither in order nor adjacent to its neighbours' the way e is
COUNTS = (0, 1, 2, 7, 8, 9, 17)      # 8, 9, 17: one full group of the kernel's eight frames ahead, one more frame, two groups and one


def _slab(counts, major):
    """-> per stream the list of its frame indices within a slab of sum(counts) frames, time-major (frame k of every stream that still
    has one, then k + 1) or stream-major."""
    lists = [[] for _ in counts]
    if major == "time":
        order = [i for k in range(max(counts)) for i, c in enumerate(counts) if k < c]
    else:
        order = [i for i, c in enumerate(counts) for _ in range(c)]
    for f, i in enumerate(order):
        lists[i].append(f)
    return lists


def _launch(verts, index_dev, K, lists, rows, state, flags):
    off = list(itertools.accumulate([0] + [len(l) for l in lists]))
    frames = [f for l in lists for f in l] or [0]
    V = verts.shape[1]
    d_rows, d_off, d_frames = torch.tensor(rows or [0], **I32), torch.tensor(off, **I32), torch.tensor(frames, **I32)      # (alive until the wait)
    rc = capi.lib().artalk_op_gaga_forehead_streams(capi.ptr(verts), capi.ptr(index_dev), K, V, len(lists), capi.ptr(d_rows), capi.ptr(d_off),
                                                    capi.ptr(d_frames), capi.ptr(state), capi.ptr(flags), capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()


def _forehead_case(K, counts, major, presets, seed):
    """One launch over len(counts) streams -> (got verts, want verts, got state pool, want state pool, got flags, want flags, inputs)."""
    V, T = 97, max(sum(counts), 1)
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(T, V, 3, generator=g)
    index = torch.randperm(V, generator=g)[:K].to(torch.int32)
    pool0 = torch.randn(ROWS, K, 3, generator=g)
    pool0[0], pool0[ROWS - 1] = float("nan"), float("nan")
    lists = _slab(counts, major)
    rows = list(POOL_ROW[:len(counts)])
    flags_in = torch.tensor([-12345, 0, 0, 0, -12345], dtype=torch.int32)
    for e, r in enumerate(rows):
        flags_in[r] = 1 if presets[e] else 0
    want, want_pool, want_flags = verts.clone(), pool0.clone(), flags_in.clone()
    for e, (l, r) in enumerate(zip(lists, rows)):
        if not l:
            continue      # a stream without frames keeps state and flag
        sub, st = ref.ema_torch(verts[l], index.long(), pool0[r][None].clone() if presets[e] else None)
        want[l] = sub
        want_pool[r] = st[0]
        want_flags[r] = 1
    vbuf = _guarded(T * V * 3)
    vbuf[GUARD:GUARD + T * V * 3] = verts.reshape(-1).cuda()
    sbuf = _guarded(ROWS * K * 3)
    sbuf[GUARD:GUARD + ROWS * K * 3] = pool0.reshape(-1).cuda()
    fdev = flags_in.cuda()
    _launch(vbuf[GUARD:GUARD + T * V * 3].view(T, V, 3), index.cuda(), K, lists, rows, sbuf[GUARD:], fdev)
    got = _take(vbuf, T * V * 3, "the vertices").view(T, V, 3)
    got_pool = _take(sbuf, ROWS * K * 3, "the state pool").view(ROWS, K, 3)
    return got, want, got_pool, want_pool, fdev.cpu(), want_flags, (verts, index, lists, rows, pool0, flags_in)


FOREHEAD_CASES = [(K, counts, major)
                  for K in (1, 8, 68, 90)
                  for counts in ((7,), (0,), (2, 7), (1, 0), (7, 1, 2), (0, 2, 0), (7, 7, 7))
                  for major in ("time", "stream")]
# the edges of the kernel's groups of eight frames; appended, so that the cases above keep their ids
FOREHEAD_CASES += [(K, counts, major)
                   for K in (1, 8, 68, 90)
                   for counts in ((8,), (9, 1), (17, 8, 2))
                   for major in ("time", "stream")]


@pytest.mark.parametrize("K,counts,major", FOREHEAD_CASES)
def test_forehead_streams(K, counts, major):
    assert all(c in COUNTS for c in counts)
    n = len(counts)
    for presets in {(False,) * n, (True,) * n, tuple(e % 2 == 0 for e in range(n)), tuple(e % 2 == 1 for e in range(n))}:
        got, want, got_pool, want_pool, got_flags, want_flags, (verts, index, lists, rows, pool0, flags_in) = _forehead_case(
            K, counts, major, presets, seed=1000 * K + 10 * sum(counts) + n)
        assert torch.equal(_bits(got), _bits(want)), f"presets {presets}: not bit-equal to the torch float32 loop per stream"
        # rows of streams not listed and the NaN guard rows are untouched; a listed stream's row is its final state
        assert torch.equal(_bits(got_pool), _bits(want_pool)), f"presets {presets}: the state pool"
        assert got_flags.tolist() == want_flags.tolist(), f"presets {presets}: the flags"
        for e, l in enumerate(lists):
            if not l:
                assert torch.equal(_bits(got_pool[rows[e]]), _bits(pool0[rows[e]])) and int(got_flags[rows[e]]) == int(flags_in[rows[e]])
            elif not presets[e]:
                assert torch.equal(_bits(got[l[0]]), _bits(verts[l[0]])), "a stream's very first frame is left as it is"
        rest = torch.ones(verts.shape[1], dtype=torch.bool)
        rest[index.long()] = False
        assert torch.equal(_bits(got[:, rest]), _bits(verts[:, rest])), "a vertex that is not listed changed"


def test_forehead_streams_excludes_an_fma():
    """The yardstick tells a contracted a * s + b * cur apart: on these inputs the FMA variant differs from what the kernel gives."""
    K, counts = 68, (7, 7, 7)
    got, want, _, _, _, _, (verts, index, lists, rows, pool0, _) = _forehead_case(K, counts, "time", (True, False, True), seed=77)
    assert torch.equal(_bits(got), _bits(want))
    differs = False
    for e, l in enumerate(lists):
        pts, _ = ref.ema_fma_numpy(verts[l][:, index.long()].numpy(), pool0[rows[e]].numpy() if e != 1 else None)
        differs = differs or not np.array_equal(pts, got[l][:, index.long()].numpy())
    assert differs, "an FMA would not be seen on this case"


@pytest.mark.parametrize("major", ("time", "stream"))
def test_forehead_streams_split_launches(major):
    """Three launches that split a slab of 16 frames (3 streams of 7, 2 and 7) equal one launch, states and flags included."""
    V, K, counts = 97, 90, (7, 2, 7)
    g = torch.Generator().manual_seed(31)
    T = sum(counts)
    verts = torch.randn(T, V, 3, generator=g)
    index = torch.randperm(V, generator=g)[:K].to(torch.int32).cuda()
    pool0 = torch.randn(ROWS, K, 3, generator=g)
    lists, rows = _slab(counts, major), list(POOL_ROW)

    def run(cuts):
        v, state = verts.cuda().clone(), pool0.cuda().clone()
        flags = torch.tensor([0, 1, 0, 0, 0], **I32)      # row 1 (stream 1) preset, rows 3 and 2 unset
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = [[f for f in l if lo <= f < hi] for l in lists]
            keep = [e for e, l in enumerate(part) if l]      # a launch lists the streams present in its part
            _launch(v, index, K, [part[e] for e in keep], [rows[e] for e in keep], state, flags)
        return v.cpu(), state.cpu(), flags.cpu()

    one, three = run([0, T]), run([0, 5, 6, T])
    for a, b in zip(one, three):
        assert torch.equal(_bits(a), _bits(b))
    assert one[2].tolist() == [0, 1, 1, 1, 0] and not torch.equal(one[0], verts)


@pytest.mark.parametrize("major,cut", (("stream", 5), ("time", 10)))
def test_forehead_streams_split_inside_a_group_of_eight(major, cut):
    """Streams of 17 and 9 frames in two launches cut after the first stream's fifth frame - 17 as 5 + 12, neither part a multiple of the
    eight frames the kernel loads ahead - equal one launch and the torch loop per stream, states and flags included."""
    V, K, counts = 97, 90, (17, 9)
    g = torch.Generator().manual_seed(43)
    T = sum(counts)
    verts = torch.randn(T, V, 3, generator=g)
    index = torch.randperm(V, generator=g)[:K].to(torch.int32)
    pool0 = torch.randn(ROWS, K, 3, generator=g)
    lists, rows = _slab(counts, major), list(POOL_ROW[:2])      # rows 3 (unset) and 1 (preset)
    assert [sum(f < cut for f in l) for l in lists] == ([5, 0] if major == "stream" else [5, 5])

    def run(cuts):
        v, state = verts.cuda().clone(), pool0.cuda().clone()
        flags = torch.tensor([0, 1, 0, 0, 0], **I32)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = [[f for f in l if lo <= f < hi] for l in lists]
            keep = [e for e, l in enumerate(part) if l]
            _launch(v, index.cuda(), K, [part[e] for e in keep], [rows[e] for e in keep], state, flags)
        return v.cpu(), state.cpu(), flags.cpu()

    one, two = run([0, T]), run([0, cut, T])
    want, want_pool = verts.clone(), pool0.clone()
    for l, r, preset in zip(lists, rows, (False, True)):
        want[l], st = ref.ema_torch(verts[l], index.long(), pool0[r][None].clone() if preset else None)
        want_pool[r] = st[0]
    for got in (one, two):
        assert torch.equal(_bits(got[0]), _bits(want)) and torch.equal(_bits(got[1]), _bits(want_pool))
        assert got[2].tolist() == [0, 1, 0, 1, 0]


def test_forehead_streams_without_work_is_a_no_op():
    verts = torch.randn(3, 11, 3).cuda()
    before = verts.clone()
    state, flags = torch.zeros(2, 3, device="cuda"), torch.zeros(2, **I32)
    _launch(verts, None, 0, [[0, 1]], [1], state, flags)
    _launch(verts, torch.tensor([4], **I32), 1, [], [], state, flags)
    assert torch.equal(verts, before) and flags.tolist() == [0, 0]


# ---- flame_inputs_sets, means_sets
SETS_CASES = [(stride, NB, slots) for stride, NB in ((106, 100), (131, 400), (112, 100), (106, 400)) for slots in (2, 3)]


@pytest.mark.parametrize("stride,NB,slots", SETS_CASES)
def test_flame_inputs_sets(stride, NB, slots):
    R, NS = 9, NB - 100
    g = torch.Generator().manual_seed(stride + NB + slots)
    motion = torch.randn(R, stride, generator=g)
    pool = torch.randn(slots, max(NS, 1), generator=g)[:, :NS]
    rows = torch.tensor([8, 0, 3, 3, 8, 1, 0])                     # out of order, repeated
    slot = torch.tensor([slots - 1, 0, 1, slots - 1, 0, 1, 1])
    T = int(rows.shape[0])
    m, p = motion.cuda(), (pool.contiguous().cuda() if NS else None)
    d_rows, d_slot = rows.cuda(), slot.to(torch.int32).cuda()
    betas, pose = _guarded(T * NB), _guarded(T * 15)
    rc = capi.lib().artalk_op_gaga_flame_inputs_sets(capi.ptr(m), stride, capi.ptr(d_rows), capi.ptr(d_slot), capi.ptr(p), NB, T,
                                                     capi.ptr(betas[GUARD:]), capi.ptr(pose[GUARD:]), capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    want_b = torch.cat([pool[slot], motion[rows, :100]], dim=1)
    want_p = torch.zeros(T, 15)
    want_p[:, 6:9] = motion[rows, 103:106]
    assert torch.equal(_bits(_take(betas, T * NB, "betas")), _bits(want_b.reshape(-1)))
    assert torch.equal(_bits(_take(pose, T * 15, "full_pose")), _bits(want_p.reshape(-1)))
    assert torch.equal(m.cpu(), motion)


@pytest.mark.parametrize("V,N,slots", [(64, 64, 2), (64, 136, 2), (64, 136, 3), (5, 300, 3)])
def test_means_sets(V, N, slots):
    g = torch.Generator().manual_seed(V + N + slots)
    slot = torch.tensor([slots - 1, 0, 1, 1, slots - 1])
    F = int(slot.shape[0])
    verts, pool = torch.randn(F, V, 3, generator=g), torch.randn(slots, N, 3, generator=g)
    pool[:, :V] = 1e6      # the dynamic rows of a resident avatar are never read (gc.avatar fills them the same way)
    out = _guarded(F * N * 3)
    d_verts, d_pool, d_slot = verts.cuda(), pool.cuda(), slot.to(torch.int32).cuda()
    rc = capi.lib().artalk_op_gaga_means_sets(capi.ptr(d_verts), capi.ptr(d_pool), capi.ptr(d_slot), capi.ptr(out[GUARD:]),
                                              F, V, N, capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    want = torch.cat([verts, pool[slot][:, V:]], dim=1)
    got = _take(out, F * N * 3, "means")
    assert torch.equal(_bits(got), _bits(want.reshape(-1)))
    assert not bool((got == 1e6).any()), "a dynamic xyz row was read"


# ---- artalk_splat_render_sets
def _splat_inputs():
    """Three attribute sets of the small head's size, five frames of means and cameras."""
    T, N = 5, gc.N
    avs = [gc.avatar(), gc.avatar(seed=3), gc.avatar(seed=4)]
    g = torch.Generator().manual_seed(12)
    means = torch.stack([torch.cat([0.5 * torch.randn(gc.V, 3, generator=g), avs[0]["xyz"][gc.V:]]) for _ in range(T)])
    codes = gc.motion_codes(T)[:, 100:103]
    view, proj, _ = gaga.camera_matrices(codes, avs[0]["transform_matrix"])
    return T, N, avs, means.cuda(), view.contiguous(), proj.contiguous()


def _render_sets(T, N, means, pools, set_strides, sets, view, proj):
    out = torch.full((T, 32, gc.S, gc.S), float("nan"), device="cuda")
    radii = torch.full((T, N), -1, **I32)
    L = capi.lib()
    h = splat._handle(torch.device("cuda", 0))
    arr = None if sets is None else (C.c_int32 * T)(*sets)
    col, opa, sca, rot = pools
    rc = L.artalk_splat_render_sets(h, N, T, gc.S, gc.S, capi.ptr(means), N * 3, capi.ptr(col), 0, capi.ptr(opa), 0, capi.ptr(sca), 0, capi.ptr(rot), 0,
                                    capi.ptr(view), capi.ptr(proj), T, 1.0 / 12.0, 1.0 / 12.0, 1.0, None, capi.ptr(out), capi.ptr(radii), arr, 3,
                                    0, *set_strides, capi.current_stream_ptr())
    assert rc == capi.OK, L.artalk_splat_last_error(h)
    torch.cuda.synchronize()
    return out.cpu(), radii.cpu()


def _render_one(N, means_t, av, view_t, proj_t):
    attr = splat._device_attr
    img, rad = splat._render(1, gc.S, gc.S, attr(means_t[None], "xyz", (3,), 1), attr(av["colors"].cuda()[None], "colors", (32,), 1),
                             attr(av["opacities"].cuda()[None], "opacities", (), 1), attr(av["scales"].cuda()[None], "scales", (3,), 1),
                             attr(av["rotations"].cuda()[None], "rotations", (4,), 1), view_t[None].contiguous(), proj_t[None].contiguous(),
                             1.0 / 12.0, 1.0 / 12.0, 1.0, None)
    return img[0].cpu(), rad[0].cpu()


def test_splat_render_sets():
    T, N, avs, means, view, proj = _splat_inputs()
    sets = (1, 0, 1, 2, 0)
    want = [_render_one(N, means[t], avs[sets[t]], view[t], proj[t]) for t in range(T)]
    want_img, want_rad = torch.stack([w[0] for w in want]), torch.stack([w[1] for w in want])
    assert float((want_img.abs().amax(dim=1) > 1e-3).float().mean()) > 0.25, "an empty image compares nothing"
    assert not torch.equal(want_img[0], _render_one(N, means[0], avs[0], view[0], proj[0])[0]), "the sets must differ in what they draw"

    def pool(key, width, pad=0):
        """The three sets one after the other, `pad` floats between two of them."""
        flat = torch.full((3 * (N * width + pad),), float("nan"))
        for k, av in enumerate(avs):
            flat[k * (N * width + pad):k * (N * width + pad) + N * width] = av[key].reshape(-1)
        return flat.cuda()

    aligned = (pool("colors", 32), pool("opacities", 1), pool("scales", 3), pool("rotations", 4))
    img, rad = _render_sets(T, N, means, aligned, (N * 32, N, N * 3, N * 4), sets, view, proj)
    assert torch.equal(_bits(img), _bits(want_img)) and torch.equal(rad, want_rad)
    # a colour set stride that is no multiple of 4 floats: sets 1 and 2 start off a 16-byte boundary, the pixels are the same
    odd = (pool("colors", 32, pad=3), pool("opacities", 1, pad=1), pool("scales", 3, pad=2), pool("rotations", 4, pad=1))
    img, rad = _render_sets(T, N, means, odd, (N * 32 + 3, N + 1, N * 3 + 2, N * 4 + 1), sets, view, proj)
    assert torch.equal(_bits(img), _bits(want_img)) and torch.equal(rad, want_rad)
    # without sets the call is artalk_splat_render: every frame from set 0
    img, rad = _render_sets(T, N, means, aligned, (N * 32, N, N * 3, N * 4), None, view, proj)
    attr = splat._device_attr
    av = avs[0]
    ref_img, ref_rad = splat._render(T, gc.S, gc.S, attr(means, "xyz", (3,), T), attr(av["colors"].cuda()[None], "colors", (32,), T),
                                     attr(av["opacities"].cuda()[None], "opacities", (), T), attr(av["scales"].cuda()[None], "scales", (3,), T),
                                     attr(av["rotations"].cuda()[None], "rotations", (4,), T), view, proj, 1.0 / 12.0, 1.0 / 12.0, 1.0, None)
    assert torch.equal(_bits(img), _bits(ref_img.cpu())) and torch.equal(rad, ref_rad.cpu())


def test_splat_render_sets_refusals():
    T, N, avs, means, view, proj = _splat_inputs()
    L, h = capi.lib(), splat._handle(torch.device("cuda", 0))
    out, radii = torch.empty(T, 32, gc.S, gc.S, device="cuda"), torch.empty(T, N, **I32)
    for sets, strides, word in (((0, 3, 0, 0, 0), (0, 0, 0, 0, 0), b"outside"), ((0, -1, 0, 0, 0), (0, 0, 0, 0, 0), b"outside"),
                                ((0, 0, 0, 0, 0), (0, -1, 0, 0, 0), b"set stride")):
        rc = L.artalk_splat_render_sets(h, N, T, gc.S, gc.S, capi.ptr(means), N * 3, capi.ptr(means), 0, capi.ptr(means), 0, capi.ptr(means), 0,
                                        capi.ptr(means), 0, capi.ptr(view), capi.ptr(proj), T, 1.0 / 12.0, 1.0 / 12.0, 1.0, None, capi.ptr(out),
                                        capi.ptr(radii), (C.c_int32 * T)(*sets), 3, *strides, capi.current_stream_ptr())
        assert rc == capi.EINVAL and word in L.artalk_splat_last_error(h)
