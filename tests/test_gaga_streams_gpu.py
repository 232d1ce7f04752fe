"""Live streams through the GAGAvatar head (GAGAvatar.open_stream / render_streams, ARTAvatarInferEngine.stream_render) on the small head
of tests/gaga_cases.py (S = 16, 64 vertices, 136 Gaussians, 8 forehead vertices, slabs of 2).

The definition: a frame of ``render_streams`` is the frame a fresh single-avatar head of the stream's own returns from ``render_clip`` over
that stream's frames in sequence.  ``render_clip`` is held to the chain of public pieces in tests/test_gaga_gpu.py and is bit-identical
for any split of its frames; every kernel between the two paths either moves fp32 values or repeats the same arithmetic, so the comparison
is exact: bit for bit."""
import ctypes as C

import pytest
import torch

import gaga_cases as gc
from artalk_amd import capi
from artalk_amd import frames as fr
from artalk_amd import gaga
from artalk_amd import styleunet as su
from test_gaga_gpu import Rig, _bits

pytestmark = pytest.mark.gpu

AVATAR_OF = ("a", "b", "a")                  # three streams; the third shares its avatar with the first
STEPS = ((5, 0, 3), (1, 4, 2))               # frames per stream in step 1 and step 2
ROWS = 6                                     # rows per stream and step in the motion array (more than any count)


def _head(rig, avatars=None, slab=gc.SLAB):
    """A head of its own (library object, EMA states, pool) on the rig's upsampler and watermark."""
    head = gaga.GAGAvatar(avatars or rig.avatars, rig.unet, water_mark=rig.mark, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
    head.set_slab(slab)
    return head


def _alone(rig, avatar, codes, noise=None, avatars=None):
    """codes (T, 106) through a fresh single-avatar head's render_clip."""
    head = _head(rig, avatars)
    head.set_avatar_id(avatar)
    return head.render_clip(codes, rig.flame, randomize_noise=False, noise=noise).cpu()


def _noise(T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(T, 1, su.noise_resolution(i), su.noise_resolution(i), device="cuda", generator=g) for i in range(su.num_noise_layers(gc.S))]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    r.avatars["c"] = gc.avatar(seed=4)
    # the codes of both steps, (step, stream, row, 106), and per stream its frames of both steps in sequence
    r.steps = gc.motion_codes(T=2 * 3 * ROWS, seed=23).reshape(2, 3, ROWS, 106).cuda()
    r.own = [torch.cat([r.steps[s, i, :STEPS[s][i]] for s in range(2)]) for i in range(3)]
    r.alone = [_alone(r, AVATAR_OF[i], r.own[i]) for i in range(3)]      # computed once, shared, read only
    r.noise = [_noise(r.own[i].shape[0], 40 + i) for i in range(3)]
    r.alone_noise = [_alone(r, AVATAR_OF[i], r.own[i], noise=r.noise[i]) for i in range(3)]
    return r


def _two_steps(rig, head, order, noise=False):
    """Both steps through render_streams -> every frame with its (stream, frame number in the stream's own sequence)."""
    streams = [head.open_stream(a) for a in AVATAR_OF]
    got, base = [], [0, 0, 0]
    for s, counts in enumerate(STEPS):
        kw = dict(randomize_noise=False)
        if noise:      # the streams' own per-frame noise, permuted into the call's order
            _, which, ks = gaga.GAGAvatar.plan_frames(counts, order)
            kw["noise"] = [torch.stack([rig.noise[i][l][base[i] + k] for i, k in zip(which, ks)]) for l in range(su.num_noise_layers(gc.S))]
        images, index = head.render_streams(streams, rig.steps[s], rig.flame, counts=counts, order=order, **kw)
        assert images.shape == (sum(counts), 3, gc.S, gc.S) and images.is_cuda
        assert index.shape == (sum(counts), 2) and index.dtype == torch.int64 and not index.is_cuda
        assert index.tolist() == [list(p) for p in zip(*gaga.GAGAvatar.plan_frames(counts, order)[1:])]
        got += [(int(i), base[int(i)] + int(k), images[t].cpu()) for t, (i, k) in enumerate(index.tolist())]
        base = [b + c for b, c in zip(base, counts)]
    for st in streams:
        st.close()
    return got


@pytest.mark.parametrize("slab", (1, 2, 5))
@pytest.mark.parametrize("order", ("time", "stream"))
def test_every_frame_is_the_frame_of_a_head_of_its_own(rig, order, slab):
    got = _two_steps(rig, _head(rig, slab=slab), order)
    assert len(got) == sum(map(sum, STEPS))
    for i, k, image in got:
        assert torch.equal(_bits(image), _bits(rig.alone[i][k])), f"stream {i}, its frame {k} ({order}, slabs of {slab})"


@pytest.mark.parametrize("order", ("time", "stream"))
def test_per_frame_noise_follows_the_index(rig, order):
    got = _two_steps(rig, _head(rig), order, noise=True)
    for i, k, image in got:
        assert torch.equal(_bits(image), _bits(rig.alone_noise[i][k])), f"stream {i}, its frame {k} ({order})"
    assert not torch.equal(rig.alone_noise[0], rig.alone[0])      # the noise is live


def test_one_classic_head_mixes_the_streams(rig):
    """The control: the same frames piece by piece through one classic head (set_avatar_id + render_clip).  Stream 2 shares avatar a with
    stream 0, whose last EMA state smooths stream 2's first frame: the wrong frame live streams remove."""
    head = _head(rig)
    pieces = {}
    for i in (0, 2):
        head.set_avatar_id(AVATAR_OF[i])
        pieces[i] = head.render_clip(rig.steps[0, i, :STEPS[0][i]], rig.flame, randomize_noise=False).cpu()
    assert torch.equal(_bits(pieces[0]), _bits(rig.alone[0][:STEPS[0][0]]))          # the first stream of the head is still right
    assert not torch.equal(_bits(pieces[2][0]), _bits(rig.alone[2][0])), "the control shows no difference: change the code seeds"


def test_reset_reopen_and_set_avatar(rig):
    head = _head(rig)
    codes = rig.own[0]
    st = head.open_stream("a")
    render = lambda s, c: head.render_streams([s], c[None], rig.flame, randomize_noise=False)[0].cpu()
    assert torch.equal(_bits(render(st, codes)), _bits(rig.alone[0]))
    assert not torch.equal(_bits(render(st, codes)), _bits(rig.alone[0])), "the EMA carries across calls"
    st.reset()
    assert torch.equal(_bits(render(st, codes)), _bits(rig.alone[0])), "reset starts the stream as a fresh head does"
    first = st.id
    st.close()
    assert st.closed
    st = head.open_stream("a")
    assert st.id != first
    assert torch.equal(_bits(render(st, codes)), _bits(rig.alone[0])), "a reopened stream starts as a fresh head does"
    # set_avatar keeps the EMA, as the classic head's set_avatar_id does (tests/test_gaga_gpu.py holds that one to the chain)
    st.reset()
    a = render(st, codes[:2])
    st.set_avatar("b")
    b = render(st, codes[2:])
    classic = _head(rig)
    classic.set_avatar_id("a")
    want_a = classic.render_clip(codes[:2], rig.flame, randomize_noise=False).cpu()
    classic.set_avatar_id("b")
    want_b = classic.render_clip(codes[2:], rig.flame, randomize_noise=False).cpu()
    assert torch.equal(_bits(a), _bits(want_a)) and torch.equal(_bits(b), _bits(want_b))
    assert not torch.equal(_bits(b), _bits(_alone(rig, "b", codes[2:]))), "the state was reset"
    with pytest.raises(KeyError):
        st.set_avatar("nobody.jpg")


def test_add_avatar_of_a_resident_name(rig):
    head, classic = _head(rig, dict(rig.avatars)), _head(rig, dict(rig.avatars))
    codes = rig.own[0]
    st = head.open_stream("a")
    classic.set_avatar_id("a")
    for part, new in ((codes[:2], None), (codes[2:4], rig.avatars["c"]), (codes[4:], None)):
        if new is not None:
            head.add_avatar("a", new)
            classic.add_avatar("a", new)
        got = head.render_streams([st], part[None], rig.flame, randomize_noise=False)[0].cpu()
        assert torch.equal(_bits(got), _bits(classic.render_clip(part, rig.flame, randomize_noise=False).cpu()))
    assert not torch.equal(_bits(got), _bits(rig.alone[0][4:])), "the new Gaussians are drawn"


def test_pool_capacity_and_eviction(rig):
    head = _head(rig).set_resident(2)
    codes = rig.own[0]
    sa, sb, sc = head.open_stream("a"), head.open_stream("b"), head.open_stream("c")
    with pytest.raises(RuntimeError, match="3 distinct avatars.*2 resident"):
        head.render_streams([sa, sb], codes[None].expand(2, -1, -1), rig.flame, randomize_noise=False)
    sc.close()
    images, index = head.render_streams([sa, sb], torch.stack([codes, codes]), rig.flame, order="stream", randomize_noise=False)
    assert torch.equal(_bits(images[:6].cpu()), _bits(rig.alone[0])) and torch.equal(_bits(images[6:].cpu()), _bits(_alone(rig, "b", codes)))
    assert sorted(head._slot_of) == ["a", "b"]
    # room is needed: b, which no open stream names, leaves; the frames are those of a head that never evicted
    sb.close()
    sc = head.open_stream("c")
    images, _ = head.render_streams([sc], codes[None], rig.flame, randomize_noise=False)
    assert sorted(head._slot_of) == ["a", "c"]
    assert torch.equal(_bits(images.cpu()), _bits(_alone(rig, "c", codes)))
    sa.reset()
    assert torch.equal(_bits(head.render_streams([sa], codes[None], rig.flame, randomize_noise=False)[0].cpu()), _bits(rig.alone[0]))


def test_the_classic_path_and_the_streams_do_not_meet(rig):
    head = _head(rig)
    codes = rig.own[0]
    st = head.open_stream("a")
    render = lambda c: head.render_streams([st], c[None], rig.flame, randomize_noise=False)[0].cpu()
    first = render(codes[:3])
    head.set_avatar_id("a")
    classic = head.render_clip(codes, rig.flame, randomize_noise=False).cpu()      # between two stream calls
    second = render(codes[3:])
    assert torch.equal(_bits(classic), _bits(rig.alone[0])), "the classic call saw the stream's state"
    assert torch.equal(_bits(torch.cat([first, second])), _bits(rig.alone[0])), "the classic call disturbed the stream's state"
    again = head.render_clip(codes, rig.flame, randomize_noise=False).cpu()        # the classic state carried over the stream call
    want = _head(rig)
    want.set_avatar_id("a")
    want.render_clip(codes, rig.flame, randomize_noise=False)
    assert torch.equal(_bits(again), _bits(want.render_clip(codes, rig.flame, randomize_noise=False).cpu()))


@pytest.mark.parametrize("out", ("rgb24", "yuv420p"))
def test_eight_bit_frames(rig, out):
    head = _head(rig)
    streams = [head.open_stream(a) for a in AVATAR_OF]
    counts = STEPS[0]

    def render(**kw):
        for st in streams:
            st.reset()
        return head.render_streams(streams, rig.steps[0], rig.flame, counts=counts, randomize_noise=False, **kw)

    images, index = render()
    want = fr.pack_frames(images, out).cpu()
    dev, index_dev = render(out=out)
    assert dev.is_cuda and dev.dtype == torch.uint8 and dev.shape == fr.frame_shape(out, sum(counts), gc.S, gc.S)
    assert torch.equal(dev.cpu(), want) and torch.equal(index_dev, index)
    host, _ = render(out=out, host=True)
    assert not host.is_cuda and host.is_pinned() and torch.equal(host, want)
    # a caller's own pinned buffer is filled and handed back; anything that is not that buffer is refused before a frame is rendered
    buf = torch.zeros(want.shape, dtype=torch.uint8, pin_memory=True)
    got, _ = render(out=out, host=True, host_buffer=buf)
    assert got is buf and torch.equal(buf, want)
    for bad, kw in ((torch.zeros(want.shape, dtype=torch.uint8), dict(out=out, host=True)),                      # not pinned
                    (torch.zeros(want[1:].shape, dtype=torch.uint8, pin_memory=True), dict(out=out, host=True)),   # a frame short
                    (torch.zeros(want.shape, dtype=torch.int8, pin_memory=True), dict(out=out, host=True)),
                    (buf, dict(out=out)), (buf, dict())):                                                          # without host=True
        with pytest.raises(ValueError, match="host_buffer"):
            render(host_buffer=bad, **kw)
    assert torch.equal(render(out=out, host=True)[0], want), "a refused call moved a stream's state"


def test_refusals_on_a_live_handle(rig):
    """artalk_gaga_pool_* and artalk_gaga_stream_* on a head's own library object after a render: every code with its message, and that a
    refused call changes nothing - a twin head that is never refused gives the same bits throughout."""
    L = capi.lib()
    codes = rig.own[0]
    other = [2, 5, 19, 33, 41, 47, 58, 62]      # eight other vertices: the same K

    def build():
        head = _head(rig).set_resident(2)
        streams = [head.open_stream("a"), head.open_stream("b")]
        return head, streams, lambda sts=streams: head.render_streams(sts, torch.stack([codes] * len(sts)), rig.flame, order="stream",
                                                                      randomize_noise=False)[0].cpu()

    head, (sa, sb), render = build()
    twin, _, twin_render = build()
    assert torch.equal(_bits(render()), _bits(twin_render()))      # the library object, a pool of 2 x 136, streams 0 and 1
    h, av, p = head._h, rig.avatars["a"], capi.ptr
    err = lambda: L.artalk_gaga_last_error(h)
    pool_set = lambda slot, N, xyz=av["xyz"]: L.artalk_gaga_pool_set(h, slot, N, p(xyz), p(av["colors"]), p(av["opacities"]), p(av["scales"]),
                                                                     p(av["rotations"]), p(av["shapecode"]), p(av["transform_matrix"]))
    assert pool_set(2, gc.N) == capi.EINVAL and b"slot 2 is outside the pool's [0, 2)" in err()
    assert pool_set(-1, gc.N) == capi.EINVAL and b"slot -1 is outside" in err()
    assert pool_set(0, gc.N - 1) == capi.EINVAL and b"N (135) is not the pool's 136" in err()
    assert pool_set(0, gc.V - 1) == capi.EINVAL and b"at least V" in err()
    assert pool_set(0, gc.N, None) == capi.EINVAL and b"must not be NULL" in err()
    assert L.artalk_gaga_pool_clear(h, 2) == capi.EINVAL and b"slot 2 is outside" in err()
    assert L.artalk_gaga_pool_clear(h, -1) == capi.EINVAL
    for fn in (L.artalk_gaga_stream_close, L.artalk_gaga_stream_reset):
        assert fn(h, 2) == capi.EINVAL and b"stream 2 was never opened" in err()
        assert fn(h, -1) == capi.EINVAL and b"stream -1 was never opened" in err()
    sid = C.c_int32(-1)
    assert L.artalk_gaga_stream_open(h, None) == capi.EINVAL and b"id is NULL" in err()
    assert L.artalk_gaga_stream_open(h, C.byref(sid)) == capi.OK and sid.value == 2
    assert L.artalk_gaga_stream_close(h, 2) == capi.OK
    assert L.artalk_gaga_stream_close(h, 2) == capi.EINVAL and b"stream 2 is closed" in err()
    assert L.artalk_gaga_stream_reset(h, 2) == capi.EINVAL and b"stream 2 is closed" in err()
    assert L.artalk_gaga_stream_open(h, C.byref(sid)) == capi.OK and sid.value == 3, "ids are never reused"
    assert L.artalk_gaga_stream_close(h, 3) == capi.OK
    # the two guards of the state rows and the pool while streams are open
    assert L.artalk_gaga_pool_reserve(h, 3, gc.N) == capi.ESTATE and b"while 2 streams are open" in err()
    assert L.artalk_gaga_pool_reserve(h, 0, gc.N) == capi.EINVAL and b"slots must be in 1..4096" in err()
    assert L.artalk_gaga_pool_reserve(h, 2, gc.V - 1) == capi.EINVAL and b"at least V" in err()
    three = (C.c_int32 * 3)(1, 2, 3)
    assert L.artalk_gaga_set_forehead(h, three, 3) == capi.ESTATE and b"K = 3 differs from the 8" in err()
    assert L.artalk_gaga_set_forehead(h, None, 0) == capi.ESTATE
    assert torch.equal(_bits(render()), _bits(twin_render())), "a refused call changed the pool or a stream's state"
    # the same K with other vertices is allowed and keeps the streams' states: their first frame is smoothed, a fresh stream's is not
    for hd in (head, twin):
        assert L.artalk_gaga_set_forehead(hd._h, (C.c_int32 * 8)(*other), 8) == capi.OK
    third = render()
    assert torch.equal(_bits(third), _bits(twin_render()))
    fresh = gaga.GAGAvatar(rig.avatars, rig.unet, water_mark=rig.mark, image_size=gc.S, n_dynamic=gc.V, forehead_indices=other)
    fresh.set_slab(gc.SLAB)
    unset = fresh.render_streams([fresh.open_stream("a")], codes[None], rig.flame, randomize_noise=False)[0].cpu()
    assert not torch.equal(_bits(third[0]), _bits(unset[0])), "the streams' states were dropped with the old vertices"
    # an emptied slot: a render that names it is refused before the device is touched, one that does not goes on
    slot_b = head._slot_of["b"]
    assert L.artalk_gaga_pool_clear(h, slot_b) == capi.OK and L.artalk_gaga_pool_clear(h, slot_b) == capi.OK
    with pytest.raises(ValueError, match=f"frame {codes.shape[0]}: slot {slot_b} is empty"):
        render()
    head._fresh.discard(slot_b)      # (the books learn of it: the next render uploads b again)
    assert torch.equal(_bits(render()), _bits(twin_render())), "the refused render moved stream a's state"
    # without open streams the pool may be reserved again
    sa.close(), sb.close()
    assert L.artalk_gaga_pool_reserve(h, 3, gc.N) == capi.OK
    assert L.artalk_gaga_set_forehead(h, three, 3) == capi.OK


def test_resident_avatars_share_n(rig):
    avatars = {"a": rig.avatars["a"], "d": gc.avatar(seed=6, n=gc.N + 4)}
    head = _head(rig, avatars)
    streams = [head.open_stream("a"), head.open_stream("d")]
    with pytest.raises(ValueError, match=r"avatar 'd'.*N \(140\) is not the pool's 136"):
        head.render_streams(streams, torch.stack([rig.own[0]] * 2), rig.flame, randomize_noise=False)
    assert torch.equal(_bits(head.render_streams(streams[:1], rig.own[0][None], rig.flame, randomize_noise=False)[0]), _bits(rig.alone[0]))


def test_engine_stream_render(rig):
    """open_stream(shape_id=) -> stream_step(smooth=True) -> stream_render equals render_streams on the same codes; the index carries
    absolute frame numbers; stream_flush's 4 frames render as the stream's last."""
    from conftest import get_gpu_model
    from artalk_amd.engine import ARTAvatarInferEngine
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    head = _head(rig, slab=0)
    eng = ARTAvatarInferEngine(model=m, gaga=head, gaga_flame=rig.flame)
    m.set_precision("f32")
    try:
        audio = torch.from_numpy(synth_audio(7, 4.0))[:64000]
        plain = eng.open_stream()
        sessions = [eng.open_stream(shape_id="a"), eng.open_stream(shape_id="b")]
        with pytest.raises(KeyError):
            eng.open_stream(shape_id="nobody.jpg")
        codes, spans = eng.stream_step(sessions, torch.stack([audio, audio.flip(0)]).cuda(), smooth=True)
        assert [c for _, c in spans] == [96, 96]
        torch.manual_seed(8)      # (the engine draws the StyleGAN noise, as rendering() does)
        images, index = eng.stream_render(sessions, codes, spans)
        assert images.shape == (192, 3, gc.S, gc.S)
        assert index[:4].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]] and index[-1].tolist() == [1, 95]
        tail, tail_spans = eng.stream_flush(sessions[:1])
        assert tail_spans == [(96, 4)]
        torch.manual_seed(9)
        last, last_index = eng.stream_render(sessions[:1], tail, tail_spans, output="rgb24")
        assert last_index.tolist() == [[0, 96 + k] for k in range(4)]
        with pytest.raises(ValueError, match="without shape_id"):
            eng.stream_render([plain], codes[:1], spans[:1])
        # the same codes through render_streams on streams of their own
        twins = [head.open_stream("a"), head.open_stream("b")]
        torch.manual_seed(8)
        want, want_index = head.render_streams(twins, codes, rig.flame, counts=[96, 96])
        torch.manual_seed(9)
        want_last, _ = head.render_streams(twins[:1], tail, rig.flame, out="rgb24")
        assert torch.equal(_bits(images), _bits(want)) and torch.equal(index, want_index)      # (first = 0: absolute = k)
        assert last.dtype == torch.uint8 and torch.equal(last.cpu(), want_last.cpu())
        assert not torch.equal(last[0].cpu(), fr.pack_frames(images[:1], "rgb24")[0].cpu())
        for st in sessions:
            eng.close_stream(st)
        assert all(st.closed for st in sessions) and len(head._streams) == 2
        plain.close()
    finally:
        m.close_sessions(list(m._sessions.values()))
        m.stream_end()
