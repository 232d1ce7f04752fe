"""Live streams through the GAGAvatar head, the parts that need no GPU: the frame planner against hand-written tables, the head's slot
books (nothing touches the device before the first render), and every refusal of the new entry points - on NULL handles directly, on
numbers through ``artalk_op_gaga_streams_check``, the host function ``artalk_gaga_render_streams`` itself calls."""
import ctypes as C

import pytest
import torch

import gaga_cases as gc
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import styleunet as su

NEW_SYMBOLS = ("artalk_splat_render_sets", "artalk_gaga_pool_reserve", "artalk_gaga_pool_set", "artalk_gaga_pool_clear", "artalk_gaga_stream_open",
               "artalk_gaga_stream_close", "artalk_gaga_stream_reset", "artalk_gaga_render_streams", "artalk_op_gaga_flame_inputs_sets",
               "artalk_op_gaga_forehead_streams", "artalk_op_gaga_means_sets", "artalk_op_gaga_streams_check", "artalk_gaga_streams_slab")


def test_new_symbols_are_exported():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS and hasattr(L, name), name


# ------------------------------------------------------------------------------------------------ plan_frames
def test_plan_frames_tables():
    plan = gaga.GAGAvatar.plan_frames
    # counts (3, 0, 2): stream 1 has nothing, stream 2 runs out after two frames
    assert plan((3, 0, 2)) == ([0, 0, 1, 1, 2], [0, 2, 0, 2, 0], [0, 0, 1, 1, 2])
    assert plan((3, 0, 2), order="stream") == ([0, 1, 2, 0, 1], [0, 0, 0, 2, 2], [0, 1, 2, 0, 1])
    # firsts move a stream's rows; rows_per_stream puts the streams' blocks one after the other
    assert plan((3, 0, 2), firsts=(4, 9, 1)) == ([4, 1, 5, 2, 6], [0, 2, 0, 2, 0], [0, 0, 1, 1, 2])
    assert plan((3, 0, 2), "time", (4, 9, 1), 104) == ([4, 209, 5, 210, 6], [0, 2, 0, 2, 0], [0, 0, 1, 1, 2])
    assert plan((3, 0, 2), "stream", (4, 9, 1), 104) == ([4, 5, 6, 209, 210], [0, 0, 0, 2, 2], [0, 1, 2, 0, 1])
    assert plan(()) == ([], [], []) and plan((0, 0)) == ([], [], [])
    with pytest.raises(ValueError, match="order"):
        plan((1,), order="frame")
    with pytest.raises(ValueError):
        plan((1, 2), firsts=(0,))
    with pytest.raises(ValueError):
        plan((1, -1))


# ------------------------------------------------------------------------------------------------ the head's books
def _head():
    return gaga.GAGAvatar({"a": gc.avatar(), "b": gc.avatar(seed=3), "c": gc.avatar(seed=4)}, su.synth_state_dict(gc.S),
                          water_mark=gc.water_mark(), image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)


def test_streams_and_slots_without_a_device():
    head = _head().set_resident(2)
    sa, sb = head.open_stream("a"), head.open_stream("b")
    assert (sa.id, sb.id) == (0, 1) and sa.avatar_id == "a" and not sa.closed
    with pytest.raises(KeyError):
        head.open_stream("nobody.jpg")
    with pytest.raises(RuntimeError, match="before the first open_stream"):
        head.set_resident(3)
    assert head._h is None, "the device is first touched by a render"
    assert head._plan_slots([sa, sb]) == [("a", 0), ("b", 1)] and head._slot_of == {"a": 0, "b": 1}
    head._fresh.update((0, 1))                                     # what a render does once the uploads went through
    assert head._plan_slots([sb, sa]) == []
    # a second stream on a resident avatar shares its slot
    sa2 = head.open_stream("a")
    assert sa2.id == 2 and head._plan_slots([sa2]) == [] and head._slot_of == {"a": 0, "b": 1}
    # add_avatar of a resident name: the slot is stale, the other is not
    head.add_avatar("a", gc.avatar(seed=5))
    assert head._plan_slots([sa, sb, sa2]) == [("a", 0)]
    head._fresh.add(0)
    # three distinct avatars among the open streams, two slots: both numbers are named, whichever streams are listed
    sc = head.open_stream("c")
    with pytest.raises(RuntimeError, match=r"3 distinct avatars.*2 resident"):
        head._plan_slots([sa])
    # b's last stream closes: its slot is reused because room is needed, and only then
    sb.close()
    assert sb.closed and head._slot_of == {"a": 0, "b": 1}
    assert head._plan_slots([sa]) == [] and head._slot_of == {"a": 0, "b": 1}
    assert head._plan_slots([sc, sa]) == [("c", 1)] and head._slot_of == {"a": 0, "c": 1}
    with pytest.raises(ValueError, match="closed"):
        sb.set_avatar("a")
    sb.close()                                                     # closing twice is harmless
    # set_avatar moves a stream to another avatar; ids are never reused
    sc.set_avatar("a")
    assert sc.avatar_id == "a" and head.open_stream("b").id == 4
    assert head._h is None


def test_render_streams_refusals_without_a_device():
    head = _head()
    sa, sb = head.open_stream("a"), head.open_stream("b")
    cpu = torch.zeros(2, 3, 106)
    with pytest.raises(ValueError, match="listed twice"):
        head.render_streams([sa, sa], cpu, None)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        head.render_streams([sa, sb], cpu, None)
    with pytest.raises(ValueError, match="host=True"):
        head.render_streams([sa, sb], cpu, None, host=True)
    with pytest.raises(ValueError):
        head.render_streams([sa, sb], cpu, None, out="bgr24")
    with pytest.raises(ValueError, match="one block of rows per listed stream"):
        head.render_streams([sa], cpu, None)
    with pytest.raises(ValueError, match="GagaStreams of this head"):
        head.render_streams([_head().open_stream("a"), sb], cpu, None)
    sb.close()
    with pytest.raises(ValueError, match="stream 1 is closed"):
        head.render_streams([sa, sb], cpu, None)
    assert head._h is None


def test_engine_stream_wiring_without_a_device():
    import types
    from artalk_amd.engine import ARTAvatarInferEngine
    opened = []
    session = lambda: types.SimpleNamespace(id=len(opened), closed=False, close=lambda: None)
    model = types.SimpleNamespace(cfg=None, open_session=lambda style: opened.append(style) or session())
    head = _head()
    eng = ARTAvatarInferEngine(model=model, gaga=head, gaga_flame=object())
    plain, live = eng.open_stream(), eng.open_stream(shape_id="b")
    assert len(head._streams) == 1 and eng._gaga_streams[live.id].avatar_id == "b"
    with pytest.raises(ValueError, match="without shape_id"):
        eng.stream_render([plain], torch.zeros(1, 4, 106), [(0, 4)])
    with pytest.raises(KeyError):
        eng.open_stream(shape_id="nobody.jpg")
    assert len(opened) == 2, "a refused shape_id opens no session"
    eng.close_stream(live)
    assert not head._streams and eng._gaga_streams == {}
    with pytest.raises(ValueError, match="without shape_id"):
        eng.stream_render([live], torch.zeros(1, 4, 106), [(0, 4)])


# ------------------------------------------------------------------------------------------------ refusals of the library
def _check(V=64, slots=2, N=136, T=3, stride=106, row=(0, 5, 1), stream=(0, 2, 0), slot=(1, 0, 1), open_=(1, 0, 1), filled=(1, 1), finalized=1,
           fmt=0, S=16):
    L = capi.lib()
    arr = lambda ty, v: None if v is None else (ty * max(len(v), 1))(*v)
    msg = C.create_string_buffer(256)
    rc = L.artalk_op_gaga_streams_check(V, slots, N, T, stride, arr(C.c_int64, row), arr(C.c_int32, stream), arr(C.c_int32, slot),
                                        arr(C.c_uint8, open_), len(open_ or ()), arr(C.c_uint8, filled), finalized, fmt, S, msg, 256)
    return rc, msg.value.decode()


def test_render_streams_refusals_are_host_checks():
    assert _check() == (capi.OK, "")
    assert _check(T=0, row=(), stream=(), slot=())[0] == capi.OK
    for kw, code, word in ((dict(row=None), capi.EINVAL, "must not be NULL"), (dict(stream=None), capi.EINVAL, "must not be NULL"),
                           (dict(slot=None), capi.EINVAL, "must not be NULL"), (dict(T=-1), capi.EINVAL, "T must not be negative"),
                           (dict(row=(0, -1, 1)), capi.EINVAL, "frame 1: motion row -1 is negative"),
                           (dict(stream=(0, 3, 0)), capi.EINVAL, "frame 1: stream 3 was never opened"),
                           (dict(stream=(0, -1, 0)), capi.EINVAL, "stream -1 was never opened"),
                           (dict(stream=(0, 2, 1)), capi.EINVAL, "frame 2: stream 1 is closed"),
                           (dict(slot=(1, 2, 1)), capi.EINVAL, "frame 1: slot 2 is outside the pool's [0, 2)"),
                           (dict(slot=(1, -1, 1)), capi.EINVAL, "slot -1 is outside"),
                           (dict(filled=(0, 1)), capi.EINVAL, "frame 1: slot 0 is empty"),
                           (dict(stride=105), capi.EINVAL, "at least 106"), (dict(finalized=0), capi.ESTATE, "not finalized"),
                           (dict(fmt=3), capi.EINVAL, "format"), (dict(fmt=capi.FRAMES_YUV420P, S=15), capi.EINVAL, "even H and W"),
                           (dict(slots=0), capi.EINVAL, "slots must be in 1..4096"), (dict(slots=4097), capi.EINVAL, "slots must be"),
                           (dict(N=63), capi.EINVAL, "at least V")):
        rc, msg = _check(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    assert _check(fmt=capi.FRAMES_YUV420P)[0] == capi.OK and _check(fmt=capi.FRAMES_RGB24, S=15)[0] == capi.OK


def test_capi_refusals_before_the_device_is_touched():
    L = capi.lib()
    p = C.c_void_p(4096)      # never dereferenced: every call below is refused
    sid = C.c_int32(7)
    for rc in (L.artalk_gaga_pool_reserve(None, 2, 136), L.artalk_gaga_pool_set(None, 0, 136, p, p, p, p, p, p, p), L.artalk_gaga_pool_clear(None, 0),
               L.artalk_gaga_stream_open(None, C.byref(sid)), L.artalk_gaga_stream_close(None, 0), L.artalk_gaga_stream_reset(None, 0),
               L.artalk_gaga_streams_slab(None),
               L.artalk_gaga_render_streams(None, p, 106, 1, p, p, p, None, None, 1, 0, p, None, None, None)):
        assert rc == capi.EINVAL and L.artalk_gaga_last_error(None) == b"handle is NULL"
    assert sid.value == 7
    rs = L.artalk_splat_render_sets
    sets = (C.c_int32 * 1)(0)
    assert rs(None, 8, 1, 16, 16, p, 0, p, 0, p, 0, p, 0, p, 0, p, p, 1, 0.1, 0.1, 1.0, None, p, p, sets, 1, 0, 0, 0, 0, 0, None) == capi.EINVAL
    assert L.artalk_splat_last_error(None) == b"rasteriser is NULL"
    fi = L.artalk_op_gaga_flame_inputs_sets
    assert fi(None, 106, p, p, p, 400, 1, p, p, None) == capi.EINVAL and fi(p, 106, None, p, p, 400, 1, p, p, None) == capi.EINVAL
    assert fi(p, 106, p, None, p, 400, 1, p, p, None) == capi.EINVAL and fi(p, 106, p, p, None, 400, 1, p, p, None) == capi.EINVAL
    assert fi(p, 105, p, p, p, 400, 1, p, p, None) == capi.EINVAL and fi(p, 106, p, p, p, 99, 1, p, p, None) == capi.EINVAL
    assert fi(p, 106, p, p, p, 400, 0, p, p, None) == capi.EINVAL and fi(p, 106, p, p, p, 400, 1, None, p, None) == capi.EINVAL
    fh = L.artalk_op_gaga_forehead_streams
    assert fh(None, p, 1, 8, 1, p, p, p, p, p, None) == capi.EINVAL and fh(p, None, 1, 8, 1, p, p, p, p, p, None) == capi.EINVAL
    assert fh(p, p, 9, 8, 1, p, p, p, p, p, None) == capi.EINVAL and fh(p, p, 1, 8, -1, p, p, p, p, p, None) == capi.EINVAL
    assert fh(p, p, 1, 8, 1, None, p, p, p, p, None) == capi.EINVAL and fh(p, p, 1, 8, 1, p, None, p, p, p, None) == capi.EINVAL
    assert fh(p, p, 1, 8, 1, p, p, None, p, p, None) == capi.EINVAL and fh(p, p, 1, 8, 1, p, p, p, None, p, None) == capi.EINVAL
    assert fh(p, p, 1, 8, 1, p, p, p, p, None, None) == capi.EINVAL
    assert fh(p, p, 1, 8, 0, None, None, None, p, p, None) == capi.OK and fh(p, None, 0, 8, 1, p, p, p, p, p, None) == capi.OK      # nothing to do
    me = L.artalk_op_gaga_means_sets
    assert me(None, p, p, p, 1, 4, 8, None) == capi.EINVAL and me(p, None, p, p, 1, 4, 8, None) == capi.EINVAL
    assert me(p, p, None, p, 1, 4, 8, None) == capi.EINVAL and me(p, p, p, None, 1, 4, 8, None) == capi.EINVAL
    assert me(p, p, p, p, 0, 4, 8, None) == capi.EINVAL and me(p, p, p, p, 1, 8, 7, None) == capi.EINVAL
