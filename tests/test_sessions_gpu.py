"""Independent streaming sessions (artalk_session_open / _step / _close, BitwiseARModel.open_session / step_sessions): streams that join
and leave between steps, their history kept in the model's session pool and gathered into the workspace for the duration of a step.

A step of n sessions runs what lockstep streaming (artalk_stream_chunk) runs for n streams - the same workspace rows, the same captured
graphs - so the bar against lockstep is identical bits; against the reference's goldens it is conftest.assert_clip_parity, and against
the same clip streamed alone the project's batch-versus-single bar, 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_clip_parity, dense_margins, get_gpu_model, get_state_dict, golden_inputs, load_golden

pytestmark = pytest.mark.gpu

SPC = 64000
_shared = {}      # references computed once per test session and left unchanged


def chunk_of(audio, j):
    """Chunk j of a clip, zero-padded by the caller as app/models.py:78-85 pads, and its number of real samples."""
    seg = audio[j * SPC:(j + 1) * SPC]
    out = torch.zeros(SPC)
    out[:seg.shape[0]] = seg
    return out, int(seg.shape[0])


def chunks(audios, js):
    return torch.stack([chunk_of(a, j)[0] for a, j in zip(audios, js)]).cuda()


def restore(m, graphs=False):
    m.close_sessions(list(m._sessions.values()))
    m.stream_end()
    if graphs:
        m.set_graphs(True)
    m.set_precision("f32")


def two_clips():
    """The two 10 s clips and styles (None, styled) of test_e2e_gpu.py::test_streaming_equals_batch_call."""
    if "two" not in _shared:
        from artalk_amd.synth import synth_audio, synth_style
        cfg, sd = get_state_dict("tiny")
        mean, std = sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()
        _shared["two"] = ([torch.from_numpy(synth_audio(20 + i, 10.0)) for i in range(2)], [None, torch.from_numpy(synth_style(21, mean, std))])
    return _shared["two"]


def lockstep_two(m, precision, fresh=False):
    """stream_begin(2) / 3 x stream_chunk of the two clips in this precision (the model is in it): the chunks, once per test session
    (fresh: run it now, so that the graphs of 2 streams are certainly in the cache)."""
    key = ("lockstep2", precision)
    if fresh or key not in _shared:
        audios, styles = two_clips()
        m.stream_begin(2, styles)
        _shared[key] = [m.stream_chunk(chunks(audios, [j, j])) for j in range(3)]
        m.stream_end()
    return _shared[key]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_same_composition_equals_lockstep_bit_for_bit(precision):
    m = get_gpu_model("tiny")
    audios, styles = two_clips()
    m.set_precision(precision)
    try:
        want = lockstep_two(m, precision, fresh=True)
        captures = m.graph_count()[1]
        ss = m.open_sessions(styles)
        for j in range(3):
            got = m.step_sessions(ss, chunks(audios, [j, j]))
            assert got.shape == (2, 100, 106)
            assert torch.equal(got, want[j]), f"[{precision}] chunk {j}: max-abs difference {(got - want[j]).abs().max().item():.3e}"
        assert m.graph_count()[1] == captures, "the sessions must replay the graphs lockstep streaming of 2 captured"
        assert [s.fed for s in ss] == [3 * SPC] * 2 and m.status() == 0
    finally:
        restore(m)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_rows_follow_the_callers_order(precision):
    m = get_gpu_model("tiny")
    audios, styles = two_clips()
    m.set_precision(precision)
    try:
        want = lockstep_two(m, precision)
        s0, s1 = m.open_sessions(styles)
        for j in range(3):
            got = m.step_sessions([s1, s0], chunks([audios[1], audios[0]], [j, j]))
            assert torch.equal(got, want[j].flip(0)), f"[{precision}] chunk {j}: max-abs difference {(got - want[j].flip(0)).abs().max().item():.3e}"
    finally:
        restore(m)


GOLDEN_CLIPS = {"A": "tiny_10s_s1_style", "B": "tiny_6p3s_s2", "C": "tiny_4s_s0"}


def golden_clip(name):
    if ("golden", name) not in _shared:
        cfg, sd = get_state_dict("tiny")
        g = load_golden(GOLDEN_CLIPS[name])
        audio, style = golden_inputs(g, sd)
        _shared[("golden", name)] = (g, audio, style)
    return _shared[("golden", name)]


def streamed_alone(m, name, precision):
    """The clip through stream_begin(1) / stream_chunk in this precision: its chunks, once per test session."""
    key = ("alone", name, precision)
    if key not in _shared:
        g, audio, style = golden_clip(name)
        m.stream_begin(1, [style])
        _shared[key] = [m.stream_chunk(chunk_of(audio, j)[0][None].cuda())[0] for j in range(g["bits"].shape[0])]
        m.stream_end()
    return _shared[key]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_join_leave_and_slot_reuse_against_reference_goldens(precision):
    """C and A start; C leaves and B joins (in C's slot, under a new id); D - C's clip again - joins late.  Every clip must be what the
    reference computes for it alone: decisions exact group by group, FLAME codes within FLAME_TOL (conftest.assert_clip_parity)."""
    from artalk_amd import capi
    m = get_gpu_model("tiny")
    L = capi.lib()
    m.set_precision(precision)
    rec = {k: dict(out=[], bits=[], hist=[], frames=[], chunk=[]) for k in "ABCD"}
    clip_of = {"A": "A", "B": "B", "C": "C", "D": "C"}

    def step(names, sess):
        js = [len(rec[k]["out"]) for k in names]
        parts = [chunk_of(golden_clip(clip_of[k])[1], j) for k, j in zip(names, js)]
        out, frames, bits, hist = m.step_sessions([sess[k] for k in names], torch.stack([p[0] for p in parts]).cuda(),
                                                  n_valid=[p[1] for p in parts], return_aux=True)
        for i, k in enumerate(names):
            r = rec[k]
            r["chunk"].append(out[i]); r["out"].append(out[i, :frames[i]].cpu().numpy()); r["frames"].append(frames[i])
            r["bits"].append(bits[i].cpu().numpy()); r["hist"].append(hist[i].cpu().numpy())

    try:
        alone = {k: streamed_alone(m, k, precision) for k in "ABC"}
        sess = {}
        sess["C"], sess["A"] = m.open_sessions([golden_clip("C")[2], golden_clip("A")[2]])
        step(["C", "A"], sess)
        sess["C"].close()
        sess["B"] = m.open_session(golden_clip("B")[2])
        assert L.artalk_session_count(m._h) == 2 and m.session_count() == 2
        assert sess["B"].id != sess["C"].id and sess["C"].closed
        step(["A", "B"], sess)
        sess["D"] = m.open_session(golden_clip("C")[2])
        step(["B", "D", "A"], sess)
        m.close_sessions([sess[k] for k in "ABD"])
        assert m.session_count() == 0
        assert m.status() == 0 and m._precision == precision
        for k in "ABCD":
            g, audio, style = golden_clip(clip_of[k])
            case, r = GOLDEN_CLIPS[clip_of[k]], rec[k]
            n_chunks = g["bits"].shape[0]
            assert len(r["out"]) == n_chunks, f"session {k} ran {len(r['out'])} of {n_chunks} chunks"
            gbits, ghist = np.unpackbits(g["bits"], axis=-1), np.unpackbits(g["hist_bits"], axis=-1)
            hist = np.stack([ghist[0]] + r["hist"])       # the initial history is the same for every clip: the golden's
            good, _, err = assert_clip_parity(case, precision, np.concatenate(r["out"]), np.stack(r["bits"]), hist, g["out"], gbits, ghist,
                                              dense_margins(g["logit_margin"]), dense_margins(g["hist_margin"]), inputs=("tiny", audio, style))
            assert sum(r["frames"]) == g["out"].shape[0] and all(f == 100 for f in r["frames"][:-1])
            worst = max((c - a).abs().max().item() for c, a in zip(r["chunk"], alone[clip_of[k]]))
            print(f"session {k} ({case}) [{precision}]: chunks exact {good}/{n_chunks}, FLAME err {err:.3e}, vs streamed alone {worst:.3e}")
            assert worst < 1e-5, f"session {k} [{precision}]: differs from the clip streamed alone by {worst:.3e}"
    finally:
        restore(m)


def test_sessions_survive_other_work():
    """A batch call that grows the workspace, a lockstep session, a style encode and a precision round trip between a session's steps:
    the workspace is scratch to a session."""
    from artalk_amd import capi
    from artalk_amd.synth import synth_audio, synth_style
    m = get_gpu_model("tiny")
    cfg, sd = get_state_dict("tiny")
    mean, std = sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()
    g, audio, style = golden_clip("A")
    m.set_precision("f16x3")
    try:
        fresh = m.open_session(style)
        want = [m.step_sessions([fresh], chunk_of(audio, j)[0][None].cuda()) for j in range(3)]
        fresh.close()
        a = m.open_session(style)
        got = [m.step_sessions([a], chunk_of(audio, 0)[0][None].cuda())]
        before = m.workspace_bytes()
        n_big = 5
        while True:      # a batch the workspace has to grow for, whatever earlier tests left behind
            m.inference_batch([torch.from_numpy(synth_audio(700 + i, 4.0 + i % 5)) for i in range(n_big)])
            if m.workspace_bytes() > before or n_big >= 40:
                break
            n_big *= 2
        assert m.workspace_bytes() > before, "the batch call did not grow the workspace"
        others, ostyles = two_clips()
        m.stream_begin(2, ostyles)
        m.stream_chunk(chunks(others, [0, 0]))
        m.stream_end()
        clip = torch.from_numpy(synth_style(733, mean, std)).cuda()[None].contiguous()
        cond = torch.empty(1, cfg.embed_dim, device="cuda")
        torch.cuda.synchronize()
        assert capi.lib().artalk_style_encode(m._h, capi.ptr(clip), 1, capi.ptr(cond), C.c_void_p(m._stream.cuda_stream)) == capi.OK
        m.set_precision("f32")
        m.set_precision("f16x3")
        assert m.session_count() == 1 and not a.closed
        got += [m.step_sessions([a], chunk_of(audio, j)[0][None].cuda()) for j in (1, 2)]
        for j in range(3):
            assert torch.equal(got[j], want[j]), f"chunk {j}: max-abs difference {(got[j] - want[j]).abs().max().item():.3e}"
    finally:
        restore(m)


def test_two_clip_groups_with_and_without_graphs():
    """9 sessions: the body runs as two clip groups on two streams (test_edge_cases_gpu.py::test_streaming_shares_the_batch_calls_graphs),
    replayed from graphs and launched eagerly."""
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    audios = [torch.from_numpy(synth_audio(620 + i, 8.0)) for i in range(9)]
    x = chunks(audios, [0] * 9)
    m.set_precision("f16x3")
    try:
        for graphs in (True, False):
            m.set_graphs(graphs)
            m.stream_begin(9)
            want = m.stream_chunk(x)
            m.stream_end()
            ss = m.open_sessions([None] * 9)
            got = m.step_sessions(ss, x)
            assert torch.equal(got, want), f"graphs {graphs}: max-abs difference {(got - want).abs().max().item():.3e}"
            assert (m.graph_count()[0] > 0) == graphs
            m.close_sessions(ss)
    finally:
        restore(m, graphs=True)


def test_more_than_one_pool_block():
    """40 sessions need two pool blocks of 32 slots; a step may list sessions of both, and leaves the others alone."""
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    clips = [torch.from_numpy(synth_audio(660 + i, 4.0)) for i in range(3)]
    x3 = chunks(clips, [0, 0, 0])
    five = torch.from_numpy(synth_audio(670, 8.0))
    a, b = chunk_of(five, 0)[0][None].cuda(), chunk_of(five, 1)[0][None].cuda()
    m.set_precision("f32")
    try:
        ss = m.open_sessions([None] * 40)
        assert m.session_count() == 40 and len({s.id for s in ss}) == 40
        m.step_sessions([ss[5]], a)
        got3 = m.step_sessions([ss[0], ss[17], ss[32]], x3)
        got5 = m.step_sessions([ss[5]], b)
        m.close_sessions(ss)
        assert m.session_count() == 0
        fresh = m.open_sessions([None] * 3)
        want3 = m.step_sessions(fresh, x3)
        m.close_sessions(fresh)
        twin = m.open_session()
        m.step_sessions([twin], a)
        want5 = m.step_sessions([twin], b)
        assert torch.equal(got3, want3), f"sessions 0, 17, 32: max-abs difference {(got3 - want3).abs().max().item():.3e}"
        assert torch.equal(got5, want5), f"session 5: max-abs difference {(got5 - want5).abs().max().item():.3e}"
        assert (want3[0] - want3[1]).abs().max().item() > 1e-3      # (the three clips do differ)
    finally:
        restore(m)


def test_precomputed_style_condition():
    """A session opened with the condition artalk_style_encode computed (flag 2: the style-clip cache) equals one opened with the clip."""
    m = get_gpu_model("tiny")
    g, audio, style = golden_clip("A")
    m.set_precision("f32")
    old = m.style_cache_size
    try:
        m.style_cache_size = 0
        m._style_cache.clear()
        by_clip = m.open_session(style)                      # flag 1: encoded inside artalk_session_open
        m.style_cache_size = 8
        by_cond = m.open_session(style)                      # flag 2: encoded by artalk_style_encode, handed in as 768 floats
        assert len(m._style_cache) == 1
        for j in range(2):
            x = chunk_of(audio, j)[0][None].cuda()
            one, two = m.step_sessions([by_clip], x), m.step_sessions([by_cond], x)
            assert torch.equal(one, two), f"chunk {j}: max-abs difference {(one - two).abs().max().item():.3e}"
        plain = m.open_session()
        assert (m.step_sessions([plain], chunk_of(audio, 0)[0][None].cuda()) - streamed_alone(m, "A", "f32")[0]).abs().max().item() > 1e-4
    finally:
        m.style_cache_size = old
        m._style_cache.clear()
        restore(m)


def test_errors_leave_everything_intact():
    from artalk_amd import capi
    from artalk_amd.model import StreamSession
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    L = capi.lib()
    audio = torch.from_numpy(synth_audio(680, 8.0))
    a, b = chunk_of(audio, 0)[0][None].cuda(), chunk_of(audio, 1)[0][None].cuda()
    m.set_precision("f32")
    try:
        twin = m.open_session()
        m.step_sessions([twin], a)
        want = m.step_sessions([twin], b)
        twin.close()
        s, gone = m.open_sessions([None, None])
        gone.close()
        m.step_sessions([s], a)
        torch.cuda.synchronize()
        ticket = m.last_ticket()
        x2 = torch.cat([a, a]).contiguous()
        out = torch.empty(2, 100, 106, device="cuda")
        stream = C.c_void_p(m._stream.cuda_stream)

        def c_step(ids, n):
            arr = (C.c_int64 * max(len(ids), 1))(*ids)
            return L.artalk_session_step(m._h, arr, n, capi.ptr(x2), x2.stride(0), capi.ptr(out), out.stride(0), None, None, stream)

        never = s.id + 1000
        assert c_step([gone.id], 1) == capi.EINVAL           # closed
        assert c_step([never], 1) == capi.EINVAL             # never issued
        assert c_step([s.id, s.id], 2) == capi.EINVAL        # listed twice
        assert c_step([s.id, gone.id], 2) == capi.EINVAL     # one bad id spoils the call
        assert c_step([s.id], 0) == capi.EINVAL              # n = 0
        assert L.artalk_session_step(m._h, None, 1, capi.ptr(x2), x2.stride(0), capi.ptr(out), out.stride(0), None, None, stream) == capi.EINVAL
        bad = (C.c_int64 * 1)(never)
        assert L.artalk_session_close(m._h, bad, 1) == capi.EINVAL and L.artalk_session_close(m._h, bad, 0) == capi.EINVAL
        assert L.artalk_session_open(m._h, 0, None, None, bad, stream) == capi.EINVAL
        assert L.artalk_session_open(m._h, 1, None, None, None, stream) == capi.EINVAL
        assert L.artalk_sessions_reserve(m._h, 0) == capi.EINVAL
        with pytest.raises((RuntimeError, AssertionError)):
            m.step_sessions([gone], a)
        with pytest.raises((RuntimeError, AssertionError)):
            m.step_sessions([StreamSession(m, never)], a)
        with pytest.raises((RuntimeError, AssertionError)):
            m.step_sessions([s, s], x2)
        with pytest.raises((RuntimeError, AssertionError)):
            m.step_sessions([], x2[:0])
        assert m.last_ticket() == ticket, "a refused call must not enqueue anything"
        assert m.session_count() == 1 and not s.closed
        got = m.step_sessions([s], b)
        assert torch.equal(got, want), f"max-abs difference {(got - want).abs().max().item():.3e}"
    finally:
        restore(m)


def test_scale_change_closes_sessions():
    """A session never mixes exponents: any change of site scales closes every session, and a step on an old one says why."""
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    x = chunk_of(torch.from_numpy(synth_audio(690, 4.0)), 0)[0][None].cuda()
    m.set_precision("f16x3")
    saved = m.scales()
    try:
        names = list(saved)
        lowered = dict(saved)
        lowered[names[0]] = saved[names[0]] - 1
        # through the C ABI alone: the Python objects do not know yet, the library's message comes through
        s1 = m.open_session()
        m.step_sessions([s1], x)
        assert m._write_site_exps([lowered[k] for k in names]) == 1
        assert m.session_count() == 0
        with pytest.raises(RuntimeError, match="scales changed"):
            m.step_sessions([s1], x)
        assert s1.closed
        # through load_scales: the sessions are marked at once
        s2 = m.open_session()
        assert m.step_sessions([s2], x).isfinite().all() and m.status() == 0 and m._precision == "f16x3"
        assert m.load_scales(saved) == 1
        assert s2.closed and m.session_count() == 0
        with pytest.raises(RuntimeError, match="scales changed"):
            m.step_sessions([s2], x)
        s3 = m.open_session()
        assert s3.id > s2.id > s1.id
        assert m.step_sessions([s3], x).isfinite().all() and m.status() == 0
        assert m.load_scales(saved) == 0 and not s3.closed      # nothing changed: nothing closes
    finally:
        m.load_scales(saved)
        restore(m)
