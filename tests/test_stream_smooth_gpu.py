"""The streaming Savitzky-Golay smoother through the model and the engine (BitwiseARModel.smooth_sessions, ARTAvatarInferEngine
.stream_step(smooth=True) / .stream_flush): live streams deliver what ``inference`` delivers, 4 frames late.

Against the reference the bar is the one its engine output is held to everywhere (FLAME_TOL against the goldens' ``engine_out``; the tiny
goldens are outside the pinned rounding-level set); against this library's own whole-clip filter it is equality: a streamed frame is the
same arithmetic on the same raw codes.  (Equality is torch.equal: dims 104: are x * 0.0 on both sides, where only the sign of a zero can
depend on x.)"""
import numpy as np
import pytest
import torch

from conftest import FLAME_TOL, get_gpu_model, get_state_dict, golden_inputs, load_golden

pytestmark = pytest.mark.gpu

SPC = 64000
GOLDEN_CLIPS = {"A": "tiny_10s_s1_style", "B": "tiny_6p3s_s2"}      # 250 frames with a style clip (3 chunks), 158 frames (2 chunks)
_shared = {}


def chunk_of(audio, j):
    """Chunk j of a clip, zero-padded as app/models.py:78-85 pads, and its number of real samples."""
    seg = audio[j * SPC:(j + 1) * SPC]
    out = torch.zeros(SPC)
    out[:seg.shape[0]] = seg
    return out, int(seg.shape[0])


def n_chunks(audio):
    return -(-audio.shape[0] // SPC)


def engine(m=None):
    from artalk_amd.engine import ARTAvatarInferEngine
    return ARTAvatarInferEngine(model=m if m is not None else get_gpu_model("tiny"))


def golden_clip(name):
    if ("golden", name) not in _shared:
        cfg, sd = get_state_dict("tiny")
        g = load_golden(GOLDEN_CLIPS[name])
        audio, style = golden_inputs(g, sd)
        _shared[("golden", name)] = (g, audio, style)
    return _shared[("golden", name)]


def restore(m):
    m.close_sessions(list(m._sessions.values()))
    m.stream_end()
    m.set_precision("f32")


def take(rec, frames, spans, i):
    first, count = spans[i]
    assert first == sum(r.shape[0] for r in rec), f"span {spans[i]} does not continue the stream at frame {sum(r.shape[0] for r in rec)}"
    rec.append(frames[i, :count].clone())


def stream_smoothed(eng, audio, style):
    """One clip through open_stream / stream_step(smooth=True, n_valid=...) alone: its smoothed frames."""
    st = eng.open_stream(style)
    rec = []
    for j in range(n_chunks(audio)):
        x, nv = chunk_of(audio, j)
        frames, spans = eng.stream_step([st], x[None].cuda(), n_valid=[nv], smooth=True)
        assert frames.shape == (1, 104, 106)
        take(rec, frames, spans, 0)
    done = st.smooth_done
    st.close()
    assert done, "the last chunk was short: the stream has ended"
    return torch.cat(rec)


def smoothed_alone(m, name, precision):
    """The golden clip streamed alone in this precision (the model is in it): computed once and left unchanged."""
    key = ("alone", name, precision)
    if key not in _shared:
        g, audio, style = golden_clip(name)
        _shared[key] = stream_smoothed(engine(m), audio, style)
    return _shared[key]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_streamed_frames_equal_the_reference_engine_output(name, precision):
    m = get_gpu_model("tiny")
    g, audio, style = golden_clip(name)
    eng = engine(m)
    m.set_precision(precision)
    try:
        got = smoothed_alone(m, name, precision)
        want = g["engine_out"]
        assert tuple(got.shape) == want.shape and want.shape[0] % 100 != 0
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"{GOLDEN_CLIPS[name]} [{precision}]: {want.shape[0]} streamed frames, max-abs difference from the reference's engine output {err:.3e}")
        assert err < FLAME_TOL
        assert float(got[:, 104:].abs().max()) == 0.0
        # the same run's raw codes through the whole-clip filter: the same bits
        st = eng.open_stream(style)
        raw = []
        for j in range(n_chunks(audio)):
            x, nv = chunk_of(audio, j)
            out, frames = eng.stream_step([st], x[None].cuda(), n_valid=[nv])
            raw.append(out[0, :frames[0]].clone())
        assert st.frames_seen == 0 and not st.smooth_done
        whole = eng._postprocess(torch.cat(raw))
        assert torch.equal(got, whole), f"streamed and whole-clip filter differ by {(got - whole).abs().max().item():.3e}"
    finally:
        restore(m)


def test_join_and_leave_out_of_phase():
    """B opens a step after A, the rows are given in swapped order, A is skipped for a step.

    The smoother first, on its own terms: every session is stepped alone (one row per step, so its raw codes are those of the clip
    streamed alone) and the sessions of a round are smoothed TOGETHER, in one artalk_session_smooth launch - each gives the same bits
    as when streamed alone.  Then the same schedule through the engine, where a step of two sessions is also a model step of two
    rows: its raw codes differ from the one-row step's at rounding level (other GEMM tiles; test_sessions_gpu.py holds batch versus
    single to 1e-5).  There the bar of bits is the whole-clip filter of the SAME steps' raw codes, taken from twin sessions run
    through the same schedule with smooth=False; the comparison with the clip streamed alone is held to 1e-5 beside it."""
    m = get_gpu_model("tiny")
    eng = engine(m)
    m.set_precision("f32")
    try:
        want = {k: smoothed_alone(m, k, "f32") for k in "AB"}
        clip = {k: golden_clip(k) for k in "AB"}
        schedule = [["A"], ["B", "A"], ["B"], ["A"]]

        rec, at = {"A": [], "B": []}, {"A": 0, "B": 0}
        sess = {"A": eng.open_stream(clip["A"][2])}
        for r, names in enumerate(schedule):
            if r == 1:
                sess["B"] = eng.open_stream(clip["B"][2])
            raw, nf = [], []
            for k in names:
                x, nv = chunk_of(clip[k][1], at[k])
                out, frames = m.step_sessions([sess[k]], x[None].cuda(), n_valid=[nv])
                raw.append(out[0])
                nf.append(frames[0])
                at[k] += 1
            frames, spans = m.smooth_sessions([sess[k] for k in names], torch.stack(raw), nf, [f < 100 for f in nf])
            for i, k in enumerate(names):
                take(rec[k], frames, spans, i)
        assert [sess[k].frames_seen for k in "AB"] == [250, 158] and sess["A"].smooth_done and sess["B"].smooth_done
        for k in "AB":
            got = torch.cat(rec[k])[:, :104]         # (the engine zeroes dims 104: afterwards)
            assert torch.equal(got, want[k][:, :104]), f"stream {k}: differs from the clip streamed alone by {(got - want[k][:, :104]).abs().max().item():.3e}"
        m.close_sessions(list(sess.values()))

        # the engine: the same schedule, and in the last round B - finished - rides along with n_valid = 0 beside the live A.  Once
        # smoothed, once on twin sessions with smooth=False (the same rows in every step, hence the same raw codes)
        schedule = [["A"], ["B", "A"], ["B"], ["B", "A"]]

        def run(smooth):
            rec, at, sess = {"A": [], "B": []}, {"A": 0, "B": 0}, {}
            for r, names in enumerate(schedule):
                if r == 0:
                    sess["A"] = eng.open_stream(clip["A"][2])
                if r == 1:
                    sess["B"] = eng.open_stream(clip["B"][2])
                parts = [chunk_of(clip[k][1], at[k]) for k in names]      # (past a clip's end: an all-zero chunk with no valid sample)
                x, nv = torch.stack([p[0] for p in parts]).cuda(), [p[1] for p in parts]
                if smooth:
                    frames, spans = eng.stream_step([sess[k] for k in names], x, n_valid=nv, smooth=True)
                    assert frames.shape == (len(names), 104, 106)
                    if r == 2:
                        assert sess["B"].smooth_done and not sess["A"].smooth_done
                    if r == 3:
                        assert spans[0] == (158, 0) and float(frames[0].abs().max()) == 0.0      # the finished stream is skipped
                    for i, k in enumerate(names):
                        take(rec[k], frames, spans, i)
                else:
                    out, counts = eng.stream_step([sess[k] for k in names], x, n_valid=nv)
                    for i, k in enumerate(names):
                        rec[k].append(out[i, :counts[i]].clone())
                for k in names:
                    at[k] += 1
            seen = [sess[k].frames_seen for k in "AB"]
            m.close_sessions(list(sess.values()))
            return {k: torch.cat(rec[k]) for k in "AB"}, seen

        got, seen = run(True)
        raw, _ = run(False)
        assert seen == [250, 158]
        for k in "AB":
            whole = eng._postprocess(raw[k])
            assert torch.equal(got[k], whole), f"stream {k}: streamed and whole-clip filter differ by {(got[k] - whole).abs().max().item():.3e}"
            worst = (got[k] - want[k]).abs().max().item()
            print(f"stream {k} through two-row engine steps: differs from the clip streamed alone by {worst:.3e}")
            assert got[k].shape == want[k].shape and worst < 1e-5
    finally:
        restore(m)


def test_slot_reuse_starts_clean():
    """A session closed mid-stream leaves 9 frames in its slot; the session that reuses the slot must not see them."""
    from artalk_amd.model import BitwiseARModel
    m = get_gpu_model("tiny")
    cfg, sd = get_state_dict("tiny")
    eng = engine(m)
    m.set_precision("f32")
    try:
        assert m.session_count() == 0
        a = eng.open_stream(golden_clip("A")[2])
        eng.stream_step([a], chunk_of(golden_clip("A")[1], 0)[0][None].cuda(), smooth=True)
        assert a.frames_seen == 100
        a.close()
        assert m.session_count() == 0                      # artalk_session_open takes the free slot of lowest index: the one `a` held
        g, audio, style = golden_clip("B")
        got = stream_smoothed(eng, audio, style)
        fresh = BitwiseARModel(cfg).eval().to("cuda")
        fresh.load_state_dict(sd, strict=True)
        fresh.set_precision("f32")
        want = stream_smoothed(engine(fresh), audio, style)
        del fresh
        assert torch.equal(got, want), f"differs from a fresh model's first session by {(got - want).abs().max().item():.3e}"
    finally:
        restore(m)


def test_smoothed_stream_survives_other_work():
    """Workspace growth, a batch call, a lockstep session and a precision round trip between a stream's steps: the carry lives in the pool."""
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    eng = engine(m)
    g, audio, style = golden_clip("A")
    m.set_precision("f16x3")
    try:
        want = smoothed_alone(m, "A", "f16x3")
        st = eng.open_stream(style)
        rec = []

        def step(j):
            x, nv = chunk_of(audio, j)
            frames, spans = eng.stream_step([st], x[None].cuda(), n_valid=[nv], smooth=True)
            take(rec, frames, spans, 0)

        step(0)
        before, b = m.workspace_bytes(), 8
        while m.workspace_bytes() == before and b <= 256:      # artalk_reserve until the workspace has to be allocated anew
            m.reserve(b, 2 * b)
            b *= 2
        assert m.workspace_bytes() > before, "artalk_reserve did not grow the workspace"
        m.inference_batch([torch.from_numpy(synth_audio(740 + i, 4.0 + i)) for i in range(3)])
        m.stream_begin(2)
        m.stream_chunk(torch.stack([chunk_of(torch.from_numpy(synth_audio(750 + i, 4.0)), 0)[0] for i in range(2)]).cuda())
        m.stream_end()
        step(1)
        m.set_precision("f32")
        m.set_precision("f16x3")
        assert m.session_count() == 1 and not st.closed
        step(2)
        got = torch.cat(rec)
        assert torch.equal(got, want), f"differs from the undisturbed stream by {(got - want).abs().max().item():.3e}"
    finally:
        restore(m)


def test_scale_change_closes_the_smoother_too():
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    x = chunk_of(torch.from_numpy(synth_audio(760, 8.0)), 0)[0][None].cuda()
    m.set_precision("f16x3")
    saved = m.scales()
    try:
        names = list(saved)
        st = m.open_session()
        raw = m.step_sessions([st], x)
        frames, spans = m.smooth_sessions([st], raw)
        assert spans == [(0, 96)] and frames.shape == (1, 104, 106)
        assert m._write_site_exps([saved[k] - (1 if k == names[0] else 0) for k in names]) == 1      # the Python object does not know yet
        with pytest.raises(RuntimeError, match="scales changed"):
            m.smooth_sessions([st], raw)
        assert st.closed and st.frames_seen == 100
        with pytest.raises(RuntimeError, match="scales changed"):
            m.smooth_sessions([st], raw)
    finally:
        m.load_scales(saved)
        restore(m)


def test_flush_short_clips_and_the_unsmoothed_path():
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    eng = engine(m)
    m.set_precision("f32")
    try:
        audio = torch.from_numpy(synth_audio(770, 8.0))         # 200 frames: the clip ends on a chunk boundary
        assert audio.shape[0] == 2 * SPC
        st, twin = eng.open_stream(), eng.open_stream()
        rec, raw = [], []
        for j in range(2):
            x, nv = chunk_of(audio, j)
            frames, spans = eng.stream_step([st], x[None].cuda(), n_valid=[nv], smooth=True)
            take(rec, frames, spans, 0)
            # smooth=False is the call of before: one tensor (with n_valid: and the frame counts), fix_pose / zeroing applied to the raw codes
            plain = eng.stream_step([twin], x[None].cuda())
            assert isinstance(plain, torch.Tensor) and plain.shape == (1, 100, 106)
            raw.append(plain[0].clone())
        assert not st.smooth_done and [r.shape[0] for r in rec] == [96, 100]
        tail, spans = eng.stream_flush([st])
        assert tail.shape == (1, 4, 106) and spans == [(196, 4)] and st.smooth_done
        got = torch.cat(rec + [tail[0]])
        whole = eng._postprocess(torch.cat(raw))
        assert torch.equal(got, whole), f"streamed and whole-clip filter differ by {(got - whole).abs().max().item():.3e}"
        with pytest.raises(RuntimeError):
            eng.stream_flush([st])                              # a second flush
        # a finished stream in a later step: skipped when it brings nothing, refused when it brings frames - before anything runs
        ticket = m.last_ticket()
        x, nv = chunk_of(audio, 0)
        with pytest.raises(RuntimeError):
            eng.stream_step([st], x[None].cuda(), n_valid=[nv], smooth=True)
        assert m.last_ticket() == ticket
        frames, spans = eng.stream_step([st], torch.zeros(1, SPC).cuda(), n_valid=[0], smooth=True)
        assert spans == [(200, 0)] and float(frames.abs().max()) == 0.0
        # smooth=False with n_valid: (codes, frame counts), the twin of step_sessions with the engine's zeroing
        p, q = eng.open_stream(), eng.open_stream()
        x, nv = chunk_of(torch.from_numpy(synth_audio(771, 3.0)), 0)
        out, counts = eng.stream_step([p], x[None].cuda(), n_valid=[nv])
        ref, ref_counts = m.step_sessions([q], x[None].cuda(), n_valid=[nv])
        ref[..., 104:] *= 0.0
        assert counts == ref_counts == [75] and out.shape == (1, 100, 106) and torch.equal(out, ref)
        # 0.3 s: 8 frames, fewer than the filter's window - ValueError as from inference, and nothing has been stepped
        short = torch.from_numpy(synth_audio(772, 0.3))
        s8 = eng.open_stream()
        ticket = m.last_ticket()
        x, nv = chunk_of(short, 0)
        with pytest.raises(ValueError):
            eng.stream_step([s8], x[None].cuda(), n_valid=[nv], smooth=True)
        with pytest.raises(ValueError):
            eng.stream_flush([s8])
        assert m.last_ticket() == ticket and s8.fed == 0 and s8.frames_seen == 0 and not s8.closed
        with pytest.raises(ValueError):
            eng.inference(short)
    finally:
        restore(m)


def test_smooth_call_leaves_a_lockstep_session_alone():
    """artalk_session_smooth touches neither the workspace nor the status word: a lockstep session goes on across it, with the same bits."""
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    audio = torch.from_numpy(synth_audio(780, 8.0))
    chunks = [chunk_of(audio, j)[0][None].cuda() for j in range(2)]
    m.set_precision("f32")
    try:
        st = m.open_session()
        raw = m.step_sessions([st], chunks[0])
        m.stream_begin(1)
        want = [m.stream_chunk(c) for c in chunks]
        m.stream_end()
        m.stream_begin(1)
        got = [m.stream_chunk(chunks[0])]
        ticket = m.last_ticket()
        frames, spans = m.smooth_sessions([st], raw)
        assert spans == [(0, 96)] and m.last_ticket() == ticket
        got.append(m.stream_chunk(chunks[1]))
        m.stream_end()
        for j in range(2):
            assert torch.equal(got[j], want[j]), f"lockstep chunk {j}: max-abs difference {(got[j] - want[j]).abs().max().item():.3e}"
    finally:
        restore(m)


def test_a_stream_is_smoothed_from_its_first_step_or_not_at_all():
    from artalk_amd.synth import synth_audio
    m = get_gpu_model("tiny")
    eng = engine(m)
    x = chunk_of(torch.from_numpy(synth_audio(790, 8.0)), 0)[0][None].cuda()
    m.set_precision("f32")
    try:
        st = eng.open_stream()
        eng.stream_step([st], x)
        ticket = m.last_ticket()
        with pytest.raises(RuntimeError, match="from its first step"):
            eng.stream_step([st], x, smooth=True)
        with pytest.raises(RuntimeError, match="from its first step"):
            eng.stream_flush([st])
        assert m.last_ticket() == ticket and st.frames_seen == 0 and not st.closed
    finally:
        restore(m)

