"""The engine object holds its device blocks, pinned blocks, events, streams and graph executables through the owner types of
csrc/device_mem.h, like the avatar-head objects (tests/test_head_buffers_gpu.py): a model whose workspace and staging ring have been
regrown must give a fresh model's bits, a model that has taken everything it can own must be destroyed cleanly and leave nothing
behind in the next one, and the side streams must come back after every change of the CU mask.  `tiny` configuration, synthetic clips;
every comparison is torch.equal on the outputs and on last_aux["bits"]."""
import pytest
import torch

from artalk_amd.model import BitwiseARModel
from artalk_amd.synth import synth_audio
from conftest import get_state_dict
from test_head_buffers_gpu import _dirty_device_memory

pytestmark = pytest.mark.gpu

_CLIPS = {}


def _clip(seed, seconds):
    if (seed, seconds) not in _CLIPS:
        _CLIPS[(seed, seconds)] = torch.from_numpy(synth_audio(seed, seconds))
    return _CLIPS[(seed, seconds)]


def _batch8():
    """8 clips of one chunk: two clip groups, so the side stream, the fork and join events and two graphs per chunk index"""
    return [_clip(300 + i, 3.0) for i in range(8)]


def _model(precision):
    cfg, sd = get_state_dict("tiny")
    m = BitwiseARModel(cfg).eval().to("cuda")
    m.load_state_dict(sd, strict=True)
    m.set_precision(precision)
    return m


def _run(m, audios):
    outs = [o.cpu() for o in m.inference_batch(audios, None, return_aux=True)]
    bits = [b.cpu() for b in m.last_aux["bits"]]
    assert m.status() == 0
    return outs, bits


def _same(got, want, what):
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert torch.equal(a, b), f"{what}: output of clip {i} differs"
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        assert torch.equal(a, b), f"{what}: bits of clip {i} differ"


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_regrown_workspace_gives_a_fresh_models_bits(precision):
    """One 2 s clip (one chunk, batch 1), three clips of 5.5 s (two chunks each: the workspace and the staging ring grow, the graphs
    are dropped), then the first call again (graphs captured again on the new workspace).  Device memory is dirtied before each call,
    so a block that is not zero-filled where it must be has a chance to show."""
    steps = ([_clip(1, 2.0)], [_clip(10 + i, 5.5) for i in range(3)], [_clip(1, 2.0)])
    want = []
    for audios in steps:
        fresh = _model(precision)
        want.append(_run(fresh, audios))
        del fresh
    live = _model(precision)
    grown = []
    for k, (audios, w) in enumerate(zip(steps, want)):
        _dirty_device_memory()
        _same(_run(live, audios), w, f"{precision}, call {k}: the long-lived model differs from a fresh one")
        grown.append(live.workspace_bytes())
    assert grown[1] > grown[0] and grown[2] == grown[1]      # the second call regrew the workspace, the third kept it


def test_a_model_that_owns_everything_is_destroyed_cleanly():
    """Three models in a row take everything a model can own - weights and packed copies, the bf16 copy, the audit block, workspace and
    staging ring, a side stream with its fork and join events, graphs, a session block and the smoother's table, the stage events of
    profiling level 1 and the kernel timer's pool of level 3 - and are deleted.  Their batch outputs are equal to each other."""
    audios = _batch8()
    results = []
    for _ in range(3):
        m = _model("f16x3")
        m.set_precision("bf16")
        m.set_precision("f16x3")
        m.calibrate([audios[0]])
        results.append(_run(m, audios))
        assert m.graph_count()[0] >= 2
        sessions = m.open_sessions([None, None])
        chunk = torch.stack([torch.nn.functional.pad(a, (0, 64000 - a.shape[0])) for a in audios[:2]])
        out = m.step_sessions(sessions, chunk)
        assert out.shape == (2, 100, 106) and torch.isfinite(out).all() and m.status() == 0
        m.set_profiling(3)
        m.inference_batch(audios)
        ks = m.get_kernel_sums()
        assert ks["kernels"] > 0 and ks["w2v_encoder"] > 0.0
        m.set_profiling(1)
        m.inference_batch(audios)
        prof = m.get_profile()
        assert prof["total_ms"] > 0.0
        m.set_profiling(0)
        del m, sessions
        torch.cuda.synchronize()
    _same(results[1], results[0], "second model")
    _same(results[2], results[0], "third model")


def test_cu_mask_twice_over():
    """Mask on, call, mask off, call, mask on again, call: the side stream and its join event go with every change of the mask and come
    back masked or unmasked with the next call.  All three results equal the first, unmasked one."""
    audios = _batch8()
    m = _model("f16x3")
    want = _run(m, audios)
    half = [0xFFFFFFFF] * 4 + [0] * 4
    for k, words in enumerate((half, None, half)):
        m.set_cu_mask(words)
        _same(_run(m, audios), want, f"after mask change {k}")
    m.set_cu_mask(None)
