"""Conv stack over the frames that hear real audio (artalk_infer_samples / artalk_set_tail_skip): skip on against skip off on the
same model, bit for bit - FLAME codes, decision bits, history bits and wav2vec2 features - with no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from artalk_amd import capi
from artalk_amd.synth import synth_audio, synth_style

from conftest import get_gpu_model, get_state_dict

pytestmark = pytest.mark.gpu


def _clips(secs, seed0, styled=()):
    _, sd = get_state_dict("tiny")
    mean, std = sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()
    audios = [torch.from_numpy(synth_audio(seed0 + i, t)) for i, t in enumerate(secs)]
    styles = [torch.from_numpy(synth_style(seed0 + i, mean, std)) if i in styled else None for i in range(len(secs))]
    return audios, styles


def _run(m, audios, styles, skip):
    m.set_tail_skip(skip)
    out = m.inference_batch(audios, styles, return_aux=True)
    a = m.last_aux
    return dict(out=[o.cpu().numpy() for o in out], bits=[b.cpu().numpy() for b in a["bits"]],
                hist_bits=[h.cpu().numpy() for h in a["hist_bits"]], w2v=a["w2v"].cpu().numpy(), status=m.status())


def _assert_same(on, off, tag):
    assert on["status"] == off["status"], tag
    assert np.array_equal(on["w2v"], off["w2v"]), f"{tag}: wav2vec2 features differ, max |diff| {np.abs(on['w2v'] - off['w2v']).max():.3e}"
    for k in ("out", "bits", "hist_bits"):
        for i, (x, y) in enumerate(zip(on[k], off[k])):
            assert x.shape == y.shape and np.array_equal(x, y), f"{tag}: {k} of clip {i} differs"


def _on_off(m, precision, audios, styles, tag):
    m.set_precision(precision)
    try:
        off = _run(m, audios, styles, False)
        on = _run(m, audios, styles, True)
    finally:
        m.set_tail_skip(True)
        m.set_precision("f32")
    _assert_same(on, off, f"{tag} [{precision}]")
    return on


PRECISIONS = ["f16x3", "f32", "bf16"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seconds", [0.5, 4.0, 4.02, 6.3, 7.95])
def test_batch1_skip_on_equals_off(seconds, precision):
    """0.5 s: one partial chunk alone; 4.0 s: no partial chunk (the same launches as off); 4.02 s: a second chunk with 320 samples;
    6.3 s: a full and a partial chunk in one pass group; 7.95 s: t_c >= 198, counts as full."""
    m = get_gpu_model("tiny")
    audios, styles = _clips([seconds], 40, styled=(0,))
    _on_off(m, precision, audios, styles, f"batch 1, {seconds} s")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_batch_skip_on_equals_off(precision):
    """10 s / 6.3 s / 1.1 s: partial chunks at all three chunk indices (17 600, 36 800 and 32 000 samples: two length classes), a call
    order that differs from the pass order, and clips handed over unsorted."""
    m = get_gpu_model("tiny")
    audios, styles = _clips([6.3, 1.1, 10.0], 50, styled=(1,))
    _on_off(m, precision, audios, styles, "ragged 6.3 / 1.1 / 10 s")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nine_equal_clips_skip_on_equals_off(precision):
    """9 x 6 s (two clip groups in the body): nine full and nine half chunks, so the passes' row counts fall on the other side of the
    GEMM planner's and the LayerNorm launcher's thresholds than the one launch over all 18 chunks - whose plan they must keep."""
    m = get_gpu_model("tiny")
    audios, styles = _clips([6.0] * 9, 60)
    _on_off(m, precision, audios, styles, "9 x 6 s")


def test_calibrated_heavy_profile_same_exponents_and_outputs():
    """The audit pass sees the same maxima with the skip on (the copied rows equal the computed one): calibrating on a clip with a
    partial chunk gives the same site exponents, and the calibrated f16x3 results are the same bits."""
    m = get_gpu_model("tiny", "heavy")
    _, sd = get_state_dict("tiny", "heavy")
    audio = torch.from_numpy(synth_audio(2, 6.3))
    style = torch.from_numpy(synth_style(2, sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()))
    got = {}
    try:
        for skip in (False, True):
            m.reset_scales()
            m.set_precision("f16x3")
            m.set_tail_skip(skip)
            changed = m.calibrate([audio], [style])
            got[skip] = (changed, m.scales(), _run(m, [audio], [style], skip))
    finally:
        m.set_tail_skip(True)
        m.reset_scales()
        m.set_precision("f32")
    assert got[True][0] == got[False][0] > 0
    assert got[True][1] == got[False][1]
    assert got[True][2]["status"] == 0
    _assert_same(got[True][2], got[False][2], "heavy profile, calibrated")


def test_skip_engages_on_the_declared_padding_only():
    """That the frames behind the declared end are really not computed: an 8 s clip declared as 6 s (its audio behind 6 s is NOT zero,
    against the contract) gives other features for its second chunk than the whole-chunk run, the same bits for its first chunk - and
    the whole-chunk features again with the switch off or without counts."""
    m = get_gpu_model("tiny")
    L = capi.lib()
    audio = torch.from_numpy(synth_audio(70, 8.0))[None].cuda().contiguous()
    nch = (C.c_int64 * 1)(2)

    def run(ns):
        out = torch.zeros(1, 200, 106, device="cuda")
        w2v = torch.zeros(2, 199, 1024, device="cuda")
        torch.cuda.synchronize()
        rc = L.artalk_infer_samples(m._h, capi.ptr(audio), audio.stride(0), nch, (C.c_int64 * 1)(ns) if ns else None, 1, None, None,
                                    capi.ptr(out), out.stride(0), None, None, capi.ptr(w2v), None)
        assert rc == capi.OK, m._err()
        torch.cuda.synchronize()
        return w2v.cpu().numpy()

    m.stream_end()
    try:
        whole = run(None)
        short = run(6 * 16000)
        m.set_tail_skip(False)
        off = run(6 * 16000)
    finally:
        m.set_tail_skip(True)
    assert np.array_equal(whole, off)
    assert np.array_equal(whole[0], short[0])
    assert not np.array_equal(whole[1], short[1])


def test_sample_counts_are_validated():
    """A count that does not fit its clip's chunk count is refused before anything is enqueued; NULL counts run whole chunks."""
    m = get_gpu_model("tiny")
    L = capi.lib()
    audio = torch.zeros(1, 2 * 64000, device="cuda")
    out = torch.zeros(1, 200, 106, device="cuda")
    nch = (C.c_int64 * 1)(2)
    for bad in (0, -1, 2 * 64000 + 1):
        ns = (C.c_int64 * 1)(bad)
        rc = L.artalk_infer_samples(m._h, capi.ptr(audio), audio.stride(0), nch, ns, 1, None, None, capi.ptr(out), out.stride(0), None, None, None, None)
        assert rc == capi.EINVAL, (bad, rc)
    torch.cuda.synchronize()
