"""End to end in the bf16 precision mode (set_precision("bf16"), artalk_set_precision 2): every GEMM but the logit / code heads on
one bf16 MFMA product, the rest on the f32 mode's schedule.  This is the error torch bf16 autocast gives the reference, not the
decision parity of the f32 / f16x3 modes: BASELINE.md measured the reference itself under bf16 autocast at 1.4-7.6 % AR bits
flipped per chunk and 1.3e-2 FLAME max-abs.  Later chunks diverge through the history once a bit flips, so only chunk 0 is held
to a bar; the whole-clip figures are printed (and recorded by tools/bf16_bench.py).

Bars (chunk 0, against the reference's golden fixtures): AR-bit flip rate <= FLIP_BAR, FLAME max-abs <= FLAME_BAR, output finite
over the whole clip, status 0, the model still in bf16 mode.  First MI355X measurement (profiles/r06_bf16_bench.json, the six cases
below and the `heavy` profile): chunk-0 flip rate 0.2-1.7 %, chunk-0 FLAME max-abs 1.8e-2 - 3.8e-2; whole clips up to 4.2 % and 0.2.
FLIP_BAR is about twice the worst chunk-0 flip rate; FLAME_BAR is the 5e-2 ceiling (twice the observed worst would be looser).

bf16 amplifies summation order: a last-bit difference of an fp32 sum can move the bf16 rounding of that activation at the next GEMM
by 2^-8 of its value.  Batch vs single runs and streaming vs the batch call tile (and split) their GEMMs differently, so in this
mode they agree to the bf16 bars, not to 1e-5 as in the f32 / f16x3 modes; every one of them is bit-identical when repeated.
"""
import numpy as np
import pytest
import torch

from conftest import drop_profile, get_gpu_model, get_state_dict, golden_inputs, load_golden

pytestmark = pytest.mark.gpu

FLIP_BAR = 0.035
FLAME_BAR = 5e-2
CASES = ["tiny_4s_s0", "tiny_10s_s1_style", "tiny_6p3s_s2", "full_4s_s2", "full_10s_s1_style", "full_demo_eng1"]


def bf16_error(m, case, name, profile="benign"):
    """(chunk-0 flip rate, chunk-0 FLAME max-abs, whole-clip flip rate, whole-clip FLAME max-abs) of one golden case in bf16 mode"""
    g = load_golden(case)
    cfg, sd = get_state_dict(name, profile)
    audio, style = golden_inputs(g, sd)
    m.set_precision("bf16")
    out = m.inference_batch([audio], [style], return_aux=True)[0].cpu().numpy()
    assert m._precision == "bf16" and m.status() == 0, f"{case}: status {m.status()} / mode {m._precision} after a bf16 call"
    assert np.isfinite(out).all(), f"{case}: non-finite output in bf16 mode"
    bits = m.last_aux["bits"][0].cpu().numpy()
    gbits = np.unpackbits(g["bits"], axis=-1)
    assert bits.shape == gbits.shape and out.shape == g["out"].shape
    flips = bits != gbits
    err = np.abs(out - g["out"])
    return float(flips[0].mean()), float(err[:100].max()), float(flips.mean()), float(err.max())


@pytest.mark.parametrize("case", CASES)
def test_bf16_error_against_reference_golden(case):
    name = case.split("_")[0]
    m = get_gpu_model(name)
    try:
        f0, e0, fa, ea = bf16_error(m, case, name)
    finally:
        m.set_precision("f32")
    print(f"{case} [bf16]: chunk 0 flips {100 * f0:.2f} % FLAME {e0:.3e}; whole clip flips {100 * fa:.2f} % FLAME {ea:.3e}")
    assert f0 <= FLIP_BAR, f"{case}: chunk 0 AR-bit flip rate {100 * f0:.2f} %"
    assert e0 <= FLAME_BAR, f"{case}: chunk 0 FLAME max-abs {e0:.3e}"


def _clips(sd, secs, seed):
    from artalk_amd.synth import synth_audio, synth_style
    mean, std = sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()
    audios = [torch.from_numpy(synth_audio(seed + i, s)) for i, s in enumerate(secs)]
    styles = [torch.from_numpy(synth_style(seed + i, mean, std)) if i % 2 else None for i in range(len(secs))]
    return audios, styles


def _agree(a_bits, a_out, b_bits, b_out, what):
    """two bf16 runs of one clip that tiled their GEMMs differently: chunk 0 within the bf16 bars of each other, finite everywhere"""
    f0 = (a_bits[0] != b_bits[0]).float().mean().item()
    e0 = (a_out[:100] - b_out[:100]).abs().max().item()
    print(f"{what}: chunk 0 flips {100 * f0:.2f} % FLAME {e0:.3e}; whole clip max-abs {(a_out - b_out).abs().max().item():.3e}")
    assert torch.isfinite(a_out).all() and torch.isfinite(b_out).all()
    assert f0 <= FLIP_BAR and e0 <= FLAME_BAR, f"{what}: chunk 0 flips {100 * f0:.2f} %, FLAME {e0:.3e}"


def test_bf16_batch_equals_single_runs():
    """A ragged batch against single runs of its clips (different tiles and split-K factors, so a different fp32 summation order): within
    the bf16 bars of each other (see the module docstring); the same batch twice and the same single run twice are bit-identical."""
    m = get_gpu_model("tiny")
    cfg, sd = get_state_dict("tiny")
    secs = [4.0, 10.0, 6.3, 1.7, 8.0]
    audios, styles = _clips(sd, secs, 10)
    m.set_precision("bf16")
    try:
        batch = m.inference_batch(audios, styles, return_aux=True)
        bbits = [b.clone() for b in m.last_aux["bits"]]
        for i in range(len(secs)):
            single = m.inference_batch([audios[i]], [styles[i]], return_aux=True)[0].clone()
            sbits = m.last_aux["bits"][0].clone()
            assert batch[i].shape == single.shape == (m.seq_length(audios[i].shape[0]), 106)
            _agree(bbits[i], batch[i], sbits, single, f"clip {i} batch vs single")
            assert torch.equal(single, m.inference_batch([audios[i]], [styles[i]])[0]), f"clip {i}: single run not repeatable"
        again = m.inference_batch(audios, styles)
        assert all(torch.equal(a, b) for a, b in zip(batch, again))
        assert m._precision == "bf16" and m.status() == 0
    finally:
        m.set_precision("f32")


def test_bf16_streaming_equals_batch_call():
    m = get_gpu_model("tiny")
    cfg, sd = get_state_dict("tiny")
    audios, styles = _clips(sd, [10.0, 10.0], 20)
    m.set_precision("bf16")
    try:
        want = m.inference_batch(audios, styles)

        def stream():
            m.stream_begin(2, styles)
            got = []
            for j in range(3):
                chunk = torch.zeros(2, 64000)
                for b in range(2):
                    seg = audios[b][j * 64000:(j + 1) * 64000]
                    chunk[b, :seg.shape[0]] = seg
                got.append(m.stream_chunk(chunk.cuda()).clone())
            m.stream_end()
            return torch.cat(got, dim=1)[:, :250]

        got = stream()
        for b in range(2):
            assert got[b].shape == want[b].shape
            for j in range(3):
                d = (got[b, j * 100:(j + 1) * 100] - want[b][j * 100:(j + 1) * 100]).abs().max().item()
                print(f"clip {b} chunk {j}: streaming vs batch call max-abs {d:.3e}")
                # two bf16 runs, each within FLAME_BAR of the reference: within 2 * FLAME_BAR of each other (the streaming session's
                # encoder GEMMs see one chunk per launch, the batch call's three: every one of them tiles and splits differently)
                assert d <= 2 * FLAME_BAR and bool(torch.isfinite(got[b]).all()), f"clip {b} chunk {j}: {d:.3e}"
        assert torch.equal(got, stream()), "the same streaming session twice must be bit-identical"
        assert m._precision == "bf16" and m.status() == 0
    finally:
        m.set_precision("f32")


@pytest.mark.parametrize("case", ["tiny_10s_s1_style", "full_10s_s1_style"])
def test_bf16_streaming_against_reference_golden(case):
    """Chunk-at-a-time streaming in bf16 against the REFERENCE's golden, chunk by chunk, and against the one-shot call of the same clip:
    the history hand-over of the streaming session in this mode.  Chunk 0 is held to the golden bars; every later chunk, which continues
    from a history both runs already reach through bf16, to 2 * FLAME_BAR of the golden (the batch call measured 3.7e-2 - 7.7e-2 on
    these clips) and to 2 * FLAME_BAR of the batch call.  Measured on MI355X: 2.8e-2 - 8.2e-2 from the golden, 2.1e-2 - 4.0e-2 from the
    batch call."""
    g = load_golden(case)
    name = case.split("_")[0]
    m = get_gpu_model(name)
    cfg, sd = get_state_dict(name)
    audio, style = golden_inputs(g, sd)
    n_chunks = g["bits"].shape[0]
    spc = cfg.samples_per_chunk
    m.set_precision("bf16")
    try:
        batch = m.inference_batch([audio], [style])[0].cpu().numpy()
        m.stream_begin(1, [style])
        for j in range(n_chunks):
            seg = audio[j * spc:(j + 1) * spc]
            chunk = torch.zeros(1, spc)
            chunk[0, :seg.shape[0]] = seg
            out, nv = m.stream_chunk(chunk.cuda(), n_valid=[seg.shape[0]])
            got = out[0, :nv[0]].cpu().numpy()
            assert nv[0] == min(100, g["out"].shape[0] - j * 100) and np.isfinite(got).all()
            e_ref = float(np.abs(got - g["out"][j * 100:j * 100 + nv[0]]).max())
            e_batch = float(np.abs(got - batch[j * 100:j * 100 + nv[0]]).max())
            print(f"{case} [bf16] streaming chunk {j}: FLAME max-abs {e_ref:.3e} vs golden, {e_batch:.3e} vs the batch call")
            assert e_ref <= (FLAME_BAR if j == 0 else 2 * FLAME_BAR), f"{case} chunk {j}: {e_ref:.3e} from the golden"
            assert e_batch <= 2 * FLAME_BAR, f"{case} chunk {j}: {e_batch:.3e} from the batch call"
        m.stream_end()
        assert m._precision == "bf16" and m.status() == 0
    finally:
        m.set_precision("f32")


def _fresh_tiny():
    from artalk_amd.model import BitwiseARModel
    cfg, sd = get_state_dict("tiny")
    m = BitwiseARModel(cfg).eval().to("cuda")
    m.load_state_dict(sd, strict=True)
    return m


def test_bf16_mode_isolation_and_weight_bytes():
    """Switching modes never mixes them: with graphs on and a batch of 8 (two clip groups, so the graph keys of group 1 exist), the f16x3
    and f32 results are bit-identical before and after bf16 calls, and the bf16 result does not depend on which modes ran before it
    (the cached initial history and the captured graphs are per mode).  The bf16 weight copy appears on the first switch: +2 bytes
    per parameter, none before."""
    cfg, sd = get_state_dict("tiny")
    audios, styles = _clips(sd, [4.0, 6.0, 3.0, 5.0, 4.5, 2.0, 7.0, 4.0], 40)
    m = _fresh_tiny()
    w0 = m.weight_bytes()
    m.set_precision("f16x3")
    r16 = [x.clone() for x in m.inference_batch(audios, styles)]
    m.set_precision("f32")
    r32 = [x.clone() for x in m.inference_batch(audios, styles)]
    assert m.weight_bytes() == w0, "a model that never selected bf16 allocated a bf16 copy"
    m.set_precision("bf16")
    assert m.weight_bytes() == w0 + w0 // 2, (m.weight_bytes(), w0)
    rb = [x.clone() for x in m.inference_batch(audios, styles)]
    assert any(not torch.equal(a, b) for a, b in zip(rb, r32)), "bf16 mode computed the f32 result"
    for mode, want in (("f16x3", r16), ("f32", r32), ("bf16", rb), ("f32", r32), ("f16x3", r16), ("bf16", rb)):
        m.set_precision(mode)
        got = m.inference_batch(audios, styles)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{mode} result changed after switching modes"
    assert m.weight_bytes() == w0 + w0 // 2
    # bf16 FIRST on a fresh model: the same bf16 result (its initial history is its own, not the f32 mode's)
    m2 = _fresh_tiny()
    m2.set_precision("bf16")
    got = m2.inference_batch(audios, styles)
    assert all(torch.equal(a, b) for a, b in zip(got, rb))
    m2.set_precision("f32")
    got = m2.inference_batch(audios, styles)
    assert all(torch.equal(a, b) for a, b in zip(got, r32)), "f32 after bf16 differs from f32 on a model that never ran bf16"


@pytest.mark.parametrize("case", ["heavy_tiny_6p3s_s2", "heavy_full_4s_s2"])
def test_bf16_heavy_profile_needs_no_calibration(case):
    """The `heavy` profile trips f16x3's range guard at the default scales; bf16 has fp32's exponent range: no calibration, status 0,
    the mode stays bf16, and the error is within the same bars."""
    import warnings
    profile, name = case.split("_")[0], case.split("_")[1]
    m = get_gpu_model(name, profile)
    try:
        m.reset_scales()
        calib = getattr(m, "_calibrations", 0)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            f0, e0, fa, ea = bf16_error(m, case, name, profile)
        assert not [str(x.message) for x in w if "artalk_amd" in str(x.message)]
        assert getattr(m, "_calibrations", 0) == calib and m._precision == "bf16" and not m._latched_f32
        print(f"{case} [bf16]: chunk 0 flips {100 * f0:.2f} % FLAME {e0:.3e}; whole clip flips {100 * fa:.2f} % FLAME {ea:.3e}")
        assert f0 <= FLIP_BAR and e0 <= FLAME_BAR, (f0, e0)
    finally:
        m.set_precision("f32")
        if name == "full":
            drop_profile(name, profile)
