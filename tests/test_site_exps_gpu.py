"""Every f16x3 site at a non-default exponent, with the result checked.

The site exponent e of a P8 producer (csrc/common.h: hi = f16(x * 2^e), lo = f16(x * 2^e - hi)) has to be removed by every consumer
of that buffer.  All launch parameters default to 4 and the benign goldens run with 4 everywhere, so a call site that forgets its
exponent - or passes its neighbour's - is bit-identical to correct code until a calibration lowers that one site.  Here the whole
site table is SCRAMBLED: three deterministic patterns e_k(name) = 1 + crc32(name + salt_k) % 3 give every site a value in {1, 2, 3}:
  * never the default 4, so a forgotten argument is a factor 2 .. 8 at that site;
  * two given sites agree in all three patterns with probability 1/27; the salts are chosen so that no two NEIGHBOURS of the site
    table do (the table lists the sites in data-flow order - conv0 -> conv1 ..., ln1 -> qkv -> attn_out -> ln2 -> ffn_hidden, layer
    i -> layer i + 1, ln -> qkv -> attn_out -> residual -> mlp_hidden - so the producer and the consumer site of one GEMM / attention
    launch are neighbours); the test asserts it;
  * lowering e only adds range, so benign clips cannot trip the guard; and at e >= 1 the fp16 subnormal quantum of the lo half is
    2^-24 / 2^e <= 2^-25 absolute, so a correct library keeps the accuracy it has at 4.
The bars are the project's own (conftest.assert_clip_parity: decisions exact, FLAME_GUARD on the codes, rounding-level flips held to the
forced-decision continuation and pinned per tag in tests/golden/rounding_level_expected.json).

Models from conftest.get_gpu_model are shared with the other test files: every test restores them in ``finally``."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from conftest import (FLAME_GUARD, assert_clip_parity, clip_set_inputs, dense_margins, get_gpu_model, get_state_dict, golden_inputs,
                      load_clip_set, load_golden)

pytestmark = pytest.mark.gpu

SALTS = {"A": "#A255", "B": "#B6042", "C": "#C54"}
STYLED = [("tiny", "tiny_10s_s1_style"), ("full", "full_5p5s_s3_style")]


def pattern(names, k):
    return {n: 1 + zlib.crc32((n + SALTS[k]).encode()) % 3 for n in names}


def linked_pairs(names):
    """Sites one launch can touch as producer and consumer: neighbours in the site table (see the module docstring).
    Why neighbours are enough: the launch sequence of a layer is ONE piece of code run for every layer, so a swap inside it (E.ln1 where
    E.ln2 belongs) is wrong in every layer at once, and two roles that happen to hold equal values in all three patterns in one layer
    (1 chance in 27) differ in most others.  Sites used from many places - ar.silu_cond, ar.history_tokens, the "(fp32 A)" inputs - are
    paired with their table neighbours only: some of them equal some far-away site in all three patterns (ar.silu_cond and
    ar.block7.ln1_mod, ar.history_tokens and ar.block0.attn_out), which would hide that one confusion only if it were written for that
    single layer; confusing them in the shared per-layer code is again visible in the other layers."""
    return list(zip(names, names[1:]))


def _restore(m):
    m.stream_end()
    m.reset_scales()
    m.set_precision("f32")
    m.auto_calibrate = True
    m.check_finite = True


class _scrambled:
    """The model in f16x3 mode with pattern k loaded, nothing allowed to rewrite the exponents, the style-clip cache off (the style
    encoder runs in every call); everything is put back on exit."""

    def __init__(self, m, k):
        self.m, self.k = m, k

    def __enter__(self):
        m = self.m
        self.cache = m.style_cache_size
        m.style_cache_size = 0
        m._style_cache.clear()
        m.reset_scales()
        m.set_precision("f16x3")
        m.auto_calibrate = False
        self.want = pattern(m._site_names(), self.k)
        assert m.load_scales(self.want) == len(self.want)
        self.calibrations = getattr(m, "_calibrations", 0)
        return self

    def check(self):
        m = self.m
        assert m.status() == 0 and m._precision == "f16x3" and not m._latched_f32
        assert m.scales() == self.want and getattr(m, "_calibrations", 0) == self.calibrations

    def __exit__(self, *exc):
        self.m.style_cache_size = self.cache
        self.m._style_cache.clear()
        _restore(self.m)
        return False


def _clip_parity(tag, m, g, config_name, audio, style, clip=0, out=None):
    aux = m.last_aux
    return assert_clip_parity(tag, "f16x3", out, aux["bits"][clip].cpu().numpy(), aux["hist_bits"][clip].cpu().numpy(), g["out"],
                              np.unpackbits(g["bits"], axis=-1), np.unpackbits(g["hist_bits"], axis=-1), dense_margins(g["logit_margin"]),
                              dense_margins(g["hist_margin"]), inputs=(config_name, audio, style))


# ------------------------------------------------------------------------------------------------------------------ the patterns
@pytest.mark.parametrize("name", ["tiny", "full"])
def test_patterns_cover_every_site(name):
    m = get_gpu_model(name)
    names = m._site_names()
    assert len(names) == len(set(names)) and set(m.scales()) == set(names)
    pats = [pattern(names, k) for k in "ABC"]
    for p in pats:
        assert set(p) == set(names) and set(p.values()) <= {1, 2, 3}, "every site at a non-default exponent inside the calibrated range"
        assert set(p.values()) == {1, 2, 3}
    same = [(a, b) for a, b in linked_pairs(names) if all(p[a] == p[b] for p in pats)]
    assert not same, f"producer / consumer sites that hold equal exponents in all three patterns: {same}"
    # the table is in the data-flow order the pairs are derived from
    for chain in (["w2v.layer0." + s for s in ("ln1", "qkv", "attn_out", "ln2", "ffn_hidden")],
                  ["ar.block1." + s for s in ("ln1_mod", "attn_out", "ln2_mod", "ffn_hidden")],
                  ["vae.decoder.layer0." + s for s in ("ln", "qkv", "attn_out", "residual", "mlp_hidden")],
                  ["w2v.conv0.ln_gelu", "w2v.conv1.ln_gelu"], ["w2v.feature_projection.ln", "w2v.posconv.input(fp32 A)", "w2v.layer0.ln1"]):
        i = names.index(chain[0])
        assert names[i:i + len(chain)] == chain


# ------------------------------------------------------------------------------------------------------------------ single clips
@pytest.mark.parametrize("k", ["A", "B", "C"])
@pytest.mark.parametrize("name,case", STYLED)
def test_scrambled_styled_clip_one_shot_and_streaming(name, case, k):
    """A styled clip of two or more chunks (style encoder, every scale step, decoder and re-encoder run) with pattern k: the one-shot
    call against the reference golden, then the same clip chunk by chunk through a streaming session against the same codes."""
    g = load_golden(case)
    assert bool(g["with_style"]) and g["bits"].shape[0] >= 2
    m = get_gpu_model(name)
    cfg, sd = get_state_dict(name)
    audio, style = golden_inputs(g, sd)
    spc = cfg.samples_per_chunk
    n_chunks = g["bits"].shape[0]
    with _scrambled(m, k) as s:
        out = m.inference_batch([audio], [style], return_aux=True)[0].cpu().numpy()
        s.check()
        good, n, err = _clip_parity(f"{case} scrambled{k} (one-shot)", m, g, name, audio, style, out=out)
        want = assert_clip_parity.last_expected_out if assert_clip_parity.last_rounding_level else g["out"]
        assert want.shape == g["out"].shape
        m.stream_begin(1, [style])
        worst, frames = 0.0, 0
        for j in range(n_chunks):
            seg = audio[j * spc:(j + 1) * spc]
            chunk = torch.zeros(1, spc)
            chunk[0, :seg.shape[0]] = seg
            o, nv = m.stream_chunk(chunk.cuda(), n_valid=[seg.shape[0]])
            s.check()
            e = float(np.abs(o[0, :nv[0]].cpu().numpy() - want[j * 100:j * 100 + nv[0]]).max())
            print(f"{case} scrambled{k} streaming chunk {j}: FLAME max-abs err {e:.3e}")
            assert e < FLAME_GUARD, f"{case} scrambled{k} streaming chunk {j}: FLAME max-abs err {e:.3e}"
            worst, frames = max(worst, e), frames + nv[0]
        m.stream_end()
        assert frames == g["out"].shape[0]
    print(f"{case} scrambled{k}: chunks exact {good}/{n}, FLAME max-abs err one-shot {err:.3e}, streaming {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ batches
def test_scrambled_batch32_full():
    """Pattern A on the batch-32 full-size workload of test_config2_batch32_synthetic_10s (M = 19200 rows in the encoder): only there do
    the big-tile GEMM kernels, the deferred-residual path and the wide / ping-pong attention kernels take the launches."""
    from artalk_amd.synth import synth_audio, synth_style
    clips = load_clip_set("full_cfg2_synth8")
    cfg, sd = get_state_dict("full")
    mean, std = sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()
    audios = [torch.from_numpy(synth_audio(s, 10.0)) for s in range(32)]
    styles = [torch.from_numpy(synth_style(s, mean, std)) if (s % 2 == 1 and (s < 8 or s % 5 == 0)) else None for s in range(32)]
    m = get_gpu_model("full")
    worst, rounding = 0.0, []
    with _scrambled(m, "A") as s:
        outs = m.inference_batch(audios, styles, return_aux=True)
        s.check()
        aux = m.last_aux
        for i, c in enumerate(clips):
            good, n, err = assert_clip_parity(f"cfg2 clip {i} scrambledA", "f16x3", outs[i].cpu().numpy(), aux["bits"][i].cpu().numpy(),
                                              aux["hist_bits"][i].cpu().numpy(), c["out"], c["bits"], c["hist_bits"], c["logit_margin"],
                                              c["hist_margin"], inputs=("full", audios[i], styles[i]))
            worst = max(worst, err)
            if assert_clip_parity.last_rounding_level:
                rounding.append(i)
    print(f"configs[2] scrambledA: 8 golden clips decision-exact, worst FLAME max-abs err {worst:.3e}; rounding_level_clips = {rounding}")


def test_scrambled_ragged_batch_tiny():
    """Pattern B on a ragged batch of three clips of 1 / 3 / 2 chunks (with and without style) of the tiny config: several clip groups,
    the small-grid GEMM kernels with split-K."""
    cases = ["tiny_4s_s0", "tiny_10s_s1_style", "tiny_6p3s_s2"]
    gs = [load_golden(c) for c in cases]
    assert sorted(g["bits"].shape[0] for g in gs) == [1, 2, 3]
    m = get_gpu_model("tiny")
    cfg, sd = get_state_dict("tiny")
    ins = [golden_inputs(g, sd) for g in gs]
    worst = 0.0
    with _scrambled(m, "B") as s:
        outs = m.inference_batch([a for a, _ in ins], [st for _, st in ins], return_aux=True)
        s.check()
        for i, (case, g) in enumerate(zip(cases, gs)):
            good, n, err = _clip_parity(f"{case} ragged3 scrambledB", m, g, "tiny", ins[i][0], ins[i][1], clip=i, out=outs[i].cpu().numpy())
            worst = max(worst, err)
    print(f"tiny ragged batch of 3 scrambledB: worst FLAME max-abs err {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ audit
def _audit(m, audio, style, precision):
    """{site: max |x|} of one audit pass over the clip in the given precision mode (artalk_set_audit / artalk_get_audit)."""
    from artalk_amd import capi
    L = capi.lib()
    m.set_precision(precision)
    assert L.artalk_set_audit(m._h, 1) == capi.OK
    try:
        m.inference_batch([audio], [style])
        assert m.status() == 0 and m._precision == precision
        buf = C.create_string_buffer(1 << 16)
        vals = (C.c_float * 1024)()
        n = L.artalk_get_audit(m._h, buf, len(buf), vals, 1024)
        assert n > 0
    finally:
        L.artalk_set_audit(m._h, 0)
    return dict(zip([x.decode() for x in buf.raw.split(b"\0")[:n]], [float(v) for v in vals[:n]]))


def _assert_same_maxima(what, a, b):
    assert set(a) == set(b), what
    for site in a:
        lo, hi = sorted((a[site], b[site]))
        assert np.isfinite(hi) and lo > 0.0 and hi <= 1.01 * lo, f"{what}: audit maximum of {site}: {a[site]:.6g} vs {b[site]:.6g}"


@pytest.mark.parametrize("name,case", STYLED)
def test_audit_under_scrambled_exponents(name, case):
    """The audit's per-site max |x| does not depend on the exponents: under pattern C the f32-mode pass (fp32 buffers) and the f16x3-mode
    pass (P8 buffers, unscaled by the site's exponent) agree within 1 % per site (a wrong exponent is a factor >= 2, the arithmetic
    difference of the modes ~1e-6), and both agree with the maxima measured with 4 everywhere."""
    g = load_golden(case)
    m = get_gpu_model(name)
    cfg, sd = get_state_dict(name)
    audio, style = golden_inputs(g, sd)
    cache = m.style_cache_size
    try:
        m.style_cache_size = 0
        m._style_cache.clear()
        m.auto_calibrate = False
        m.reset_scales()
        base32 = _audit(m, audio, style, "f32")
        base16 = _audit(m, audio, style, "f16x3")
        assert set(base32) == set(m._site_names())
        want = pattern(m._site_names(), "C")
        assert m.load_scales(want) == len(want)
        scr32 = _audit(m, audio, style, "f32")
        scr16 = _audit(m, audio, style, "f16x3")
        assert m.scales() == want
        _assert_same_maxima("f32 vs f16x3 at exponent 4", base32, base16)
        _assert_same_maxima("scrambled: f32 vs f16x3", scr32, scr16)
        _assert_same_maxima("f32: scrambled vs 4", scr32, base32)
        _assert_same_maxima("f16x3: scrambled vs 4", scr16, base32)
    finally:
        m.style_cache_size = cache
        m._style_cache.clear()
        _restore(m)


# ------------------------------------------------------------------------------------------------------------------ calibration
def test_calibrate_from_scrambled_heavy_tiny():
    """artalk_calibrate starting from pattern B on the `heavy` tiny model (encoder FFN hidden activations of ~1.5e4): no exponent goes up,
    every site holds its audited maximum with the headroom, and the heavy golden passes parity at the resulting exponents."""
    headroom = 4.0
    g = load_golden("heavy_tiny_6p3s_s2")
    m = get_gpu_model("tiny", "heavy")
    cfg, sd = get_state_dict("tiny", "heavy")
    audio, style = golden_inputs(g, sd)
    cache = m.style_cache_size
    try:
        m.style_cache_size = 0
        m._style_cache.clear()
        m.reset_scales()
        m.auto_calibrate = False
        before = pattern(m._site_names(), "B")
        assert m.load_scales(before) == len(before)
        m.set_precision("f16x3")
        changed = m.calibrate([audio], [style], headroom=headroom)
        after = m.scales()
        assert changed == sum(after[s] != before[s] for s in before) > 0
        assert all(-8 <= after[s] <= before[s] for s in before), {s: (before[s], after[s]) for s in before if after[s] > before[s]}
        maxima = _audit(m, audio, style, "f32")
        # (the heavy golden clip has no style clip: the style encoder's sites do not run and keep their pattern value)
        assert set(maxima) <= set(after) and len(maxima) >= len(after) - 17 and m.scales() == after
        assert all(after[s] == before[s] for s in after if s not in maxima)
        for site, mx in maxima.items():
            assert mx * 2.0 ** after[site] * headroom < 65504.0, (site, mx, after[site])
        m.set_precision("f16x3")
        out = m.inference_batch([audio], [style], return_aux=True)[0].cpu().numpy()
        assert m.status() == 0 and m._precision == "f16x3" and m.scales() == after
        good, n, err = _clip_parity("heavy_tiny_6p3s_s2 scrambledB (calibrated)", m, g, ("tiny", "heavy"), audio, style, out=out)
    finally:
        m.style_cache_size = cache
        m._style_cache.clear()
        _restore(m)
    lowered = {s: (before[s], after[s]) for s in before if after[s] != before[s]}
    print(f"heavy tiny from scrambledB: {changed} sites lowered {lowered}, chunks exact {good}/{n}, FLAME max-abs err {err:.3e}")
