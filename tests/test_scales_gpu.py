"""Portable f16x3 site scales on the GPU: the static site table (artalk_scale_sites) against the audit, the setter's semantics
(artalk_set_site_scales), a calibration saved by one model and loaded by a fresh one, streaming with loaded scales, the streaming
range trip that recalibrates instead of latching f32, the all-or-nothing artalk_calibrate, the engine's ``calibration`` argument and
``dist.agree_scales`` over RCCL at world size 1.

Models from conftest.get_gpu_model are shared with the other test files: every test that changes one restores it in ``finally``."""
import ctypes as C
import gc
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import (FLAME_TOL, assert_clip_parity, dense_margins, drop_profile, get_gpu_model, get_state_dict, golden_inputs,
                      load_golden)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restore(m):
    m.stream_end()
    m.reset_scales()
    m.set_precision("f32")
    m.auto_calibrate = True
    m.check_finite = True


def _audit_names(m, audio, style):
    """Site names one exact-f32 audit pass over this clip reports (artalk_get_audit)."""
    from artalk_amd import capi
    L = capi.lib()
    m.set_precision("f32")
    cache = m.style_cache_size
    m.style_cache_size = 0          # a style clip seen by an earlier test would pass as its cached condition: the encoder must run
    assert L.artalk_set_audit(m._h, 1) == capi.OK
    try:
        m.inference_batch([audio], [style])
        buf = C.create_string_buffer(1 << 16)
        vals = (C.c_float * 1024)()
        n = L.artalk_get_audit(m._h, buf, len(buf), vals, 1024)
        assert n > 0
    finally:
        L.artalk_set_audit(m._h, 0)
        m.style_cache_size = cache
    return [x.decode() for x in buf.raw.split(b"\0")[:n]]


@pytest.mark.parametrize("name,case", [("tiny", "tiny_10s_s1_style"), ("full", "full_5p5s_s3_style")])
def test_site_table_equals_audit(name, case):
    """The table built from the config alone names exactly the sites an audit pass over a styled clip of two or more chunks (style
    encoder and re-encoder included) reports; the audit keeps its first-seen order, the table its own; fresh models hold 4 everywhere."""
    from artalk_amd import capi
    g = load_golden(case)
    assert bool(g["with_style"]) and g["bits"].shape[0] >= 2
    m = get_gpu_model(name)
    cfg, sd = get_state_dict(name)
    audio, style = golden_inputs(g, sd)
    try:
        table = m._site_names()
        assert len(table) == len(set(table)) == capi.lib().artalk_scale_sites(m._h, None, 0)
        assert set(m.scales().values()) == {4}
        audited = _audit_names(m, audio, style)
        assert len(audited) == len(set(audited))
        assert set(table) == set(audited), (sorted(set(table) - set(audited))[:8], sorted(set(audited) - set(table))[:8])
        small = C.create_string_buffer(16)
        assert capi.lib().artalk_scale_sites(m._h, small, len(small)) == capi.EINVAL
    finally:
        _restore(m)
    print(f"{name}: {len(table)} sites in the table = the audit's")


def test_set_site_scales_semantics():
    from artalk_amd import capi
    from artalk_amd.synth import synth_audio
    L = capi.lib()
    m = get_gpu_model("tiny")
    audio = torch.from_numpy(synth_audio(41, 6.0))
    try:
        m.reset_scales()
        m.set_precision("f16x3")
        want = m.inference_batch([audio])[0].clone()
        assert m.status() == 0 and m.graph_count()[0] > 0
        names = m._site_names()
        n = len(names)
        base = m.scales()
        assert list(base) == names and set(base.values()) == {4}
        low = dict(base)
        for k, e in (("w2v.layer1.ffn_hidden", 2), ("ar.block0.ln1_mod", 1), ("vae.decoder.layer0.qkv", 0)):
            low[k] = e
        exps = (C.c_int * (n + 1))(*[low[k] for k in names], 4)
        assert L.artalk_set_site_scales(m._h, exps, n) == 3
        got = (C.c_int * n)()
        assert L.artalk_get_site_scales(m._h, got, n) == capi.OK and list(got) == [low[k] for k in names]
        assert m.graph_count()[0] == 0, "the graphs captured with the old exponents must be dropped"
        m.inference_batch([audio])
        held = m.graph_count()[0]
        assert held > 0
        assert L.artalk_set_site_scales(m._h, exps, n) == 0 and m.graph_count()[0] == held      # same values: a no-op
        # bad arguments: nothing changes
        bad = (C.c_int * (n + 1))(*list(exps))
        for count in (n - 1, n + 1):
            assert L.artalk_set_site_scales(m._h, bad, count) == capi.EINVAL
            assert L.artalk_get_site_scales(m._h, got, count) == capi.EINVAL
        for e in (5, -9):
            bad[3] = e
            assert L.artalk_set_site_scales(m._h, bad, n) == capi.EINVAL
        assert m.scales() == low and m.graph_count()[0] == held
        # everything back to 4: bit-identical to the untouched model
        assert m.load_scales(base) == 3
        assert torch.equal(m.inference_batch([audio])[0], want) and m.status() == 0
        # a change during a streaming session ends it: the next chunk fails in the library
        m.stream_begin(1)
        chunk = audio[None, :64000].cuda()
        m.stream_chunk(chunk)
        assert L.artalk_set_site_scales(m._h, exps, n) == 3
        with pytest.raises(RuntimeError, match="site scales changed"):
            m.stream_chunk(chunk)
    finally:
        _restore(m)


# ---------------------------------------------------------------------------------------------- heavy profile: saved -> loaded
def _parity(case, name, m, g, audio, style):
    out = m.inference_batch([audio], [style], return_aux=True)[0].cpu().numpy()
    aux = m.last_aux
    return assert_clip_parity(case, "f16x3", out, aux["bits"][0].cpu().numpy(), aux["hist_bits"][0].cpu().numpy(), g["out"],
                              np.unpackbits(g["bits"], axis=-1), np.unpackbits(g["hist_bits"], axis=-1), dense_margins(g["logit_margin"]),
                              dense_margins(g["hist_margin"]), inputs=((name, "heavy"), audio, style))


def _fresh_model(name, profile):
    from artalk_amd.model import BitwiseARModel
    cfg, sd = get_state_dict(name, profile)
    m = BitwiseARModel(cfg).eval().to("cuda")
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def heavy_tiny_scales(tmp_path_factory):
    """The heavy tiny model's scales calibrated on its golden clip, saved once for the tests below."""
    g = load_golden("heavy_tiny_6p3s_s2")
    m = get_gpu_model("tiny", "heavy")
    cfg, sd = get_state_dict("tiny", "heavy")
    audio, style = golden_inputs(g, sd)
    path = str(tmp_path_factory.mktemp("scales") / "heavy_tiny.json")
    try:
        m.reset_scales()
        assert m.calibrate([audio], [style]) > 0
        m.save_scales(path)
    finally:
        _restore(m)
    return path


@pytest.mark.parametrize("case", ["heavy_tiny_6p3s_s2", "heavy_full_4s_s2"])
def test_saved_calibration_loads_into_a_fresh_model(case, tmp_path):
    g = load_golden(case)
    name = case.split("_")[1]
    a = get_gpu_model(name, "heavy")
    cfg, sd = get_state_dict(name, "heavy")
    audio, style = golden_inputs(g, sd)
    path = str(tmp_path / "scales.json")
    b = None
    try:
        a.reset_scales()
        a.set_precision("f16x3")
        assert a.calibrate([audio], [style]) > 0
        a.save_scales(path)
        want = a.inference_batch([audio], [style])[0].clone()
        assert a.status() == 0 and a._precision == "f16x3"
        b = _fresh_model(name, "heavy")
        assert b.load_scales(path) > 0 and b.scales() == a.scales()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = b.inference_batch([audio], [style])[0]
            st = b.status()
        assert not w, [str(x.message) for x in w]
        assert st == 0 and b._precision == "f16x3" and not b._latched_f32 and getattr(b, "_calibrations", 0) == 0
        assert torch.equal(got, want), "a model that loaded the scales must compute what the calibrated model computes"
        good, n, err = _parity(case, name, b, g, audio, style)
        assert b.status() == 0 and getattr(b, "_calibrations", 0) == 0
    finally:
        _restore(a)
        del b
        gc.collect()
        if name == "full":
            drop_profile("full", "heavy")
    print(f"{case}: loaded scales, first f16x3 call status 0 without calibrating, chunks exact {good}/{n}, FLAME err {err:.3e}")


def _stream_parity(m, g, audio, style):
    """One streaming session over the clip: status 0 and no warning after every chunk, every chunk's codes within FLAME_TOL."""
    spc = m.cfg.samples_per_chunk
    n_chunks = g["bits"].shape[0]
    assert n_chunks >= 2
    m.stream_begin(1, [style])
    worst = 0.0
    for j in range(n_chunks):
        seg = audio[j * spc:(j + 1) * spc]
        chunk = torch.zeros(1, spc)
        chunk[0, :seg.shape[0]] = seg
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out, nv = m.stream_chunk(chunk.cuda(), n_valid=[seg.shape[0]])
            st = m.status()
        assert not w and st == 0 and m._precision == "f16x3", (j, st, [str(x.message) for x in w])
        err = float(np.abs(out[0, :nv[0]].cpu().numpy() - g["out"][j * 100:j * 100 + nv[0]]).max())
        assert err < FLAME_TOL, f"streaming chunk {j}: FLAME max-abs err {err:.3e}"
        worst = max(worst, err)
    m.stream_end()
    return worst


def test_streaming_with_loaded_scales(heavy_tiny_scales):
    g = load_golden("heavy_tiny_6p3s_s2")
    m = get_gpu_model("tiny", "heavy")
    cfg, sd = get_state_dict("tiny", "heavy")
    audio, style = golden_inputs(g, sd)
    try:
        m.reset_scales()
        m.set_precision("f16x3")
        assert m.load_scales(heavy_tiny_scales) > 0
        before = getattr(m, "_calibrations", 0)
        err = _stream_parity(m, g, audio, style)
        assert getattr(m, "_calibrations", 0) == before
    finally:
        _restore(m)
    print(f"heavy tiny streaming with loaded scales: status 0 on every chunk, FLAME max-abs err {err:.3e}")


def test_streaming_trip_recalibrates():
    g = load_golden("heavy_tiny_6p3s_s2")
    m = get_gpu_model("tiny", "heavy")
    cfg, sd = get_state_dict("tiny", "heavy")
    audio, style = golden_inputs(g, sd)
    spc = cfg.samples_per_chunk
    try:
        m.reset_scales()
        m.set_precision("f16x3")
        assert m.auto_calibrate
        m.stream_begin(1, [style])
        with pytest.raises(RuntimeError, match="begin the streaming session again") as e:
            m.stream_chunk(audio[None, :spc].cuda())
        assert "recalibrated" in str(e.value)
        assert m._precision == "f16x3" and not m._latched_f32
        low = {k: v for k, v in m.scales().items() if v != 4}
        assert low and all(k.startswith("w2v.layer") and k.endswith(".ffn_hidden") for k in low), low
        err = _stream_parity(m, g, audio, style)
    finally:
        _restore(m)
    print(f"heavy tiny streaming trip: recalibrated {len(low)} sites on the chunk, new session FLAME max-abs err {err:.3e}")


def test_calibrate_is_all_or_nothing():
    """An early site that would be lowered (conv0's LayerNorm gain x1e4) and a later one that no exponent can hold (the feature-projection
    LayerNorm x1e8 -> ~3e8 > 65504 * 2^8; the projection x1e-8 keeps the f32 pass finite): artalk_calibrate fails and changes nothing."""
    from artalk_amd import capi
    from artalk_amd.model import BitwiseARModel
    from artalk_amd.synth import synth_audio
    L = capi.lib()
    cfg, sd = get_state_dict("tiny")
    big = dict(sd)
    k0 = "audio_encoder.feature_extractor.conv_layers.0.layer_norm.weight"
    big[k0] = sd[k0] * 1e4
    k = "audio_encoder.feature_projection.layer_norm.weight"
    big[k] = sd[k] * 1e8
    kk = "audio_encoder.feature_projection.projection.weight"
    big[kk] = sd[kk] * 1e-8
    m = BitwiseARModel(cfg).eval().to("cuda")
    try:
        m.load_state_dict(big, strict=True)
        audio = torch.from_numpy(synth_audio(3, 4.0))
        m.set_precision("f32")
        m.inference_batch([audio])
        graphs = m.graph_count()[0]
        assert L.artalk_set_audit(m._h, 1) == capi.OK
        m.inference_batch([audio])
        rc = L.artalk_calibrate(m._h, C.c_float(4.0))
        L.artalk_set_audit(m._h, 0)
        assert rc == capi.EINVAL, rc
        assert "exceeds every supported scale" in m._err()
        assert set(m.scales().values()) == {4} and m.graph_count()[0] == graphs
        with pytest.raises(RuntimeError, match="artalk_calibrate failed"):
            m.calibrate([audio])
        assert set(m.scales().values()) == {4}
    finally:
        del m
        gc.collect()


def test_engine_calibration_argument(heavy_tiny_scales):
    from artalk_amd.engine import ARTAvatarInferEngine
    g = load_golden("heavy_tiny_6p3s_s2")
    cfg, sd = get_state_dict("tiny", "heavy")
    audio, style = golden_inputs(g, sd)
    eng = ARTAvatarInferEngine(state_dict=sd, config=cfg, calibration=heavy_tiny_scales)
    try:
        m = eng.ARTalk
        assert getattr(m, "_calibrations", 0) == 0 and {v for v in m.scales().values()} != {4}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            pred = eng.inference(audio)
            st = m.status()
        assert not w, [str(x.message) for x in w]
        assert st == 0 and m._precision == "f16x3" and getattr(m, "_calibrations", 0) == 0
        assert pred.shape == (min(750, g["out"].shape[0]), 106)
    finally:
        del eng
        gc.collect()


_AGREE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
import torch.distributed as dist
from artalk_amd.config import ARTalkConfig
from artalk_amd.dist import agree_scales, init_single_process_group
from artalk_amd.model import BitwiseARModel
from artalk_amd.weights import generate_state_dict
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
init_single_process_group("nccl", dev)
cfg = ARTalkConfig.tiny()
m = BitwiseARModel(cfg).eval().to(dev)
m.load_state_dict(generate_state_dict(cfg), strict=True)
s = m.scales()
s["w2v.layer0.ffn_hidden"] = -2
assert m.load_scales(s) == 1
before = m.scales()
changed = agree_scales(m)
assert changed == 0 and m.scales() == before, (changed, m.scales() == before)
dist.destroy_process_group()
print("AGREE_OK", len(before))
"""


def test_agree_scales_rccl_world1():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-c", _AGREE_CHILD, REPO], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0 and "AGREE_OK" in p.stdout, p.stderr[-3000:]
