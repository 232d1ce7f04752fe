"""The four kernels of the GAGAvatar head alone (artalk_op_gaga_*), each in one launch with its outputs inside poisoned guard bands.
They only move and blend fp32 values, so every comparison is exact: bit-equal to the torch CPU statement of tests/gaga_ref.py (which
tests/test_gaga_cpu.py shows to exclude an FMA-contracted variant)."""
import numpy as np
import pytest
import torch

import gaga_cases as gc
import gaga_ref as ref
from artalk_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7.25e9


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


@pytest.mark.parametrize("T,stride,NB", gc.FLAME_INPUT_CASES)
def test_flame_inputs(T, stride, NB):
    g = torch.Generator().manual_seed(T + stride + NB)
    motion = torch.randn(T, stride, generator=g)
    shape = torch.randn(NB - 100, generator=g)
    m, s = motion.cuda(), (shape.cuda() if NB > 100 else None)
    betas, pose = _guarded(T * NB), _guarded(T * 15)
    rc = capi.lib().artalk_op_gaga_flame_inputs(capi.ptr(m), stride, capi.ptr(s), NB, T, capi.ptr(betas[GUARD:]), capi.ptr(pose[GUARD:]),
                                                capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    want_b = torch.cat([shape[None].expand(T, -1), motion[:, :100]], dim=1)
    want_p = torch.zeros(T, 15)
    want_p[:, 6:9] = motion[:, 103:106]
    assert torch.equal(_bits(_take(betas, T * NB, "betas")), _bits(want_b.reshape(-1)))
    assert torch.equal(_bits(_take(pose, T * 15, "full_pose")), _bits(want_p.reshape(-1)))
    assert torch.equal(m.cpu(), motion)


def _forehead(verts, idx_dev, K, state, flag):
    T, V = verts.shape[0], verts.shape[1]
    rc = capi.lib().artalk_op_gaga_forehead(capi.ptr(verts), capi.ptr(idx_dev), K, T, V, capi.ptr(state), capi.ptr(flag), capi.current_stream_ptr())
    assert rc == capi.OK


@pytest.mark.parametrize("K,T,preset", gc.FOREHEAD_CASES)
def test_forehead(K, T, preset):
    V = 97
    g = torch.Generator().manual_seed(100 * K + 10 * T + int(preset))
    verts = torch.randn(T, V, 3, generator=g)
    index = torch.randperm(V, generator=g)[:K].to(torch.int32)
    state0 = torch.randn(1, K, 3, generator=g) if preset else None
    want, want_state = ref.ema_torch(verts, index.long(), state0)

    vbuf = _guarded(T * V * 3)
    vbuf[GUARD:GUARD + T * V * 3] = verts.reshape(-1).cuda()
    sbuf = _guarded(K * 3, fill=0.0)
    if preset:
        sbuf[GUARD:GUARD + K * 3] = state0.reshape(-1).cuda()
    fbuf = torch.tensor([-12345, 1 if preset else 0, -12345], dtype=torch.int32, device="cuda")
    dv = vbuf[GUARD:GUARD + T * V * 3].view(T, V, 3)
    _forehead(dv, index.cuda(), K, sbuf[GUARD:], fbuf[1:])
    torch.cuda.synchronize()
    got = _take(vbuf, T * V * 3, "the vertices").view(T, V, 3)
    assert torch.equal(_bits(got), _bits(want)), "not bit-equal to the torch float32 loop"
    assert torch.equal(_bits(_take(sbuf, K * 3, "the state")), _bits(want_state.reshape(-1)))
    assert fbuf.tolist() == [-12345, 1, -12345]
    rest = torch.ones(V, dtype=torch.bool)
    rest[index.long()] = False
    assert torch.equal(_bits(got[:, rest]), _bits(verts[:, rest])), "a vertex that is not listed changed"
    if not preset:
        assert torch.equal(_bits(got[0]), _bits(verts[0])), "the very first frame is left as it is"
    np_pts, np_state = ref.ema_numpy(verts[:, index.long()].numpy(), None if state0 is None else state0[0].numpy())
    assert np.array_equal(got[:, index.long()].numpy(), np_pts) and np.array_equal(want_state[0].numpy(), np_state)


@pytest.mark.parametrize("preset", (False, True))
def test_forehead_split_calls(preset):
    """7 frames in one call = 3 + 4 in two, bit for bit: the state carries the recurrence across calls."""
    V, K = 97, 68
    g = torch.Generator().manual_seed(5 + int(preset))
    verts = torch.randn(7, V, 3, generator=g)
    index = torch.randperm(V, generator=g)[:K].to(torch.int32).cuda()
    state0 = torch.randn(K, 3, generator=g)

    def run(splits):
        v = verts.cuda().clone()
        state = state0.cuda().clone() if preset else torch.zeros(K, 3, device="cuda")
        flag = torch.tensor([1 if preset else 0], dtype=torch.int32, device="cuda")
        f0 = 0
        for n in splits:
            _forehead(v[f0:f0 + n], index, K, state, flag)
            f0 += n
        torch.cuda.synchronize()
        return v.cpu(), state.cpu()

    a, b = run([7]), run([3, 4])
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert not torch.equal(a[0], verts)


def test_forehead_without_indices_is_a_no_op():
    verts = torch.randn(3, 11, 3).cuda()
    before = verts.clone()
    state, flag = torch.zeros(3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    _forehead(verts, None, 0, state, flag)
    torch.cuda.synchronize()
    assert torch.equal(verts, before) and int(flag[0]) == 0


@pytest.mark.parametrize("F,V,N", gc.MEANS_CASES)
def test_means(F, V, N):
    g = torch.Generator().manual_seed(F + V + N)
    verts, xyz = torch.randn(F, V, 3, generator=g), torch.randn(N, 3, generator=g)
    out, dv, dx = _guarded(F * N * 3), verts.cuda(), xyz.cuda()
    rc = capi.lib().artalk_op_gaga_means(capi.ptr(dv), capi.ptr(dx), capi.ptr(out[GUARD:]), F, V, N, capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    want = torch.cat([verts, xyz[None, V:].expand(F, -1, -1)], dim=1)
    assert torch.equal(_bits(_take(out, F * N * 3, "means")), _bits(want.reshape(-1)))


@pytest.mark.parametrize("mark", gc.FINISH_MARKS)
def test_finish(mark):
    S, F = gc.FINISH_S, 2
    g = torch.Generator().manual_seed(9)
    img = torch.randn(F, 3, S, S, generator=g) * 0.8 + 0.5
    flat = img.view(-1)
    flat[:8] = torch.tensor([-3.0e38, 3.0e38, -1e-30, 0.0, 1.0, 1.0 + 2.0 ** -23, 1e-30, 1.0 - 2.0 ** -24])      # NaN-free extremes
    img[1, :, -1, -1] = torch.tensor([-5.0, 7.0, 0.5])      # the last pixel, inside every watermark
    assert bool((img < 0).any()) and bool((img > 1).any())
    wm = gc.water_mark(*mark) if mark else None
    want = ref.finish_torch(img, wm)
    n = F * 3 * S * S
    buf = _guarded(n)
    buf[GUARD:GUARD + n] = img.reshape(-1).cuda()
    dwm = wm.cuda() if mark else None
    rc = capi.lib().artalk_op_gaga_finish(capi.ptr(buf[GUARD:]), F, S, capi.ptr(dwm), mark[0] if mark else 0, mark[1] if mark else 0,
                                          capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    got = _take(buf, n, "the image").view(F, 3, S, S)
    assert torch.equal(_bits(got), _bits(want)), "not bit-equal to the torch statement"
    outside = torch.ones(S, S, dtype=torch.bool)
    if mark:
        outside[S - mark[0]:, S - mark[1]:] = False
    assert torch.equal(_bits(got[..., outside]), _bits(img.clamp(0, 1)[..., outside])), "a pixel outside the patch is only clamped"
    if mark and mark != (S, S):
        assert not torch.equal(got, img.clamp(0, 1))
