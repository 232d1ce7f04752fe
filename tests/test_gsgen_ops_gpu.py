"""The Gaussian generators' kernels alone (artalk_op_gs_*, artalk_op_conv2d_relu), one launch each, every output between poisoned guard
bands that must stay poisoned.  The layout kernels are exact; the others stay within the project's allowance for a float32 kernel:
max-abs error <= 4 x e32, e32 being the restatement (tests/gsgen_ref.py, tests/styleunet_ref.py) in float32 against float64 on the CPU,
with a floor of one float32 ulp of the attribute's largest value.  Run with -s for error / e32."""
import math

import numpy as np
import pytest
import torch

import gsgen_cases as cases
import gsgen_ref
from artalk_amd import capi
from styleunet_ref import conv2d

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7.25e9
WIDTHS = cases.ATTRS


def _guarded(n):
    """A device buffer of n floats, NaN inside, between two poisoned bands."""
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def _payload(buf, n, what="the kernel"):
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), f"{what} wrote outside its output"
    got = whole[GUARD:GUARD + n]
    assert bool(torch.isfinite(got).all()), f"{what} left an output value unwritten"
    return got


def _pad8(c):
    """A concatenation with direnc is stored with zero channels up to a multiple of 8 (the conv's vector loads)."""
    return (c + 7) // 8 * 8


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# ---- the three layout kernels: exact
@pytest.mark.parametrize("C,P", [(16, 6), (24, 12), (5, 3), (40, 7)])      # (40, 7): two channel tiles, pixels across a tile edge
def test_local_input(C, P):
    f0, enc = _rnd(C + P, C, P, P), _rnd(7, 27)
    W = _pad8(C + 27)
    n = P * P * W
    buf = _guarded(n)
    x = f0.cuda()
    assert capi.lib().artalk_op_gs_local_input(capi.ptr(x), capi.ptr(enc), capi.ptr(buf[GUARD:]), C, P, capi.current_stream_ptr()) == capi.OK
    want = torch.cat([f0, enc[:, None, None].expand(-1, P, P), torch.zeros(W - C - 27, P, P)], dim=0).permute(1, 2, 0).reshape(-1)
    assert torch.equal(_payload(buf, n), want)


@pytest.mark.parametrize("V,Dh,Dg", [(50, 16, 48), (130, 24, 40), (3, 1, 2)])
def test_global_input(V, Dh, Dg):
    hb, f1 = _rnd(V, V, Dh), _rnd(Dg, Dg)
    n = V * (Dh + Dg)
    buf = _guarded(n)
    a, b = hb.cuda(), f1.cuda()
    assert capi.lib().artalk_op_gs_global_input(capi.ptr(a), capi.ptr(b), capi.ptr(buf[GUARD:]), V, Dh, Dg, capi.current_stream_ptr()) == capi.OK
    assert torch.equal(_payload(buf, n), torch.cat([hb, f1[None].expand(V, -1)], dim=1).reshape(-1))


@pytest.mark.parametrize("V,H", [(50, 16), (130, 16), (33, 256), (2, 1)])
def test_concat_dir(V, H):
    feat, enc = _rnd(V + H, V, H), _rnd(9, 27)
    W = _pad8(H + 27)
    n = V * W
    buf = _guarded(n)
    a = feat.cuda()
    assert capi.lib().artalk_op_gs_concat_dir(capi.ptr(a), capi.ptr(enc), capi.ptr(buf[GUARD:]), V, H, capi.current_stream_ptr()) == capi.OK
    assert torch.equal(_payload(buf, n), torch.cat([feat, enc[None].expand(V, -1), torch.zeros(V, W - H - 27)], dim=1).reshape(-1))


# ---- the conv with bias and ReLU on the layer shapes of the cases
def _layer_shapes():
    """(Cin, Cout, k, H, W) of every layer of cases A-D, as the reference has it and as it is launched (the width of a concatenation
    with direnc padded to a multiple of 8), without repeats."""
    seen = []
    for V, Dh, Dg, C, P in cases.CASES.values():
        hid = (Dh + Dg) // 4
        for s in ((C + 27, C // 2, 3, P, P), (_pad8(C + 27), C // 2, 3, P, P), (C // 2, C // 2, 3, P, P), (C // 2, 41, 1, P, P),
                  (Dh + Dg, hid, 1, V, 1), (hid, hid, 1, V, 1), (hid + 27, 128, 1, V, 1), (_pad8(hid + 27), 128, 1, V, 1), (128, 32, 1, V, 1),
                  (128, 1, 1, V, 1), (128, 3, 1, V, 1), (128, 4, 1, V, 1)):
            if s not in seen:
                seen.append(s)
    return seen


def _conv_relu(x, w, b, shape, relu):
    Cin, Cout, k, H, W = shape
    n = H * W * Cout
    buf = _guarded(n)
    xd = x.permute(0, 2, 3, 1).contiguous().float().cuda()
    wd = w.permute(2, 3, 1, 0).contiguous().float().cuda()
    bd = b.float().cuda()
    rc = capi.lib().artalk_op_conv2d_relu(capi.ptr(xd), H * W * Cin, capi.ptr(wd), capi.ptr(buf[GUARD:]), 1, H, W, Cin, Cout, k, capi.ptr(bd), relu,
                                          capi.current_stream_ptr())
    assert rc == capi.OK
    return _payload(buf, n, "the conv").reshape(1, H, W, Cout).permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", _layer_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_conv_bias_relu(shape):
    Cin, Cout, k, H, W = shape
    x = _rnd(Cin + H, 1, Cin, H, W).double()
    w = _rnd(Cout + 3 * Cin, Cout, Cin, k, k).double() * math.sqrt(2.0 / (Cin * k * k))
    b = _rnd(Cout, Cout).double() * 0.1
    with torch.no_grad():
        pre = conv2d(x, w, bias=b)
        want = torch.relu(pre)
        e32 = float((torch.relu(conv2d(x.float(), w.float(), bias=b.float())).double() - want).abs().max())
    got = _conv_relu(x, w, b, shape, 1)
    err = float((got.double() - want).abs().max())
    allowed = cases.allowance(e32, float(want.abs().max()))
    print(f"conv + bias + ReLU {shape}: max-abs error {err:.3e}, e32 {e32:.3e}, error / e32 {err / max(e32, 1e-300):.2f}")
    assert err <= allowed, f"error {err:.3e} > allowed {allowed:.3e}"
    clear = pre < -allowed      # negative beyond any rounding: the ReLU must give an exact zero
    assert bool(clear.any()) and bool((got[clear] == 0.0).all()) and float(got.min()) >= 0.0
    off = _conv_relu(x, w, b, shape, 0)
    assert float((off.double() - pre).abs().max()) <= cases.allowance(e32, float(pre.abs().max())) and float(off.min()) < 0.0


def test_relu_off_is_the_existing_conv():
    """artalk_op_conv2d and the new op with the ReLU off: the same bits (a shape of tests/test_styleunet_ops_gpu.py)."""
    Cin, Cout, k, B, H, W = 64, 32, 3, 2, 16, 16
    x, w, b = _rnd(1, B, H, W, Cin).cuda(), (_rnd(2, k, k, Cin, Cout) / math.sqrt(Cin * k * k)).cuda(), _rnd(3, Cout).cuda()
    old, new = torch.full((B, H, W, Cout), float("nan"), device="cuda"), torch.full((B, H, W, Cout), float("nan"), device="cuda")
    L = capi.lib()
    assert L.artalk_op_conv2d(capi.ptr(x), H * W * Cin, capi.ptr(w), capi.ptr(old), B, H, W, Cin, Cout, k, None, None, 1.0, None, 0, None, capi.ptr(b), 0,
                              None, None, None, capi.current_stream_ptr()) == capi.OK
    assert L.artalk_op_conv2d_relu(capi.ptr(x), H * W * Cin, capi.ptr(w), capi.ptr(new), B, H, W, Cin, Cout, k, capi.ptr(b), 0,
                                   capi.current_stream_ptr()) == capi.OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(old).all()) and torch.equal(old.view(torch.int32), new.view(torch.int32))
    assert float(old.min()) < 0.0


# ---- the two attribute kernels
def _avatar_buffers(rows):
    return {k: _guarded(rows * w) for k, w in WIDTHS.items()}


def _check_attrs(tag, bufs, rows, want, want32):
    for k, w in WIDTHS.items():
        got = _payload(bufs[k], rows * w, tag).reshape(rows, w).double()
        e32 = float((want32[k].double() - want[k]).abs().max())
        err = float((got - want[k]).abs().max())
        allowed = cases.allowance(e32, float(want[k].abs().max()))
        print(f"{tag} {k}: max-abs error {err:.3e}, e32 {e32:.3e}, error / e32 {err / max(e32, 1e-300):.2f}")
        assert err <= allowed, f"{tag} {k}: error {err:.3e} > allowed {allowed:.3e}"
    return got


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("P", [5, 6, 12])
def test_local_attr(P, sign):
    tm = cases.transform_matrix("ABCD"[P % 4])
    o = _rnd(P + sign, P, P, 41) * 1.5
    with torch.no_grad():
        want = gsgen_ref.local_attributes(o.double(), *gsgen_ref.planes(P, tm, torch.float64), float(sign))
        want32 = gsgen_ref.local_attributes(o, *gsgen_ref.planes(P, tm, torch.float32), float(sign))
    bufs = _avatar_buffers(P * P)
    od, tmh = o.cuda(), torch.from_numpy(tm).contiguous()
    rc = capi.lib().artalk_op_gs_local_attr(capi.ptr(od), capi.ptr(tmh), P, sign, 0, *[capi.ptr(bufs[k][GUARD:]) for k in WIDTHS], capi.current_stream_ptr())
    assert rc == capi.OK
    _check_attrs(f"local_attr P {P} sign {sign:+d}", bufs, P * P, want, want32)
    colors = bufs["colors"][GUARD:GUARD + P * P * 32].cpu().reshape(P, P, 32)
    assert torch.equal(colors[:, 3:, :], o[:, 3:, :32]), "a colour outside columns 0..2 must stay raw"
    assert bool(((colors[:, :3, :] > 0) & (colors[:, :3, :] < 1)).all()) and float(o[:, :3, :32].min()) < 0.0


def test_local_attr_row_offset():
    """row0 places the generator's rows inside the avatar arrays: nothing before them is written."""
    P, row0 = 5, 33
    tm = cases.transform_matrix("C")
    o = _rnd(3, P, P, 41)
    bufs = _avatar_buffers(row0 + P * P)
    od, tmh = o.cuda(), torch.from_numpy(tm).contiguous()
    rc = capi.lib().artalk_op_gs_local_attr(capi.ptr(od), capi.ptr(tmh), P, 1, row0, *[capi.ptr(bufs[k][GUARD:]) for k in WIDTHS], capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    for k, w in WIDTHS.items():
        body = bufs[k].cpu()
        assert bool((body[:GUARD] == POISON).all()) and bool((body[GUARD + (row0 + P * P) * w:] == POISON).all())
        assert bool(torch.isnan(body[GUARD:GUARD + row0 * w]).all()) and bool(torch.isfinite(body[GUARD + row0 * w:GUARD + (row0 + P * P) * w]).all())


@pytest.mark.parametrize("V", [33, 130, 700, 9000])      # 700: more rows than a workgroup has threads; 9000: the grid at its cap
def test_global_attr(V):
    raw = {"colors": _rnd(V, V, 32) * 1.5, "opacities": _rnd(V + 1, V, 1), "scales": _rnd(V + 2, V, 3), "rotations": _rnd(V + 3, V, 4)}
    with torch.no_grad():
        want = gsgen_ref.global_attributes({k: v.double() for k, v in raw.items()})
        want32 = gsgen_ref.global_attributes(raw)
    bufs = _avatar_buffers(V)
    dev = {k: v.contiguous().cuda() for k, v in raw.items()}
    rc = capi.lib().artalk_op_gs_global_attr(capi.ptr(dev["colors"]), capi.ptr(dev["opacities"]), capi.ptr(dev["scales"]), capi.ptr(dev["rotations"]), V,
                                             *[capi.ptr(bufs[k][GUARD:]) for k in WIDTHS], capi.current_stream_ptr())
    assert rc == capi.OK
    _check_attrs(f"global_attr V {V}", bufs, V, want, want32)
    assert float(bufs["xyz"][GUARD:GUARD + 3 * V].abs().max()) == 0.0
    rot = bufs["rotations"][GUARD:GUARD + 4 * V].cpu().reshape(V, 4).double()
    assert float((rot.norm(dim=0) - 1.0).abs().max()) < 1e-5 and float((rot.norm(dim=1) - 1.0).abs().max()) > 0.1
