"""Conv stack over the frames that hear real audio: the geometry (artalk_conv_tail_geometry / _class, host only) against a brute-force
receptive-field computation, and the premise - the rows of a zero-padded chunk that see the padding alone are one row - against the
oracle's conv stack on the CPU."""
import numpy as np
import pytest
import torch

from artalk_amd import capi
from artalk_amd.config import ARTalkConfig

from conftest import get_oracle, get_state_dict

CFG = ARTalkConfig.full()
KERNEL, STRIDE = list(CFG.w2v["conv_kernel"]), list(CFG.w2v["conv_stride"])
SPC = CFG.samples_per_chunk
T_FULL = CFG.w2v_lengths()
VALID = [1, 399, 400, 401, 8000, 31999, 32000, 32001, 63039, 63040, 63041, 64000]


def _fields():
    """Per layer, (first sample, one past the last sample) of every output row's receptive field, by walking the rows of the layer below."""
    lo, hi = np.arange(SPC), np.arange(SPC) + 1
    out = []
    for k, s in zip(KERNEL, STRIDE):
        n = (len(lo) - k) // s + 1
        lo, hi = np.array([lo[s * t] for t in range(n)]), np.array([hi[s * t + k - 1] for t in range(n)])
        out.append((lo, hi))
    return out


FIELDS = _fields()


def _brute(v):
    """t_const per layer (first row whose field starts at or after sample v; the row count if there is none), and - when the last
    layer has a constant row before its last row - the rows each layer must compute for the last layer's rows 0 .. t_const."""
    t_const = []
    for lo, _ in FIELDS:
        at = np.nonzero(lo >= v)[0]
        t_const.append(int(at[0]) if len(at) else None)
    tc = t_const[-1]
    if tc is None or tc >= T_FULL[-1] - 1:
        return t_const, None, None
    need = tc + 1
    rows = [need]
    for k, s in zip(KERNEL[:0:-1], STRIDE[:0:-1]):
        need = (need - 1) * s + k      # rows 0 .. need-1 of a layer read rows 0 .. (need-1) s + k - 1 of the layer below
        rows.append(need)
    rows = rows[::-1]
    samples = int(FIELDS[0][1][rows[0] - 1])
    return t_const, rows, samples


@pytest.mark.parametrize("v", VALID)
def test_geometry_matches_receptive_fields(v):
    partial, t_const, Tp, Sp, read = capi.conv_tail_geometry(v)
    want_const, want_rows, want_read = _brute(v)
    for i, w in enumerate(want_const):
        if w is not None:
            assert t_const[i] == w, (v, i, t_const, want_const)
        else:
            assert t_const[i] >= T_FULL[i], (v, i)      # no row of the chunk starts that late
    assert partial == (want_rows is not None)
    if partial:
        assert Tp == want_rows and read == want_read == 320 * t_const[-1] + 400
        assert Tp[-1] == t_const[-1] + 1 <= T_FULL[-1] - 1
        # every computed row past t_const sees the padding alone; row t_const[-1] of the last layer is such a row
        assert FIELDS[-1][0][t_const[-1]] >= v and read <= SPC
    else:
        assert Tp == T_FULL and read == SPC and Sp[-1] == T_FULL[-1] + 1
    # layout invariants (the strided-GEMM form of the stack): S[i-1] = 2 S[i] holds the rows of layer i-1; one spare row at the top
    assert Sp[-1] == Tp[-1] + 1
    for i in range(1, len(Sp)):
        assert Sp[i - 1] == 2 * Sp[i] and Tp[i - 1] <= 2 * Sp[i] and Tp[i - 1] <= T_FULL[i - 1]
        assert Tp[i - 1] >= (Tp[i] - 1) * STRIDE[i] + KERNEL[i]      # the rows layer i reads exist


def test_counts_as_full_threshold():
    """t_c = ceil(v / 320) >= 198 leaves no constant row to skip: the last partial count is 197 * 320."""
    assert capi.conv_tail_geometry(197 * 320)[0] is True
    assert capi.conv_tail_geometry(197 * 320 + 1)[0] is False
    assert capi.conv_tail_geometry(SPC)[0] is False
    for bad in (0, -5, SPC + 1):
        with pytest.raises(ValueError):
            capi.conv_tail_geometry(bad)
        with pytest.raises(ValueError):
            capi.conv_tail_class(bad)


def test_class_bounds():
    """Classes are quarters of a chunk; a chunk runs at its class's upper bound, which covers it; the last class is the whole chunk."""
    q = SPC // 4
    for v in VALID + [q - 1, q, q + 1, 2 * q, 2 * q + 1, 3 * q, 3 * q + 1]:
        b = capi.conv_tail_class(v)
        assert b in (q, 2 * q, 3 * q, SPC) and b - q < v <= b, (v, b)
        # running at the bound computes every row the chunk itself needs
        pv, _, Tv, _, _ = capi.conv_tail_geometry(v)
        pb, tcb, Tb, _, _ = capi.conv_tail_geometry(b)
        assert all(x <= y for x, y in zip(Tv, Tb))
        if pb:
            assert pv and FIELDS[-1][0][tcb[-1]] >= v      # the bound's representative row is constant for the chunk too
    assert [capi.conv_tail_geometry(k * q)[0] for k in (1, 2, 3, 4)] == [True, True, True, False]
    assert capi.conv_tail_geometry(2 * q)[1][-1] == 100 and capi.conv_tail_geometry(2 * q)[2][-1] == 101


def test_padded_rows_of_the_oracle_conv_stack_agree():
    """The premise, on the reference's arithmetic: one chunk with 8 000 real samples and 56 000 zeros through the oracle's
    feature extractor - every row from t_c = 25 on equals row 25 (to what torch's CPU convolution guarantees: 1e-6)."""
    from artalk_amd.synth import synth_audio
    o = get_oracle("tiny")
    v = 8000
    x = torch.zeros(1, SPC)
    x[0, :v] = torch.from_numpy(synth_audio(3, v / 16000.0))[:v]
    with torch.no_grad():
        h = o.w2v_feature_extractor(o.normalize_audio(x))[0].T.numpy()      # (199, 512)
    tc = capi.conv_tail_geometry(v)[1][-1]
    assert tc == 25 and h.shape[0] == T_FULL[-1]
    tail, rep = h[tc:], h[tc]
    print(f"rows {tc}..{h.shape[0] - 1} vs row {tc}: max |diff| {np.abs(tail - rep).max():.3e}, bit-equal {np.array_equal(tail, np.broadcast_to(rep, tail.shape))}")
    assert np.allclose(tail, rep, rtol=0.0, atol=1e-6)
    assert not np.allclose(h[tc - 1], rep, rtol=0.0, atol=1e-6)      # (the row before still hears the clip)
