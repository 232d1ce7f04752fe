"""Every kernel of attention.hip at its key-block, query-tile and dispatch edges: the cases of tests/attn_cases.py, one launch each through
artalk_op_attention_rows_cus, which reports the kernel that ran - a case that ran as another kernel than the one it names fails.

(a) float64.  The reference is softmax(scale * q k^T [+ mask]) v in float64 of the values the kernel is given (for P8 rows: of the unpacked
    P8 words).  Bars, the project's own: fp32 O |err| < 2e-5 (test_ops_gpu.py::test_attention, outputs of magnitude ~1), P8 O
    p8_format.bound(ref, e) + 2e-5 * max|ref| with status word 0 (test_p8_exps_ops_gpu.py::test_attention_f32_rows_p8_output).
(b) poison.  Q, K, V lie in buffers of pitch H * HD + 64 with two more rows per clip than Lq / Lk and one more clip than B; the pitch gap,
    the surplus rows and the surplus clip hold NaN (P8 rows: the fp16 NaN 0x7E00 in every half), the sizes given end at the last valid
    element, O (laid out the same way) is prefilled with 0xABABABAB.  The result is finite and every word of O outside
    [clip < B][row < Lq][column < H * HD] still holds the fill - the surplus clip included, which is where a workgroup that should have
    returned (a (clip, head) pair past B * H) would read and write.
(c) bit identity of the wide, ping-pong and both wide-AR forms with the 64-query f16 kernel: ARTALK_ATTN_WIDE is read once per process,
    so the whole table runs once in a child with ARTALK_ATTN_WIDE=0 (which writes every O buffer into one .npz) and once in a child with
    ARTALK_ATTN_WIDE=1 (which compares against it): two children in all.
(d) peaked softmax: see test_peaked_softmax."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch      # before the library is loaded, as in every GPU test file: torch brings its own HIP runtime
import torch.nn.functional as F

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
                if p not in sys.path]      # (for the child processes of (c), which run this file as a script)
import attn_cases as ac  # noqa: E402
import p8_format as p8  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -1414812757        # 0xABABABAB
NAN_F32 = 0x7FC00000
NAN_P8 = 0x7E007E00       # two fp16 NaNs: every hi and every lo half of a poisoned group


def _embed(x, rows, ld, p8rows):
    """float32 [B, L, D] -> int32 words [B + 1, rows, ld]: the values (P8 rows: packed at QKV_EXP) in the corner, NaN everywhere else"""
    B, L, D = x.shape
    buf = np.full((B + 1, rows, ld), NAN_P8 if p8rows else NAN_F32, dtype=np.int32)
    buf[:B, :L, :D] = p8.pack(x, ac.QKV_EXP) if p8rows else x.view(np.int32)
    return buf


def _given(x, p8rows):
    """what the kernel is given, in float64"""
    return p8.unpack(p8.pack(x, ac.QKV_EXP), ac.QKV_EXP) if p8rows else x.astype(np.float64)


def _heads(x, H, HD, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(x.shape[0], x.shape[1], H, HD).transpose(1, 2)


def reference(c, Q, K, V, qs, scale, dtype):
    """the formula of test_rows_ops_gpu.py::_attn_ref in `dtype` on the CPU -> float64 numpy [B, Lq, H * HD]"""
    q, k, v = (_heads(t, c.H, c.HD, dtype) for t in (Q, K, V))
    if qs is not None:
        q = F.normalize(q, dim=-1) * torch.from_numpy(qs).to(dtype).view(1, c.H, 1, 1)
        k = F.normalize(k, dim=-1)
    s = q @ k.transpose(-1, -2) * scale
    if c.split:
        mask = torch.zeros(c.Lq, c.Lk, dtype=dtype)
        mask[:c.split, c.split:] = -float("inf")
        s = s + mask
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(c.B, c.Lq, c.H * c.HD).double().numpy()


def run_case(L, c, index):
    """one launch -> (O words [B + 1, Lq + 2, ld] int32, kernel that ran, status word, the float32 inputs)"""
    Q, K, V, qs, scale = ac.make_inputs(c, index)
    lay, p8rows = ac.layout(c), bool(c.flags & 4)
    ld = lay["ld"]
    dq, dk, dv = (torch.from_numpy(_embed(x, x.shape[1] + ac.PAD_ROWS, ld, p8rows)).cuda() for x in (Q, K, V))
    dqs = None if qs is None else torch.from_numpy(qs).cuda()
    o = torch.full((c.B + 1, c.Lq + ac.PAD_ROWS, ld), FILL, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    used = C.c_int32(-7)
    rc = L.artalk_op_attention_rows_cus(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), o.data_ptr(), c.B, c.H, c.HD, c.Lq, c.Lk, scale, c.flags,
                                        None if dqs is None else dqs.data_ptr(), c.split, ac.QKV_EXP, c.o_exp, c.out_p8, st.data_ptr(), ld, ld, ld, ld,
                                        lay["qbs"], lay["kbs"], lay["kbs"], lay["qbs"], lay["qn"], lay["kn"], lay["kn"], lay["qn"], c.cus,
                                        C.byref(used), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o.cpu().numpy(), used.value, int(st.item()), (Q, K, V, qs, scale)


def check_poison(c, words, what):
    D = c.H * c.HD
    outside = np.ones(words.shape, dtype=bool)
    outside[:c.B, :c.Lq, :D] = False
    assert bool((words[outside] == FILL).all()), (what, "a word outside the rows and columns of O was written")
    own = words[:c.B, :c.Lq, :D]
    vals = p8.unpack(own, c.o_exp) if c.out_p8 else own.view(np.float32).astype(np.float64)
    assert bool(np.isfinite(vals).all()), (what, "not finite")
    return vals


def _lib():
    from artalk_amd import capi
    return capi.lib()


_INDEX = {c: i for i, c in enumerate(ac.ALL)}


@pytest.mark.parametrize("c", ac.CASES, ids=ac.case_id)
def test_edge_case_against_float64_with_poisoned_surroundings(c):
    what = ac.case_id(c)
    words, used, status, (Q, K, V, qs, scale) = run_case(_lib(), c, _INDEX[c])
    assert used == c.kernel, (what, "ran as", ac.KERNELS[used] if 0 <= used < 9 else used)
    got = check_poison(c, words, what)
    p8rows = bool(c.flags & 4)
    ref = reference(c, _given(Q, p8rows), _given(K, p8rows), _given(V, p8rows), qs, scale, torch.float64)
    err = np.abs(got - ref)
    if c.out_p8:
        assert status == 0, what
        tol = p8.bound(ref, c.o_exp) + 2e-5 * float(np.abs(ref).max())
        assert not bool((err > tol).any()), (what, float(err.max()))
    else:
        assert float(err.max()) < 2e-5, (what, float(err.max()))


@pytest.mark.parametrize("c", ac.PEAKED, ids=ac.case_id)
def test_peaked_softmax(c):
    """Scores up to +-100 (the engine uploads exp(min(scale_mul, log 100)) as the per-head q scale), and for the P8 kernels up to +-20, the
    range the comment on the fast exp names; random data, and keys that drift towards a common direction so that the running maximum
    rises in every 64-key block (-rev: the first block holds it and every later one is rescaled against it).

    The project's 2e-5 is not the bar here: a plain float32 torch evaluation of the same formula on the CPU is itself up to about 2e-5 away
    from float64 at such scores.  That distance, measured per case on the same inputs, is the yardstick; the bar is four times it (the
    f16x3 product drops the lo * lo term: 2^-22 per product against 2^-24 for fp32), and never below 2e-5.  The poison and which-kernel
    checks hold as everywhere.  Figures of the run this was written with: DESIGN.md, "Attention: dispatch and edge tests"."""
    what = ac.case_id(c)
    words, used, status, (Q, K, V, qs, scale) = run_case(_lib(), c, _INDEX[c])
    assert used == c.kernel, (what, "ran as", used)
    got = check_poison(c, words, what)
    p8rows = bool(c.flags & 4)
    giv = [_given(x, p8rows) for x in (Q, K, V)]
    ref = reference(c, *giv, qs, scale, torch.float64)
    yard = float(np.abs(reference(c, *giv, qs, scale, torch.float32) - ref).max())
    err = float(np.abs(got - ref).max())
    bar = max(4.0 * yard, 2e-5)
    print(f"PEAKED | {what} | max|ref| {float(np.abs(ref).max()):.2f} | float32 yardstick {yard:.2e} | kernel {err:.2e} | bar {bar:.2e}")
    assert err < bar, (what, err, yard, bar)


# ---------------------------------------------------------------------------------------------------------------- (c) bit identity
_BIT = [c for c in ac.ALL if c.kernel in ac.BIT_IDENTICAL]


def _child_main(arm, npz, report):
    """arm 0 (ARTALK_ATTN_WIDE=0): every O buffer into one .npz.  arm 1: run again, compare with it, write the report."""
    L = _lib()
    outs, used = {}, {}
    for c in _BIT:
        i = _INDEX[c]
        outs[f"o{i}"], used[i], _, _ = run_case(L, c, i)
    if arm == 0:
        np.savez(npz, used=np.array([used[_INDEX[c]] for c in _BIT], dtype=np.int32), **outs)
        return
    base = np.load(npz)
    rep = {}
    for n, c in enumerate(_BIT):
        i = _INDEX[c]
        rep[str(i)] = [bool(np.array_equal(base[f"o{i}"], outs[f"o{i}"])), int(base["used"][n]), int(used[i])]
    with open(report, "w") as f:
        json.dump(rep, f)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_arms")
    npz, report = str(d / "narrow.npz"), str(d / "report.json")
    for arm in ("0", "1"):      # fresh processes, one after the other; the second is not started unless the first ended well
        subprocess.run([sys.executable, os.path.abspath(__file__), arm, npz, report], check=True, timeout=300,
                       env=dict(os.environ, ARTALK_ATTN_WIDE=arm))
    with open(report) as f:
        return json.load(f)


@pytest.mark.parametrize("c", _BIT, ids=ac.case_id)
def test_wide_forms_are_bit_identical_to_the_64_query_kernel(arms, c):
    equal, narrow, wide = arms[str(_INDEX[c])]
    assert wide == c.kernel and narrow == ac.BIT_IDENTICAL[c.kernel], (ac.case_id(c), narrow, wide)
    assert equal, ac.case_id(c)


if __name__ == "__main__":
    _child_main(int(sys.argv[1]), sys.argv[2], sys.argv[3])
