"""artalk_op_w2v_front_rows / artalk_op_pool_silu_rows / artalk_op_posconv_rows: the argument checks, every one of which is made before
the device is touched.  As in tests/test_rows_ops_cpu.py each call takes the arguments of a launch of run_wav2vec - chunk offsets into a
clip buffer and a row stride of T + 1, the 200-row frame stride of the encoder, the grouped positional convolution over padded chunks -
with sizes that are exactly the furthest element + 1, and adds ONE defect; the dummy pointers are never dereferenced because the call
returns first.  The calls without the defect are accepted under artalk_op_rows_dry_run, so every EINVAL below is the defect's and every
size is pinned from both sides.  tests/test_w2v_ops_gpu.py launches the same forms."""
import ctypes as C

import pytest

from artalk_amd import capi

P = 1 << 26       # a 4096-byte aligned address that is never dereferenced
P2, P3 = 2 * P, 3 * P
NCH, N, T, S = 4, 2583, 515, 516          # chunks, samples per chunk, frames (n - 10) // 5 + 1, row stride
LEN = 6000                                # samples in the clip buffer
OFFS = (7, 1300, 0, LEN - N)              # overlapping, unordered, the last chunk ends on the buffer end


def _front(**kw):
    a = dict(audio=P, audio_elems=LEN, off=OFFS, C=NCH, n=N, w=P2, bias=P2, lnw=P2, lnb=P2, xnorm=P3, Y=P, row_stride=S,
             y_elems=((NCH - 1) * S + T) * 512, out_p8=0, p8_exp=4, status=None)
    a.update(kw)
    off = None if a["off"] is None else (C.c_int64 * len(a["off"]))(*a["off"])
    return capi.lib().artalk_op_w2v_front_rows(a["audio"], a["audio_elems"], off, a["C"], a["n"], a["w"], a["bias"], a["lnw"], a["lnb"],
                                               a["xnorm"], a["Y"], a["row_stride"], a["y_elems"], a["out_p8"], a["p8_exp"], a["status"], None)


PC, PT, PTS, PD = 3, 199, 200, 1024       # pooling: chunks, frames, frame stride, width


def _pool(**kw):
    a = dict(X=P, C=PC, T=PT, D=PD, Y=P2, out_p8=0, p8_exp=4, status=None, x_tstride=PTS, x_elems=((PC - 1) * PTS + PT) * PD,
             y_elems=PC * 181 * PD)
    a.update(kw)
    return capi.lib().artalk_op_pool_silu_rows(a["X"], a["C"], a["T"], a["D"], a["Y"], a["out_p8"], a["p8_exp"], a["status"], a["x_tstride"],
                                               a["x_elems"], a["y_elems"], None)


def _posconv(mode, **kw):
    """the model's geometry (16 groups of 64 channels, 128 taps, 199 frames in 200-row chunks), the residual in place"""
    a = dict(mode=mode, X=P, W=P2, bias=P2, R=P3, C=P3, n_chunks=3, T=199, Ts=200, groups=16, cg=64, taps=128, act=1, a_exp=4, force_cfg=-1,
             status=None)
    a.update(kw)
    H = a["groups"] * a["cg"]
    a.setdefault("x_elems", ((a["n_chunks"] - 1) * a["Ts"] + a["T"]) * H)
    a.setdefault("c_elems", a["n_chunks"] * a["Ts"] * H)
    return capi.lib().artalk_op_posconv_rows(a["mode"], a["X"], a["x_elems"], a["W"], a["bias"], a["R"], a["C"], a["c_elems"], a["n_chunks"], a["T"],
                                             a["Ts"], a["groups"], a["cg"], a["taps"], a["act"], a["a_exp"], a["force_cfg"], a["status"], None)


SMALL = dict(groups=3, cg=32, taps=8, T=5, Ts=8)      # the small geometry of modes 0 and 2: every frame touches both paddings


@pytest.fixture
def dry():
    """artalk_op_rows_dry_run on: a call that passes every check returns ARTALK_OK without touching the device"""
    L = capi.lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    yield L
    assert L.artalk_op_rows_dry_run(0) == 0


def test_w2v_ops_are_exported():
    L = capi.lib()
    for name in ("artalk_op_w2v_front_rows", "artalk_op_pool_silu_rows", "artalk_op_posconv_rows"):
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    assert len(L.artalk_op_w2v_front_rows.argtypes) == 17 and len(L.artalk_op_pool_silu_rows.argtypes) == 12
    assert len(L.artalk_op_posconv_rows.argtypes) == 19
    assert _front(audio=None) == capi.EINVAL


# ------------------------------------------------------------------------------------------------------------------ normalise + conv0
def test_front_baselines_are_accepted(dry):
    assert _front() == capi.OK
    assert _front(out_p8=1, p8_exp=0) == capi.OK and _front(p8_exp=-8) == capi.OK
    assert _front(row_stride=T, y_elems=NCH * T * 512) == capi.OK                          # dense rows
    assert _front(C=1, off=(0,), n=10, audio_elems=10, row_stride=1, y_elems=512) == capi.OK      # the smallest call: one frame of one chunk
    assert _front(off=(0, 0, 0, 0), audio_elems=N) == capi.OK                             # every chunk the same samples
    assert _front(Y=P + 16) == capi.OK                                                     # fp32 rows: 16-byte vectors


def test_front_refusals(dry):
    for f in ("audio", "off", "w", "bias", "lnw", "lnb", "xnorm", "Y"):
        assert _front(**{f: None}) == capi.EINVAL, f
    assert _front(C=0, off=()) == capi.EINVAL and _front(C=-1) == capi.EINVAL
    assert _front(n=9, row_stride=1) == capi.EINVAL
    for e in (-9, 5, 16):
        assert _front(p8_exp=e) == capi.EINVAL, e
    # offsets: negative, or the chunk ends one sample past the buffer
    for i in range(NCH):
        off = list(OFFS)
        off[i] = -1
        assert _front(off=tuple(off)) == capi.EINVAL, i
        off[i] = LEN - N + 1
        assert _front(off=tuple(off)) == capi.EINVAL, i
        off[i] = LEN - N
        assert _front(off=tuple(off)) == capi.OK, i
    assert _front(audio_elems=LEN - 1) == capi.EINVAL                                      # the last chunk one sample short
    assert _front(audio_elems=N - 1, off=(0, 0, 0, 0)) == capi.EINVAL and _front(audio_elems=0) == capi.EINVAL
    # the row stride and the size of Y
    assert _front(row_stride=T - 1, y_elems=1 << 40) == capi.EINVAL and _front(row_stride=0, y_elems=1 << 40) == capi.EINVAL
    assert _front(row_stride=-S, y_elems=1 << 40) == capi.EINVAL and _front(row_stride=1 << 31, y_elems=1 << 60) == capi.EINVAL
    assert _front(y_elems=((NCH - 1) * S + T) * 512 - 1) == capi.EINVAL
    assert _front(row_stride=S + 1) == capi.EINVAL                                         # a stride that carries the last chunk past the size
    assert _front(row_stride=T, y_elems=NCH * T * 512 - 1) == capi.EINVAL
    assert _front(C=NCH + 1, off=OFFS + (0,)) == capi.EINVAL                               # a fifth chunk's rows
    # alignment of the stored rows
    assert _front(Y=P + 4, y_elems=1 << 40) == capi.EINVAL and _front(Y=P + 8, y_elems=1 << 40) == capi.EINVAL
    assert _front(Y=P + 16, out_p8=1, y_elems=1 << 40) == capi.EINVAL                      # P8 rows are 32-byte groups


def test_front_refuses_without_dry_run_too():
    """the checks do not depend on the switch: a refused call is refused before the device either way"""
    assert _front(row_stride=T - 1, y_elems=1 << 40) == capi.EINVAL and _front(off=(-1, 0, 0, 0)) == capi.EINVAL
    assert _pool(x_tstride=PT - 1, x_elems=1 << 40) == capi.EINVAL and _posconv(0, Ts=198) == capi.EINVAL


# ------------------------------------------------------------------------------------------------------------------ pooling + SiLU
def test_pool_baselines_are_accepted(dry):
    assert _pool() == capi.OK and _pool(out_p8=1, p8_exp=-8) == capi.OK
    assert _pool(x_tstride=PT, x_elems=PC * PT * PD) == capi.OK
    assert _pool(C=1, T=1, D=4, x_tstride=1, x_elems=4, y_elems=181 * 4) == capi.OK        # the smallest call
    assert _pool(C=1, T=1, D=8, x_tstride=1, x_elems=8, y_elems=181 * 8, out_p8=1) == capi.OK
    assert _pool(D=8, T=7, x_tstride=8, x_elems=(2 * 8 + 7) * 8, y_elems=PC * 181 * 8) == capi.OK


def test_pool_refusals(dry):
    assert _pool(X=None) == capi.EINVAL and _pool(Y=None) == capi.EINVAL
    big = dict(x_elems=1 << 40, y_elems=1 << 40)
    for f, v in (("C", 0), ("C", -2), ("T", 0), ("T", -1), ("D", 0), ("D", 6), ("D", 1022), ("p8_exp", -9), ("p8_exp", 5),
                 ("x_tstride", PT - 1), ("x_tstride", 0), ("x_tstride", -PTS), ("x_tstride", 1 << 31), ("X", P + 4), ("X", P + 8), ("Y", P2 + 4),
                 ("Y", P2 + 8)):
        assert _pool(**{f: v}, **big) == capi.EINVAL, (f, v)
    assert _pool(D=12, out_p8=1, **big) == capi.EINVAL and _pool(D=12, **big) == capi.OK   # P8 rows are groups of 8
    assert _pool(Y=P2 + 16, out_p8=1, **big) == capi.EINVAL and _pool(Y=P2 + 16, **big) == capi.OK
    assert _pool(x_elems=((PC - 1) * PTS + PT) * PD - 1) == capi.EINVAL
    assert _pool(y_elems=PC * 181 * PD - 1) == capi.EINVAL
    assert _pool(x_tstride=PTS + 1) == capi.EINVAL and _pool(T=PT + 1) == capi.EINVAL and _pool(C=PC + 1) == capi.EINVAL
    assert _pool(x_tstride=PT, x_elems=PC * PT * PD - 1) == capi.EINVAL


# ------------------------------------------------------------------------------------------------------------------ positional convolution
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_posconv_baselines_are_accepted(dry, mode):
    assert _posconv(mode) == capi.OK
    assert _posconv(mode, R=None) == capi.OK and _posconv(mode, bias=None) == capi.OK
    assert _posconv(mode, T=39, Ts=40) == capi.OK and _posconv(mode, T=200) == capi.OK and _posconv(mode, n_chunks=1, T=1, Ts=1) == capi.OK
    assert _posconv(mode, a_exp=-8) == capi.OK and _posconv(mode, act=0) == capi.OK and _posconv(mode, act=3) == capi.OK
    if mode != 1:
        assert _posconv(mode, **SMALL) == capi.OK
        assert _posconv(mode, groups=1, cg=4, taps=8, T=1, Ts=1, n_chunks=1) == capi.OK     # the smallest: cg % 4 == 0, cg * taps = 32
        for cfg in ((1, 2, 3, 4) if mode == 0 else (0, 1, 2)):
            assert _posconv(mode, force_cfg=cfg) == capi.OK, cfg
        assert _posconv(mode, C=P3 + 4, R=P3 + 4, bias=P2 + 4) == capi.OK                    # the fp32 / bf16 epilogue takes any alignment
        assert _posconv(mode, Ts=300, T=299) == capi.OK


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_posconv_refusals(dry, mode):
    assert _posconv(3) == capi.EINVAL and _posconv(-1) == capi.EINVAL
    for f in ("X", "W", "C"):
        assert _posconv(mode, **{f: None}, R=None) == capi.EINVAL, f
    assert _posconv(mode, R=P) == capi.EINVAL and _posconv(mode, R=P3 + 16) == capi.EINVAL      # the residual: none, or C in place
    big = dict(x_elems=1 << 40, c_elems=1 << 40)
    for f, v in (("n_chunks", 0), ("n_chunks", -1), ("T", 0), ("T", -3), ("T", 201), ("Ts", 198), ("act", -1), ("act", 4), ("a_exp", -9),
                 ("a_exp", 5), ("a_exp", 16), ("force_cfg", -2), ("force_cfg", 5 if mode == 0 else 3), ("X", P + 4), ("X", P + 8), ("W", P2 + 4),
                 ("W", P2 + 8)):
        assert _posconv(mode, **{f: v}, **big) == capi.EINVAL, (f, v)
    # sizes, one element short; a geometry that reaches further than the sizes of the baseline
    H = 1024
    assert _posconv(mode, x_elems=(2 * 200 + 199) * H - 1) == capi.EINVAL and _posconv(mode, c_elems=3 * 200 * H - 1) == capi.EINVAL
    assert _posconv(mode, x_elems=(2 * 200 + 199) * H, c_elems=3 * 200 * H) == capi.OK
    assert _posconv(mode, n_chunks=4, x_elems=(2 * 200 + 199) * H) == capi.EINVAL and _posconv(mode, n_chunks=4, c_elems=3 * 200 * H) == capi.EINVAL
    assert _posconv(mode, T=200, x_elems=(2 * 200 + 199) * H) == capi.EINVAL
    assert _posconv(mode, Ts=201, x_elems=(2 * 200 + 199) * H, c_elems=1 << 40) == capi.EINVAL
    assert _posconv(mode, Ts=201, x_elems=1 << 40, c_elems=3 * 200 * H) == capi.EINVAL
    # X is read by many rows of C: no overlap
    assert _posconv(mode, X=P3, R=None) == capi.EINVAL and _posconv(mode, X=P3 + 4 * 599 * H, R=None) == capi.EINVAL
    assert _posconv(mode, X=P3 + 4 * 600 * H, R=None) == capi.OK
    if mode == 1:
        # the LDS-window kernel is the model's geometry only, with the 16-byte epilogue
        for f, v in (("groups", 8), ("groups", 32), ("cg", 32), ("cg", 128), ("taps", 64), ("taps", 256), ("force_cfg", 0), ("force_cfg", 1),
                     ("force_cfg", 99)):
            assert _posconv(1, **{f: v}, **big) == capi.EINVAL, (f, v)
        assert _posconv(1, Ts=257, T=199, **big) == capi.EINVAL and _posconv(1, Ts=256, T=256, **big) == capi.OK
        assert _posconv(1, **SMALL, **big) == capi.EINVAL
        for f, v in (("bias", P2 + 4), ("bias", P2 + 8)):
            assert _posconv(1, **{f: v}, **big) == capi.EINVAL, (f, v)
        for d in (4, 8):
            assert _posconv(1, C=P3 + d, R=P3 + d, **big) == capi.EINVAL, d
            assert _posconv(1, C=P3 + d, R=None, **big) == capi.EINVAL, d
    else:
        for f, v in (("groups", 0), ("groups", -1), ("cg", 0), ("cg", 2), ("cg", 6), ("cg", 62), ("taps", 0), ("taps", -8)):
            assert _posconv(mode, **{f: v}, **big) == capi.EINVAL, (f, v)
        assert _posconv(mode, cg=4, taps=4, **big) == capi.EINVAL and _posconv(mode, cg=4, taps=8, **big) == capi.OK      # cg * taps % 32
        assert _posconv(mode, cg=12, taps=4, **big) == capi.EINVAL and _posconv(mode, cg=12, taps=8, **big) == capi.OK
        assert _posconv(mode, force_cfg=0 if mode == 0 else 4, **big) == capi.EINVAL
