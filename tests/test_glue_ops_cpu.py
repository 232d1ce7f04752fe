"""Single-kernel entry points of the AR / VAE / style glue kernels (csrc/ar_glue.hip): the parts that need no GPU - the C ABI export
and the argument checks, every one of which is made before the device is touched (no table upload, no launch)."""
import pytest

from artalk_amd import capi

NEW = ["artalk_op_bsq_history_ex", "artalk_op_ar_bits_next", "artalk_op_vq_embed", "artalk_op_ar_begin", "artalk_op_dec_input",
       "artalk_op_dec_finish", "artalk_op_enc_input_zero", "artalk_op_style_input", "artalk_op_add_row", "artalk_op_style_finish",
       "artalk_op_broadcast16", "artalk_op_session_gather", "artalk_op_session_scatter", "artalk_op_absmax"]
P = 4096      # a 16-byte aligned address that is never dereferenced: the checks come first

# (entry point, a call with valid arguments, positions of the pointers that may be NULL)
VALID = {
    "bsq_history_ex": ([P, P, P, P, 3, None, None], {5, 6}),
    "ar_bits_next": ([P, P, P, P, 3, 2, None, None], {6, 7}),
    "vq_embed": ([P, 5, P, P, P, P, 6, 1, P, P, 3, None], {8, 9, 11}),
    "ar_begin": ([P, P, P, P, 3, None], {5}),
    "dec_input": ([P, P, P, P, P, 3, None], {6}),
    "dec_finish": ([P, P, P, P, P, 3 * 10600, 2, P, 3, None, None], {9, 10}),
    "enc_input_zero": ([P, P, P, P, 3, None], {5}),
    "style_input": ([P, P, P, P, 3, None], {5}),
    "add_row": ([P, P, 7, 128, None], {4}),
    "style_finish": ([P, P, P, P, None, P, 4, None, 0, None], {4, 7, 9}),
    "broadcast16": ([P, P, 64, 3, None], {4}),
    "session_gather": ([P, P, P, P, 3, 5, 2, 3, None], {8}),
    "session_scatter": ([P, P, P, P, 3, 5, 2, 3, 1, None], {9}),
    "absmax": ([P, 4, 64, 64, 0, 4, 0, 0, P, None], {9}),
}


def _call(name, args):
    return getattr(capi.lib(), "artalk_op_" + name)(*args)


def _with(args, i, v):
    a = list(args)
    a[i] = v
    return a


def test_glue_ops_are_exported():
    L = capi.lib()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert sorted("artalk_op_" + k for k in VALID) == sorted(NEW)


@pytest.mark.parametrize("name", sorted(VALID))
def test_null_required_pointer_is_refused(name):
    args, optional = VALID[name]
    n = 0
    for i, v in enumerate(args):
        if v == P and i not in optional:
            assert _call(name, _with(args, i, None)) == capi.EINVAL, (name, i)
            n += 1
    assert n >= 2


@pytest.mark.parametrize("name,pos", [("bsq_history_ex", 4), ("ar_bits_next", 4), ("vq_embed", 10), ("vq_embed", 1), ("ar_begin", 4),
                                      ("dec_input", 5), ("dec_finish", 8), ("enc_input_zero", 4), ("style_input", 4), ("add_row", 2),
                                      ("add_row", 3), ("style_finish", 6), ("broadcast16", 3), ("broadcast16", 2), ("session_gather", 7),
                                      ("session_scatter", 7), ("session_gather", 4), ("session_gather", 5), ("session_scatter", 6)])
def test_non_positive_count_is_refused(name, pos):
    """B <= 0, n <= 0 (and the other counts that size a launch)."""
    args, _ = VALID[name]
    for bad in (0, -1):
        assert _call(name, _with(args, pos, bad)) == capi.EINVAL, (name, pos, bad)


def test_level_outside_0_to_4_is_refused():
    args, _ = VALID["ar_bits_next"]
    for bad in (-1, 5, 181):
        assert _call("ar_bits_next", _with(args, 5, bad)) == capi.EINVAL
    # the last level writes neither fhat nor nextfeat: they may be NULL there, and only there
    assert _call("ar_bits_next", _with(_with(args, 2, None), 5, 3)) == capi.EINVAL
    assert _call("ar_bits_next", _with(_with(args, 3, None), 5, 0)) == capi.EINVAL


def test_broadcast16_wants_whole_aligned_units():
    args, _ = VALID["broadcast16"]
    for bad in (1, 15, 17, 16 * 255 + 8):
        assert _call("broadcast16", _with(args, 2, bad)) == capi.EINVAL
    assert _call("broadcast16", _with(args, 0, P + 4)) == capi.EINVAL
    assert _call("broadcast16", _with(args, 1, P + 8)) == capi.EINVAL


def test_absmax_shape_and_exponent_checks():
    args, _ = VALID["absmax"]
    for cols in (0, 4, 63, 65, 68):
        assert _call("absmax", _with(_with(args, 2, cols), 3, 128)) == capi.EINVAL, cols
    for e in (-9, 5, 16, -100):
        assert _call("absmax", _with(args, 5, e)) == capi.EINVAL, e
        assert _call("absmax", _with(_with(args, 4, 1), 5, e)) == capi.EINVAL, e
    assert _call("absmax", _with(args, 3, 56)) == capi.EINVAL          # row pitch shorter than a row
    assert _call("absmax", _with(args, 1, -1)) == capi.EINVAL
    assert _call("absmax", _with(args, 6, -1)) == capi.EINVAL
    assert _call("absmax", _with(_with(args, 6, 8), 7, 9)) == capi.EINVAL     # junk rows start past the period


def test_layout_checks_of_the_row_ops():
    a, _ = VALID["vq_embed"]
    assert _call("vq_embed", _with(a, 6, 5)) == capi.EINVAL            # xrows < xoff + n
    assert _call("vq_embed", _with(a, 7, -1)) == capi.EINVAL
    assert _call("vq_embed", _with(_with(a, 7, 0), 6, 5)) == capi.EINVAL      # a style row needs xoff >= 1
    assert _call("vq_embed", _with(a, 9, None)) == capi.EINVAL         # style_cond without pos0
    d, _ = VALID["dec_finish"]
    assert _call("dec_finish", _with(d, 6, -1)) == capi.EINVAL
    assert _call("dec_finish", _with(d, 5, 3 * 10600 - 1)) == capi.EINVAL     # chunk 2 does not fit the clip stride
    s, _ = VALID["style_finish"]
    assert _call("style_finish", _with(_with(s, 7, P), 8, 767)) == capi.EINVAL
    g, _ = VALID["session_gather"]
    assert _call("session_gather", _with(g, 2, P + 4)) == capi.EINVAL
