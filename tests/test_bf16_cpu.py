"""bf16 precision mode (artalk_set_precision 2): the parts that need no GPU - the C ABI export, argument checks made before the device
is touched, and the Python mode names."""
import pytest

from artalk_amd import capi


def test_bf16_gemm_is_exported():
    L = capi.lib()
    assert "artalk_op_gemm_bf16" in capi.SYMBOLS
    assert hasattr(L, "artalk_op_gemm_bf16")


def test_bf16_gemm_argument_errors_without_gpu():
    """Null operands and K % 32 != 0 are refused before any allocation or launch."""
    L = capi.lib()
    assert L.artalk_op_gemm_bf16(None, 32, None, None, None, None, None, 1, 1, 32, 0, -1, None) == capi.EINVAL
    fake = 16     # never dereferenced: the checks come first
    assert L.artalk_op_gemm_bf16(fake, 32, fake, None, None, None, None, 1, 1, 32, 0, -1, None) == capi.EINVAL    # C missing
    assert L.artalk_op_gemm_bf16(fake, 48, fake, None, None, None, fake, 1, 1, 48, 0, -1, None) == capi.EINVAL    # K % 32
    assert L.artalk_op_gemm_bf16(fake, 32, fake, None, None, None, fake, 1, 1, 32, 0, 7, None) == capi.EINVAL     # no such kernel
    assert L.artalk_op_gemm_bf16(fake + 4, 32, fake, None, None, None, fake, 1, 1, 32, 0, -1, None) == capi.EINVAL  # A not 16-byte aligned
    assert L.artalk_op_gemm_bf16(fake, 32, fake + 8, None, None, None, fake, 1, 1, 32, 0, -1, None) == capi.EINVAL  # W not 16-byte aligned
    assert L.artalk_set_precision(None, 2) == capi.EINVAL


def test_unknown_mode_names_bf16():
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.model import BitwiseARModel
    m = BitwiseARModel(ARTalkConfig.tiny())
    for bad in ("fp16", 3, "BF16x"):
        with pytest.raises(ValueError, match="'bf16'"):
            m.set_precision(bad)
    m.set_precision("bf16")          # before the weights are loaded: remembered, applied by load_state_dict
    assert m._precision == "bf16"
    m.set_precision(2)
    assert m._precision == "bf16"
    import numpy as np
    for code, name in ((np.int64(1), "f16x3"), (np.int32(0), "f32"), (np.int64(2), "bf16")):     # numpy integers, as before the mode existed
        m.set_precision(code)
        assert m._precision == name
