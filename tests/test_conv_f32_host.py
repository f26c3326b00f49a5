"""Host side of the fp32-MFMA RPN convolutions (csrc/dense_f32.hip): exported symbols, argument validation before any launch, and
the SEC_FP32_RPN process default.  No GPU needed."""
import ctypes

import pytest

F32_SYMBOLS = ["sec_conv2d_f32_packed_weight_bytes", "sec_conv2d_f32_pack_weight", "sec_conv2d_nhwc_f32", "sec_conv2d_nhwc_f32_tiles",
               "sec_conv1x1_chain_f32"]
OK, INVALID, UNSUPPORTED = 0, -1, -3


def test_library_exports_the_fp32_conv_symbols_and_the_abi_version_stays():
    from second_amd import runtime as rt
    l = rt.lib()
    for name in F32_SYMBOLS:
        assert name in rt.SYMBOLS, name
        assert getattr(l, name) is not None, name
    assert l.sec_abi_version() == 9 == rt.ABI_VERSION


def test_packed_weight_bytes_says_which_shapes_are_taken():
    from second_amd import runtime as rt
    l = rt.lib()
    assert l.sec_conv2d_f32_packed_weight_bytes(128, 128, 3) >= 9 * 128 * 128 * 4
    assert l.sec_conv2d_f32_packed_weight_bytes(256, 128, 3) >= 9 * 128 * 256 * 4
    assert l.sec_conv2d_f32_packed_weight_bytes(128, 128, 1) >= 128 * 128 * 4
    assert l.sec_conv2d_f32_packed_weight_bytes(64, 128, 1) >= 128 * 64 * 4
    for shape in ((96, 128, 3), (128, 64, 3), (128, 128, 5)):
        assert l.sec_conv2d_f32_packed_weight_bytes(*shape) == 0, shape


def test_fp32_conv_entry_points_validate_before_any_launch():
    """Status codes of include/second_hip.h, decided on the host: the pointers below are never dereferenced."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)
    # pack
    assert l.sec_conv2d_f32_pack_weight(None, 128, 128, 3, one, None) == INVALID
    assert l.sec_conv2d_f32_pack_weight(one, 128, 128, 3, None, None) == INVALID
    assert l.sec_conv2d_f32_pack_weight(one, 96, 128, 3, one, None) == UNSUPPORTED
    assert l.sec_conv2d_f32_pack_weight(one, 128, 64, 3, one, None) == UNSUPPORTED
    # every tile
    assert l.sec_conv2d_nhwc_f32(None, 1, 8, 16, one, None, 128, 1, one, None) == INVALID
    assert l.sec_conv2d_nhwc_f32(one, 1, 8, 16, None, None, 128, 1, one, None) == INVALID
    assert l.sec_conv2d_nhwc_f32(one, 1, 8, 16, one, None, 128, 1, None, None) == INVALID
    assert l.sec_conv2d_nhwc_f32(one, 0, 8, 16, one, None, 128, 1, one, None) == INVALID
    assert l.sec_conv2d_nhwc_f32(one, 1, 8, 16, one, None, 96, 1, one, None) == UNSUPPORTED
    assert l.sec_conv2d_nhwc_f32(one, 1, 8, 16, one, None, 64, 1, one, None) == UNSUPPORTED
    assert l.sec_conv2d_nhwc_f32(one, 1, 2048, 2048, one, None, 128, 1, one, None) == UNSUPPORTED       # h * w * 512 >= 2^31
    # tile lists
    tiles = lambda **kw: l.sec_conv2d_nhwc_f32_tiles(*[kw.get(k, d) for k, d in (
        ("x", one), ("batch", 1), ("h", 8), ("w", 16), ("packed", one), ("bias", None), ("cout", 128), ("relu", 1), ("order", one),
        ("counts", one), ("background", None), ("masks", None), ("background_in", None), ("y", one), ("stream", None))])
    assert tiles(x=None) == INVALID and tiles(packed=None) == INVALID and tiles(y=None) == INVALID
    assert tiles(order=None) == INVALID and tiles(counts=None) == INVALID
    assert tiles(masks=one) == INVALID                                     # masks without the producer's empty-frame map
    assert tiles(cout=96, background=one) == UNSUPPORTED
    assert tiles(h=2048, w=2048, background=one) == UNSUPPORTED
    # 1x1 chain
    chain = lambda **kw: l.sec_conv1x1_chain_f32(*[kw.get(k, d) for k, d in (
        ("x", one), ("pixels", 100), ("w1", one), ("b1", one), ("relu1", 1), ("w2", one), ("b2", None), ("cout2", 64), ("y", one), ("stream", None))])
    assert chain(x=None) == INVALID and chain(w1=None) == INVALID and chain(w2=None) == INVALID and chain(b1=None) == INVALID
    assert chain(y=None) == INVALID and chain(pixels=-1) == INVALID
    assert chain(cout2=32) == UNSUPPORTED and chain(cout2=96) == UNSUPPORTED
    assert chain(pixels=0) == OK and chain(pixels=0, cout2=128) == OK
    # the 16-bit entry points keep refusing fp32 images
    assert l.sec_conv2d_packed_weight_bytes(128, 128, 3, rt.SEC_F32) == 0
    assert l.sec_conv2d_nhwc(one, 1, 8, 16, 128, one, None, 128, 3, 1, 1, 1, one, rt.SEC_F32, None) == UNSUPPORTED


def test_sec_fp32_rpn_default_is_validated_where_it_is_read(monkeypatch):
    from second_amd import models
    monkeypatch.delenv("SEC_FP32_RPN", raising=False)
    assert models.exact_rpn_default() == "torch"
    monkeypatch.setenv("SEC_FP32_RPN", "hip")
    assert models.exact_rpn_default() == "hip"
    monkeypatch.setenv("SEC_FP32_RPN", "bogus")
    with pytest.raises(ValueError) as e:
        models.exact_rpn_default()
    assert "torch" in str(e.value) and "hip" in str(e.value) and "bogus" in str(e.value)


def test_ops_refuse_cpu_tensors():
    import torch
    from second_amd import ops, runtime as rt
    x = torch.zeros(1, 128, 8, 16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(rt.SecondHipError):
        ops.conv2d_pack_weight_f32(torch.zeros(128, 128, 3, 3))
    with pytest.raises(rt.SecondHipError):
        ops.conv2d_nhwc_f32(x, torch.zeros(4), None, 128)
    with pytest.raises(rt.SecondHipError):
        ops.conv1x1_chain_f32(x, torch.zeros(4), torch.zeros(128), torch.zeros(4), None, 64)
