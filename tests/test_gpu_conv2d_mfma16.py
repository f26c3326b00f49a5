"""The 16x16x32 main loop of the 128-channel 3x3 conv (k_conv2d_halo_reg<..., ROLL = 3>): row-streamed halo fragments, its own swizzle
key and its own accumulator-to-tile packing.

1. On small integers every fp32 partial sum is exact in any order, so the output must equal the integer convolution rounded once
   to the output type BIT FOR BIT -- a wrong lane, chunk, tap or key mapping cannot hide inside a tolerance.
2. The 32x32x16 loop (SEC_CONV2D_MFMA=32, read once per process: two child interpreters) against the default loop on random
   post-ReLU data: the two group the products of an output element differently, nothing else."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops as o
    return o


def _int_case(cout, h, w, dtype, seed):
    """x in [-4, 4], w in [-2, 2], integer bias: |any partial sum| <= 1152 * 8 = 9 216 < 2^24.  Returns the cuda inputs and the int64
    convolution + bias (CPU, in fp64: exact on these magnitudes)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (2, 128, h, w), generator=g)
    wgt = torch.randint(-2, 3, (cout, 128, 3, 3), generator=g)
    bias = torch.randint(-8, 9, (cout,), generator=g)
    ref = torch.nn.functional.conv2d(x.double(), wgt.double(), bias.double(), 1, 1).to(torch.int64)
    assert int(ref.abs().max()) <= 9216 + 8
    xd = x.to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    return xd, wgt.to(dtype).cuda(), bias.float().cuda(), ref


def _rounded(ref, relu, dtype):
    r = ref.clamp(min=0) if relu else ref
    return r.float().to(dtype)                        # int -> fp32 is exact here; ONE rounding to the output type


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("sparse_input", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cout,h,w", [(128, 9, 17),      # four tiles, ragged bottom and right
                                      (256, 8, 16),      # one full tile, two channel blocks
                                      (128, 1, 1)])
def test_integer_conv_is_exact(ops, cout, h, w, dtype, relu, sparse_input):
    x, wgt, bias, ref = _int_case(cout, h, w, dtype, seed=cout + 31 * h + w)
    out = ops.conv2d_nhwc(x, ops.conv2d_pack_weight(wgt), bias, cout, 3, 1, 1, relu=relu, sparse_input=sparse_input)
    assert ", 128, 8, 3, " in ops.last_kernel_name(), ops.last_kernel_name()
    want = _rounded(ref, relu, dtype)
    assert out.shape == want.shape
    bad = _bits(out) != _bits(want)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_integer_conv_is_exact_through_the_tile_lists(ops, dtype, relu):
    """9 x 33 = 2 x 3 tiles per frame: frame 0 has ONE live tile (the others are copied from the background image), frame 1 ONE
    background tile (the others are convolved).  Live tiles: the exact convolution; background tiles: the background image's bits."""
    h, w, cout = 9, 33, 128
    x, wgt, bias, ref = _int_case(cout, h, w, dtype, seed=933)
    tiles = 6
    live = [[4], [0, 1, 2, 3, 5]]
    order = torch.zeros((2, tiles), dtype=torch.int16)
    for f, lv in enumerate(live):
        rest = [t for t in range(tiles) if t not in lv]
        order[f, :len(lv)] = torch.tensor(lv, dtype=torch.int16)
        order[f, len(lv):] = torch.tensor(rest[::-1], dtype=torch.int16)       # background tiles: from the end backwards
    counts = torch.tensor([len(lv) for lv in live], dtype=torch.int32)
    g = torch.Generator().manual_seed(7)
    bg = torch.randint(-100, 101, (1, cout, h, w), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    out = ops.conv2d_nhwc_tiles(x, ops.conv2d_pack_weight(wgt), bias, cout, order.cuda(), counts.cuda(), bg, relu=relu)
    assert ", 128, 8, 3, " in ops.last_kernel_name(), ops.last_kernel_name()
    want = _rounded(ref, relu, dtype)
    for f in range(2):
        for t in range(tiles):
            ys, xs = slice((t // 3) * 8, (t // 3) * 8 + 8), slice((t % 3) * 16, (t % 3) * 16 + 16)
            exp = want[f, :, ys, xs] if t in live[f] else bg[0, :, ys, xs]
            assert torch.equal(_bits(out[f, :, ys, xs]), _bits(exp)), (f, t)


_CHILD_SHAPE = (2, 128, 23, 40, 256)


def _child_inputs(dtype):
    b, cin, h, w, cout = _CHILD_SHAPE
    g = torch.Generator().manual_seed(2340)
    x = torch.relu(torch.randn(b, cin, h, w, generator=g)).to(dtype)           # post-ReLU activations: half of them zero
    wgt = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to(dtype)
    return x, wgt


def _child_main(path):
    from second_amd import ops
    res = {}
    for dtype in (torch.bfloat16, torch.float16):
        x, wgt = _child_inputs(dtype)
        xd = x.cuda().contiguous(memory_format=torch.channels_last)
        out = ops.conv2d_nhwc(xd, ops.conv2d_pack_weight(wgt.cuda()), None, _CHILD_SHAPE[4], 3, 1, 1, relu=False)
        res[str(dtype)] = (out.float().cpu().contiguous(), ops.last_kernel_name())
    torch.save(res, path)


@pytest.fixture(scope="module")
def both_loops(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("mfma16")
    got = {}
    for name, val in (("new", None), ("old", "32")):     # the switch is read once per process
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "second.pytorch_amd"), os.environ.get("PYTHONPATH", "")]))
        env.pop("SEC_CONV2D_MFMA", None)
        if val:
            env["SEC_CONV2D_MFMA"] = val
        path = str(d / (name + ".pt"))
        r = subprocess.run([sys.executable, __file__, "--loop-child", path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[name] = torch.load(path)
    return got


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_old_loop_against_new_loop(both_loops, dtype):
    """Per element |a - b| <= 2 (K + 2) 2^-23 sum|x||w| + one output ulp of |ref|, K = 1152: twice the accumulation bound of
    test_conv2d_nhwc_mfma_vs_torch (each loop is within gamma_K sum|x||w| of the exact sum) plus the two roundings to the output
    type, half a unit in the last place each -- taken relative to the exact value: 2^-7 |ref| (bf16), 2^-10 |ref| (fp16)."""
    a, name_a = both_loops["new"][str(dtype)]
    b, name_b = both_loops["old"][str(dtype)]
    assert ", 128, 8, 3, " in name_a and ", 128, 8, 2, " in name_b, (name_a, name_b)
    x, wgt = _child_inputs(dtype)
    ref = torch.nn.functional.conv2d(x.double(), wgt.double(), None, 1, 1)
    mag = torch.nn.functional.conv2d(x.double().abs(), wgt.double().abs(), None, 1, 1)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    bound = 2 * (1152 + 2) * 2.0 ** -23 * mag + ulp * ref.abs()
    diff = (a.double() - b.double()).abs()
    print("share of elements that differ", float((diff > 0).double().mean()), "largest |a - b| / bound", float((diff / (bound + 1e-300)).max()))
    assert a.shape == ref.shape and bool((diff <= bound).all()), float((diff / (bound + 1e-300)).max())
    # and each loop is the convolution (not both wrong alike): the per-element bound of test_conv2d_nhwc_mfma_vs_torch
    each = ulp / 2 * ref.abs() + 2 * (1152 + 2) * 2.0 ** -24 * mag + 1e-30
    for out in (a, b):
        assert bool(((out.double() - ref).abs() <= each).all())


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--loop-child":
    _child_main(sys.argv[2])
