"""sec_conv2d_fwd_plan_name tied to the launch: for one small shape per kernel form of the dense conv2d forward -- every call form,
every instantiation the decision function can answer in a default process, the two kernels that used not to report themselves among
them -- the op reports the instantiation the host-only query announced, that instantiation is the one the case was written for, and
its output agrees per element with torch's fp32 convolution of the same 16-bit inputs (the bound of
test_gpu_parity.test_conv2d_nhwc_mfma_vs_torch).  Maps are ragged against the tiles; the forms behind a "several rounds of
workgroups" test (more than 1 024 workgroups) get the smallest map that crosses it."""
import pytest
import torch

from test_gpu_parity import conv2d_per_element_bound

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
TYPE_NAME = {BF: "__hip_bfloat16", HF: "__half"}

# call form, cin, cout, ksize, stride, pad, (batch, h, w), the instantiation (%s = element type)
CASES = [
    ("plain", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false>"),
    ("plain", 64, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 64, 8, 0, false>"),
    ("plain", 256, 256, 3, 1, 1, (1, 130, 250), "k_conv2d_halo_reg<%s, 256, 4, 0, false>"),          # 33 x 16 tiles x 2 = 1 056 workgroups
    ("plain", 64, 64, 3, 1, 1, (1, 515, 500), "k_conv2d_halo_reg<%s, 64, 8, 0, false, 2>"),          # 33 x 32 = 1 056
    ("tiles", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false>"),
    ("tiles_lazy", 128, 256, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false>"),
    ("tail", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, false, true>"),
    ("x3", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>"),
    ("x3_tiles", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>"),
    ("gather", 128, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_halo_reg<%s, 128, 8, 3, true>"),
    ("plain", 64, 64, 3, 2, 1, (1, 24, 20), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>"),
    ("plain", 64, 128, 3, 2, 1, (1, 24, 20), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1>"),
    ("plain", 128, 128, 3, 2, 1, (1, 24, 20), "k_conv2d_patch<%s, 128, 3, 2, 4, 16, 1>"),
    ("plain", 64, 64, 3, 1, 1, (1, 24, 20), "k_conv2d_patch<%s, 64, 3, 1, 16, 16, 2>"),
    ("plain", 256, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_patch<%s, 256, 3, 1, 4, 16, 1>"),
    ("plain", 64, 128, 4, 4, 0, (1, 24, 20), "k_conv2d_patch<%s, 64, 4, 4, 2, 16, 1>"),
    ("plain", 128, 128, 2, 2, 0, (1, 24, 20), "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>"),
    ("plain", 128, 128, 2, 2, 0, (1, 132, 1000), "k_conv2d_patch<%s, 128, 2, 2, 4, 16, 1>"),         # 33 x 32 = 1 056 tiles of 2 x 16
    ("plain", 256, 128, 1, 1, 0, (1, 24, 20), "k_conv2d_patch<%s, 256, 1, 1, 2, 16, 1>"),
    ("plain", 384, 128, 1, 1, 0, (1, 24, 20), "k_conv2d_patch<%s, 384, 1, 1, 2, 16, 1>"),
    ("into", 128, 128, 2, 2, 0, (1, 24, 20), "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>"),
    ("rows", 64, 64, 3, 2, 1, (1, 24, 20), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true>"),
    ("rows", 64, 64, 3, 2, 1, (1, 520, 1000), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true, true>"),  # 33 x 32 = 1 056
    ("rows", 64, 128, 3, 2, 1, (1, 24, 20), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1, true>"),
    ("plain", 128, 128, 1, 1, 0, (1, 24, 20), "k_conv1x1_nhwc<%s, 128, 4>"),
    ("plain", 128, 64, 1, 1, 0, (1, 24, 20), "k_conv1x1_nhwc<%s, 64, 4>"),
    ("plain", 192, 128, 3, 1, 1, (1, 24, 20), "k_conv2d_nhwc_dma<%s, 64>"),
    ("plain", 192, 256, 3, 1, 1, (1, 160, 150), "k_conv2d_nhwc_dma<%s, 128>"),                      # 192 pixel tiles x 2 = 384 workgroups
]
PARAMS = [pytest.param(*c, dt, id="%s-%d-%d-k%ds%d-%dx%dx%d-%s" % (c[0], c[1], c[2], c[3], c[4], *c[6], "bf16" if dt == BF else "f16"))
          for c in CASES for dt in ((BF,) if c[0].startswith("x3") else (BF, HF))]


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops as o
    return o


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _from_rows(rows, site_map):
    """[..., C] gathered through a map of row + 1 (0: zeros)"""
    return torch.cat([torch.zeros_like(rows[:1]), rows])[site_map.long()]


def _run(ops, form, x, w, cout, k, stride, pad, dtype):
    """The op of `form` on the dense image x (16-bit values, fp32 tensor): (its output as fp32, the image it really convolved)."""
    b, cin, h, wd = x.shape
    dev = x.device
    pk = ops.conv2d_pack_weight(w)
    xd = _cl(x.to(dtype))
    tiles = -(-h // 8) * -(-wd // 16)
    # lists with every tile live, masks with every neighbour written, backgrounds that are never read
    order = torch.arange(tiles, dtype=torch.int16, device=dev).repeat(b, 1).contiguous()
    counts = torch.full((b,), tiles, dtype=torch.int32, device=dev)
    masks = torch.full((2, b, tiles), 0x1ff, dtype=torch.int16, device=dev)
    bg_out, bg_in = _cl(torch.zeros(1, cout, h, wd, device=dev, dtype=dtype)), _cl(torch.zeros(1, 128, h, wd, device=dev, dtype=dtype))
    if form == "plain":
        return ops.conv2d_nhwc(xd, pk, None, cout, k, stride, pad, relu=False).float(), x
    if form == "into":
        ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
        wide = _cl(torch.zeros(b, cout + 64, ho, wo, device=dev, dtype=dtype))
        return ops.conv2d_nhwc_into(xd, pk, None, cout, k, stride, pad, False, wide, 64).float(), x
    if form == "rows":                                  # pillars in ~30 % of the cells, the ragged corner among them
        occ = torch.rand(b, h, wd, device=dev) < 0.3
        occ[:, -1, -1] = True
        site_map = torch.zeros(b, h, wd, dtype=torch.int32, device=dev)
        site_map[occ] = torch.arange(1, int(occ.sum()) + 1, dtype=torch.int32, device=dev)
        rows = x.permute(0, 2, 3, 1)[occ].to(dtype).contiguous()
        out = ops.conv2d_nhwc_rows(rows, site_map, pk, None, cout, k, stride, pad, relu=False)
        return out.float(), _from_rows(rows, site_map).permute(0, 3, 1, 2).float()
    if form == "gather":                                # sites in ~70 % of the two planes; input channel z * 64 + c
        occ = torch.rand(b, 2, h, wd, device=dev) < 0.7
        occ[:, :, -1, -1] = True
        site_map = torch.zeros(b, 2, h, wd, dtype=torch.int32, device=dev)
        site_map[occ] = torch.arange(1, int(occ.sum()) + 1, dtype=torch.int32, device=dev)
        rows = x.view(b, 2, 64, h, wd).permute(0, 1, 3, 4, 2)[occ].to(dtype).contiguous()
        out = ops.conv2d_nhwc_gather(rows, site_map, pk, None, cout, relu=False)
        return out.float(), _from_rows(rows, site_map).permute(0, 1, 4, 2, 3).reshape(b, 128, h, wd).float()
    if form == "tiles":
        return ops.conv2d_nhwc_tiles(xd, pk, None, cout, order, counts, bg_out, relu=False).float(), x
    if form == "tiles_lazy":
        return ops.conv2d_nhwc_tiles(xd, pk, None, cout, order, counts, None, relu=False, nbr_masks=masks, background_in=bg_in).float(), x
    if form == "tail":
        # a 1x1 tail that copies: W1 = identity, W2 = the first 64 channels, no bias, no ReLU -- every product is 1 * v or 0 * v, so the
        # head tensor is the conv's 16-bit output tile itself
        w1 = torch.eye(128, device=dev).view(128, 128, 1, 1).to(dtype)
        w2 = torch.eye(64, 128, device=dev).view(64, 128, 1, 1).to(dtype)
        out = ops.conv2d_nhwc_tiles_tail(xd, pk, None, order, counts, masks, bg_in, ops.conv2d_pack_weight(w1), torch.zeros(128, device=dev),
                                         ops.conv2d_pack_weight(w2), None, 64, relu=False, relu1=False)
        return out.float(), x
    # split-fp32 forms on operands that ARE bf16 values (lo planes zero): the fp32 result leaves as hi + lo
    pk3 = ops.conv2d_pack_weight_x3(w.float())
    zero = torch.zeros_like(xd)
    if form == "x3":
        hi, lo = ops.conv2d_nhwc_x3(xd, zero, pk3, None, cout, relu=False)
    else:
        hi, lo = ops.conv2d_nhwc_x3_tiles(xd, zero, pk3, None, cout, order, counts, background=(bg_out, bg_out), relu=False)
    return hi.float() + lo.float(), x


@pytest.mark.parametrize("form,cin,cout,k,stride,pad,bhw,kernel,dtype", PARAMS)
def test_launch_reports_the_planned_kernel_and_matches_torch(ops, form, cin, cout, k, stride, pad, bhw, kernel, dtype):
    torch.manual_seed(cin + cout + 7 * k + bhw[1])
    b, h, wd = bhw
    x = torch.randn(b, cin, h, wd, device="cuda").to(dtype).float()
    w = (torch.randn(cout, cin, k, k, device="cuda") / (cin * k * k) ** 0.5).to(dtype)
    plan = ops.conv2d_plan_name(b, h, wd, cin, cout, k, stride, pad, dtype, "tiles" if form == "tiles_lazy" else form)
    assert plan == kernel % TYPE_NAME[dtype]
    out, x_seen = _run(ops, form, x, w, cout, k, stride, pad, dtype)
    assert ops.last_kernel_name() == plan
    ref = torch.nn.functional.conv2d(x_seen, w.float(), None, stride, pad)
    bound = conv2d_per_element_bound(x_seen, w, ref, stride, pad, dtype)
    if form == "tail":
        ref, bound = ref[:, :64], bound[:, :64]
    assert out.shape == ref.shape
    err = (out - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
