"""The RPN's lazy chain on COVER lists (sec_conv2d_nhwc_gather_cover -> sec_conv2d_nhwc_tiles_cover x 4 -> sec_conv2d_nhwc_tiles_tail_cover
-> sec_predict_select_cover / _decode_cover): tiles start at any column of their 8-row band, so a layer's written region is no
union of grid tiles and its consumer picks x or the empty frame's map per halo PIXEL.  Per-pixel arithmetic is unchanged, so every
comparison is torch.equal: written pixels of every intermediate and of the head tensor against the grid form and the dense
every-tile form, selections and decoded boxes against the grid form.  Unwritten regions hold NaN throughout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CONVS = ("conv2d_nhwc_gather", "conv2d_nhwc_tiles", "conv2d_nhwc", "conv2d_nhwc_tiles_tail", "conv1x1_chain")


def _rpn(dtype, seed=3):
    from second_amd.models import RPNV2, RPNInference
    torch.manual_seed(seed)
    rpn = RPNV2().cuda().eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    for mod in rpn.modules():                         # statistics that leave a NON-ZERO background after every layer
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.empty(mod.num_features).uniform_(-0.3, 0.3, generator=g))
            mod.running_var.copy_(torch.empty(mod.num_features).uniform_(0.5, 1.5, generator=g))
            mod.bias.data.copy_(torch.empty(mod.num_features).uniform_(-0.2, 0.4, generator=g))
            mod.weight.data.copy_(torch.empty(mod.num_features).uniform_(0.5, 1.5, generator=g))
    return RPNInference(rpn, dtype)


def _bev(features, smap):
    from second_amd import models

    class BEV(models.SparseBEV):
        def __init__(self):
            self.features = features

        def site_map(self):
            return smap
    return BEV()


def _scene(name, h, w):
    """[n, 4] int32 (b, z, y, x) sites of a batch of 2"""
    s = []
    if name == "straddle":          # a blob across the grid line x = 16: two grid tiles, one cover tile (conv 0 reaches columns 12..19)
        s += [(0, 0, 3, 13), (0, 1, 4, 18), (0, 0, 2, 15), (1, 0, min(h - 2, 12), 14), (1, 0, min(h - 2, 12), 17)]
    elif name == "seam":            # blobs in vertically adjacent bands at different x: partial halo masks across the seam at rows 7 / 8
        s += [(0, 0, 6, 5), (0, 0, 9, 14), (0, 1, 7, 21 % w), (1, 0, 7, 10), (1, 0, 8, 3), (1, 0, min(h - 1, 16), 12)]
    elif name == "last_column":
        s += [(0, 0, 4, w - 1), (0, 0, h - 1, w - 1), (1, 1, 0, w - 1), (1, 0, 10, 0)]
    elif name == "empty_busy":      # an all-empty frame next to a busy one
        rng = np.random.default_rng(h + w)
        s += [(1, int(z), int(y), int(x)) for z, y, x in zip(rng.integers(0, 2, 14), rng.integers(0, h, 14), rng.integers(0, w, 14))]
    return np.unique(np.array(s, np.int32), axis=0)


def _run(rpn, bev, mode):
    """One forward in ``mode`` = cover / grid / dense -> (outputs of the conv ops in order, preds)."""
    from second_amd import ops
    rpn.skip_background = mode != "dense"
    rpn.lazy_background, rpn.lazy_heads, rpn.fused_tail = True, mode != "dense", True
    rpn.tile_cover = mode == "cover"
    rpn.empty_frame_maps(*bev.site_map().shape[2:])       # (cached: its convs stay out of the hook's record)
    seen = []
    ops.set_op_hook(lambda name, fn, a, kw, res: seen.append((name, res)) if name in CONVS else None)
    ops.POISON_LAZY_OUTPUTS = True
    try:
        with torch.no_grad():
            preds = rpn(bev)
    finally:
        ops.POISON_LAZY_OUTPUTS = False
        ops.set_op_hook(None)
        rpn.tile_cover = False
    return seen, preds


def _written(cols, h, w):
    """TileCover.cols of one layer [B, bands, wr] int32 -> [B, H, W] bool"""
    u = cols.cpu().numpy().astype(np.int64) & 0xffffffff
    bits = ((u[..., None] >> np.arange(32)) & 1).reshape(u.shape[0], u.shape[1], -1)[..., :w].astype(bool)
    return torch.from_numpy(np.repeat(bits, 8, axis=1)[:, :h]).cuda()


def _px(t, m):
    return t.permute(0, 2, 3, 1)[m]                    # [B, C, H, W] channels_last -> the pixels of mask [B, H, W]


def _select_decode(preds, anchors, k=64, thr=0.3):
    from second_amd import ops
    lz = preds["lazy_heads"]
    sel = ops.predict_select(preds["cls_preds"], k, thr, lazy=(lz[0], lz[1]["cls_preds"]))
    dec = ops.predict_decode(preds["box_preds"], preds["dir_cls_preds"], anchors, sel[0], sel[1],
                             lazy=(lz[0], (lz[1]["box_preds"], lz[1]["dir_cls_preds"])))
    n = sel[3].cpu().tolist()
    rows = lambda t: [t[f, :n[f]].clone() for f in range(len(n))]
    return n, [rows(t) for t in sel[:3]] + [rows(t) for t in dec]


def _check(dtype, h, w, scene):
    from second_amd import ops
    batch = 2
    idx = _scene(scene, h, w)
    torch.manual_seed(11)
    feat = torch.randn(len(idx), 64, device="cuda").to(dtype)
    smap = ops.sparse_site_map(torch.from_numpy(idx).cuda(), batch, [2, h, w])
    rpn = _rpn(dtype)
    assert rpn.background_convs == 6
    bev = _bev(feat, smap)
    conv_c, preds_c = _run(rpn, bev, "cover")
    cover_counts = rpn.last_cover_counts.clone()
    conv_g, preds_g = _run(rpn, bev, "grid")
    assert rpn.last_cover_counts is None
    conv_d, preds_d = _run(rpn, bev, "dense")
    names = [n for n, _ in conv_c]
    assert names == ["conv2d_nhwc_gather"] + ["conv2d_nhwc_tiles"] * 4 + ["conv2d_nhwc_tiles_tail"] == [n for n, _ in conv_g], names
    assert len(conv_d) == 7 and conv_d[-1][0] == "conv1x1_chain"
    assert preds_c["lazy_heads"][0].dtype == torch.int32 and preds_g["lazy_heads"][0].dtype == torch.int16
    _, _, cv = bev.tile_lists(6, cover=True)
    order_g, counts_g = bev.tile_lists(6)
    assert torch.equal(cv.counts, cover_counts) and bool((cover_counts.sum(1) <= counts_g.sum(1)).all())
    tiles = order_g.shape[-1]
    tx = (w + 15) // 16
    for l in range(5):                                 # (the sixth conv's output stays in LDS: the tail's result is the head tensor, below)
        yc, yg, yd = conv_c[l][1], conv_g[l][1], conv_d[l][1]
        wc = _written(cv.cols[l], h, w)
        gl = torch.zeros(batch, tiles, dtype=torch.bool, device="cuda")
        for f in range(batch):
            gl[f, order_g[l, f, :int(counts_g[l, f])].long()] = True
        wg = gl.view(batch, -1, tx).repeat_interleave(8, 1).repeat_interleave(16, 2)[:, :h, :w]
        assert not torch.isnan(_px(yc, wc).float()).any(), l
        assert torch.equal(_px(yc, wc), _px(yd, wc)), f"conv {l}: written pixels against the dense form"
        both = wc & wg
        assert torch.equal(_px(yc, both), _px(yg, both)), f"conv {l}: written pixels against the grid form"
        if _follows_list(cover_counts[l].sum(), batch * tiles):
            assert bool(torch.isnan(_px(yc, ~wc).float()).all()), f"conv {l}: only the listed tiles are written"
            assert bool((~wc).any())
    # the heads: every written element against the dense every-tile form; selections and decoded boxes against the grid form
    wc = _written(cv.cols[5], h, w)
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        a, d = preds_c[k].permute(0, 2, 3, 1, 4)[wc], preds_d[k].permute(0, 2, 3, 1, 4)[wc]
        assert not torch.isnan(a.float()).any() and torch.equal(a, d), k
    a_, hh, ww = preds_c["cls_preds"].shape[1:4]
    g = torch.Generator().manual_seed(5)
    anchors = torch.rand(a_ * hh * ww, 7, generator=g).mul_(4.0).add_(0.5).cuda()
    n_c, out_c = _select_decode(preds_c, anchors)
    n_g, out_g = _select_decode(preds_g, anchors)
    assert n_c == n_g and sum(n_c) > 0
    for tc, tg in zip(out_c, out_g):
        for rc, rg in zip(tc, tg):
            assert torch.equal(rc, rg)
    return cover_counts.sum(1).cpu().numpy(), counts_g.sum(1).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h,w", [(24, 40), (17, 21)])
@pytest.mark.parametrize("scene", ["straddle", "seam", "last_column", "empty_busy"])
def test_cover_chain_is_bit_identical_to_the_grid_and_dense_forms(dtype, h, w, scene):
    cover, grid = _check(dtype, h, w, scene)
    if scene == "straddle" and w >= 32:
        assert cover[0] < grid[0], "the blob across a grid line must cost the grid more tiles than the cover"


def _follows_list(count, total_tiles):
    """the kernel's rule (csrc/dense.hip g_list_max_live_q8): the list up to SEC_RPN_LIST_MAX_LIVE percent of the tiles (default 225 / 256)"""
    pct = os.environ.get("SEC_RPN_LIST_MAX_LIVE", "")
    q8 = min(max(int(pct) * 256 // 100, 0), 256) if pct else 225
    return int(count) * 256 <= int(total_tiles) * q8


def _plain_order_child(direction, dtype):
    """Runs with SEC_RPN_LIST_MAX_LIVE=70 (read once per process) on a scene whose cover lists hold 56 / 56 / 67 / 78 / 89 / 100 % of the
    tiles.  ``after``: convs 0-2 follow their cover lists, convs 3-5 take the plain tile order behind them and read their input through
    the GRID-indexed halo masks.  ``before``: the other way round by direct calls -- conv 1 in the plain order (its counts say every
    tile: a producer that wrote everything), conv 2 on its cover list behind it."""
    from second_amd import ops
    h, w, batch = 24, 40, 2
    idx = np.array([(f, 0, y, x) for f in range(2) for y, x in ((2, 3), (5, 30), (12, 14), (20, 36), (21, 2))], np.int32)
    torch.manual_seed(13)
    feat = torch.randn(len(idx), 64, device="cuda").to(dtype)
    smap = ops.sparse_site_map(torch.from_numpy(idx).cuda(), batch, [2, h, w])
    rpn = _rpn(dtype)
    bev = _bev(feat, smap)
    _, _, cv = bev.tile_lists(6, cover=True)
    total = batch * cv.order.shape[-1]
    lists = [_follows_list(c, total) for c in cv.counts.sum(1).cpu().tolist()]
    assert lists == [True, True, True, False, False, False], (lists, cv.counts.sum(1).cpu().tolist())
    conv_c, preds_c = _run(rpn, bev, "cover")
    conv_d, preds_d = _run(rpn, bev, "dense")

    def on_list(y, l):
        wc = _written(cv.cols[l], h, w)
        return torch.equal(_px(y, wc), _px(conv_d[l][1], wc)) and bool(torch.isnan(_px(y, ~wc).float()).all()) and bool((~wc).any())
    if direction == "after":
        for l in range(5):
            y = conv_c[l][1]
            assert torch.equal(y, conv_d[l][1]) if not lists[l] else on_list(y, l), l         # plain order: every pixel computed
        for k in ("box_preds", "cls_preds", "dir_cls_preds"):       # the tail took the plain order too: the whole head tensor
            assert torch.equal(preds_c[k], preds_d[k]), k
        return
    empty = rpn.empty_frame_maps(h, w)
    every = torch.full_like(cv.counts[1], cv.order.shape[-1])
    ops.POISON_LAZY_OUTPUTS = True
    try:
        y1 = ops.conv2d_nhwc_tiles(conv_c[0][1], rpn.packed[1], rpn.bs[1], 128, cv.order[1], every, None, relu=True,
                                   cover_halo=cv.halo[1], background_in=empty[0])
        y2 = ops.conv2d_nhwc_tiles(y1, rpn.packed[2], rpn.bs[2], 128, cv.order[2], cv.counts[2], None, relu=True,
                                   cover_halo=cv.halo[2], background_in=empty[1])
    finally:
        ops.POISON_LAZY_OUTPUTS = False
    assert torch.equal(y1, conv_d[1][1]), "conv 1 in the plain order behind a cover-form conv 0"
    assert on_list(y2, 2), "conv 2 on its cover list behind the plain-order conv 1"


@pytest.mark.parametrize("direction", ["after", "before"])
def test_cover_chain_across_a_change_between_lists_and_the_plain_order(direction):
    """SEC_RPN_LIST_MAX_LIVE forces layer l + 1 into the plain tile order behind a cover-form layer l (its halo comes through the
    grid-indexed masks), and the other way round: a conv on its cover list behind a producer that wrote every tile."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SEC_COVER_TEST_DIRECTION=direction,
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "second.pytorch_amd"), os.environ.get("PYTHONPATH", "")]))
    env["SEC_RPN_LIST_MAX_LIVE"] = "70"
    r = subprocess.run([sys.executable, __file__, "--plain-order-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cover-child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__" and "--plain-order-child" in sys.argv:
    _plain_order_child(os.environ["SEC_COVER_TEST_DIRECTION"], torch.bfloat16)
    print("cover-child ok")
