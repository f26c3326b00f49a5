"""-m gpu: boxes with custom values (rows of box_ndim = 7 + custom_ndim values) through every kernel that takes a width --
sec_predict_decode_nd / _segments_nd / sec_predict_finalize_nd, sec_assign_targets_nd_f32, sec_second_loss_nd_f32,
sec_augment_boxes_nd_f32 -- and through the public routes (SecondDetector, DeviceTrainer, accelerate_model).

Columns 0-6, and everything that never sees a custom column (dets, dir_label, labels, importance, kept set), are compared BIT FOR BIT
with the seven-column entry points run on the [..., :7] slices; the custom columns with exact references (one rounded addition /
subtraction); the loss with the float64 reference under the comparison of tests/test_gpu_train_edges.py, and the velocity stages with the float64
helper within 16 * 2^-24 (|vx| + |vy| + 1), the constant README states for the augmentation kernel's values.  The references are tests/box_custom_helpers.py, pinned to the executed reference by tests/test_box_custom_host.py."""
import numpy as np
import pytest
import torch

import box_custom_helpers as H
import predict_ref_helpers as P
import train_ref_helpers as T

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WIDTHS = [8, 9, 11]
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
_id = lambda d: str(d).split(".")[-1]


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


@pytest.fixture(scope="module")
def g():
    return H.fixture()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ------------------------------------------------------------------------------------------------------------ decode and finalize
def _head(b, ahw, nd, dtype, seed, bins=2):
    """A channels-last head tensor [B, A * (nd + bins), H, W] and its strided box [B, A, H, W, nd] / dir [B, A, H, W, bins] views;
    custom encodings and custom anchor values have magnitudes in [2^-10, 64] (box_custom_helpers.exact_sum_values)."""
    a, h, w = ahw
    n = a * h * w
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    enc = torch.cat([torch.randn(b, n, 7, generator=gen) * 0.2, torch.from_numpy(H.exact_sum_values(rng, (b, n, nd - 7)))], -1).to(dtype)
    dirs = torch.randn(b, n, bins, generator=gen).to(dtype)
    parts = [t.reshape(b, a, h, w, c).permute(0, 1, 4, 2, 3).reshape(b, a * c, h, w) for t, c in ((enc, nd), (dirs, bins))]
    packed = torch.cat(parts, 1).contiguous(memory_format=torch.channels_last).cuda()
    box = packed[:, :a * nd].reshape(b, a, nd, h, w).permute(0, 1, 3, 4, 2)
    dirv = packed[:, a * nd:].reshape(b, a, bins, h, w).permute(0, 1, 3, 4, 2)
    assert not box.is_contiguous() and torch.equal(box.reshape(b, n, nd).cpu(), enc)
    anchors = torch.cat([torch.rand(n, 3, generator=gen) * 40, torch.rand(n, 3, generator=gen) * 3 + 0.5, torch.rand(n, 1, generator=gen) * 3,
                         torch.from_numpy(H.exact_sum_values(rng, (n, nd - 7)))], 1).cuda()
    return box, dirv, enc, anchors


def _picks(b, n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(n, generator=gen)[:k] if k <= n else torch.randint(0, n, (k,), generator=gen) for _ in range(b)])
    return idx.to(torch.int32).cuda(), torch.rand(b, k, generator=gen).cuda()


def _check_decode_nd(got, seven, enc, anchors, top_idx, nd):
    dec, dets, dlab = got
    dec7, dets7, dlab7 = seven
    assert dec.shape == (*top_idx.shape, nd) and _same(dec[..., :7], dec7) and _same(dets, dets7) and torch.equal(dlab, dlab7)
    idx = top_idx.long().cpu()
    e = torch.gather(enc.float(), 1, idx.unsqueeze(-1).expand(-1, -1, nd))[..., 7:].numpy()
    H.check_decode_custom(dec[..., 7:].cpu().numpy(), e, anchors.cpu()[idx][..., 7:].numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("nd", WIDTHS)
@pytest.mark.parametrize("k", [1, 255, 256, 257, 1000])
def test_decode_nd_plain_form(ops, k, nd, dtype):
    """The 12 x 10 map (two anchors per cell), one frame: B * k on both sides of a multiple of the block size."""
    ahw, b = (2, 12, 10), 1
    box, dirv, enc, anchors = _head(b, ahw, nd, dtype, 100 + nd)
    top_idx, top_score = _picks(b, 240, k, k)
    for rotate in (True, False):
        got = ops.predict_decode(box, dirv, anchors, top_idx, top_score, rotate=rotate)
        seven = ops.predict_decode(box[..., :7], dirv, anchors[:, :7].contiguous(), top_idx, top_score, rotate=rotate)
        _check_decode_nd(got, seven, enc, anchors, top_idx, nd)


def _lazy_tables(form, b, h, w, gen):
    """Half the 8 x 16 tiles (``form`` "tiles") / about half of the cover bits ("cover") written; -> (table on the device, written [B, H, W])."""
    if form == "tiles":
        ty, tx = (h + 7) // 8, (w + 15) // 16
        live = torch.rand(b, ty * tx, generator=gen) < 0.5
        live[:, 0], live[:, 1] = True, False
        written = live.reshape(b, ty, 1, tx, 1).expand(b, ty, 8, tx, 16).reshape(b, ty * 8, tx * 16)[:, :h, :w]
        return (live.to(torch.int16) << 4).contiguous().cuda(), written
    bands, words = (h + 7) // 8, (w + 31) // 32
    cover = torch.randint(-2 ** 31, 2 ** 31, (b, bands, words), generator=gen, dtype=torch.int64)
    ys, xs = torch.arange(h), torch.arange(w)
    written = ((cover[:, ys // 8][:, :, xs // 32] >> (xs % 32)) & 1).bool()
    return cover.to(torch.int32).contiguous().cuda(), written


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("nd", WIDTHS)
@pytest.mark.parametrize("form", ["tiles", "cover"])
def test_decode_nd_lazy_and_cover_forms_on_a_ragged_map(ops, form, nd, dtype):
    """A 12 x 20 map, ragged against the 8 x 16 tiles and the 32-column cover words, half of it unwritten (junk in the head, values read
    from the empty frame's map): equal to the seven-column lazy entry point on columns 0-6 and to the plain form on
    where(written, head, background) throughout."""
    ahw, b = (2, 12, 20), 2
    a, h, w = ahw
    n = a * h * w
    box, dirv, enc, anchors = _head(b, ahw, nd, dtype, 200 + nd)
    bgbox, bgdir, bgenc, _ = _head(1, ahw, nd, dtype, 300 + nd)
    gen = torch.Generator().manual_seed(5)
    table, written = _lazy_tables(form, b, h, w, gen)
    assert 0.25 < written.float().mean() < 0.75
    wr = written.reshape(b, 1, h, w, 1).cuda()
    holes_box, holes_dir = torch.where(wr, box, torch.full_like(box, 5.0)), torch.where(wr, dirv, torch.full_like(dirv, 9.0))
    # (the junk goes into the SAME strided layout: views of fresh packed tensors)
    def packed_like(box_t, dir_t):
        bb = box_t.shape[0]
        p = torch.cat([box_t.permute(0, 1, 4, 2, 3).reshape(bb, a * nd, h, w), dir_t.permute(0, 1, 4, 2, 3).reshape(bb, a * 2, h, w)], 1)
        p = p.contiguous(memory_format=torch.channels_last)
        return p[:, :a * nd].reshape(bb, a, nd, h, w).permute(0, 1, 3, 4, 2), p[:, a * nd:].reshape(bb, a, 2, h, w).permute(0, 1, 3, 4, 2)
    hb, hd = packed_like(holes_box, holes_dir)
    fb, fd = packed_like(torch.where(wr, box, bgbox.expand(b, -1, -1, -1, -1)), torch.where(wr, dirv, bgdir.expand(b, -1, -1, -1, -1)))
    bb, bd = packed_like(bgbox, bgdir)
    assert hb.stride() == fb.stride() and tuple(bb.stride()[1:]) == tuple(hb.stride()[1:])
    top_idx, top_score = _picks(b, n, 257, 9)
    on_bg = (~written.reshape(b, 1, h * w).expand(b, a, h * w).reshape(b, n).gather(1, top_idx.long().cpu())).sum()
    assert int(on_bg) > 50, "the picks must include anchors read from the background map"
    full_enc = torch.where(written.reshape(b, 1, h * w, 1).expand(b, a, h * w, nd).reshape(b, n, nd), enc, bgenc.expand(b, -1, -1))
    for rotate in (True, False):
        got = ops.predict_decode(hb, hd, anchors, top_idx, top_score, rotate=rotate, lazy=(table, (bb, bd)))
        seven = ops.predict_decode(hb[..., :7], hd, anchors[:, :7].contiguous(), top_idx, top_score, rotate=rotate,
                                   lazy=(table, (bb[..., :7], bd)))
        _check_decode_nd(got, seven, full_enc, anchors, top_idx, nd)
        plain = ops.predict_decode(fb, fd, anchors, top_idx, top_score, rotate=rotate)
        assert all(_same(x, y) for x, y in zip(got, plain))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("nd", WIDTHS)
def test_decode_nd_over_three_segments(ops, nd, dtype):
    maps, b = [(3, 7, 13), (5, 11, 3), (1, 1, 1)], 2
    heads = [_head(b, m, nd, dtype, 400 + 10 * i + nd) for i, m in enumerate(maps)]
    n = sum(a * h * w for a, h, w in maps)
    enc = torch.cat([hd[2] for hd in heads], 1)
    anchors = torch.cat([hd[3] for hd in heads], 0).contiguous()
    top_idx, top_score = _picks(b, n, 256, 11)
    starts = np.cumsum([a * h * w for a, h, w in maps])
    top_idx[:, :4] = torch.tensor([0, starts[0] - 1, starts[0], starts[1]], dtype=torch.int32)      # both sides of every border
    boxes, dirs = [hd[0] for hd in heads], [hd[1] for hd in heads]
    got = ops.predict_decode(boxes, dirs, anchors, top_idx, top_score)
    seven = ops.predict_decode([v[..., :7] for v in boxes], dirs, anchors[:, :7].contiguous(), top_idx, top_score)
    _check_decode_nd(got, seven, enc, anchors, top_idx, nd)


@pytest.mark.parametrize("nd", WIDTHS)
@pytest.mark.parametrize("setting", [(0.0, 1.0, 2), (0.78539, 0.0, 2)])
def test_finalize_nd_is_the_float32_restatement_with_the_custom_columns_copied(ops, setting, nd):
    """The table of tests/test_gpu_predict_edges.py (rotations around integer quotients of limit_period, centres on and just outside
    every face of the range, a NaN row) with num_keep of 0, 1, post_max and k, post_max 16 < k 64: columns 0-6 are
    predict_ref_helpers.finalize_reference32 bit for bit and equal sec_predict_finalize on the seven-column slice."""
    import test_gpu_predict_edges as E
    dir_offset, dir_limit_offset, bins = setting
    table = E._finalize_table(*setting)
    b, k, p = 6, 64, 16
    gen = torch.Generator().manual_seed(3)
    custom = torch.randn(b, k, nd - 7, generator=gen).numpy() * 5
    custom[:, 12] = np.nan
    dec = np.concatenate([np.repeat(table[None], b, 0), custom.astype(np.float32)], -1)
    keep = np.stack([np.roll(np.arange(k), -16 * (f % 4)) for f in range(b)]).astype(np.int32)
    num_keep = np.array([p, k, p, k, 0, 1], np.int32)
    top_score = torch.rand(b, k, generator=gen).numpy()
    top_label = torch.randint(0, 10, (b, k), generator=gen).to(torch.int32).numpy()
    dir_label = torch.randint(0, bins, (b, k), generator=gen).to(torch.int32).numpy()
    for use_dir in (1, 0):
        for r6 in (E.RANGE6, None):
            args = (dev(top_score), dev(top_label), dev(dir_label) if use_dir else None, dev(keep), dev(num_keep), p, use_dir, dir_offset,
                    dir_limit_offset, bins, dev(r6) if r6 is not None else None)
            want = P.finalize_reference32(dec[..., :7], top_score, top_label, dir_label, keep, num_keep, p, use_dir, dir_offset,
                                          dir_limit_offset, bins, r6)
            got = ops.predict_finalize(dev(dec), *args)
            seven = ops.predict_finalize(dev(dec[..., :7]), *args)
            assert got["boxes"].shape == (b, p, nd)
            assert P.same_bits_f32(got["boxes"][..., :7].cpu().numpy(), want["boxes"]) and _same(got["boxes"][..., :7], seven["boxes"])
            for key in ("scores", "labels", "valid"):
                assert torch.equal(got[key], seven[key]), key
            assert np.array_equal(got["valid"].cpu().numpy(), want["valid"])
            sel = np.where(np.arange(p)[None, :] < num_keep[:, None], keep[:, :p], 0)
            assert P.same_bits_f32(got["boxes"][..., 7:].cpu().numpy(), dec[np.arange(b)[:, None], sel][..., 7:])


def test_nd_entry_points_with_seven_columns_equal_the_existing_ones(ops):
    """box_ndim = 7 through sec_predict_decode_nd / _segments_nd / sec_predict_finalize_nd, sec_assign_targets_nd_f32,
    sec_second_loss_nd_f32 and sec_augment_boxes_nd_f32 (ctypes, the allocations of the ops wrappers): the results of the existing
    entry points bit for bit."""
    import ctypes
    from second_amd import runtime as rt
    l = rt.lib()
    ahw, b, k = (2, 12, 10), 2, 200
    box, dirv, enc, anchors = _head(b, ahw, 8, torch.bfloat16, 77)
    box, anchors = box[..., :7], anchors[:, :7].contiguous()
    top_idx, top_score = _picks(b, 240, k, 4)
    want = ops.predict_decode(box, dirv, anchors, top_idx, top_score)
    dec, dets, dlab = ops._decode_outputs((b, k), box.device)
    rc = l.sec_predict_decode_nd(rt.ptr(box), ops._strides5(box), rt.ptr(dirv), ops._strides5(dirv), 2, b, *ahw, k, rt.ptr(anchors),
                                 rt.ptr(top_idx), rt.ptr(top_score), 1, rt.ptr(dec), rt.ptr(dets), rt.ptr(dlab), rt.dtype_code(box.dtype), 7,
                                 None, None, None, None, rt.stream())
    assert rc == 0 and all(_same(x, y) for x, y in zip((dec, dets, dlab), want))
    ptrs, strides, dims = ops._segment_args([box])
    dptrs, dstrides, _ = ops._segment_args([dirv])
    dec2, dets2, dlab2 = ops._decode_outputs((b, k), box.device)
    rc = l.sec_predict_decode_segments_nd(1, ptrs, strides, dptrs, dstrides, dims, 2, b, k, rt.ptr(anchors), rt.ptr(top_idx), rt.ptr(top_score),
                                          1, rt.ptr(dec2), rt.ptr(dets2), rt.ptr(dlab2), rt.dtype_code(box.dtype), 7, rt.stream())
    assert rc == 0 and all(_same(x, y) for x, y in zip((dec2, dets2, dlab2), want))
    keep = torch.arange(k, dtype=torch.int32).repeat(b, 1).cuda()
    num_keep = torch.tensor([k, 3], dtype=torch.int32).cuda()
    top_label = torch.zeros((b, k), dtype=torch.int32).cuda()
    r6 = dev(np.array([0, 0, 0, 30, 30, 3], np.float32))
    fin = ops.predict_finalize(dec, top_score, top_label, dlab, keep, num_keep, 100, True, 0.78, 0.0, 2, r6)
    boxes, scores, labels, valid = ops._finalize_outputs(b, 100, dec.device)
    rc = l.sec_predict_finalize_nd(rt.ptr(dec), rt.ptr(top_score), rt.ptr(top_label), rt.ptr(dlab), rt.ptr(keep), rt.ptr(num_keep), b, k, 100, 1,
                                   0.78, 0.0, 2, rt.ptr(r6), rt.ptr(boxes), rt.ptr(scores), rt.ptr(labels), rt.ptr(valid), 7, rt.stream())
    assert rc == 0 and _same(boxes, fin["boxes"]) and _same(scores, fin["scores"]) and torch.equal(valid.view(torch.bool), fin["valid"])
    # assignment
    c = T.lattice_case(1, counts=(40, 0, 1))
    anc, gt = dev(c["anchors"]), dev(np.concatenate(c["gt"]))
    offs = dev(np.cumsum([0] + [len(x) for x in c["gt"]]).astype(np.int32))
    cls = dev(np.concatenate(c["classes"]))
    begins, ids, mt, ut = [0, 301, 874], [1, 3], [0.6, 0.5], [0.45, 0.375]
    want = ops.assign_targets_per_class(anc, gt, offs, cls, begins, ids, mt, ut, similarities=[None, None])
    a, nb, ng = anc.shape[0], 3, gt.shape[0]
    labels_, targets_, imp_ = (torch.empty((nb, a), dtype=torch.int32).cuda(), torch.empty((nb, a, 7)).cuda(), torch.empty((nb, a)).cuda())
    ws = rt.workspace(l.sec_assign_targets_workspace_bytes(nb, a, ng), anc.device)
    rc = l.sec_assign_targets_nd_f32(rt.ptr(anc), a, rt.ptr(gt), rt.ptr(cls), None, rt.ptr(offs), ng, nb, 2, (ctypes.c_int * 3)(*begins),
                                     (ctypes.c_int * 2)(*ids), (ctypes.c_float * 2)(*mt), (ctypes.c_float * 2)(*ut), (ctypes.c_int * 2)(0, 0),
                                     (ctypes.c_double * 6)(), rt.ptr(labels_), rt.ptr(targets_), rt.ptr(imp_), rt.ptr(ws), ws.numel(), None, 7,
                                     rt.stream())
    assert rc == 0 and torch.equal(labels_, want[0]) and _same(targets_, want[1]) and _same(imp_, want[2])
    # loss
    lc = T.loss_case(3, 2, 257, 3, 2)
    t = [dev(lc[key]) for key in ("cls", "box", "dir", "labels", "reg", "anchors", "importance")]
    want = ops.second_loss_raw(*t, **T.LOSS_NONDEFAULT)
    p = dict(ops.LOSS_DEFAULTS, **T.LOSS_NONDEFAULT)
    params = rt.f_arr([p["alpha"], p["gamma"], p["sigma"], p["pos_cls_weight"], p["neg_cls_weight"], p["classification_weight"],
                       p["localization_weight"], p["direction_loss_weight"], p["direction_offset"], p["sin_error_factor"], *p["code_weights"]])
    d_cls, d_box, d_dir, out6 = torch.empty_like(t[0]), torch.empty_like(t[1]), torch.empty_like(t[2]), torch.empty(6).cuda()
    ws = rt.workspace(l.sec_second_loss_workspace_bytes(2, 257), anc.device)
    rc = l.sec_second_loss_nd_f32(*(rt.ptr(x) for x in t), 2, 257, 3, 2, params, 7, rt.ptr(d_cls), rt.ptr(d_box), rt.ptr(d_dir), rt.ptr(out6),
                                  rt.ptr(ws), ws.numel(), rt.stream())
    assert rc == 0 and all(_same(x, y) for x, y in zip((out6, d_cls, d_box, d_dir), want))
    # augmentation
    vb = H.velocity_batch(2, (12, 0, 300))
    boxes7 = dev(vb["boxes"][:, :7])
    args = (dev(vb["box_offsets"]), dev(vb["params"]), (0, -40, 70.4, 40))
    kw = dict(valid=dev(vb["valid"]), classes=dev(vb["classes"]), importance=dev(vb["importance"]), loc_transform=dev(vb["loc_transform"]),
              rot_transform=dev(vb["rot_transform"]))
    want = ops.augment_boxes(boxes7, *args, **kw)
    n = boxes7.shape[0]
    ob, oo, oc, oi = (torch.empty((n, 7)).cuda(), torch.empty(4, dtype=torch.int32).cuda(), torch.empty(n, dtype=torch.int32).cuda(),
                      torch.empty(n).cuda())
    rc = l.sec_augment_boxes_nd_f32(rt.ptr(boxes7), rt.ptr(args[0]), n, 3, rt.ptr(kw["valid"].view(torch.uint8)), rt.ptr(kw["classes"]),
                                    rt.ptr(kw["importance"]), rt.ptr(kw["loc_transform"]), rt.ptr(kw["rot_transform"]), rt.ptr(args[1]),
                                    rt.f_arr(args[2]), 7, rt.ptr(ob), rt.ptr(oc), rt.ptr(oi), rt.ptr(oo), rt.stream())
    assert rc == 0 and _same(ob, want[0]) and torch.equal(oo, want[1]) and torch.equal(oc, want[2]) and _same(oi, want[3])


# ------------------------------------------------------------------------------------------------------------------ assignment
@pytest.fixture(scope="module")
def lattice():
    """train_ref_helpers.lattice_case (300, 256, 257, 0 and 1 boxes per frame: both sides of one LDS chunk) widened to 9 and 11
    columns: custom anchor values per anchor, custom ground-truth values per box (duplicated boxes get DIFFERENT ones)."""
    c = T.lattice_case(1)
    rng = np.random.default_rng(12)
    out = {}
    for nd in (9, 11):
        out[nd] = dict(c, anchors=np.concatenate([c["anchors"], rng.normal(0, 1, (len(c["anchors"]), nd - 7)).astype(np.float32)], 1),
                       gt=[np.concatenate([x, rng.normal(0, 3, (len(x), nd - 7)).astype(np.float32)], 1) for x in c["gt"]])
    return out


RANGES = {"per_class": ([0, 130, 301, 874], [1, 2, 3]), "all": ([0, 130, 301, 874], [0, 0, 0]), "one_range": ([0, 874], [0])}
MATCHED, UNMATCHED = [0.6, 0.5, 0.5], [0.45, 0.375, 0.375]


def _check_assign_nd(ops, c, nd, begins, ids, sims, mask):
    anchors, gts = c["anchors"], c["gt"]
    offs = np.cumsum([0] + [len(x) for x in gts]).astype(np.int32)
    cls = np.concatenate(c["classes"])
    imp = np.concatenate(c["importance"])
    n = len(ids)
    kw = dict(gt_importance=dev(imp), anchors_mask=None if mask is None else dev(mask), similarities=sims)
    got = ops.assign_targets_per_class(dev(anchors), dev(np.concatenate(gts)), dev(offs), dev(cls), begins, ids, MATCHED[:n], UNMATCHED[:n], **kw)
    seven = ops.assign_targets_per_class(dev(anchors[:, :7]), dev(np.concatenate(gts)[:, :7]), dev(offs), dev(cls), begins, ids, MATCHED[:n],
                                         UNMATCHED[:n], **dict(kw, similarities=sims or [None] * n))
    assert got[1].shape == (len(gts), len(anchors), nd)
    assert torch.equal(got[0], seven[0]) and _same(got[2], seven[2]) and _same(got[1][..., :7], seven[1])
    labels, targets = got[0].cpu().numpy(), got[1].cpu().numpy()
    positives = 0
    for f, gt in enumerate(gts):
        k = c["classes"][f]
        cand = np.zeros((len(anchors), len(gt)), bool)
        for r, cid in enumerate(ids):
            cand[begins[r]:begins[r + 1]] = True if cid == 0 else (k[None, :] == cid)
        arg = H.matched_rows(anchors[:, :7], gt[:, :7], targets[f, :, :7], labels[f], cand)
        H.check_assign_custom(targets[f, :, 7:], anchors, gt, arg)
        positives += int((arg >= 0).sum())
        if sims is None and len(gt):        # nearest IoU on the lattice: the float64 matching's own argmax
            ref = H.assign_ref_nd(anchors, gt, k, begins, ids, MATCHED[:n], UNMATCHED[:n], mask=None if mask is None else mask[f])
            assert np.array_equal(ref[0], labels[f]) and np.array_equal(ref[2], arg)
    assert positives > 100


@pytest.mark.parametrize("nd", [9, 11])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "anchors_mask"])
@pytest.mark.parametrize("ranges", ["per_class", "all"])
def test_assign_targets_nd_on_the_lattice(ops, lattice, ranges, masked, nd):
    mask = (np.random.default_rng(7).random((5, 874)) >= 0.3) if masked else None
    _check_assign_nd(ops, lattice[nd], nd, *RANGES[ranges], None, mask)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "anchors_mask"])
def test_assign_targets_nd_with_a_distance_similarity_on_one_range(ops, lattice, masked):
    mask = (np.random.default_rng(8).random((5, 874)) >= 0.3) if masked else None
    sims = [None, dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0), None]
    _check_assign_nd(ops, lattice[9], 9, *RANGES["per_class"], sims, mask)


def test_assign_targets_nd_single_range_entry(ops, lattice):
    """ops.assign_targets (one range, every ground truth) with nine columns, with and without a similarity."""
    c = lattice[9]
    offs = dev(np.cumsum([0] + [len(x) for x in c["gt"]]).astype(np.int32))
    gt, cls = np.concatenate(c["gt"]), np.concatenate(c["classes"])
    for sim in (None, "nearest_iou"):
        got = ops.assign_targets(dev(c["anchors"]), dev(gt), offs, 0.6, 0.45, gt_classes=dev(cls), similarity=sim)
        seven = ops.assign_targets(dev(c["anchors"][:, :7]), dev(gt[:, :7]), offs, 0.6, 0.45, gt_classes=dev(cls), similarity=sim)
        assert torch.equal(got[0], seven[0]) and _same(got[1][..., :7], seven[1]) and _same(got[2], seven[2])
        for f, x in enumerate(c["gt"]):
            lab, tg = got[0][f].cpu().numpy(), got[1][f].cpu().numpy()
            arg = H.matched_rows(c["anchors"][:, :7], x[:, :7], tg[:, :7], lab, np.ones((874, len(x)), bool))
            H.check_assign_custom(tg[:, 7:], c["anchors"], x, arg)


@pytest.mark.parametrize("tag,ids", [("per_class", [1, 2]), ("all", [0, 0])])
def test_assign_targets_nd_on_the_fixture_frames(ops, g, tag, ids):
    """The executed reference's frames: labels exact, targets within rtol 1e-5 / atol 2e-6 of its float64 values (the tolerance
    tests/test_gpu_train_edges.py uses for this kernel against float64), custom columns exact."""
    lab, tg = H.fixture_targets(g, tag)
    anchors = g["anchors"].astype(np.float32)
    frames = H.fixture_frames(g)
    offs = np.cumsum([0] + [len(x) for x, _ in frames]).astype(np.int32)
    got = ops.assign_targets_per_class(dev(anchors), dev(np.concatenate([x for x, _ in frames])), dev(offs),
                                       dev(np.concatenate([k for _, k in frames])), g["class_anchor_begin"].tolist(), ids,
                                       g["matched"].tolist(), g["unmatched"].tolist())
    assert np.array_equal(got[0].cpu().numpy(), lab)
    t = got[1].cpu().numpy()
    np.testing.assert_allclose(t, tg, rtol=1e-5, atol=2e-6)
    assert P.same_bits_f32(t[..., 7:], tg[..., 7:].astype(np.float32)) and not np.signbit(t[lab <= 0]).any()


# ------------------------------------------------------------------------------------------------------------------------ loss
NINE_WEIGHTS = (1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 0.25, 1.5)


@pytest.mark.parametrize("n_anchor", [1, 255, 257, 1000])
@pytest.mark.parametrize("nc", [1, 10])
@pytest.mark.parametrize("bins", [0, 2])
def test_second_loss_nd_against_float64(ops, bins, nc, n_anchor):
    """LOSS_NONDEFAULT with nine non-uniform code weights; frame 1 has no positive, and a second batch is all don't-care: out6, d_cls,
    d_box (all nine columns) and d_dir under the comparison of tests/test_gpu_train_edges.py."""
    cfg = dict(T.LOSS_NONDEFAULT, code_weights=NINE_WEIGHTS)
    for seed, dont_care in ((21, False), (22, True)):
        c = H.loss_case_nd(seed, 3, n_anchor, nc, bins, 9, direction_offset=cfg["direction_offset"], all_dont_care=dont_care)
        args = (c["cls"], c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"])
        got = ops.second_loss_raw(*(None if a is None else dev(a) for a in args), **cfg)
        got = [None if x is None else x.cpu().numpy() for x in got]
        H.check_loss(got, H.loss_nd(*args, nc, bins, **cfg))
        if not dont_care and n_anchor >= 8:
            assert np.abs(got[2][..., 7:]).max() > 0 and not got[2][1].any()          # velocity gradients; none in the frame without positives


def test_second_loss_nd_on_the_fixture(ops, g):
    cfg = dict(zip([str(k) for k in g["loss_cfg_keys"]], g["loss_cfg"].tolist()), code_weights=tuple(g["code_weights"].tolist()))
    anchors = g["anchors"].astype(np.float32)[g["loss_anchor_rows"]]
    got = ops.second_loss_raw(dev(g["loss_cls"]), dev(g["loss_box"]), dev(g["loss_dir"]), dev(g["loss_labels"].astype(np.int32)),
                              dev(g["loss_reg"]), dev(anchors), dev(g["loss_importance"]), **cfg)
    H.check_loss([x.cpu().numpy() for x in got], (g["loss_out6"], g["loss_d_cls"], g["loss_d_box"], g["loss_d_dir"]))
    with pytest.raises(ValueError, match="code_weights"):
        ops.second_loss_raw(dev(g["loss_cls"]), dev(g["loss_box"]), dev(g["loss_dir"]), dev(g["loss_labels"].astype(np.int32)),
                            dev(g["loss_reg"]), dev(anchors), dev(g["loss_importance"]))


# ---------------------------------------------------------------------------------------------------------------- augmentation
@pytest.mark.parametrize("counts", [(12, 0, 255, 1), (256, 257, 5, 300), (7,)], ids=["ragged4", "scan_block_edges", "one_frame"])
def test_augment_boxes_nd_against_the_seven_column_kernel_and_float64(ops, counts):
    """Frames of 0, 1, 255, 256, 257 and 300 boxes (both sides of one 256-box scan block), every flip combination, invalid boxes, boxes
    pushed out of the range: the kept set, order, classes, importance, offsets and columns 0-6 equal sec_augment_boxes_f32 on the
    seven-column slice; the velocity is within 16 * 2^-24 (|vx| + |vy| + 1) of the float64 helper."""
    vb = H.velocity_batch(3, counts)
    n = len(vb["boxes"])
    marker = np.arange(n, dtype=np.int32)                                # classes carry the input row of every survivor
    args = (dev(vb["box_offsets"]), dev(vb["params"]), (0, -40, 70.4, 40))
    kw = dict(valid=dev(vb["valid"]), classes=dev(marker), importance=dev(vb["importance"]), loc_transform=dev(vb["loc_transform"]),
              rot_transform=dev(vb["rot_transform"]))
    got = ops.augment_boxes(dev(vb["boxes"]), *args, **kw)
    seven = ops.augment_boxes(dev(vb["boxes"][:, :7]), *args, **kw)
    assert got[0].shape == (n, 9) and _same(got[0][:, :7], seven[0])
    assert torch.equal(got[1], seven[1]) and torch.equal(got[2], seven[2]) and _same(got[3], seven[3])
    offs, rows = got[1].cpu().numpy(), got[2].cpu().numpy()
    kept = int(offs[-1])
    assert 0 < kept < n or n < 10
    out = got[0].cpu().numpy()
    assert not out[kept:].any()
    frame = np.searchsorted(vb["box_offsets"], rows[:kept], side="right") - 1
    for f in range(len(counts)):
        m = frame == f
        if not m.any():
            continue
        v_in = vb["boxes"][rows[:kept][m], 7:9]
        fx, fy, angle, scale = vb["params"][f, :4]
        H.check_velocity(out[:kept][m, 7:9], v_in, H.velocity_ref(v_in, fx, fy, float(angle), float(scale)))
    # flips only (angle 0, scale 1): sign changes, bit for bit
    params = vb["params"].copy()
    params[:, 2], params[:, 3] = 0.0, 1.0
    flips = ops.augment_boxes(dev(vb["boxes"]), args[0], dev(params), args[2], **kw)
    k2 = int(flips[1][-1])
    r2 = flips[2].cpu().numpy()[:k2]
    f2 = np.searchsorted(vb["box_offsets"], r2, side="right") - 1
    want = np.concatenate([H.velocity_ref(vb["boxes"][r2[f2 == f], 7:9], params[f, 0], params[f, 1], 0.0, 1.0, dtype=np.float32, rotate=False)
                           for f in range(len(counts))]) if k2 else np.zeros((0, 2), np.float32)
    assert P.same_bits_f32(flips[0].cpu().numpy()[:k2, 7:9], want)
    with pytest.raises(ValueError, match="7 or 9"):
        ops.augment_boxes(dev(np.zeros((n, 8), np.float32)), *args)


@pytest.mark.parametrize("fx", [0, 1])
@pytest.mark.parametrize("fy", [0, 1])
def test_augment_boxes_nd_on_the_fixture(ops, g, fx, fy):
    """The executed reference's random_flip / global_rotation_v2 / global_scaling_v2 on [G, 9] boxes, one frame, no translation."""
    boxes = g["aug_boxes"]
    n = len(boxes)
    offs = dev(np.array([0, n], np.int32))
    wide = (-100, -100, 100, 100)
    flips = ops.augment_boxes(dev(boxes), offs, dev(np.array([[fx, fy, 0, 1, 0, 0, 0, 0]], np.float32)), wide)
    assert int(flips[1][-1]) == n and P.same_bits_f32(flips[0][:, 7:9].cpu().numpy(), g[f"aug_flip_{fx}{fy}"][:, 7:9])
    full = ops.augment_boxes(dev(boxes), offs, dev(np.array([[fx, fy, g["aug_angle"], g["aug_scale"], 0, 0, 0, 0]], np.float32)), wide)
    H.check_velocity(full[0][:, 7:9].cpu().numpy(), boxes[:, 7:9], g[f"aug_full_{fx}{fy}"][:, 7:9].astype(np.float64))
    np.testing.assert_allclose(full[0][:, :6].cpu().numpy(), g[f"aug_full_{fx}{fy}"][:, :6], rtol=1e-5, atol=1e-5)


def test_device_augmenter_takes_nine_column_boxes(ops):
    from second_amd.augment import DeviceAugmenter
    vb = H.velocity_batch(5, (12, 30))
    aug = DeviceAugmenter([-0.3, 0.3], [0.3, 0.3, 0.2], [-0.5, 0.5], [0.95, 1.05], [0.1, 0.1, 0.1], True, True, [0, -40, -3, 70.4, 40, 1], num_try=5)
    n = len(vb["boxes"])
    gen = torch.Generator(device="cuda").manual_seed(0)
    aug.draw(gen, num_boxes=n, batch_size=2)
    pts = torch.rand(500, 4, device="cuda") * 30
    poffs = torch.tensor([0, 200, 500], dtype=torch.int32, device="cuda")
    out9 = aug(pts, poffs, dev(vb["boxes"]), dev(vb["box_offsets"]), gt_classes=dev(vb["classes"]))
    out7 = aug(pts, poffs, dev(vb["boxes"][:, :7]), dev(vb["box_offsets"]), gt_classes=dev(vb["classes"]))
    assert out9[2].shape == (n, 9) and _same(out9[2][:, :7], out7[2]) and _same(out9[0], out7[0]) and torch.equal(out9[3], out7[3])
    assert out9[2][:, 7:].abs().max() > 0


# --------------------------------------------------------------------------------------------- whole path, reduced geometry
@pytest.fixture(scope="module")
def velo_det():
    """car.fhd on the 28 x 36 map with anchor_custom_values = [0, 0], trained-like weights (CPU state dict to load from)."""
    from second_amd.models import SecondDetector
    torch.manual_seed(0)
    det = SecondDetector(H.car_velo_cfg())
    assert det.box_ndim == 9 and det.feature_map_size == [1, 28, 36] and det.rpn.conv_box.out_channels == 18
    det = H.trained_like_on_device(det, H.car_clouds((0,))[0])
    return {k: v.detach().cpu().clone() for k, v in det.state_dict().items()}


def _velo_detector(state, dtype):
    from second_amd.models import SecondDetector
    det = SecondDetector(H.car_velo_cfg())
    det.load_state_dict(state)
    return det.cuda().prepare_inference(dtype)


def _batch(seeds=(0, 1)):
    from second_amd import synthetic as syn
    pts, offs = syn.batch_clouds(H.car_clouds(seeds))
    return torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda()


def test_forward_points_fused_and_torch_chains_agree_in_fp32(velo_det):
    """SecondDetector.forward_points returns [B, P, 9].  The fused chain and the plain-torch chain of the same detector, fp32: the same
    valid rows and labels; columns 7-8 bit-equal -- with the custom anchor values 0 they are the head's own encodings, which also
    identify the anchor of every row; columns 0-5 of both chains within predict_ref_helpers.decode_bounds of the float64 decode of
    that anchor; column 6 (decoded by one addition both chains perform alike, then the direction fix in float32 on either side:
    four more roundings of values below |o6| + 2 pi) within 2^-22 (|o6| + 2 pi) of each other."""
    from second_amd import models
    det = _velo_detector(velo_det, torch.float32)
    pts, offs = _batch()
    seen = []
    inner = det.predict_device
    det.predict_device = lambda preds, b, *a, **k: (seen.append(preds), inner(preds, b, *a, **k))[1]
    with torch.no_grad():
        fused = det.forward_points(pts, offs)
        det.fused_predict = False
        plain = det.forward_points(pts, offs)
    p = det.cfg["nms_post_max_size"]
    assert fused["boxes"].shape == (2, p, 9) and plain["boxes"].shape == (2, p, 9)
    assert torch.equal(fused["valid"], plain["valid"]) and int(fused["valid"].sum()) >= 6
    m = fused["valid"]
    assert torch.equal(fused["labels"][m].long(), plain["labels"][m].long())
    assert _same(fused["boxes"][m][:, 7:], plain["boxes"][m][:, 7:])
    enc = models.flat_preds(seen[0], 2)["box_preds"].reshape(2, -1, 9).float()
    anchors = det.anchors.float()
    for f in range(2):
        rows = fused["boxes"][f][m[f]]
        hit = (enc[f][None, :, 7:].view(torch.int32) == rows[:, None, 7:].contiguous().view(torch.int32)).all(-1)
        assert (hit.sum(1) == 1).all(), "the encodings of columns 7-8 identify one anchor per row"
        idx = hit.float().argmax(1)
        ref = P.decode_reference64(enc[f][idx][:, :7], anchors[idx][:, :7])
        bound = P.decode_bounds(enc[f][idx][:, :7], anchors[idx][:, :7], ref)
        for out in (fused, plain):
            got = out["boxes"][f][m[f]][:, :6].double()
            assert bool(((got - ref[:, :6]).abs() <= bound[:, :6]).all())
        d6 = (rows[:, 6].double() - plain["boxes"][f][m[f]][:, 6].double()).abs()
        assert bool((d6 <= 2.0 ** -22 * (rows[:, 6].double().abs() + 2 * np.pi)).all())


def test_staged_capture_replays_identical_bits(velo_det):
    det = _velo_detector(velo_det, torch.bfloat16)
    pts, offs = _batch()
    with torch.no_grad():
        det.calibrate(pts, offs)
        replays, out = det._capture_stages(pts, offs)
        runs = []
        for _ in range(2):
            for r in replays:
                r()
            torch.cuda.synchronize()
            runs.append({k: v.clone() for k, v in out.items()})
    det.check_overflow()
    assert runs[0]["boxes"].shape[0] == 2 and runs[0]["boxes"].shape[2] == 9 and int(runs[0]["valid"].sum()) >= 4
    for k in runs[0]:
        assert _same(runs[0][k], runs[1][k]), k


def _train_batch(det, seeds=(0, 1), boxes=10):
    """Clouds on the reduced range and per frame ten [*, 9] boxes: anchors of the map nudged by centimetres and turned by 0.2 .. 0.4 rad
    (tests/test_gpu_train_step_audit.py's car_batch), with velocities from N(0, 3)."""
    rng = np.random.default_rng(1000 + seeds[0])
    pts, offs = _batch(seeds)
    anc = det.anchors.cpu().numpy()
    x0, y0, _, x1, y1, _ = H.CAR_RANGE
    inner = anc[(anc[:, 0] > x0 + 2) & (anc[:, 0] < x1 - 2) & (anc[:, 1] > y0 + 2) & (anc[:, 1] < y1 - 2)]
    gts = []
    for _ in seeds:
        b = inner[rng.choice(len(inner), boxes, replace=False)].astype(np.float32)
        b[:, :2] += rng.normal(0, 0.03, (boxes, 2)).astype(np.float32)
        b[:, 6] += rng.uniform(0.2, 0.4, boxes).astype(np.float32)
        b[:, 7:9] = rng.normal(0, 3, (boxes, 2)).astype(np.float32)
        gts.append(b)
    return [pts, offs, dev(np.concatenate(gts)), dev(np.arange(len(seeds) + 1, dtype=np.int32) * boxes)]


def test_device_trainer_steps_on_nine_column_boxes_and_its_captured_step_equals_the_eager_one():
    """Three eager steps: finite losses and gradients in conv_box's velocity rows.  capture_step: the replay's loss scalars equal the
    eager forward of a fresh trainer on the same weights within rtol 2e-3 / atol 1e-5, the tolerance the seven-column captured step is
    held to (tests/test_gpu_train_dense.py::test_captured_step_has_no_memory_of_the_previous_batch)."""
    from second_amd.models import SecondDetector
    from second_amd.training import DeviceTrainer
    cfg = dict(H.car_velo_cfg(), code_weights=list(NINE_WEIGHTS))
    torch.manual_seed(0)
    tr = DeviceTrainer(SecondDetector(cfg).cuda(), amp_dtype=torch.bfloat16)
    assert tr.loss_cfg["code_weights"] == NINE_WEIGHTS
    ins = _train_batch(tr.det)
    velocity_rows = torch.tensor([a * 9 + j for a in range(2) for j in (7, 8)])
    for _ in range(3):
        out6 = tr.step(*ins)
        assert torch.isfinite(out6).all()
    loss, out6, labels = tr.forward_loss(*ins)
    loss.backward()
    assert torch.isfinite(out6).all() and int((labels > 0).sum()) >= 20
    gw = tr.det.rpn.conv_box.weight.grad.float().reshape(18, -1)[velocity_rows]
    assert torch.isfinite(gw).all() and bool((gw.abs().amax(1) > 0).all())
    torch.manual_seed(0)
    a = DeviceTrainer(SecondDetector(cfg).cuda(), amp_dtype=torch.bfloat16, lr=0.0, weight_decay=0.0)
    replay = a.capture_step(*ins)
    got = replay(*ins).clone()
    torch.cuda.synchronize()
    a.check_overflow()
    torch.manual_seed(0)
    b = DeviceTrainer(SecondDetector(cfg).cuda(), amp_dtype=torch.bfloat16, lr=0.0, weight_decay=0.0)
    _, want, _ = b.forward_loss(*ins)
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize("deferred", [False, True], ids=["synchronous", "deferred"])
def test_accelerate_model_returns_nine_column_boxes(velo_det, deferred):
    """A stand-in network whose box coder has custom_ndim = 2: accelerate_model serves it and returns box3d_lidar [k, 9] equal to
    SecondDetector.predict on the module graph's own head outputs (scores 1e-4, boxes rtol 1e-3 / atol 2e-3: the rule of
    tests/test_gpu_dropin_fused.py for fp32), on the synchronous and on the deferred lane."""
    from reference_standin import example_of
    from second_amd import compat
    net = H.standin_net(H.car_velo_cfg(), 2)
    net.load_state_dict(velo_det)
    net = net.eval().cuda()
    clouds = H.car_clouds((0, 1))
    ex = example_of(net, clouds, "cuda")
    assert ex["anchors"].shape[-1] == 9
    with torch.no_grad():
        preds = net.network_forward(ex["voxels"], ex["num_points"], ex["coordinates"], 2)
        want = net.predict({k: v.float() for k, v in preds.items()}, ex["anchors"].view(2, -1, 9).float())
    assert sum(w["scores"].shape[0] for w in want) >= 6 and want[0]["box3d_lidar"].shape[1] == 9
    compat.accelerate_model(net, deferred=deferred)
    eng = net._second_amd_engine
    assert eng.box_ndim == 9
    with torch.no_grad():
        got = [net(ex) for _ in range(eng.lanes + 1 if deferred else 2)][-1]
    assert eng.stats["original_calls"] == 0 and eng.stats["fused_calls" if not deferred else "deferred_calls"] >= 2
    for gd, wd in zip(got, want):
        assert gd["box3d_lidar"].shape == wd["box3d_lidar"].shape and gd["box3d_lidar"].shape[1] == 9
        np.testing.assert_allclose(gd["scores"].cpu().numpy(), wd["scores"].cpu().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(gd["box3d_lidar"].cpu().numpy(), wd["box3d_lidar"].cpu().numpy(), rtol=1e-3, atol=2e-3)
        np.testing.assert_array_equal(gd["label_preds"].cpu().numpy(), wd["label_preds"].long().cpu().numpy())
