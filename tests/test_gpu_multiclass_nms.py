"""-m gpu: multi-class NMS on the device (sec_predict_select_classes / _decode_classes / sec_nms_sorted_items_f32 /
sec_predict_finalize_classes and SecondDetector's fused path over them).

(a) the fused path against what the reference's VoxelNet.predict returns (tests/golden/multiclass_nms.npz), fp32;
(b) every new entry point against the per-class loop over the entry points that existed before -- sec_predict_select on the strided
    one-class view, sec_predict_decode, sec_nms_sorted_f32, sec_predict_finalize -- bit for bit, fp32 / bf16 / fp16, on the head
    tensor's channels-last strides.  The new select has two forms, chosen by the number of passing anchors (at most 1 024: one
    sweep; more: radix select): the fixture's class 1 has more than 1 024 in the class-agnostic cases, the other items fewer, and the
    16-bit casts make equal keys frequent (tie order);
(c) a frame without survivors has no valid row; (d) refused arguments return their codes and launch nothing;
(e) forward_points replayed from its graph equals the eager call."""
import ctypes

import numpy as np
import pytest
import torch

import multiclass_nms_helpers as H

pytestmark = pytest.mark.gpu
HW = H.H * H.W


@pytest.fixture(scope="module")
def fx():
    return H.load()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


def head_views(fx, dtype):
    """cls / box / dir as [B, A, H, W, code] VIEWS of channels-last tensors [B, H, W, A, code], as the RPN head leaves them."""
    out = []
    for name in ("cls", "box", "dir"):
        t = torch.from_numpy(fx[name]).to(dtype).cuda()
        out.append(t.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4))
        assert not out[-1].is_contiguous()
    return out


def ranges(agnostic):
    return [(0, H.A)] * H.C if agnostic else [(2 * c, 2 * c + 2) for c in range(H.C)]


@pytest.fixture(scope="module")
def anchors():
    from second_amd import models as M
    return torch.from_numpy(M.generate_anchors(H.config(), [1, H.H, H.W])).cuda()


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", sorted(H.CASES))
def test_fused_path_equals_the_reference(fx, name):
    from second_amd.models import SecondDetector
    from test_multiclass_nms_host import assert_frames, frames_of
    rotate, agnostic = H.CASES[name]
    det = SecondDetector(H.config(rotate, agnostic)).eval().cuda()
    cls, box, dirs = head_views(fx, torch.float32)
    seen = []
    real = det._predict_multiclass_fused
    det._predict_multiclass_fused = lambda *a, **k: seen.append(1) or real(*a, **k)
    with torch.no_grad():
        out = det.predict_device({"cls_preds": cls, "box_preds": box, "dir_cls_preds": dirs}, H.B)
    assert seen == [1] and out["boxes"].shape == (H.B, sum(H.POST), 7)
    assert_frames(frames_of(out), fx["cases"][name], name)
    # the torch formulation on the same device tensors (what a pre_max above 1024 takes) gives the same rows
    det.fused_predict = False
    with torch.no_grad():
        ref = det.predict_device({"cls_preds": cls, "box_preds": box, "dir_cls_preds": dirs}, H.B)
    assert seen == [1] and torch.equal(ref["valid"], out["valid"]) and torch.equal(ref["labels"][ref["valid"]].int(), out["labels"][out["valid"]])
    assert torch.allclose(ref["scores"][ref["valid"]], out["scores"][out["valid"]], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_entry_points_equal_the_per_class_loop(fx, ops, anchors, dtype, rotate, agnostic):
    cls, box, dirs = head_views(fx, dtype)
    rng = ranges(agnostic)
    top_idx, top_score, counts = ops.predict_select_classes(cls, rng, H.PRE, H.THR)
    kout = top_idx.shape[2]
    assert kout == (1024 if agnostic else 2 * HW) and tuple(counts.shape) == (H.B, H.C)
    n_sel = 0
    for c, (a0, a1) in enumerate(rng):
        view = cls[:, a0:a1, :, :, c:c + 1]                                   # the strided one-class view: pointer + c channels, its a-range
        idx, score, _, cnt = ops.predict_select(view, H.PRE[c], H.THR[c])
        assert torch.equal(cnt, counts[:, c]), (c, cnt.tolist(), counts[:, c].tolist())
        for b in range(H.B):
            m = int(cnt[b])
            n_sel += m
            assert torch.equal(top_idx[b, c, :m], idx[b, :m] + a0 * HW), (b, c)
            assert torch.equal(top_score[b, c, :m].view(torch.int32), score[b, :m].view(torch.int32)), (b, c)
            assert not top_idx[b, c, m:].any() and not top_score[b, c, m:].any()      # rows behind counts: anchor 0 / score 0
    assert n_sel > 0 and int(counts[1, 2]) == 0 and int(counts[0, 0]) == H.PRE[0]
    if agnostic:
        assert int(counts[0, 1]) == 1024                                        # more passing anchors than the sort buffer: radix form
    # decode
    dec, dets, dlab = ops.predict_decode_classes(box, dirs, anchors, top_idx, top_score, rotate=rotate)
    for c in range(H.C):
        d1, t1, l1 = ops.predict_decode(box, dirs, anchors, top_idx[:, c].contiguous(), top_score[:, c].contiguous(), rotate=rotate)
        assert torch.equal(dec[:, c].view(torch.int32), d1.view(torch.int32)) and torch.equal(dets[:, c].view(torch.int32), t1.view(torch.int32))
        assert torch.equal(dlab[:, c], l1)
    # NMS
    kind, sem = ("rotate", "cpu") if rotate else ("axis_aligned", "numba")
    iou_t = torch.tensor(H.IOU, dtype=torch.float32, device="cuda")
    post_t = torch.tensor(H.POST, dtype=torch.int32, device="cuda")
    keep, num_keep = ops.nms_sorted_items(dets, counts, iou_t, post_t, kind, sem)
    loops = []
    for c in range(H.C):
        k1, n1 = ops.nms_sorted(dets[:, c].contiguous(), counts[:, c].contiguous(), H.IOU[c], kind, sem, post_max=H.POST[c])
        loops.append((k1, n1))
        assert torch.equal(n1, num_keep[:, c]), (c, n1.tolist(), num_keep[:, c].tolist())
        for b in range(H.B):
            assert torch.equal(keep[b, c, :int(n1[b])], k1[b, :int(n1[b])]), (b, c)
    assert int(num_keep.max()) > 1 and (num_keep <= post_t.unsqueeze(0)).all()
    # finalize
    off = np.concatenate([[0], np.cumsum(H.POST)]).astype(np.int32)
    off_t = torch.from_numpy(off).cuda()
    r6 = torch.tensor(H.config()["post_center_range"], dtype=torch.float32, device="cuda")
    out = ops.predict_finalize_classes(dec, top_score, dlab, keep, num_keep, off_t, int(off[-1]), True, 0.0, 1.0, 2, r6)
    assert out["boxes"].shape == (H.B, int(off[-1]), 7)
    for c in range(H.C):
        k1, n1 = loops[c]
        lab = torch.full((H.B, kout), c, dtype=torch.int32, device="cuda")
        one = ops.predict_finalize(dec[:, c].contiguous(), top_score[:, c].contiguous(), lab, dlab[:, c].contiguous(), k1, n1, H.POST[c],
                                   True, 0.0, 1.0, 2, r6)
        p = one["valid"].shape[1]
        seg = slice(int(off[c]), int(off[c]) + p)
        v = one["valid"]
        assert torch.equal(out["valid"][:, seg], v) and not out["valid"][:, int(off[c]) + p:int(off[c + 1])].any()
        assert torch.equal(out["boxes"][:, seg][v].view(torch.int32), one["boxes"][v].view(torch.int32))
        assert torch.equal(out["scores"][:, seg][v].view(torch.int32), one["scores"][v].view(torch.int32))
        assert (out["labels"][:, int(off[c]):int(off[c + 1])] == c).all()
    assert out["valid"].any(1).all() and not out["valid"].all()


# ---------------------------------------------------------------- (c)
def test_a_frame_without_survivors_has_no_valid_row(fx):
    from second_amd.models import SecondDetector
    det = SecondDetector(H.config(True, True)).eval().cuda()
    cls, box, dirs = head_views(fx, torch.float32)
    cls = cls.clone()
    cls[1] = -9.0
    with torch.no_grad():
        out = det.predict_device({"cls_preds": cls, "box_preds": box, "dir_cls_preds": dirs}, H.B)
    assert not out["valid"][1].any() and out["valid"][0].any()


# ---------------------------------------------------------------- (d)
def test_refused_arguments_launch_nothing(fx, ops):
    from second_amd import runtime as rt
    cls, _, _ = head_views(fx, torch.float32)
    l = rt.lib()
    ia = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
    top_idx = torch.full((H.B, H.C, 1024), -7, dtype=torch.int32, device="cuda")
    top_score = torch.full((H.B, H.C, 1024), -7.0, device="cuda")
    counts = torch.full((H.B, H.C), -7, dtype=torch.int32, device="cuda")
    mask = torch.ones((H.B, H.A * HW), dtype=torch.uint8, device="cuda")

    def call(k=H.PRE, thr=H.THR, m=None):
        return l.sec_predict_select_classes(rt.ptr(cls), ops._strides5(cls), H.B, H.A, H.H, H.W, H.C, ia([0, 2, 4]), ia([2, 4, 6]), ia(k),
                                            rt.f_arr(thr), 1024, rt.ptr(top_idx), rt.ptr(top_score), rt.ptr(counts), rt.SEC_F32, rt.ptr(m),
                                            rt.stream())
    assert call(thr=(0.3, 0.0, 0.4)) == -3 and call(k=(16, 1025, 7)) == -3 and call(m=mask) == -3
    torch.cuda.synchronize()
    assert (top_idx == -7).all() and (top_score == -7.0).all() and (counts == -7).all()
    with pytest.raises(rt.SecondHipError, match="SEC_E_UNSUPPORTED"):
        ops.predict_select_classes(cls, ranges(False), H.PRE, H.THR, anchor_mask=mask)
    assert call() == 0
    torch.cuda.synchronize()
    assert (counts >= 0).all()


# ---------------------------------------------------------------- accelerate_model
def test_accelerate_model_serves_a_multiclass_network_on_both_lanes():
    """net(example) of a reference-shaped network with _multiclass_nms: adopted, served from the captured graph with P = sum(post)
    output rows per frame, synchronous and deferred lanes alike, and the detections are those of the object's own module graph (the
    torch formulation)."""
    from lite_helpers import clouds_for
    from reference_standin import build_voxelnet, example_of
    from second_amd import compat, models as M, synthetic as syn
    from test_gpu_dropin_fused import _same
    thr = [0.3, 0.3, 0.4]                              # (above the score of the sharpened heads' empty regions: no tied candidates)
    cfg = dict(H.config(), nms_score_thresholds=thr)

    def make():
        torch.manual_seed(0)
        net = build_voxelnet(cfg)
        begin = M.anchor_class_ranges(cfg, net.feature_map_size)
        net._multiclass_nms, net._nms_class_agnostic, net._nms_score_thresholds = True, False, list(thr)
        net._nms_pre_max_sizes, net._nms_post_max_sizes, net._nms_iou_thresholds = list(H.PRE), list(H.POST), list(H.IOU)
        net.target_assigner.anchors_range = lambda c: (begin[c], begin[c + 1])
        syn.randomise_like_trained(net, seed=1)
        return net.eval().cuda()
    net = make()
    assert net.multiclass is not None and not net.fused_predict
    clouds = clouds_for(cfg, range(2), num_points=5000, num_voxels=3500)
    ex = example_of(net, clouds, torch.device("cuda"))
    one = ex["coordinates"][:, 0] == 0
    with torch.no_grad():
        p = net.network_forward(ex["voxels"][one], ex["num_points"][one], ex["coordinates"][one], 1)
        syn.sharpen_heads(net, p["cls_preds"].float(), p["box_preds"].float())
        want = net(ex)
    state = net.state_dict()
    assert sum(w["scores"].shape[0] for w in want) >= 4
    for lane, kw in (("sync", {}), ("deferred", {"deferred": True})):
        n = make()
        n.load_state_dict(state)
        compat.accelerate_model(n, multiclass_nms=True, **kw)
        with torch.no_grad():
            got = [dict(r) for r in n(dict(ex))]
        eng = n._second_amd_engine
        assert eng.stats["original_calls"] == 0 and eng.stats["fused_calls"] + eng.stats["deferred_calls"] >= 1, (lane, eng.stats)
        assert eng._det.multiclass is not None and eng._det.multiclass["P"] == sum(H.POST)
        assert [s.outs["post"] for s in eng._sessions.values()] == [sum(H.POST)]
        _same(got, want)
        for g in got:
            assert (np.diff(g["label_preds"].cpu().numpy()) >= 0).all()


# ---------------------------------------------------------------- (e)
def test_forward_points_under_a_graph_equals_its_eager_result():
    from lite_helpers import clouds_for
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    cfg = dict(H.config(True, False), nms_score_thresholds=[0.02, 0.01, 0.03])
    torch.manual_seed(0)
    det = SecondDetector(cfg)
    syn.randomise_like_trained(det, seed=1)
    det = det.eval().cuda().prepare_inference(torch.bfloat16)
    pts, offs = syn.batch_clouds(clouds_for(cfg, range(2), num_points=5000, num_voxels=3500))
    pts, offs = torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda()
    calls = []
    real = det._predict_multiclass_fused
    det._predict_multiclass_fused = lambda *a, **k: calls.append(1) or real(*a, **k)
    with torch.no_grad():
        det.calibrate(pts, offs)
        eager = {k: v.clone() for k, v in det.forward_points(pts, offs, static=True).items()}
        det.check_overflow()
    assert calls and eager["boxes"].shape == (2, sum(H.POST), 7)
    replay, outs = det.make_graphed(pts, offs)
    replay()
    torch.cuda.synchronize()
    det.check_overflow()
    assert int(eager["valid"].sum()) > 0
    for k in eager:
        assert torch.equal(eager[k], outs[k]), k
