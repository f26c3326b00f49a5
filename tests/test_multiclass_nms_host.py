"""CPU-only: multi-class NMS (use_multi_class_nms, voxelnet.py:458-547).

tests/golden/multiclass_nms.npz holds what the reference's own VoxelNet.predict returns (tests/golden/make_golden_multiclass_nms.py);
the plain-torch formulation of SecondDetector.predict_device must reproduce it (kept set, order and labels exactly; scores and boxes to
the tolerance of the predict comparison in tests/test_dropin_reference.py).  dropin.model_config reads the settings off a network and
refuses the combinations the device path does not reproduce by name; a config without the key predicts what it predicted before;
the new C entry points validate their arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import multiclass_nms_helpers as H


@pytest.fixture(scope="module")
def fx():
    return H.load()


def frames_of(out):
    res = []
    for b in range(out["valid"].shape[0]):
        m = out["valid"][b].cpu()
        res.append({"boxes": out["boxes"][b].cpu()[m].numpy(), "scores": out["scores"][b].cpu()[m].numpy(),
                    "labels": out["labels"][b].cpu()[m].numpy().astype(np.int64)})
    return res


def assert_frames(got, want, tag):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["labels"], w["labels"]), (tag, f, g["labels"].tolist(), w["labels"].tolist())
        np.testing.assert_allclose(g["scores"], w["scores"], rtol=1e-5, atol=1e-6, err_msg=f"{tag} frame {f}")
        np.testing.assert_allclose(g["boxes"], w["boxes"], rtol=1e-4, atol=1e-4, err_msg=f"{tag} frame {f}")


def test_fixture_has_the_cases_it_was_built_for(fx):
    assert fx["cls"].shape == (H.B, H.A, H.H, H.W, H.C) and fx["cls"].dtype == np.float32
    n = H.A * H.H * H.W
    s = 1.0 / (1.0 + np.exp(-fx["cls"].astype(np.float64).reshape(H.B, n, H.C)))
    assert ((s[:, :, 1] >= H.THR[1]).sum(1) > 1024).all()                       # class-agnostic: more passing anchors than any pre_max
    assert ((s[:, :2 * H.H * H.W, 0] >= H.THR[0]).sum(1) > H.PRE[0]).all()      # more candidates than pre_max
    assert (s[1, :, 2] >= H.THR[2]).sum() == 0 and (s[0, 4 * H.H * H.W:, 2] >= H.THR[2]).sum() > 0
    for name, frames in fx["cases"].items():
        for fr in frames:
            assert len(fr["labels"]) > 0 and (np.diff(fr["labels"]) >= 0).all()  # every frame keeps something; classes in class order
    assert 2 not in fx["cases"]["rot_ranges"][1]["labels"]


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_torch_formulation_equals_the_reference(fx, name):
    import oracle_backend
    from second_amd.models import SecondDetector
    rotate, agnostic = H.CASES[name]
    det = SecondDetector(H.config(rotate, agnostic)).eval()
    assert det.multiclass is not None and det.multiclass["P"] == sum(H.POST)
    assert det.multiclass["a_ranges"] == ([(0, H.A)] * H.C if agnostic else [(0, 2), (2, 4), (4, 6)])
    with torch.no_grad(), oracle_backend.installed():
        out = det.predict_device(H.preds_of(fx), H.B)
    assert out["boxes"].shape == (H.B, sum(H.POST), 7) and out["valid"].dtype == torch.bool
    assert_frames(frames_of(out), fx["cases"][name], name)


def test_a_frame_without_survivors_has_no_valid_row(fx):
    import oracle_backend
    from second_amd.models import SecondDetector
    det = SecondDetector(H.config(True, False)).eval()
    preds = H.preds_of(fx)
    preds["cls_preds"] = preds["cls_preds"].clone()
    preds["cls_preds"][1] = -9.0
    with torch.no_grad(), oracle_backend.installed():
        out = det.predict_device(preds, H.B)
    assert not out["valid"][1].any() and out["valid"][0].any()


def test_config_without_the_key_predicts_as_before(fx):
    """The single-list predict is untouched: same calls, same output with and without the (ignored) per-class lists."""
    import oracle_backend
    from second_amd.models import SecondDetector
    plain = dict(H.config(multiclass=False), nms_pre_max_size=150)
    with_lists = dict(plain, nms_score_thresholds=list(H.THR), nms_pre_max_sizes=list(H.PRE), nms_class_agnostic=True, multiclass_nms=False)
    outs = []
    for cfg in (plain, with_lists):
        det = SecondDetector(cfg).eval()
        assert det.multiclass is None
        with torch.no_grad(), oracle_backend.installed():
            outs.append(det.predict_device(H.preds_of(fx), H.B))
    assert outs[0]["boxes"].shape == (H.B, 100, 7)
    for k in ("boxes", "scores", "labels", "valid"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    # labels of the single-list mode are the best class per anchor: not the per-class result
    got = frames_of(outs[0])
    assert any(not np.array_equal(g["labels"], w["labels"]) for g, w in zip(got, fx["cases"]["rot_ranges"]))


def test_refused_configurations_are_named():
    from second_amd import models as M
    cfg = H.config()
    with pytest.raises(ValueError, match="score threshold <= 0"):
        M.SecondDetector(dict(cfg, nms_score_thresholds=[0.3, 0.0, 0.4]))
    with pytest.raises(ValueError, match="nms_pre_max_sizes has 2 entries for 3 classes"):
        M.SecondDetector(dict(cfg, nms_pre_max_sizes=[16, 7]))
    with pytest.raises(ValueError, match="multi-head"):
        M.multiclass_nms_settings(dict(M.ALL_PP_MHEAD, multiclass_nms=True), 20, [1, 100, 100])
    det = M.SecondDetector(cfg).eval()
    preds = {k: torch.zeros(H.B, H.A, H.H, H.W, c) for k, c in (("cls_preds", H.C), ("box_preds", 7), ("dir_cls_preds", 2))}
    with pytest.raises(ValueError, match="multiclass_nms with anchors_mask"):
        det.predict_device(preds, H.B, anchors_mask=torch.ones(H.B, H.A * H.H * H.W, dtype=torch.uint8))
    with pytest.raises(ValueError, match="multi-head"):
        det.predict_device({k: [v] for k, v in preds.items()}, H.B)
    # scalar settings stand for every class when a list is absent
    mc = M.multiclass_nms_settings(dict(H.config(multiclass=False), multiclass_nms=True), H.A, [1, H.H, H.W])
    assert mc["pre"] == [1000] * 3 and mc["post"] == [100] * 3 and mc["P"] == 300 and not mc["agnostic"]


def standin_network(agnostic=False):
    from reference_standin import build_voxelnet
    from second_amd import models as M
    cfg = H.config(multiclass=False)
    net = build_voxelnet(cfg)
    begin = M.anchor_class_ranges(cfg, net.feature_map_size)
    net._multiclass_nms, net._nms_class_agnostic = True, agnostic
    net._nms_score_thresholds, net._nms_pre_max_sizes = list(H.THR), list(H.PRE)
    net._nms_post_max_sizes, net._nms_iou_thresholds = list(H.POST), list(H.IOU)
    net.target_assigner.anchors_range = lambda c: (begin[c], begin[c + 1])
    return net


def test_model_config_reads_the_settings_off_the_network():
    from second_amd import dropin, models as M
    for agnostic in (False, True):
        cfg = dropin.model_config(standin_network(agnostic), multiclass_nms=True)
        assert cfg["multiclass_nms"] is True and cfg["nms_class_agnostic"] is agnostic
        assert cfg["nms_score_thresholds"] == list(H.THR) and cfg["nms_pre_max_sizes"] == list(H.PRE)
        assert cfg["nms_post_max_sizes"] == list(H.POST) and cfg["nms_iou_thresholds"] == list(H.IOU)
        assert ("class_anchor_ranges" in cfg) is (not agnostic)
        mc = M.multiclass_nms_settings(cfg, H.A, [1, H.H, H.W])                 # an adopted config carries no anchor table
        assert mc["a_ranges"] == ([(0, H.A)] * H.C if agnostic else [(0, 2), (2, 4), (4, 6)]) and mc["P"] == sum(H.POST)
    plain = standin_network()
    plain._multiclass_nms = False
    assert "multiclass_nms" not in dropin.model_config(plain)                   # existing configs get no new key
    assert "multiclass_nms" not in dropin.model_config(plain, multiclass_nms=True)
    with pytest.raises(dropin.NotAccelerable, match=r"multiclass_nms \(served on request"):   # not asked for: refused by name, as before
        dropin.model_config(standin_network())


def test_model_config_refuses_by_name():
    from second_amd import dropin
    net = standin_network()
    net._nms_score_thresholds = [0.3, 0.0, 0.4]
    with pytest.raises(dropin.NotAccelerable, match="multiclass_nms with a score threshold <= 0"):
        dropin.model_config(net, multiclass_nms=True)
    net = standin_network()
    net._nms_pre_max_sizes = [16]
    with pytest.raises(dropin.NotAccelerable, match="one threshold / size per class"):
        dropin.model_config(net, multiclass_nms=True)
    net = standin_network()
    net.rpn.__class__ = type("RPNNoHead", (type(net.rpn),), {})                 # a multi-head network's trunk
    with pytest.raises(dropin.NotAccelerable, match="multiclass_nms on a multi-head network"):
        dropin.model_config(net, multiclass_nms=True)


def test_entry_points_exist_and_validate_before_any_launch():
    from second_amd import runtime as rt
    from test_capi_symbols import header_functions
    l = rt.lib()
    hdr = header_functions()
    for n in ("sec_predict_select_classes", "sec_predict_decode_classes", "sec_nms_sorted_items_f32", "sec_predict_finalize_classes"):
        assert n in hdr and n in rt.SYMBOLS and hasattr(l, n), n
    assert l.sec_abi_version() == 9
    one = ctypes.c_void_p(4096)                      # never dereferenced: validation fails first
    st = (ctypes.c_int64 * 5)(6 * 384 * 3, 3, 24 * 18, 18, 1)
    ia = lambda *v: (ctypes.c_int * len(v))(*v)

    def sel(begin=(0, 2, 4), end=(2, 4, 6), k=(16, 1024, 7), thr=(0.3, 0.05, 0.4), kout=1024, mask=None, nc=3):
        return l.sec_predict_select_classes(one, st, 2, 6, 16, 24, nc, ia(*begin), ia(*end), ia(*k), rt.f_arr(thr), kout, one, one, one,
                                            rt.SEC_F32, mask, None)
    assert sel(thr=(0.3, 0.0, 0.4)) == -3 and sel(thr=(0.3, -1.0, 0.4)) == -3        # a threshold <= 0
    assert sel(k=(16, 1025, 7)) == -3                                                # more than the select ranks
    assert sel(mask=one) == -3                                                       # an anchor mask
    assert sel(nc=33) == -3
    assert sel(k=(16, 0, 7)) == -1 and sel(begin=(0, 2, 6)) == -1 and sel(end=(2, 4, 7)) == -1
    assert sel(kout=100) == -1 and sel(kout=2048) == -1                              # rows of class 1 do not fit / above 1024
    assert l.sec_predict_select_classes(None, st, 2, 6, 16, 24, 3, ia(0, 2, 4), ia(2, 4, 6), ia(16, 1024, 7), rt.f_arr(H.THR), 1024, one, one,
                                        one, rt.SEC_F32, None, None) == -1
    dec = lambda nc, k, box=one: l.sec_predict_decode_classes(box, st, one, st, 2, 2, 6, 16, 24, nc, k, one, one, one, 1, one, one, one, rt.SEC_F32, None)
    assert dec(0, 16) == -1 and dec(3, 0) == -1 and dec(3, 16, None) == -1
    need = l.sec_nms_workspace_bytes(6, 1024)
    nms = lambda items=6, nc=3, thr=one, post=one, ws=one, nbytes=need, kind=0: l.sec_nms_sorted_items_f32(
        one, one, items, nc, 1024, 6, thr, kind, 1, 1.0, post, one, one, ws, nbytes, None)
    assert nms(items=7) == -1 and nms(thr=None) == -1 and nms(post=None) == -1 and nms(kind=2) == -1
    assert nms(nbytes=need - 1) == -2 and nms(ws=None) == -2
    assert nms(items=65536 * 3, nbytes=1 << 62) == -3
    fin = lambda off=one, p=107, nc=3: l.sec_predict_finalize_classes(one, one, one, one, one, off, 2, nc, 1024, p, 1, 0.0, 1.0, 2, one, one, one,
                                                                      one, one, None)
    assert fin(off=None) == -1 and fin(p=0) == -1 and fin(nc=0) == -1
