"""On the MI355X: sec_kitti_annos_f64 and second_amd.kitti_annos against the executed reference (tests/golden/kitti_annos.npz) and,
for the hand-built cases and the compaction shapes, against the float64 restatement of tests/kitti_annos_helpers.py (which
test_kitti_annos_host.py holds to the same fixture).

Exact: the kept set, its order, out_off, src, labels, scores, dimensions, rotation_y and the dicts' keys, dtypes and shapes -- every
compared value of the drop rule lies at least 1e3 error bounds from its threshold in everything that runs here (the fixture by
construction, random inputs by drawing such rows again), so no decision hangs on a last bit.  location and bbox: the helper's first-order forward
bound per element; alpha: two float32 ulps of the arc tangent plus the rounding of the sum.  The hand-built cases use powers of two,
where every operation is exact up to one shared division: there the bbox must EQUAL the restatement, NaNs in the same places."""
import numpy as np
import pytest
import torch

import kitti_annos_helpers as H
import kitti_eval_helpers as EH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return H.load_fixture()


def run(boxes, scores, labels, det_off, lidar2cam, P2, image_hw):
    """ops.kitti_annos on numpy inputs -> the compacted numpy arrays (cut at n = out_off[-1]); asserts the inputs were not written."""
    from second_amd import ops
    dev = torch.device("cuda")
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
           (np.asarray(boxes, np.float32).reshape(-1, 7), np.asarray(scores, np.float32), np.asarray(labels, np.int32), np.asarray(det_off, np.int32),
            np.asarray(lidar2cam, np.float64), np.asarray(P2, np.float64), np.asarray(image_hw, np.int32))]
    before = [t.clone() for t in ins]
    out = ops.kitti_annos(*ins)
    host = ops.kitti_annos_views(out["packed"].cpu().numpy(), ins[0].shape[0], len(det_off) - 1)
    assert all(torch.equal(a, b) for a, b in zip(ins, before)), "an input was written"
    n = int(host["out_off"][-1])
    assert 0 <= n <= ins[0].shape[0]
    return {k: (v if k == "out_off" else v[:n]) for k, v in host.items()}


def check(got, want, label, exact_bbox=False):
    """``got`` of :func:`run` against a helpers.compact result (values and bounds)."""
    assert np.array_equal(got["out_off"], want["out_off"]), label
    assert np.array_equal(got["src"], want["src"]) and np.array_equal(got["label"], want["label"]) and np.array_equal(got["score"], want["score"]), label
    assert np.array_equal(got["box3d"][:, 3:], want["box3d"][:, 3:]), label                           # dimensions, rotation_y: promoted float32
    for key, g, w, bound in (("bbox", got["bbox"], want["bbox"], want["bbox_err"]), ("location", got["box3d"][:, :3], want["box3d"][:, :3], want["location_err"]),
                             ("alpha", got["alpha"], want["alpha"], want["alpha_err"])):
        ok, share = H.within(g, w, bound)
        print(f"{label} {key}: largest share of the bound used {share:.3g}")
        assert ok, (label, key)
    if exact_bbox:
        assert np.array_equal(got["bbox"], want["bbox"], equal_nan=True) and np.array_equal(got["box3d"], want["box3d"]), label


def test_device_against_the_fixture(fx):
    got = run(fx["boxes"], fx["scores"], fx["labels"], fx["det_off"], fx["lidar2cam"], fx["P2"], fx["image_shape"])
    r = H.restate(fx["boxes"], fx["det_off"], fx["lidar2cam"], fx["P2"], fx["image_shape"])
    want = H.compact(r, fx["scores"], fx["labels"], fx["det_off"])              # the bounds, and src (which the dicts do not record)
    rec = lambda key: np.concatenate([a[key] for a in fx["annos"] if len(a["name"])], 0)
    want.update(bbox=rec("bbox"), alpha=rec("alpha"), out_off=fx["out_off"], score=rec("score"),
                box3d=np.concatenate([rec("location"), rec("dimensions"), rec("rotation_y")[:, None]], 1))
    check(got, want, "fixture")
    assert np.array_equal(np.array(fx["class_names"])[got["label"]], rec("name"))


def _cuda_detections(fx):
    off = fx["det_off"]
    dev = torch.device("cuda")
    return [{"box3d_lidar": torch.from_numpy(fx["boxes"][off[i]:off[i + 1]].copy()).to(dev), "scores": torch.from_numpy(fx["scores"][off[i]:off[i + 1]].copy()).to(dev),
             "label_preds": torch.from_numpy(fx["labels"][off[i]:off[i + 1]].copy()).to(dev), "metadata": {"image_idx": int(fx["image_idx"][i])}}
            for i in range(len(off) - 1)]


class _Recording(H.StandinDataset):
    def _second_amd_original_convert_detection_to_kitti_annos(self, detection):
        return "the reference's own result"


def test_drop_in_returns_the_recorded_dicts(fx):
    from second_amd import kitti_annos as KA
    ds = _Recording(H.fixture_infos(fx), fx["class_names"])
    det = _cuda_detections(fx)
    before, stats = [d["box3d_lidar"].clone() for d in det], dict(KA.stats)
    annos = KA.convert_detection_to_kitti_annos(ds, det)
    assert isinstance(annos, KA.DeviceAnnoList) and len(annos) == len(det) and KA.stats["device"] == stats["device"] + 1
    assert all(torch.equal(a, d["box3d_lidar"]) for a, d in zip(before, det)), "the detections were edited (the reference does, the device form must not)"
    r = H.restate(fx["boxes"], fx["det_off"], fx["lidar2cam"], fx["P2"], fx["image_shape"])
    bounds = H.compact(r, fx["scores"], fx["labels"], fx["det_off"])
    for i, (got, want, lay, d) in enumerate(zip(annos, fx["annos"], fx["layout"], det)):
        a, b = fx["out_off"][i], fx["out_off"][i + 1]
        assert list(got) == H.ANNO_KEYS + ["metadata"] and got["metadata"] is d["metadata"]
        for k in H.ANNO_KEYS:
            dtype, shape = np.dtype(lay[k][0]), tuple(lay[k][1])
            assert got[k].shape == shape and (got[k].dtype == dtype or (dtype.kind == "U" and got[k].dtype.kind == "U")), (i, k)
        for k in ("name", "truncated", "occluded", "dimensions", "rotation_y", "score"):
            assert np.array_equal(got[k], want[k]), (i, k)
        for k, bound in (("bbox", bounds["bbox_err"]), ("location", bounds["location_err"]), ("alpha", bounds["alpha_err"])):
            assert H.within(got[k], want[k], bound[a:b])[0], (i, k)
    held = annos.handoff()
    assert held is not None and held["dt_off"].is_cuda and held["dt_off"].cpu().tolist() == fx["out_off"].tolist()
    assert held["dt_score"].dtype == torch.float64 and held["max_dt"] == int(np.diff(fx["out_off"]).max())
    assert held["dt_name"].cpu().tolist() == [EH_NAME_IDS[n.lower()] for a in fx["annos"] for n in a["name"]]
    # on the device too, what is outside the contract goes to the original: float16 boxes, a 3 x 4 P2
    half = [dict(d, box3d_lidar=d["box3d_lidar"].half()) for d in det]
    assert KA.convert_detection_to_kitti_annos(ds, half) == "the reference's own result" and "boxes" in KA.last_fallback_reason
    narrow = _Recording([dict(i, calib=dict(i["calib"], P2=i["calib"]["P2"][:3])) for i in H.fixture_infos(fx)], fx["class_names"])
    assert KA.convert_detection_to_kitti_annos(narrow, det) == "the reference's own result" and "calibration" in KA.last_fallback_reason
    assert KA.stats["fallback"] == stats["fallback"] + 2
    # a label outside the class names: IndexError, as the reference's list indexing
    with pytest.raises(IndexError):
        KA.convert_detection_to_kitti_annos(_Recording(H.fixture_infos(fx), fx["class_names"][:2]), det)


EH_NAME_IDS = {'car': 0, 'pedestrian': 1, 'cyclist': 2}


def test_hand_built_edges_equal_the_restatement():
    """Identity lidar -> camera, P2 = diag(2, 2, 1) with a fourth column that must not matter, r = 0, small integers: every sum is exact.
    A box w = l = h = 2 at lidar (x, y, z) has corners x +- 1, {y - 2, y}, (z - 1) +- 1 and image points (2 cx / cz, 2 cy / cz)."""
    P = np.array([[2.0, 0, 0, 1000.0], [0, 2.0, 0, 1000.0], [0, 0, 1.0, 1000.0], [0, 0, 0, 1.0]])
    rows = [
        ([17, 2, 4, 2, 2, 2, 0], (64, 8)),         # min u = 2 * 16 / 4 = 8 == W: kept (the rule is a strict >); bbox = (8, 0, 8, 2)
        ([17, 2, 4, 2, 2, 2, 0], (64, 7)),         # the same box, W = 7: dropped
        ([-1, 2, 4, 2, 2, 2, 0], (64, 128)),       # max u = 2 * 0 / 2 = 0: kept (strict <); bbox = (0, 0, 0, 2)
        ([-1.5, 2, 4, 2, 2, 2, 0], (64, 128)),     # max u = -0.25: dropped
        ([3, 66, 4, 2, 2, 2, 0], (32, 128)),       # min v = 2 * 64 / 4 = 32 == H: kept
        ([3, 66.5, 4, 2, 2, 2, 0], (32, 128)),     # min v = 32.25 > H: dropped
        ([1, 0, 1, 0, 2, 2, 0], (64, 128)),        # w = 0, z' = 0: every corner on the image plane, 0 / 0 and 4 / 0: a NaN bbox, KEPT
        ([3, 2, -6, 2, 2, 2, 0], (64, 128)),       # wholly behind the camera, x > 0: u < 0 there, dropped
        ([-3, -1, -6, 2, 2, 2, 0], (64, 128)),     # wholly behind, x < 0 and y < 0: the mirror image lands inside and is KEPT (nothing is clamped)
        ([5, 2, 1, 2, 2, 2, 0], (64, 128)),        # across the image plane: cz in {-1, 1}, u from -12 to 12, v from -4 to 4: kept, clamped at 0
    ]
    boxes = np.array([r[0] for r in rows], np.float32)
    hw = np.array([r[1] for r in rows], np.int32)
    n = len(rows)
    det_off = np.arange(n + 1, dtype=np.int32)                      # one image per row
    eye, P2 = np.tile(np.eye(4), (n, 1, 1)), np.tile(P, (n, 1, 1))
    scores, labels = np.linspace(0.1, 0.9, n).astype(np.float32), (np.arange(n) % 3).astype(np.int32)
    r = H.restate(boxes, det_off, eye, P2, hw)
    assert r["keep"].tolist() == [True, False, True, False, True, False, True, False, True, True]
    assert r["bbox"][0].tolist() == [8.0, 0.0, 8.0, 2.0] and r["bbox"][2].tolist() == [0.0, 0.0, 0.0, 2.0] and np.isnan(r["bbox"][6]).all()
    assert r["raw_bbox"][4, 1] == 32.0 and r["bbox"][9].tolist() == [0.0, 0.0, 12.0, 4.0] and (r["raw_bbox"][8] > 0).all()
    got = run(boxes, scores, labels, det_off, eye, P2, hw)
    check(got, H.compact(r, scores, labels, det_off), "hand-built", exact_bbox=True)
    assert got["out_off"].tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6] and got["src"].tolist() == [0, 2, 4, 6, 8, 9]
    assert np.isnan(got["bbox"][3]).all() and not np.isnan(got["box3d"]).any()


def _boxes(rng, n, mode):
    boxes = H.random_boxes(rng, n)
    if mode == "all":
        boxes[:, 0], boxes[:, 1] = rng.uniform(12, 40, n), rng.uniform(-3, 3, n)
    if mode == "none":
        boxes[:, 0], boxes[:, 1] = rng.uniform(8, 12, n), rng.uniform(60, 80, n)            # far to the left of the image
    return boxes


def _shape_case(rng, n, images, mode):
    rect, trv2c, p2, hw = H.synthetic_calibration(rng, images, other_size_at=0)
    l2c = np.stack([a @ b for a, b in zip(rect, trv2c)])
    if images == 1:
        det_off = np.array([0, n], np.int64)
    else:
        cuts = np.sort(rng.integers(0, n + 1, images - 1))
        cuts[:3], cuts[-3:], cuts[100:110] = 0, n, cuts[100]          # empty images first, last and in a run
        det_off = np.concatenate([[0], np.sort(cuts), [n]])
    boxes = _boxes(rng, n, mode)
    for _ in range(20):               # rows whose decision could hang on a last bit are drawn again: N stays N
        ratio, _ = H.decision_margins(H.restate(boxes, det_off, l2c, p2, hw))
        close = ratio.min(axis=1) < H.MARGIN if n else np.zeros(0, bool)
        if not close.any():
            break
        boxes[close] = _boxes(rng, n, mode)[close]
    assert not close.any()
    return boxes, det_off, l2c, p2, hw


@pytest.mark.parametrize("n,images,mode", [(0, 1, "random"), (0, 300, "random"), (1, 1, "all"), (1, 300, "none"), (255, 1, "random"), (256, 300, "random"),
                                           (257, 1, "random"), (257, 300, "all"), (65537, 1, "random"), (65537, 300, "random"), (65537, 300, "none"),
                                           (65537, 1, "all")])
def test_compaction_shapes(n, images, mode):
    """N around the 256-row count blocks and one past what one round of the second-level scan covers (256 * 256 rows); one image and
    300 with empty ones first, last and in runs; everything kept and nothing kept."""
    rng = np.random.default_rng(1000 + n + images)
    boxes, det_off, l2c, p2, hw = _shape_case(rng, n, images, mode)
    assert len(boxes) == n and det_off[-1] == n and len(det_off) == images + 1
    scores, labels = rng.uniform(0, 1, n).astype(np.float32), rng.integers(0, 3, n).astype(np.int32)
    r = H.restate(boxes, det_off, l2c, p2, hw)
    want = H.compact(r, scores, labels, det_off)
    if mode == "all":
        assert r["keep"].all()
    if mode == "none":
        assert not r["keep"].any()
    if mode == "random" and n > 200:
        assert 0 < r["keep"].sum() < n
    got = run(boxes, scores, labels, det_off, l2c, p2, hw)
    check(got, want, f"N={n} I={images} {mode}")
    assert got["out_off"][0] == 0 and (np.diff(got["out_off"]) >= 0).all() and len(got["out_off"]) == images + 1


def _gt_for(fx, rng):
    """Synthetic gt for the fixture's images (kitti_eval_helpers.random_annos), the first rows of every image moved onto jittered
    copies of that image's recorded detections so that the matching has work to do at all three metrics."""
    gts, _ = EH.random_annos(rng, len(fx["annos"]), 6, 1, classes=("Car", "Pedestrian", "Cyclist"), dontcare=1)
    for g, d in zip(gts, fx["annos"]):
        k = min(4, len(d["name"]))
        if k:
            g["name"][:k] = d["name"][:k]
            g["bbox"][:k] = d["bbox"][:k] + rng.normal(0, 1.0, (k, 4))
            g["location"][:k] = d["location"][:k] + rng.normal(0, 0.05, (k, 3))
            g["dimensions"][:k] = d["dimensions"][:k] * rng.uniform(0.97, 1.03, (k, 3))
            g["rotation_y"][:k] = d["rotation_y"][:k] + rng.normal(0, 0.03, k)
            g["alpha"][:k] = d["alpha"][:k] + rng.normal(0, 0.1, k)
    return gts


def test_handoff_to_the_evaluation_is_bit_equal_to_the_plain_route(fx, monkeypatch):
    from second_amd import kitti_annos as KA, kitti_eval as KE
    ds = _Recording(H.fixture_infos(fx), fx["class_names"])
    annos = KA.convert_detection_to_kitti_annos(ds, _cuda_detections(fx))
    gts = _gt_for(fx, np.random.default_rng(11))
    calls = {"handoff": 0}
    raw = KE._pack_handoff

    def counted(*a):
        calls["handoff"] += 1
        return raw(*a)
    monkeypatch.setattr(KE, "_pack_handoff", counted)
    mo = EH.official_min_overlaps([0, 1, 2])
    plain = list(annos)
    results = {}
    for metric in range(3):
        a = KE.eval_class_v3(gts, annos, [0, 1, 2], EH.DIFFICULTYS, metric, mo, True, z_axis=1, z_center=1.0)
        cache = annos.pack_cache
        assert calls["handoff"] == metric + 1 and cache is not None and cache[0] is gts
        if metric:
            assert cache[2] is first_pack, "the gt side is packed once for the calls of a val pass"
        first_pack = cache[2]
        b = KE.eval_class_v3(gts, plain, [0, 1, 2], EH.DIFFICULTYS, metric, mo, True, z_axis=1, z_center=1.0)
        assert calls["handoff"] == metric + 1                          # a plain list never takes the hand-off
        for k in ("precision", "orientation", "thresholds", "recall", "min_overlaps"):
            assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype, (metric, k)
        assert np.nanmax(a["precision"]) > 0 and (a["thresholds"] > 0).any(), "the synthetic gt matches nothing: the comparison would be empty"
        results[metric] = a
    assert all(k.startswith("gt_") or k.startswith("dt_") or k in ("dc_bbox", "dc_off", "ov_off") for k in first_pack["_device"])
    assert all(v.is_cuda for v in first_pack["_device"].values()) and "gt_bbox" in first_pack["_device"]
    # another gt list: packed anew
    gts2 = list(gts)
    KE.eval_class_v3(gts2, annos, [0, 1, 2], EH.DIFFICULTYS, 0, mo, True)
    assert annos.pack_cache[0] is gts2 and annos.pack_cache[2] is not first_pack
    # one dict's name replaced: the list is not what was built any more, the plain route serves the call and the results still agree
    n_before = calls["handoff"]
    busiest = int(np.argmax([len(a["name"]) for a in annos]))
    annos[busiest] = dict(annos[busiest], name=annos[busiest]["name"].copy())
    assert annos.handoff() is None
    for metric in range(3):
        c = KE.eval_class_v3(gts, annos, [0, 1, 2], EH.DIFFICULTYS, metric, mo, True, z_axis=1, z_center=1.0)
        for k in ("precision", "orientation", "thresholds"):
            assert np.array_equal(c[k], results[metric][k], equal_nan=True), (metric, k)
    assert calls["handoff"] == n_before
