"""-m gpu: the KITTI AP evaluation on the device (csrc/kitti_eval.hip, second_amd/kitti_eval.py) against tests/golden/kitti_eval.npz
(the reference executed on CPU, tests/golden/make_golden_kitti_eval.py) and, for the hand-built cases, against the numpy restatement of
tests/kitti_eval_helpers.py (held to the same fixture by test_kitti_eval_host.py).

Bounds: metric 0 overlaps are float64 with the reference's operations in its order -- bit exact; metrics 1 and 2 go through the float32
polygon clipper, held to 2e-5 absolute like sec_rotate_iou_f32 (with sinf / cosf in the corners an MI355X gave 4.1e-5 on case A: the
clipper is ill-conditioned at 60 m; the kernel rounds the float64 sine / cosine instead, as the recorded reference does).  Flags, true-positive scores, thresholds, tp / fp / fn are exact.  A
similarity is a float64 sum of n terms (1 + cos) / 2 with sum S: the summation order differs from np.sum's and each cosine may differ
by an ulp, so |error| <= n * 2^-52 * S.  The fixture's overlaps of metrics 1 / 2 keep 1e-4 from every min_overlap in use, so a
last-bit difference of the clipper cannot move a match in the end-to-end tests.  Every test prints the largest similarity error and its
share of the bound (largest share seen on an MI355X: 0.51)."""
import os

import numpy as np
import pytest
import torch

import kitti_eval_helpers as H

pytestmark = pytest.mark.gpu
REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def KE():
    from second_amd import kitti_eval
    return kitti_eval


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


@pytest.fixture(scope="module")
def cases(golden):
    return {name: H.load_case(golden, name) for name in H.CASES}


def _stages(KE, gts, dts, class_ids, metric, mo, aos=False, z_axis=1, z_center=1.0, overlaps=None):
    p = KE.pack(gts, dts)
    ov = None if overlaps is None else torch.from_numpy(np.ascontiguousarray(overlaps)).cuda()
    r = KE.run_stages(p, class_ids, H.DIFFICULTYS, metric, mo, aos, z_axis, z_center, overlaps=ov)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _flat(blocks):
    return np.concatenate([b.reshape(-1) for b in blocks]) if blocks else np.zeros(0)


worst_fraction = [0.0]


def _check(got, want_flags, want, label):
    """``want``: scores (list per configuration, descending), thresholds, n_thresholds, pr [configs, 41, 4]."""
    ig, idt, nvg = want_flags
    assert np.array_equal(got["ignored_gt"], ig) and np.array_equal(got["ignored_dt"], idt), label
    assert np.array_equal(got["num_valid_gt"], nvg), label
    assert np.array_equal(got["n_scores"], [len(s) for s in want["scores"]]), label
    assert np.array_equal(got["tp_count"].sum(1), got["n_scores"])
    for c, s in enumerate(want["scores"]):                      # the multiset of a configuration's true-positive scores
        assert np.array_equal(got["sorted_scores"][c, :len(s)], s), (label, c)
    assert np.array_equal(got["n_thresholds"], want["n_thresholds"]), label
    assert np.array_equal(got["thresholds"], want["thresholds"]), label
    assert np.array_equal(got["counts"], want["pr"][..., :3].astype(np.int32)), (label, np.argwhere(got["counts"] != want["pr"][..., :3])[:5])
    err, bound = np.abs(got["similarity"] - want["pr"][..., 3]), H.similarity_bound(want["pr"])
    print(label, "similarity: largest error", err.max(initial=0.0), "largest fraction of the bound",
          (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    worst_fraction[0] = max(worst_fraction[0], (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    assert (err <= bound).all(), (label, err.max())


# ------------------------------------------------------------------------------------------------------------ overlaps, flags
@pytest.mark.parametrize("name", sorted(H.CASES))
def test_overlaps_against_the_fixture(KE, cases, name):
    from second_amd import ops
    case, c = H.CASES[name], cases[name]
    p = KE.pack(c["gt_annos"], c["dt_annos"])
    t = {k: torch.from_numpy(v).cuda() for k, v in p.items() if isinstance(v, np.ndarray)}
    for metric in range(3):
        boxes = ("dt_bbox", "gt_bbox") if metric == 0 else ("dt_box3d", "gt_box3d")
        got = ops.kitti_eval_overlaps(metric, t["dt_off"], t["gt_off"], t["ov_off"], t[boxes[0]], t[boxes[1]], int(p["ov_off"][-1]), p["max_dt"],
                                      p["max_gt"], case["z_axis"], case["z_center"]).cpu().numpy()
        want = c["flat"][metric]
        assert got.shape == want.shape and got.dtype == np.float64
        print(name, "metric", metric, "largest difference", np.abs(got - want).max(), "non-zero", int((want > 0).sum()), "of", want.size)
        if metric == 0:
            assert np.array_equal(got, want)
        else:
            assert np.abs(got - want).max() <= 2e-5
            assert np.array_equal((got > 0), (want > 0)) or np.abs(got - want)[(got > 0) != (want > 0)].max() <= 2e-5
        if metric == 2:
            assert np.array_equal(got.astype(np.float32).astype(np.float64), got)          # rounded to float32 before it was widened


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_flags_against_the_fixture(KE, golden, cases, name):
    case, c = H.CASES[name], cases[name]
    got = _stages(KE, c["gt_annos"], c["dt_annos"], case["class_ids"], 0, H.official_min_overlaps(case["class_ids"]), overlaps=c["flat"][0])
    assert got["ignored_gt"].dtype == np.int8 and np.array_equal(got["ignored_gt"], golden[f"{name}_ignored_gt"])
    assert np.array_equal(got["ignored_dt"], golden[f"{name}_ignored_dt"])
    assert np.array_equal(got["num_valid_gt"], golden[f"{name}_num_valid_gt"])


# ------------------------------------------------------------------------------------------------------------ the matching on recorded overlaps
@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(H.CASES) for k in H.KINDS])
def test_matching_on_recorded_overlaps(KE, golden, cases, name, kind):
    case, c = H.CASES[name], cases[name]
    flags = (golden[f"{name}_ignored_gt"], golden[f"{name}_ignored_dt"], golden[f"{name}_num_valid_gt"])
    for metric in range(3):
        rec = H.recorded(golden, name, kind, metric)
        got = _stages(KE, c["gt_annos"], c["dt_annos"], case["class_ids"], metric, H.min_overlaps_of(kind, case["class_ids"]), rec["compute_aos"],
                      case["z_axis"], case["z_center"], overlaps=c["flat"][metric])
        _check(got, flags, rec, f"{name} {kind} metric {metric}")
        assert (got["similarity"] == 0).all() or rec["compute_aos"]


def test_pr_is_deterministic(KE, cases):
    case, c = H.CASES["A"], cases["A"]
    mo = H.coco_min_overlaps(case["class_ids"])
    a = _stages(KE, c["gt_annos"], c["dt_annos"], case["class_ids"], 0, mo, True, overlaps=c["flat"][0])
    b = _stages(KE, c["gt_annos"], c["dt_annos"], case["class_ids"], 0, mo, True, overlaps=c["flat"][0])
    assert a["similarity"].any()
    assert a["similarity"].tobytes() == b["similarity"].tobytes() and a["counts"].tobytes() == b["counts"].tobytes()


# ------------------------------------------------------------------------------------------------------------ end to end
def _orientation_tolerance(pr, shape):
    scale = np.where(pr[..., 0] + pr[..., 1] > 0, pr[..., 0] + pr[..., 1], 1.0)
    return np.maximum.accumulate((H.similarity_bound(pr) / scale)[:, ::-1], axis=1)[:, ::-1].reshape(shape) + 1e-300


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(H.CASES) for k in H.KINDS])
def test_eval_class_v3_end_to_end(KE, golden, cases, name, kind):
    case, c = H.CASES[name], cases[name]
    mo = H.min_overlaps_of(kind, case["class_ids"])
    for metric in range(3):
        rec = H.recorded(golden, name, kind, metric)
        before = KE.stats["device"]
        ret = KE.eval_class_v3(c["gt_annos"], c["dt_annos"], case["class_ids"], H.DIFFICULTYS, metric, mo, rec["compute_aos"],
                               z_axis=case["z_axis"], z_center=case["z_center"])
        assert KE.stats["device"] == before + 1
        assert sorted(ret) == ["min_overlaps", "orientation", "precision", "recall", "thresholds"] and ret["min_overlaps"] is mo
        assert ret["precision"].shape == rec["precision"].shape and not ret["recall"].any()
        assert np.array_equal(ret["precision"], rec["precision"], equal_nan=True), (name, kind, metric)
        assert np.array_equal(ret["thresholds"].reshape(-1, 41), rec["thresholds"])
        assert np.array_equal(np.isnan(ret["orientation"]), np.isnan(rec["orientation"]))
        ok = ~np.isnan(rec["orientation"])
        assert (np.abs(ret["orientation"] - rec["orientation"]) <= _orientation_tolerance(rec["pr"], rec["orientation"].shape))[ok].all()


def _map(prec):
    return sum(prec[..., i] for i in range(0, prec.shape[-1], 4)) / 11 * 100


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_result_strings_through_the_reference_seam(KE, golden, cases, name, monkeypatch):
    """With the reference checkout: its own get_official_eval_result / get_coco_eval_result over the installed replacement return the
    recorded strings.  Without it (the GPU machines): the numbers behind those strings, from the replacement's arrays."""
    case, c = H.CASES[name], cases[name]
    want = H.recorded_results(golden, name)
    if os.path.isdir(os.path.join(REF, "second")):
        from second_amd import compat
        compat.install(REF)
        ev = compat.accelerate_eval(statistics=True)
        assert ev.eval_class_v3 is KE.eval_class_v3
        got = {"official": ev.get_official_eval_result(c["gt_annos"], c["dt_annos"], case["classes"], z_axis=case["z_axis"], z_center=case["z_center"]),
               "coco": ev.get_coco_eval_result(c["gt_annos"], c["dt_annos"], case["classes"], z_axis=case["z_axis"], z_center=case["z_center"])}
        for kind in H.KINDS:
            assert got[kind]["result"] == want[kind]["result"], kind
        return
    mo = H.official_min_overlaps(case["class_ids"])
    rets = [KE.eval_class_v3(c["gt_annos"], c["dt_annos"], case["class_ids"], H.DIFFICULTYS, m, mo, case["compute_aos"], z_axis=case["z_axis"],
                             z_center=case["z_center"]) for m in range(3)]
    for j, cname in enumerate(case["classes"]):
        detail = want["official"]["detail"][cname]
        for i in range(2):
            for m, key in enumerate(("bbox", "bev", "3d")):
                assert np.array_equal(_map(rets[m]["precision"][j, :, i]), detail[f"{key}@{mo[i, m, j]:.2f}"], equal_nan=True), (cname, key, i)
        if case["compute_aos"]:
            assert np.allclose(_map(rets[0]["orientation"][j, :, 1]), detail["aos"], rtol=0, atol=1e-9, equal_nan=True)
    mo = H.coco_min_overlaps(case["class_ids"])
    for m, key in enumerate(("bbox", "bev", "3d")):
        ret = KE.eval_class_v3(c["gt_annos"], c["dt_annos"], case["class_ids"], H.DIFFICULTYS, m, mo, case["compute_aos"] and m == 0,
                               z_axis=case["z_axis"], z_center=case["z_center"])
        for j, cname in enumerate(case["classes"]):
            assert np.array_equal(_map(ret["precision"])[j].mean(-1), want["coco"]["detail"][cname][key], equal_nan=True), (cname, key)


# ------------------------------------------------------------------------------------------------------------ hand-built cases
def _against_restatement(KE, gts, dts, class_ids, mo, aos, label, metric=0, overlaps=None):
    blocks = H.bbox_overlaps(gts, dts) if overlaps is None else overlaps
    want = H.eval_np(gts, dts, blocks, class_ids, H.DIFFICULTYS, metric, mo, aos)
    got = _stages(KE, gts, dts, class_ids, metric, mo, aos, overlaps=None if overlaps is None else _flat(blocks))
    if overlaps is None:
        assert np.array_equal(got["overlaps"], _flat(blocks)), label
    _check(got, (want["ignored_gt"], want["ignored_dt"], want["num_valid_gt"]), want, label)
    return got, want


def test_bitmask_words_are_crossed(KE):
    """33 and 65 detections in one image: the assigned set of a lane spans two and three 32-bit words (pass 2), a lane owns a second
    detection (pass 1).  Equal scores, DontCare regions, all three classes."""
    rng = np.random.default_rng(33)
    gts, dts = H.random_annos(rng, 3, [20, 30, 4], [33, 65, 5], classes=("Car", "Pedestrian", "Cyclist"), dontcare=2, tie_scores=True)
    got, want = _against_restatement(KE, gts, dts, [0, 1, 2], H.official_min_overlaps([0, 1, 2]), True, "33 / 65 detections")
    assert want["pr"][..., 0].max() >= 5 and want["pr"][..., 1].max() >= 5


def test_a_single_true_positive(KE):
    rng = np.random.default_rng(1)
    gts, dts = H.random_annos(rng, 1, 1, 1, classes=("Car",))
    gts[0].update(name=np.array(["Car"], dtype="U16"), occluded=np.array([0]), truncated=np.array([0.0]), bbox=np.array([[100.0, 100.0, 180.0, 150.0]]))
    dts[0].update(bbox=np.array([[101.0, 100.0, 181.0, 151.0]]), score=np.array([0.625]))
    got, want = _against_restatement(KE, gts, dts, [0], H.official_min_overlaps([0]), True, "one tp")
    assert got["n_scores"].tolist() == [1] * 6 and got["n_thresholds"].tolist() == [1] * 6 and (got["counts"][:, 0] == [1, 0, 0]).all()
    assert (got["thresholds"][:, 0] == 0.625).all()


def test_more_than_64_configurations_and_more_images_than_one_chunk(KE):
    """3 classes x 3 difficulties x 10 overlaps = 90 configurations; 2 * CHUNK + 3 images: three chunks of partial sums, the last one short."""
    rng = np.random.default_rng(90)
    n = 2 * H.CHUNK + 3
    gts, dts = H.random_annos(rng, n, list(rng.integers(0, 15, n)), list(rng.integers(0, 21, n)), classes=("Car", "Pedestrian", "Cyclist"), dontcare=1)
    mo = H.coco_min_overlaps([0, 1, 2])
    got, want = _against_restatement(KE, gts, dts, [0, 1, 2], mo, True, "90 configurations, 67 images")
    assert got["counts"].shape == (90, 41, 3) and want["n_thresholds"].max() > 20
    # the same through random overlap blocks and metric 1 (no DontCare pass)
    blocks = [np.round(rng.random((len(d["name"]), len(g["name"]))), 3) * (rng.random((len(d["name"]), len(g["name"]))) < 0.3) for g, d in zip(gts, dts)]
    _against_restatement(KE, gts, dts, [0, 1, 2], mo, False, "90 configurations, random blocks", metric=1, overlaps=blocks)


def test_all_detections_ignored_by_threshold(KE):
    """Pass 2 with thresholds above every score: nothing is matched, nothing is a false positive, every valid gt is missed."""
    from second_amd import ops
    rng = np.random.default_rng(7)
    gts, dts = H.random_annos(rng, 4, 6, 9, classes=("Car",), dontcare=1, score_range=(0.05, 0.9))
    mo = H.official_min_overlaps([0])
    p = KE.pack(gts, dts)
    r = KE.run_stages(p, [0], H.DIFFICULTYS, 0, mo, True, 1, 1.0)
    t = {k: torch.from_numpy(v).cuda() for k, v in p.items() if isinstance(v, np.ndarray)}
    thr = torch.full((6, 41), 0.95, dtype=torch.float64, device="cuda")
    n_thr = torch.full((6,), 41, dtype=torch.int32, device="cuda")
    counts, sim = ops.kitti_eval_pr(t["gt_off"], t["dt_off"], t["dc_off"], t["ov_off"], r["overlaps"], t["dt_score"], t["gt_alpha"], t["dt_alpha"],
                                    t["dt_bbox"], t["dc_bbox"], r["ignored_gt"], r["ignored_dt"], p["max_gt"], p["max_dt"], r["cfg_min_overlap"], 2, thr,
                                    n_thr, 0, True)
    counts, nvg = counts.cpu().numpy(), r["num_valid_gt"].cpu().numpy()
    assert nvg.max() > 0 and not sim.any()
    assert (counts[..., 0] == 0).all() and (counts[..., 1] == 0).all() and np.array_equal(counts[..., 2], np.repeat(nvg, 2)[:, None].repeat(41, 1))


def test_an_image_at_the_cap_and_one_above(KE, monkeypatch):
    from second_amd import ops
    from second_amd.runtime import SecondHipError
    rng = np.random.default_rng(512)
    gts, dts = H.random_annos(rng, 2, [H.MAX_GT, 3], [H.MAX_DT, 4], classes=("Car",), tie_scores=True)
    mo = H.official_min_overlaps([0])
    got, want = _against_restatement(KE, gts, dts, [0], mo, True, "512 gt x 512 detections")
    assert want["pr"][..., 0].max() > 50
    gts, dts = H.random_annos(rng, 2, [5, 3], [H.MAX_DT + 1, 4], classes=("Car",))
    p = KE.pack(gts, dts)
    with pytest.raises(SecondHipError, match="SEC_E_UNSUPPORTED"):
        KE.run_stages(p, [0], H.DIFFICULTYS, 0, mo, False, 1, 1.0)
    t = {k: torch.from_numpy(v).cuda() for k, v in p.items() if isinstance(v, np.ndarray)}
    with pytest.raises(SecondHipError, match="SEC_E_UNSUPPORTED"):
        ops.kitti_eval_overlaps(0, t["dt_off"], t["gt_off"], t["ov_off"], t["dt_bbox"], t["gt_bbox"], int(p["ov_off"][-1]), p["max_dt"], p["max_gt"])
    monkeypatch.setattr(KE, "_reference_eval_class_v3", lambda: (lambda *a, **k: "reference result"))
    before = dict(KE.stats)
    assert KE.eval_class_v3(gts, dts, [0], H.DIFFICULTYS, 0, mo) == "reference result"
    assert KE.stats["fallback"] == before["fallback"] + 1 and KE.stats["device"] == before["device"]


def test_no_images(KE):
    mo = H.official_min_overlaps([0, 1])
    ret = KE.eval_class_v3([], [], [0, 1], H.DIFFICULTYS, 0, mo, True)
    assert ret["precision"].shape == (2, 3, 2, 41) and not ret["precision"].any() and not ret["orientation"].any() and not ret["thresholds"].any()
    got = _stages(KE, [], [], [0, 1], 2, mo)
    assert got["counts"].shape == (12, 41, 3) and not got["counts"].any() and not got["n_thresholds"].any() and not got["num_valid_gt"].any()
