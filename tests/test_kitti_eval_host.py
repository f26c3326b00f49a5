"""CPU-only: the KITTI evaluation's fixture, the numpy restatement of its four stages, the entry points and the compat switch.

tests/golden/kitti_eval.npz holds what the reference computes (tests/golden/make_golden_kitti_eval.py).  The restatement of
tests/kitti_eval_helpers.py -- which the GPU tests use for the hand-built cases -- must reproduce every recorded array: integers,
scores, thresholds and precision exactly, similarity sums within the float64 summation bound.  The sec_kitti_eval_* entry points exist
in header, library and runtime.SYMBOLS and refuse bad arguments before any launch."""
import ctypes
import sys
import types

import numpy as np
import pytest

import kitti_eval_helpers as H


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


@pytest.fixture(scope="module")
def cases(golden):
    return {name: H.load_case(golden, name) for name in H.CASES}


def test_fixture_holds_the_cases_the_matching_needs(golden, cases):
    a, b = cases["A"], cases["B"]
    gt_n, dt_n = [len(g["name"]) for g in a["gt_annos"]], [len(d["name"]) for d in a["dt_annos"]]
    assert len(gt_n) == 8 and len(b["gt_annos"]) == 5
    assert any(g == 0 and d > 0 for g, d in zip(gt_n, dt_n)) and any(g > 0 and d == 0 for g, d in zip(gt_n, dt_n))
    assert any(g == 0 and d == 0 for g, d in zip(gt_n, dt_n))
    names = np.concatenate([g["name"] for g in a["gt_annos"]])
    assert {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare"} <= set(names.tolist())
    assert any(len(set(d["score"].tolist())) < len(d["score"]) for d in a["dt_annos"])                 # equal scores within an image
    assert 70 in [len(d["name"]) for d in b["dt_annos"]] and all((d["alpha"] == -10).all() for d in b["dt_annos"])
    for name in H.CASES:                       # no overlap of metrics 1 / 2 within 1e-4 of a min_overlap in use
        in_use = np.unique(np.concatenate([H.min_overlaps_of(k, H.CASES[name]["class_ids"])[:, 1:].reshape(-1) for k in H.KINDS]))
        vals = np.concatenate([cases[name]["flat"][1], cases[name]["flat"][2]])
        dist = np.abs(vals[:, None] - in_use[None, :]).min()
        assert dist == float(golden[f"{name}_min_distance"]) and dist > 1e-4
        assert np.array_equal(cases[name]["flat"][2].astype(np.float32).astype(np.float64), cases[name]["flat"][2])
    n_thr = np.concatenate([golden[f"A_{k}_m{m}_n_thresholds"] for k in H.KINDS for m in range(3)])
    assert n_thr.max() == 41 and n_thr.min() < 5


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_metric0_overlaps_are_restated_bit_for_bit(cases, name):
    c = cases[name]
    mine = H.bbox_overlaps(c["gt_annos"], c["dt_annos"])
    for got, want in zip(mine, c["overlaps"][0]):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name,kind,metric", [(n, k, m) for n in sorted(H.CASES) for k in H.KINDS for m in range(3)])
def test_numpy_restatement_equals_the_reference(golden, cases, name, kind, metric):
    case, c = H.CASES[name], cases[name]
    rec = H.recorded(golden, name, kind, metric)
    counters = {}
    mine = H.eval_np(c["gt_annos"], c["dt_annos"], c["overlaps"][metric], case["class_ids"], H.DIFFICULTYS, metric,
                     H.min_overlaps_of(kind, case["class_ids"]), rec["compute_aos"], counters)
    assert np.array_equal(mine["ignored_gt"], golden[f"{name}_ignored_gt"]) and np.array_equal(mine["ignored_dt"], golden[f"{name}_ignored_dt"])
    assert np.array_equal(mine["num_valid_gt"], golden[f"{name}_num_valid_gt"])
    assert len(mine["scores"]) == len(rec["scores"]) and all(np.array_equal(a, b) for a, b in zip(mine["scores"], rec["scores"]))
    assert np.array_equal(mine["n_thresholds"], rec["n_thresholds"]) and np.array_equal(mine["thresholds"], rec["thresholds"])
    assert np.array_equal(mine["pr"][..., :3], rec["pr"][..., :3])
    assert (np.abs(mine["pr"][..., 3] - rec["pr"][..., 3]) <= H.similarity_bound(rec["pr"])).all()
    assert np.array_equal(mine["precision"], rec["precision"], equal_nan=True)
    scale = np.where(rec["pr"][..., 0] + rec["pr"][..., 1] > 0, rec["pr"][..., 0] + rec["pr"][..., 1], 1.0)
    tol = np.maximum.accumulate((H.similarity_bound(rec["pr"]) / scale)[:, ::-1], axis=1)[:, ::-1].reshape(rec["orientation"].shape) + 1e-300
    assert (np.abs(mine["orientation"] - rec["orientation"]) <= tol)[~np.isnan(rec["orientation"])].all()
    assert np.array_equal(np.isnan(mine["orientation"]), np.isnan(rec["orientation"]))
    if name == "A" and metric == 0:
        assert counters["nstuff"] > 0                                  # detections inside DontCare regions were discounted
    if name == "A" and metric > 0:
        assert counters["replaced_ignored_det"] > 0                    # the assigned_ignored_det branch was taken


def test_host_finish_of_the_product_equals_the_reference(golden):
    from second_amd import kitti_eval as KE
    for name, case in H.CASES.items():
        for kind in H.KINDS:
            for m in range(3):
                rec = H.recorded(golden, name, kind, m)
                shape = rec["precision"].shape[:3]
                precision, aos, thr = KE.finish(rec["pr"][..., :3].astype(np.int32), rec["pr"][..., 3], rec["thresholds"], rec["n_thresholds"], shape,
                                                rec["compute_aos"])
                assert np.array_equal(precision, rec["precision"], equal_nan=True) and np.array_equal(aos, rec["orientation"], equal_nan=True)
                assert np.array_equal(thr.reshape(-1, 41), rec["thresholds"])


def test_pack_encodes_names_not_class_indices(cases):
    from second_amd import kitti_eval as KE
    c = cases["A"]
    p = KE.pack(c["gt_annos"], c["dt_annos"])
    assert p["images"] == 8 and p["gt_off"].dtype == np.int32 and p["ov_off"][-1] == len(c["flat"][0])
    names = np.concatenate([g["name"] for g in c["gt_annos"]])
    assert (p["gt_name"][names == "Van"] == 3).all() and (p["gt_name"][names == "DontCare"] == KE.NAME_OTHER).all()
    assert len(p["dc_bbox"]) == int((names == "DontCare").sum()) == p["dc_off"][-1]
    assert KE.class_difficulty_pairs([5, 0], [0, 2]) == ([0, 0, 0, 0], [0, 2, 0, 2])                 # 'car' twice in the table: one name
    lower = [dict(g, name=np.char.lower(g["name"])) for g in c["gt_annos"]]
    assert len(KE.pack(lower, c["dt_annos"])["dc_bbox"]) == 0                                            # 'dontcare' is no DontCare row
    assert p["max_dt"] == max(len(d["name"]) for d in c["dt_annos"])
    empty = KE.pack([], [])
    assert empty["images"] == 0 and empty["gt_off"].tolist() == [0] and empty["gt_box3d"].shape == (0, 7)


def test_entry_points_exist_and_validate_before_any_launch():
    from second_amd import ops, runtime as rt
    from test_capi_symbols import header_functions
    new = ["sec_kitti_eval_overlaps", "sec_kitti_eval_flags", "sec_kitti_eval_tp_scores", "sec_kitti_eval_thresholds",
           "sec_kitti_eval_pr_workspace_bytes", "sec_kitti_eval_pr"]
    l = rt.lib()
    hdr = header_functions()
    for n in new:
        assert n in hdr and n in rt.SYMBOLS and hasattr(l, n), n
    assert l.sec_abi_version() == 9
    assert (ops.KITTI_EVAL_MAX_GT, ops.KITTI_EVAL_MAX_DT, ops.KITTI_EVAL_CHUNK) == (H.MAX_GT, H.MAX_DT, H.CHUNK)
    one = ctypes.c_void_p(4096)                      # never dereferenced: validation fails first
    # ---- overlaps
    ov = lambda metric, dt_boxes, max_dt, max_gt, out=one: l.sec_kitti_eval_overlaps(metric, 4, one, one, one, dt_boxes, one, 40, 30, 300, max_dt, max_gt,
                                                                                  1, 1.0, out, None)
    assert ov(0, None, 10, 10) == -1 and ov(0, one, 10, 10, None) == -1 and ov(3, one, 10, 10) == -1
    assert ov(1, one, H.MAX_DT + 1, 10) == -3 and ov(2, one, 10, H.MAX_GT + 1) == -3
    assert l.sec_kitti_eval_overlaps(0, 4, None, one, one, one, one, 40, 30, 300, 10, 10, 1, 1.0, one, None) == -1
    assert l.sec_kitti_eval_overlaps(1, 4, one, one, one, one, one, 40, 30, 300, 10, 10, 3, 1.0, one, None) == -1          # z_axis
    # ---- flags
    i2 = (ctypes.c_int * 2)(0, 1)
    fl = lambda names, ncd, nvg: l.sec_kitti_eval_flags(names, i2, ncd, 30, 40, one, one, one, one, one, one, one, one, nvg, None)
    assert fl(None, 2, one) == -1 and fl(i2, 2, None) == -1 and fl(i2, 0, one) == -1
    assert fl((ctypes.c_int * 2)(0, 9), 2, one) == -1                                                  # no such name id
    assert l.sec_kitti_eval_flags((ctypes.c_int * 40)(), (ctypes.c_int * 40)(), 40, 30, 40, one, one, one, one, one, one, one, one, one, None) == -3
    # ---- tp scores
    tp = lambda max_gt, max_dt, mo=one, configs=6: l.sec_kitti_eval_tp_scores(4, one, one, one, one, 300, one, one, one, 30, 40, max_gt, max_dt, mo, 2,
                                                                               configs, one, one, None)
    assert tp(10, 10, None) == -1 and tp(10, 10, one, 5) == -1                                          # configs is a multiple of num_k
    assert tp(H.MAX_GT + 1, 10) == -3 and tp(10, H.MAX_DT + 1) == -3
    # ---- thresholds
    assert l.sec_kitti_eval_thresholds(one, 30, None, one, 2, 6, one, one, None) == -1
    assert l.sec_kitti_eval_thresholds(None, 30, one, one, 2, 6, one, one, None) == -1
    # ---- pr
    need = l.sec_kitti_eval_pr_workspace_bytes(4, 6)
    assert need >= 6 * 41 * (3 * 4 + 8) and l.sec_kitti_eval_pr_workspace_bytes(4, 0) == 0
    assert l.sec_kitti_eval_pr_workspace_bytes(H.CHUNK + 1, 6) > need                                   # a second chunk of partial sums
    pr = lambda max_gt, max_dt, ws, nbytes, counts=one, aos=0, galpha=one: l.sec_kitti_eval_pr(
        4, one, one, one, one, one, 300, one, galpha, one, one, one, 3, one, one, 30, 40, max_gt, max_dt, one, 2, 6, one, one, 0, aos, counts, one,
        ws, nbytes, None)
    assert pr(10, 10, one, need, None) == -1 and pr(10, 10, one, need, one, 1, None) == -1              # no output / aos without alphas
    assert pr(10, 10, one, need - 1) == -2 and pr(10, 10, None, need) == -2                             # short / no workspace
    assert pr(H.MAX_GT + 1, 10, one, need) == -3 and pr(10, H.MAX_DT + 1, one, need) == -3              # over a cap


def _fake_eval_module(monkeypatch):
    """A stand-in ``second.utils.eval`` with the names accelerate_eval touches, and do_eval_v3 resolving eval_class_v3 at call time."""
    ev = types.ModuleType("second.utils.eval")
    exec("def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):\n    return 'original iou'\n"
         "def eval_class_v3(*a, **k):\n    return 'original statistics'\n"
         "def do_eval_v3(*a, **k):\n    return eval_class_v3(*a, **k)\n", ev.__dict__)
    second, utils = types.ModuleType("second"), types.ModuleType("second.utils")
    second.utils, utils.eval = utils, ev
    for k, v in (("second", second), ("second.utils", utils), ("second.utils.eval", ev)):
        monkeypatch.setitem(sys.modules, k, v)
    return ev


@pytest.fixture
def keep_linspace():
    saved = np.linspace
    yield
    np.linspace = saved


def test_accelerate_eval_without_statistics_is_todays_behaviour(monkeypatch, keep_linspace):
    from second_amd import compat
    monkeypatch.delenv("SEC_EVAL_DEVICE", raising=False)
    ev = _fake_eval_module(monkeypatch)
    original = ev.eval_class_v3
    assert compat.accelerate_eval() is ev
    assert ev.eval_class_v3 is original and not hasattr(ev, "_second_amd_original_eval_class_v3")
    assert ev.rotate_iou_gpu_eval is compat.rotate_iou_gpu_eval and ev._second_amd_original_rotate_iou(None, None) == "original iou"
    for value in ("0", "true", "yes", ""):                            # only "1" turns the statistics on
        monkeypatch.setenv("SEC_EVAL_DEVICE", value)
        compat.accelerate_eval()
        assert ev.eval_class_v3 is original
    compat.accelerate_eval(statistics=False)
    assert ev.eval_class_v3 is original and ev.do_eval_v3() == "original statistics"


def test_accelerate_eval_statistics_installs_the_replacement(monkeypatch, keep_linspace):
    from second_amd import compat, kitti_eval as KE
    monkeypatch.delenv("SEC_EVAL_DEVICE", raising=False)
    ev = _fake_eval_module(monkeypatch)
    original = ev.eval_class_v3
    compat.accelerate_eval(statistics=True)
    assert ev.eval_class_v3 is KE.eval_class_v3 and ev._second_amd_original_eval_class_v3 is original
    assert ev.do_eval_v3.__globals__["eval_class_v3"] is KE.eval_class_v3                               # the seam do_eval_v2 / v3 call through
    assert ev.rotate_iou_gpu_eval is compat.rotate_iou_gpu_eval
    compat.accelerate_eval(statistics=True)                                                             # idempotent
    assert ev._second_amd_original_eval_class_v3 is original and KE._reference_eval_class_v3() is original
    assert np.array_equal(np.linspace(*np.array([0.5, 0.95, 10])), np.linspace(0.5, 0.95, 10))          # what do_coco_style_eval calls
    # the environment switch, as launch.run_evaluate reaches it
    ev2 = _fake_eval_module(monkeypatch)
    monkeypatch.setenv("SEC_EVAL_DEVICE", "1")
    compat.accelerate_eval()
    assert ev2.eval_class_v3 is KE.eval_class_v3


def test_eval_class_v3_falls_back_above_a_cap(monkeypatch):
    """An image with more detections than the device form takes: the reference's function serves the call and stats counts it (no GPU,
    no launch: the decision is the host's)."""
    from second_amd import kitti_eval as KE
    rng = np.random.default_rng(5)
    gts, dts = H.random_annos(rng, 2, 3, [4, H.MAX_DT + 1])
    seen = {}

    def reference(*a, **k):
        seen["args"], seen["kwargs"] = a, k
        return "reference result"
    monkeypatch.setattr(KE, "_reference_eval_class_v3", lambda: reference)
    before = dict(KE.stats)
    mo = H.official_min_overlaps([0])
    assert KE.eval_class_v3(gts, dts, [0], [0, 1, 2], 0, mo, True, z_axis=1, z_center=1.0) == "reference result"
    assert KE.stats["fallback"] == before["fallback"] + 1 and KE.stats["device"] == before["device"]
    assert seen["args"][4] == 0 and seen["args"][6] is True and seen["kwargs"] == dict(z_axis=1, z_center=1.0, num_parts=50)
