"""CPU-only: the KITTI-annotation fixture, the float64 restatement of the conversion, the dict builder, the entry points, the compat
switch, the fallbacks and the unchanged plain route of kitti_eval.pack.

tests/golden/kitti_annos.npz holds what the reference's ``KittiDataset.convert_detection_to_kitti_annos`` returns
(tests/golden/make_golden_kitti_annos.py).  tests/kitti_annos_helpers.py's restatement -- which the GPU tests use for the hand-built
cases -- must reproduce it: the kept set, order, scores, names, dimensions and rotation_y exactly, location / bbox / alpha within the
derived bounds of the helper."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import kitti_annos_helpers as H
import kitti_eval_helpers as EH

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def fx():
    return H.load_fixture()


@pytest.fixture(scope="module")
def restated(fx):
    r = H.restate(fx["boxes"], fx["det_off"], fx["lidar2cam"], fx["P2"], fx["image_shape"])
    return r, H.compact(r, fx["scores"], fx["labels"], fx["det_off"])


def recorded_flat(fx, key):
    parts = [a[key] for a in fx["annos"] if len(a["name"])]
    return np.concatenate(parts, 0)


def test_fixture_holds_the_cases_the_conversion_needs(fx, restated):
    r, _ = restated
    counts, kept = np.diff(fx["det_off"]), np.diff(fx["out_off"])
    assert len(counts) == 40 and counts.max() == 60 and counts.min() == 0 and 100 < fx["boxes"].nbytes < 200_000
    assert counts[0] == 0 and counts[-1] == 0 and (counts[17:20] == 0).all()                       # none at the start, in a run, at the end
    assert any(c > 0 and k == 0 for c, k in zip(counts, kept)), "a frame where everything is dropped"
    assert len(fx["class_names"]) == 3 and len({tuple(s) for s in fx["image_shape"].tolist()}) == 2
    assert (fx["P2"][:, :3, 3] != 0).all(), "a fourth column of P2 the projection must ignore"
    x = fx["boxes"][:, 0]
    assert x.min() < 0 and x.max() > 70
    raw = r["raw_bbox"]
    assert ((raw[:, 0] < 0) & (raw[:, 2] > r["hw"][:, 1])).any(), "a box across the image plane spans more than the image"
    assert 0 < r["keep"].sum() < len(x)
    ratio, dist = H.decision_margins(r)
    assert ratio.min() == float(fx["min_margin"]) >= H.MARGIN and dist.min() == float(fx["min_distance"])


def test_restatement_reproduces_the_reference(fx, restated):
    r, mine = restated
    assert np.array_equal(mine["out_off"], fx["out_off"])                                          # the kept set per image, exactly
    assert np.array_equal(mine["score"], recorded_flat(fx, "score")) and mine["score"].dtype == np.float32
    assert np.array_equal(np.array(fx["class_names"])[mine["label"]], recorded_flat(fx, "name"))
    assert np.array_equal(mine["box3d"][:, 3:6], recorded_flat(fx, "dimensions")) and np.array_equal(mine["box3d"][:, 6], recorded_flat(fx, "rotation_y"))
    assert np.array_equal(mine["src"], np.flatnonzero(r["keep"]))
    for key, got, bound in (("bbox", mine["bbox"], mine["bbox_err"]), ("location", mine["box3d"][:, :3], mine["location_err"]),
                            ("alpha", mine["alpha"], mine["alpha_err"])):
        ok, share = H.within(got, recorded_flat(fx, key), bound)
        print(f"{key}: largest share of the bound used {share:.3g} (largest bound {np.max(bound):.3g})")
        assert ok, key
    assert np.isfinite(mine["bbox_err"]).all() and mine["bbox_err"].max() < 1e-6                   # the bounds bind: far under a pixel


def test_restatement_quirks_by_hand():
    """Identity calibration, power-of-two numbers: the values are exact and can be written down."""
    eye = np.eye(4)[None]
    P = np.array([[[2.0, 0, 0, 1000.0], [0, 2.0, 0, 1000.0], [0, 0, 1.0, 1000.0], [0, 0, 0, 1.0]]])  # a fourth column that must not matter
    hw = np.array([[64, 128]], np.int32)
    # lidar box at (x, y, z) = (4, 2, 8), w = l = h = 2, r = 0: z' = 7, corners x in {3, 5}, y in {0, 2}, z in {6, 8}
    box = np.array([[4, 2, 8, 2, 2, 2, 0]], np.float32)
    r = H.restate(box, [0, 1], eye, P, hw)
    assert r["location"].tolist() == [[4.0, 2.0, 7.0]] and r["dimensions"].tolist() == [[2.0, 2.0, 2.0]]
    assert r["raw_bbox"].tolist() == [[2 * 3 / 8, 0.0, 2 * 5 / 6, 2 * 2 / 6]] and r["keep"].tolist() == [True]
    assert r["alpha"][0] == -float(np.float32(np.arctan2(-2.0, 4.0))) + 0.0
    # a NaN propagates through min / max and the clamps, and the row is kept
    box[0, 2], box[0, 5] = 1.0, 2.0                                # z' = 0: the corners with pz = -1 ... loc z = 0, w = 2: z in {-1, 1}
    box[0, 0], box[0, 4] = 1.0, 2.0                                # x in {0, 2}
    box[0, 1] = 0.0                                                # y in {-2, 0}
    box[0, 3] = 0.0                                                # w = 0: all corners at z = 0; the corner (0, 0, 0) gives 0 / 0
    r = H.restate(box, [0, 1], eye, P, hw)
    assert np.isnan(r["raw_bbox"]).all() and np.isnan(r["bbox"]).all() and r["keep"].tolist() == [True]
    assert np.isinf(r["bbox_err"]).all()


def test_annos_from_packed_reproduces_the_recorded_dicts(fx, restated):
    from second_amd import kitti_annos as KA
    n = int(fx["out_off"][-1])
    src = restated[1]["src"]
    pad = lambda a: np.concatenate([a, np.full((7,) + a.shape[1:], 99, a.dtype)])                 # rows behind n are ignored
    packed = dict(bbox=pad(recorded_flat(fx, "bbox")), alpha=pad(recorded_flat(fx, "alpha")), score=pad(recorded_flat(fx, "score")),
                  box3d=pad(np.concatenate([recorded_flat(fx, "location"), recorded_flat(fx, "dimensions"), recorded_flat(fx, "rotation_y")[:, None]], 1)),
                  label=pad(fx["labels"][src].astype(np.int32)), out_off=fx["out_off"])
    metadata = [a["metadata"] for a in fx["annos"]]
    annos, names = KA.annos_from_packed(packed, fx["class_names"], metadata)
    assert len(annos) == len(fx["annos"]) == len(names) and sum(len(a["name"]) for a in annos) == n
    empties = 0
    for i, (got, want, lay) in enumerate(zip(annos, fx["annos"], fx["layout"])):
        assert list(got) == H.ANNO_KEYS + ["metadata"] and got["metadata"] is metadata[i] and got["name"] is names[i]
        for k in H.ANNO_KEYS:
            dtype, shape = np.dtype(lay[k][0]), tuple(lay[k][1])
            assert got[k].shape == shape, (i, k)
            assert got[k].dtype == dtype or (dtype.kind == "U" and got[k].dtype.kind == "U"), (i, k, got[k].dtype, dtype)
            assert np.array_equal(got[k], want[k]), (i, k)
        if not len(want["name"]):
            empties += 1
            assert got["name"].dtype == np.float64 and got["score"].dtype == np.float64 and got["bbox"].shape == (0, 4)
        else:
            assert got["truncated"].dtype == np.float64 and not got["truncated"].any() and got["occluded"].dtype == np.int64 and not got["occluded"].any()
            assert got["score"].dtype == np.float32
    assert empties == 9


def test_label_out_of_range_raises_index_error(fx):
    from second_amd import kitti_annos as KA
    packed = dict(bbox=np.zeros((2, 4)), alpha=np.zeros(2), box3d=np.zeros((2, 7)), score=np.zeros(2, np.float32), label=np.array([1, 3], np.int32),
                  out_off=np.array([0, 2], np.int32))
    with pytest.raises(IndexError):
        KA.annos_from_packed(packed, ["Car", "Pedestrian", "Cyclist"], [{}])
    packed["label"] = np.array([1, -1], np.int32)                   # Python list indexing: -1 is the last class, in the reference too
    annos, _ = KA.annos_from_packed(packed, ["Car", "Pedestrian", "Cyclist"], [{}])
    assert annos[0]["name"].tolist() == ["Pedestrian", "Cyclist"]
    packed["out_off"] = np.array([0, 1], np.int32)                  # a label behind n is never looked at
    packed["label"] = np.array([1, 7], np.int32)
    assert KA.annos_from_packed(packed, ["Car", "Pedestrian", "Cyclist"], [{}])[0][0]["name"].tolist() == ["Pedestrian"]


def test_entry_points_exist_and_validate_before_any_launch():
    from second_amd import ops, runtime as rt
    from test_capi_symbols import header_functions
    l = rt.lib()
    hdr = header_functions()
    for n in ("sec_kitti_annos_workspace_bytes", "sec_kitti_annos_f64"):
        assert n in hdr and n in rt.SYMBOLS and hasattr(l, n), n
    assert l.sec_abi_version() == 9
    need = l.sec_kitti_annos_workspace_bytes(1000)
    assert need >= 1000 * (12 * 8 + 1) + 4 * 4 and l.sec_kitti_annos_workspace_bytes(-1) == 0
    assert l.sec_kitti_annos_workspace_bytes(0) > 0 and l.sec_kitti_annos_workspace_bytes(65537) > l.sec_kitti_annos_workspace_bytes(65536)
    one = ctypes.c_void_p(4096)                      # never dereferenced: validation fails first
    good = [one, one, one, 1000, one, 40, one, one, one, one, one, one, one, one, one, one, one, need, None]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return l.sec_kitti_annos_f64(*a)
    for pos in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert call(**{f"a{pos}": None}) == -1, pos                                                # a NULL array
    assert call(a3=-1) == -1 and call(a5=-1) == -1                                                 # negative counts
    assert call(a17=need - 1) == -2 and call(a16=None) == -2                                       # short / no workspace
    lay = ops.kitti_annos_layout(1000, 40)
    assert lay["bbox"] == (0, "float64", (1000, 4)) and lay["out_off"][2] == (41,) and all(v[0] % 256 == 0 for k, v in lay.items() if k != "bytes")
    host = ops.kitti_annos_views(np.zeros(lay["bytes"], np.uint8), 1000, 40)
    assert host["box3d"].shape == (1000, 7) and host["score"].dtype == np.float32 and host["src"].dtype == np.int32
    assert ops.kitti_annos_views(np.zeros(ops.kitti_annos_layout(0, 0)["bytes"], np.uint8), 0, 0)["out_off"].shape == (1,)


def _cpu_detections(fx, dtype=torch.float32):
    off = fx["det_off"]
    return [{"box3d_lidar": torch.from_numpy(fx["boxes"][off[i]:off[i + 1]].copy()).to(dtype), "scores": torch.from_numpy(fx["scores"][off[i]:off[i + 1]].copy()),
             "label_preds": torch.from_numpy(fx["labels"][off[i]:off[i + 1]].copy()), "metadata": {"image_idx": int(fx["image_idx"][i])}}
            for i in range(len(off) - 1)]


class _Recording(H.StandinDataset):
    def _second_amd_original_convert_detection_to_kitti_annos(self, detection):
        self.seen = detection
        return "the reference's own result"


def test_calls_outside_the_contract_reach_the_original_and_are_counted(fx):
    """float16 boxes, a 3 x 4 P2, infos without calib, detections on the CPU: the decision is the host's, nothing is launched."""
    from second_amd import kitti_annos as KA
    infos = H.fixture_infos(fx)
    cases = []
    cases.append(("boxes not float32", _Recording(infos, fx["class_names"]), _cpu_detections(fx, torch.float16)))
    narrow = [dict(i, calib=dict(i["calib"], P2=i["calib"]["P2"][:3])) for i in infos]
    cases.append(("calibration", _Recording(narrow, fx["class_names"]), _cpu_detections(fx)))
    cases.append(("calibration", _Recording([{"image": i["image"]} for i in infos], fx["class_names"]), _cpu_detections(fx)))
    cases.append(("calibration", _Recording([{"calib": i["calib"], "image": {"image_idx": 0}} for i in infos], fx["class_names"]), _cpu_detections(fx)))
    cases.append(("on the CPU", _Recording(infos, fx["class_names"]), _cpu_detections(fx)))
    six = _cpu_detections(fx)
    six[3]["box3d_lidar"] = six[3]["box3d_lidar"][:, :6]
    cases.append(("boxes not float32", _Recording(infos, fx["class_names"]), six))
    cases.append(("no frames", _Recording(infos, fx["class_names"]), []))
    for reason, ds, det in cases:
        before = dict(KA.stats)
        boxes_before = [d["box3d_lidar"].clone() for d in det]
        assert KA.convert_detection_to_kitti_annos(ds, det) == "the reference's own result" and ds.seen is det
        assert KA.stats["fallback"] == before["fallback"] + 1 and KA.stats["device"] == before["device"]
        assert reason in KA.last_fallback_reason, (reason, KA.last_fallback_reason)
        assert all(torch.equal(a, d["box3d_lidar"]) for a, d in zip(boxes_before, det))


def test_device_anno_list_handoff_rule():
    from second_amd import kitti_annos as KA
    names = [np.array(["Car"]), np.array([])]
    annos = [{"name": names[0]}, {"name": names[1]}]
    held = {"dt_num": np.array([1, 0])}
    l = KA.DeviceAnnoList(annos, names, held)
    assert l.handoff() is held and isinstance(l, list) and len(l) == 2
    assert type(pickle.loads(pickle.dumps(l))) is list
    assert KA.DeviceAnnoList(annos).handoff() is None
    l[0] = dict(l[0], name=np.array(["Car"]))                       # an equal array, another object
    assert l.handoff() is None
    l[0] = annos[0]
    assert l.handoff() is held
    l.append({"name": np.array([])})
    assert l.handoff() is None
    assert not hasattr([], "handoff")


@pytest.fixture
def kitti_dataset_class():
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    import importlib
    from second_amd import compat, kitti_annos as KA
    compat.install(REF)
    cls = importlib.import_module("second.data.kitti_dataset").KittiDataset
    assert not hasattr(cls, KA.ORIGINAL)
    original = cls.convert_detection_to_kitti_annos
    saved_linspace = np.linspace
    yield cls
    cls.convert_detection_to_kitti_annos = original
    if hasattr(cls, KA.ORIGINAL):
        delattr(cls, KA.ORIGINAL)
    np.linspace = saved_linspace


def test_accelerate_eval_annos_switch(monkeypatch, kitti_dataset_class, fx):
    from second_amd import compat, kitti_annos as KA
    cls = kitti_dataset_class
    original = cls.convert_detection_to_kitti_annos
    monkeypatch.delenv("SEC_EVAL_ANNOS", raising=False)
    monkeypatch.delenv("SEC_EVAL_DEVICE", raising=False)
    compat.accelerate_eval()
    assert cls.convert_detection_to_kitti_annos is original and not hasattr(cls, KA.ORIGINAL)
    for value in ("0", "true", ""):                                   # only "1" turns it on
        monkeypatch.setenv("SEC_EVAL_ANNOS", value)
        compat.accelerate_eval()
        assert cls.convert_detection_to_kitti_annos is original
    monkeypatch.setenv("SEC_EVAL_DEVICE", "1")                        # keeps its meaning: the statistics, not the annotations
    monkeypatch.delenv("SEC_EVAL_ANNOS")
    compat.accelerate_eval(annos=False)
    assert cls.convert_detection_to_kitti_annos is original
    compat.accelerate_eval(annos=True)
    assert cls.convert_detection_to_kitti_annos is KA.convert_detection_to_kitti_annos and getattr(cls, KA.ORIGINAL) is original
    compat.accelerate_eval(annos=True)                                # idempotent
    assert getattr(cls, KA.ORIGINAL) is original
    # an instance reaches the replacement, and through it -- CPU tensors are outside the contract -- the reference's own method
    ds = cls.__new__(cls)
    ds._kitti_infos, ds._class_names = H.fixture_infos(fx), fx["class_names"]
    before = dict(KA.stats)
    annos = ds.convert_detection_to_kitti_annos(_cpu_detections(fx))
    assert KA.stats["fallback"] == before["fallback"] + 1 and type(annos) is list
    assert np.array_equal(np.array([len(a["name"]) for a in annos]), np.diff(fx["out_off"]))
    for got, want in zip(annos, fx["annos"]):
        assert all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in H.ANNO_KEYS if k != "name")


def test_annos_environment_switch(monkeypatch, kitti_dataset_class):
    from second_amd import compat, kitti_annos as KA
    monkeypatch.setenv("SEC_EVAL_ANNOS", "1")
    monkeypatch.delenv("SEC_EVAL_DEVICE", raising=False)
    compat.accelerate_eval()
    assert kitti_dataset_class.convert_detection_to_kitti_annos is KA.convert_detection_to_kitti_annos


def _pack_as_before(gt_annos, dt_annos):
    """kitti_eval.pack as it stood before the hand-off was added, restated on plain numpy: what a plain list must still give."""
    ids = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3, 'person_sitting': 4, 'tractor': 5, 'trailer': 6}
    name_ids = lambda names: np.array([ids.get(str(n).lower(), 7) for n in names], np.int32)

    def cat(annos, key, cols=None):
        parts = [np.asarray(a[key], dtype=np.float64).reshape((-1,) if cols is None else (-1, cols)) for a in annos]
        return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0,) if cols is None else (0, cols)))

    def offsets(counts):
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    gt_num = np.array([len(a["name"]) for a in gt_annos], np.int64)
    dt_num = np.array([len(a["name"]) for a in dt_annos], np.int64)
    gt_names = [n for a in gt_annos for n in a["name"]]
    p = {"images": len(gt_annos), "gt_off": offsets(gt_num), "dt_off": offsets(dt_num), "ov_off": offsets(gt_num * dt_num),
         "max_gt": int(gt_num.max(initial=0)), "max_dt": int(dt_num.max(initial=0)),
         "gt_name": name_ids(gt_names), "dt_name": name_ids([n for a in dt_annos for n in a["name"]]),
         "gt_bbox": cat(gt_annos, "bbox", 4), "dt_bbox": cat(dt_annos, "bbox", 4), "gt_alpha": cat(gt_annos, "alpha"), "dt_alpha": cat(dt_annos, "alpha"),
         "dt_score": cat(dt_annos, "score"), "gt_occluded": cat(gt_annos, "occluded"), "gt_truncated": cat(gt_annos, "truncated")}
    for side, annos in (("gt", gt_annos), ("dt", dt_annos)):
        p[side + "_box3d"] = np.ascontiguousarray(np.concatenate([cat(annos, "location", 3), cat(annos, "dimensions", 3), cat(annos, "rotation_y")[:, None]], 1))
    dontcare = np.array([n == "DontCare" for n in gt_names], bool)
    p["dc_bbox"] = np.ascontiguousarray(p["gt_bbox"][dontcare])
    p["dc_off"] = offsets(np.array([int(dontcare[a:b].sum()) for a, b in zip(p["gt_off"][:-1], p["gt_off"][1:])], np.int64))
    return p


def test_pack_of_a_plain_list_is_unchanged(fx):
    from second_amd import kitti_eval as KE
    golden = np.load(EH.GOLDEN)
    pairs = [(c["gt_annos"], c["dt_annos"]) for c in (EH.load_case(golden, n) for n in EH.CASES)]
    pairs.append(EH.random_annos(np.random.default_rng(3), 6, [0, 3, 5, 0, 2, 9], [4, 0, 7, 0, 1, 30], classes=("Car", "Cyclist"), dontcare=1))
    gts, _ = EH.random_annos(np.random.default_rng(4), len(fx["annos"]), 4, 1, classes=("Car", "Pedestrian", "Cyclist"), dontcare=1)
    pairs.append((gts, fx["annos"]))                                  # the dicts the reference's conversion returns, empty images included
    pairs.append(([], []))
    for gt, dt in pairs:
        got, want = KE.pack(gt, dt), _pack_as_before(gt, dt)
        assert list(got) == list(want)
        for k in want:
            if isinstance(want[k], np.ndarray):
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
                assert got[k].flags["C_CONTIGUOUS"]
            else:
                assert type(got[k]) is type(want[k]) and got[k] == want[k], k
