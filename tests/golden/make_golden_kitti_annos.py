"""Produces tests/golden/kitti_annos.npz by EXECUTING the reference's ``KittiDataset.convert_detection_to_kitti_annos``
(second/data/kitti_dataset.py:38-107) on CPU tensors.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_kitti_annos.py [path to the reference checkout]

The method runs unbound on a stand-in object carrying the two attributes it reads (``_kitti_infos``, ``_class_names``).  The import
of second.data.kitti_dataset happens under make_golden.install_shims plus three things the module chain asks for and never uses here:
``np.bool`` (removed from numpy) and empty stub modules for skimage / skimage.io / fire.  Nothing the method computes is touched.
The reference lowers ``box3d_lidar[:, 2]`` in place on the array ``.cpu().numpy()`` returns -- for CPU tensors the caller's own
memory -- so every frame is handed over as a clone and the fixture records the inputs as they were BEFORE the call (checked below).

Contents: 40 images with 0-60 detections (none at the start, in the middle and at the end; one frame where every detection is
dropped; one image of another size), three class names, boxes with x in -5 .. 75 m so that some lie beside, behind and across the
image plane.  The case is reseeded until every compared value of the drop rule is at least 1e3 error bounds of
tests/kitti_annos_helpers.py from its threshold; the smallest margin and distance are recorded.  The helper's restatement is checked
against the executed reference here as well."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
IMAGES = 40
CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]


def make_case(H, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 61, IMAGES)
    counts[[0, 1, 17, 18, 19, 30, IMAGES - 1]] = 0                  # no detections at the start, in runs in the middle, at the end
    counts[5], counts[9] = 60, 1
    rect, trv2c, p2, shape = H.synthetic_calibration(rng, IMAGES, other_size_at=7)
    frames = []
    for i, c in enumerate(counts):
        b = H.random_boxes(rng, int(c))
        if i == 12:                                                 # everything far to the left of the image: all dropped
            b[:, 0], b[:, 1] = rng.uniform(3, 8, c), rng.uniform(40, 60, c)
        frames.append(b)
    boxes = np.concatenate(frames, 0).astype(np.float32)
    n = len(boxes)
    scores = rng.uniform(0.05, 1.0, n).astype(np.float32)
    labels = rng.integers(0, len(CLASS_NAMES), n).astype(np.int64)
    det_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    image_idx = (np.arange(IMAGES) * 3 + 7).astype(np.int64)
    return dict(boxes=boxes, scores=scores, labels=labels, det_off=det_off, rect=rect, trv2c=trv2c, P2=p2, image_shape=shape, image_idx=image_idx)


def main():
    if len(sys.argv) > 1:
        os.environ["SECOND_REFERENCE"] = sys.argv[1]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden
    make_golden.install_shims()
    if not hasattr(np, "bool"):
        np.bool = bool
    for name in ("skimage", "skimage.io", "fire"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    import torch
    import kitti_annos_helpers as H
    from second.data.kitti_dataset import KittiDataset

    seed = 300
    while True:
        case = make_case(H, seed)
        r = H.restate(case["boxes"], case["det_off"], np.stack([a @ b for a, b in zip(case["rect"], case["trv2c"])]), case["P2"],
                      case["image_shape"])
        ratio, dist = H.decision_margins(r)
        print("seed", seed, "detections", len(case["boxes"]), "kept by the restatement", int(r["keep"].sum()), "smallest margin", ratio.min(),
              "bounds, smallest distance", dist.min(), "px")
        if ratio.min() >= H.MARGIN:
            break
        seed += 1

    f = dict(case, class_names=CLASS_NAMES)
    standin = H.StandinDataset(H.fixture_infos(f), CLASS_NAMES)
    off = case["det_off"]
    detections = [{"box3d_lidar": torch.from_numpy(case["boxes"][off[i]:off[i + 1]].copy()), "scores": torch.from_numpy(case["scores"][off[i]:off[i + 1]].copy()),
                   "label_preds": torch.from_numpy(case["labels"][off[i]:off[i + 1]].copy()), "metadata": {"image_idx": int(case["image_idx"][i])}}
                  for i in range(IMAGES)]
    annos = KittiDataset.convert_detection_to_kitti_annos(standin, detections)
    assert len(annos) == IMAGES
    # the quirk the device form does not repeat: the caller's boxes were edited (z lowered by h / 2)
    edited = np.concatenate([d["box3d_lidar"].numpy() for d in detections])
    assert np.array_equal(edited[:, 2], (case["boxes"][:, 2] - case["boxes"][:, 5] / np.float32(2)).astype(np.float32)) and len(edited)
    assert not np.array_equal(edited[:, 2], case["boxes"][:, 2])

    out = {k: v for k, v in case.items()}
    out["class_names"] = np.array(CLASS_NAMES, dtype="U16")
    out["seed"], out["min_margin"], out["min_distance"] = np.int64(seed), np.float64(ratio.min()), np.float64(dist.min())
    num = np.array([len(a["name"]) for a in annos], np.int32)
    out["anno_num"] = num
    layout = []
    for a, d in zip(annos, detections):
        assert a["metadata"] is d["metadata"] and sorted(a) == sorted(H.ANNO_KEYS + ["metadata"])
        layout.append({k: [a[k].dtype.str, list(a[k].shape)] for k in H.ANNO_KEYS})
    out["layout"] = np.array(json.dumps(layout))
    for k in H.ANNO_KEYS:
        parts = [a[k] for a in annos if len(a["name"])]
        out["anno_" + k] = np.concatenate(parts, 0) if k != "name" else np.array([x for p in parts for x in p], dtype="U16")
    assert out["anno_score"].dtype == np.float32 and out["anno_bbox"].dtype == np.float64 and out["anno_occluded"].dtype == np.int64

    # the restatement against what was just recorded: decisions exact, values within the bounds
    mine = H.compact(r, case["scores"], case["labels"], case["det_off"])
    assert np.array_equal(mine["out_off"], np.concatenate([[0], np.cumsum(num)])), "kept set"
    assert np.array_equal(mine["score"], out["anno_score"]) and np.array_equal(np.array(CLASS_NAMES)[mine["label"]], out["anno_name"])
    assert np.array_equal(mine["box3d"][:, 3:6], out["anno_dimensions"]) and np.array_equal(mine["box3d"][:, 6], out["anno_rotation_y"])
    for key, got, bound in (("bbox", mine["bbox"], mine["bbox_err"]), ("location", mine["box3d"][:, :3], mine["location_err"]),
                            ("alpha", mine["alpha"], mine["alpha_err"])):
        ok, share = H.within(got, out["anno_" + key], bound)
        print(key, "largest difference", np.nanmax(np.abs(got - out["anno_" + key])), "largest share of the bound", share)
        assert ok, key
    assert num[12] == 0 and case["det_off"][13] - case["det_off"][12] > 0, "the frame where everything is dropped"
    raw = r["raw_bbox"]
    corners_behind = int(((raw[:, 0] < 0) & (raw[:, 2] > r["hw"][:, 1])).sum())
    print("kept", int(num.sum()), "of", len(case["boxes"]), "| images without a kept row", int((num == 0).sum()), "| boxes spanning the whole width",
          corners_behind, "| behind the camera (x < 0)", int((case["boxes"][:, 0] < 0).sum()))
    path = os.path.join(HERE, "kitti_annos.npz")
    H.save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
