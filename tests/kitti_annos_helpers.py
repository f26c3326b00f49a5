"""Host side of the KITTI-annotation tests: the fixture's layout, a float64 restatement of the conversion and its error bound.

tests/golden/kitti_annos.npz is recorded by executing ``KittiDataset.convert_detection_to_kitti_annos`` of the reference
(tests/golden/make_golden_kitti_annos.py).  :func:`restate` is this project's own text of steps 1-8 of DESIGN.md section 9e: every
product, sum and quotient written out as one elementwise IEEE float64 operation (no ``@``, no ``einsum``: those do not fix a summation
order), vectorised over the detections only.  It also evaluates the first-order forward error bound the tests hold ``location`` and
``bbox`` to:
  * every sum of products is charged 16 * 2^-53 times the sum of the magnitudes of its terms (a sum of up to four products in any
    order, with or without fused steps, stays far inside it), on top of what its operands carry in;
  * sin and cos are charged 2 ulp each;
  * the quotient u / w carries (err_u + |u / w| * err_w) / (|w| - err_w) plus its own rounding, and is unbounded (inf) where the
    bound of w reaches |w| / 2 -- a corner on the image plane;
  * the min / max over the eight corners and the clamps carry the largest bound of their operands (both are non-expansive).
``alpha`` is held to two float32 ulps of the arc tangent plus the float64 rounding of the sum.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_annos.npz")
U = 2.0 ** -53
SUM_CHARGE = 16 * U
ANNO_KEYS = ["name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score"]
MARGIN = 1e3                    # the fixture's decisions: every compared value is this many error bounds from its threshold


def np_min(a, b):
    """np.minimum of two float64 values / arrays (a NaN propagates), spelt out."""
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(b < a, b, a))


def np_max(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(b > a, b, a))


def image_of_rows(det_off):
    det_off = np.asarray(det_off, np.int64)
    return np.repeat(np.arange(len(det_off) - 1), np.diff(det_off))


def restate(boxes, det_off, lidar2cam, P2, image_hw):
    """Steps 1-8 for flat float32 boxes [n, 7] -> dict of per-INPUT-row arrays: keep bool [n]; bbox [n, 4], alpha [n], location
    [n, 3], dimensions [n, 3], rotation_y [n] (float64, as written when kept); the bounds location_err [n, 3], bbox_err [n, 4] (of
    the clamped values = of the unclamped ones), alpha_err [n]; raw_bbox [n, 4] (before the clamp) for the decision margins."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 7)
    n = boxes.shape[0]
    img = image_of_rows(det_off)
    assert len(img) == n
    M, P = np.asarray(lidar2cam, np.float64)[img], np.asarray(P2, np.float64)[img]
    hw = np.asarray(image_hw)[img].astype(np.float64).reshape(n, 2)
    with np.errstate(all="ignore"):
        fz = (boxes[:, 2] - (boxes[:, 5] / np.float32(2))).astype(np.float32)               # float32, as the reference's in-place line
        x, y, z = boxes[:, 0].astype(np.float64), boxes[:, 1].astype(np.float64), fz.astype(np.float64)
        loc, loc_err = np.empty((n, 3)), np.empty((n, 3))
        for r in range(3):
            terms = [M[:, r, 0] * x, M[:, r, 1] * y, M[:, r, 2] * z, M[:, r, 3] * 1.0]
            loc[:, r] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
            loc_err[:, r] = SUM_CHARGE * sum(np.abs(t) for t in terms)
        l, h, w, ry = (boxes[:, k].astype(np.float64) for k in (4, 5, 3, 6))
        c, s = np.cos(ry), np.sin(ry)
        c_err, s_err = 2 * np.spacing(np.abs(c)), 2 * np.spacing(np.abs(s))
        pts, errs = [], []
        for k in range(8):
            px, py, pz = l * (0.5 if k & 4 else -0.5), h * (0.0 if k & 2 else -1.0), w * (0.5 if k & 1 else -0.5)
            cx = ((px * c + py * 0.0) + pz * s) + loc[:, 0]
            cy = ((px * 0.0 + py * 1.0) + pz * 0.0) + loc[:, 1]
            cz = ((px * (-s) + py * 0.0) + pz * c) + loc[:, 2]
            ex = SUM_CHARGE * (np.abs(px * c) + np.abs(pz * s) + np.abs(loc[:, 0])) + np.abs(px) * c_err + np.abs(pz) * s_err + loc_err[:, 0]
            ey = SUM_CHARGE * (np.abs(py) + np.abs(loc[:, 1])) + loc_err[:, 1]
            ez = SUM_CHARGE * (np.abs(px * s) + np.abs(pz * c) + np.abs(loc[:, 2])) + np.abs(px) * s_err + np.abs(pz) * c_err + loc_err[:, 2]
            row, row_err = [], []
            for r in range(3):                  # the fourth coordinate is zero: the fourth column of P2 takes no part
                t = [P[:, r, 0] * cx, P[:, r, 1] * cy, P[:, r, 2] * cz]
                row.append((t[0] + t[1]) + t[2])
                row_err.append(SUM_CHARGE * sum(np.abs(v) for v in t) + np.abs(P[:, r, 0]) * ex + np.abs(P[:, r, 1]) * ey + np.abs(P[:, r, 2]) * ez)
            q, q_err = row[2], row_err[2]
            iu, iv = row[0] / q, row[1] / q
            den = np.abs(q) - q_err
            ok = q_err < np.abs(q) / 2
            eu = np.where(ok, (row_err[0] + np.abs(iu) * q_err) / np.where(ok, den, 1.0) + 2 * U * np.abs(iu), np.inf)
            ev = np.where(ok, (row_err[1] + np.abs(iv) * q_err) / np.where(ok, den, 1.0) + 2 * U * np.abs(iv), np.inf)
            pts.append((iu, iv)); errs.append((eu, ev))
        mn_u, mn_v = pts[0]
        mx_u, mx_v = pts[0]
        for iu, iv in pts[1:]:
            mn_u, mn_v, mx_u, mx_v = np_min(mn_u, iu), np_min(mn_v, iv), np_max(mx_u, iu), np_max(mx_v, iv)
        eu = np.max(np.stack([e[0] for e in errs]), 0) if n else np.zeros(0)
        ev = np.max(np.stack([e[1] for e in errs]), 0) if n else np.zeros(0)
        H, W = hw[:, 0], hw[:, 1]
        drop = ((mn_u > W) | (mn_v > H)) | ((mx_u < 0) | (mx_v < 0))
        bbox = np.stack([np_max(mn_u, 0.0), np_max(mn_v, 0.0), np_min(mx_u, W), np_min(mx_v, H)], 1).reshape(n, 4)
        at = np.arctan2(-boxes[:, 1].astype(np.float64), boxes[:, 0].astype(np.float64)).astype(np.float32)    # evaluated in float64, rounded once
        alpha = (-at).astype(np.float64) + ry
        alpha_err = 2 * np.spacing(np.abs(at)).astype(np.float64) + np.spacing(np.abs(alpha))
    return dict(keep=~drop, bbox=bbox, raw_bbox=np.stack([mn_u, mn_v, mx_u, mx_v], 1).reshape(n, 4), alpha=alpha, location=loc,
                dimensions=np.stack([l, h, w], 1).reshape(n, 3), rotation_y=ry, location_err=loc_err,
                bbox_err=np.stack([eu, ev, eu, ev], 1).reshape(n, 4), alpha_err=alpha_err, image=img, hw=hw)


def decision_margins(r):
    """For every row of a :func:`restate` result: the distance of each compared value of step 6 from its threshold, in units of its
    own error bound [n, 4] (bbox[0] vs W, bbox[1] vs H, bbox[2] vs 0, bbox[3] vs 0), and the absolute distances [n, 4].  A NaN operand
    decides nothing (its comparison is false whatever the last bits are): its margin is inf."""
    thr = np.stack([r["hw"][:, 1], r["hw"][:, 0], np.zeros(len(r["hw"])), np.zeros(len(r["hw"]))], 1)
    dist = np.abs(r["raw_bbox"] - thr)
    with np.errstate(all="ignore"):
        ratio = np.where(np.isnan(r["raw_bbox"]), np.inf, dist / r["bbox_err"])
    return ratio, np.where(np.isnan(r["raw_bbox"]), np.inf, dist)


def compact(r, scores, labels, det_off):
    """What the kernel returns for a :func:`restate` result: the kept rows in order.  -> dict(bbox, alpha, box3d, score, label, src,
    out_off, and the bounds bbox_err, location_err, alpha_err of the kept rows)."""
    keep = r["keep"]
    src = np.flatnonzero(keep).astype(np.int32)
    det_off = np.asarray(det_off, np.int64)
    prefix = np.concatenate([[0], np.cumsum(keep)])
    return dict(bbox=r["bbox"][keep], alpha=r["alpha"][keep],
                box3d=np.concatenate([r["location"][keep], r["dimensions"][keep], r["rotation_y"][keep][:, None]], 1),
                score=np.asarray(scores, np.float32)[keep], label=np.asarray(labels, np.int32)[keep], src=src,
                out_off=prefix[det_off].astype(np.int32), bbox_err=r["bbox_err"][keep], location_err=r["location_err"][keep],
                alpha_err=r["alpha_err"][keep])


def within(got, want, bound):
    """|got - want| <= bound elementwise with NaNs in the same places; -> (ok, largest share of the bound used)."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False, np.inf
    m = ~np.isnan(want)
    with np.errstate(all="ignore"):
        diff = np.abs(got[m] - want[m])
        share = np.where(diff == 0, 0.0, diff / bound[m])
    return bool((diff <= bound[m]).all()), float(share.max(initial=0.0))


# ------------------------------------------------------------------------------------------------ fixture layout
def synthetic_calibration(rng, images, other_size_at=None):
    """KITTI-like calibrations: (R0_rect, Tr_velo_to_cam, P2) float64 [images, 4, 4] and image_shape int32 [images, 2].  Focal length
    about 720 px, principal point near the centre of a 375 x 1242 image, small rotations, the usual velodyne -> camera axes, and a
    NON-zero fourth column of P2 (which the reference's projection ignores)."""
    def small_rotation(scale):
        a = rng.normal(0, scale, 3)
        cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        return rz @ ry @ rx
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    rect, trv2c, p2 = np.zeros((images, 4, 4)), np.zeros((images, 4, 4)), np.zeros((images, 4, 4))
    shape = np.tile(np.array([375, 1242], np.int32), (images, 1))
    for i in range(images):
        rect[i, :3, :3], rect[i, 3, 3] = small_rotation(0.01), 1.0
        trv2c[i, :3, :3], trv2c[i, :3, 3], trv2c[i, 3, 3] = small_rotation(0.01) @ axes, rng.normal([0.0, -0.08, -0.27], 0.01), 1.0
        f = rng.uniform(705, 735)
        p2[i] = [[f, 0, rng.uniform(600, 620), rng.uniform(40, 50)], [0, f, rng.uniform(165, 185), rng.uniform(-0.5, 0.5)],
                 [0, 0, 1, rng.uniform(0.002, 0.004)], [0, 0, 0, 1]]
    if other_size_at is not None:
        shape[other_size_at] = [370, 1224]
    return rect, trv2c, p2, shape


def random_boxes(rng, n, x_range=(-5.0, 75.0)):
    """float32 lidar boxes [n, 7] = x, y, z, w, l, h, r."""
    return np.stack([rng.uniform(*x_range, n), rng.uniform(-30, 30, n), rng.uniform(-2.5, 0.5, n), rng.uniform(0.5, 2.2, n),
                     rng.uniform(0.6, 5.5, n), rng.uniform(1.2, 2.2, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32).reshape(n, 7)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def load_fixture(g=None):
    """-> dict: inputs (boxes, scores, labels, det_off, rect, trv2c, P2, image_shape, class_names, image_idx), the recorded annos as a
    list of dicts (``annos``) with their per-image dtype / shape records (``layout``), and lidar2cam = rect @ trv2c per image."""
    g = np.load(GOLDEN) if g is None else g
    f = {k: g[k] for k in ("boxes", "scores", "labels", "det_off", "rect", "trv2c", "P2", "image_shape", "image_idx", "min_margin", "min_distance",
                           "seed")}
    f["class_names"] = [str(c) for c in g["class_names"]]
    f["lidar2cam"] = np.stack([a @ b for a, b in zip(f["rect"], f["trv2c"])])
    num = g["anno_num"]
    off = np.concatenate([[0], np.cumsum(num)])
    f["layout"] = json.loads(str(g["layout"]))
    annos = []
    for i in range(len(num)):
        if num[i]:
            annos.append({k: g["anno_" + k][off[i]:off[i + 1]] for k in ANNO_KEYS})
        else:                                   # recorded as empty_result_anno gave it: dtype and shape from the layout record
            annos.append({k: np.zeros(shape, dtype) for k, (dtype, shape) in f["layout"][i].items()})
        annos[-1]["metadata"] = {"image_idx": int(f["image_idx"][i])}
    f["annos"], f["out_off"] = annos, off.astype(np.int32)
    return f


def fixture_infos(f):
    """The stand-in ``_kitti_infos`` of the fixture (what the generator handed the reference)."""
    return [{"image": {"image_idx": int(f["image_idx"][i]), "image_shape": f["image_shape"][i]},
             "calib": {"R0_rect": f["rect"][i], "Tr_velo_to_cam": f["trv2c"][i], "P2": f["P2"][i]}} for i in range(len(f["image_idx"]))]


class StandinDataset:
    """The two attributes convert_detection_to_kitti_annos reads."""

    def __init__(self, infos, class_names):
        self._kitti_infos, self._class_names = infos, class_names
