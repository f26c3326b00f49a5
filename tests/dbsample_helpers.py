"""numpy restatement of the device database sampling (include/second_hip.h, "Ground-truth database sampling") and the seeded inputs
of tests/golden/dbsample.npz.  Written from the specification, not from the kernels: acceptance in float64 unless the caller passes
another dtype, containment counted as a collision (augment_helpers.collide); the merge in float32, as the reference does it.
tests/golden/make_golden_dbsample.py pins it -- and the kernels -- to the reference's own DataBaseSamplerV2; the fixture stores a
digest of every input built here, so a drift of these generators is noticed, not absorbed."""
import os

import numpy as np

import augment_helpers as ah

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbsample.npz")
MAX_BOXES = 512                                       # gt boxes + candidates in use a frame may hold (sec_db_sample_select_f32)
DIMS = {"Car": (1.7, 3.9, 1.6), "Pedestrian": (0.6, 0.8, 1.73), "Cyclist": (0.6, 1.76, 1.73), "Van": (1.9, 5.0, 2.2)}


# ---------------------------------------------------------------------------------------------- the specification
def num_table(groups, rate):
    """[C, T]: np.round(rate * (max_num - n)) as sample_all computes it (float64, half to even), never negative."""
    t = max(m for _, m in groups) + 1
    return np.array([[max(int(np.round(rate * int(m - n))), 0) for n in range(t)] for _, m in groups], np.int32)


def accept_class(avoid, cand, seen=None):
    """sample_class_v2's walk on corner lists: -> the indices of ``cand`` accepted.  Candidate i is rejected when its row of the
    collision matrix has an entry: a collision with an avoid box, with an earlier ACCEPTED candidate or with ANY later candidate
    (only a rejected candidate's column is cleared, and only when the walk reaches it).  ``seen`` receives (i, j) for every pair
    tested where one rectangle lies wholly inside the other."""
    total = list(avoid) + list(cand)
    na, m = len(avoid), len(cand)
    coll = np.zeros((m, na + m), bool)
    for i in range(m):
        for j in range(na + m):
            if j == na + i:
                continue
            coll[i, j] = ah.collide(cand[i], total[j])
            if seen is not None and ah._standup_overlap(cand[i], total[j]) and ah.contained(cand[i], total[j]):
                seen.append((i, j))
    out = []
    for i in range(m):
        if coll[i].any():
            coll[:, na + i] = False
        else:
            out.append(i)
    return out


def sample_frame(gt_boxes, gt_classes, db_boxes, cands, class_of_group, table, dtype=np.float64, seen=None):
    """One frame: ``cands`` [C][k] database rows (-1 = absent) -> (accepted rows in order, accepted per group)."""
    gt_boxes, gt_classes = np.asarray(gt_boxes).reshape(-1, 7), np.asarray(gt_classes)
    use = []
    for c, cls in enumerate(class_of_group):
        n = int((gt_classes == cls).sum()) if cls > 0 else 0
        want = int(table[c][n]) if n < len(table[c]) else 0
        use.append([int(r) for r in cands[c] if 0 <= r < len(db_boxes)][:max(want, 0)])
    if len(gt_boxes) + sum(len(u) for u in use) > MAX_BOXES:
        return [], [0] * len(use)
    avoid = list(ah.bev_corners(gt_boxes.astype(dtype)))
    accepted, per_group = [], []
    for rows in use:
        corners = ah.bev_corners(np.asarray(db_boxes)[rows].astype(dtype).reshape(-1, 7))
        idx = accept_class(avoid, corners, seen)
        accepted += [rows[i] for i in idx]
        avoid += [corners[i] for i in idx]
        per_group.append(len(idx))
    return accepted, per_group


def merge_frame(points, db_boxes, pool_points, pool_offsets, accepted, remove=True):
    """-> (merged points float32, removed [N] bool): the accepted objects' points, x y z plus the box centre (float32 + float32),
    then the scene points outside every accepted box, in order."""
    points, db_boxes = np.asarray(points, np.float32), np.asarray(db_boxes, np.float32)
    parts = []
    for r in accepted:
        p = np.array(pool_points[pool_offsets[r]:pool_offsets[r + 1]], np.float32)
        p[:, :3] += db_boxes[r, :3]
        parts.append(p)
    removed = np.zeros(len(points), bool)
    if remove and len(accepted) and len(points):
        removed = ah.points_in_boxes_mask(points, db_boxes[list(accepted)]).any(1)
    return np.concatenate(parts + [points[~removed]]).astype(np.float32), removed


def chain(batch, db, case, cands, remove=True):
    """The whole specified chain on a batch: dict with accepted (flat) / accepted_offsets / accepted_per_group, the merged boxes,
    classes, mask, importance, box_offsets, points, point_offsets and the removed flags of the scene points."""
    table = num_table(case["groups"], case["rate"])
    cog = [case["class_names"].index(n) + 1 for n, _ in case["groups"]]
    po, bo = batch["point_offsets"], batch["box_offsets"]
    out = dict(accepted=[], accepted_offsets=[0], accepted_per_group=[], boxes=[], classes=[], mask=[], importance=[], box_offsets=[0],
               points=[], point_offsets=[0], removed=[])
    for f in range(len(bo) - 1):
        bs, ps = slice(bo[f], bo[f + 1]), slice(po[f], po[f + 1])
        acc, per = sample_frame(batch["boxes"][bs], batch["classes"][bs], db["boxes"], cands[f], cog, table)
        cls = [c for c, k in zip(cog, per) for _ in range(k)]
        pts, removed = merge_frame(batch["points"][ps], db["boxes"], db["points"], db["offsets"], acc, remove)
        out["accepted"] += acc
        out["accepted_offsets"].append(len(out["accepted"]))
        out["accepted_per_group"].append(per)
        out["boxes"] += [batch["boxes"][bs], db["boxes"][acc].reshape(-1, 7)]
        out["classes"] += [batch["classes"][bs], np.array(cls, np.int32)]
        out["mask"] += [batch["valid"][bs], np.ones(len(acc), bool)]
        out["importance"] += [batch["importance"][bs], np.full(len(acc), case["sample_importance"], np.float32)]
        out["box_offsets"].append(out["box_offsets"][-1] + bo[f + 1] - bo[f] + len(acc))
        out["points"].append(pts)
        out["point_offsets"].append(out["point_offsets"][-1] + len(pts))
        out["removed"].append(removed)
    for k in ("boxes", "classes", "mask", "importance", "points", "removed"):
        out[k] = np.concatenate(out[k])
    for k in ("accepted", "accepted_offsets", "accepted_per_group", "box_offsets", "point_offsets"):
        out[k] = np.array(out[k], np.int32)
    return out


# ---------------------------------------------------------------------------------------------- seeded inputs of the fixture
# case -> sampler settings, the pool ({class: objects} or "ab": the hand-placed pool of the later-candidate case) and the frames
# (gt names or a count, scene points).  The frames of a case pass through ONE sampler in order, so the end of a class's permutation
# (fewer candidates than asked, then a reshuffle) falls where the draws put it.
CASES = {
    # 15 cars at rate 1: a frame without gt boxes, one without points, one of > 4 blocks of points; the permutation ends on the way
    "car": dict(class_names=["Car"], groups=[("Car", 15)], rate=1.0, sample_importance=1.0, pool={"Car": 40}, pool_seed=11,
                min_num_points={"Car": 5}, removed_difficulties=[-1], gt_names=["Car", "Car", "Car", "Van"],
                frames=[(("Car", "Van", "Car"), 800), (0, 600), (5, 0), (12, 1300)]),
    # one gt box, candidates A and B that overlap each other and nothing else: the earlier of the two is rejected because of the
    # later one, which is accepted; a greedy test against what was accepted so far would take the earlier one
    "ab": dict(class_names=["Car"], groups=[("Car", 5)], rate=1.0, sample_importance=1.0, pool="ab", pool_seed=12,
               min_num_points={}, removed_difficulties=[], gt_names=["Car"], frames=[(("Car",), 300)]),
    # three classes at rate 0.5.  Frame 0: 2 cars of 7 -> round(2.5) = 2 (to even, down), 1 pedestrian of 4 -> round(1.5) = 2 (to
    # even, up), 2 cyclists of 2 -> nothing to draw; a van that is no target class
    "multi": dict(class_names=["Car", "Pedestrian", "Cyclist"], groups=[("Car", 7), ("Pedestrian", 4), ("Cyclist", 2)], rate=0.5,
                  sample_importance=0.7, pool={"Car": 20, "Pedestrian": 12, "Cyclist": 10}, pool_seed=13,
                  min_num_points={"Car": 5, "Pedestrian": 3}, removed_difficulties=[-1],
                  gt_names=["Car", "Pedestrian", "Cyclist", "Van"],
                  frames=[(("Car", "Car", "Pedestrian", "Cyclist", "Cyclist", "Van"), 500), (4, 400), (2, 250)]),
}
NUM_POINT_FEATURES = 4


def _object(rs, name, box=None):
    d = DIMS[name]
    if box is None:
        box = [rs.uniform(3, 45), rs.uniform(-20, 20), rs.uniform(-1.2, -0.6), d[0] * rs.uniform(0.9, 1.1), d[1] * rs.uniform(0.9, 1.1),
               d[2] * rs.uniform(0.9, 1.1), rs.uniform(-np.pi, np.pi)]
    box = np.array(box, np.float32)
    n = rs.randint(0, 61)
    local = rs.uniform(-0.45, 0.45, (n, 3)) * box[3:6].astype(np.float64)
    pts = np.concatenate([ah._rot(local[:, :2], box[6]), local[:, 2:], rs.uniform(0, 1, (n, NUM_POINT_FEATURES - 3))], 1).astype(np.float32)
    return box, pts


def build_pool(case):
    """{name: [info]} as create_groundtruth_database pickles it, plus ``points`` (what the info's .bin file holds) in every info."""
    rs = np.random.RandomState(case["pool_seed"])
    if case["pool"] == "ab":
        placed = [[15.0, 0, -1, 1.7, 3.9, 1.6, 0.0], [15.5, 0.5, -1, 1.7, 3.9, 1.6, 0.3], [35.0, 10, -1, 1.7, 3.9, 1.6, 0.0],
                  [50.0, -20, -1, 1.7, 3.9, 1.6, 1.0]]
        spec = [("Car", b) for b in placed]
    else:
        spec = [(name, None) for name, n in case["pool"].items() for _ in range(n)]
    infos = {}
    for name, box in spec:
        box, pts = _object(rs, name, box)
        i = len(infos.setdefault(name, []))
        infos[name].append(dict(name=name, path=f"gt_database/{name}_{i}.bin", box3d_lidar=box, num_points_in_gt=len(pts),
                                difficulty=int(rs.randint(-1, 3)) if case["pool"] != "ab" else 0, points=pts))
    return infos


def pool_arrays(infos, filtered):
    """The filtered pool as the device holds it: rows in class order, then in the order of ``filtered`` {name: info indices}."""
    rows = [(n, i) for n in infos for i in filtered[n]]
    pts = [infos[n][i]["points"] for n, i in rows]
    return dict(boxes=np.stack([infos[n][i]["box3d_lidar"] for n, i in rows]).astype(np.float32),
                points=np.concatenate(pts), offsets=np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32),
                names=[n for n, _ in rows])


def build_frame(case, infos, seed, gt, n_points):
    """One candidate frame: dict(points [N, 4], boxes [n, 7], names, classes, valid, importance), float32.  About a third of the
    points lie inside objects of the pool at their database place, so accepted objects remove some."""
    rs = np.random.RandomState(seed)
    names = list(gt) if isinstance(gt, tuple) else [case["gt_names"][i] for i in rs.randint(0, len(case["gt_names"]), gt)]
    boxes = ah._boxes(rs, len(names))
    if case["pool"] == "ab":
        boxes[:, :2] = (5.0, 0.0)
    for i, n in enumerate(names):
        boxes[i, 3:6] = np.array(DIMS[n]) * rs.uniform(0.9, 1.1, 3)
    pts = ah._points(rs, n_points, boxes)
    every = [info["box3d_lidar"] for v in infos.values() for info in v]
    for i in range(1, n_points, 3):
        b = every[rs.randint(len(every))].astype(np.float64)
        l = rs.uniform(-0.45, 0.45, 3) * b[3:6]
        pts[i, :2] = (ah._rot(l[None, :2], b[6])[0] + b[:2]).astype(np.float32)
        pts[i, 2] = np.float32(b[2] + l[2])
    cn = case["class_names"]
    return dict(points=pts, boxes=boxes, names=np.array(names, dtype="<U12"), classes=np.array([cn.index(n) + 1 if n in cn else 0 for n in names], np.int32),
                valid=np.array([n in cn for n in names], bool), importance=rs.uniform(0.5, 1.5, len(names)).astype(np.float32))


def concat_frames(frames):
    out = {k: np.concatenate([f[k] for f in frames]) for k in frames[0] if k != "names"}
    out["point_offsets"] = np.concatenate([[0], np.cumsum([len(f["points"]) for f in frames])]).astype(np.int32)
    out["box_offsets"] = np.concatenate([[0], np.cumsum([len(f["boxes"]) for f in frames])]).astype(np.int32)
    return out


def load_case(name, golden=None):
    """-> (case, infos, pool arrays, batch rebuilt from the admitted seeds, the fixture's arrays for this case, prefix stripped)."""
    golden = golden if golden is not None else np.load(GOLDEN)
    case = CASES[name]
    ref = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "/")}
    infos = build_pool(case)
    db = pool_arrays(infos, {n: ref[f"filtered/{n}"] for n in infos})
    frames = [build_frame(case, infos, int(s), gt, npts) for s, (gt, npts) in zip(ref["seeds"], case["frames"])]
    batch = concat_frames(frames)
    assert ah.digest(dict(batch, db_boxes=db["boxes"], db_points=db["points"], db_offsets=db["offsets"])) == str(ref["digest"]), \
        "the seeded inputs no longer match the ones the fixture was recorded on"
    return case, infos, db, batch, ref


def candidates_of(ref):
    """The fixture's candidates [F, C, K] as nested lists without the padding."""
    return [[[int(r) for r in row if r >= 0] for row in frame] for frame in ref["candidates"]]
