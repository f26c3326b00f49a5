"""numpy restatement of the device augmentation (include/second_hip.h, "Training augmentation") and the seeded inputs of
tests/golden/augment.npz.  Written from the specification, not from the kernels: float64 unless the caller passes another dtype,
containment counted as a collision.  tests/golden/make_golden_augment.py pins it -- and the kernels -- to the reference's own
functions; the fixture stores a digest of every input built here, so a drift of these generators is noticed, not absorbed."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")
RANGE = (-70.4, -40.0, -3.0, 70.4, 40.0, 1.0)        # car.fhd.config's point_cloud_range mirrored in x: an x flip keeps boxes inside
BEV_RANGE = (RANGE[0], RANGE[1], RANGE[3], RANGE[4])
LOC_STD, ROT_RANGE = (1.0, 1.0, 0.5), (-0.78539816, 0.78539816)      # car.fhd.config groundtruth_* noise


# ---------------------------------------------------------------------------------------------- geometry
def bev_corners(boxes):
    """[n, 7] -> [n, 4, 2], clockwise from the minimum corner, corners_norm * dims @ [[c, -s], [s, c]] + centre."""
    boxes = np.asarray(boxes)
    norm = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], boxes.dtype)
    local = boxes[:, None, 3:5] * norm[None]
    c, s = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    x = local[..., 0] * c[:, None] + local[..., 1] * s[:, None]
    y = -local[..., 0] * s[:, None] + local[..., 1] * c[:, None]
    return np.stack([x, y], -1) + boxes[:, None, :2]


def _inside_all(a, q):
    """every corner of q strictly inside the clockwise rectangle a"""
    for l in range(4):
        for k in range(4):
            v = a[(k + 1) % 4] - a[k]
            if v[1] * (a[k, 0] - q[l, 0]) - v[0] * (a[k, 1] - q[l, 1]) >= 0:
                return False
    return True


def contained(a, b):
    return _inside_all(a, b) or _inside_all(b, a)


def edges_cross(a, b):
    for k in range(4):
        A, B = a[k], a[(k + 1) % 4]
        for l in range(4):
            C, D = b[l], b[(l + 1) % 4]
            acd = (D[1] - A[1]) * (C[0] - A[0]) > (C[1] - A[1]) * (D[0] - A[0])
            bcd = (D[1] - B[1]) * (C[0] - B[0]) > (C[1] - B[1]) * (D[0] - B[0])
            if acd != bcd:
                abc = (C[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (C[0] - A[0])
                abd = (D[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (D[0] - A[0])
                if abc != abd:
                    return True
    return False


def _standup_overlap(a, b):
    iw = min(a[:, 0].max(), b[:, 0].max()) - max(a[:, 0].min(), b[:, 0].min())
    ih = min(a[:, 1].max(), b[:, 1].max()) - max(a[:, 1].min(), b[:, 1].min())
    return iw > 0 and ih > 0


def collide(a, b):
    """box_collision_test for one pair of [4, 2] rectangles, containment included."""
    return _standup_overlap(a, b) and (edges_cross(a, b) or contained(a, b))


def noise_per_box(boxes, valid, loc_noises, rot_noises, containment_seen=None):
    """One frame: -> selected [n] int64.  ``containment_seen`` (a list) receives (box, try) for every try either implementation
    evaluates that lies wholly inside or around another box at that box's current place (condition (b) of the fixture)."""
    boxes = np.asarray(boxes)
    n, t = boxes.shape[0], loc_noises.shape[1]
    cur = bev_corners(boxes)
    selected = -np.ones(n, np.int64)
    for i in range(n):
        if not valid[i]:
            continue
        for j in range(t):
            c, s = np.cos(rot_noises[i, j]), np.sin(rot_noises[i, j])
            d = cur[i] - boxes[i, :2]
            tr = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c], -1) + (boxes[i, :2] + loc_noises[i, j, :2])
            near = [k for k in range(n) if k != i and _standup_overlap(tr, cur[k])]
            if containment_seen is not None and any(contained(tr, cur[k]) for k in near):
                containment_seen.append((i, j))
            if not any(collide(tr, cur[k]) for k in near):
                selected[i] = j
                cur[i] = tr
                break
    return selected


def select_transform(noise, selected, valid):
    out = np.zeros((noise.shape[0],) + noise.shape[2:], noise.dtype)
    for i, s in enumerate(selected):
        if s >= 0 and valid[i]:
            out[i] = noise[i, s]
    return out


def box_frame_excess(points, boxes):
    """[N, n] float64: max over the three box axes of |local coordinate| - half extent; < 0 inside, its magnitude bounds the distance
    to the nearest face from below for a point that is inside or beside one."""
    p, b = np.asarray(points, np.float64)[:, None, :3], np.asarray(boxes, np.float64)[None]
    d = p - b[..., :3]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    lx, ly = d[..., 0] * c - d[..., 1] * s, d[..., 0] * s + d[..., 1] * c
    return np.max(np.stack([np.abs(lx) - b[..., 3] / 2, np.abs(ly) - b[..., 4] / 2, np.abs(d[..., 2]) - b[..., 5] / 2]), 0)


def points_in_boxes_mask(points, boxes):
    return box_frame_excess(points, boxes) < 0 if len(boxes) else np.zeros((len(points), 0), bool)


def first_set(mask, valid):
    m = mask & np.asarray(valid, bool)[None]
    return np.where(m.any(1), m.argmax(1), -1) if m.shape[1] else -np.ones(m.shape[0], np.int64)


def _rot(xy, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.stack([xy[..., 0] * c + xy[..., 1] * s, -xy[..., 0] * s + xy[..., 1] * c], -1)


def augment_frame(points, boxes, valid, loc_t, rot_t, params, bev_range=BEV_RANGE, dtype=np.float64):
    """One frame through stages 1-6 of the specification: -> (points [N, 3], boxes [n, 7] before the filter, keep [n] bool)."""
    p, b = np.array(points, dtype)[:, :3], np.array(boxes, dtype)
    loc_t, rot_t, params = np.asarray(loc_t, dtype), np.asarray(rot_t, dtype), np.asarray(params, dtype)
    fb = first_set(points_in_boxes_mask(points, boxes), valid)
    for i in np.nonzero(fb >= 0)[0]:
        g = fb[i]
        q = p[i] - b[g, :3]
        q[:2] = _rot(q[:2], rot_t[g])
        p[i] = q + b[g, :3] + loc_t[g]
    v = np.asarray(valid, bool)
    b[v, :3] += loc_t[v]
    b[v, 6] += rot_t[v]
    if params[1]:
        p[:, 1], b[:, 1], b[:, 6] = -p[:, 1], -b[:, 1], -b[:, 6] + dtype(np.pi)
    if params[0]:
        p[:, 0], b[:, 0], b[:, 6] = -p[:, 0], -b[:, 0], -b[:, 6]
    p[:, :2], b[:, :2] = _rot(p[:, :2], params[2]), _rot(b[:, :2], params[2])
    b[:, 6] += params[2]
    p *= params[3]
    b[:, :6] *= params[3]
    p += params[4:7]
    b[:, :3] += params[4:7]
    keep = v & (b[:, 0] > bev_range[0]) & (b[:, 0] < bev_range[2]) & (b[:, 1] > bev_range[1]) & (b[:, 1] < bev_range[3])
    b[:, 6] = b[:, 6] - np.floor(b[:, 6] / dtype(2 * np.pi) + dtype(0.5)) * dtype(2 * np.pi)
    return p, b, keep


# ---------------------------------------------------------------------------------------------- seeded inputs of the fixture
def _boxes(rs, n, spacing=5.5):
    """n car-sized boxes on a jittered grid inside the range (neighbours close enough for some tries to collide)."""
    cols = int(np.ceil(np.sqrt(n * 70.4 / 80.0))) or 1
    rows = int(np.ceil(n / cols)) if n else 0
    gx, gy = np.meshgrid(np.arange(cols), np.arange(rows))
    cx = 6.0 + gx.reshape(-1)[:n] * spacing + rs.uniform(-0.5, 0.5, n)
    cy = -(rows - 1) * spacing / 2 + gy.reshape(-1)[:n] * spacing + rs.uniform(-0.5, 0.5, n)
    return np.stack([cx, cy, rs.uniform(-1.2, -0.6, n), rs.uniform(1.5, 1.9, n), rs.uniform(3.4, 4.4, n), rs.uniform(1.4, 1.8, n),
                     rs.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)


def _points(rs, n, boxes):
    """n points: about a third inside boxes (within 90 % of the half extents), the rest anywhere in the range."""
    pts = np.stack([rs.uniform(0.5, RANGE[3] - 0.5, n), rs.uniform(RANGE[1] + 0.5, RANGE[4] - 0.5, n),
                    rs.uniform(-2.5, 0.5, n), rs.uniform(0, 1, n)], 1)
    if len(boxes):
        for i in range(0, n, 3):
            b = boxes[rs.randint(len(boxes))].astype(np.float64)
            l = rs.uniform(-0.45, 0.45, 3) * b[3:6]
            pts[i, :2] = _rot(l[None, :2], b[6])[0] + b[:2]
            pts[i, 2] = b[2] + l[2]
    return pts.astype(np.float32)


def build_frame(seed, n_boxes, n_points, num_try, kind=""):
    """One candidate frame: dict(points [N, 4], boxes [n, 7], valid, classes, importance, loc_noises [n, T, 3], rot_noises [n, T]),
    float32.  ``kind`` adds what a special frame needs by construction."""
    rs = np.random.RandomState(seed)
    boxes = _boxes(rs, n_boxes)
    valid = np.ones(n_boxes, bool)
    loc = (rs.normal(size=(n_boxes, num_try, 3)) * np.array(LOC_STD)).astype(np.float32)
    rot = rs.uniform(ROT_RANGE[0], ROT_RANGE[1], (n_boxes, num_try)).astype(np.float32)
    if "overlap" in kind:          # boxes 1 and 2 overlap (edges cross, neither contains the other): points inside both
        boxes[2] = boxes[1]
        boxes[2, 0] += 0.8
        boxes[2, 6] += 0.3
    if "fail" in kind:             # every try of box 0 drops it half a width onto box 1: selected = -1
        d = (boxes[1, :2] - boxes[0, :2]).astype(np.float64)
        loc[0, :, :2] = (d + _rot(np.array([[0.5 * boxes[1, 3], 0.0]]), boxes[1, 6])[0]).astype(np.float32)
        rot[0] = (boxes[1, 6] - boxes[0, 6] + 0.2) * np.ones(num_try, np.float32)
    if "late" in kind:             # the first 70 tries of the last box land on its predecessor's ORIGINAL place: a success past lane 63
        a, b = n_boxes - 1, n_boxes - 2
        d = (boxes[b, :2] - boxes[a, :2]).astype(np.float64)
        m = min(70, num_try - 1)
        loc[a, :m, :2] = (d + _rot(np.array([[0.4 * boxes[b, 3], 0.3]]), boxes[b, 6])[0]).astype(np.float32)
        loc[b, :, :2] *= 0.05      # ... which stays (almost) where it was
        rot[a, :m] = boxes[b, 6] - boxes[a, 6] + 0.25
    if "invalid" in kind:          # boxes 0 and 3 are not of a trained class: they block, they never move, they are dropped
        valid[[0, 3]] = False
        d = (boxes[3, :2] - boxes[4, :2]).astype(np.float64)      # box 4's first try lands on invalid box 3
        loc[4, 0, :2] = (d + _rot(np.array([[0.5 * boxes[3, 3], 0.2]]), boxes[3, 6])[0]).astype(np.float32)
        rot[4, 0] = boxes[3, 6] - boxes[4, 6] + 0.2
    if "edge" in kind:             # the last box sits 0.3 m inside the range's far edge: scaling / translation can push it out
        boxes[-1, 0] = RANGE[3] - 0.3
    pts = _points(rs, n_points, boxes)
    return dict(points=pts, boxes=boxes, valid=valid, classes=rs.randint(1, 4, n_boxes).astype(np.int32),
                importance=rs.uniform(0.5, 1.5, n_boxes).astype(np.float32), loc_noises=loc, rot_noises=rot)


# case -> (tries, [(boxes, points, kind)] per frame).  Batch 1 and a ragged batch of 5; 0 / 1 / 3 / 12 / 70 boxes (70 crosses a wave);
# 1 / 5 / 100 tries (100 crosses a wave); 0 / 1 / 257 / ~600 points.
CASES = {
    "b1_t5": (5, [(12, 257, "overlap fail invalid edge")]),
    "b1_t1": (1, [(3, 65, "")]),
    "b5_t100": (100, [(0, 257, ""), (1, 0, ""), (3, 1, "overlap"), (70, 601, "invalid edge"), (12, 150, "overlap fail late")]),
}


def concat_frames(frames):
    """list of build_frame dicts -> batch dict with point_offsets / box_offsets [B+1] int32."""
    out = {k: np.concatenate([f[k] for f in frames]) for k in frames[0]}
    out["point_offsets"] = np.concatenate([[0], np.cumsum([len(f["points"]) for f in frames])]).astype(np.int32)
    out["box_offsets"] = np.concatenate([[0], np.cumsum([len(f["boxes"]) for f in frames])]).astype(np.int32)
    return out


def digest(batch):
    h = hashlib.sha256()
    for k in sorted(batch):
        h.update(k.encode())
        h.update(np.ascontiguousarray(batch[k]).tobytes())
    return h.hexdigest()


def load_case(name, golden=None):
    """-> (inputs rebuilt from the seeds the fixture admitted, the fixture's arrays for this case with the prefix stripped)."""
    golden = golden if golden is not None else np.load(GOLDEN)
    tries, frames = CASES[name]
    seeds = golden[f"{name}/seeds"]
    batch = concat_frames([build_frame(int(s), nb, npts, tries, kind) for s, (nb, npts, kind) in zip(seeds, frames)])
    assert digest(batch) == str(golden[f"{name}/digest"]), "the seeded inputs no longer match the ones the fixture was recorded on"
    batch["frame_params"] = golden[f"{name}/frame_params"]
    ref = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "/")}
    return batch, ref


def fixture_first_and_counts(batch, ref):
    """From the fixture's per-frame masks (the reference's points_in_rbbox): the first set column of each point among the valid boxes,
    as a global box row (-1 for none), and the points inside every box."""
    po, bo = batch["point_offsets"], batch["box_offsets"]
    first, counts = [], []
    for f in range(len(bo) - 1):
        n, npts = bo[f + 1] - bo[f], po[f + 1] - po[f]
        mask = np.unpackbits(ref[f"mask{f}"], count=npts * n).reshape(npts, n).astype(bool)
        fb = first_set(mask, batch["valid"][bo[f]:bo[f + 1]])
        first.append(np.where(fb >= 0, fb + bo[f], -1))
        counts.append(mask.sum(0))
    return np.concatenate(first), np.concatenate(counts)


def chain(batch, dtype=np.float64):
    """The whole specified chain on a batch, frame by frame: dict with selected, first_box (global rows), counts, points [N, 3],
    kept boxes / classes / importance, new offsets."""
    po, bo = batch["point_offsets"], batch["box_offsets"]
    out = dict(selected=[], first_box=[], counts=[], points=[], boxes=[], classes=[], importance=[], offsets=[0])
    for f in range(len(bo) - 1):
        ps, bs = slice(po[f], po[f + 1]), slice(bo[f], bo[f + 1])
        pts, boxes, valid = batch["points"][ps], batch["boxes"][bs], batch["valid"][bs]
        loc, rot = batch["loc_noises"][bs].astype(dtype), batch["rot_noises"][bs].astype(dtype)
        sel = noise_per_box(boxes.astype(dtype), valid, loc, rot)
        mask = points_in_boxes_mask(pts, boxes)
        fb = first_set(mask, valid)
        p, b, keep = augment_frame(pts, boxes, valid, select_transform(loc, sel, valid), select_transform(rot, sel, valid),
                                   batch["frame_params"][f], dtype=dtype)
        out["selected"].append(sel)
        out["first_box"].append(np.where(fb >= 0, fb + bo[f], -1))
        out["counts"].append(mask.sum(0))
        out["points"].append(p)
        out["boxes"].append(b[keep])
        out["classes"].append(batch["classes"][bs][keep])
        out["importance"].append(batch["importance"][bs][keep])
        out["offsets"].append(out["offsets"][-1] + int(keep.sum()))
    res = {k: np.concatenate(v) if len(v) else np.zeros(0) for k, v in out.items() if k != "offsets"}
    res["offsets"] = np.array(out["offsets"], np.int32)
    return res


def _mag(v):
    """[.., 3] -> the magnitude that enters each output element: the rotations about z mix x and y, so the x and y elements carry
    hypot(x, y); z carries |z|."""
    v = np.asarray(v, np.float64)
    r = np.hypot(v[..., 0], v[..., 1])
    return np.stack([r, r, np.abs(v[..., 2])], -1)


def point_bound(batch):
    """The issue's per-element bound 16 * 2^-24 * (|p| + |c| + |t| + 1) for every point coordinate [N, 3]: p the input point, c the
    centre of the box that moves it (0 without one), t the per-object plus the global translation.  Its basis -- about 12 roundings on
    magnitudes bounded by these terms -- fixes what |.| means for an element: a rotation about z computes x' and y' from BOTH x and y, so
    the magnitude behind the x and y elements is hypot(x, y) of the term (:func:`_mag`), not the element's own coordinate (for a point
    at x = 60, y = 0.1 a single rounding of the x product already exceeds 16 ulp of 1.1); z never mixes and keeps |z|."""
    po, bo = batch["point_offsets"], batch["box_offsets"]
    ref = chain(batch)
    loc_t = np.concatenate([select_transform(batch["loc_noises"][bo[f]:bo[f + 1]].astype(np.float64),
                                             ref["selected"][bo[f]:bo[f + 1]], batch["valid"][bo[f]:bo[f + 1]])
                            for f in range(len(bo) - 1)] + [np.zeros((0, 3))])
    p = _mag(batch["points"][:, :3])
    c, t = np.zeros_like(p), np.zeros_like(p)
    for f in range(len(po) - 1):
        t[po[f]:po[f + 1]] = _mag(batch["frame_params"][f, 4:7])
    fb = ref["first_box"]
    has = fb >= 0
    c[has] = _mag(batch["boxes"][fb[has], :3])
    t[has] += _mag(loc_t[fb[has]])
    return 16 * 2.0 ** -24 * (p + c + t + 1)


def box_bound(batch, kept_rows):
    """The same bound for columns 0-5 of the kept boxes: for the centre p = c = the box's input centre and t as above; the extents are
    only scaled (p = the extent, c = t = 0)."""
    bo = batch["box_offsets"]
    ref = chain(batch)
    b = batch["boxes"][kept_rows].astype(np.float64)
    frame = np.searchsorted(bo, kept_rows, side="right") - 1
    t = np.zeros((len(kept_rows), 3))
    for r, (g, f) in enumerate(zip(kept_rows, frame)):
        s = ref["selected"][g]
        t[r] = _mag(batch["frame_params"][f, 4:7]) + (_mag(batch["loc_noises"][g, s]) if s >= 0 else 0)
    centre = 2 * _mag(b[:, :3]) + t + 1
    return 16 * 2.0 ** -24 * np.concatenate([centre, np.abs(b[:, 3:6]) + 1], 1)
