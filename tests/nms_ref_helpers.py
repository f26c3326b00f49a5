"""float64 geometry references for csrc/nms.hip (rotated IoU matrix, greedy NMS of both kinds) and the seeded inputs of
tests/test_gpu_nms_edges.py.  numpy only; tests/test_nms_ref_host.py pins everything here to the executed reference's recorded outputs,
to the fp32 oracle and to planted mistakes, on the CPU.

References
  rect_inter64(a, b)      exact convex clipping (Sutherland-Hodgman) of two rotated rectangles in float64.  The inputs are the float32
                          rows (x, y, w, l, r); the corners follow box_corners (nms_gpu.py:353-376) with cos / sin taken in float64.
  iou64(a, b, criterion)  a = box n, b = query box k of ops.rotate_iou(boxes, qboxes): -1 IoU, 0 inter / area(b), 1 inter / area(a),
                          2 inter (include/second_hip.h: criterion 0 divides by the QUERY box's area).
  aa_iou64(a, b, eps)     the `+eps` axis-aligned IoU of (x1, y1, x2, y2) rows (box_np_ops.iou_jit / nms_gpu.iou_device with eps = 1).
  greedy_nms64(...)       the sequential greedy loop on top of either.

General position.  The reference algorithm (point-in-quad tests with a 1e-6 tolerance, strict segment crossings, an angular sort) is not
geometry when a corner of one rectangle lies on an edge line of the other: collinear edges and duplicated rotated boxes give 1 or 1/3
depending on the libm (tests/test_gpu_parity.py::test_rotate_iou_degenerate_and_tied_polygons_vs_oracle).  general_position(a, b, ETA)
is true when no corner of either rectangle lies within ETA = 1e-3 of an edge SEGMENT of the other; only such pairs are compared with
float64.  For two disjoint rectangles the smallest corner-to-segment distance is the distance between them, so a disjoint pair in
general position is at least ETA apart: no fp32 clipper finds a vertex there and its intersection is exactly 0.

The intersection bound, inter_bound(a, b) = C * delta * P
  delta = 2^-23 (max(|x|, |y|) + max side) over the two boxes: one float32 rounding (2^-24) of a corner coordinate, twice, because the
          corner is a sum of two rounded products and the centre;
  P     = the smaller of the two perimeters: moving every edge of the intersection polygon by delta changes its area by at most delta
          times its perimeter, and a convex polygon inside both rectangles has at most the smaller perimeter.
  C     is the number of such roundings the clipper stacks up (crossing points are quotients of differences of products of corner
        coordinates, the fan sums up to six triangle areas).  It is MEASURED on the fp32 oracle (oracle.rotate_iou(..., 2), CPU), never
        on the device: C0 = the largest |oracle - rect_inter64| / (delta P) over the general-position pairs of every IoU-matrix input of
        this file (iou_matrix_cases(): generators car / long / small x the six (N, K) shapes, 18 inputs), and C = 4 C0 --
        the factor 4 for the device's sinf / cosf differing from the host libm in the last bits and for the division.
        Recorded: C0 = 2.2 (measured 2.18, on the `car` generator at (64, 64); largest absolute error of an intersection 1.9e-4; at most
        0.8 % of the pairs of an input are outside general position, the duplicate included), C = 8.8.
        test_nms_ref_host.py re-measures C0 and fails when it exceeds the recorded value.
        The model's limit: the clipper's crossing points come from cross products of ABSOLUTE coordinates (A0 B1 - B0 A1), whose rounding
        |x| |y| 2^-24 / side is not in delta P.  Boxes of side 0.05-0.3 at coordinates up to 70 m measure C0 = 39 on the oracle; the
        `small` generator therefore stays within 4 m of the origin, and such inputs are outside this comparison.
Propagation to the quotients (u = 2^-24, e = inter_bound, I the float64 intersection, a1, a2 the exact areas w l):
  criterion 2   |v - I| <= e
  criterion 0/1 v = fl(I' / fl(w l)):  |v - I / A| <= e / A + 3 u I / A          (area product, quotient, and I' / A against I / A)
  criterion -1  v = fl(I' / fl(fl(fl(a1) + fl(a2)) - I')).  The denominator U' differs from U = a1 + a2 - I by at most
                e + 5 u U (two products and one sum, each relative to a1 + a2 <= 2 U, and the difference relative to U), so
                v lies in [(I - e) / (U + e + 5 u U), (I + e) / (U - e - 5 u U)] widened by the quotient's own rounding 2 u v;
                iou_bound() evaluates exactly that interval (infinite when U - e - 5 u U <= 0).
The axis-aligned bound (aa_bound) is the same interval with e = the rounding of the two clipped lengths, see there.

Decision band.  A greedy decision is comparable with float64 only where |IoU - thr| exceeds the pair's bound (or the intersection is
exactly 0 by the general-position argument above).  greedy_nms64 returns the smallest |IoU - thr| over the pairs it consulted and, in
``info``, the smallest |IoU - thr| / bound; the input generators filter the pairs they can (two-box frames) and place the others by
construction, and the host test asserts that every consulted pair of every GPU input is outside its band.
"""
import functools

import numpy as np

U24 = 2.0 ** -24
ETA = 1e-3
C0 = 2.2
C = 4.0 * C0
FAR_GAP = 2e-3                 # standup gap (float64) above which the device must return exactly 0 (far_apart's margin is 1e-3)
THRESHOLDS = (0.0, 0.01, 0.1, 0.3, 0.5, 0.9)
PAIR_SHAPES = ("square", "car", "long", "small", "far")
PAIR_FRAMES = 4096
IOU_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (129, 1), (1, 129))
IOU_GENERATORS = ("car", "long", "small")
TILE_POSITIONS = ((0, 1), (15, 16), (16, 17), (63, 64), (0, 64), (0, -1), (-2, -1))      # negative = counted from n


# ---------------------------------------------------------------------------------------------------------------- geometry
def _rows(a, width=5):
    a = np.asarray(a, np.float32)
    assert a.shape[-1] >= width
    return a[..., :width].astype(np.float64)


def corners64(b):
    """[..., 5] float32 rows -> [..., 4, 2] float64 corners in box_corners' order."""
    b = _rows(b)
    x, y, w, l, r = (b[..., i, None] for i in range(5))
    c, s = np.cos(r), np.sin(r)
    xs = np.concatenate([-w / 2, -w / 2, w / 2, w / 2], -1)
    ys = np.concatenate([-l / 2, l / 2, l / 2, -l / 2], -1)
    return np.stack([c * xs + s * ys + x, -s * xs + c * ys + y], -1)


def _shoelace(poly, cnt):
    v = poly.shape[1]
    idx = np.arange(v)[None]
    nidx = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    nx = np.take_along_axis(poly[..., 0], nidx, 1)
    ny = np.take_along_axis(poly[..., 1], nidx, 1)
    term = np.where(idx < cnt[:, None], poly[..., 0] * ny - nx * poly[..., 1], 0.0)
    return 0.5 * term.sum(1)


def _clip_halfplane(poly, cnt, p0, e, sgn):
    """Sutherland-Hodgman step for M polygons at once: keep sgn * cross(e, q - p0) >= 0."""
    m, v, _ = poly.shape
    idx = np.arange(v)[None]
    valid = idx < cnt[:, None]
    nidx = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    d = sgn[:, None] * (e[:, None, 0] * (poly[..., 1] - p0[:, None, 1]) - e[:, None, 1] * (poly[..., 0] - p0[:, None, 0]))
    dn = np.take_along_axis(d, nidx, 1)
    nxt = np.stack([np.take_along_axis(poly[..., k], nidx, 1) for k in (0, 1)], -1)
    inc, inn = d >= 0, dn >= 0
    crossing = valid & (inc != inn)
    with np.errstate(all="ignore"):
        t = np.where(crossing, d / (d - dn), 0.0)
    ip = poly + t[..., None] * (nxt - poly)
    flags = np.stack([valid & inc, crossing], 2).reshape(m, 2 * v)
    pts = np.stack([poly, ip], 2).reshape(m, 2 * v, 2)
    pos = np.cumsum(flags, 1) - 1
    ncnt = flags.sum(1)
    assert ncnt.max(initial=0) <= v
    out = np.zeros_like(poly)
    mi, ki = np.nonzero(flags)
    out[mi, pos[mi, ki]] = pts[mi, ki]
    return out, ncnt


def rect_inter64(a, b):
    """Intersection area of rotated rectangles a, b ([..., 5] float32 rows, broadcast against each other) in float64."""
    a, b = np.broadcast_arrays(_rows(a), _rows(b))
    shape = a.shape[:-1]
    ca, cb = corners64(a.reshape(-1, 5)), corners64(b.reshape(-1, 5))
    m = ca.shape[0]
    org = ca[:, :1].copy()                       # work relative to a corner of a: float64 cancellation stays ~1e-16 of the box size
    ca, cb = ca - org, cb - org
    poly = np.zeros((m, 10, 2))
    poly[:, :4] = ca
    cnt = np.full(m, 4)
    sgn = np.sign(_shoelace(cb, np.full(m, 4)))
    for k in range(4):
        poly, cnt = _clip_halfplane(poly, cnt, cb[:, k], cb[:, (k + 1) % 4] - cb[:, k], sgn)
    area = np.abs(_shoelace(poly, cnt))
    finite = np.isfinite(ca).all((1, 2)) & np.isfinite(cb).all((1, 2))
    return np.where(finite, area, np.nan).reshape(shape)


def _areas(a, b):
    a, b = _rows(a), _rows(b)
    return a[..., 2] * a[..., 3], b[..., 2] * b[..., 3]


def iou64(a, b, criterion=-1, inter=None):
    inter = rect_inter64(a, b) if inter is None else inter
    aa, ab = _areas(a, b)
    with np.errstate(all="ignore"):
        if criterion == -1:
            return inter / (aa + ab - inter)
        if criterion == 0:
            return inter / ab
        if criterion == 1:
            return inter / aa
    assert criterion == 2
    return inter


def iou_matrix64(boxes, qboxes, criterion=-1):
    """[N, K] like ops.rotate_iou(boxes, qboxes, criterion)."""
    return iou64(np.asarray(boxes)[:, None, :5], np.asarray(qboxes)[None, :, :5], criterion)


def _point_segment(p, s0, s1):
    """distance of points p [..., 2] to segments s0-s1 [..., 2]."""
    d = s1 - s0
    dd = (d * d).sum(-1)
    with np.errstate(all="ignore"):
        t = np.clip(np.where(dd > 0, ((p - s0) * d).sum(-1) / dd, 0.0), 0.0, 1.0)
    q = s0 + t[..., None] * d
    return np.sqrt(((p - q) ** 2).sum(-1))


def corner_edge_distance(a, b):
    """smallest distance between a corner of one rectangle and an edge segment of the other (the distance of disjoint rectangles)."""
    a, b = np.broadcast_arrays(_rows(a), _rows(b))
    ca, cb = corners64(a), corners64(b)

    def one(c, q):       # corners c [..., 4, 2] against the segments of q
        s0, s1 = q[..., None, :, :], np.roll(q, -1, -2)[..., None, :, :]
        return _point_segment(c[..., :, None, :], s0, s1).min((-1, -2))
    return np.minimum(one(ca, cb), one(cb, ca))


def general_position(a, b, eta=ETA):
    with np.errstate(all="ignore"):
        return corner_edge_distance(a, b) >= eta


def standup64(b):
    c = corners64(b)
    return np.concatenate([c.min(-2), c.max(-2)], -1)           # x0, y0, x1, y1


def standup_overlap64(a, b):
    """min(iw, ih) of the two standup boxes: > 0 exactly when their eps-0 IoU is > 0 (nms_cpu.py:25); -(the gap) when negative."""
    sa, sb = standup64(a), standup64(b)
    iw = np.minimum(sa[..., 2], sb[..., 2]) - np.maximum(sa[..., 0], sb[..., 0])
    ih = np.minimum(sa[..., 3], sb[..., 3]) - np.maximum(sa[..., 1], sb[..., 1])
    return np.minimum(iw, ih)


def _delta(a, b):
    a, b = np.broadcast_arrays(_rows(a), _rows(b))
    both = np.stack([a, b], 0)
    return 2.0 ** -23 * (np.abs(both[..., :2]).max((0, -1)) + np.abs(both[..., 2:4]).max((0, -1)))


def delta_perimeter(a, b):
    a, b = np.broadcast_arrays(_rows(a), _rows(b))
    per = np.minimum(2 * (np.abs(a[..., 2]) + np.abs(a[..., 3])), 2 * (np.abs(b[..., 2]) + np.abs(b[..., 3])))
    return _delta(a, b) * per


def inter_bound(a, b, c=C):
    return c * delta_perimeter(a, b)


def iou_bound(a, b, criterion=-1, inter=None, c=C):
    """bound of |fp32 result - iou64| for a general-position pair (module docstring)."""
    inter = rect_inter64(a, b) if inter is None else inter
    e = inter_bound(a, b, c)
    aa, ab = _areas(a, b)
    with np.errstate(all="ignore"):
        if criterion == 2:
            return e
        if criterion in (0, 1):
            area = ab if criterion == 0 else aa
            return e / area + 3 * U24 * inter / area
        u = aa + ab - inter
        v = inter / u
        lo = np.maximum(inter - e, 0.0) / (u + e + 5 * U24 * u)
        den = u - e - 5 * U24 * u
        hi = np.where(den > 0, (inter + e) / den, np.inf)
        return np.maximum(hi - v, v - lo) + 2 * U24 * v


def aa_iou64(a, b, eps):
    a, b = _rows(a, 4), _rows(b, 4)
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + eps, 0.0)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + eps, 0.0)
    inter = w * h
    sa = (a[..., 2] - a[..., 0] + eps) * (a[..., 3] - a[..., 1] + eps)
    sb = (b[..., 2] - b[..., 0] + eps) * (b[..., 3] - b[..., 1] + eps)
    with np.errstate(all="ignore"):
        return inter / (sa + sb - inter)


def aa_bound(a, b, eps):
    """fp32 evaluation of aa_iou64: every length is a difference of float32 inputs plus eps -- two roundings relative to the larger
    operand, dl = 2 u (max |coordinate| + eps); a product of two lengths p, q then errs by dl (p + q) + dl^2 + u p q.  With e_i for the
    intersection and e_a, e_b for the two areas the quotient lies in [(I - e_i) / (U + E), (I + e_i) / (U - E)],
    E = e_i + e_a + e_b + 3 u (sa + sb), widened by its own rounding."""
    a, b = _rows(a, 4), _rows(b, 4)
    dl = 2 * U24 * (np.maximum(np.abs(a).max(-1), np.abs(b).max(-1)) + abs(eps))

    def prod_err(p, q):
        return dl * (np.abs(p) + np.abs(q)) + dl * dl + U24 * np.abs(p * q)
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + eps, 0.0)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + eps, 0.0)
    wa, ha = a[..., 2] - a[..., 0] + eps, a[..., 3] - a[..., 1] + eps
    wb, hb = b[..., 2] - b[..., 0] + eps, b[..., 3] - b[..., 1] + eps
    inter, sa, sb = w * h, wa * ha, wb * hb
    e_i = prod_err(w, h)
    big = e_i + prod_err(wa, ha) + prod_err(wb, hb) + 3 * U24 * (np.abs(sa) + np.abs(sb))
    u = sa + sb - inter
    with np.errstate(all="ignore"):
        v = inter / u
        hi = np.where(u - big > 0, (inter + e_i) / (u - big), np.inf)
        lo = np.maximum(inter - e_i, 0.0) / (u + big)
        return np.maximum(hi - v, v - lo) + 2 * U24 * v


# ---------------------------------------------------------------------------------------------------------------- greedy NMS
def rotate_iou_fn(a, b):
    """iou_fn of the rotated kind: (IoU, bound, comparable) of row a against rows b.  A pair with an exactly empty float64
    intersection in general position has IoU exactly 0 in fp32 too: its bound is 0."""
    inter = rect_inter64(a, b)
    iou = iou64(a, b, -1, inter)
    gp = general_position(a, b)
    bound = np.where(inter == 0.0, 0.0, iou_bound(a, b, -1, inter))
    return iou, bound, gp


def aa_iou_fn(eps):
    def fn(a, b):
        iou = aa_iou64(a, b, eps)
        return iou, aa_bound(a, b, eps), np.ones(np.shape(iou), bool)
    return fn


def dense_neighbours(n):
    return [np.arange(i + 1, n) for i in range(n)]


def greedy_nms64(boxes, thr, kind="rotate", semantics="numba", eps=1.0, post_max=0, iou_fn=None, neighbours=None, info=None):
    """Sequential greedy NMS of score-sorted rows in float64.

    A dead box suppresses nothing; the cap is counted while keeping (the loop stops at post_max kept boxes, post_max <= 0: no cap);
    numba semantics suppress at IoU > thr (axis-aligned: the +1 convention whatever ``eps``), cpu semantics at IoU >= thr (rotated:
    pairs whose standup IoU at eps 0 is not > 0 are skipped first).  ``neighbours[i]``: ascending positions j > i that may overlap box
    i -- every other pair is known by construction to be disjoint AND standup-disjoint (IoU exactly 0, never suppressed at thr >= 0
    except by the axis-aligned cpu rule at thr = 0, which needs the dense list).  Returns (keep, band): band = the smallest
    |IoU - thr| over the consulted pairs (inf when none).  ``info`` (a dict) receives ratio = the smallest |IoU - thr| / bound,
    standup = the smallest |min(iw, ih)| / (8 delta) over the pre-filter's decisions, comparable = all consulted pairs are in
    general position, consulted = their number."""
    boxes = np.asarray(boxes, np.float32)
    n = boxes.shape[0]
    rot = kind == "rotate"
    cpu = semantics == "cpu"
    if iou_fn is None:
        iou_fn = rotate_iou_fn if rot else aa_iou_fn(eps if cpu else 1.0)
    if neighbours is None:
        neighbours = dense_neighbours(n)
    else:
        assert thr > 0 or (thr == 0 and (rot or not cpu)), "a sparse neighbour list presumes that IoU 0 never suppresses"
    dead = np.zeros(n, bool)
    keep = []
    band, ratio, su_ratio, comparable, consulted = np.inf, np.inf, np.inf, True, 0
    # all candidate pairs in one vectorised evaluation, then the loop only looks them up
    rows = np.concatenate([np.full(len(nb), i) for i, nb in enumerate(neighbours)] or [np.zeros(0, int)]).astype(int)
    cols = np.concatenate([np.asarray(nb, int) for nb in neighbours] or [np.zeros(0, int)]).astype(int)
    start = np.concatenate([[0], np.cumsum([len(nb) for nb in neighbours])]).astype(int)
    if rows.size:
        assert (cols > rows).all() and cols.max() < n
        iou, bound, gp = iou_fn(boxes[rows], boxes[cols])
        su = standup_overlap64(boxes[rows], boxes[cols]) if (rot and cpu) else None
        su_unit = 8 * _delta(boxes[rows], boxes[cols]) if (rot and cpu) else None
    for i in range(n):
        if dead[i]:
            continue
        if post_max > 0 and len(keep) >= post_max:
            break
        keep.append(i)
        s = slice(start[i], start[i + 1])
        if s.start == s.stop:
            continue
        j = cols[s]
        live = ~dead[j]
        if rot and cpu:
            with np.errstate(all="ignore"):
                su_ratio = min(su_ratio, np.min(np.abs(su[s][live]) / su_unit[s][live], initial=np.inf))
            live = live & (su[s] > 0)
        v, bd = iou[s][live], bound[s][live]
        if v.size == 0:
            continue
        consulted += v.size
        comparable = comparable and bool(gp[s][live].all())
        with np.errstate(all="ignore"):
            dist = np.abs(v - thr)
            band = min(band, np.nanmin(dist, initial=np.inf))
            ratio = min(ratio, np.nanmin(np.where((bd == 0) & (dist == 0), np.inf, dist / bd), initial=np.inf))
            hit = (v >= thr) if cpu else (v > thr)
        dead[j[live][hit]] = True
    if info is not None:
        info.update(ratio=ratio, standup=su_ratio, comparable=comparable, consulted=consulted)
    return np.asarray(keep, np.int32), band


def check_keep(keep, num_keep, want):
    """The comparison of the GPU tests: keep [B, max_n] / num_keep [B] of ops.nms_sorted against a list of reference keep lists.
    num_keep exact, rows [0, num_keep) equal and ascending."""
    keep, num_keep = np.asarray(keep), np.asarray(num_keep)
    assert len(want) == num_keep.shape[0]
    for f, w in enumerate(want):
        k = int(num_keep[f])
        assert k == len(w), f"frame {f}: num_keep {k}, reference keeps {len(w)}"
        got = keep[f, :k]
        assert (np.diff(got) > 0).all(), f"frame {f}: keep is not ascending"
        assert np.array_equal(got, w), f"frame {f}: first difference at {int(np.argmax(got != np.asarray(w)))}"


def check_iou_matrix(got, boxes, qboxes, criterion, c=C):
    """The comparison of the GPU IoU-matrix test.  Returns the largest |got - iou64| / bound over the general-position pairs."""
    got = np.asarray(got, np.float64)
    b, q = np.asarray(boxes)[:, None, :5], np.asarray(qboxes)[None, :, :5]
    inter = rect_inter64(b, q)
    ref = iou64(b, q, criterion, inter)
    bound = iou_bound(b, q, criterion, inter, c)
    gp = general_position(b, q)
    assert np.isfinite(bound[gp]).all()
    err = np.abs(got - ref)
    ratio = float((err[gp] / bound[gp]).max(initial=0.0))
    assert ratio <= 1.0, f"criterion {criterion}: |device - float64| is {ratio:.3g} x the bound"
    far = (inter == 0.0) & (-standup_overlap64(b, q) > FAR_GAP)
    assert (got[far] == 0.0).all(), "a far-apart pair is not exactly 0"
    return ratio


# ---------------------------------------------------------------------------------------------------------------- IoU-matrix inputs
_IOU_GEN = {
    # objects' spread, centre jitter, (w range), (l = w * aspect range or l range), rotation jitter
    "car": dict(jit=0.9, w=(1.5, 1.9), l=(3.4, 4.6), aspect=None, rj=0.25, extent=(70.0, 40.0)),
    "long": dict(jit=2.0, w=(0.5, 1.0), l=None, aspect=(10.0, 10.0), rj=0.4, extent=(70.0, 40.0)),
    "small": dict(jit=0.12, w=(0.05, 0.3), l=(0.05, 0.3), aspect=None, rj=0.5, extent=(4.0, 3.0)),
}


def _cluster(rng, gen, n, n_obj, extent=None):
    g = _IOU_GEN[gen]
    extent = extent or g["extent"]
    cx, cy = rng.uniform(0, extent[0], n_obj), rng.uniform(-extent[1], extent[1], n_obj)
    rot = rng.uniform(-3.2, 3.2, n_obj)
    o = rng.integers(0, n_obj, n)
    w = rng.uniform(*g["w"], n)
    l = rng.uniform(*g["l"], n) if g["aspect"] is None else w * rng.uniform(*g["aspect"], n)
    r = rot[o] + rng.normal(0, g["rj"], n) + (rng.random(n) < 0.1) * np.pi / 2
    return np.stack([cx[o] + rng.normal(0, g["jit"], n), cy[o] + rng.normal(0, g["jit"], n), w, l, r], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def iou_matrix_input(gen, n, k):
    """(boxes [n, 5], qboxes [k, 5]) drawn from the same objects, so a fair share of the pairs overlap (4 to 13 %); the last query box is a
    copy of the last box at r = 0 (a duplicate: exactly 1 for criteria -1, 0, 1), except for the single pair of (1, 1)."""
    rng = np.random.default_rng(1000 * IOU_GENERATORS.index(gen) + 7 * n + k)
    both = _cluster(rng, gen, n + k, 1 + (n + k) // 12)
    boxes, q = both[:n].copy(), both[n:].copy()
    if n * k >= 64:
        # on a dyadic grid (centre in 1 / 64, sides in 1 / 32) at r = 0: corners, triangle areas and w l are exact in float32
        boxes[-1, :2] = np.round(boxes[-1, :2] * 64) / 64
        boxes[-1, 2:4] = np.maximum(np.round(boxes[-1, 2:4] * 32), 2) / 32
        boxes[-1, 4] = 0.0
        q[-1] = boxes[-1]
    else:                                        # the single pair overlaps, turned and shifted by a fraction of its sides
        q[0] = boxes[0] + np.array([0.3 * boxes[0, 2], 0.2 * boxes[0, 3], 0, 0, 0.3], np.float32)
    boxes.setflags(write=False)
    q.setflags(write=False)
    return boxes, q


def iou_matrix_cases():
    return [(g, n, k) for g in IOU_GENERATORS for n, k in IOU_SHAPES]


# ---------------------------------------------------------------------------------------------------------------- exact-threshold pairs
# rotated (x, y, w, l, r) at r = 0 on a dyadic grid: corners, intersection, union and quotient are exact in float32
EXACT_ROTATED = {
    0.25: [([0, 0, 2, 2.5, 0], [1, 0.5, 2, 2.5, 0]),          # 1 x 2 = 2 of 5 + 5 - 2 = 8
           ([0, 0, 5, 4, 0], [1, 2, 5, 4, 0])],               # 4 x 2 = 8 of 20 + 20 - 8 = 32
    0.5: [([0, 0, 9, 8, 0], [1, 2, 9, 8, 0]),                 # 8 x 6 = 48 of 72 + 72 - 48 = 96
          ([0, 0, 6, 6, 0], [0.5, 0.25, 4, 4.5, 0])],         # 4 x 4.5 = 18 strictly inside 36: 18 of 36
}
# axis-aligned integer (x1, y1, x2, y2): `plus1` rows hit the threshold under the +1 convention, `eps0` rows at eps = 0
EXACT_AA = {
    ("plus1", 0.5): ([0, 0, 8, 7], [1, 2, 9, 9]), ("plus1", 0.25): ([0, 0, 4, 3], [1, 2, 5, 5]),
    ("eps0", 0.5): ([0, 0, 9, 8], [1, 2, 10, 10]), ("eps0", 0.25): ([0, 0, 5, 4], [1, 2, 6, 6]),
}


def exact_pair_frames(kind, pair, n, shift=(0.0, 0.0)):
    """One frame of n boxes per TILE_POSITIONS entry: the pair at (row, col), every other box far away from everything.
    -> (dets [7, n, 5 or 4] float32, cols [7])."""
    a, b = (np.asarray(p, np.float32) for p in pair)
    width = 5 if kind == "rotate" else 4
    frames, cols = [], []
    for row, col in TILE_POSITIONS:
        row, col = row % n, col % n
        d = np.zeros((n, width), np.float32)
        i = np.arange(n, dtype=np.float32)
        if kind == "rotate":
            d[:, 0], d[:, 1], d[:, 2], d[:, 3] = 1024 + 64 * (i % 16), 1024 + 64 * (i // 16), 2, 2
        else:
            d[:, 0], d[:, 1] = 1024 + 64 * (i % 16), 1024 + 64 * (i // 16)
            d[:, 2], d[:, 3] = d[:, 0] + 2, d[:, 1] + 2
        d[row], d[col] = a, b
        if kind == "rotate":
            d[[row, col], 0] += shift[0]
            d[[row, col], 1] += shift[1]
        else:
            d[[row, col]] += np.asarray([shift[0], shift[1], shift[0], shift[1]], np.float32)
        frames.append(d)
        cols.append(col)
    return np.stack(frames), np.asarray(cols)


# ---------------------------------------------------------------------------------------------------------------- two-box frames
_PAIR_GEN = {
    "square": dict(w=(0.6, 2.6), l=(0.6, 2.6), centre=20.0),
    "car": dict(w=(1.5, 1.9), l=(3.4, 4.6), centre=40.0),
    "long": dict(w=(0.5, 1.0), l=10.0, centre=40.0),
    "small": dict(w=(0.05, 0.05), l=(0.05, 0.05), centre=5.0),
    "far": dict(w=(1.4, 2.0), l=(3.0, 5.0), centre=(69.0, 71.0)),
}
FAR_PAIR = np.array([[0, 0, 2, 2, 0.3], [50, 50, 2, 2, 0.1]], np.float32)


def _pair_candidates(rng, shape, m):
    g = _PAIR_GEN[shape]

    def sides(k):
        w = rng.uniform(*g["w"], k)
        l = w * g["l"] if np.isscalar(g["l"]) else rng.uniform(*g["l"], k)
        return w, l
    wa, la = sides(m)
    wb, lb = sides(m)
    same = rng.random(m) < 0.5                       # half of the partners have nearly the first box's size (IoU up to 0.98)
    wb = np.where(same, wa * rng.uniform(0.99, 1.01, m), wb)
    lb = np.where(same, la * rng.uniform(0.99, 1.01, m), lb)
    if np.isscalar(g["centre"]):
        xa, ya = rng.uniform(-g["centre"], g["centre"], m), rng.uniform(-g["centre"], g["centre"], m)
    else:
        sx, sy = rng.choice([-1.0, 1.0], m), rng.choice([-1.0, 1.0], m)
        xa, ya = sx * rng.uniform(*g["centre"], m), sy * rng.uniform(*g["centre"], m)
    ra = rng.uniform(-3.2, 3.2, m)
    # offsets from a hair to beyond the box, rotations from parallel to anything
    reach = 0.5 * np.hypot(wa, la) * 2.2
    dist = reach * rng.random(m) ** rng.choice([0.5, 1.0, 3.0], m)
    phi = rng.uniform(0, 2 * np.pi, m)
    dr = rng.normal(0, 1, m) * rng.choice([0.02, 0.2, 1.5], m)
    a = np.stack([xa, ya, wa, la, ra], 1)
    b = np.stack([xa + dist * np.cos(phi), ya + dist * np.sin(phi), wb, lb, ra + dr], 1)
    return np.stack([a, b], 1).astype(np.float32)


def pair_comparable(dets, thr, cpu):
    """[M, 2, 5] -> mask of the pairs whose decision float64 may judge: general position, |IoU - thr| beyond the bound (or an exactly
    empty intersection), and for the cpu pre-filter a standup overlap / gap beyond 8 delta."""
    a, b = dets[:, 0], dets[:, 1]
    iou, bound, gp = rotate_iou_fn(a, b)
    with np.errstate(all="ignore"):
        ok = gp & (np.abs(iou - thr) > bound) | (gp & (bound == 0))
        if cpu:
            ok &= np.abs(standup_overlap64(a, b)) > 8 * _delta(a, b)
    return ok & np.isfinite(iou)


@functools.lru_cache(maxsize=None)
def decision_pairs(shape, thr):
    """PAIR_FRAMES two-box frames for threshold ``thr``: float64 IoU from 0 to 0.98, a third of them within [0.8 thr, 1.15 thr + 2e-4]
    (the upper part is where the inscribed-circle screen's margin 1.02 thr + 1e-4 decides), band-filtered for both semantics; a
    filtered frame is replaced by FAR_PAIR.  -> (dets [4096, 2, 5] float32 read-only, share filtered away)."""
    rng = np.random.default_rng(100 * PAIR_SHAPES.index(shape) + int(round(thr * 1000)))
    cand = _pair_candidates(rng, shape, 40000)
    iou = iou64(cand[:, 0], cand[:, 1])
    # General position is a property of the distribution the pairs are drawn from, not of the threshold: a candidate with a corner
    # within ETA of the other box's edge is redrawn (dropped from the pool) -- 0.5 to 1.4 % of the candidates of four shapes and 19 % of the
    # side-0.05 ones (24 % of the overlapping ones), where ETA is 2 % of a side.  What is filtered below, and counted, is the decision band.
    ok = np.isfinite(iou) & (iou <= 0.98) & general_position(cand[:, 0], cand[:, 1])
    cand, iou = cand[ok], iou[ok]
    near = np.nonzero((iou >= 0.8 * thr) & (iou <= 1.15 * thr + 2e-4) & (iou > 0))[0]
    take_near = near[:PAIR_FRAMES // 3 if thr > 0 else PAIR_FRAMES // 32]      # at thr = 0 that zone is the band itself
    rest = np.setdiff1d(np.arange(len(cand)), take_near)
    # the others: uniform over ten IoU bins (disjoint pairs are a bin of their own)
    bins = np.where(iou[rest] == 0, -1, np.minimum((iou[rest] * 10).astype(int), 9))
    need = PAIR_FRAMES - len(take_near)
    chosen = []
    per = need // 11 + 1
    for bidx in range(-1, 10):
        chosen.append(rest[bins == bidx][:per])
    chosen = np.concatenate(chosen)
    left = np.setdiff1d(rest, chosen)
    sel = np.concatenate([take_near, chosen, left])[:PAIR_FRAMES]
    assert len(sel) == PAIR_FRAMES
    dets = cand[rng.permutation(sel)]
    ok = pair_comparable(dets, thr, False) & pair_comparable(dets, thr, True)
    dets[~ok] = FAR_PAIR
    dets.setflags(write=False)
    return dets, float((~ok).mean())


def pair_decisions64(dets, thr, semantics):
    """num_keep of every two-box frame: 1 when box 1 is suppressed."""
    a, b = dets[:, 0], dets[:, 1]
    iou = iou64(a, b)
    if semantics == "cpu":
        sup = (standup_overlap64(a, b) > 0) & (iou >= thr)
    else:
        sup = iou > thr
    return np.where(sup, 1, 2).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- reduce layouts
# A layout places boxes on SITES 8 m apart (2 x 2 boxes: different sites are disjoint under every convention used); boxes of one
# site overlap each other by construction (offsets of 0.05 .. 0.43 in x and y: IoU >= 0.44, corners >= 0.02 from every edge), so the
# first box of a site suppresses the others and the neighbour lists are the within-site pairs.
SITE_THR = 0.2
_OFFS = np.array([(0.05 + 0.02 * (k % 20), 0.05 + 0.02 * (k // 20)) for k in range(400)])


def _site_boxes(kind, site_of, slot_of):
    n = len(site_of)
    sx, sy = 8.0 * (site_of % 64) - 252.0, 8.0 * (site_of // 64) - 252.0
    x, y = sx + _OFFS[slot_of, 0], sy + _OFFS[slot_of, 1]
    if kind == "rotate":
        return np.stack([x, y, np.full(n, 2.0), np.full(n, 2.0), np.full(n, 0.2)], 1).astype(np.float32)
    return np.stack([x - 1, y - 1, x + 1, y + 1], 1).astype(np.float32)


def _site_layout(kind, n, victim_of):
    """victim_of: {column: row it shares a site with (row < column)}.  -> (dets, neighbours, keep by construction)."""
    site_of, slot_of = np.zeros(n, int), np.zeros(n, int)
    members = {}
    for i in range(n):
        root = i
        if i in victim_of:
            assert victim_of[i] < i
            root = site_of[victim_of[i]]             # sites are numbered by their first box
        site_of[i] = root
        members.setdefault(root, []).append(i)
        slot_of[i] = len(members[root]) - 1
    assert slot_of.max(initial=0) < len(_OFFS)
    neighbours = [np.zeros(0, int)] * n
    for mem in members.values():
        for q, i in enumerate(mem):
            neighbours[i] = np.asarray(mem[q + 1:], int)
    keep = np.asarray(sorted(members), np.int32)
    return _site_boxes(kind, site_of, slot_of), neighbours, keep


def _chain_layout(kind, n):
    """box i overlaps only box i + 1 (the dense reference agrees; the neighbour list also names i + 2, which touches under +1)."""
    step = 1.1 if kind == "rotate" else 1.5
    x = step * (np.arange(n) - n // 2)
    if kind == "rotate":
        d = np.stack([x, np.zeros(n), np.full(n, 2.0), np.full(n, 2.0), np.full(n, 0.05)], 1)
    else:
        d = np.stack([x - 1, np.full(n, -1.0), x + 1, np.full(n, 1.0)], 1)
    nb = [np.arange(i + 1, min(i + 3, n)) for i in range(n)]
    return d.astype(np.float32), nb, np.arange(0, n, 2, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reduce_layout(name, kind, n=None):
    """-> (dets [n, 5 or 4] read-only, neighbours, keep by construction at SITE_THR without a cap)."""
    if name == "chain":
        out = _chain_layout(kind, n)
    elif name == "mixed":
        # each box joins the site of a random earlier box with probability 0.3
        rng = np.random.default_rng(n)
        v = {j: int(rng.integers(0, j)) for j in range(1, n) if rng.random() < 0.3}
        out = _site_layout(kind, n, v)
    elif name == "far":
        # kept rows of block 0 and of block 62 suppress columns of block 63 (words 62 / 63 of a 64-word row), n = 4096
        assert n == 4096
        b62, b63 = 62 * 64, 63 * 64
        out = _site_layout(kind, n, {b63: 3, b63 + 17: 40, b63 + 62: b62 + 5, b63 + 63: b62 + 63, b63 + 1: 63, b62 + 1: 0})
    elif name == "merge":
        # blocks 1..6 keep exactly 1, 2, 3, 4, 5 and 9 rows (their other boxes share the site of a kept row of block 0 and are dead,
        # six sites of at most 63 dead boxes); every kept row suppresses a distinct column of block 7.  n = 512.
        assert n in (None, 512)
        n, v, col = 512, {}, 7 * 64
        for blk, k in zip(range(1, 7), (1, 2, 3, 4, 5, 9)):
            lanes = [0, 63, 31, 7, 40, 1, 62, 16, 50][:k]
            for lane in range(64):
                j = blk * 64 + lane
                if lane in lanes:
                    v[col] = j
                    col += 2
                else:
                    v[j] = blk - 1                       # the dead boxes of block blk sit on box blk - 1 of block 0
        out = _site_layout(kind, n, v)
    else:
        raise KeyError(name)
    out[0].setflags(write=False)
    return out


RAGGED_COUNTS = (4096, 0, 4095, 1, 2, 63, 64, 65, 128, 129, 0, 4096)


def ragged_batch(kind):
    """[B, 4096, width] and counts: frame f holds the `mixed` layout of RAGGED_COUNTS[f] boxes; a count-0 frame sits between full ones."""
    width = 5 if kind == "rotate" else 4
    buf = np.zeros((len(RAGGED_COUNTS), 4096, width), np.float32)
    for f, c in enumerate(RAGGED_COUNTS):
        if c:
            buf[f, :c] = reduce_layout("mixed", kind, c)[0]
    return buf, np.asarray(RAGGED_COUNTS, np.int32)


# ---------------------------------------------------------------------------------------------------------------- special values
def special_frame(kind):
    """Ordinary clustered boxes with non-finite / negative-sided rows among them (the reference's rule: comparisons with NaN are false).
    The expected keep list is the fp32 oracle's.  Zero sides are in degenerate_frame(): against a ROTATED box their IoU is
    area / (area - intersection) with intersection = area up to rounding, a sign the libm decides."""
    rng = np.random.default_rng(77)
    nan, inf = np.nan, np.inf
    if kind == "rotate":
        d = _cluster(rng, "car", 90, 6, extent=(30.0, 20.0))
        sp = {3: (0, nan), 10: (1, nan), 17: (4, nan), 20: (2, nan), 26: (3, nan), 41: (2, -1.7), 47: (3, -4.0),
              52: (0, inf), 58: (1, -inf), 59: (0, inf), 63: (4, inf), 64: (2, nan), 70: (2, inf)}
        for row, (col, val) in sp.items():
            d[row, col] = val
        # a non-finite rotation / side on top of an ordinary box
        d[5] = d[4]; d[5, 4] = nan
        d[66] = d[65]; d[66, 4] = inf
        d[12] = d[11]; d[12, 2] = nan
        return d
    xy = rng.uniform(0, 40, (90, 2))
    wh = rng.uniform(2, 15, (90, 2))
    d = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    for row, (col, val) in {3: (0, nan), 10: (3, nan), 17: (2, inf), 20: (1, -inf), 33: (2, -5.0), 64: (0, nan), 65: (1, inf)}.items():
        d[row, col] = val
    d[41, 2:] = d[41, :2]                       # zero width and height
    d[50, 2:] = d[50, :2] - 3                   # negative sides
    return d


# ---------------------------------------------------------------------------------------------------------------- the reduce cases
REDUCE_CASES = ("ragged", "clamp", "chain", "far", "merge", "post1", "post_block0", "post64", "post65", "post_n1")


def _frames_case(kind, frames, post_max=0, counts=None, max_n=None):
    """frames: list of (dets, neighbours, keep) layouts (None: an empty frame)."""
    width = 5 if kind == "rotate" else 4
    max_n = max_n or max(1, max(len(f[0]) for f in frames if f is not None))
    buf = np.zeros((len(frames), max_n, width), np.float32)
    for i, f in enumerate(frames):
        if f is not None:
            buf[i, :len(f[0])] = f[0]
    real = np.asarray([0 if f is None else len(f[0]) for f in frames], np.int32)
    return dict(kind=kind, dets=buf, counts=real if counts is None else np.asarray(counts, np.int32), sizes=real, post_max=post_max,
                neighbours=[None if f is None else f[1] for f in frames], built=[np.zeros(0, np.int32) if f is None else f[2] for f in frames],
                thr=SITE_THR)


@functools.lru_cache(maxsize=None)
def reduce_case(name, kind):
    """The inputs of the reduce-edge GPU tests: dict(kind, dets [B, max_n, width], counts [B], sizes [B] (the boxes really there),
    post_max, neighbours (per frame), built (keep by construction, no cap), thr)."""
    lay = functools.partial(reduce_layout, kind=kind)
    if name == "ragged":
        return _frames_case(kind, [lay("mixed", n=c) if c else None for c in RAGGED_COUNTS], max_n=4096)
    if name == "clamp":                              # counts = max_n + 7: the result at max_n (the rows behind it are the next frame's)
        return _frames_case(kind, [lay("mixed", n=130), lay("chain", n=130)], counts=[137, 137])
    if name == "chain":
        return _frames_case(kind, [lay("chain", n=4096), lay("chain", n=129)])
    if name == "far":
        return _frames_case(kind, [lay("far", n=4096)])
    if name == "merge":
        return _frames_case(kind, [lay("merge", n=512)])
    frames = [lay("mixed", n=200), lay("chain", n=200), lay("mixed", n=65)]
    block0 = int((frames[0][2] < 64).sum())
    assert 1 < block0 < 64
    post = {"post1": 1, "post_block0": block0, "post64": 64, "post65": 65, "post_n1": 201}[name]
    return _frames_case(kind, frames, post_max=post)


def reduce_reference(case, semantics, info=None):
    """greedy_nms64 of every frame of a reduce case (eps = 1 for the axis-aligned kind: the layouts are built for it)."""
    keeps, worst = [], dict(ratio=np.inf, standup=np.inf, comparable=True, consulted=0, band=np.inf)
    max_n = case["dets"].shape[1]
    for f, nb in enumerate(case["neighbours"]):
        n = min(int(case["counts"][f]), max_n)
        assert n == case["sizes"][f] or case["counts"][f] > max_n
        one = {}
        keep, band = greedy_nms64(case["dets"][f, :n], case["thr"], case["kind"], semantics, 1.0, case["post_max"], neighbours=nb, info=one)
        keeps.append(keep)
        worst.update(ratio=min(worst["ratio"], one["ratio"]), standup=min(worst["standup"], one["standup"]), band=min(worst["band"], band),
                     comparable=worst["comparable"] and one["comparable"], consulted=worst["consulted"] + one["consulted"])
    if info is not None:
        info.update(worst)
    return keeps


def degenerate_frame():
    """Zero-area and zero-width boxes among ordinary ones, everything at r = 0 on a dyadic grid, so that the reference's arithmetic is
    exact and its answer does not depend on the libm: the point-in-quad test of a box with a zero side accepts every point of the
    strip its other side spans (of the plane, for a 0 x 0 box), the far box's own corners become the intersection and
    IoU = area / (0 + area - area) = +inf -- the reference suppresses boxes metres away, in either order.  [n, 5] float32."""
    rows = []
    for i in range(4):
        for j in range(3):
            rows.append([8.0 * i, 8.0 * j, 2.0, 4.0, 0.0])
            if (i + j) % 2 == 0:
                rows.append([8.0 * i + 0.5, 8.0 * j + 1.0, 2.0, 4.0, 0.0])
    zero = [[100.0, 100.0, 0.0, 0.0, 0.0], [0.25, 0.5, 0.0, 0.0, 0.0], [-40.0, 0.5, 0.0, 4.0, 0.0], [8.5, 64.0, 2.0, 0.0, 0.0],
            [16.0, 8.0, 0.0, 1.0, 0.0], [100.0, 100.0, 0.0, 0.0, 0.0]]
    d = np.asarray(rows + zero, np.float32)
    order = np.random.default_rng(3).permutation(len(d))
    return d[order]
