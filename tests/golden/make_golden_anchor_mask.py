"""Produces tests/golden/anchor_mask.npz by EXECUTING the reference on CPU: AnchorGeneratorStride / TargetAssigner.generate_anchors,
box_np_ops.rbbox2d_to_near_bbox, sparse_sum_for_anchors_mask, the two cumsums and fused_get_anchors_area in prep_pointcloud's order
(second/data/preprocess.py:336-357), and TargetAssigner.assign (assign_all and assign_per_class -> create_target_np with
prune_anchor_fn) with the mask.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_anchor_mask.py [path to the reference checkout]

numba is stubbed by make_golden.install_shims (as for every other fixture): the reference's loops run as plain Python on numpy float32
scalars -- the same float32 operations numba compiles; the dtypes of everything that enters the quotients are asserted here.  The
geometry of the cases is tests/anchor_mask_helpers.CASES; the frames are seeded below.  Masks are stored with np.packbits and
coordinates as int16.  Per case the number of anchors whose mask differs when the four quotients are evaluated in float64 is recorded,
and asserted to be above zero for A and C: a device that does not reproduce the float32 order of operations fails those cases."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def blobs(rng, ny, nx, n_blobs, radius, fill):
    """bool [ny, nx]: cells inside a few discs, each kept with probability ``fill``."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    m = np.zeros((ny, nx), bool)
    for _ in range(n_blobs):
        cy, cx, r = rng.integers(0, ny), rng.integers(0, nx), rng.uniform(0.5, 1.0) * radius
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m & (rng.random((ny, nx)) < fill)


def frames_of(name, grid):
    """list of [M, 3] int (z, y, x) voxel coordinates, unique rows, in scrambled order."""
    nx, ny, nz = (int(v) for v in grid)
    rng = np.random.default_rng({"A": 11, "B": 12, "C": 13}[name])
    occ = []
    if name == "A":
        occ = [np.zeros((1, ny, nx), bool), blobs(rng, ny, nx, 3, 9, 0.8)[None], (rng.random((ny, nx)) < 0.2)[None]]
    elif name == "B":
        col = [blobs(rng, ny, nx, 4, 8, 0.9), rng.random((ny, nx)) < 0.15, blobs(rng, ny, nx, 2, 12, 0.6)]
        occ = [c[None] & (rng.random((nz, ny, nx)) < 0.5) for c in col]                   # up to nz voxels per BEV cell
    else:
        occ = [(blobs(rng, ny, nx, 30, 22, 0.22) | (rng.random((ny, nx)) < 0.004))[None] for _ in range(2)]
    out = []
    for o in occ:
        c = np.argwhere(o)
        out.append(c[rng.permutation(len(c))])
    return out


def gt_of(name, case, anchors, begin, masks, rng):
    """Per frame (boxes [G, 7] float32, names): jittered copies of kept anchors of each class, plus -- where the frame has voxels --
    one box over empty ground, whose best-overlapping anchors are all masked out.  0-6 boxes per frame."""
    out = []
    for f in range(case["frames"]):
        kept = np.flatnonzero(masks[f])
        g, names = [], []
        if len(kept):
            for ci, c in enumerate(case["classes"]):
                if name == "B" and f == 1 and ci == 1:
                    continue                                            # one frame with none of the second class
                pool = kept[(kept >= begin[ci]) & (kept < begin[ci + 1])]
                k = min(len(pool), int(rng.integers(1, 4)) if ci == 0 else 2)
                b = anchors[rng.choice(pool, k, replace=False)].copy()
                b[:, :2] += rng.normal(0, 0.12 if ci == 0 else 0.04, (k, 2)).astype(np.float32)
                b[:, 3:6] *= rng.uniform(0.92, 1.1, (k, 3)).astype(np.float32)
                b[:, 6] += rng.normal(0, 0.15, k).astype(np.float32)
                g.append(b); names += [c["name"]] * k
            dropped = np.flatnonzero(~masks[f][:begin[1]])
            if len(dropped):
                b = anchors[rng.choice(dropped, 1)].copy()
                b[:, :2] += rng.normal(0, 0.05, (1, 2)).astype(np.float32)
                g.append(b); names += [case["classes"][0]["name"]]
        boxes = np.concatenate(g).astype(np.float32) if g else np.zeros((0, 7), np.float32)
        order = rng.permutation(len(names))
        assert len(names) <= 6
        out.append((boxes[order], [names[i] for i in order]))
    return out


def main():
    if len(sys.argv) > 1:
        os.environ["SECOND_REFERENCE"] = sys.argv[1]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden
    make_golden.install_shims()
    if not getattr(np.meshgrid, "_as_list", False):        # numpy >= 2 returns a tuple; create_anchors_3d_stride assigns into it
        _mg = np.meshgrid
        np.meshgrid = lambda *a, **k: list(_mg(*a, **k))
        np.meshgrid._as_list = True
    import anchor_mask_helpers as H
    from second.core import box_np_ops, region_similarity
    from second.core.anchor_generator import AnchorGeneratorStride
    from second.core.box_coders import GroundBox3dCoder
    from second.core.target_assigner import TargetAssigner
    out = {}
    for name, case in H.CASES.items():
        vs, pcr, grid = H.geometry(case)
        classes = [c["name"] for c in case["classes"]]
        gens = [AnchorGeneratorStride(sizes=c["sizes"], anchor_strides=c["strides"], anchor_offsets=c["offsets"], rotations=c["rotations"],
                                      class_name=c["name"], match_threshold=c["matched"], unmatch_threshold=c["unmatched"])
                for c in case["classes"]]
        fm = list(case["fm"])

        def assigner(per_class):
            return TargetAssigner(GroundBox3dCoder(), gens, classes, feature_map_sizes=[fm] * len(gens), positive_fraction=None,
                                  region_similarity_calculators=[region_similarity.NearestIouSimilarity() for _ in gens],
                                  sample_size=512, assign_per_class=per_class)
        ta = assigner(True)
        ret = ta.generate_anchors(fm)
        anchors = ret["anchors"].reshape(-1, 7)
        mine, begin = H.anchors_of(case)
        assert anchors.dtype == np.float32 and np.array_equal(anchors, mine), "anchor_mask_helpers.anchors_of is not the reference's generator"
        anchors_bv = box_np_ops.rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]])
        assert anchors_bv.dtype == np.float32 and vs.dtype == np.float32 and pcr.dtype == np.float32
        assert np.array_equal(anchors_bv, H.near_bbox_np(anchors))
        # the device clamps every index on both sides; the reference only c0, c1 from below and c2, c3 from above: they agree when
        # no near box lies wholly outside the map (numpy would wrap a negative index around)
        raw = np.stack([np.floor((anchors_bv[:, i] - pcr[i % 2]) / vs[i % 2]) for i in range(4)], 1)
        assert raw.dtype == np.float32 and (raw[:, 2] >= 0).all() and (raw[:, 3] >= 0).all()
        assert (raw[:, 0] <= grid[0] - 1).all() and (raw[:, 1] <= grid[1] - 1).all()
        frames = frames_of(name, grid)
        masks = {t: [] for t in case["thresholds"]}
        flips = 0
        for f, coors in enumerate(frames):
            assert len(np.unique(coors, axis=0)) == len(coors) and coors.max(initial=0) < 32767
            dense = box_np_ops.sparse_sum_for_anchors_mask(coors, tuple(grid[::-1][1:]))
            dense = dense.cumsum(0)
            dense = dense.cumsum(1)
            assert dense.dtype == np.float32 and dense.max(initial=0) < 2 ** 24
            area = box_np_ops.fused_get_anchors_area(dense, anchors_bv, vs, pcr, grid)
            for t in case["thresholds"]:
                m = area > t
                assert np.array_equal(m, H.anchor_mask_np(coors, anchors, vs, pcr, grid, t)), (name, f, t)
                flips += int((m != H.anchor_mask_np(coors, anchors, vs, pcr, grid, t, dtype=np.float64)).sum())
                masks[t].append(m)
            out[f"{name}_coors_{f}"] = coors.astype(np.int16)
            print(name, "frame", f, "voxels", len(coors), "max count", int(np.diff(np.diff(np.pad(dense, ((1, 0), (1, 0))), axis=0), axis=1).max(initial=0)),
                  "kept", {t: int(masks[t][-1].sum()) for t in case["thresholds"]}, "of", len(anchors))
        for t in case["thresholds"]:
            out[f"{name}_mask_t{t}"] = np.packbits(np.stack(masks[t]), axis=1)
        out[f"{name}_float64_flips"] = np.int64(flips)
        c32 = H.anchor_cells(anchors, vs, pcr, grid)
        c64 = H.anchor_cells(anchors, vs, pcr, grid, dtype=np.float64)
        print(name, "anchors whose mask differs with float64 quotients (summed over frames and thresholds):", flips,
              "| anchors with a different cell index:", int((c32 != c64).any(1).sum()))
        if name in ("A", "C"):
            assert flips > 0, "the fixture would not notice float64 / reciprocal arithmetic"
        if name == "A":
            m1 = masks[1]
            assert not m1[0].any() and m1[1].any() and not m1[1].all()
        if name == "C":
            continue
        # ---- case D: target assignment with the threshold-1 mask
        rng = np.random.default_rng({"A": 21, "B": 22}[name])
        m1 = np.stack(masks[1])
        gts = gt_of(name, case, anchors, begin, m1, rng)
        imps = [rng.uniform(0.5, 1.5, len(g[0])).astype(np.float32) for g in gts]
        out[f"{name}_class_anchor_begin"] = np.array(begin, np.int32)
        for per_class in (True, False):
            ta = assigner(per_class)
            ret = ta.generate_anchors(fm)
            adict = ta.generate_anchors_dict(fm)
            labels, targets, importance = [], [], []
            for f, ((gt, names), imp) in enumerate(zip(gts, imps)):
                gt_classes = np.array([classes.index(n) + 1 for n in names], np.int32)
                r = ta.assign(anchors, adict, gt, m1[f], gt_classes=gt_classes, gt_names=np.array(names),
                              matched_thresholds=ret["matched_thresholds"], unmatched_thresholds=ret["unmatched_thresholds"],
                              importance=imp)
                labels.append(r["labels"]); targets.append(r["bbox_targets"]); importance.append(r["importance"])
                out[f"{name}_gt_{f}"], out[f"{name}_gt_classes_{f}"], out[f"{name}_gt_importance_{f}"] = gt, gt_classes, imp
                # an un-masked run differs: the mask is not a no-op for the assignment
                r0 = ta.assign(anchors, adict, gt, None, gt_classes=gt_classes, gt_names=np.array(names),
                               matched_thresholds=ret["matched_thresholds"], unmatched_thresholds=ret["unmatched_thresholds"],
                               importance=imp)
                inside = m1[f]
                print(name, "per_class" if per_class else "all", "frame", f, "gt", len(gt), "positives", int((r["labels"] > 0).sum()),
                      "dont-care", int((r["labels"] == -1).sum()), "| inside anchors whose label changes without the mask:",
                      int((r["labels"][inside] != r0["labels"][inside]).sum()))
            tag = "per_class" if per_class else "all"
            out[f"{name}_labels_{tag}"] = np.stack(labels).astype(np.int8)
            tg = np.stack(targets).astype(np.float32)
            pos = np.argwhere(np.stack(labels) > 0)
            assert not tg[np.stack(labels) <= 0].any()
            out[f"{name}_target_rows_{tag}"] = pos.astype(np.int32)                # bbox_targets are zero outside the positives
            out[f"{name}_target_vals_{tag}"] = tg[pos[:, 0], pos[:, 1]]
            imp_all = np.stack(importance).astype(np.float32)
            assert np.isin(imp_all[np.stack(labels) <= 0], (0.0, 1.0)).all()
            out[f"{name}_importance_pos_{tag}"] = imp_all[pos[:, 0], pos[:, 1]]     # 1 for the other kept anchors, 0 for masked-out ones
            assert ((imp_all == 0) == ~m1).all() and (np.stack(labels)[~m1] == -1).all()
    path = os.path.join(HERE, "anchor_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
