"""Produces tests/golden/distance_similarity.npz by EXECUTING the reference on CPU: DistanceSimilarity.compare
(second/core/region_similarity.py:96-122 -> box_np_ops.distance_similarity :950-973) and TargetAssigner.assign (assign_per_class and
assign_all -> create_target_np) with a DistanceSimilarity on some anchor generators.  Build container only (needs the reference
checkout):

    python tests/golden/make_golden_distance_sim.py [path to the reference checkout]

numba is stubbed by make_golden.install_shims: distance_similarity runs as plain Python on numpy float32 scalars, where Python floats
are weak -- the whole chain is float32 with float32(dist_norm) ("float32" meaning of tests/distance_sim_helpers.py).  Compiled by
numba, the chain is float64 from the division on ("compiled" meaning, what the kernels implement).  The fixture therefore admits only
frames on which BOTH meanings, and the executed reference, take the same decisions, with room to spare:

  * labels, per-anchor argmax and the forced set identical under the executed reference and both restated meanings;
  * decision_margin >= 64 float32 ulp of 1 for every range of every frame;
  * no |dx| or |dy| within 1e-4 of dist_norm.

Ground truth = jittered anchors; a frame that is not admitted is drawn again (the number of draws is recorded), so 100 % of the
frames in the file are admitted by construction -- this is asserted at the end, nothing is filtered out afterwards.

Setup: feature map [1, 12, 10]; car (nearest IoU, two rotations, 0.6 / 0.45), pedestrian (distance 1.414, one rotation, 0.5 / 0.35),
cyclist (distance 1.0 with rotation, alpha 0.5, two rotations, 0.5 / 0.35).  Modes: per_class; all (assign_all: calculator 0 = nearest
IoU for every range); all_dist (assign_all with the calculators rotated so that calculator 0 is the pedestrian's distance)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

FM = [1, 12, 10]
CLASSES = ["car", "pedestrian", "cyclist"]
SPEC = [dict(sizes=[1.6, 3.9, 1.56], rotations=[0, 1.57], z=-1.0, mt=0.6, ut=0.45, sim=None),
        dict(sizes=[0.6, 0.8, 1.73], rotations=[0], z=-0.6, mt=0.5, ut=0.35,
             sim=dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0)),
        dict(sizes=[0.6, 1.76, 1.73], rotations=[0, 1.57], z=-0.6, mt=0.5, ut=0.35,
             sim=dict(kind="distance", distance_norm=1.0, with_rotation=True, rotation_alpha=0.5))]
RANGE_XY = (-4.0, -4.8, 4.0, 4.8)
MARGIN = 64 * 2.0 ** -23
WINDOW_GAP = 1e-4
MODES = {"per_class": (True, [0, 1, 2]), "all": (False, [0, 1, 2]), "all_dist": (False, [1, 0, 0])}   # calculator index per generator


def draw_frame(rng, adict, counts, jitter):
    g, names = [], []
    for ci, (c, k) in enumerate(zip(CLASSES, counts)):
        if k == 0:
            continue
        a = adict[c]["anchors"]
        b = a[rng.choice(len(a), k, replace=False)].copy()
        b[:, :2] += rng.normal(0, jitter[ci], (k, 2)).astype(np.float32)
        b[:, 3:6] *= rng.uniform(0.9, 1.15, (k, 3)).astype(np.float32)
        b[:, 6] += rng.normal(0, 0.25, k).astype(np.float32)
        g.append(b); names += [c] * k
    order = rng.permutation(len(names))              # classes interleaved: index within the class != index in the frame
    boxes = np.concatenate(g)[order].astype(np.float32) if g else np.zeros((0, 7), np.float32)
    return boxes, [names[i] for i in order]


def main():
    if len(sys.argv) > 1:
        os.environ["SECOND_REFERENCE"] = sys.argv[1]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden
    make_golden.install_shims()
    if not getattr(np.meshgrid, "_as_list", False):
        _mg = np.meshgrid
        np.meshgrid = lambda *a, **k: list(_mg(*a, **k))
        np.meshgrid._as_list = True
    import distance_sim_helpers as H
    from second.core import region_similarity
    from second.core.anchor_generator import AnchorGeneratorRange
    from second.core.box_coders import GroundBox3dCoder
    from second.core.target_assigner import TargetAssigner

    def calc(sim):
        if sim is None:
            return region_similarity.NearestIouSimilarity()
        return region_similarity.DistanceSimilarity(sim["distance_norm"], sim["with_rotation"], sim["rotation_alpha"])

    gens = [AnchorGeneratorRange([RANGE_XY[0], RANGE_XY[1], sp["z"], RANGE_XY[2], RANGE_XY[3], sp["z"]], sizes=sp["sizes"],
                                 rotations=sp["rotations"], class_name=c, match_threshold=sp["mt"], unmatch_threshold=sp["ut"])
            for c, sp in zip(CLASSES, SPEC)]
    assigners = {}
    for tag, (per_class, pick) in MODES.items():
        assigners[tag] = TargetAssigner(GroundBox3dCoder(), gens, CLASSES, feature_map_sizes=[FM] * 3, positive_fraction=None,
                                        region_similarity_calculators=[calc(SPEC[i]["sim"]) for i in pick], sample_size=512,
                                        assign_per_class=per_class)
    ta = assigners["per_class"]
    ret = ta.generate_anchors(FM)
    anchors = ret["anchors"].reshape(-1, 7)
    adict = ta.generate_anchors_dict(FM)
    begin = np.cumsum([0] + [adict[c]["anchors"].shape[0] for c in CLASSES]).astype(np.int32)
    assert anchors.dtype == np.float32
    mts, uts = [sp["mt"] for sp in SPEC], [sp["ut"] for sp in SPEC]
    out = {"feature_map_size": np.array(FM), "anchors": anchors, "class_anchor_begin": begin, "matched": np.array(mts, np.float32),
           "unmatched": np.array(uts, np.float32), "margin_required": np.float64(MARGIN), "window_gap_required": np.float64(WINDOW_GAP)}
    for ci, sp in enumerate(SPEC):
        s = sp["sim"]
        out[f"sim_{ci}"] = np.array([0, 0, 0, 0] if s is None else [1, s["distance_norm"], float(s["with_rotation"]), s["rotation_alpha"]],
                                    np.float64)
    for tag, (_, pick) in MODES.items():
        out[f"calculators_{tag}"] = np.array(pick, np.int32)

    def run(tag, gt, names, imp):
        gt_classes = np.array([CLASSES.index(n) + 1 for n in names], np.int32)
        r = assigners[tag].assign(anchors, adict, gt, None, gt_classes=gt_classes, gt_names=np.array(names),
                                  matched_thresholds=ret["matched_thresholds"], unmatched_thresholds=ret["unmatched_thresholds"],
                                  importance=imp)
        return gt_classes, r

    def admitted(gt, names, imp):
        """(ok, smallest margin, smallest window gap, executed results per mode)"""
        res, margin, gap = {}, np.inf, np.inf
        for tag, (per_class, pick) in MODES.items():
            gt_classes, r = run(tag, gt, names, imp)
            res[tag] = r
            ids = [1, 2, 3] if per_class else [0, 0, 0]
            sims = [SPEC[i]["sim"] for i in pick]
            refs = {}
            for meaning in ("compiled", "float32"):
                l, t, i, infos = H.assign_ranges_ref(anchors, gt, gt_classes, begin, ids, mts, uts, sims, imp, None, meaning, want_info=True)
                refs[meaning] = (l, infos)
                if not np.array_equal(l, r["labels"]) or not np.array_equal(i, r["importance"]):
                    return False, 0.0, 0.0, res
            for (ia, ib) in zip(refs["compiled"][1], refs["float32"][1]):
                if ia["sim"] is None:
                    continue
                if not (np.array_equal(ia["arg"], ib["arg"]) and np.array_equal(ia["force"], ib["force"])
                        and np.array_equal(ia["pos"], ib["pos"])):
                    return False, 0.0, 0.0, res
            for c, info in enumerate(refs["compiled"][1]):
                if info["sim"] is None:
                    continue
                margin = min(margin, H.decision_margin(info["sim"], info["gmax"], mts[c], uts[c]), H.argmax_margin(info["sim"]))
                s = sims[0] if not per_class else sims[c]
                if s is not None:
                    sel = np.ones(len(gt), bool) if not per_class else gt_classes == c + 1
                    a, q = anchors[begin[c]:begin[c + 1]].astype(np.float64), gt[sel].astype(np.float64)
                    for ax in (0, 1):
                        gap = min(gap, np.abs(np.abs(a[:, None, ax] - q[None, :, ax]) - s["distance_norm"]).min(initial=np.inf))
        return margin >= MARGIN and gap >= WINDOW_GAP, margin, gap, res

    rng = np.random.default_rng(41)
    plans = [dict(counts=(4, 4, 3), jitter=(0.15, 0.25, 0.2)),        # every class, interleaved
             dict(counts=(0, 5, 0), jitter=(0.0, 0.3, 0.0)),          # pedestrians only: the other ranges are background
             dict(counts=(0, 0, 0), jitter=(0.0, 0.0, 0.0)),          # no ground truth at all
             dict(counts=(2, 6, 6), jitter=(0.1, 0.4, 0.3))]          # crowded distance classes
    draws, margins, gaps = [], [], []
    stored = {tag: dict(labels=[], targets=[], importance=[]) for tag in MODES}
    for f, plan in enumerate(plans):
        for n_draw in range(1, 200):
            gt, names = draw_frame(rng, adict, plan["counts"], plan["jitter"])
            imp = rng.uniform(0.5, 1.5, len(gt)).astype(np.float32)
            ok, margin, gap, res = admitted(gt, names, imp)
            if ok:
                break
        else:
            raise AssertionError(f"frame {f}: no admitted draw")
        draws.append(n_draw); margins.append(margin); gaps.append(gap)
        out[f"gt_{f}"], out[f"gt_importance_{f}"] = gt, imp
        out[f"gt_classes_{f}"] = np.array([CLASSES.index(n) + 1 for n in names], np.int32)
        for tag in MODES:
            stored[tag]["labels"].append(res[tag]["labels"]); stored[tag]["targets"].append(res[tag]["bbox_targets"])
            stored[tag]["importance"].append(res[tag]["importance"])
        print("frame", f, "draws", n_draw, "margin", margin, "window gap", gap,
              {tag: [int((res[tag]["labels"] == k).sum()) for k in (-1, 0, 1, 2, 3)] for tag in MODES})
    for tag in MODES:
        lab = np.stack(stored[tag]["labels"])
        tg = np.stack(stored[tag]["targets"]).astype(np.float32)
        imp_all = np.stack(stored[tag]["importance"]).astype(np.float32)
        assert not tg[lab <= 0].any()
        pos = np.argwhere(lab > 0)
        out[f"labels_{tag}"] = lab.astype(np.int8)
        out[f"target_rows_{tag}"] = pos.astype(np.int32)                 # bbox_targets are zero outside the positives
        out[f"target_vals_{tag}"] = tg[pos[:, 0], pos[:, 1]]
        assert (imp_all[lab <= 0] == 1.0).all()
        out[f"importance_pos_{tag}"] = imp_all[pos[:, 0], pos[:, 1]]     # 1 everywhere else
    # ---- DistanceSimilarity.compare itself, on every ground truth of frames 0 and 3 (windows of other classes included)
    for ci in (1, 2):
        s = SPEC[ci]["sim"]
        a = anchors[begin[ci]:begin[ci + 1]]
        for f in (0, 3):
            gt = out[f"gt_{f}"]
            m = calc(s).compare(a[:, [0, 1, 3, 4, 6]], gt[:, [0, 1, 3, 4, 6]])
            assert m.dtype == np.float32
            mine = H.distance_similarity_ref(H.xyr(a), H.xyr(gt), s["distance_norm"], s["with_rotation"], s["rotation_alpha"], "float32")
            assert np.array_equal(m.view(np.uint32), mine.view(np.uint32)), "the float32 restatement is not the executed reference"
            comp = H.distance_similarity_ref(H.xyr(a), H.xyr(gt), s["distance_norm"], s["with_rotation"], s["rotation_alpha"], "compiled")
            bound = H.meanings_bound(H.xyr(a), H.xyr(gt), s["distance_norm"], s["with_rotation"], s["rotation_alpha"])
            err = np.abs(comp.astype(np.float64) - m.astype(np.float64))
            assert (err <= bound).all(), (err - bound).max()
            print("compare class", ci, "frame", f, "non-zero", int((m != 0).sum()), "negative", int((m < 0).sum()),
                  "compiled != float32 in", int((comp != m).sum()), "elements, largest", err.max(), "bound there", bound.flat[err.argmax()])
            out[f"compare_{ci}_{f}"] = m
    out["frames"] = np.int64(len(plans))
    out["admitted"] = np.int64(len(draws))                    # every frame in the file; draws_per_frame says how many were drawn
    out["draws_per_frame"] = np.array(draws, np.int64)
    out["margin_per_frame"] = np.array(margins, np.float64)
    out["window_gap_per_frame"] = np.array(gaps, np.float64)
    assert out["admitted"] == out["frames"]
    path = os.path.join(HERE, "distance_similarity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
