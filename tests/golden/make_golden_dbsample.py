"""Produces tests/golden/dbsample.npz by EXECUTING the reference's database sampler on CPU: DataBaseSamplerV2.sample_all
(second/core/sample_ops.py, with its DataBasePreprocessor filters and BatchSampler) and box_np_ops.points_in_rbbox, followed by the
concatenations of prep_pointcloud (second/data/preprocess.py:224-249) in that order.  Build container only (needs the reference):

    python tests/golden/make_golden_dbsample.py [path to the reference checkout]

The pools and frames are the seeded float32 inputs of tests/dbsample_helpers.py (CASES, build_pool, build_frame); every pool is
written to a temporary directory as the .bin files its infos name.  Every info is tagged with its row in the filtered pool; the
candidates each BatchSampler.sample call returned and what each sample_class_v2 call accepted are recorded through those tags.
The frames of a case pass through one sampler in order; np.random is seeded per case (the first shuffles) and per frame (a reshuffle
at the end of a permutation).

A candidate frame is admitted only if (conditions on the INPUTS, checked here; rejected candidates are counted and printed):
 (a) the accepted set is the same from the float32 boxes, from float64 copies of them and with every candidate centre moved by
     +1e-5 m and by -1e-5 m;
 (b) no candidate lies wholly inside or around a box it is tested against (independent float64 test, augment_helpers.contained):
     numba's jit is a stub here, `ret[i, j] is False` is then never true and the reference skips its containment branch;
 (c) every scene point is >= 1e-3 m from every face of every accepted box.
What the fixture has to contain is asserted at the end, so a regenerated fixture cannot lose it."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CAND_LOG, ACC_LOG = [], []


def write_pool(root, infos):
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    for v in infos.values():
        for info in v:
            info["points"].tofile(os.path.join(root, info["path"]))


def make_sampler(prep, sample_ops, case, infos):
    """The reference's sampler on the pool (infos without their points, tagged with their index), as dbsampler_builder.build makes it."""
    db_infos = {n: [dict({k: x for k, x in info.items() if k != "points"}, tag=i) for i, info in enumerate(v)] for n, v in infos.items()}
    prepor = prep.DataBasePreprocessor([prep.DBFilterByMinNumPoint(dict(case["min_num_points"])),
                                        prep.DBFilterByDifficulty(list(case["removed_difficulties"]))])
    np.random.seed(case["pool_seed"])
    sampler = sample_ops.DataBaseSamplerV2(db_infos, [{n: m} for n, m in case["groups"]], prepor, case["rate"], [0.0, 0.0])
    row = 0
    for v in sampler.db_infos.values():
        for info in v:
            info["row"] = row
            row += 1
    return sampler


def sampler_state(sampler):
    return {k: (bs._indices.copy(), bs._idx) for k, bs in sampler._sampler_dict.items()}


def restore(sampler, state):
    for k, (ind, idx) in state.items():
        sampler._sampler_dict[k]._indices, sampler._sampler_dict[k]._idx = ind.copy(), idx


def run_sampler(sampler, state, root, fr, seed, dtype=np.float32, delta=0.0):
    """sample_all from ``state`` on the frame: -> (its dict or None, candidates per sample class, accepted rows)."""
    restore(sampler, state)
    saved = {}
    for v in sampler.db_infos.values():
        for info in v:
            saved[info["row"]] = info["box3d_lidar"]
            b = info["box3d_lidar"].copy()
            b[:2] = b[:2] + np.float32(delta)
            info["box3d_lidar"] = b.astype(dtype)
    CAND_LOG.clear()
    ACC_LOG.clear()
    np.random.seed(seed)
    try:
        ret = sampler.sample_all(root, fr["boxes"].astype(dtype), fr["names"], 4)
    finally:
        for v in sampler.db_infos.values():
            for info in v:
                info["box3d_lidar"] = saved[info["row"]]
    cands = {name: rows for name, _, rows in CAND_LOG}
    return ret, cands, [r for rows in ACC_LOG for r in rows]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT, os.path.join(ROOT, "tests")]
    from second_amd import compat
    compat.install(ref)
    from second.core import box_np_ops, preprocess as prep, sample_ops
    import augment_helpers as ah
    import dbsample_helpers as dh

    orig_sample, orig_class = prep.BatchSampler.sample, sample_ops.DataBaseSamplerV2.sample_class_v2

    def sample(self, num):
        out = orig_sample(self, num)
        CAND_LOG.append((self._name, int(num), [i["row"] for i in out]))
        return out

    def sample_class_v2(self, name, num, gt_boxes):
        out = orig_class(self, name, num, gt_boxes)
        ACC_LOG.append([i["row"] for i in out])
        return out

    prep.BatchSampler.sample, sample_ops.DataBaseSamplerV2.sample_class_v2 = sample, sample_class_v2
    out, rejected = {}, dict(a=0, b=0, c=0)
    seen_kinds = dict(later=0, full=0, down=0, up=0, fewer=0, nogt=0, nopoints=0)
    for ci, (name, case) in enumerate(dh.CASES.items()):
        infos = dh.build_pool(case)
        groups, cn = case["groups"], case["class_names"]
        table = dh.num_table(groups, case["rate"])
        cog = [cn.index(n) + 1 for n, _ in groups]
        with tempfile.TemporaryDirectory() as root:
            write_pool(root, infos)
            sampler = make_sampler(prep, sample_ops, case, infos)
            filtered = {n: np.array([i["tag"] for i in sampler.db_infos[n]], np.int32) for n in infos}
            db = dh.pool_arrays(infos, filtered)
            frames, seeds, res = [], [], []
            for fi, (gt, npts) in enumerate(case["frames"]):
                seed = 1000 * (ci + 1) + 100 * fi
                state = sampler_state(sampler)
                while True:
                    fr = dh.build_frame(case, infos, seed, gt, npts)
                    ret, cands, acc = run_sampler(sampler, state, root, fr, seed)
                    after = sampler_state(sampler)
                    cl = [cands.get(n, []) for n, _ in groups]
                    seen = []
                    mine, per = dh.sample_frame(fr["boxes"], fr["classes"], db["boxes"], cl, cog, table, seen=seen)
                    same = all(run_sampler(sampler, state, root, fr, seed, dt, d)[2] == acc
                               for dt, d in ((np.float64, 0.0), (np.float32, 1e-5), (np.float32, -1e-5)))
                    excess = ah.box_frame_excess(fr["points"], db["boxes"][acc]) if acc and npts else np.ones((1, 1))
                    if seen:
                        rejected["b"] += 1
                    elif not same:
                        rejected["a"] += 1
                    elif np.abs(excess).min() < 1e-3:
                        rejected["c"] += 1
                    else:
                        assert mine == acc, "the helper disagrees with the reference on an admitted frame"
                        break
                    seed += 1
                restore(sampler, after)
                # the merge of second/data/preprocess.py:224-249
                boxes, names, mask, imp, points = fr["boxes"], fr["names"], fr["valid"], fr["importance"], fr["points"]
                removed = np.zeros(len(points), bool)
                if ret is not None:
                    assert ret["gt_boxes"].dtype == np.float32 and ret["points"].dtype == np.float32
                    names = np.concatenate([names, ret["gt_names"]], axis=0)
                    boxes = np.concatenate([boxes, ret["gt_boxes"]])
                    mask = np.concatenate([mask, ret["gt_masks"]], axis=0)
                    imp = np.concatenate([imp, np.full([ret["gt_boxes"].shape[0]], case["sample_importance"], dtype=ret["gt_boxes"].dtype)])
                    if len(points):
                        removed = box_np_ops.points_in_rbbox(points, ret["gt_boxes"]).any(-1)
                        assert np.array_equal(removed, box_np_ops.points_in_rbbox(points.astype(np.float64), ret["gt_boxes"].astype(np.float64)).any(-1))
                    points = np.concatenate([ret["points"], points[np.logical_not(removed)]], axis=0)
                my_points, my_removed = dh.merge_frame(fr["points"], db["boxes"], db["points"], db["offsets"], acc)
                assert np.array_equal(my_removed, removed) and np.array_equal(my_points, points), "the helper's merge differs"
                # what this frame shows
                counts = [int((fr["classes"] == c).sum()) for c in cog]
                wants = [int(table[c][n]) if n < table.shape[1] else 0 for c, n in enumerate(counts)]
                halves = [case["rate"] * (m - n) for (_, m), n in zip(groups, counts)]
                seen_kinds["full"] += any(n >= m for (_, m), n in zip(groups, counts))
                seen_kinds["down"] += any(h > 0 and h % 1 == 0.5 and w == h - 0.5 for h, w in zip(halves, wants))
                seen_kinds["up"] += any(h > 0 and h % 1 == 0.5 and w == h + 0.5 for h, w in zip(halves, wants))
                seen_kinds["down_and_up"] = seen_kinds.get("down_and_up", 0) + (
                    any(h > 0 and h % 1 == 0.5 and w == h - 0.5 for h, w in zip(halves, wants)) and
                    any(h > 0 and h % 1 == 0.5 and w == h + 0.5 for h, w in zip(halves, wants)))
                seen_kinds["fewer"] += any(0 < len(c) < w for c, w in zip(cl, wants))
                seen_kinds["nogt"] += len(fr["boxes"]) == 0
                seen_kinds["nopoints"] += npts == 0
                seen_kinds["later"] += later_only(ah, fr, db, cl, acc)
                frames.append(fr)
                seeds.append(seed)
                res.append(dict(cands=cl, acc=acc, per=per, boxes=boxes, classes=np.array([cn.index(n) + 1 if n in cn else 0 for n in names], np.int32),
                                mask=mask, imp=imp.astype(np.float32), points=points, removed=removed))
        batch = dh.concat_frames(frames)
        k = max([len(c) for r in res for c in r["cands"]] + [1])
        cand = -np.ones((len(res), len(groups), k), np.int16)
        for f, r in enumerate(res):
            for c, rows in enumerate(r["cands"]):
                cand[f, c, :len(rows)] = rows
        out[f"{name}/seeds"] = np.array(seeds, np.int32)
        out[f"{name}/digest"] = np.array(ah.digest(dict(batch, db_boxes=db["boxes"], db_points=db["points"], db_offsets=db["offsets"])))
        for n, v in filtered.items():
            out[f"{name}/filtered/{n}"] = v
        out[f"{name}/candidates"] = cand
        out[f"{name}/accepted"] = np.array([r for x in res for r in x["acc"]], np.int16)
        out[f"{name}/accepted_offsets"] = np.concatenate([[0], np.cumsum([len(x["acc"]) for x in res])]).astype(np.int32)
        out[f"{name}/accepted_per_group"] = np.array([x["per"] for x in res], np.int16)
        out[f"{name}/boxes"] = np.concatenate([x["boxes"] for x in res]).astype(np.float32)
        out[f"{name}/box_offsets"] = np.concatenate([[0], np.cumsum([len(x["boxes"]) for x in res])]).astype(np.int32)
        out[f"{name}/classes"] = np.concatenate([x["classes"] for x in res]).astype(np.int8)
        out[f"{name}/mask"] = np.concatenate([x["mask"] for x in res])
        out[f"{name}/importance"] = np.concatenate([x["imp"] for x in res])
        out[f"{name}/removed"] = np.packbits(np.concatenate([x["removed"] for x in res]))
        out[f"{name}/points"] = np.concatenate([x["points"] for x in res]).astype(np.float32)
        out[f"{name}/point_offsets"] = np.concatenate([[0], np.cumsum([len(x["points"]) for x in res])]).astype(np.int32)
        print(name, "seeds", seeds, "pool", {n: len(v) for n, v in filtered.items()}, "candidates", [[len(c) for c in x["cands"]] for x in res],
              "accepted", [x["per"] for x in res], "removed points", [int(x["removed"].sum()) for x in res])
    prep.BatchSampler.sample, sample_ops.DataBaseSamplerV2.sample_class_v2 = orig_sample, orig_class
    print("frames showing:", seen_kinds)
    for kind in ("later", "full", "down_and_up", "fewer", "nogt", "nopoints"):
        assert seen_kinds[kind] > 0, f"no frame of the fixture shows '{kind}'"
    path = os.path.join(HERE, "dbsample.npz")
    np.savez_compressed(path, **out)
    print("rejected candidates:", rejected, "| bytes:", os.path.getsize(path))


def later_only(ah, fr, db, cands, acc):
    """True if some candidate of the frame is rejected ONLY because of a later candidate of its class that is itself accepted: it
    collides with no gt box, with no accepted object at all, except ones that come later in its own class's candidate list."""
    gt = list(ah.bev_corners(fr["boxes"].astype(np.float64)))
    for rows in cands:
        corners = ah.bev_corners(db["boxes"][rows].astype(np.float64).reshape(-1, 7))
        for i, r in enumerate(rows):
            if r in acc:
                continue
            hits = [j for j in range(len(rows)) if j != i and ah.collide(corners[i], corners[j])]
            other = [a for a in acc if a not in rows and ah.collide(corners[i], ah.bev_corners(db["boxes"][[a]].astype(np.float64))[0])]
            if hits and all(j > i and rows[j] in acc for j in hits) and not other and not any(ah.collide(corners[i], g) for g in gt):
                return True
    return False


if __name__ == "__main__":
    main()
