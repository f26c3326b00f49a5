"""Produces tests/golden/augment.npz by EXECUTING the reference's augmentation functions on CPU (second/core/preprocess.py:
noise_per_box, _select_transform, points_transform_, box3d_transform_, random_flip, global_rotation_v2, global_scaling_v2,
global_translate_, filter_gt_box_outside_range_by_center; second/core/box_np_ops.py: points_in_rbbox, limit_period) in
prep_pointcloud's order (second/data/preprocess.py:255-286).  Build container only (needs the reference checkout):

    python tests/golden/make_golden_augment.py [path to the reference checkout]

The inputs are the seeded float32 frames of tests/augment_helpers.py (CASES, build_frame); the per-object noise is GIVEN to the
reference, the draws of the functions that draw their own (flip flags, angle, scale, translation) are recorded by seeding
np.random, calling, re-seeding and repeating the draws in the same order -- rounded to float32 on the way out of np.random, so the
reference and the device read the same numbers.  `selected`, the masks and the kept set come from the float32 run, the point and
box values from the same functions on float64 copies of the float32 inputs.

A candidate frame is admitted only if (conditions on the INPUTS, checked here; rejected candidates are counted and printed):
 (a) the reference's `selected` is the same in float32, in float64 and with every noise value moved by +1e-5 and by -1e-5;
 (b) no try that is evaluated lies wholly inside or around another box (independent float64 test, augment_helpers.contained):
     numba's jit is a stub here, `ret[i, j] is False` is then never true and the reference skips its containment branch;
 (c) every point is >= 1e-3 m from every face of every box of its frame (float64, box frame, original boxes) and every box centre
     is >= 1e-3 m from the range edge after the transforms.
A frame whose kind says "edge" additionally has to lose a valid box to the range filter (the seed of the global draws is advanced
until it does)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GLOBAL_ROT, GLOBAL_SCALE, GLOBAL_T_STD = (-0.78539816, 0.78539816), (0.95, 1.05), (0.2, 0.2, 0.2)


class rounded_draws:
    """np.random.uniform / normal return float32-representable values while active."""

    def __enter__(self):
        self.u, self.n = np.random.uniform, np.random.normal
        np.random.uniform = lambda *a, **k: np.float64(np.float32(self.u(*a, **k)))
        np.random.normal = lambda *a, **k: np.asarray(self.n(*a, **k), np.float32).astype(np.float64)

    def __exit__(self, *exc):
        np.random.uniform, np.random.normal = self.u, self.n


def replay_draws(seed):
    """(flip_x, flip_y, angle, scale, tx, ty, tz, 0) as random_flip, global_rotation_v2, global_scaling_v2, global_translate_ draw them."""
    np.random.seed(seed)
    with rounded_draws():
        fx = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
        fy = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
        angle, scale = np.random.uniform(*GLOBAL_ROT), np.random.uniform(*GLOBAL_SCALE)
        t = [np.random.normal(0, GLOBAL_T_STD[0], 1)[0], np.random.normal(0, GLOBAL_T_STD[1], 1)[0],
             np.random.normal(0, GLOBAL_T_STD[0], 1)[0]]            # (preprocess.py:894-896 draws z with the x entry)
    return np.array([fx, fy, angle, scale, *t, 0.0], np.float32)


def ref_selected(prep, fr, dtype, delta=0.0):
    if not len(fr["boxes"]):
        return np.zeros(0, np.int64)
    b = fr["boxes"].astype(dtype)[:, [0, 1, 3, 4, 6]]
    return prep.noise_per_box(b, fr["valid"], (fr["loc_noises"] + np.float32(delta)).astype(dtype),
                              (fr["rot_noises"] + np.float32(delta)).astype(dtype))


def ref_frame(prep, ops, fr, pseed, bev_range):
    """The reference's chain on float64 copies; `selected` and the mask from the float32 run."""
    boxes, pts, valid = fr["boxes"].astype(np.float64), fr["points"].astype(np.float64), fr["valid"]
    loc, rot = fr["loc_noises"].astype(np.float64), fr["rot_noises"].astype(np.float64)
    n, npts = len(boxes), len(pts)
    sel = ref_selected(prep, fr, np.float32)
    loc_t = prep._select_transform(loc, sel) if n else np.zeros((0, 3))
    rot_t = prep._select_transform(rot, sel) if n else np.zeros(0)
    mask = ops.points_in_rbbox(fr["points"], fr["boxes"]) if n and npts else np.zeros((npts, n), bool)
    if n and npts:
        assert np.array_equal(mask, ops.points_in_rbbox(pts, boxes)), "points_in_rbbox differs between float32 and float64"
        prep.points_transform_(pts, boxes[:, :3], mask, loc_t, rot_t, valid)
    prep.box3d_transform_(boxes, loc_t, rot_t, valid)
    b = boxes[valid]                                               # _dict_select(gt_dict, gt_boxes_mask)
    np.random.seed(pseed)
    with rounded_draws():
        b, pts = prep.random_flip(b, pts, 0.5, True, True)
        b, pts = prep.global_rotation_v2(b, pts, *GLOBAL_ROT)
        b, pts = prep.global_scaling_v2(b, pts, *GLOBAL_SCALE)
        prep.global_translate_(b, pts, list(GLOBAL_T_STD))
    inside = prep.filter_gt_box_outside_range_by_center(b, bev_range) if len(b) else np.zeros(0, bool)
    margin = np.min(np.abs(np.stack([b[:, 0] - bev_range[0], b[:, 0] - bev_range[2], b[:, 1] - bev_range[1], b[:, 1] - bev_range[3]]))) \
        if len(b) else np.inf
    keep = np.zeros(n, bool)
    keep[np.nonzero(valid)[0][inside]] = True
    out = b[inside]
    out[:, 6] = ops.limit_period(out[:, 6], offset=0.5, period=2 * np.pi)
    return dict(selected=sel, mask=mask, points=pts[:, :3], boxes=out, keep=keep, margin=margin)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT, os.path.join(ROOT, "tests")]
    from second_amd import compat
    compat.install(ref)
    from second.core import box_np_ops as ops, preprocess as prep
    import augment_helpers as ah

    out, rejected = {}, dict(a=0, b=0, c=0, globals=0)
    for ci, (name, (tries, frames)) in enumerate(ah.CASES.items()):
        admitted, seeds, pseeds, results = [], [], [], []
        for fi, (nb, npts, kind) in enumerate(frames):
            seed = 1000 * (ci + 1) + 100 * fi
            while True:
                fr = ah.build_frame(seed, nb, npts, tries, kind)
                s32 = ref_selected(prep, fr, np.float32)
                seen = []
                mine = ah.noise_per_box(fr["boxes"].astype(np.float64), fr["valid"], fr["loc_noises"].astype(np.float64),
                                        fr["rot_noises"].astype(np.float64), containment_seen=seen)
                excess = ah.box_frame_excess(fr["points"], fr["boxes"]) if nb and npts else np.ones((1, 1))
                if seen:
                    rejected["b"] += 1
                elif not (np.array_equal(s32, ref_selected(prep, fr, np.float64)) and np.array_equal(s32, ref_selected(prep, fr, np.float32, 1e-5))
                          and np.array_equal(s32, ref_selected(prep, fr, np.float32, -1e-5))):
                    rejected["a"] += 1
                elif np.abs(excess).min() < 1e-3:
                    rejected["c"] += 1
                else:
                    assert np.array_equal(mine, s32), "the helper disagrees with the reference on an admitted frame"
                    break
                seed += 1
            pseed = seed
            while True:
                r = ref_frame(prep, ops, fr, pseed, np.array(ah.BEV_RANGE))
                lost = bool((fr["valid"] & ~r["keep"]).any())
                if r["margin"] >= 1e-3 and (lost or "edge" not in kind):
                    break
                rejected["c" if r["margin"] < 1e-3 else "globals"] += 1
                pseed += 1
            if "fail" in kind:
                assert r["selected"][0] == -1
            if "late" in kind:
                assert r["selected"][-1] >= 64, r["selected"]
            if "invalid" in kind:
                assert r["selected"][4] > 0 and r["selected"][0] == -1 and r["selected"][3] == -1
            if "overlap" in kind:
                assert (r["mask"].sum(1) >= 2).any(), "no point inside two boxes"
            admitted.append(fr)
            seeds.append(seed)
            pseeds.append(pseed)
            results.append(r)
            out[f"{name}/mask{fi}"] = np.packbits(r["mask"])
        batch = ah.concat_frames(admitted)
        out[f"{name}/seeds"] = np.array(seeds, np.int32)
        out[f"{name}/digest"] = np.array(ah.digest(batch))
        out[f"{name}/frame_params"] = np.stack([replay_draws(p) for p in pseeds])
        out[f"{name}/selected"] = np.concatenate([r["selected"] for r in results]).astype(np.int16)
        out[f"{name}/keep"] = np.concatenate([r["keep"] for r in results])
        out[f"{name}/points"] = np.concatenate([r["points"] for r in results])
        out[f"{name}/boxes"] = np.concatenate([r["boxes"] for r in results])
        out[f"{name}/offsets"] = np.concatenate([[0], np.cumsum([len(r["boxes"]) for r in results])]).astype(np.int32)
        print(name, "seeds", seeds, "global seeds", pseeds, "selected max", out[f"{name}/selected"].max(initial=-1),
              "kept", int(out[f"{name}/keep"].sum()), "of", len(out[f"{name}/keep"]))
    np.savez_compressed(os.path.join(HERE, "augment.npz"), **out)
    print("rejected candidates:", rejected, "| bytes:", os.path.getsize(os.path.join(HERE, "augment.npz")))


if __name__ == "__main__":
    main()
