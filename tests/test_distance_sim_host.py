"""Host side of the DistanceSimilarity target assignment: tests/distance_sim_helpers.py (the restatement the GPU tests compare the
kernels with) against tests/golden/distance_similarity.npz (the EXECUTED reference, make_golden_distance_sim.py), and the Python
plumbing that needs no GPU: second_amd.targets.similarity_config, ops.similarity_spec, DeviceTrainer's ``group_similarity``."""
import os
import re

import numpy as np
import pytest

import distance_sim_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("per_class", "all", "all_dist")


@pytest.fixture(scope="module")
def g(golden):
    return golden("distance_similarity")


def _ids(tag):
    return [1, 2, 3] if tag == "per_class" else [0, 0, 0]


@pytest.mark.parametrize("meaning", ["compiled", "float32"])
@pytest.mark.parametrize("tag", MODES)
def test_restatement_reproduces_the_executed_target_assigner(g, tag, meaning):
    """Labels and importance exactly, box targets within the tolerance of test_gpu_train.py's fixture tests -- under BOTH arithmetic
    meanings: the fixture admits only frames on which they take the same decisions."""
    labels, targets, importance = H.fixture_expected(g, tag)
    assert sorted(set(np.unique(labels).tolist())) == [-1, 0, 1, 2, 3]
    assert (importance != 1.0).any()
    sims = H.fixture_sims(g, tag)
    for f, (gt, cls, imp) in enumerate(H.fixture_frames(g)):
        l, t, i = H.assign_ranges_ref(g["anchors"], gt, cls, g["class_anchor_begin"].tolist(), _ids(tag), g["matched"].tolist(),
                                      g["unmatched"].tolist(), sims, imp, None, meaning)
        np.testing.assert_array_equal(l, labels[f], err_msg=f"labels of frame {f}")
        np.testing.assert_array_equal(i, importance[f], err_msg=f"importance of frame {f}")
        np.testing.assert_allclose(t, targets[f], rtol=1e-5, atol=2e-6, err_msg=f"targets of frame {f}")


def test_fixture_frames_are_all_admitted(g):
    """What the generator asserted, recomputed from the stored frames: margins, window gaps, equal argmax / forced sets."""
    assert int(g["admitted"]) == int(g["frames"]) == len(g["draws_per_frame"]) == 4
    need, gap_need = float(g["margin_required"]), float(g["window_gap_required"])
    assert need == 64 * 2.0 ** -23 and gap_need == 1e-4
    begin = g["class_anchor_begin"].tolist()
    mts, uts = g["matched"].astype(np.float64), g["unmatched"].astype(np.float64)
    negative = 0
    for tag in MODES:
        sims = H.fixture_sims(g, tag)
        for f, (gt, cls, imp) in enumerate(H.fixture_frames(g)):
            a = H.assign_ranges_ref(g["anchors"], gt, cls, begin, _ids(tag), mts, uts, sims, imp, None, "compiled", want_info=True)[3]
            b = H.assign_ranges_ref(g["anchors"], gt, cls, begin, _ids(tag), mts, uts, sims, imp, None, "float32", want_info=True)[3]
            for c, (ia, ib) in enumerate(zip(a, b)):
                if ia["sim"] is None:
                    continue
                for key in ("arg", "force", "pos"):
                    np.testing.assert_array_equal(ia[key], ib[key], err_msg=f"{tag} frame {f} range {c} {key}")
                assert H.decision_margin(ia["sim"], ia["gmax"], mts[c], uts[c]) >= need, (tag, f, c)
                assert H.argmax_margin(ia["sim"]) >= need, (tag, f, c)
                negative += int((ia["sim"] < 0).sum())
                s = sims[0] if tag != "per_class" else sims[c]
                if s is not None:
                    q = gt[cls == c + 1] if tag == "per_class" else gt
                    an = g["anchors"][begin[c]:begin[c + 1]].astype(np.float64)
                    for ax in (0, 1):
                        d = np.abs(np.abs(an[:, None, ax] - q[None, :, ax].astype(np.float64)) - s["distance_norm"])
                        assert d.min() >= gap_need, (tag, f, c, ax)
    assert negative > 100, "the fixture must hold negative similarities"


@pytest.mark.parametrize("ci", [1, 2])
@pytest.mark.parametrize("f", [0, 3])
def test_similarity_matrices(g, ci, f):
    """DistanceSimilarity.compare as executed: the float32 meaning is bit-equal to it, the compiled meaning within meanings_bound."""
    kind, dn, rot, alpha = g[f"sim_{ci}"].tolist()
    assert kind == 1
    begin = g["class_anchor_begin"].tolist()
    p, q = H.xyr(g["anchors"][begin[ci]:begin[ci + 1]]), H.xyr(g[f"gt_{f}"])
    want = g[f"compare_{ci}_{f}"]
    assert want.dtype == np.float32 and want.shape == (len(p), len(q))
    f32 = H.distance_similarity_ref(p, q, dn, bool(rot), alpha, "float32")
    np.testing.assert_array_equal(f32.view(np.uint32), want.view(np.uint32))
    comp = H.distance_similarity_ref(p, q, dn, bool(rot), alpha, "compiled")
    err = np.abs(comp.astype(np.float64) - want.astype(np.float64))
    bound = H.meanings_bound(p, q, dn, bool(rot), alpha)
    assert (err <= bound).all(), float((err - bound).max())
    assert bound.max() < 4e-7                        # a few float32 ulp of 1: the bound is not vacuous
    assert (comp != want).any(), "the two meanings must differ somewhere, or the fixture cannot tell them apart in value"
    assert ((want != 0).sum() > 50) and (ci == 2 or (want < 0).any())


def test_hand_cases_agree_in_both_meanings():
    """Exactly representable coordinates and norms: both meanings agree bit for bit (the GPU tests rely on it), negative values,
    the -1 value, the window edge and the clamp come out as the formula says."""
    p = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [np.nextafter(np.float32(2), np.float32(3)), 0, 0], [0.5, 0.25, 0], [1.5, 1.5, 0]],
                 np.float32)
    q = np.zeros((1, 3), np.float32)
    for rot, alpha in ((False, 0.0), (True, 0.5), (True, 0.25)):
        a = H.distance_similarity_ref(p, q, 2.0, rot, alpha, "compiled")
        b = H.distance_similarity_ref(p, q, 2.0, rot, alpha, "float32")
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    s = H.distance_similarity_ref(p, q, 2.0)[:, 0]
    np.testing.assert_array_equal(s, np.array([1.0, -1.0, -1.0, 0.0, 1 - 0.3125 / 2, -1.0], np.float32))


# ------------------------------------------------------------------------------------------------------------- similarity_config
def test_similarity_config_reads_a_target_assigner(g):
    from second_amd import targets
    cfg = targets.similarity_config(H.standin_assigner(g, "per_class"))
    assert cfg["assign_per_class"] is True and cfg["class_ids"] == [1, 2, 3] and cfg["class_names"] == H.FIXTURE_CLASSES
    assert cfg["similarities"][0] == "nearest_iou"
    assert cfg["similarities"][1] == dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0)
    assert cfg["similarities"][2] == dict(kind="distance", distance_norm=1.0, with_rotation=True, rotation_alpha=0.5)
    np.testing.assert_allclose(cfg["matched_thresholds"], [0.6, 0.5, 0.5], rtol=1e-7)
    np.testing.assert_allclose(cfg["unmatched_thresholds"], [0.45, 0.35, 0.35], rtol=1e-7)
    # assign_all: class id 0 and calculator 0 for every range
    cfg = targets.similarity_config(H.standin_assigner(g, "all_dist"))
    assert cfg["assign_per_class"] is False and cfg["class_ids"] == [0, 0, 0]
    assert cfg["similarities"] == [dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0)] * 3
    # generators in another order than `classes`: the id is the class's position, not the generator's
    ta = H.standin_assigner(g, "per_class")
    ta._classes = ["cyclist", "car", "pedestrian"]
    assert targets.similarity_config(ta)["class_ids"] == [2, 3, 1]


def test_similarity_config_refuses_by_name(g):
    from second_amd import targets
    ta = H.standin_assigner(g, "per_class")
    ta._sim_calcs[2] = H.RotateIouSimilarity()
    with pytest.raises(NotImplementedError, match="RotateIouSimilarity"):
        targets.similarity_config(ta)
    ta = H.standin_assigner(g, "all")                 # refused even where assign_all would not use it
    ta._sim_calcs[1] = H.RotateIouSimilarity()
    with pytest.raises(NotImplementedError, match="RotateIouSimilarity"):
        targets.similarity_config(ta)
    with pytest.raises(NotImplementedError, match="sample_positive_fraction"):
        targets.similarity_config(H.standin_assigner(g, "per_class", positive_fraction=0.5))
    targets.similarity_config(H.standin_assigner(g, "per_class", positive_fraction=-1))      # "no sub-sampling" spelt as a number
    with pytest.raises(NotImplementedError, match="box coder"):
        targets.similarity_config(H.standin_assigner(g, "per_class", box_coder=H.GroundBox3dCoder(vec_encode=True)))

    class BevBoxCoder:
        code_size = 5
    with pytest.raises(NotImplementedError, match="BevBoxCoder"):
        targets.similarity_config(H.standin_assigner(g, "per_class", box_coder=BevBoxCoder()))


# ---------------------------------------------------------------------------------------------------------- argument plumbing
def test_similarity_spec():
    from second_amd import ops
    assert ops.similarity_spec(None) == ops.similarity_spec("nearest_iou") == ops.similarity_spec(dict(kind="nearest_iou")) == (0, 0.0, False, 0.0)
    assert ops.similarity_spec(dict(kind="distance", distance_norm=1.414)) == (1, 1.414, False, 0.5)       # DistanceSimilarity's defaults
    assert ops.similarity_spec(dict(kind="distance", distance_norm=1, with_rotation=1, rotation_alpha=0)) == (1, 1.0, True, 0.0)
    assert ops.similarity_spec((1, 2.0, True, 0.25)) == (1, 2.0, True, 0.25)
    for bad in ("distance", "rotate_iou", dict(kind="rotate_iou"), dict(kind="distance"), dict(kind="distance", distance_norm=0.0),
                dict(kind="distance", distance_norm=-1.0), dict(kind="distance", distance_norm=1.0, norm=2), (2, 1.0, False, 0.0), 3):
        with pytest.raises(ValueError):
            ops.similarity_spec(bad)


def test_group_similarity_of_the_trainer_config():
    from second_amd import models, training
    cfg = models.ALL_FHD_NUSC
    assert "group_similarity" not in cfg, "the stock config keeps the near-box IoU for every class in this change"
    assert training.group_similarities(cfg, 10) is None                        # absent key: the trainer's calls stay as they were
    sims = models.NUSC_FHD_GROUP_SIMILARITY
    assert len(sims) == len(cfg["anchor_groups"]) == 10
    want = dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0)
    assert [i for i, s in enumerate(sims) if s is not None] == [5, 6] and sims[5] == want and sims[6] == want
    assert [cfg["group_rotations"].get(i) for i in (5, 6)] == [[0], [0]]       # the two one-rotation groups: pedestrian, traffic_cone
    specs = training.group_similarities(dict(cfg, group_similarity=sims), 10)
    assert specs[0] == (0, 0.0, False, 0.0) and specs[5] == specs[6] == (1, 1.414, False, 0.0)
    with pytest.raises(ValueError, match="10 anchor groups"):
        training.group_similarities(dict(cfg, group_similarity=sims[:9]), 10)
    with pytest.raises(ValueError):
        training.group_similarities(dict(cfg, group_similarity=["rotate_iou"] * 10), 10)
    with pytest.raises(ValueError, match="assign_per_class is false"):          # assign_all has ONE similarity
        training.group_similarities(dict(cfg, assign_per_class=False, group_similarity=sims), 10)
    same = [dict(want)] * 10
    assert training.group_similarities(dict(cfg, assign_per_class=False, group_similarity=same), 10) == [(1, 1.414, False, 0.0)] * 10


def test_new_symbols_are_declared_and_bound():
    from second_amd import runtime, ops
    header = open(os.path.join(ROOT, "include", "second_hip.h")).read()
    for sym in ("sec_region_similarity_f32", "sec_assign_targets_sim_f32"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in runtime.SYMBOLS
    assert re.search(r"#define\s+SEC_SIM_NEAREST_IOU\s+0\b", header) and re.search(r"#define\s+SEC_SIM_DISTANCE\s+1\b", header)
    assert (ops.SIM_NEAREST_IOU, ops.SIM_DISTANCE) == (0, 1)
    assert re.search(r"#define\s+SEC_ABI_VERSION\s+9\b", header) and runtime.ABI_VERSION == 9      # additions only
    assert "every shipped config" not in header
    assert "every shipped config" not in open(os.path.join(ROOT, "second.pytorch_amd", "csrc", "train.hip")).read().split("namespace sec")[0]
