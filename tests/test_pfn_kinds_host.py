"""CPU-only checks of the PillarFeatureNet family (PillarFeatureNetOld, PillarFeatureNetRadiusHeight, with_distance on all four):
the float64 row reference of tests/pfn_kinds_helpers.py reproduces what the reference's modules computed (tests/golden/pfn_kinds.npz,
eight variants); a float32 emulation of the kernels' order passes every comparison tests/test_gpu_pfn_kinds.py uses and each planted
mistake fails it; the new C entry points validate on the host before any launch; the models' torch formulations agree with the
fixture and leave their input alone; dropin.model_config adopts a reference-built PillarFeatureNetOld network."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pfn_kinds_helpers as K
import pfn_ref_helpers as H

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def fixture():
    return K.load_fixture()


# ---- the float64 reference against the reference's own modules ------------------------------------------------------------------
@pytest.mark.parametrize("row", K.ALL_ROWS, ids=K.row_id)
def test_float64_reference_reproduces_the_fixture(fixture, row):
    g = fixture
    case, key = K.fixture_case(g, *row)
    out, _ = K.eval64(case, *row)
    np.testing.assert_allclose(out, g[key + "eval64"], rtol=1e-11, atol=1e-12)
    # the reference's float32 run sits inside the bound a float32 kernel is held to (its own error is recorded beside it)
    assert K.check_eval(g[key + "eval32"], case, *row, "fp32") <= 1.0
    ref = K.train_ref(case, *row)
    for q in ("out", "running_mean", "running_var"):
        np.testing.assert_allclose(ref[q], g[key + q], rtol=1e-10, atol=1e-12, err_msg=q)
    bw = H.backward64(ref, case, ref["argmax"], ref["out"] > 0, case["grad_out"])
    for q in H.BWD_KEYS:
        np.testing.assert_allclose(bw[q], g[key + q], rtol=1e-9, atol=1e-12, err_msg=q)
    got = dict(mean=ref["mean"], invstd=ref["invstd"], out=g[key + "out"], argmax=ref["argmax"], running_mean=g[key + "running_mean"],
               running_var=g[key + "running_var"], d_linear_weight=g[key + "d_linear_weight"], d_norm_weight=g[key + "d_norm_weight"],
               d_norm_bias=g[key + "d_norm_bias"])
    res = K.check_train(got, case, *row)
    assert max(res.values()) <= 1e-3, res
    for q in H.FWD_KEYS[2:] + H.BWD_KEYS:
        assert 0 <= float(g[key + "f32_err." + q]) < 1e-4, q          # the reference's own float32 error, recorded per quantity


def test_old_row_is_what_the_reference_leaves_in_its_input(fixture):
    """PillarFeatureNetOld centres the caller's x, y columns in place: the recorded columns are x - cx, y - cy on EVERY slot (the
    padded ones too: 0 - c), which is the row's columns 0, 1 = 7, 8 on the live slots; the distance is taken over them."""
    g = fixture
    for dist in (False, True):
        case, key = K.fixture_case(g, K.OLD, dist)
        mutated = g[key + "mutated_xy"]
        vx, vy, xo, yo = (np.float32(v) for v in case["geom"])
        co = g["coords"]
        cen = np.stack([co[:, 3].astype(np.float32) * vx + xo, co[:, 2].astype(np.float32) * vy + yo], 1)
        assert np.array_equal(mutated, g["voxels"][..., :2] - cen[:, None, :])
        dec, _, live = K.decorate64(case["vox"], case["num"], case["coords"], case["geom"], K.OLD, dist)
        assert np.array_equal(dec[..., 0:2], dec[..., 7:9])
        np.testing.assert_allclose(dec[..., 0:2], mutated * live[..., None], rtol=0, atol=2e-6)
        if dist:
            want = np.sqrt(dec[..., 0] ** 2 + dec[..., 1] ** 2 + dec[..., 2] ** 2)
            np.testing.assert_allclose(dec[..., 9], want, rtol=1e-14)
            raw = np.sqrt((g["voxels"].astype(np.float64)[..., :3] ** 2).sum(-1)) * live
            assert np.abs(dec[..., 9] - raw).max() > 1.0                   # nowhere near the raw distance


# ---- a float32 emulation passes, planted mistakes fail --------------------------------------------------------------------------
HOST_TRAIN = [c for c in H.TRAIN_CASES if c[0] * c[1] * c[2] <= 150000 or c[3] == "offset"]


@pytest.mark.parametrize("row", K.ALL_ROWS, ids=K.row_id)
def test_float32_emulation_passes_every_eval_comparison(row):
    for case_id in K.EVAL_CASES:
        case = K.eval_case(*case_id)
        out = K.emulate32(case, *row, "eval")
        for kind, dt in H.KINDS.items():
            got = torch.from_numpy(out).to(dt)
            assert K.check_eval(got, case, *row, kind) <= 1.0, (case_id, kind)


@pytest.mark.parametrize("row", K.NEW_ROWS, ids=K.row_id)
@pytest.mark.parametrize("case_id", HOST_TRAIN, ids=lambda c: "-".join(map(str, c)))
def test_float32_emulation_passes_every_train_comparison(case_id, row):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    res = K.check_train(K.emulate32(case, *row, "train"), case, *row)
    assert set(res) == set(H.FWD_KEYS + H.BWD_KEYS + ("argmax", "gate"))
    assert max(res.values()) <= 1.0, res


# (bug, row, points): the point set on which the mistake moves a value
BUG_CASES = [
    ("plain_for_old", (K.OLD, False), "far"), ("old_mean_after_centre", (K.OLD, False), "far"), ("old_dist_raw", (K.OLD, True), "far"),
    ("h_live_only", (K.RADIUS_HEIGHT, False), "below"), ("h_live_only", (K.RADIUS_HEIGHT, False), "above"),
    ("h_lanes_zero", (K.RADIUS_HEIGHT, False), "full"), ("h_unmasked", (K.RADIUS_HEIGHT, False), "far"),
    ("dist_before_h", (K.RADIUS_HEIGHT, True), "far"),
]


def _h_weighted(case, row):
    """The case's weights with a line for h (and the distance) that no channel ignores."""
    w = K.wt_of(case, *row).copy()
    w[8:] = np.where(np.abs(w[8:]) < 0.1, 0.2, w[8:])
    return w


@pytest.mark.parametrize("bug,row,points", BUG_CASES, ids=lambda v: v if isinstance(v, str) else K.row_id(v))
def test_planted_mistakes_fail_the_comparisons(bug, row, points):
    assert bug in K.BUGS
    case = K.eval_case(33, 12, 64, points, "plain")
    case["wt"] = _h_weighted(case, row)
    assert K.check_eval(K.emulate32(case, *row, "eval"), case, *row, "fp32") <= 1.0
    assert K.check_eval(K.emulate32(case, *row, "eval", bug=bug), case, *row, "fp32") > 1.0
    # training: the same pillars with train-mode parameters
    tc = H.train_case(33, 12, 64, "plain")
    tc["vox"], tc["num"], tc["coords"] = case["vox"], case["num"], case["coords"]
    tc["wt"] = case["wt"]
    del tc["wt9"]
    ok = K.check_train(K.emulate32(tc, *row, "train"), tc, *row)
    assert max(ok.values()) <= 1.0, ok
    bad = K.check_train(K.emulate32(tc, *row, "train", bug=bug), tc, *row)
    assert max(bad.values()) > 1.0, bad


def test_every_planted_mistake_is_exercised():
    assert {b for b, _, _ in BUG_CASES} == set(K.BUGS)


def test_new_point_sets_have_their_properties():
    for t in (1, 5, 64, 65, 200):
        vox, n, _ = K.pillars(33, t, "below")
        live = np.arange(t)[None, :] < n[:, None]
        assert (vox[..., 2][live] < 0).all() and ((n < t).all() if t > 1 else True)
        if t > 1:                                                          # the padded zero is the maximum: h = -min z
            dec = K.decorate64(vox, n, np.zeros((33, 4), np.int32), H.GEOM, K.RADIUS_HEIGHT, False)[0]
            assert np.array_equal(dec[:, 0, 8], -vox[..., 2].astype(np.float64).min(1))
        vox, n, _ = K.pillars(33, t, "above")
        assert (vox[..., 2][np.arange(t)[None, :] < n[:, None]] > 0).all()
        vox, n, _ = K.pillars(33, t, "flat")
        assert (n == t).all() and (vox[..., 2] == vox[:, :1, 2]).all()
        assert (K.decorate64(vox, n, np.zeros((33, 4), np.int32), H.GEOM, K.RADIUS_HEIGHT, False)[0][..., 8] == 0).all()
    ts, cs, ps = ({c[i] for c in K.EVAL_CASES} for i in (1, 2, 0))
    assert ts >= {1, 5, 63, 64, 65, 127, 200} and cs >= {1, 64, 65, 128} and ps >= {1, 3, 4, 5, 33}
    assert {c[3] for c in K.EVAL_CASES} >= {"far", "axis", "single", "full", "intensity255", "below", "above", "flat"}


def test_trimmed_slots_keep_the_padded_zero_in_h():
    case = H.train_case(33, 20, 16, "plain")
    case["vox"] = case["vox"].copy()
    case["vox"][..., 2] = -np.abs(case["vox"][..., 2]) - 0.5 * (case["vox"][..., 2] != 0)          # every live z < 0
    trimmed = H.trim_slots(case)
    a, b = K.train64(case, K.RADIUS_HEIGHT, True), K.train64(trimmed, K.RADIUS_HEIGHT, True)
    np.testing.assert_allclose(a["mean"], b["mean"], rtol=1e-12)
    np.testing.assert_allclose(a["out"], b["out"], rtol=1e-12, atol=1e-14)


# ---- host validation of the new entry points ------------------------------------------------------------------------------------
def test_kind_entry_points_validate_before_any_launch():
    from second_amd import ops, runtime as rt
    l = rt.lib()
    assert [l.sec_pfn_row_width(k, 0) for k in range(4)] == [9, 8, 9, 9]
    assert [l.sec_pfn_row_width(k, 1) for k in range(4)] == [10, 9, 10, 10]
    assert l.sec_pfn_row_width(4, 0) == 0 and l.sec_pfn_row_width(-1, 0) == 0 and l.sec_pfn_row_width(0, 2) == 0
    for k in range(4):
        for d in (0, 1):
            assert ops.pfn_row_width(k, bool(d)) == l.sec_pfn_row_width(k, d) == K.width(k, bool(d))
    assert (rt.SEC_PFN_PLAIN, rt.SEC_PFN_RADIUS, rt.SEC_PFN_OLD, rt.SEC_PFN_RADIUS_HEIGHT) == (K.PLAIN, K.RADIUS, K.OLD, K.RADIUS_HEIGHT)
    # the workspace grows with the row width; nine entries ask what sec_pfn_train_workspace_bytes asks
    q = l.sec_pfn_kind_train_workspace_bytes
    assert q(K.RADIUS, 0, 5000, 64) < q(K.PLAIN, 0, 5000, 64) < q(K.PLAIN, 1, 5000, 64) == q(K.OLD, 1, 5000, 64) == q(K.RADIUS_HEIGHT, 1, 5000, 64)
    assert q(K.PLAIN, 0, 5000, 64) == q(K.OLD, 0, 5000, 64) == q(K.RADIUS, 1, 5000, 64) == l.sec_pfn_train_workspace_bytes(5000, 64)
    assert q(4, 0, 100, 64) == 0 and q(0, 2, 100, 64) == 0 and q(0, 0, 100, 65) == 0 and q(0, 0, -1, 64) == 0
    one = ctypes.c_void_p(4096)                       # non-NULL, never dereferenced: validation fails first
    f = [ctypes.c_float(0.25)] * 4
    fwd = lambda kind, dist, feats=4: l.sec_pfn_kind_fwd(kind, dist, one, one, one, 10, None, 12, feats, one, one, one, 16, *f, one, rt.SEC_F32, None)
    assert fwd(4, 0) == -1 and fwd(-1, 0) == -1 and fwd(K.OLD, 2) == -1 and fwd(K.OLD, -1) == -1
    assert fwd(K.OLD, 1, feats=5) == -3 and fwd(K.RADIUS_HEIGHT, 0, feats=3) == -3
    assert l.sec_pfn_kind_fwd(K.OLD, 0, one, one, one, 10, None, 12, 4, one, one, one, 16, *f, one, 7, None) == -3      # unknown dtype
    slots = lambda kind, dist, feats=4: l.sec_pfn_kind_fwd_slots(kind, dist, one, one, 1 << 20, 100, 1, 10, 12, feats, one, one, 10, None,
                                                                 one, one, one, 16, *f, one, rt.SEC_F32, None)
    assert slots(4, 0) == -1 and slots(K.OLD, 3) == -1 and slots(K.OLD, 0, feats=5) == -3
    big = 1 << 30
    tf = lambda kind, dist, t=12, feats=4, c=16, ws=big: l.sec_pfn_kind_train_fwd(
        kind, dist, one, one, one, 10, None, t, feats, one, one, one, ctypes.c_float(1e-3), ctypes.c_float(0.01), None, None, c, *f,
        one, one, one, one, ws, None)
    tb = lambda kind, dist, t=12, feats=4, c=16, ws=big: l.sec_pfn_kind_train_bwd(
        kind, dist, one, one, one, 10, None, t, feats, one, one, one, c, *f, one, one, one, one, one, one, one, ws, None)
    for fn in (tf, tb):
        assert fn(4, 0) == -1 and fn(K.OLD, 2) == -1
        assert fn(K.OLD, 0, feats=5) == -3 and fn(K.RADIUS_HEIGHT, 1, c=65) == -3
        for kind, dist in K.NEW_ROWS:
            need = q(kind, int(dist), 10, 16)
            assert need > 0 and fn(kind, int(dist), ws=need - 1) == -2
    assert tf(K.OLD, 0, t=128) == -3 and tb(K.OLD, 0, t=128) == -3                   # T > 127: the int8 argmax ends at slot 126


def test_one_training_function_per_row_of_the_family():
    """ops.pfn_kind_train_function (no library call): one cached class per (kind, with_distance), the two named classes for the rows
    they name, every class a PFNTrainFunction that carries its row and the row's width."""
    from second_amd import ops
    assert len(K.ALL_ROWS) == 8
    classes = {row: ops.pfn_kind_train_function(*row) for row in K.ALL_ROWS}
    assert classes[(K.PLAIN, False)] is ops.PFNTrainFunction and classes[(K.RADIUS, False)] is ops.PFNRadiusTrainFunction
    assert ops.PFNKindTrainFunction is ops.PFNTrainFunction            # the earlier base's name: callers' issubclass checks hold
    assert len(set(classes.values())) == 8 and len({cls.__name__ for cls in classes.values()}) == 8
    for (kind, dist), cls in classes.items():
        assert ops.pfn_kind_train_function(kind, dist) is cls and ops.pfn_kind_train_function(int(kind), int(dist)) is cls
        assert issubclass(cls, ops.PFNTrainFunction)
        assert (cls.KIND, cls.WITH_DISTANCE, cls.K) == (kind, dist, K.width(kind, dist))
    with pytest.raises(ValueError):
        ops.pfn_kind_train_function(4, False)


# ---- the models' torch formulations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.ALL_ROWS, ids=K.row_id)
def test_torch_formulation_matches_the_fixture_and_leaves_its_input(fixture, row):
    from second_amd import models
    g = fixture
    kind, dist = row
    case, key = K.fixture_case(g, kind, dist)
    cls = models.VFES[K.KIND_NAMES[kind]]
    assert K.KIND_NAMES[kind] in models.PILLAR_VFES and cls.kind == kind
    for dt, tol in ((torch.float64, 1e-10), (torch.float32, 2e-5)):
        m = cls(4, [16], g["voxel_size"].tolist(), g["pc_range"].tolist(), with_distance=dist)
        layer = m.pfn_layers[0]
        assert tuple(layer.linear.weight.shape) == (16, K.width(kind, dist))
        assert set(m.state_dict()) >= {"pfn_layers.0.linear.weight", "pfn_layers.0.norm.weight", "pfn_layers.0.norm.running_var"}
        with torch.no_grad():
            layer.linear.weight.copy_(torch.from_numpy(case["wt"].T.copy()))
            for name in ("weight", "bias", "running_mean", "running_var"):
                getattr(layer.norm, name).copy_(torch.from_numpy(g["norm_" + name] if name in ("weight", "bias") else g[name]))
        m.to(dt)
        v = torch.from_numpy(g["voxels"].copy()).to(dt)
        keep = v.clone()
        n, co = torch.from_numpy(g["num_points"]), torch.from_numpy(g["coords"])
        out = m.eval()(v, n, co)
        assert torch.equal(v, keep)                                         # PillarFeatureNetOld included: the input is only read
        np.testing.assert_allclose(out.detach().double().numpy(), g[key + "eval64"], rtol=tol, atol=tol)
        m.train()
        out = m(v, n, co)
        (out * torch.from_numpy(g["w"]).to(dt)).sum().backward()
        assert torch.equal(v, keep)
        scale = float(np.abs(g[key + "d_linear_weight"]).max())
        np.testing.assert_allclose(out.detach().double().numpy(), g[key + "out"], rtol=tol, atol=tol)
        np.testing.assert_allclose(layer.linear.weight.grad.double().numpy(), g[key + "d_linear_weight"], rtol=tol, atol=tol * scale)
        np.testing.assert_allclose(layer.norm.running_var.double().numpy(), g[key + "running_var"], rtol=tol, atol=tol)
    dec = m.decorate(v, n, co).detach().double().numpy()
    np.testing.assert_allclose(dec, K.decorate64(g["voxels"], g["num_points"], g["coords"], case["geom"], kind, dist)[0], rtol=1e-4, atol=2e-5)


def test_detector_config_reads_the_distance_option():
    from second_amd import models
    cfg = models.ALL_PP_MIDA
    assert cfg["vfe"] == "PillarFeatureNetOld" and cfg["max_points_per_voxel"] == 60 and cfg["max_voxels"] == 30000
    assert models.anchors_per_location(cfg) == 20 and cfg["downsample_factor"] == 4 and cfg["assign_per_class"]
    assert [i for i, s in enumerate(cfg["group_similarity"]) if s] == [5, 6] and cfg["group_similarity"][5]["distance_norm"] == 1.414
    small = dict(cfg, point_cloud_range=[-8, -8, -5, 8, 8, 3], anchor_ranges=[[-8, -8, r[2], 8, 8, r[5]] for r in cfg["anchor_ranges"]])
    for dist in (False, True):
        det = models.SecondDetector(dict(small, vfe_with_distance=dist))
        vfe = det.voxel_feature_extractor
        assert type(vfe) is models.PillarFeatureNetOld and vfe.with_distance == dist
        assert vfe.pfn_layers[0].linear.in_features == 9 + int(dist)


# ---- drop-in adoption of a reference-built network ------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [False, True], ids=["plain", "with_distance"])
def test_model_config_adopts_a_reference_built_old_network(dist):
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    import oracle_backend
    from second_amd import compat, dropin
    from second_amd.models import ALL_PP_MIDA, SecondDetector
    compat.install(REF)
    from google.protobuf import text_format
    from second.protos import pipeline_pb2
    import second.pytorch.train as train
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(REF, "second/configs/nuscenes/all.pp.mida.config")).read(), cfg)
    cfg.model.second.voxel_feature_extractor.with_distance = dist
    with oracle_backend.installed():
        net = train.build_network(cfg.model.second).eval()
        assert type(net.voxel_feature_extractor).__name__ == "PillarFeatureNetOld"
        c = dropin.model_config(net)
    assert c["vfe"] == "PillarFeatureNetOld" and c["vfe_with_distance"] is dist and c["vfe_filters"] == [64]
    for k in ("point_cloud_range", "voxel_size", "max_points_per_voxel", "middle", "middle_in", "downsample_factor", "num_class",
              "num_direction_bins", "direction_offset", "direction_limit_offset", "nms_score_threshold", "nms_pre_max_size",
              "nms_post_max_size", "nms_iou_threshold", "use_rotate_nms", "post_center_range"):
        assert c[k] == pytest.approx(ALL_PP_MIDA[k]), k
    for k in ("layer_nums", "layer_strides", "num_filters", "upsample_strides", "num_upsample_filters", "num_input_features"):
        assert c["rpn"][k] == ALL_PP_MIDA["rpn"][k], k
    assert c["num_anchor_per_loc"] == 20
    det = SecondDetector(c)
    mine, theirs = det.state_dict(), net.state_dict()
    for k in theirs:
        if k.startswith("voxel_feature_extractor."):
            assert k in mine and tuple(mine[k].shape) == tuple(theirs[k].shape), k
    # training stays refused by name
    from second_amd import dropin_train
    with pytest.raises(dropin_train.NotTrainable, match="PillarFeatureNetOld|PointPillars"):
        dropin_train.FusedTrainStep(net, c, torch.bfloat16)
