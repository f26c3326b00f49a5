"""CPU-only: boxes with custom values (rows of 7 + custom_ndim values; nuScenes velocity).

  * tests/box_custom_helpers.py reproduces tests/golden/box_custom.npz, which the executed reference produced;
  * models.generate_anchors with ``anchor_custom_values`` equals the reference's anchors cast to float32, exactly;
  * a float32 emulation of every kernel's custom-column arithmetic passes the comparisons tests/test_gpu_box_custom.py applies to
    the kernels, and each planted mistake fails them;
  * every *_nd entry point answers with its documented status before anything is enqueued;
  * dropin.model_config adopts a ground coder with custom_ndim = 2 and still refuses vec_encode; the refusals are named."""
import ctypes
import types

import numpy as np
import pytest
import torch

import box_custom_helpers as H
import train_ref_helpers as T


@pytest.fixture(scope="module")
def g():
    return H.fixture()


NINE_WEIGHTS = (1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 0.25, 1.5)


# -------------------------------------------------------------------------------------------- the helpers reproduce the fixture
def test_fixture_is_small_and_typed_as_the_reference_returns_it(g):
    import os
    assert os.path.getsize(H.GOLDEN) < 100 * 1024
    assert str(g["anchors_dtype"]) == "float64" and g["anchors"].dtype == np.float64 and g["anchors"].shape == (360, 9)
    assert g["target_vals_per_class"].dtype == np.float64
    a = g["anchors"]
    assert np.array_equal(a[:, :7].astype(np.float32).astype(np.float64), a[:, :7])          # float32 values widened
    begin = g["class_anchor_begin"]
    for c in range(2):
        assert np.array_equal(a[begin[c]:begin[c + 1], 7:], np.broadcast_to(g["custom_values"][c], (begin[c + 1] - begin[c], 2)))


def test_generate_anchors_with_custom_values_equals_the_reference(g):
    from second_amd import models
    cfg = H.fixture_cfg(g)
    got = models.generate_anchors(cfg, [int(v) for v in g["feature_map_size"]])
    assert got.dtype == np.float32 and got.shape == (360, 9)
    assert np.array_equal(got, g["anchors"].astype(np.float32))
    assert np.array_equal(got[:240, 7:], np.broadcast_to(np.float32([0.25, -0.5]), (240, 2)))
    assert models.box_ndim_of(cfg) == 9 and models.box_ndim_of(dict(cfg, anchor_custom_values=[])) == 7
    # one list for every group; absent = seven columns, as before
    one = models.generate_anchors(dict(cfg, anchor_custom_values=[0.25, -0.5]), [1, 12, 10])
    assert np.array_equal(one[:, 7:], np.broadcast_to(np.float32([0.25, -0.5]), (360, 2)))
    plain = models.generate_anchors({k: v for k, v in cfg.items() if k != "anchor_custom_values"}, [1, 12, 10])
    assert plain.shape == (360, 7) and np.array_equal(plain, got[:, :7])
    assert np.array_equal(models.generate_anchors(dict(cfg, anchor_custom_values=[0.1]), [1, 12, 10])[:, 7], np.full(360, np.float32(0.1)))
    with pytest.raises(ValueError, match="same number"):
        models.generate_anchors(dict(cfg, anchor_custom_values=[[0, 0], [0]]), [1, 12, 10])
    with pytest.raises(ValueError, match="at most 4"):
        models.generate_anchors(dict(cfg, anchor_custom_values=[0] * 5), [1, 12, 10])


@pytest.mark.parametrize("tag,ids", [("per_class", [1, 2]), ("all", [0, 0])])
def test_assign_reference_reproduces_the_fixture(g, tag, ids):
    lab, tg = H.fixture_targets(g, tag)
    begin = g["class_anchor_begin"].tolist()
    for f, (gt, cls) in enumerate(H.fixture_frames(g)):
        l, t, arg = H.assign_ref_nd(g["anchors"], gt, cls, begin, ids, g["matched"].astype(np.float64), g["unmatched"].astype(np.float64))
        assert np.array_equal(l, lab[f]), f
        np.testing.assert_allclose(t, tg[f], rtol=1e-12, atol=1e-13)
        assert ((arg >= 0) == (l > 0)).all()
    assert (lab[1] == 0).all() and (lab[0] == 1).any() and (lab[0] == 2).any() and np.abs(tg[0][..., 7:]).max() > 1.0


def test_decode_reference_reproduces_the_fixture(g):
    anc = torch.from_numpy(g["anchors"])[torch.from_numpy(g["decode_rows"]).long()]
    got = H.decode_ref(torch.from_numpy(g["decode_enc"]), anc).numpy()
    np.testing.assert_allclose(got, g["decode_out"], rtol=1e-13, atol=1e-14)
    assert np.array_equal(got[:, 7:], g["decode_enc"][:, 7:] + anc.numpy()[:, 7:])


def _fixture_loss(g, dtype=torch.float64, mistake=None):
    cfg = dict(zip([str(k) for k in g["loss_cfg_keys"]], g["loss_cfg"].tolist()), code_weights=tuple(g["code_weights"].tolist()))
    anchors = g["anchors"].astype(np.float32)[g["loss_anchor_rows"]]
    return H.loss_nd(g["loss_cls"], g["loss_box"], g["loss_dir"], g["loss_labels"].astype(np.int32), g["loss_reg"], anchors,
                     g["loss_importance"], 2, 2, dtype=dtype, mistake=mistake, **cfg)


def test_loss_reference_reproduces_the_fixture(g):
    out6, d_cls, d_box, d_dir = _fixture_loss(g)
    np.testing.assert_allclose(out6, g["loss_out6"], rtol=1e-11)
    for got, key in ((d_cls, "loss_d_cls"), (d_box, "loss_d_box"), (d_dir, "loss_d_dir")):
        np.testing.assert_allclose(got, g[key], rtol=1e-10, atol=1e-15)
    assert np.abs(g["loss_d_box"][..., 7:]).max() > 0


@pytest.mark.parametrize("fx", [0, 1])
@pytest.mark.parametrize("fy", [0, 1])
def test_velocity_reference_reproduces_the_fixture(g, fx, fy):
    v = g["aug_boxes"][:, 7:9]
    flips = H.velocity_ref(v, fx, fy, 0.0, 1.0, dtype=np.float32, rotate=False)
    assert np.array_equal(flips, g[f"aug_flip_{fx}{fy}"][:, 7:9])                              # sign changes only: exact
    full = H.velocity_ref(v, fx, fy, float(g["aug_angle"]), float(g["aug_scale"]))
    H.check_velocity(g[f"aug_full_{fx}{fy}"][:, 7:9], v, full)
    assert np.abs(full - v).max() > 0.1


# ------------------------------------------------------------------- float32 emulations through the GPU tests' comparisons
def test_decode_emulation_passes_and_the_planted_mistake_fails():
    rng = np.random.default_rng(3)
    e, a = H.exact_sum_values(rng, (500, 4)), H.exact_sum_values(rng, (500, 4))
    H.check_decode_custom(e + a, e, a)                                                         # one float32 addition
    with pytest.raises(AssertionError):
        H.check_decode_custom(e - a, e, a)                                                     # custom value subtracted


def test_assign_emulation_passes_the_custom_column_comparison(g):
    anchors = g["anchors"].astype(np.float32)
    gt, cls = H.fixture_frames(g)[0]
    lab, tg = H.fixture_targets(g, "per_class")
    _, _, arg = H.assign_ref_nd(anchors, gt, cls, g["class_anchor_begin"].tolist(), [1, 2], g["matched"].astype(np.float64),
                                g["unmatched"].astype(np.float64))
    emu = np.zeros((len(anchors), 2), np.float32)
    emu[arg >= 0] = gt[arg[arg >= 0], 7:] - anchors[arg >= 0, 7:]
    H.check_assign_custom(emu, anchors, gt, arg)
    # what the reference returned (float64 arithmetic on the same float32 values) rounds to the same bits
    assert np.array_equal(emu, tg[0][:, 7:].astype(np.float32))
    # the rows recovered from the 7-column targets are the reference's
    cand = np.zeros((len(anchors), len(gt)), bool)
    begin = g["class_anchor_begin"]
    for c in range(2):
        cand[begin[c]:begin[c + 1]] = cls[None, :] == c + 1
    t7 = np.zeros((len(anchors), 7), np.float32)
    fg = arg >= 0
    a32, g32 = anchors[fg], gt[arg[fg]]
    t7[fg, 6], t7[fg, 2] = g32[:, 6] - a32[:, 6], (g32[:, 2] - a32[:, 2]) / a32[:, 5]
    assert np.array_equal(H.matched_rows(anchors, gt, t7, lab[0], cand), arg)
    with pytest.raises(AssertionError):
        H.check_assign_custom(-emu, anchors, gt, arg)


@pytest.fixture(scope="module")
def loss_case():
    c = H.loss_case_nd(5, 2, 257, 3, 2, 9, direction_offset=T.LOSS_NONDEFAULT["direction_offset"])
    cfg = dict(T.LOSS_NONDEFAULT, code_weights=NINE_WEIGHTS)
    args = (c["cls"], c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"], 3, 2)
    return args, cfg, H.loss_nd(*args, **cfg)


def test_loss_emulation_passes(loss_case):
    args, cfg, want = loss_case
    H.check_loss(H.loss_nd(*args, dtype=torch.float32, **cfg), want)


@pytest.mark.parametrize("mistake", ["sin_last", "weight_shift", "dir_last"])
def test_planted_loss_mistakes_fail(loss_case, mistake):
    """Sin-difference on the last column instead of column 6; code weight j applied to column j - 1; direction target from column
    box_ndim - 1."""
    args, cfg, want = loss_case
    with pytest.raises(AssertionError):
        H.check_loss(H.loss_nd(*args, dtype=torch.float32, mistake=mistake, **cfg), want)


def test_velocity_emulation_passes_and_planted_mistakes_fail():
    rng = np.random.default_rng(8)
    v = rng.normal(0, 3, (300, 2)).astype(np.float32)
    angle, scale = np.float32(0.61), np.float32(1.04)
    for fx in (0, 1):
        for fy in (0, 1):
            want = H.velocity_ref(v, fx, fy, float(angle), float(scale))
            H.check_velocity(H.velocity_ref(v, fx, fy, angle, scale, dtype=np.float32), v, want)
            for mistake in ("rot_sign", "no_scale", "translate") + (("flip_col",) if fy else ()):
                with pytest.raises(AssertionError):
                    H.check_velocity(H.velocity_ref(v, fx, fy, angle, scale, dtype=np.float32, mistake=mistake), v, want)
    flips = H.velocity_ref(v, 0, 1, 0.0, 1.0, dtype=np.float32, rotate=False)
    assert not np.array_equal(H.velocity_ref(v, 0, 1, 0.0, 1.0, dtype=np.float32, rotate=False, mistake="flip_col"), flips)


# ------------------------------------------------------------------------------------------------ C ABI: statuses on the host
OK_, INVALID, UNSUPPORTED = 0, -1, -3


def test_nd_entry_points_validate_before_any_launch():
    """NULL arguments: SEC_E_INVALID; box_ndim 6 and 12: SEC_E_UNSUPPORTED; two tables at once: SEC_E_INVALID; augmentation widths 8 and
    10: SEC_E_UNSUPPORTED.  Every pointer is a non-NULL address that is never dereferenced: validation answers first (no GPU needed)."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)
    s5 = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)

    def decode(nd, box=one, tile=None, cover=None, bg=None):
        return l.sec_predict_decode_nd(box, s5, None, None, 0, 1, 2, 8, 16, 4, one, one, one, 1, one, one, one, rt.SEC_F32, nd, tile, cover,
                                       bg, None, None)
    assert decode(9, box=None) == INVALID
    assert decode(6) == UNSUPPORTED and decode(12) == UNSUPPORTED
    assert decode(9, tile=one, cover=one, bg=one) == INVALID                     # two tables at once
    assert decode(9, tile=one) == INVALID and decode(9, bg=one) == INVALID        # a table without its background, and the reverse

    ptrs, dims = (ctypes.c_void_p * 1)(4096), (ctypes.c_int * 3)(2, 8, 16)

    def segments(nd, n=1, anchors=one):
        return l.sec_predict_decode_segments_nd(n, ptrs, s5, None, None, dims, 0, 1, 4, anchors, one, one, 1, one, one, one, rt.SEC_F32, nd, None)
    assert segments(9, anchors=None) == INVALID and segments(9, n=5) == INVALID
    assert segments(6) == UNSUPPORTED and segments(12) == UNSUPPORTED

    def finalize(nd, dec=one):
        return l.sec_predict_finalize_nd(dec, one, one, one, one, one, 1, 4, 4, 1, 0.0, 0.0, 2, None, one, one, one, one, nd, None)
    assert finalize(9, dec=None) == INVALID
    assert finalize(6) == UNSUPPORTED and finalize(12) == UNSUPPORTED

    begin, ids = (ctypes.c_int * 2)(0, 10), (ctypes.c_int * 1)(0)
    thr, kinds, params = (ctypes.c_float * 1)(0.5), (ctypes.c_int * 1)(0), (ctypes.c_double * 3)(0, 0, 0)

    def assign(nd, anchors=one, k=kinds):
        return l.sec_assign_targets_nd_f32(anchors, 10, one, one, None, one, 3, 1, 1, begin, ids, thr, thr, k, params, one, one, one, one,
                                           1 << 20, None, nd, None)
    assert assign(9, anchors=None) == INVALID and assign(9, k=None) == INVALID
    assert assign(6) == UNSUPPORTED and assign(12) == UNSUPPORTED

    h = rt.f_arr([0.25, 2.0, 3.0, 1, 1, 1, 2, 0.2, 0, 1] + [1.0] * 12)

    def loss(nd, cls=one, hp=h):
        return l.sec_second_loss_nd_f32(cls, one, one, one, one, one, one, 1, 10, 1, 2, hp, nd, one, one, one, one, one, 1 << 20, None)
    assert loss(9, cls=None) == INVALID and loss(9, hp=None) == INVALID
    assert loss(6) == UNSUPPORTED and loss(12) == UNSUPPORTED

    r4 = rt.f_arr([0, -40, 70.4, 40])

    def augment(nd, boxes=one, rng=r4):
        return l.sec_augment_boxes_nd_f32(boxes, one, 5, 1, None, None, None, None, None, one, rng, nd, one, None, None, one, None)
    assert augment(9, boxes=None) == INVALID and augment(9, rng=None) == INVALID
    for nd in (6, 8, 10, 11, 12):
        assert augment(nd) == UNSUPPORTED, nd


def test_ops_name_the_width_they_refuse():
    from second_amd import ops
    assert ops.BOX_MAX_NDIM == H.BOX_MAX_NDIM == 11 and len(ops.LOSS_DEFAULTS["code_weights"]) == 7
    with pytest.raises(ValueError, match="7 to 11"):
        ops._box_ndim(12, "predict_decode")
    with pytest.raises(ValueError, match="7 to 11"):
        ops._box_ndim(6, "predict_decode")


# --------------------------------------------------------------------------------------------------- adoption and named refusals
def _standin_net(custom_ndim=2, **coder_kw):
    from second_amd import models
    return H.standin_net(dict(models.CAR_FHD, anchor_custom_values=[0.0] * custom_ndim), custom_ndim, **coder_kw)


def test_model_config_adopts_custom_ndim_and_still_refuses_vec_encode():
    from second_amd import dropin, models
    net = _standin_net(2)
    assert net.rpn.conv_box.out_channels == 2 * 9
    cfg = dropin.model_config(net)
    assert cfg["anchor_custom_values"] == [[0.0, 0.0]] and models.box_ndim_of(cfg) == 9
    assert "anchor_custom_values" not in dropin.model_config(_standin_net(0))
    for kw in (dict(vec_encode=True), dict(linear_dim=True)):
        with pytest.raises(dropin.NotAccelerable, match="vec_encode, linear_dim and the BEV coder"):
            dropin.model_config(_standin_net(2, **kw))
    net = _standin_net(2)
    net._box_coder.custom_ndim, net._box_coder.code_size = 5, 12
    with pytest.raises(dropin.NotAccelerable, match="at most 4"):
        dropin.model_config(net)
    net = _standin_net(2)
    net.target_assigner._anchor_generators[0]._custom_values = [0.0]
    with pytest.raises(dropin.NotAccelerable, match="custom_values"):
        dropin.model_config(net)


def test_target_assigner_config_accepts_custom_ndim(golden):
    import distance_sim_helpers as D
    from second_amd import targets
    coder = D.GroundBox3dCoder()
    coder.custom_ndim, coder.code_size = 2, 9
    ta = D.standin_assigner(golden("distance_similarity"), "per_class", box_coder=coder)
    assert targets.similarity_config(ta)["box_ndim"] == 9
    coder.vec_encode = True
    with pytest.raises(NotImplementedError, match="box coder"):
        targets.similarity_config(ta)


def test_named_refusals():
    from second_amd import augment, dropin_train, models, training
    with pytest.raises(ValueError, match="multiclass_nms with anchor_custom_values"):
        models.SecondDetector(dict(models.CAR_FHD, anchor_custom_values=[0.0, 0.0], multiclass_nms=True))
    det = types.SimpleNamespace(heads=[{}], pillars=True, box_ndim=9, cfg={"name": "standin"})
    with pytest.raises(NotImplementedError, match="custom box values"):
        training.MultiHeadDeviceTrainer._check_network(det)
    with pytest.raises(dropin_train.NotTrainable, match="custom box values"):
        dropin_train.FusedTrainStep(None, {"anchor_custom_values": [[0.0, 0.0]]}, torch.bfloat16)
    aug = augment.DeviceAugmenter([-0.1, 0.1], [0.2, 0.2, 0.2], [-0.5, 0.5], [0.95, 1.05], [0, 0, 0], True, True, [0, -40, -3, 70.4, 40, 1],
                                  device="cpu", sampler=object())
    pts, offs = torch.zeros((4, 4)), torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="database sampling with 9-column"):
        aug(pts, offs, torch.zeros((2, 9)), torch.tensor([0, 2], dtype=torch.int32))
    aug.sampler = None
    with pytest.raises(ValueError, match="rows of 7 values, or of 9"):
        aug(pts, offs, torch.zeros((2, 8)), torch.tensor([0, 2], dtype=torch.int32))
