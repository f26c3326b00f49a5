"""CPU-only: the anchor-area mask's fixture, host-side restatement and entry points.

tests/golden/anchor_mask.npz holds what the reference computes (tests/golden/make_golden_anchor_mask.py); the numpy float32
restatement of tests/anchor_mask_helpers.py -- which the GPU tests use where no fixture exists -- must equal it exactly.  The new
C entry points exist in header, library and runtime.SYMBOLS and refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest

import anchor_mask_helpers as H


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_numpy_restatement_equals_the_reference(golden, name):
    case = H.CASES[name]
    vs, rng, grid = H.geometry(case)
    anchors, _ = H.anchors_of(case)
    fx = H.load_case(golden, name)
    for t in case["thresholds"]:
        for f, coors in enumerate(fx["coors"]):
            got = H.anchor_mask_np(coors, anchors, vs, rng, grid, t)
            assert np.array_equal(got, fx["masks"][t][f]), (name, t, f, int((got != fx["masks"][t][f]).sum()))
    if name in ("A", "C"):         # float64 quotients give another mask: the cases notice a wrong order of operations
        assert int(golden[f"{name}_float64_flips"]) > 0
        t = case["thresholds"][-1] if name == "C" else 1
        diff = sum(int((H.anchor_mask_np(c, anchors, vs, rng, grid, t, dtype=np.float64) != fx["masks"][t][f]).sum())
                   for f, c in enumerate(fx["coors"]))
        assert diff > 0
    if name == "A":
        m = fx["masks"][1]
        assert not m[0].any() and m[1].any() and not m[1].all() and m[2].all()       # empty frame, both values, all ones


def test_kitti_pp_car_16_config():
    from second_amd import models as M
    cfg = M.KITTI_PP_CAR_16
    assert M.grid_size_of(cfg).tolist() == [432, 496, 1] and M.anchors_per_location(cfg) == 2
    assert M.anchor_area_threshold_of(cfg) == 1.0
    for other in (M.CAR_FHD, M.ALL_PP_LARGEA, M.ALL_FHD_NUSC, M.CAR_LITE, M.PEOPLE_FHD, M.ALL_FHD_KITTI):
        assert M.anchor_area_threshold_of(other) is None
    assert M.anchor_area_threshold_of(dict(cfg, anchor_area_threshold=-1)) is None
    anchors = M.generate_anchors(cfg, [1, 248, 216])
    assert anchors.shape == (248 * 216 * 2, 7) and anchors.dtype == np.float32
    assert np.array_equal(anchors, H.anchors_of(H.CASES["C"])[0])                      # == the reference's AnchorGeneratorStride (fixture generator)
    det = M.SecondDetector(cfg)
    assert det.feature_map_size == [1, 248, 216] and det.anchors.shape == (107136, 7) and det.pillars
    assert M.RPNInference.supports(det.rpn)


def test_entry_points_exist_and_validate_before_any_launch():
    from second_amd import runtime as rt
    from test_capi_symbols import header_functions
    new = ["sec_anchor_area_mask_workspace_bytes", "sec_anchor_area_mask", "sec_predict_select_masked", "sec_assign_targets_masked_f32"]
    l = rt.lib()
    hdr = header_functions()
    for n in new:
        assert n in hdr and n in rt.SYMBOLS and hasattr(l, n), n
    assert l.sec_abi_version() == 9
    one = ctypes.c_void_p(4096)                      # never dereferenced: validation fails first
    f2 = rt.f_arr([0.16, 0.16])
    # ---- sec_anchor_area_mask
    need = l.sec_anchor_area_mask_workspace_bytes(8, 496, 432)
    assert need >= 8 * 496 * 432 * 4 and l.sec_anchor_area_mask_workspace_bytes(0, 496, 432) == 0
    args = (one, 100, None, 8, 496, 432, one, 107136, f2, f2, 1.0)
    assert l.sec_anchor_area_mask(*args, None, one, need, None) == -1                 # no mask output
    assert l.sec_anchor_area_mask(one, 100, None, 8, 496, 432, None, 107136, f2, f2, 1.0, one, one, need, None) == -1       # no anchors
    assert l.sec_anchor_area_mask(one, 100, None, 8, 496, 432, one, 107136, None, f2, 1.0, one, one, need, None) == -1      # no voxel size
    assert l.sec_anchor_area_mask(one, 100, None, 8, 496, 432, one, 107136, f2, f2, -1.0, one, one, need, None) == -1       # negative threshold
    assert l.sec_anchor_area_mask(*args, one, one, need - 1, None) == -2              # short workspace
    assert l.sec_anchor_area_mask(*args, one, None, need, None) == -2
    # ---- sec_predict_select_masked
    st = (ctypes.c_int64 * 5)(2048, 1024, 32, 1, 1)
    sel = lambda thr, outs, live, bg, mask: l.sec_predict_select_masked(one, st, 2, 2, 32, 32, 1, 100, thr, one, *outs, rt.SEC_F32, live, bg, mask, None)
    ok = (one, one, one, one)
    assert sel(0.3, (None, one, one, one), None, None, one) == -1                     # NULL outputs
    assert sel(0.3, (one, one, one, None), None, None, one) == -1
    assert sel(0.0, ok, None, None, one) == -3                                        # a mask with score_thr = 0
    assert sel(-1.0, ok, None, None, one) == -3
    assert sel(0.3, ok, one, None, one) == -1                                         # tile_live without background
    assert sel(0.3, ok, None, one, None) == -1
    assert l.sec_predict_select_masked(one, st, 2, 2, 32, 32, 1, 100, 0.3, None, *ok, rt.SEC_F32, None, None, one, None) == -2   # no key scratch
    # ---- sec_assign_targets_masked_f32
    need = l.sec_assign_targets_workspace_bytes(2, 2048, 4)
    begin, ids = (ctypes.c_int * 2)(0, 2048), (ctypes.c_int * 1)(0)
    thr = (ctypes.c_float * 1)(0.5)
    asg = lambda labels, ws, nbytes, b=begin: l.sec_assign_targets_masked_f32(one, 2048, one, one, None, one, 4, 2, 1, b, ids, thr, thr, labels, one, one,
                                                                               ws, nbytes, one, None)
    assert asg(None, one, need) == -1                                                 # NULL outputs
    assert asg(one, one, need - 1) == -2 and asg(one, None, need) == -2               # short / no workspace
    assert asg(one, one, need, (ctypes.c_int * 2)(0, 2000)) == -1                     # ranges do not cover the anchors
