"""-m gpu: the fused pipeline for ``car.lite.config`` (SimpleVoxelRadius + SpMiddleFHDLite), ``people.fhd.config`` (SimpleVoxel +
SpMiddleFHDPeople) and, end to end, KITTI ``all.fhd.config`` (SimpleVoxelRadius + SpMiddleFHD with three input channels): the SimpleVoxelRadius kernels (fused voxeliser epilogue and stand-alone), the three-channel first sparse conv on
the four-channel kernels, the adopted networks end to end behind ``net(example)`` (tests/reference_standin_lite.py's objects, pinned
to the reference's in tests/test_dropin_reference_lite.py), graph capture of ``forward_points``, the fused rulebook chain on both
geometries and the RPN's tile forms at the two map sizes (160 x 132: not a multiple of the 16-pixel tile width; 200 x 240)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402  (test infrastructure only)
from test_gpu_parity import dev, _conv_case  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _clouds(batch, max_points):
    """lite-range clouds; with max_points > 1 most voxels hold several points; a few points sit ON the sensor axis (x = y = 0)"""
    from lite_helpers import clouds_for
    from second_amd.models import CAR_LITE
    out = []
    for c in clouds_for(CAR_LITE, range(batch), num_points=2400 if max_points > 1 else 1500, num_voxels=1200):
        axis = np.zeros((6, 4), np.float32)
        axis[:, 2] = np.linspace(-2.9, 0.9, 6)               # six voxels of the column x = y = 0
        axis[:, 3] = 0.5
        out.append(np.concatenate([c[:len(c) // 2], axis, c[len(c) // 2:]]))
    return out


# ------------------------------------------------------------------ 4. the radius kernels
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("max_points", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_epilogue_and_standalone_kernel(ops, dtype, max_points, batch):
    from second_amd import synthetic as syn
    from second_amd.models import CAR_LITE
    rng_, vs = CAR_LITE["point_cloud_range"], CAR_LITE["voxel_size"]
    pts, offs = syn.batch_clouds(_clouds(batch, max_points))
    pts, offs = dev(pts), dev(offs)
    kw = dict(mean_features=4, sync=False)
    rad = ops.voxelize(pts, offs, rng_, vs, max_points, 30000, mean_dtype=dtype, encoder="SimpleVoxelRadius", **kw)
    rad32 = ops.voxelize(pts, offs, rng_, vs, max_points, 30000, mean_dtype=torch.float32, encoder="SimpleVoxelRadius", **kw)
    mean = ops.voxelize(pts, offs, rng_, vs, max_points, 30000, mean_dtype=dtype, **kw)
    mean32 = ops.voxelize(pts, offs, rng_, vs, max_points, 30000, mean_dtype=torch.float32, **kw)
    n = int(rad["voxel_offsets"][-1].item())
    assert n >= 1200 * batch and tuple(rad["mean"].shape[1:]) == (4,) and rad["mean"].dtype == dtype
    for k in ("coordinates", "num_points_per_voxel", "voxels", "voxel_offsets"):
        assert torch.equal(rad[k][:n] if k != "voxel_offsets" else rad[k], mean[k][:n] if k != "voxel_offsets" else mean[k]), k
    r, m = rad["mean"][:n], mean["mean"][:n]
    # z and the fourth feature: the SimpleVoxel means, bit for bit; channel 3: exactly zero
    assert torch.equal(_bits(r[:, 1:3]), _bits(m[:, 2:4]))
    assert not _bits(r[:, 3]).any()
    # the radius in fp32 against float64 on the kernel's own fp32 means: 2^-22 relative
    r32, m32 = rad32["mean"][:n].cpu().numpy(), mean32["mean"][:n].cpu().numpy().astype(np.float64)
    want = np.sqrt(m32[:, 0] ** 2 + m32[:, 1] ** 2)
    err = np.abs(r32[:, 0].astype(np.float64) - want)
    print(f"radius vs float64: max rel err {float((err / np.maximum(want, 1e-300)).max()):.3e} (bound {2.0 ** -22:.3e})")
    assert np.all(err <= 2.0 ** -22 * want)
    on_axis = (m32[:, 0] == 0) & (m32[:, 1] == 0)
    assert on_axis.sum() >= 6 * batch and not r32[on_axis, 0].view(np.int32).any()          # exactly +0
    # 16-bit rows = the fp32 rows rounded once
    assert torch.equal(_bits(r), _bits(rad32["mean"][:n].to(dtype)))
    # the stand-alone kernel on the voxel tensor: the fused epilogue's rows bit for bit; rows past num_dev are zero
    alone = ops.simple_voxel_radius(rad["voxels"][:n].contiguous(), rad["num_points_per_voxel"][:n].contiguous(), 4, out_dtype=dtype)
    assert alone.shape == (n, 4) and torch.equal(_bits(alone), _bits(r))
    cut = torch.tensor([n // 3], dtype=torch.int32, device="cuda")
    part = ops.simple_voxel_radius(rad["voxels"][:n].contiguous(), rad["num_points_per_voxel"][:n].contiguous(), 4, out_dtype=dtype, num_dev=cut)
    assert torch.equal(_bits(part[:n // 3]), _bits(r[:n // 3])) and not _bits(part[n // 3:]).any()


@pytest.mark.parametrize("num_features,max_points", [(5, 3), (4, 12)])
def test_radius_epilogue_on_the_shapes_the_fused_fill_does_not_take(ops, num_features, max_points):
    """five point features / more than eight points per voxel: k_vox_fill + the stand-alone kernel inside the voxeliser"""
    from second_amd import synthetic as syn
    from second_amd.models import CAR_LITE
    cl = _clouds(2, max_points)
    if num_features > 4:
        cl = [np.concatenate([c, np.full((len(c), num_features - 4), 7.0, np.float32)], 1) for c in cl]
    pts, offs = syn.batch_clouds(cl)
    pts, offs = dev(pts), dev(offs)
    a = (pts, offs, CAR_LITE["point_cloud_range"], CAR_LITE["voxel_size"], max_points, 30000)
    rad = ops.voxelize(*a, mean_features=4, sync=False, encoder="SimpleVoxelRadius")
    mean = ops.voxelize(*a, mean_features=4, sync=False)
    n = int(rad["voxel_offsets"][-1].item())
    r, m = rad["mean"][:n], mean["mean"][:n]
    assert n > 2000 and torch.equal(_bits(r[:, 1:3]), _bits(m[:, 2:4])) and not _bits(r[:, 3]).any()
    m64 = m.cpu().numpy().astype(np.float64)
    want = np.sqrt(m64[:, 0] ** 2 + m64[:, 1] ** 2)
    assert np.all(np.abs(r[:, 0].cpu().numpy().astype(np.float64) - want) <= 2.0 ** -22 * want)
    alone = ops.simple_voxel_radius(rad["voxels"][:n].contiguous(), rad["num_points_per_voxel"][:n].contiguous(), 4)
    assert torch.equal(_bits(alone), _bits(r))


def test_radius_kernel_against_the_reference_fixture(ops, golden):
    """tests/golden/simple_voxel_radius.npz (the reference's SimpleVoxelRadius.forward on CPU): channel 0 within 2^-21 relative -- the
    kernel's 2^-22 against float64 plus torch's own (its CPU norm is 1.9 * 2^-24 off float64 and one ulp off the plain formula in
    some elements, so bit equality is not expected); r = 0 rows exactly 0."""
    z = golden("simple_voxel_radius")
    for t in (1, 5):
        got = ops.simple_voxel_radius(dev(z[f"voxels_t{t}"]), dev(z[f"num_points_t{t}"]), 4).cpu().numpy()
        want = z[f"out_t{t}"].astype(np.float64)
        err = np.abs(got[:, 0].astype(np.float64) - want[:, 0])
        print(f"t={t}: radius vs the fixture: max rel err {float((err / np.maximum(want[:, 0], 1e-300)).max()):.3e} (bound {2.0 ** -21:.3e})")
        assert np.all(err <= 2.0 ** -21 * want[:, 0])
        assert (want[:, 0] == 0).sum() >= 16 and not got[want[:, 0] == 0, 0].any()
        assert not got[:, 3].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_points,mean_features", [(5, 4), (1, 4), (5, 3), (12, 4)])
def test_old_voxelize_symbol_is_the_encoder_0_form_bit_for_bit(ops, dtype, max_points, mean_features):
    from second_amd import runtime as rt, synthetic as syn
    from second_amd.models import CAR_LITE
    pts, offs = syn.batch_clouds(_clouds(2, max_points))
    pts, offs = dev(pts), dev(offs)
    old = ops.voxelize(pts, offs, CAR_LITE["point_cloud_range"], CAR_LITE["voxel_size"], max_points, 30000, mean_features=mean_features,
                       sync=False, mean_dtype=dtype)
    l = rt.lib()
    n, f = pts.shape
    rows = old["coordinates"].shape[0]
    voxels = torch.zeros((rows, max_points, f), dtype=torch.float32, device="cuda")
    coors = torch.zeros((rows, 4), dtype=torch.int32, device="cuda")
    npv = torch.zeros((rows,), dtype=torch.int32, device="cuda")
    voff = torch.zeros((3,), dtype=torch.int32, device="cuda")
    mean = torch.zeros((rows, mean_features), dtype=dtype, device="cuda")
    ws = rt.workspace(l.sec_voxelize_workspace_bytes(n, 2, 30000, max_points), pts.device)
    rc = l.sec_voxelize_encode_f32(rt.ptr(pts), rt.ptr(offs), n, f, 2, rt.f_arr(CAR_LITE["point_cloud_range"]), rt.f_arr(CAR_LITE["voxel_size"]),
                                   max_points, 30000, 0, rt.ptr(voxels), rt.ptr(coors), rt.ptr(npv), rt.ptr(voff), rt.ptr(mean), mean_features,
                                   rt.dtype_code(dtype), 0, mean_features, rt.ptr(ws), ws.numel(), rt.stream())
    assert rc == 0
    k = int(voff[-1].item())
    assert k == int(old["voxel_offsets"][-1].item()) and k > 2000
    assert torch.equal(voxels[:k], old["voxels"][:k]) and torch.equal(coors[:k], old["coordinates"][:k])
    assert torch.equal(npv[:k], old["num_points_per_voxel"][:k]) and torch.equal(_bits(mean[:k]), _bits(old["mean"][:k]))


# ------------------------------------------------------------------ 5. the three-channel first layer
@pytest.mark.parametrize("subm", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_three_channel_first_layer_on_the_c4_kernels_16bit(ops, dtype, subm):
    """cin = 3 weights zero-padded to 4 on rows [f0, f1, f2, 0]: PLAN_C4 (fp32 store) and k_conv_c4_mfma (16-bit store) against the
    generic kernel on the unpadded operands and the oracle: the max-relative and per-element bounds of
    test_gpu_parity::test_indice_conv_half_mfma, taken with the UNPADDED cin = 3."""
    rng = np.random.default_rng(3 + int(subm))
    feat, w, pairs, pair_num, nbr_out, _, n_out = _conv_case(rng, 3, 16, subm)
    f3, w3 = dev(feat, dtype), dev(w, dtype)
    f4 = torch.nn.functional.pad(f3, (0, 1)).contiguous()
    w4 = torch.nn.functional.pad(w3, (0, 0, 0, 1)).contiguous()
    packed = ops.pack_weight(w4)
    assert packed is not None and ops.pack_weight(w3) is None
    assert ops.indice_conv_plan(4, 16, 27, n_out, dtype, packed=True) == 12                          # PLAN_C4_MFMA
    assert ops.indice_conv_plan(4, 16, 27, n_out, dtype, out_dtype=torch.float32, packed=True) == 2  # PLAN_C4
    assert ops.indice_conv_plan(3, 16, 27, n_out, dtype, packed=False) == 0                          # PLAN_GENERIC
    ref = orc.indice_conv(f3.float().cpu().numpy(), w3.float().cpu().numpy(), pairs, pair_num, n_out, acc64=True)
    mag = orc.indice_conv(np.abs(f3.float().cpu().numpy()), np.abs(w3.float().cpu().numpy()), pairs, pair_num, n_out, acc64=True)
    nbr = dev(nbr_out)
    out32 = ops.indice_conv(f4, w4, nbr, n_out, packed=packed, out_dtype=torch.float32).cpu().numpy()
    np.testing.assert_allclose(out32, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    # the existing test's per-element bound with cin = 3, the unpadded operands' K = 27 * 3 terms: the 27 padded products are
    # 0 * 0 and add exact zeros, so they bring no rounding of their own
    bound = (27 * 3 + 2) * 2.0 ** -24 * mag + 1e-30
    print(f"PLAN_C4 vs oracle: max err / bound {float((np.abs(out32 - ref) / bound).max()):.3f}")
    assert np.all(np.abs(out32 - ref) <= bound)
    gen = ops.indice_conv(f3, w3, nbr, n_out, packed=None, out_dtype=torch.float32).cpu().numpy()
    np.testing.assert_allclose(out32, gen, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    scale = dev(rng.uniform(0.5, 1.5, 16).astype(np.float32))
    shift = dev(rng.uniform(-0.2, 0.2, 16).astype(np.float32))
    fused = ops.indice_conv(f4, w4, nbr, n_out, packed=packed, scale=scale, shift=shift, relu=True)
    assert fused.dtype == dtype
    ref_f = torch.from_numpy(np.maximum(ref * scale.cpu().numpy() + shift.cpu().numpy(), 0)).to(dtype).float().numpy()
    tol = 2 ** -7 if dtype == torch.bfloat16 else 2 ** -10
    np.testing.assert_allclose(fused.float().cpu().numpy(), ref_f, rtol=tol, atol=tol * np.abs(ref_f).max())


@pytest.mark.parametrize("subm", [True, False])
@pytest.mark.parametrize("mode", ["split", "exact"])
def test_three_channel_first_layer_on_the_c4_kernels_fp32(ops, mode, subm):
    """fp32 storage, split-operand and exact products: the bounds of test_gpu_parity::test_indice_conv_fp32 with cin = 3"""
    rng = np.random.default_rng(13 + int(subm))
    feat, w, pairs, pair_num, nbr_out, _, n_out = _conv_case(rng, 3, 16, subm)
    f3, w3 = dev(feat), dev(w)
    f4 = torch.nn.functional.pad(f3, (0, 1)).contiguous()
    w4 = torch.nn.functional.pad(w3, (0, 0, 0, 1)).contiguous()
    ref = orc.indice_conv(feat, w, pairs, pair_num, n_out, acc64=True)
    mag = orc.indice_conv(np.abs(feat), np.abs(w), pairs, pair_num, n_out, acc64=True)
    nbr = dev(nbr_out)
    with ops.fp32_mode("exact" if mode == "exact" else None):
        assert ops.indice_conv_plan(4, 16, 27, n_out, torch.float32, packed=True) == 2               # PLAN_C4
        out = ops.indice_conv(f4, w4, nbr, n_out, packed=ops.pack_weight(w4)).cpu().numpy()
        gen = ops.indice_conv(f3, w3, nbr, n_out, packed=None).cpu().numpy()
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    bound = (4 * 2.0 ** -18 + (27 * 3 + 2) * 2.0 ** -24) * mag + 1e-30          # cin = 3: the padded products are exact zeros
    print(f"{mode}: padded vs oracle: max err / bound {float((np.abs(out - ref) / bound).max()):.3f}")
    assert np.all(np.abs(out - ref) <= bound)
    np.testing.assert_allclose(out, gen, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


# ------------------------------------------------------------------ 6. end to end
def _cfgs():
    from second_amd.models import ALL_FHD_KITTI, CAR_LITE, PEOPLE_FHD
    return {"lite": CAR_LITE, "people": PEOPLE_FHD, "all": ALL_FHD_KITTI}


@pytest.fixture(scope="module", params=["lite", "people", "all"])          # all: KITTI all.fhd (SimpleVoxelRadius + SpMiddleFHD(3), two-block RPN)
def nets(request):
    from lite_helpers import clouds_for, trained_like
    from reference_standin_lite import build_voxelnet_lite
    cfg = _cfgs()[request.param]
    clouds = clouds_for(cfg, range(3), num_points=9000, num_voxels=8000)
    like = trained_like(cfg, clouds[0])                   # CPU, fp32: distinct scores, empty regions below the threshold

    def make():
        net = build_voxelnet_lite(cfg)
        net.load_state_dict(like.state_dict())
        return net.eval().cuda()
    return cfg, make, clouds


def test_fp32_forward_example_is_one_graph_and_returns_the_module_graphs_detections(nets):
    from reference_standin import example_of
    from second_amd import compat
    from test_gpu_dropin_fused import _same
    cfg, make, clouds = nets
    net = make()
    ex = example_of(net, clouds[:2], "cuda")
    with torch.no_grad():
        want = net(ex)
        heads_want = net.network_forward(ex["voxels"], ex["num_points"], ex["coordinates"], 2)
    assert sum(w["scores"].shape[0] for w in want) >= 6
    assert compat.accelerate_model(net) is net
    eng = net._second_amd_engine
    assert eng.cfg["middle"] == cfg["middle"] and eng.cfg.get("vfe", "SimpleVoxel") == cfg.get("vfe", "SimpleVoxel") and eng.cfg["downsample_factor"] == cfg["downsample_factor"]
    with torch.no_grad():
        got = net(ex)
    assert eng.stats == dict(eng.stats, fused_calls=1, original_calls=0, adoptions=1, captures=1, overflow_recaptures=0)
    assert eng.run_dtype() is None and eng._det._infer_dtype in (None, torch.float32)
    _same(got, want)
    det = eng._det
    with torch.no_grad():
        pitch = None
        if det.encoder == "SimpleVoxelRadius":
            feats, pitch = det.voxel_feature_extractor.encode(ex["voxels"], ex["num_points"])
            assert pitch == 4 and feats.shape[1] == 4
            assert det.voxel_feature_extractor(ex["voxels"], ex["num_points"]).shape[1] == 3       # the module itself: always (r, z, w)
        else:
            feats = det.voxel_feature_extractor(ex["voxels"], ex["num_points"], ex["coordinates"])
        heads_got = det.network_forward(feats, ex["coordinates"], 2, in_pitch=pitch)
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        a, b = heads_got[k].float().cpu().numpy(), heads_want[k].float().cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * float(np.abs(b).max()), err_msg=k)
    # a second example of the same batch size reuses the session and its graph
    ex2 = example_of(net, clouds[1:3], "cuda")
    with torch.no_grad():
        got2 = net(ex2)
        want2 = net._second_amd_original_forward(ex2)
    assert eng.stats["captures"] == 1 and eng.stats["fused_calls"] == 2 and eng.stats["original_calls"] == 0 and len(eng._sessions) == 1, eng.stats
    _same(got2, want2)
    # training mode keeps the object's own forward (dropin_train refuses these networks)
    net.train()
    assert not eng.accepts(ex)
    net.eval()


def test_half_network_runs_the_fp16_pipeline_and_bf16_can_be_forced(nets):
    """the detection rule and share of tests/test_gpu_dropin_fused.py's car.fhd case (``_found``, 85 %)"""
    from reference_standin import example_of
    from second_amd import compat
    from test_gpu_dropin_fused import _found
    cfg, make, clouds = nets
    ref32 = make()
    ex32 = example_of(ref32, clouds[:2], "cuda")
    with torch.no_grad():
        want = ref32(ex32)
    net = make().half()
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.float()
    compat.accelerate_model(net)
    eng = net._second_amd_engine
    ex16 = example_of(net, clouds[:2], "cuda", dtype=torch.float16)
    with torch.no_grad():
        got = net(ex16)
    assert eng.run_dtype() == torch.float16 and eng._det._infer_dtype == torch.float16 and eng.stats["captures"] == 1
    assert eng.stats["original_calls"] == 0
    hit, tot = _found(got, want)
    print(f"{cfg['name']} fp16: {hit} of {tot} fp32 detections found")
    assert tot >= 6 and hit >= 0.85 * tot, (hit, tot)
    assert abs(sum(g["scores"].shape[0] for g in got) - tot) <= 2 * len(got)
    nb = compat.accelerate_model(make(), dtype=torch.bfloat16)
    with torch.no_grad():
        gotb = nb(ex32)
    assert nb._second_amd_engine._det._infer_dtype == torch.bfloat16 and nb._second_amd_engine.stats["original_calls"] == 0
    hit, tot = _found(gotb, want)
    print(f"{cfg['name']} bf16: {hit} of {tot} fp32 detections found")
    assert hit >= 0.85 * tot, (hit, tot)


def _prepared(cfg, dtype):
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    torch.manual_seed(0)
    det = SecondDetector(cfg)
    syn.randomise_like_trained(det, seed=1)
    det = det.eval().cuda()
    return det.prepare_inference(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_forward_points_of_car_lite_under_a_graph_equals_its_eager_result(dtype):
    from lite_helpers import clouds_for
    from second_amd import synthetic as syn
    from second_amd.models import CAR_LITE
    det = _prepared(CAR_LITE, dtype)
    pts, offs = syn.batch_clouds(clouds_for(CAR_LITE, range(2), num_points=9000, num_voxels=8000))
    pts, offs = dev(pts), dev(offs)
    with torch.no_grad():
        det.calibrate(pts, offs)
        eager = {k: v.clone() for k, v in det.forward_points(pts, offs, static=True).items()}
        det.check_overflow()
        dyn = det.forward_points(pts, offs)
    replay, outs = det.make_graphed(pts, offs)
    replay()
    torch.cuda.synchronize()
    det.check_overflow()
    assert int(eager["valid"].sum()) > 0
    for k in eager:
        assert torch.equal(eager[k], outs[k]), k
    assert torch.equal(dyn["valid"], eager["valid"]) and torch.equal(dyn["scores"][dyn["valid"]], eager["scores"][eager["valid"]])


@pytest.mark.parametrize("name", ["lite", "people", "all"])
def test_fused_rulebook_chain_on_both_geometries_equals_the_layer_by_layer_builds(ops, name, monkeypatch):
    """as tests/test_gpu_chain.py::test_detector_with_and_without_the_fused_chain_agree for car.fhd; the chain must not decline
    any geometry (lite: no SubM level at all; people: three strided levels; all: KITTI all.fhd, SpMiddleFHD on the lite grid)."""
    from lite_helpers import clouds_for
    from second_amd import synthetic as syn
    cfg = _cfgs()[name]
    det = _prepared(cfg, torch.bfloat16)
    pts, offs = syn.batch_clouds(clouds_for(cfg, range(2), num_points=9000, num_voxels=8000))
    pts, offs = dev(pts), dev(offs)
    built = []
    real = ops.rulebook_chain

    def spy(*a, **k):
        r = real(*a, **k)
        built.append(r is not None)
        return r
    monkeypatch.setattr(ops, "rulebook_chain", spy)
    with torch.no_grad():
        det.calibrate(pts, offs)
        mfe = det.middle_feature_extractor
        assert mfe.fused_chain
        a = det.forward_points(pts, offs, static=True)
        det.check_overflow()
        assert built == [True], built
        mfe.fused_chain = False
        b = det.forward_points(pts, offs, static=True)
        mfe.fused_chain = True
        assert built == [True]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["valid"].sum()) > 0


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("batch,h,w,n", [(2, 160, 132, 1500), (2, 200, 240, 1500), (1, 160, 132, 1)])
def test_rpn_tiles_at_the_lite_and_people_map_sizes(ops, dtype, batch, h, w, n, lazy):
    import test_gpu_rpn_tiles as T
    T.test_rpn_with_background_tiles_is_bit_identical_to_the_full_convs(ops, dtype, batch, h, w, n, lazy)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("batch,h,w,n", [(2, 160, 132, 700), (2, 200, 240, 700)])
def test_rpn_fused_tail_at_the_lite_and_people_map_sizes(ops, dtype, batch, h, w, n):
    import test_gpu_rpn_tiles as T
    T.test_fused_tail_on_ragged_maps_matches_the_two_launches(ops, dtype, batch, h, w, n)
