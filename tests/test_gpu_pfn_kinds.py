"""The PillarFeatureNet family on the device (sec_pfn_kind_fwd / _fwd_slots / _train_fwd / _train_bwd: PillarFeatureNetOld,
PillarFeatureNetRadiusHeight and with_distance on all four rows) per element against float64, at every form's edges, then through
models.SecondDetector and training.DeviceTrainer at a reduced nuscenes/all.pp.mida geometry.  References, bounds, point sets and the
case tables: tests/pfn_kinds_helpers.py on top of tests/pfn_ref_helpers.py; tests/test_pfn_kinds_host.py proves on the CPU that a
float32 emulation passes these comparisons and that each planted mistake (plain row for old, old's mean after centring, old's
distance from raw x, y, h without the padded zeros, h with idle lanes as zeros, h unmasked, distance before h) fails them."""
import ctypes

import numpy as np
import pytest
import torch

import pfn_kinds_helpers as K
import pfn_ref_helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ids(c):
    return "-".join(str(v) for v in c)


def _fwd(case, row, dtype=None, num_dev=None):
    from second_amd import ops
    kind, dist = row
    return ops.pfn_forward(dev(case["vox"]), dev(case["num"]), dev(case["coords"]), dev(K.wt_of(case, kind, dist)), dev(case["scale"]),
                           dev(case["shift"]), *case["geom"], out_dtype=dtype, num_dev=num_dev, kind=kind, with_distance=dist)


# ---- inference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.NEW_ROWS, ids=K.row_id)
def test_inference_per_element_against_float64(row):
    """Every case of K.EVAL_CASES (T 1 .. 200 on both sides of the 64-slot pass, C 1 .. 128, P 1 .. 33, the eight point sets) in the
    three output dtypes."""
    worst = {}
    for case_id in K.EVAL_CASES:
        case = K.eval_case(*case_id)
        for kind, dt in H.KINDS.items():
            out = _fwd(case, row, dt)
            assert out.dtype == dt
            worst[(case_id, kind)] = K.check_eval(out, case, *row, kind)
    top = max(worst, key=worst.get)
    print("eval", K.row_id(row), "worst", top, f"{worst[top]:.3f}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_flat_pillars_have_exactly_zero_height():
    """All z of a full pillar equal: h = 0 exactly, so the h line of the weights cannot move the output (idle lanes at +-inf, not 0:
    with z = -2 everywhere a zero would make h = 2)."""
    row = (K.RADIUS_HEIGHT, False)
    for t in (5, 64, 65):
        case = K.eval_case(5, t, 64, "flat", "plain")
        case["vox"][..., 2] = -2.0
        w = K.wt_of(case, *row).copy()
        a = _fwd(dict(case, wt=w), row)
        w[8] = 100.0
        b = _fwd(dict(case, wt=w), row)
        assert torch.equal(a, b), t


@pytest.mark.parametrize("row", [(K.OLD, True), (K.RADIUS_HEIGHT, True)], ids=K.row_id)
@pytest.mark.parametrize("live", [0, 20, 33, 50])
def test_inference_live_count_through_the_c_entry_point(live, row):
    """num_dev below, equal to and above P on a sentinel-filled output: rows at or past the live count are untouched."""
    from second_amd import runtime as rt
    case = K.eval_case(33, 9, 65, "below", "plain")
    p, c = 33, 65
    args = [dev(case[k]) for k in ("vox", "num", "coords")] + [dev(K.wt_of(case, *row)), dev(case["scale"]), dev(case["shift"])]
    nd = torch.tensor([live], dtype=torch.int32, device="cuda")
    for kind, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        out = torch.full((p + 3, c), -7.5, dtype=dt, device="cuda")                     # three guard rows behind the P rows
        rc = rt.lib().sec_pfn_kind_fwd(row[0], int(row[1]), rt.ptr(args[0]), rt.ptr(args[1]), rt.ptr(args[2]), p, rt.ptr(nd), 9, 4,
                                       rt.ptr(args[3]), rt.ptr(args[4]), rt.ptr(args[5]), c, *[ctypes.c_float(v) for v in case["geom"]],
                                       rt.ptr(out), rt.dtype_code(dt), rt.stream())
        assert rc == 0
        torch.cuda.synchronize()
        n = min(live, p)
        assert bool((out[n:] == -7.5).all()), (live, kind)
        if n:
            head = {k: (v[:n] if k in ("vox", "num", "coords") else v) for k, v in case.items() if not isinstance(k, tuple)}
            assert K.check_eval(out[:n], head, *row, kind) <= 1.0


SLOTS_RANGE, SLOTS_VOXEL, SLOTS_GEOM = [0, 0, -3, 1, 1, 1], [0.25, 0.25, 4], (0.25, 0.25, 0.125, 0.125)


def _slots_cloud(rng):
    """The cloud of tests/test_gpu_pfn_edges.py: 300 points in one pillar (it overflows every T), 400 spread over the others; every
    z below zero.  -> points [700, 4], the offsets of its two frames."""
    pts = rng.uniform([0, 0, -3, 0], [1, 1, -0.25, 1], (700, 4)).astype(np.float32)
    pts[:300, :2] = rng.uniform(0.51, 0.74, (300, 2))                                # all in pillar (2, 2) of the first cloud
    pts[:380] = pts[rng.permutation(380)]
    return pts, np.array([0, 380, 700], np.int32)


def _older_forward(radius):
    """sec_pfn_fwd / sec_pfn_radius_fwd through ctypes against ops.pfn_forward (T > 64: the second pass of the slot loop; C > 64: the
    second pass of the channel loop; a negative BN scale)."""
    from second_amd import ops, runtime as rt
    fn = rt.lib().sec_pfn_radius_fwd if radius else rt.lib().sec_pfn_fwd
    for case_id in ((33, 65, 65, "far", "plain"), (5, 9, 128, "axis", "negative_scale")):
        case = H.eval_case(*case_id)
        p, t, _ = case["vox"].shape
        wt = H._wt(case, radius)
        c = wt.shape[1]
        a = [dev(case[k]) for k in ("vox", "num", "coords")] + [dev(wt), dev(case["scale"]), dev(case["shift"])]
        for dt in H.KINDS.values():
            want = (ops.pfn_radius_forward if radius else ops.pfn_forward)(*a, *case["geom"], out_dtype=dt)
            got = torch.empty_like(want)
            rc = fn(rt.ptr(a[0]), rt.ptr(a[1]), rt.ptr(a[2]), p, None, t, 4, rt.ptr(a[3]), rt.ptr(a[4]), rt.ptr(a[5]), c,
                    *[ctypes.c_float(v) for v in case["geom"]], rt.ptr(got), rt.dtype_code(dt), rt.stream())
            assert rc == 0
            assert torch.equal(got, want), (case_id, dt)


def _older_forward_slots(radius):
    """sec_pfn_fwd_slots / sec_pfn_radius_fwd_slots through ctypes against ops.pfn_forward_slots on the voxeliser's point lists
    (fill=False), on both sides of the 64-slot pass."""
    from second_amd import ops, runtime as rt
    fn = rt.lib().sec_pfn_radius_fwd_slots if radius else rt.lib().sec_pfn_fwd_slots
    for t in (5, 65):
        rng = np.random.default_rng(t)
        pts, offs = _slots_cloud(rng)
        c = 65
        wt = dev((rng.standard_normal((8 if radius else 9, c)) / 3).astype(np.float32))
        sc, sh = dev(rng.uniform(0.5, 1.5, c).astype(np.float32)), dev(rng.uniform(-0.3, 0.3, c).astype(np.float32))
        dpts = dev(pts)
        v = ops.voxelize(dpts, dev(offs), SLOTS_RANGE, SLOTS_VOXEL, t, 32, "break", fill=False)
        table, ws, n, max_voxels, max_points, _ = v["site_table"]
        npv, coords = v["num_points_per_voxel"], v["coordinates"].contiguous()
        assert int(npv.max()) == t and int(npv.min()) < t and (n, max_points) == (700, t)
        p = coords.shape[0]
        for dt in H.KINDS.values():
            want = ops.pfn_forward_slots(dpts, v, wt, sc, sh, *SLOTS_GEOM, out_dtype=dt, radius=radius)
            got = torch.empty_like(want)
            rc = fn(rt.ptr(dpts), rt.ptr(ws), ws.numel(), n, 2, max_voxels, max_points, 4, rt.ptr(npv), rt.ptr(coords), p, None, rt.ptr(wt),
                    rt.ptr(sc), rt.ptr(sh), c, *[ctypes.c_float(g) for g in SLOTS_GEOM], rt.ptr(got), rt.dtype_code(dt), rt.stream())
            assert rc == 0
            assert torch.equal(got, want), (t, dt)


def _older_training(radius):
    """sec_pfn_train_fwd / _bwd (or their radius forms; no count, the workspace of sec_pfn_train_workspace_bytes) through ctypes
    against ops.PFNTrainFunction / PFNRadiusTrainFunction: out, argmax, stats, running statistics and the three gradients, bit for
    bit.  T = 127: the int8 argmax sits at its last slot."""
    from second_amd import ops, runtime as rt
    l = rt.lib()
    fwd = l.sec_pfn_radius_train_fwd if radius else l.sec_pfn_train_fwd
    bwd = l.sec_pfn_radius_train_bwd if radius else l.sec_pfn_train_bwd
    cls = ops.PFNRadiusTrainFunction if radius else ops.PFNTrainFunction
    assert (3, 127, 64, "plain", (-0.3, 0.3)) in H.TRAIN_CASES
    for p, t, c in ((33, 5, 16), (3, 127, 64)):
        case = H.train_case(p, t, c, "plain")
        wt = H._wt(case, radius)
        k = wt.shape[0]
        a = {n: dev(case[n]) for n in ("vox", "num", "coords", "gamma", "beta", "grad_out")}
        geom = [ctypes.c_float(v) for v in case["geom"]]
        # through ops
        w, ga, be = dev(wt.T.copy()).requires_grad_(), a["gamma"].clone().requires_grad_(), a["beta"].clone().requires_grad_()
        rm, rv = dev(np.asarray(case["rm0"], np.float32)), dev(np.asarray(case["rv0"], np.float32))
        out = cls.apply(a["vox"], a["num"], a["coords"], w, ga, be, rm, rv, case["eps"], case["momentum"], case["geom"])
        assert type(out.grad_fn).__name__ == cls.__name__ + "Backward"
        saved = out.grad_fn.saved_tensors                          # voxels, num_points, coords, wt, gamma, stats, out, argmax
        out.backward(a["grad_out"])
        want = dict(out=out.detach(), argmax=saved[7], stats=saved[5], running_mean=rm, running_var=rv, d_linear_weight=w.grad,
                    d_norm_weight=ga.grad, d_norm_bias=be.grad)
        if t == 127:
            assert bool((want["argmax"] == 126).any())
        # the older symbols
        dwt = dev(wt)
        rm2, rv2 = dev(np.asarray(case["rm0"], np.float32)), dev(np.asarray(case["rv0"], np.float32))
        out2, arg2 = torch.empty((p, c), device="cuda"), torch.empty((p, c), dtype=torch.int8, device="cuda")
        stats2 = torch.empty((c * (2 + k) + k,), device="cuda")
        dw, dg, db = torch.empty((k, c), device="cuda"), torch.empty((c,), device="cuda"), torch.empty((c,), device="cuda")
        ws = rt.workspace(l.sec_pfn_train_workspace_bytes(p, c), "cuda")
        rc = fwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), p, t, 4, rt.ptr(dwt), rt.ptr(a["gamma"]), rt.ptr(a["beta"]),
                 float(case["eps"]), float(case["momentum"]), rt.ptr(rm2), rt.ptr(rv2), c, *geom, rt.ptr(out2), rt.ptr(arg2), rt.ptr(stats2),
                 rt.ptr(ws), ws.numel(), rt.stream())
        assert rc == 0
        rc = bwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), p, t, 4, rt.ptr(dwt), rt.ptr(a["gamma"]), rt.ptr(stats2), c, *geom,
                 rt.ptr(a["grad_out"]), rt.ptr(out2), rt.ptr(arg2), rt.ptr(dw), rt.ptr(dg), rt.ptr(db), rt.ptr(ws), ws.numel(), rt.stream())
        assert rc == 0
        got = dict(out=out2, argmax=arg2, stats=stats2, running_mean=rm2, running_var=rv2, d_linear_weight=dw.t(), d_norm_weight=dg,
                   d_norm_bias=db)
        for name in want:
            assert torch.equal(got[name], want[name]), ((p, t, c), name)


@pytest.mark.parametrize("radius", [False, True], ids=["plain", "radius"])
def test_existing_rows_through_the_kind_entry_are_bit_equal(radius):
    """The eight older C symbols without a count -- sec_pfn_fwd, sec_pfn_fwd_slots, sec_pfn_train_fwd / _bwd and their radius forms
    -- forward to the launchers of sec_pfn_kind_* with kinds 0 / 1 and no distance.  The Python side calls the kind entry points
    only, so here the older symbols are called through ctypes and must reproduce ops bit for bit (the four _live forms:
    tests/test_gpu_pfn_live.py)."""
    _older_forward(radius)
    _older_forward_slots(radius)
    _older_training(radius)


# ---- slots forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.NEW_ROWS, ids=K.row_id)
@pytest.mark.parametrize("t", [5, 64, 65, 200])
def test_slots_form_is_bit_equal_to_the_tensor_form(t, row):
    """The cloud of _slots_cloud; every z below zero, so a ragged pillar's h has the padded zero as its maximum in both forms (the
    slots form reads slots >= n as zero)."""
    from second_amd import ops
    kind, dist = row
    rng = np.random.default_rng(t)
    pts, offs = _slots_cloud(rng)
    rg, vs = SLOTS_RANGE, SLOTS_VOXEL
    geom = SLOTS_GEOM
    c = 65
    wt = (rng.standard_normal((K.width(kind, dist), c)) / 3).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
    dpts, doffs = dev(pts), dev(offs)
    full = ops.voxelize(dpts, doffs, rg, vs, t, 32, "break", fill=True)
    npv = full["num_points_per_voxel"]
    assert int(npv.max()) == t and int(npv.min()) < t
    for dtk, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        want = ops.pfn_forward(full["voxels"].contiguous(), npv, full["coordinates"], dev(wt), dev(sc), dev(sh), *geom, out_dtype=dt,
                               kind=kind, with_distance=dist)
        case = dict(vox=full["voxels"].cpu().numpy(), num=npv.cpu().numpy(), coords=full["coordinates"].cpu().numpy(), geom=geom, wt=wt,
                    scale=sc, shift=sh)
        assert K.check_eval(want, case, kind, dist, dtk) <= 1.0                       # the tensor form itself is held to float64
        for fill in (False, True):
            v = ops.voxelize(dpts, doffs, rg, vs, t, 32, "break", fill=fill)
            got = ops.pfn_forward_slots(dpts, v, dev(wt), dev(sc), dev(sh), *geom, out_dtype=dt, kind=kind, with_distance=dist)
            assert torch.equal(got, want), (t, dtk, fill)


# ---- training -------------------------------------------------------------------------------------------------------------------
def _train(case, row, backward=True, num_dev=None):
    from second_amd import ops
    kind, dist = row
    cls = ops.pfn_kind_train_function(kind, dist)
    assert issubclass(cls, ops.PFNTrainFunction) and (cls.KIND, cls.WITH_DISTANCE, cls.K) == (kind, dist, K.width(kind, dist))
    wt = K.wt_of(case, kind, dist)
    c = wt.shape[1]
    w, ga, be = dev(wt.T.copy()).requires_grad_(), dev(case["gamma"]).requires_grad_(), dev(case["beta"]).requires_grad_()
    rm, rv = dev(np.asarray(case["rm0"], np.float32)), dev(np.asarray(case["rv0"], np.float32))
    extra = () if num_dev is None else (num_dev,)
    out = cls.apply(dev(case["vox"]), dev(case["num"]), dev(case["coords"]), w, ga, be, rm, rv, case["eps"], case["momentum"], case["geom"], *extra)
    saved = out.grad_fn.saved_tensors                              # voxels, num_points, coords, wt, gamma, stats, out, argmax
    stats, arg = saved[5], saved[7]
    assert arg.dtype == torch.int8 and stats.numel() == c * (2 + wt.shape[0]) + wt.shape[0]
    got = dict(mean=stats[:c], invstd=stats[c:2 * c], out=out.detach(), argmax=arg, running_mean=rm, running_var=rv)
    if backward and case.get("grad_out") is not None:
        out.backward(dev(case["grad_out"]))
        got.update(d_linear_weight=w.grad, d_norm_weight=ga.grad, d_norm_bias=be.grad)
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("row", K.NEW_ROWS, ids=K.row_id)
@pytest.mark.parametrize("case_id", H.TRAIN_CASES, ids=_ids)
def test_training_per_element_against_float64(case_id, row):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    got = _train(case, row)
    res = K.check_train(got, case, *row)
    print("train", case_id, K.row_id(row), {k: f"{v:.3f}" for k, v in res.items()}, "torch f32 constants", case[("constsk",) + row])
    assert set(res) == set(H.FWD_KEYS + H.BWD_KEYS + ("argmax", "gate"))
    if t == 127:
        assert (got["argmax"] == 126).any()                        # the int8 argmax at its last slot
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("row", [(K.OLD, True), (K.RADIUS_HEIGHT, True), (K.RADIUS_HEIGHT, False)], ids=K.row_id)
def test_training_live_count_behind_a_garbage_tail(row):
    """Static capacity: P + 7 rows, of which num_dev are pillars; the tail holds in-range garbage (other pillars' points, counts and
    cells) that must enter no statistic, output or gradient."""
    p, t, c = 33, 9, 64
    base = H.train_case(p + 7, t, c, "plain")
    for live in (0, 1, p - 1, p, p + 7):
        n = min(live, p + 7)
        nd = torch.tensor([live], dtype=torch.int32, device="cuda")
        got = _train(dict(base), row, num_dev=nd)
        assert np.all(got["out"][n:] == 0) and np.all(got["argmax"][n:] == -1)
        if n == 0:
            for k in ("d_linear_weight", "d_norm_weight", "d_norm_bias"):
                assert np.all(got[k] == 0), k
            assert np.array_equal(got["running_mean"], base["rm0"]) and np.array_equal(got["running_var"], base["rv0"])
            continue
        head = {k: (v[:n] if k in ("vox", "num", "coords", "grad_out") else v) for k, v in base.items() if not isinstance(k, tuple)}
        cut = {k: (v[:n] if k in ("out", "argmax") else v) for k, v in got.items()}
        res = K.check_train(cut, head, *row)
        assert max(res.values()) <= 1.0, (live, res)


# ---- the module, the detector, the trainer --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.NEW_ROWS, ids=K.row_id)
def test_module_runs_the_kernels_and_matches_the_fixture(row):
    """models.PillarFeatureNet* on the GPU against what the reference's module computed (tests/golden/pfn_kinds.npz): eval through
    forward, training through the row's class of ops.pfn_kind_train_function, input untouched."""
    from second_amd import models, ops
    kind, dist = row
    g = K.load_fixture()
    case, key = K.fixture_case(g, kind, dist)
    m = models.VFES[K.KIND_NAMES[kind]](4, [16], g["voxel_size"].tolist(), g["pc_range"].tolist(), with_distance=dist)
    layer = m.pfn_layers[0]
    with torch.no_grad():
        layer.linear.weight.copy_(torch.from_numpy(case["wt"].T.copy()))
        for name in ("weight", "bias"):
            getattr(layer.norm, name).copy_(torch.from_numpy(g["norm_" + name]))
        layer.norm.running_mean.copy_(torch.from_numpy(g["running_mean"]))
        layer.norm.running_var.copy_(torch.from_numpy(g["running_var"]))
    m = m.cuda().eval()
    v, n, co = dev(g["voxels"]), dev(g["num_points"]), dev(g["coords"])
    keep = v.clone()
    seen = []
    orig = ops.rt.check
    with torch.no_grad():
        ops.rt.check = lambda rc, name: (seen.append(name), orig(rc, name))[1]
        try:
            out = m(v, n, co)
        finally:
            ops.rt.check = orig
    assert seen == ["sec_pfn_kind_fwd"] and torch.equal(v, keep)
    f32 = dict(case, scale=case["scale"].astype(np.float32), shift=case["shift"].astype(np.float32))
    assert K.check_eval(out, f32, kind, dist, "fp32") <= 1.0
    m.train()
    out = m(v, n, co)
    assert type(out.grad_fn).__name__.startswith("PFNKind") and torch.equal(v, keep)
    out.backward(dev(g["w"]))
    got = dict(out=out.detach(), running_mean=layer.norm.running_mean, running_var=layer.norm.running_var,
               d_linear_weight=layer.linear.weight.grad, d_norm_weight=layer.norm.weight.grad, d_norm_bias=layer.norm.bias.grad)
    res = K.check_train_undecided(got, case, kind, dist)
    print("module", K.row_id(row), res)
    assert max(res.values()) <= 1.0, res


def mida_small(**over):
    """nuscenes/all.pp.mida at +-8 m: 64 x 64 pillars, a 16 x 16 map of 20 anchors per cell.  The 40 best boxes of 200 candidates
    instead of 300 of 1000: on a map this small the stand-in's scores are a dense run (every anchor sees the whole cloud), and the
    comparison below orders detections by their score rounded to four digits."""
    from second_amd.models import ALL_PP_MIDA as c
    cfg = dict(c, point_cloud_range=[-8, -8, -5, 8, 8, 3], anchor_ranges=[[-8, -8, r[2], 8, 8, r[5]] for r in c["anchor_ranges"]],
               max_voxels=4096, nms_pre_max_size=200, nms_post_max_size=40)
    cfg.update(over)
    return cfg


def _clouds(points=600):
    rng = np.random.default_rng(5)
    clouds = []
    for f in range(2):
        centres = rng.uniform(-6, 6, (12, 2))
        p = np.empty((points, 4), np.float32)
        p[:, :2] = centres[rng.integers(0, 12, points)] + rng.normal(0, 0.4, (points, 2))
        p[:, 2] = rng.uniform(-3, 1, points)
        p[:, 3] = rng.uniform(0, 1, points)
        clouds.append(np.clip(p, [-7.9, -7.9, -4.9, 0], [7.9, 7.9, 2.9, 1]).astype(np.float32))
    return clouds


@pytest.fixture(scope="module", params=[False, True], ids=["old", "old+dist"])
def mida(request):
    from reference_standin import build_voxelnet, example_of
    from second_amd import synthetic as syn
    cfg = mida_small(vfe_with_distance=request.param)
    torch.manual_seed(0)
    net = build_voxelnet(cfg)
    syn.randomise_like_trained(net, seed=1)
    net = net.eval().cuda()
    clouds = _clouds()
    ex = example_of(net, clouds, "cuda")
    with torch.no_grad():
        first = ex["coordinates"][:, 0] == 0
        p = net.network_forward(ex["voxels"][first], ex["num_points"][first], ex["coordinates"][first], 1)
        syn.sharpen_heads(net, p["cls_preds"].float(), p["box_preds"].float())
        net.rpn.conv_cls.weight.mul_(0.5)                           # logits -1 .. 6 instead of -2 .. 12: no run of scores at 1.0000
        net.rpn.conv_cls.bias.mul_(0.5)
        keep = ex["voxels"].clone()
        want = net(ex)
        assert torch.equal(ex["voxels"], keep)                      # no centring in place
    return cfg, net, clouds, ex, want


def _as_lists(out):
    res = []
    for b in range(out["valid"].shape[0]):
        m = out["valid"][b]
        res.append({"box3d_lidar": out["boxes"][b][m].float(), "scores": out["scores"][b][m].float(), "label_preds": out["labels"][b][m].long(),
                    "metadata": {"image_idx": 100 + b}})
    return res


def test_detector_forward_points_matches_the_module_graph_eager_and_graphed(mida):
    from test_gpu_dropin_fused import _same
    from second_amd import models, synthetic as syn
    cfg, net, clouds, ex, want = mida
    assert type(net.voxel_feature_extractor) is models.PillarFeatureNetOld
    assert net.voxel_feature_extractor.with_distance == cfg["vfe_with_distance"]
    assert tuple(net.anchors.shape) == (16 * 16 * 20, 7) and net.feature_map_size == [1, 16, 16]
    assert sum(w["scores"].shape[0] for w in want) >= 4
    pts, offs = syn.batch_clouds(clouds)
    pts, offs = dev(pts), dev(offs)
    det = models.SecondDetector(cfg)
    missing = det.load_state_dict({k: v for k, v in net.state_dict().items() if k in det.state_dict()}, strict=False)
    assert not missing.missing_keys
    det = det.cuda().prepare_inference(torch.float32)
    with torch.no_grad():
        e = det.forward_points(pts, offs)
        s = det.forward_points(pts, offs, static=True)
        replay, g = det.make_graphed(pts, offs)
        replay()
        torch.cuda.synchronize()
    for served in (e, s, g):                                        # eager, static capacity, one hipGraph
        _same(_as_lists(served), want, score_tol=2e-4, box_tol=5e-3, canonical=True)


def test_accelerate_model_serves_the_old_network_on_both_lanes(mida):
    from test_gpu_dropin_fused import _same
    from second_amd import compat, dropin, dropin_train
    cfg, net, clouds, ex, want = mida
    c = dropin.model_config(net)
    assert c["vfe"] == "PillarFeatureNetOld" and c["vfe_with_distance"] == cfg["vfe_with_distance"] and c["num_anchor_per_loc"] == 20
    with pytest.raises(dropin_train.NotTrainable):
        dropin_train.FusedTrainStep(net, c, torch.bfloat16)
    for deferred in (False, True):
        assert compat.accelerate_model(net, deferred=deferred) is net
        eng = net._second_amd_engine
        try:
            with torch.no_grad():
                got = net(ex)
                again = net(ex)
            assert eng.stats["original_calls"] == 0 and (eng.stats["deferred_calls"] == 2 if deferred else eng.stats["fused_calls"] == 2)
            _same(again, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
            _same(got, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
            if deferred:
                eng.flush()
        finally:
            del net.forward                                        # the instance attribute accelerate_model put over the class's method
            net._second_amd_engine = None


GT_CLASSES = (1, 2, 6, 10)            # car, bicycle, pedestrian (distance similarity), barrier


def _batch(det, points=600, seed=0):
    from second_amd.models import anchor_class_ranges
    rng = np.random.default_rng(seed)
    begin = anchor_class_ranges(det.cfg, det.feature_map_size)
    anc = det.anchors.cpu().numpy()
    clouds = _clouds(points)
    gts = []
    for _ in clouds:
        boxes = []
        for c in GT_CLASSES:
            seg = anc[begin[c - 1]:begin[c]]
            seg = seg[(np.abs(seg[:, 0]) < 6) & (np.abs(seg[:, 1]) < 6)]
            boxes.append(seg[rng.integers(len(seg))])
        b = np.stack(boxes).astype(np.float32)
        b[:, :2] += rng.normal(0, 0.03, (len(b), 2)).astype(np.float32)
        gts.append(b)
    arrays = (np.concatenate(clouds), np.array([0, points, 2 * points], np.int32), np.concatenate(gts), np.array([0, 4, 8], np.int32),
              np.array(GT_CLASSES * 2, np.int32))
    return tuple(dev(a) for a in arrays)


@pytest.fixture
def reproducible_convs():
    """Two executions of one step are compared: MIOpen's default solvers are not reproducible run to run (tests/test_gpu_mhead_train.py)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _fp32_formulation(vfe):
    """The module's torch formulation outside autocast (the precision of the kernels it is compared with)."""
    inner = vfe._forward_torch

    def fp32(*args):
        with torch.autocast("cuda", enabled=False):
            return inner(*args)
    vfe._forward_torch = fp32


@pytest.mark.parametrize("dist", [False, True], ids=["old", "old+dist"])
def test_layer_gradients_agree_on_the_same_upstream_gradient(dist, reproducible_convs):
    """One fp32 DeviceTrainer step per backend; then each backend's layer is run again on its own inputs with the OTHER run's
    gradient at the layer's output: it reproduces the other backend's parameter gradients (2e-3 of test_pfn_training_kernels_vs_
    torch_autograd; measured 8e-7), so whatever separates the two steps' gradients enters above the layer."""
    from second_amd import models
    from second_amd.training import DeviceTrainer
    runs, args = {}, None
    for backend in ("torch", "hip"):
        torch.manual_seed(0)
        det = models.SecondDetector(mida_small(vfe_with_distance=dist)).cuda()
        vfe = det.voxel_feature_extractor
        vfe.train_backend = backend
        tr = DeviceTrainer(det, lr=1e-3)
        args = args or _batch(det)
        keep = {}

        def hook(m, i, o, keep=keep):
            keep["in"] = [t.detach().clone() for t in i[:3]]
            o.register_hook(lambda g: keep.__setitem__("g", g.detach().float().clone()))
        h = vfe.register_forward_hook(hook)
        loss, _, _ = tr.forward_loss(*args)
        loss.backward()
        h.remove()
        l = vfe.pfn_layers[0]
        keep.update(vfe=vfe, dw=l.linear.weight.grad.clone(), dg=l.norm.weight.grad.clone(), db=l.norm.bias.grad.clone())
        runs[backend] = keep
    for mine, other in (("torch", "hip"), ("hip", "torch")):
        vfe = runs[mine]["vfe"]
        for p in vfe.parameters():
            p.grad = None
        vfe(*runs[mine]["in"]).backward(runs[other]["g"])
        l = vfe.pfn_layers[0]
        for k, g in (("dw", l.linear.weight.grad), ("dg", l.norm.weight.grad), ("db", l.norm.bias.grad)):
            err = float((g - runs[other][k]).abs().max()) / max(float(runs[other][k].abs().max()), 1e-6)
            print("layer", mine, "on the gradient of", other, k, f"{err:.2e}")
            assert err <= 2e-3, (mine, k, err)


class _Gate(torch.nn.Module):
    """A ReLU of the RPN whose decisions can be carried from one run to another: "record" is a ReLU that keeps its gates (x > 0);
    "follow" applies the gates it was given (forward x * gate, backward dy * gate) and keeps its own for the comparison."""
    CONTEST = 1e-4      # see test_device_trainer_step_...: how close to zero a pre-activation must be for its gate to count as open

    def __init__(self):
        super().__init__()
        self.mode, self.gate, self.own, self.pre = "record", None, None, None

    def forward(self, x):
        self.pre = x.detach()
        self.own = self.pre > 0
        if self.mode == "follow":
            return x * self.gate.to(x.dtype)
        self.gate = self.own
        return torch.relu(x)


def _gates(det):
    """Every ReLU of det.rpn's blocks and deblocks replaced by a _Gate (no parameters: the state dict is what it was)."""
    gates = []
    for seq in list(det.rpn.blocks) + list(det.rpn.deblocks):
        for i, m in enumerate(seq):
            if isinstance(m, torch.nn.ReLU):
                seq[i] = _Gate()
                gates.append(seq[i])
    assert len(gates) == 19
    return gates


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dist", [False, True], ids=["old", "old+dist"])
def test_device_trainer_step_hip_backend_matches_torch_backend_and_learns(dist, amp, reproducible_convs):
    """DeviceTrainer's pillar branch calls det.voxel_feature_extractor(...) as a module: with the module on the kind kernels the step
    gives the loss and the PFN gradients of the materialised torch formulation (the tolerances of
    tests/test_gpu_train.py::test_pfn_training_kernels_vs_torch_autograd: loss as its ``out``, 2e-4; gradients 2e-3; running
    statistics 1e-5, each relative to the quantity's maximum), and the loss falls over 20 steps.
    bf16: the kernels compute in fp32 whatever the autocast state, so the torch formulation they are compared with is held in fp32
    too (autocast off around it; under autocast its Linear runs in bf16 and its own running_mean is 1.9e-3 off).  Measured: 7e-7
    (dw), 2e-7 (dg), 2e-8 (db).
    fp32: the comparison is decision-aware, like check_train is for the layer's own argmax and ReLU gate.  Measured on an MI355X:
    the two formulations' outputs differ by 5e-7 of their maximum and the loss is equal to the last bit or to 9e-8, but in about one
    process in three the layer's gradients differed by 1.0e-2 (dw), 1.5e-2 (dg), 6.6e-3 (db) and the weight gradient of
    rpn.blocks.2.10 by 1.2e-1, everything behind that layer to 2e-5: the BatchNorm output in front of the ReLU rpn.blocks.2.12 (2 x 8 x 8
    cells) holds three values below 1e-5, and one of them lies on either side of zero in the two runs -- one gate of the RPN, not the
    layer under test, decides 1 % of the gradient that reaches it (tests/test_gpu_mhead_train.py's reproducible_convs describes
    the same for its geometry; which processes show it follows the convolution library's choices, not this code: all runs of one
    process are bit-reproducible).  So the hip step runs first and every ReLU of the RPN records its gates; the torch step
    FOLLOWS them, and every gate on which the torch step itself would have decided otherwise must be contested: both runs'
    pre-activations within _Gate.CONTEST = 1e-4 of zero.  Why 1e-4: the pre-activations are BatchNorm outputs of unit variance;
    inputs that agree to a few ulp (2^-23) pass at most 19 convolutions of fan-in up to 2304 with their BatchNorms, and 2^-13 leaves
    a factor 2^10 for that -- while a gate that differs for any other reason (a wrong row, a wrong mean) sits at O(1).  With the
    decisions shared, loss, gradients and running statistics are held to the tolerances above, unchanged."""
    from second_amd import models
    from second_amd.training import DeviceTrainer
    res, args, gates = {}, None, {}
    for backend in ("hip", "torch"):
        torch.manual_seed(0)
        det = models.SecondDetector(mida_small(vfe_with_distance=dist)).cuda()
        det.voxel_feature_extractor.train_backend = backend
        if amp is not None:
            _fp32_formulation(det.voxel_feature_extractor)
        else:
            gates[backend] = _gates(det)
            if backend == "torch":
                for mine, theirs in zip(gates["torch"], gates["hip"]):
                    mine.mode, mine.gate = "follow", theirs.step_gate
        tr = DeviceTrainer(det, lr=1e-3, amp_dtype=amp)
        assert tr.similarities is not None and tr.class_ranges is not None
        args = args or _batch(det)
        keep = args[0].clone()
        loss, out6, labels = tr.forward_loss(*args)
        loss.backward()
        assert torch.equal(args[0], keep)
        l = det.voxel_feature_extractor.pfn_layers[0]
        assert set(np.unique(labels.cpu().numpy()).tolist()) >= {0, 1, 2, 6, 10}
        res[backend] = dict(loss=loss.detach().float().cpu().reshape(1), dw=l.linear.weight.grad.detach().cpu().clone(),
                            dg=l.norm.weight.grad.detach().cpu().clone(), db=l.norm.bias.grad.detach().cpu().clone(),
                            rm=l.norm.running_mean.detach().cpu().clone(), rv=l.norm.running_var.detach().cpu().clone())
        if amp is None:
            for g in gates[backend]:                                # keep this step's decisions: the steps below overwrite them
                g.step_gate, g.step_own, g.step_pre = g.gate, g.own, g.pre
        if backend == "hip":
            for p in det.parameters():
                p.grad = None
            tr.bucket.zero_grad()
            losses = [float(tr.step(*args)[0]) for _ in range(20)]
            print("losses", losses[0], losses[-1])
            assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    if amp is None:
        contested = 0
        for i, (t, h) in enumerate(zip(gates["torch"], gates["hip"])):
            assert torch.equal(t.step_gate, h.step_gate)            # the torch step followed the hip step's decisions ...
            differ = t.step_own != h.step_gate                      # ... and where it would have decided otherwise itself,
            contested += int(differ.sum())
            assert int(differ.sum()) <= 4, (i, int(differ.sum()))   # it is a handful of values at zero, not a layer that went astray
            if bool(differ.any()):
                near = torch.maximum(t.step_pre[differ].abs(), h.step_pre[differ].abs())
                assert float(near.max()) <= _Gate.CONTEST, (i, float(near.max()))
        print("contested RPN gates", contested)
    a, b = res["torch"], res["hip"]
    errs = {}
    for k, tol in (("loss", 2e-4), ("dw", 2e-3), ("dg", 2e-3), ("db", 2e-3), ("rm", 1e-5), ("rv", 1e-5)):
        scale = max(a[k].abs().max().item(), 1e-6)
        errs[k] = ((a[k] - b[k]).abs().max().item() / scale, tol)
    print("trainer", "old+dist" if dist else "old", amp, {k: f"{e:.2e}" for k, (e, _) in errs.items()})
    assert float(a["dw"].abs().max()) > 0
    assert all(e <= tol for e, tol in errs.values()), errs
