"""nuscenes/all.pp.mhead on the fused path (GPU): the PillarFeatureNetRadius kernel, select / decode over several head tensors, the
head-less trunk with its two heads, and the whole detector against the stand-in's module graph (tests/reference_standin_mhead.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VS, XO, YO = 0.25, 0.125 - 50, 0.125 - 50


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


# ------------------------------------------------------------------------------------------ PillarFeatureNetRadius
def pfn_radius_f64(vox, n, coords, wt, scale, shift, vx, vy, xo, yo):
    """float64 restatement of PillarFeatureNetRadius.forward + PFNLayer (eval) from pointpillars.py:290-325, 51-65."""
    vox, wt, scale, shift = (np.asarray(a, np.float64) for a in (vox, wt, scale, shift))
    p, t, _ = vox.shape
    mean = vox[:, :, :3].sum(1, keepdims=True) / n.reshape(-1, 1, 1).astype(np.float64)
    cx = coords[:, 3].astype(np.float64)[:, None] * vx + xo
    cy = coords[:, 2].astype(np.float64)[:, None] * vy + yo
    dec = np.concatenate([np.sqrt(vox[:, :, 0:1] ** 2 + vox[:, :, 1:2] ** 2), vox[:, :, 2:], vox[:, :, :3] - mean,
                          (vox[:, :, 0] - cx)[..., None], (vox[:, :, 1] - cy)[..., None]], -1)
    dec *= (np.arange(t)[None, :] < n[:, None])[..., None]
    return np.maximum((dec @ wt) * scale + shift, 0).max(1)


def _random_pillars(p, t, c, seed):
    rng = np.random.default_rng(seed)
    vox = rng.uniform(-3, 3, (p, t, 4)).astype(np.float32)
    n = rng.integers(1, t + 1, p).astype(np.int32)
    n[:min(10, p)] = t
    if p > 20:
        n[10:20] = 1
        vox[20, 0, :2] = 0.0                                    # a point on the sensor axis: radius exactly 0
    vox *= (np.arange(t)[None, :] < n[:, None])[..., None]
    coords = np.stack([rng.integers(0, 4, p), np.zeros(p, int), rng.integers(0, 400, p), rng.integers(0, 400, p)], 1).astype(np.int32)
    wt = (rng.standard_normal((8, c)) / 3).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
    return vox, n, coords, wt, sc, sh


def test_pfn_radius_kernel_matches_the_reference_module(ops, golden):
    g = golden("mhead")
    w = g["pfn_sd.pfn_layers.0.linear.weight"]
    bw, bb, rm, rv = [g["pfn_sd.pfn_layers.0.norm." + k] for k in ("weight", "bias", "running_mean", "running_var")]
    scale = bw / np.sqrt(rv + g["pfn_eps"])
    shift = bb - rm * scale
    n = g["pfn_num_points"]
    assert n.min() == 1 and n.max() == 60 and g["pfn_voxels"].shape == (64, 60, 4)
    out = ops.pfn_radius_forward(dev(g["pfn_voxels"]), dev(n), dev(g["pfn_coords"]), dev(w.T.copy()), dev(scale), dev(shift), VS, VS, XO, YO)
    np.testing.assert_allclose(out.cpu().numpy(), g["pfn_out"], rtol=1e-4, atol=1e-5)      # the reference's own module


def test_pfn_radius_kernel_vs_float64_and_edge_cases(ops):
    p, t, c = 3000, 60, 64
    vox, n, coords, wt, sc, sh = _random_pillars(p, t, c, 0)
    ref = pfn_radius_f64(vox, n, coords, wt, sc, sh, VS, VS, XO, YO)
    args = (dev(wt), dev(sc), dev(sh), VS, VS, XO, YO)
    out = ops.pfn_radius_forward(dev(vox), dev(n), dev(coords), *args)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    assert n[20] >= 1 and vox[20, 0, 0] == 0 and vox[20, 0, 1] == 0 and (n[:10] == t).all() and (n[10:20] == 1).all()
    # one pillar
    one = ops.pfn_radius_forward(dev(vox[:1]), dev(n[:1]), dev(coords[:1]), *args)
    assert torch.equal(one, out[:1])
    # num_dev < P: rows past it stay untouched
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        full = ops.pfn_radius_forward(dev(vox), dev(n), dev(coords), *args, out_dtype=dt)
        np.testing.assert_allclose(full.float().cpu().numpy(), ref, rtol=2 ** -7 if dt != torch.float32 else 1e-4, atol=2 ** -7 if dt != torch.float32 else 1e-4)
        assert torch.equal(full, out.to(dt))                                         # the 16-bit forms round the fp32 result
        from second_amd import runtime as rt
        buf = torch.full((p, c), 7.0, dtype=dt, device="cuda")
        nd = torch.tensor([1234], dtype=torch.int32, device="cuda")
        dv, dn, dc = dev(vox), dev(n), dev(coords)
        rc = rt.lib().sec_pfn_radius_fwd(rt.ptr(dv), rt.ptr(dn), rt.ptr(dc), p, rt.ptr(nd), t, 4, rt.ptr(args[0]), rt.ptr(args[1]),
                                         rt.ptr(args[2]), c, VS, VS, XO, YO, rt.ptr(buf), rt.dtype_code(dt), rt.stream())
        rt.check(rc, "sec_pfn_radius_fwd")
        assert torch.equal(buf[:1234], full[:1234]) and bool((buf[1234:] == 7.0).all())
    # the weight must be [F + 4, C]; the Cartesian kernel is another function
    with pytest.raises(AssertionError):
        ops.pfn_forward(dev(vox), dev(n), dev(coords), *args)


def test_pfn_radius_slots_form_is_bit_identical(ops):
    from second_amd import synthetic as syn
    from second_amd.models import ALL_PP_MHEAD as C
    rng_, vs = C["point_cloud_range"], C["voxel_size"]
    cloud = syn.syn_nusc_cloud(5, 60000, tuple(rng_))
    pts, offs = syn.batch_clouds([cloud, cloud[::3]])
    pts, offs = dev(pts), dev(offs)
    _, _, _, wt, sc, sh = _random_pillars(1, 60, 64, 3)
    xo, yo = vs[0] / 2 + rng_[0], vs[1] / 2 + rng_[1]
    full = ops.voxelize(pts, offs, rng_, vs, C["max_points_per_voxel"], C["max_voxels"], "break", fill=True)
    p = full["voxel_num"]
    assert p > 5000 and int(full["num_points_per_voxel"].max()) > 1
    want = ops.pfn_radius_forward(full["voxels"][:p].contiguous(), full["num_points_per_voxel"][:p].contiguous(), full["coordinates"][:p].contiguous(),
                                  dev(wt), dev(sc), dev(sh), vs[0], vs[1], xo, yo)
    for fill in (False, True):
        v2 = ops.voxelize(pts, offs, rng_, vs, C["max_points_per_voxel"], C["max_voxels"], "break", fill=fill)
        for dt in (torch.float32, torch.bfloat16):
            got = ops.pfn_forward_slots(pts, v2, dev(wt), dev(sc), dev(sh), vs[0], vs[1], xo, yo, out_dtype=dt, radius=True)
            assert torch.equal(got[:p], want.to(dt))


# ------------------------------------------------------------------------------------------ select / decode over segments
def _padded_views(maps, b, nc, dtype, seed, fill=None):
    """Per map (A, H, W): cls / box / dir views [B, A, H, W, code] into one channel-padded NHWC head tensor, as RPNInference hands them out."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    # class logits: ONE shuffled grid over [-5, 1.5] shared by all maps -- two thirds above the 0.05 threshold's logit, and every two
    # values at least 7e-5 apart, so that their fp32 sigmoids are ordered like the logits (torch.topk ranks scores, the kernels logits)
    total = sum(b * a * nc * h * w for a, h, w in maps)
    grid = torch.linspace(-5.0, 1.5, total, device="cuda")[torch.randperm(total, device="cuda", generator=g)]
    for a, h, w in maps:
        tot = a * (7 + nc + 2)
        cpad = tot + (-tot) % 64
        t = torch.randn(b, cpad, h, w, device="cuda", generator=g)
        m = b * a * nc * h * w
        t[:, a * 7:a * (7 + nc)] = grid[:m].reshape(b, a * nc, h, w)
        grid = grid[m:]
        t[:, :a * 7] *= 0.2
        if fill is not None:
            fill(t, a, len(out))
        t = t.to(dtype).contiguous(memory_format=torch.channels_last)
        c0, views = 0, {}
        for name, code in (("box", 7), ("cls", nc), ("dir", 2)):
            views[name] = t[:, c0:c0 + a * code].reshape(b, a, code, h, w).permute(0, 1, 3, 4, 2)
            c0 += a * code
        out.append(views)
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(3, 5, 7), (12, 100, 100)])
def test_one_segment_equals_the_single_map_entry_points(ops, shape, dtype):
    (v,) = _padded_views([shape], 2, 10, dtype, 1)
    n = shape[0] * shape[1] * shape[2]
    anchors = torch.randn(n, 7, device="cuda").abs() + 0.5
    for thr in (0.05, 0.5):
        one = ops.predict_select(v["cls"], 1000, thr)
        seg = ops.predict_select([v["cls"]], 1000, thr)
        for a, b in zip(one, seg):
            assert torch.equal(_bits(a), _bits(b))
        for rotate in (True, False):
            d1 = ops.predict_decode(v["box"], v["dir"], anchors, one[0], one[1], rotate=rotate)
            d2 = ops.predict_decode([v["box"]], [v["dir"]], anchors, seg[0], seg[1], rotate=rotate)
            for a, b in zip(d1, d2):
                assert torch.equal(_bits(a), _bits(b))
    assert int(one[3].min()) >= 0


def _reference_select(views, b, nc, k, thr, anchors):
    """SecondDetector._select (the torch formulation of voxelnet.py:545-569) on the concatenated [B, N, C] tensors."""
    from second_amd.models import SecondDetector, ALL_PP_LARGEA
    det = SecondDetector.__new__(SecondDetector)
    torch.nn.Module.__init__(det)
    det.cfg = dict(ALL_PP_LARGEA, num_class=nc, nms_pre_max_size=k, nms_score_threshold=thr)
    preds = {"cls_preds": torch.cat([v["cls"].reshape(b, -1, nc) for v in views], 1).float(),
             "box_preds": torch.cat([v["box"].reshape(b, -1, 7) for v in views], 1).float(),
             "dir_cls_preds": torch.cat([v["dir"].reshape(b, -1, 2) for v in views], 1).float()}
    dec, top_scores, counts, dir_labels, top_labels = det._select(preds, b, anchors)
    scores = torch.sigmoid(preds["cls_preds"]).max(-1).values if nc > 1 else torch.sigmoid(preds["cls_preds"][..., 0])
    return preds, dec, top_scores, counts, dir_labels, top_labels, scores


def _check_segments(ops, views, b, nc, k, thr, tie_free=True):
    n = sum(v["cls"].shape[1] * v["cls"].shape[2] * v["cls"].shape[3] for v in views)
    ga = torch.Generator(device="cuda").manual_seed(9)
    anchors = torch.rand(n, 7, device="cuda", generator=ga) + 0.5
    top_idx, top_score, top_label, counts = ops.predict_select([v["cls"] for v in views], k, thr)
    preds, dec_ref, ref_scores, ref_counts, ref_dir, ref_labels, scores = _reference_select(views, b, nc, min(k, n, 1024), thr, anchors)
    assert torch.equal(counts, ref_counts), (counts, ref_counts)
    assert top_idx.shape[1] == min(k, n, 1024)
    # stable order by descending logit, ties by ascending global index: what the kernels document
    best = preds["cls_preds"].max(-1).values
    order = torch.sort(best, dim=1, descending=True, stable=True).indices
    dec, dets, dlab = ops.predict_decode([v["box"] for v in views], [v["dir"] for v in views], anchors, top_idx, top_score, rotate=False)
    for f in range(b):
        c = int(counts[f])
        idx = top_idx[f, :c].long()
        assert torch.equal(idx, order[f, :c]), f
        np.testing.assert_allclose(top_score[f, :c].cpu().numpy(), ref_scores[f, :c].cpu().numpy(), rtol=1e-6)
        assert torch.equal(top_label[f, :c].long(), preds["cls_preds"][f, idx].max(-1).indices)
        if tie_free:
            assert torch.equal(top_label[f, :c].long(), ref_labels[f, :c].long())
            np.testing.assert_allclose(dec[f, :c].cpu().numpy(), dec_ref[f, :c].cpu().numpy(), rtol=1e-5, atol=1e-5)
            assert torch.equal(dlab[f, :c].long(), ref_dir[f, :c].long())
        # decode of the rows it selected, whatever the tie order: decode_boxes + direction argmax on the gathered rows
        from second_amd.models import decode_boxes
        want = decode_boxes(preds["box_preds"][f, idx], anchors[idx])
        np.testing.assert_allclose(dec[f, :c].cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-5)
        assert torch.equal(dlab[f, :c].long(), preds["dir_cls_preds"][f, idx].max(-1).indices)
        np.testing.assert_allclose(dets[f, :c, 4].cpu().numpy(), top_score[f, :c].cpu().numpy(), rtol=0, atol=0)
    return counts


# the issue's two pairs (the 32-bit and the 16-bit register forms) + one of 19 200 + 32 768 anchors, which 16-bit heads select in
# 8 192-anchor chunks: the border between the maps falls inside a chunk (and inside a wave's run of pairs)
SEG_MAPS = [[(3, 5, 7), (2, 9, 6)], [(12, 9, 6), (8, 28, 16)], [(12, 40, 40), (8, 64, 64)]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nc", [1, 10])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("maps", SEG_MAPS)
def test_two_segments_match_the_torch_selection_on_the_concatenation(ops, maps, b, nc, dtype):
    # 16-bit logits tie, and torch.topk's tie order is its own; so do fp32 SCORES once the grid of logits is finer than ~2e-5 (the
    # largest case): the order is then checked against the stable sort by logit alone, counts and scores still against _select
    values = sum(b * a * nc * h * w for a, h, w in maps)
    tie_free = dtype == torch.float32 and values <= 200000
    views = _padded_views(maps, b, nc, dtype, 2)
    counts = _check_segments(ops, views, b, nc, 1000, 0.05, tie_free)
    n0 = maps[0][0] * maps[0][1] * maps[0][2]
    n = n0 + maps[1][0] * maps[1][1] * maps[1][2]
    assert int(counts.min()) > 0
    # k larger than N (the small maps) / smaller than the candidates
    _check_segments(ops, views, b, nc, 5000, 0.05, tie_free)
    _check_segments(ops, views, b, nc, 7, 0.05, tie_free)
    # every anchor over the threshold (logits >= -2.8, the threshold's is -2.94; the larger maps have 4 232 anchors, more than 1 024): counts == k
    hot = _padded_views(maps, b, nc, dtype, 3, fill=lambda t, a, s: t[:, a * 7:a * (7 + nc)].add_(2.2))
    c = _check_segments(ops, hot, b, nc, 1000, 0.05, tie_free)
    assert int(c.min()) == min(1000, n)
    # every candidate in the second segment
    def second_only(t, a, s):
        if s == 0:
            t[:, a * 7:a * (7 + nc)] -= 20.0
    late = _padded_views(maps, b, nc, dtype, 4, fill=second_only)
    top_idx, _, _, c = ops.predict_select([v["cls"] for v in late], 1000, 0.05)
    assert int(c.min()) > 0 and all(int(top_idx[f, :int(c[f])].min()) >= n0 for f in range(b))
    _check_segments(ops, late, b, nc, 1000, 0.05, tie_free)
    # equal logits on the last anchor of segment 0 and the first of segment 1: the lower global index ranks first
    def tie(t, a, s):
        cls = t[:, a * 7:a * (7 + nc)]
        cls -= 20.0
        if s == 0:
            cls[:, (a - 1) * nc:, -1, -1] = 2.5            # anchor (A - 1, H - 1, W - 1): global index n0 - 1
        else:
            cls[:, :nc, 0, 0] = 2.5                        # anchor (0, 0, 0): global index n0
    tied = _padded_views(maps, b, nc, dtype, 5, fill=tie)
    top_idx, top_score, _, c = ops.predict_select([v["cls"] for v in tied], 1000, 0.05)
    assert c.tolist() == [2] * b and top_idx[:, :2].tolist() == [[n0 - 1, n0]] * b and bool((top_score[:, 0] == top_score[:, 1]).all())
    # no candidate at all
    none = _padded_views(maps, b, nc, dtype, 6, fill=lambda t, a, s: t[:, a * 7:a * (7 + nc)].sub_(20.0))
    assert ops.predict_select([v["cls"] for v in none], 1000, 0.05)[3].tolist() == [0] * b


# ------------------------------------------------------------------------------------------ trunk and heads
def test_trunk_and_heads_match_the_module_graph():
    from reference_standin_mhead import module_graph_dense
    from mhead_helpers import standin
    from second_amd.models import ALL_PP_MHEAD, MultiHeadInference, stage0_crop
    net = standin(ALL_PP_MHEAD).eval().cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(2, 64, 72, 48, device="cuda", generator=g).abs()
    assert stage0_crop(36) == 4 and int(36 * 0.1) == 3                       # rounded, not floored
    with torch.no_grad():
        s0 = net.rpn.blocks[0](x)
        assert tuple(s0.shape) == (2, 64, 36, 24)
        large_want, small_want = module_graph_dense(net, x)
        assert small_want["cls_preds"].shape == (2, 8 * 28 * 16, 10) and large_want["cls_preds"].shape == (2, 12 * 18 * 12, 10)
        f32 = MultiHeadInference(net.rpn, net.large_head, net.small_head, torch.float32)
        bf = MultiHeadInference(net.rpn, net.large_head, net.small_head, torch.bfloat16)
        assert bf.use_hip and bf.tower.head_cout == 192 and bf.trunk.head_cout == 256
        got32 = f32(x.contiguous(memory_format=torch.channels_last))
        got16 = bf(x.bfloat16().contiguous(memory_format=torch.channels_last))
        # the border rule: stage 0 scaled by 100 OUTSIDE the crop.  The module graph slices, so its tower zero-pads at the crop's
        # border; a tower conv of the inference form that read stage-0 cells across that border would be off by far more than the bound
        m = torch.full_like(s0, 100.0)
        m[:, :, 4:-4, 4:-4] = 1.0
        boosted = (s0 * m).contiguous(memory_format=torch.channels_last)
        assert torch.equal(boosted[:, :, 4:-4, 4:-4], s0[:, :, 4:-4, 4:-4]) and float(boosted.abs().max()) > 50 * float(s0.abs().max())
        border32, border16 = f32.small_head_of(boosted), bf.small_head_of(boosted.bfloat16())
        got32 = {k: [got32[k][0], got32[k][1], border32[k]] for k in got32}
        got16 = {k: [got16[k][0], got16[k][1], border16[k]] for k in got16}
    for got, is16 in ((got32, False), (got16, True)):
        for k in ("box_preds", "cls_preds", "dir_cls_preds"):
            assert len(got[k]) == 3
            for view, want in zip(got[k], (large_want[k], small_want[k], small_want[k])):
                flat = view.reshape(2, -1, view.shape[-1]).float()
                assert flat.shape == want.shape
                if is16:
                    err = (flat - want).abs().max().item() / want.abs().max().item()
                    assert err < 4e-2, (k, err)
                else:
                    np.testing.assert_allclose(flat.cpu().numpy(), want.cpu().numpy(), rtol=2e-3, atol=2e-4)
    # default-eps norms: folding with 1e-3 instead would be far outside the bound
    bn = net.small_head.net[1]
    assert bn.eps == 1e-5 and float((torch.rsqrt(bn.running_var + 1e-5) / torch.rsqrt(bn.running_var + 1e-3)).max()) > 1.5
    with pytest.raises(ValueError, match="crop"):
        stage0_crop(4)


# ------------------------------------------------------------------------------------------ whole detector
@pytest.fixture(scope="module")
def mhead():
    from mhead_helpers import trained_like_standin
    from reference_standin import example_of
    from second_amd import synthetic as syn
    from second_amd.models import ALL_PP_MHEAD
    cloud = syn.syn_nusc_cloud(0, num_points=60000, point_cloud_range=tuple(ALL_PP_MHEAD["point_cloud_range"]))
    clouds = [cloud, cloud[::3]]
    net = trained_like_standin(ALL_PP_MHEAD, cloud)
    ex = example_of(net, clouds, "cuda")
    with torch.no_grad():
        want = net(ex)
    return net, clouds, ex, want


def _as_lists(out):
    res = []
    for b in range(out["valid"].shape[0]):
        m = out["valid"][b]
        res.append({"box3d_lidar": out["boxes"][b][m].float(), "scores": out["scores"][b][m].float(), "label_preds": out["labels"][b][m].long(),
                    "metadata": {"image_idx": 100 + b}})
    return res


def test_detector_forward_points_matches_the_module_graph_eager_static_and_graphed(mhead):
    from test_gpu_dropin_fused import _found, _same
    from second_amd import synthetic as syn
    from second_amd.models import ALL_PP_MHEAD, MultiHeadInference, SecondDetector
    net, clouds, ex, want = mhead
    assert sum(w["scores"].shape[0] for w in want) >= 6
    labels = torch.cat([w["label_preds"] for w in want])
    assert bool((labels < 5).any()) and bool((labels >= 5).any())                      # classes of both heads
    pts, offs = syn.batch_clouds(clouds)
    pts, offs = dev(pts), dev(offs)
    sd = net.state_dict()
    results = {}
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        det = SecondDetector(ALL_PP_MHEAD)
        assert tuple(det.anchors.shape) == (324800, 7)
        missing = det.load_state_dict({k: v for k, v in sd.items() if k in det.state_dict()}, strict=False)
        assert not missing.missing_keys
        det = det.cuda().prepare_inference(dt)
        assert isinstance(det.rpn, MultiHeadInference) and (dt == torch.float32 or det.rpn.use_hip)
        with torch.no_grad():
            e = det.forward_points(pts, offs)
            s = det.forward_points(pts, offs, static=True)
            replay, g = det.make_graphed(pts, offs)
            replay()
            torch.cuda.synchronize()
        for other in (s, g):
            assert torch.equal(e["valid"], other["valid"])
            m = e["valid"]
            assert torch.equal(e["scores"][m], other["scores"][m]) and torch.equal(e["boxes"][m], other["boxes"][m])
            assert torch.equal(e["labels"][m], other["labels"][m])
        results[dt] = _as_lists(e)
    _same(results[torch.float32], want, score_tol=2e-4, box_tol=5e-3, canonical=True)
    for dt in (torch.bfloat16, torch.float16):
        hit, tot = _found(results[dt], results[torch.float32])
        assert tot >= 6 and hit >= 0.85 * tot, (dt, hit, tot)


def test_accelerate_model_serves_the_multi_head_network(mhead):
    from test_gpu_dropin_fused import _same
    from second_amd import compat, dropin, dropin_train, models, training
    net, clouds, ex, want = mhead
    cfg = dropin.model_config(net)
    for k in set(cfg) & set(models.ALL_PP_MHEAD) - {"name"}:
        a, b = cfg[k], models.ALL_PP_MHEAD[k]
        if isinstance(a, float) or (isinstance(a, list) and a and isinstance(a[0], float)):
            np.testing.assert_allclose(a, b, rtol=1e-6, err_msg=k)           # values the network keeps in float32
        else:
            assert a == b, (k, a, b)
    assert cfg["vfe"] == "PillarFeatureNetRadius" and cfg["rpn_class"] == "RPNNoHead" and [h["num_anchor_per_loc"] for h in cfg["heads"]] == [12, 8]
    with pytest.raises(dropin_train.NotTrainable, match="multi-head"):
        dropin_train.FusedTrainStep(net, cfg, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="multi-head"):
        training.DeviceTrainer(models.SecondDetector(models.ALL_PP_MHEAD))
    assert compat.accelerate_model(net) is net
    eng = net._second_amd_engine
    try:
        with torch.no_grad():
            got = net(ex)
        assert eng.stats["fused_calls"] == 1 and eng.stats["original_calls"] == 0 and eng.stats["captures"] == 1
        _same(got, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
        net.train()
        assert not eng.accepts(ex)                         # training mode keeps the object's own forward
        net.eval()
    finally:
        del net.forward                                    # the instance attribute accelerate_model put over the class's method
        net._second_amd_engine = None                      # (accelerate_model leaves an accelerated network as it is)
    # the deferred lanes: the call returns at once, the dicts fill themselves when read
    compat.accelerate_model(net, deferred=True)
    eng = net._second_amd_engine
    try:
        with torch.no_grad():
            first, second = net(ex), net(ex)
        assert eng.stats["deferred_calls"] == 2 and eng.stats["original_calls"] == 0
        _same(second, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
        _same(first, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
        eng.flush()
    finally:
        del net.forward
        net._second_amd_engine = None
