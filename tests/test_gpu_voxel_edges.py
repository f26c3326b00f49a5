"""-m gpu: csrc/voxelize.hip against exact references at every boundary of its forms (tests/voxel_ref_helpers.py; the references, the
generators and the planted mistakes are held on the CPU by tests/test_voxel_ref_host.py).

Every case goes through ``ops.voxelize`` twice in a row -- the kernels are atomics and spin-waits: both runs must give the same bits --
and is compared with ``assert_voxelize_equal``: offsets, coordinates, counts and the voxel tensor's bit patterns exactly, the mean bit
for bit with the fp32 restatement of the kernels' operation order after one rounding and inside the derived float64 bound.  Calls
without a voxel tensor are compared as tests/test_gpu_parity.py compares the pillar path: offsets, coordinates and counts exactly,
and the PillarFeatureNet read through the point lists bit-equal to the one read from the reference's voxel tensor.
"""
import numpy as np
import pytest
import torch

import voxel_ref_helpers as H

pytestmark = pytest.mark.gpu

KEYS = ("voxels", "coordinates", "num_points_per_voxel", "voxel_offsets", "mean")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


def _batch(clouds, spare=None):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    return np.concatenate(list(clouds) + ([spare] if spare is not None else [])).astype(np.float32), offs


def _bits_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    return torch.equal(a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16),
                       b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16))


def _same(a, b):
    for k in KEYS:
        if a.get(k) is not None:
            assert _bits_equal(a[k], b[k]), f"two runs in a row differ in {k}"


def _twice(ops, pts, offs, geo, T, V, cap_mode, **kw):
    a = ops.voxelize(pts, offs, geo[0], geo[1], T, V, cap_mode, **kw)
    a = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}      # (the second call reuses nothing of the first)
    b = ops.voxelize(pts, offs, geo[0], geo[1], T, V, cap_mode, **kw)
    _same(a, b)
    return b


_PFN = {}


def _pfn_weights(features):
    if features not in _PFN:
        rng = np.random.default_rng(11)
        _PFN[features] = (dev((rng.standard_normal((features + 5, 64)) / 3).astype(np.float32)), dev(rng.uniform(0.5, 1.5, 64).astype(np.float32)),
                          dev(rng.uniform(-0.3, 0.3, 64).astype(np.float32)))
    return _PFN[features]


def _check_lists(ops, pts, got, ref, geo):
    """No voxel tensor: offsets, coordinates, counts; the point lists through the PillarFeatureNet that reads them."""
    H.assert_voxelize_equal(got, ref)
    assert got["voxels"] is None
    m = int(ref["voxel_offsets"][-1])
    if m == 0:
        return
    wt, sc, sh = _pfn_weights(pts.shape[1])
    vs, r = geo[1], geo[0]
    xo, yo = vs[0] / 2 + r[0], vs[1] / 2 + r[1]
    want = ops.pfn_forward(dev(ref["voxels"]), dev(ref["num_points_per_voxel"]), dev(ref["coordinates"]), wt, sc, sh, vs[0], vs[1], xo, yo)
    have = ops.pfn_forward_slots(pts, got, wt, sc, sh, vs[0], vs[1], xo, yo)[:m]
    assert _bits_equal(have, want), "point lists: PillarFeatureNet through the slots differs from the reference's voxel tensor"


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_case(ops, case):
    """One row of the case table (voxel_ref_helpers._cases; the forms each row selects are asserted on the CPU)."""
    pts, offs = _batch(case.clouds(), case.spare())
    pts, offs = dev(pts), dev(offs)
    ref = case.reference()
    kw = dict(fill=case.fill, mean_features=case.nf if case.fill else 0, mean_dtype=H.TORCH_DTYPES[case.dtype], encoder=case.encoder)
    got = _twice(ops, pts, offs, case.geo, case.max_points, case.max_voxels, case.cap_mode, **kw)
    assert (got["site_table"][0] == "vox") == case.forms()["keys"]
    if case.fill:
        H.assert_voxelize_equal(got, ref, case.nf, case.dtype, case.encoder)
    else:
        _check_lists(ops, pts, got, ref, case.geo)


def test_more_than_256_points_per_voxel_is_refused_before_any_launch(ops):
    from second_amd import runtime as rt
    c = H.CASE["fused/n513"]
    pts, offs = _batch(c.clouds())
    with pytest.raises(rt.SecondHipError, match="256"):
        ops.voxelize(dev(pts), dev(offs), c.geo[0], c.geo[1], 257, 1000)
    assert rt.lib().sec_voxelize_workspace_bytes(513, 1, 1000, 257) == 0 and rt.lib().sec_voxelize_workspace_bytes(513, 1, 1000, 256) > 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- epilogues
G = H.grid_geometry(64, 64, 4)


def _epilogue_clouds(F):
    a, b = H.mixed_cloud(G, 700, 150, 60 + F, F), H.mixed_cloud(G, 300, 90, 70 + F, F)
    a[5, 3 if F > 3 else 2] = np.nan if F > 3 else a[5, 2]       # a NaN intensity travels through the voxel tensor unchanged
    a[7, 2] = -0.0                                                # z = -0.0 is in range (lo = 0) and keeps its sign
    return [a, b]


@pytest.mark.parametrize("F", [3, 4, 5, 6])
@pytest.mark.parametrize("T", [5, 9])
def test_epilogues_every_feature_count_mean_width_and_dtype(ops, F, T):
    """F = 4 at max_points <= 8 takes k_vox_fill_mean4, everything else k_vox_fill + k_vox_mean: all bit-equal to one restatement."""
    clouds = _epilogue_clouds(F)
    pts, offs = _batch(clouds)
    pts, offs = dev(pts), dev(offs)
    ref = H.ref_voxelize(clouds, G[1], G[0], T, 100000, "break")
    assert H.forms(1000, 2, T, 100000, 64 * 64 * 4, features=F)["epilogue"] == ("fill_mean4" if (F == 4 and T == 5) else "fill+mean")
    assert np.signbit(ref["voxels"][..., 2]).any() and (F == 3 or np.isnan(ref["voxels"][..., 3]).any())
    for nf in range(1, F + 1):
        for dtype in ("float32", "float16", "bfloat16"):
            got = _twice(ops, pts, offs, G, T, 100000, "break", mean_features=nf, mean_dtype=H.TORCH_DTYPES[dtype])
            H.assert_voxelize_equal(got, ref, nf, dtype)
    none = _twice(ops, pts, offs, G, T, 100000, "break")                       # no mean asked for: k_vox_fill alone
    assert "mean" not in none
    H.assert_voxelize_equal(none, ref)


@pytest.mark.parametrize("T", [5, 9])
def test_points_four_bytes_off_alignment_take_the_two_kernel_epilogue_bit_for_bit(ops, T):
    clouds = _epilogue_clouds(4)
    pts, offs = _batch(clouds)
    n = len(pts)
    flat = torch.zeros(n * 4 + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(n, 4)
    off.copy_(torch.from_numpy(pts))
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    aligned = dev(pts)
    assert aligned.data_ptr() % 16 == 0
    offs = dev(offs)
    ref = H.ref_voxelize(clouds, G[1], G[0], T, 100000, "break")
    for dtype in ("float32", "bfloat16"):
        for enc, nf in (("SimpleVoxel", 4), ("SimpleVoxel", 3), ("SimpleVoxelRadius", 4)):
            kw = dict(mean_features=nf, mean_dtype=H.TORCH_DTYPES[dtype], encoder=enc)
            a = _twice(ops, aligned, offs, G, T, 100000, "break", **kw)
            b = _twice(ops, off, offs, G, T, 100000, "break", **kw)
            _same(a, b)
            H.assert_voxelize_equal(b, ref, nf, dtype, enc)


@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("T", [5, 9])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_radius_rows_on_both_routes(ops, F, T, dtype):
    """encoder="SimpleVoxelRadius": the fused epilogue (F = 4, max_points <= 8) and the stand-alone kernel behind k_vox_fill, bit-equal
    to ops.simple_voxel_radius on the same voxel tensor and to ref_radius32 after one rounding."""
    clouds = _epilogue_clouds(F)
    pts, offs = _batch(clouds)
    ref = H.ref_voxelize(clouds, G[1], G[0], T, 100000, "break")
    got = _twice(ops, dev(pts), dev(offs), G, T, 100000, "break", mean_features=4, mean_dtype=H.TORCH_DTYPES[dtype], encoder="SimpleVoxelRadius")
    H.assert_voxelize_equal(got, ref, 4, dtype, "SimpleVoxelRadius")
    alone = ops.simple_voxel_radius(got["voxels"].contiguous(), got["num_points_per_voxel"].contiguous(), 4, out_dtype=H.TORCH_DTYPES[dtype])
    nan = torch.isnan(alone)
    assert torch.equal(nan, torch.isnan(got["mean"])) and _bits_equal(torch.where(nan, 0, alone), torch.where(nan, 0, got["mean"]))


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_stand_alone_simple_voxel_below_at_and_above_the_row_count(ops, dtype):
    ref = H.CASE["fused/n2571"].reference()
    m = len(ref["voxels"])
    v, npv = dev(ref["voxels"]), dev(ref["num_points_per_voxel"])
    for live in (0, 1, m - 1, m, m + 5):
        nd = torch.tensor([live], dtype=torch.int32, device="cuda")
        k = min(live, m)
        part = {key: ref[key][:k] for key in ("voxels", "num_points_per_voxel")}
        for nf in (1, 4):
            out = ops.simple_voxel(v, npv, nf, out_dtype=H.TORCH_DTYPES[dtype], num_dev=nd)
            assert out.shape == (m, nf) and not out[k:].view(torch.int32 if dtype == "float32" else torch.int16).any()     # +0.0 bits
            H.assert_mean_equal(out[:k], part, nf, dtype)
        out = ops.simple_voxel_radius(v, npv, 4, out_dtype=H.TORCH_DTYPES[dtype], num_dev=nd)
        assert out.shape == (m, 4) and not out[k:].view(torch.int32 if dtype == "float32" else torch.int16).any()
        H.assert_mean_equal(out[:k], part, 4, dtype, "SimpleVoxelRadius")
    H.assert_mean_equal(ops.simple_voxel(v, npv, 4, out_dtype=H.TORCH_DTYPES[dtype]), ref, 4, dtype)


# ----------------------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("T", [5, 9])
@pytest.mark.parametrize("cap_mode,V", [("break", 100000), ("break", 120), ("continue", 120)])
def test_static_capacity_call_leaves_rows_past_the_count_alone(ops, T, cap_mode, V):
    """sync=False, straight through the C ABI on sentinel-filled caller buffers: rows at or past voxel_offsets[B] are not written."""
    from second_amd import runtime as rt
    clouds = [H.mixed_cloud(G, 900, 200, 81), H.mixed_cloud(G, 0, 1, 82), H.mixed_cloud(G, 600, 150, 83)]
    pts, offs = _batch(clouds)
    n, B = len(pts), 3
    ref = H.ref_voxelize(clouds, G[1], G[0], T, V, cap_mode)
    m = int(ref["voxel_offsets"][-1])
    rows = min(B * V, n)
    assert m < rows
    pts, offs = dev(pts), dev(offs)
    voxels = torch.full((rows, T, 4), -7.5, device="cuda")
    coors = torch.full((rows, 4), -7, dtype=torch.int32, device="cuda")
    npv = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    mean = torch.full((rows, 4), -7.5, device="cuda")
    voff = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    l = rt.lib()
    ws = rt.workspace(l.sec_voxelize_workspace_bytes(n, B, V, T), pts.device)
    for _ in range(2):
        rt.check(l.sec_voxelize_f32(rt.ptr(pts), rt.ptr(offs), n, 4, B, rt.f_arr(G[0]), rt.f_arr(G[1]), T, V, {"break": 0, "continue": 1}[cap_mode],
                                    rt.ptr(voxels), rt.ptr(coors), rt.ptr(npv), rt.ptr(voff), rt.ptr(mean), 4, rt.dtype_code(torch.float32),
                                    rt.ptr(ws), ws.numel(), rt.stream()), "sec_voxelize_f32")
        torch.cuda.synchronize()
        assert (voxels[m:] == -7.5).all() and (coors[m:] == -7).all() and (npv[m:] == -7).all() and (mean[m:] == -7.5).all()
        H.assert_voxelize_equal({"voxels": voxels[:m], "coordinates": coors[:m], "num_points_per_voxel": npv[:m], "voxel_offsets": voff,
                                 "mean": mean[:m]}, ref, 4)


@pytest.mark.parametrize("B", [1, 3, 65])
def test_no_points_at_all(ops, B):
    pts = torch.zeros((0, 4), dtype=torch.float32, device="cuda")
    offs = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    for T, fill in ((5, True), (9, True), (9, False)):
        got = _twice(ops, pts, offs, G, T, 100, "break", fill=fill, mean_features=4 if fill else 0)
        assert got["voxel_num"] == 0 and got["coordinates"].shape == (0, 4) and not got["voxel_offsets"].any()
        assert got["voxel_offsets"].numel() == B + 1


# ----------------------------------------------------------------------------------------------------------------- stale keys
SUBM_GEO = H.grid_geometry(36, 40, 12)
SUBM_SHAPE = [12, 40, 36]


def test_rulebook_builders_refuse_a_voxeliser_table_without_keys(ops):
    """fill=False, max_points > 8 and B * cells inside the table: slots are numbered by cell and the key array is never written, so
    its site_table names no lookup -- rulebook_subm / rulebook_chain refuse it by name before anything is launched."""
    from second_amd import runtime as rt
    geo = H.grid_geometry(32, 32, 1)
    pts, offs = _batch([H.mixed_cloud(geo, 500, 200, 31)])
    pts = dev(pts)
    vox = ops.voxelize(pts, dev(offs), geo[0], geo[1], 20, 100000, fill=False)
    assert vox["site_table"][0] == "vox_slots" and vox["voxel_num"] > 100
    idx = vox["coordinates"].contiguous()
    with pytest.raises(rt.SecondHipError, match="vox_slots"):
        ops.rulebook_subm(idx, 1, [1, 32, 32], 3, 1, site_table=vox["site_table"])
    with pytest.raises(rt.SecondHipError, match="vox_slots"):
        ops.rulebook_chain(idx, 1, [1, 32, 32], [(3, 2, 1, 512)], site_table=vox["site_table"], want_subm=[True, False])
    plain = ops.rulebook_subm(idx, 1, [1, 32, 32], 3, 1)                       # without the table: built as ever
    assert (plain["nbr_out"][:, 13] == torch.arange(idx.shape[0], device="cuda", dtype=torch.int32)).all()
    # the point lists are what this table is for
    wt, sc, sh = _pfn_weights(4)
    assert ops.pfn_forward_slots(pts, vox, wt, sc, sh, 0.5, 0.5, 0.25, 0.25).shape == (vox["voxel_num"], 64)


@pytest.mark.parametrize("form,T,V,fill", [("fused", 5, 100000, True), ("unfused", 9, 100000, True), ("fused+cap", 5, 2000, True),
                                           ("unfused+cap", 9, 2000, True), ("fused+peek+cap", 5, 1200, True), ("unfused+peek+cap", 9, 1200, True),
                                           ("lists+hash", 20, 1200, False)])
@pytest.mark.parametrize("cap_mode", ["break", "continue"])
def test_every_hash_form_leaves_the_table_the_first_subm_rulebook_reads(ops, form, T, V, fill, cap_mode):
    """12 x 40 x 36 cells: the table a call WITH keys leaves (fused and unfused scan, with the peek, the voxel cap hit so that slots
    with svid = -1 exist) gives the stand-alone build's nbr_out."""
    clouds = [H.mixed_cloud(SUBM_GEO, 3300, 9000, 91), H.mixed_cloud(SUBM_GEO, 3300, 9000, 92)]
    pts, offs = _batch(clouds)
    n = len(pts)
    f = H.forms(n, 2, T, V, 12 * 40 * 36, fill=fill)
    assert f["keys"] and f["first"] == ("hash+peek" if "peek" in form or "lists" in form else "hash") and (f["scan"] == "fused") == form.startswith("fused")
    ref = H.ref_voxelize(clouds, SUBM_GEO[1], SUBM_GEO[0], T, V, cap_mode)
    per = np.diff(ref["voxel_offsets"])
    assert (per == V).all() if "cap" in form or "lists" in form else (per < V).all()
    vox = ops.voxelize(dev(pts), dev(offs), SUBM_GEO[0], SUBM_GEO[1], T, V, cap_mode, fill=fill)
    assert vox["site_table"][0] == "vox"
    H.assert_voxelize_equal(vox, ref)
    idx = vox["coordinates"].contiguous()
    reuse = ops.rulebook_subm(idx, 2, SUBM_SHAPE, 3, 1, site_table=vox["site_table"])
    plain = ops.rulebook_subm(idx.clone(), 2, SUBM_SHAPE, 3, 1)
    assert torch.equal(reuse["nbr_out"], plain["nbr_out"])
    assert (reuse["nbr_out"][:, 13] == torch.arange(idx.shape[0], device="cuda", dtype=torch.int32)).all()
    assert int((reuse["nbr_out"] >= 0).sum()) > 2 * idx.shape[0]               # a crowded grid: neighbours exist
