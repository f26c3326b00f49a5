"""CPU: what tests/test_gpu_voxel_edges.py compares the voxeliser with is right, and its comparison can fail.

  * ``ref_voxelize`` equals the executed reference (tests/golden/voxel_edges.npz: every cell border of five geometries with its fp32
    neighbours, with and without the cap; the older voxel_coords.npz) and the C oracle's sequential loop on every listed GPU input in
    both cap modes; ``ref_mean32`` equals the oracle's mean bit for bit, sits inside the float64 bound and holds the recorded
    ``SimpleVoxel`` output inside it.
  * Every generator's stated property.
  * A sequential float32 emulation of the kernels' stated arithmetic passes ``assert_voxelize_equal``; fourteen planted mistakes
    each fail it on a listed GPU input.
  * Every GPU case selects the forms it is listed for, by a restatement of voxelize_impl's five conditions whose constants are read
    from csrc/voxelize.hip.
"""
import os

import numpy as np
import pytest
import torch

import voxel_ref_helpers as H
from oracle import oracle as orc

HOST_CASES = [c for c in H.CASES if c.host]


# ------------------------------------------------------------------------------------------- the executed reference's fixtures
def _density(ref, grid):
    kept = ref["point_voxel"][ref["point_voxel"] >= 0]
    co = ref["coordinates"][kept]
    d = np.zeros((int(grid[1]), int(grid[0])), np.int64)
    np.add.at(d, (co[:, 2], co[:, 3]), 1)
    return d


@pytest.mark.parametrize("g", H.BOUNDARY_GEOMETRIES)
def test_reference_equals_the_executed_loop_on_every_cell_border(golden, g):
    z = golden("voxel_edges")
    geo = H.geometry(g)
    pts, _ = H.boundary_points(geo, int(z[f"{g}_stride"]))
    assert np.array_equal(pts.view(np.int32), z[f"{g}_points"].view(np.int32)), "the generator no longer makes the fixture's points"
    assert np.array_equal(np.asarray(geo[0], np.float32), z[f"{g}_range"]) and np.array_equal(np.asarray(geo[1], np.float32), z[f"{g}_voxel_size"])
    grid = H.grid_of(*geo)
    for cap, tag in ((1 << 30, ""), (int(z[f"{g}_cap"]), "_cap")):
        ref = H.ref_voxelize([pts], geo[1], geo[0], 3, cap, "break")
        np.testing.assert_array_equal(ref["coordinates"][:, 1:], z[f"{g}{tag}_coors"])
        d = _density(ref, grid)
        yx = np.argwhere(d > 0)
        np.testing.assert_array_equal(np.concatenate([yx, d[d > 0][:, None]], 1), z[f"{g}{tag}_density"])
    assert 0 < int(z[f"{g}_cap"]) < len(z[f"{g}_coors"]) and len(z[f"{g}_cap_coors"]) == int(z[f"{g}_cap"])


@pytest.mark.parametrize("tag", ["kitti", "coarse_cap"])
def test_reference_equals_the_older_fixture(golden, tag):
    z = golden("voxel_coords")
    pts, vs, pr, cap = z[f"{tag}_points"], z[f"{tag}_voxel_size"], z[f"{tag}_range"], int(z[f"{tag}_cap"])
    ref = H.ref_voxelize([pts], vs, pr, 5, cap, "break")
    np.testing.assert_array_equal(ref["coordinates"][:, 1:], z[f"{tag}_coors"])
    np.testing.assert_array_equal(_density(ref, H.grid_of(pr, vs)), z[f"{tag}_density"].astype(np.int64))


def test_borders_that_decide_against_intuition():
    geo = H.geometry("kitti")
    y = np.nextafter(np.float32(40), np.float32(-np.inf))
    x = np.nextafter(np.float32(70.4), np.float32(-np.inf))
    ok, c = H.cells_of(np.array([[1.0, y, 0.0], [x, 0.0, 0.0], [-0.0, 0.0, 0.0], [np.nan, 0, 0], [1, np.inf, 0], [1, 0, -np.inf]], np.float32), *geo)
    assert y < 40 and not ok[0]                    # below hi, yet fl((y + 40) / 0.05) = 1600: out of range
    assert ok[1] and c[1, 0] == 1407
    assert ok[2] and c[2, 0] == 0                  # -0.0: `c < 0` is false
    assert not ok[3:].any()


# ------------------------------------------------------------------------------------------- the oracle's sequential loop
def _equal_oracle(clouds, geo, T, V, cap_mode, ref):
    for b, c in enumerate(clouds):
        o = orc.points_to_voxel(c, geo[1], geo[0], T, V, cap_mode)
        lo, hi = ref["voxel_offsets"][b:b + 2]
        assert hi - lo == o["voxel_num"], (b, hi - lo, o["voxel_num"])
        np.testing.assert_array_equal(ref["coordinates"][lo:hi, 1:], o["coordinates"])
        assert (ref["coordinates"][lo:hi, 0] == b).all()
        np.testing.assert_array_equal(ref["num_points_per_voxel"][lo:hi], o["num_points_per_voxel"])
        np.testing.assert_array_equal(ref["voxels"][lo:hi].view(np.int32), o["voxels"].view(np.int32))


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_reference_equals_the_oracle_loop_on_every_gpu_input(case):
    for cap_mode in ("break", "continue"):
        ref = H.ref_voxelize(case.clouds(), case.geo[1], case.geo[0], case.max_points, case.max_voxels, cap_mode)
        _equal_oracle(case.clouds(), case.geo, case.max_points, case.max_voxels, cap_mode, ref)
        # slots name the points the voxel tensor holds
        allp = np.concatenate(case.clouds())
        live = ref["slots"] >= 0
        assert np.array_equal(allp[ref["slots"][live]].view(np.int32), ref["voxels"][live].view(np.int32))
        assert np.array_equal(live.sum(1), ref["num_points_per_voxel"])


def test_live_rows_cut_the_concatenated_clouds():
    c = H.CASE["spare/hash"]
    a, b = c.clouds()
    spare = c.spare()
    ref = c.reference()
    cut = H.ref_voxelize([a, np.concatenate([b, spare])], c.geo[1], c.geo[0], c.max_points, c.max_voxels, c.cap_mode, live_rows=len(a) + len(b))
    for k in ref:
        assert np.array_equal(ref[k], cut[k]), k
    more = H.ref_voxelize([a, np.concatenate([b, spare])], c.geo[1], c.geo[0], c.max_points, c.max_voxels, c.cap_mode)
    assert more["voxel_offsets"][-1] > ref["voxel_offsets"][-1]          # the spare rows WOULD open voxels


# ------------------------------------------------------------------------------------------- means
@pytest.mark.parametrize("name", ["fused/n2571", "hash/onecell/T5", "slots/T60/runs", "cells/kitti/fused", "slots/T256/edges"])
def test_mean32_equals_the_oracle_bit_for_bit_and_sits_inside_the_float64_bound(name):
    ref = H.CASE[name].reference()
    for nf in (1, 3, 4):
        m32 = H.ref_mean32(ref["voxels"], ref["num_points_per_voxel"], nf)
        o = orc.simple_voxel_mean(ref["voxels"], ref["num_points_per_voxel"], nf)
        assert np.array_equal(m32.view(np.int32), o.view(np.int32))
        m64, bound = H.ref_mean64(ref["voxels"], ref["num_points_per_voxel"], nf)
        assert (np.abs(m32.astype(np.float64) - m64) <= bound).all()
        assert (bound <= 2.0 ** -15 * np.abs(ref["voxels"][:, :, :nf]).max(1) + 1e-30).all()      # the bound is tight: T <= 256 roundings


def test_recorded_simple_voxel_output_is_inside_the_float64_bound(golden):
    z = golden("torch_modules")
    m64, bound = H.ref_mean64(z["sv_voxels"], z["sv_num_points"], 4)
    assert (np.abs(z["sv_out"].astype(np.float64) - m64) <= bound).all()
    m32 = H.ref_mean32(z["sv_voxels"], z["sv_num_points"], 4)
    assert (np.abs(m32.astype(np.float64) - m64) <= bound).all()


def test_radius_rows_and_the_one_rounding():
    ref = H.CASE["fused/n2571"].reference()
    r = H.ref_radius32(ref["voxels"], ref["num_points_per_voxel"])
    m = H.ref_mean32(ref["voxels"], ref["num_points_per_voxel"], 4)
    assert r.shape == (len(m), 4) and (r[:, 3] == 0).all() and np.array_equal(r[:, 1:3], m[:, 2:4])
    exact = np.sqrt(m[:, 0].astype(np.float64) ** 2 + m[:, 1].astype(np.float64) ** 2)
    assert (np.abs(r[:, 0] - exact) <= 3 * H.U * exact).all()            # two products' sum (relative 2u, halved by the root) + the root's u
    for dt in ("float16", "bfloat16"):
        once = H.round_to(m, dt)
        assert torch.equal(once, torch.from_numpy(m).to(H.TORCH_DTYPES[dt]))


# ------------------------------------------------------------------------------------------- generator properties
# which (geometry, axis) cannot show a reciprocal multiply: 0.25 = 2^-2 has an exact reciprocal; one-cell axes and the coarse
# z axis (0.5) likewise divide exactly
NO_RECIPROCAL = {("nusc_pp", 0), ("nusc_pp", 1), ("nusc_pp", 2), ("kitti_pp", 2), ("coarse", 2)}
BORDER_COUNTS = {("kitti", 0): (4227, 378, 383), ("kitti", 1): (4803, 159, 883), ("kitti", 2): (123, 2, 18), ("kitti_pp", 0): (1299, 111, 348),
                ("nusc_pp", 0): (1203, 0, 271)}


@pytest.mark.parametrize("g", H.BOUNDARY_GEOMETRIES)
def test_boundary_points_properties(g):
    geo = H.geometry(g)
    pts, info = H.boundary_points(geo)
    grid = H.grid_of(*geo)
    r, v = np.asarray(geo[0], np.float32), np.asarray(geo[1], np.float32)
    ok, cells = H.cells_of(pts, *geo)
    for j in range(3):
        i = info[j]
        assert i["full_rows"] == 3 * (grid[j] + 1)
        rows = np.arange(i["rows"].start, i["rows"].stop)
        vals = pts[rows, j].reshape(-1, 3)
        e = r[j] + np.arange(grid[j] + 1, dtype=np.float32) * v[j]
        assert np.array_equal(vals[:, 1], e) and np.array_equal(vals[:, 0], np.nextafter(e, np.float32(-np.inf))) and \
            np.array_equal(vals[:, 2], np.nextafter(e, np.float32(np.inf)))
        extra = pts[i["rows"].stop:i["rows"].stop + 6, j]
        assert extra[0] == r[3 + j] and extra[1] < r[3 + j] and extra[2] < r[j] and extra[3] == 0 and extra[4] == 0
        assert not np.signbit(extra[3]) and np.signbit(extra[4]) and extra[5] == np.float32(2.0 ** -149) and extra[5] > 0
        # the other two coordinates sit mid-cell: only axis j decides
        others = [a for a in range(3) if a != j]
        allrows = np.arange(i["rows"].start, i["rows"].stop + 6)
        q = (pts[allrows][:, others] - r[others]) / v[others]
        assert np.array_equal(np.floor(q), np.tile(grid[others] // 2, (len(allrows), 1))) and (np.abs(q - np.floor(q) - 0.5) < 0.01).all()
        if (g, j) in BORDER_COUNTS:
            assert (i["full_rows"], i["full_recip"], i["full_f64"]) == BORDER_COUNTS[g, j]
        if (g, j) in NO_RECIPROCAL:
            assert i["recip"] == 0          # this axis cannot expose a reciprocal: stated, not asserted away
        else:
            assert i["recip"] * 100 >= len(rows), (g, j, i)
        assert i["f64"] * 100 >= len(rows), (g, j, i)
        # both sides of the range on every axis
        assert ok[allrows].any() and (~ok[allrows]).any() and cells[allrows][ok[allrows], j].max() == grid[j] - 1
    assert pts.shape[1] == 4 and np.isfinite(pts).all()


def test_boundary_subsampling_keeps_the_ends_and_every_disagreement():
    geo = H.geometry("kitti")
    full, fi = H.boundary_points(geo)
    sub, si = H.boundary_points(geo, 8)
    assert len(sub) < len(full)
    grid = H.grid_of(*geo)
    r, v = np.asarray(geo[0], np.float32), np.asarray(geo[1], np.float32)
    for j in range(3):
        assert si[j]["recip"] == fi[j]["full_recip"] == si[j]["full_recip"] and si[j]["f64"] == fi[j]["full_f64"]
        vals = set(sub[si[j]["rows"], j].tolist())
        for k in (0, grid[j] - 1, grid[j]):
            assert float(r[j] + np.float32(k) * v[j]) in vals


@pytest.mark.parametrize("tile", [512, 1024])
@pytest.mark.parametrize("B", [1, 2, 12, 63, 64, 65])
def test_tile_clouds_properties(tile, B):
    for pattern in ("shared", "distinct", "one"):
        clouds, props = H.tile_clouds(tile, B, pattern)
        assert len(clouds) == B and [len(c) for c in clouds] == props["lengths"]
        lens, starts = props["lengths"], props["starts"]
        assert max(lens) > 3 * tile
        if pattern == "one":
            assert sum(1 for n in lens if n) == 1
            continue
        if B >= 12:
            live = {s for s, n in zip(starts, lens) if n}
            assert {tile - 1, tile, tile + 1, 2 * tile} <= live
            assert lens[0] == 0 and lens[-1] == 0 and any(lens[i] == lens[i + 1] == lens[i + 2] == 0 for i in range(1, B - 3))
        if B == 2:
            assert starts[1] == tile - 1
        ref = H.ref_voxelize(clouds, H.grid_geometry(64, 64, 4)[1], H.grid_geometry(64, 64, 4)[0], 3, 1 << 30, "break")
        per = np.diff(ref["voxel_offsets"])
        if pattern == "distinct":
            assert np.array_equal(per, lens)
        else:
            assert (per[np.asarray(lens) > 20] < np.asarray(lens)[np.asarray(lens) > 20]).all()      # revisits


@pytest.mark.parametrize("tile", [512, 1024])
def test_revisit_cloud_has_a_revisit_in_every_later_tile_and_last(tile):
    pts, props = H.revisit_cloud(tile, 200)
    geo = H.grid_geometry(64, 64, 4)
    ref = H.ref_voxelize([pts], geo[1], geo[0], 1 << 12, 1 << 30, "break")
    first = ref["slots"][:, 0]
    assert len(first) == 200 and first.max() < 200 <= tile                 # every voxel opens in tile 0
    n = props["n"]
    assert n % tile and n // tile >= 3 and ref["point_voxel"][n - 1] >= 0 and (n - 1) // tile == n // tile
    for t in range(1, n // tile + 1):
        assert (ref["point_voxel"][t * tile:min((t + 1) * tile, n)] >= 0).all()


@pytest.mark.parametrize("R", [1, 2, 4])
def test_pillar_runs_enter_the_insertion_loop(R):
    pts, props = H.pillar_runs([63, 64, 65, 127, 128, 129, 255, 256, 257, 1000])
    assert props["n"] >= 3 * 1024
    lab = props["labels"]
    hit = 0
    for p, length in enumerate(props["lengths"]):
        idx = np.nonzero(lab == p)[0]
        assert len(idx) == length
        if length >= 63:
            assert len(set((idx // 1024).tolist())) >= 3                  # interleaved across three groups of k_vox_group_rank
        if length > 64 * R:
            run = H.model_run_order(idx)
            kth = np.sort(idx)[64 * R - 1]
            hit += int((run[64 * R:] < kth).any())
    assert hit >= 1
    geo = H.grid_geometry(64, 64, 1)
    ref = H.ref_voxelize([pts], geo[1], geo[0], 1, 1 << 30, "break")
    assert len(ref["coordinates"]) == len(props["lengths"]) + (lab < 0).sum()     # every filler point is a pillar of its own


@pytest.mark.parametrize("at", [59, 511, 512, 1023, 1024])
def test_cap_clouds_have_revisits_behind_the_break(at):
    v = 60
    pts, props = H.cap_clouds(v, at)
    geo = H.grid_geometry(64, 64, 4)
    full = H.ref_voxelize([pts], geo[1], geo[0], 4, 1 << 30, "break")
    assert len(full["coordinates"]) == v and full["slots"][v - 1, 0] == at == props["break_at"]
    brk = H.ref_voxelize([pts], geo[1], geo[0], 1 << 10, v - 1, "break")
    con = H.ref_voxelize([pts], geo[1], geo[0], 1 << 10, v - 1, "continue")
    behind = np.arange(len(pts)) > at
    assert (brk["point_voxel"][behind] < 0).all() and (con["point_voxel"][behind] >= 0).sum() >= 10
    assert (con["point_voxel"][behind] < 0).any()                         # later points of the voxel past the cap
    assert not np.array_equal(brk["num_points_per_voxel"], con["num_points_per_voxel"])


# ------------------------------------------------------------------------------------------- emulation and planted mistakes
def _emulated(case, mistake=None, nf=None, dtype="float32", encoder="SimpleVoxel", cap_mode=None):
    nf = case.nf if nf is None else nf
    cap_mode = cap_mode or case.cap_mode
    got = H.emulate(case.clouds(), case.geo, case.max_points, case.max_voxels, cap_mode, nf, dtype, encoder, mistake)
    ref = H.ref_voxelize(case.clouds(), case.geo[1], case.geo[0], case.max_points, case.max_voxels, cap_mode)
    H.assert_voxelize_equal(got, ref, nf, dtype, encoder)


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.name)
def test_emulation_of_the_stated_arithmetic_passes(case):
    _emulated(case, nf=min(case.features, 4))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("encoder", ["SimpleVoxel", "SimpleVoxelRadius"])
def test_emulation_passes_in_16_bit_and_radius(dtype, encoder):
    for name in ("fused/n2571", "slots/T60/runs", "cells/kitti_pp/fused"):
        _emulated(H.CASE[name], nf=4, dtype=dtype, encoder=encoder)
    _emulated(H.CASE["fused/n2571"], nf=4, dtype="float32", encoder=encoder)


PLANTED = {     # mistake -> (listed GPU inputs, keyword arguments of the run)
    "reciprocal": (["cells/kitti/fused", "cells/kitti_pp/run", "cells/nusc_fhd/fused"], {}),
    "trunc": (["cells/kitti/fused", "cells/nusc_pp/run"], {}),
    "le_grid": (["cells/kitti/fused", "cells/coarse/run"], {}),
    "neg_zero": (["cells/kitti/fused", "cells/kitti_pp/run"], {}),
    "break_as_continue": (["fused/cap/at511/V59/break", "flag4/cap/at1024/V59/break"], {}),
    "continue_as_break": (["fused/cap/at511/V59/continue", "fused/tiles/B64/shared/continue"], {}),
    "batch_cap": (["fused/cap/at512/V60/break", "flag4/tiles/B65/shared/break"], {}),
    "by_cell": (["fused/n513", "hash/table/n513/T9"], {}),
    "slots_reversed": (["slots/T8/edges", "slots/T60/runs"], {}),
    "last_points": (["slots/T8/edges", "slots/T200/runs"], {}),
    "uncapped_count": (["slots/T9/edges", "hash/onecell/T5"], {}),
    "div_max_points": (["fused/n2571", "slots/T60/runs"], {"nf": 4}),
    "reverse_sum": (["fused/n2571", "slots/T60/runs"], {"nf": 4}),
    "truncate16": (["fused/n2571", "slots/T60/runs"], {"nf": 4, "dtype": "bfloat16"}),
}


@pytest.mark.parametrize("mistake", H.MISTAKES)
def test_planted_mistake_fails_the_comparison_on_a_listed_gpu_input(mistake):
    names, kw = PLANTED[mistake]
    for name in names:
        _emulated(H.CASE[name], **kw)                    # the same run without the mistake passes
        with pytest.raises(AssertionError):
            _emulated(H.CASE[name], mistake, **kw)
    if mistake == "truncate16":
        with pytest.raises(AssertionError):
            _emulated(H.CASE[names[0]], mistake, nf=4, dtype="float16")
        with pytest.raises(AssertionError):
            _emulated(H.CASE[names[0]], mistake, nf=4, dtype="float16", encoder="SimpleVoxelRadius")


def test_the_quarter_metre_pillars_cannot_show_a_reciprocal():
    """0.25 has an exact reciprocal: multiply and divide agree on every border, so this geometry's cases say nothing about it."""
    _emulated(H.CASE["cells/nusc_pp/fused"], "reciprocal")


# ------------------------------------------------------------------------------------------- case table against the sources
def test_form_constants_equal_the_sources():
    assert H.read_constants() == H.DEFAULT_CONSTANTS


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_case_selects_the_forms_it_is_listed_for(case):
    from second_amd import ops
    f = case.forms(H.read_constants())
    for k, v in case.expect.items():
        assert f[k] == v, (case.name, k, f[k], v)
    n = sum(len(c) for c in case.clouds()) + case.spare_rows
    assert ops.voxelize_keeps_keys(n, len(case.clouds()), case.max_points, case.fill, int(np.prod(H.grid_of(*case.geo)))) == f["keys"]


def test_case_table_holds_both_sides_of_every_switch():
    seen = {}
    for c in H.CASES:
        f = c.forms()
        n = sum(len(x) for x in c.clouds()) + c.spare_rows
        for k in ("first", "scan", "frames", "slots", "table"):
            seen.setdefault(k, {}).setdefault(f[k], []).append((n, len(c.clouds()), c.max_points, c.max_voxels))
    assert set(seen["first"]) == {"hash", "hash+peek", "dense", "dense+staged"}
    assert set(seen["scan"]) == {"fused", "flag4", "flag16"}
    assert set(seen["frames"]) == {"lds", "k_vox_frames"}
    assert set(seen["slots"]) == {"cascade", "select<1>", "select<2>", "select<4>"}
    ns = {k: {t[0] for t in v} for k, v in seen["scan"].items()}
    assert 524287 in ns["flag4"] and 524288 in ns["flag16"]
    assert {64} <= {t[1] for t in seen["frames"]["lds"]} and {65} <= {t[1] for t in seen["frames"]["k_vox_frames"]}
    tp = {k: {t[2] for t in v} for k, v in seen["slots"].items()}
    assert 8 in tp["cascade"] and {9, 64} <= tp["select<1>"] and {65, 128} <= tp["select<2>"] and {129, 256} <= tp["select<4>"]
    assert 512 in {t[0] for t in seen["table"][1024]} and 513 in {t[0] for t in seen["table"][2048]}
    assert 262143 in {t[0] for t in seen["first"]["dense"]} and 262144 in {t[0] for t in seen["first"]["dense+staged"]}
    peek_on = {(t[0], t[1], t[3]) for t in seen["first"]["hash+peek"]}
    peek_off = {(t[0], t[1], t[3]) for t in seen["first"]["hash"]}
    assert (601, 1, 300) in peek_on and (600, 1, 300) in peek_off
    # dense | hash at B * cells = table | just above, at both table sizes
    f = lambda name: H.CASE[name].forms()["first"]
    assert f("dense/n500/32x32") == "dense" and f("dense/n500/34x32") == "hash"
    assert f("dense/n3000/128x64/break100000") == "dense" and f("dense/n3000/129x64/break100000") == "hash"
    assert H.forms(10, 1, 257, 10, 10)["refused"] and not H.forms(10, 1, 256, 10, 10)["refused"]


def test_epilogue_forms():
    k = H.read_constants()
    assert H.forms(100, 1, 5, 100, 64, features=4, k=k)["epilogue"] == "fill_mean4"
    assert H.forms(100, 1, 5, 100, 64, features=4, aligned=False, k=k)["epilogue"] == "fill+mean"
    assert H.forms(100, 1, 9, 100, 64, features=4, k=k)["epilogue"] == "fill+mean"
    assert H.forms(100, 1, 5, 100, 64, features=5, k=k)["epilogue"] == "fill+mean"
    assert H.forms(100, 1, 5, 100, 64, features=4, mean=False, k=k)["epilogue"] == "fill"
    assert H.forms(100, 1, 5, 100, 64, fill=False, k=k)["epilogue"] == "counts"


def test_fixture_regenerates_from_the_committed_generator():
    """The generator script and the fixture travel together (python tests/golden/make_golden_voxel_edges.py rewrites it byte for byte
    where the reference checkout is at hand); here: the fixture is small and holds every geometry's six arrays."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_edges.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    for g in H.BOUNDARY_GEOMETRIES:
        for k in ("points", "range", "voxel_size", "coors", "density", "cap", "cap_coors", "cap_density"):
            assert f"{g}_{k}" in z.files
