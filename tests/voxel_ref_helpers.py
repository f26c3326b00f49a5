"""References, input generators, the case table and the comparison of the voxeliser's edge suite (csrc/voxelize.hip), shared by
tests/test_voxel_ref_host.py (CPU) and tests/test_gpu_voxel_edges.py (GPU).

Three statements of points_to_voxel stand next to each other here and are held to one another on the CPU:
  * ``ref_voxelize``: vectorised numpy (what the GPU tests compare with; half a million points in well under a second),
  * the C oracle's sequential loop (``oracle.points_to_voxel``), called from the host file,
  * ``emulate``: a sequential restatement of the arithmetic the kernels promise, which also carries the planted mistakes.
The executed reference (second/utils/simplevis.py:8-60) pins all three through tests/golden/voxel_edges.npz and voxel_coords.npz.

No tolerance in this file is a measured number: integers and copied floats are compared exactly, fp32 means and radius rows bit for
bit with the restatement of the kernels' documented operation order and against float64 with the bound derived at ``ref_mean64``,
16-bit outputs bit for bit after one round-to-nearest-even.
"""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXELIZE_HIP = os.path.join(ROOT, "second.pytorch_amd", "csrc", "voxelize.hip")
COMMON_HPP = os.path.join(ROOT, "second.pytorch_amd", "csrc", "common.hpp")

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
TORCH_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


# ----------------------------------------------------------------------------------------------------------------- geometries
def _nusc_fhd():
    from second_amd import models
    c = models.ALL_FHD_NUSC
    return [float(v) for v in c["point_cloud_range"]], [float(v) for v in c["voxel_size"]]


def geometry(name):
    """(range6, voxel_size3) of the five geometries whose cell borders the suite walks."""
    if name == "nusc_fhd":
        return _nusc_fhd()
    return {
        "kitti": ([0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1]),                   # kitti/car.fhd
        "nusc_pp": ([-50, -50, -10, 50, 50, 10], [0.25, 0.25, 20]),               # nuscenes/all.pp.largea
        "kitti_pp": ([0, -39.68, -3, 69.12, 39.68, 1], [0.16, 0.16, 4]),          # kitti/pointpillars car
        "coarse": ([0, -8, -3, 16, 8, 1], [0.4, 0.4, 0.5]),                       # the cap geometry of voxel_coords.npz
    }[name]


BOUNDARY_GEOMETRIES = ("kitti", "nusc_pp", "kitti_pp", "nusc_fhd", "coarse")


def grid_geometry(gx, gy, gz=1):
    """A grid of gx x gy x gz cells of 0.5 x 0.5 x 1 from the origin: every cell border is a binary fraction, so the cell arithmetic
    is exact and the case is about order, caps and forms only."""
    return [0.0, 0.0, 0.0, 0.5 * gx, 0.5 * gy, 1.0 * gz], [0.5, 0.5, 1.0]


def grid_of(range6, voxel_size):
    r, v = np.asarray(range6, np.float32), np.asarray(voxel_size, np.float32)
    return np.round((r[3:] - r[:3]) / v).astype(np.int64)          # fp32 divide, round half to even (simplevis.py:26-29)


def cells_of(points, range6, voxel_size):
    """-> (in_range [N] bool, cell [N, 3] int64 (x, y, z)).  np.float32 subtract and divide are IEEE: exact restatement of
    ``np.floor((p - lo) / vs)``; NaN and +-inf fail both comparisons, -0.0 passes ``c < 0`` (simplevis.py:37-38)."""
    r, v = np.asarray(range6, np.float32), np.asarray(voxel_size, np.float32)
    g = grid_of(range6, voxel_size).astype(np.float32)
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(points, np.float32)[:, :3] - r[:3]) / v)
        ok = ((q >= 0) & (q < g)).all(1)
    return ok, np.where(ok[:, None], q, 0).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------- reference
def _split_live(clouds, live_rows):
    if live_rows is None:
        return [np.asarray(c, np.float32) for c in clouds]
    out, left = [], int(live_rows)
    for c in clouds:
        k = min(len(c), max(left, 0))
        out.append(np.asarray(c[:k], np.float32))
        left -= len(c)
    return out


def ref_voxelize(clouds, voxel_size, range6, max_points, max_voxels, cap_mode, live_rows=None):
    """points_to_voxel of every cloud (VoxelGeneratorV2.generate; loop: simplevis.py:31-50), numpy, vectorised.
    ``live_rows``: rows of the concatenated clouds at or past it do not exist for the voxeliser (capacity rows).
    -> dict(voxels [M, T, F], coordinates [M, 4] (b, z, y, x), num_points_per_voxel [M], voxel_offsets [B + 1],
            slots [M, T] = index of the slot's point in the concatenated clouds, -1 = padded;
            point_voxel [N] = voxel row of every point the loop counted into a voxel (also past max_points), -1 = dropped)."""
    assert cap_mode in ("break", "continue")
    clouds = _split_live(clouds, live_rows)
    T, V = int(max_points), int(max_voxels)
    F = clouds[0].shape[1]
    gx, gy, _ = (int(v) for v in grid_of(range6, voxel_size))
    vox, coo, npv, slo, pvx, offs, start = [], [], [], [], [], [0], 0
    for b, pts in enumerate(clouds):
        ok, c = cells_of(pts, range6, voxel_size)
        idx = np.nonzero(ok)[0]
        lin = (c[idx, 2] * gy + c[idx, 1]) * gx + c[idx, 0]
        uniq, first, inv = np.unique(lin, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                  # voxels numbered by their first point
        rank = np.empty(len(uniq), np.int64)
        rank[order] = np.arange(len(uniq))
        vid = rank[inv.reshape(-1)]
        keep = vid < V                                             # `continue`: only points of voxels past the cap are dropped
        if cap_mode == "break" and len(uniq) > V:
            keep &= idx < idx[first[order[V]]]                     # everything at or behind the point that would open voxel V
        nv = min(len(uniq), V)
        idk, vk = idx[keep], vid[keep]
        o = np.argsort(vk, kind="stable")                          # arrival order inside a voxel
        sv, si = vk[o], idk[o]
        cnt = np.bincount(vk, minlength=nv)
        pos = np.arange(len(o)) - (np.cumsum(cnt) - cnt)[sv]
        sel = pos < T                                              # the first max_points of every voxel
        voxels = np.zeros((nv, T, F), np.float32)                  # padded with +0.0
        slots = -np.ones((nv, T), np.int64)
        voxels[sv[sel], pos[sel]] = pts[si[sel]]
        slots[sv[sel], pos[sel]] = si[sel] + start
        cf = c[idx[first[order[:nv]]]]
        pv = -np.ones(len(pts), np.int64)
        pv[idk] = vk + offs[-1]
        pvx.append(pv)
        vox.append(voxels)
        slo.append(slots)
        coo.append(np.stack([np.full(nv, b), cf[:, 2], cf[:, 1], cf[:, 0]], 1).astype(np.int32).reshape(nv, 4))
        npv.append(np.minimum(cnt, T).astype(np.int32))
        offs.append(offs[-1] + nv)
        start += len(pts)
    return {"voxels": np.concatenate(vox), "coordinates": np.concatenate(coo), "num_points_per_voxel": np.concatenate(npv),
            "voxel_offsets": np.asarray(offs, np.int32), "slots": np.concatenate(slo), "point_voxel": np.concatenate(pvx)}


def ref_mean32(voxels, npv, nf):
    """SimpleVoxel in the kernels' documented order (k_vox_mean / k_vox_fill_mean4 / k_simple_voxel): an fp32 sum over ALL max_points
    slots in slot order from +0.0 (padded slots add +0.0), one fp32 division by the count."""
    v = np.asarray(voxels, np.float32)
    s = np.zeros((v.shape[0], nf), np.float32)
    with np.errstate(all="ignore"):
        for t in range(v.shape[1]):
            s = s + v[:, t, :nf]
        return s / np.asarray(npv).astype(np.float32)[:, None]


def ref_radius32(voxels, npv):
    """SimpleVoxelRadius rows [r, mz, mw, 0] with r = sqrt(fl(fl(mx mx) + fl(my my))) of the fp32 means (store_radius_row4)."""
    m = ref_mean32(voxels, npv, 4)
    with np.errstate(all="ignore"):
        r = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1])
    return np.stack([r, m[:, 2], m[:, 3], np.zeros_like(r)], 1).astype(np.float32)


def ref_mean64(voxels, npv, nf):
    """-> (float64 mean, per-element bound of an fp32 mean computed in ANY order over the T slots).
    T - 1 rounded additions of T terms: |fl(sum) - sum| <= gamma_{T-1} sum|x| <= gamma_T sum|x| (Higham, Accuracy and Stability,
    eq. 4.4), with gamma_T = T u / (1 - T u), u = 2^-24; the division by the exactly representable count adds one rounding of the
    quotient: u |m|, or, where the quotient is subnormal (the boundary sets hold 2^-149 itself), half a subnormal spacing: 2^-150.
    Additions do not underflow (a subnormal sum is exact).  Padded slots are exact zeros and add nothing."""
    v = np.asarray(voxels, np.float64)[:, :, :nf]
    n = np.asarray(npv, np.float64)[:, None]
    T = v.shape[1]
    gamma = T * U / (1 - T * U)
    with np.errstate(all="ignore"):
        m = v.sum(1) / n
        return m, gamma * np.abs(v).sum(1) / n + U * np.abs(m) + 2.0 ** -150


def round_to(x32, dtype):
    """ONE round-to-nearest-even of fp32 values to the storage type (torch's CPU cast)."""
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(TORCH_DTYPES[dtype])


# ----------------------------------------------------------------------------------------------------------------- comparison
def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def assert_mean_equal(got_mean, ref, nf, dtype="float32", encoder="SimpleVoxel"):
    """``mean`` of a voxeliser (or stand-alone SimpleVoxel) call against the references of ``ref`` (a ref_voxelize result): bit for
    bit after the one rounding, and -- fp32 -- inside the float64 bound.  A NaN must be a NaN (IEEE 754 leaves its payload open)."""
    radius = encoder == "SimpleVoxelRadius"
    r32 = ref_radius32(ref["voxels"], ref["num_points_per_voxel"]) if radius else ref_mean32(ref["voxels"], ref["num_points_per_voxel"], nf)
    want = round_to(r32, dtype)
    got = got_mean.detach().cpu() if isinstance(got_mean, torch.Tensor) else torch.from_numpy(np.asarray(got_mean))
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.dtype, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN means"
    gb, wb = _bits(got), _bits(want)
    bad = (gb != wb) & ~nan.numpy()
    assert not bad.any(), f"mean differs from the fp32 restatement in {int(bad.sum())} elements, first at {np.argwhere(bad)[0]}"
    if dtype == "float32":
        m64, bound = ref_mean64(ref["voxels"], ref["num_points_per_voxel"], 4 if radius else nf)
        g64 = got.double().numpy()
        if radius:          # columns z, w of the radius row ARE means; r adds three roundings and a root and has the bit check above
            g64, m64, bound = g64[:, 1:3], m64[:, 2:4], bound[:, 2:4]
        fin = np.isfinite(m64)
        assert (np.abs(g64 - m64)[fin] <= bound[fin]).all(), "mean outside the float64 bound"


def assert_voxelize_equal(got, ref, nf=0, dtype="float32", encoder="SimpleVoxel"):
    """``got``: a sync=True result of ops.voxelize (or an emulation in the same layout, numpy or torch) against ``ref_voxelize``."""
    np.testing.assert_array_equal(_np(got["voxel_offsets"]), ref["voxel_offsets"], err_msg="voxel_offsets")
    m = int(ref["voxel_offsets"][-1])
    co = _np(got["coordinates"])
    assert co.shape == (m, 4), (co.shape, m)
    np.testing.assert_array_equal(co, ref["coordinates"], err_msg="coordinates")
    np.testing.assert_array_equal(_np(got["num_points_per_voxel"]), ref["num_points_per_voxel"], err_msg="num_points_per_voxel")
    if got.get("voxels") is not None:
        gv = got["voxels"]
        assert tuple(gv.shape) == ref["voxels"].shape, (tuple(gv.shape), ref["voxels"].shape)
        np.testing.assert_array_equal(_bits(gv), _bits(ref["voxels"]), err_msg="voxels (bit patterns)")
    if nf:
        assert_mean_equal(got["mean"], ref, nf, dtype, encoder)


# ----------------------------------------------------------------------------------------------------------------- generators
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def cell_points(geo, cells_xyz, seed=0, features=4):
    """One point inside every listed cell (x, y, z), between a quarter and three quarters of the cell, seeded; the further features
    are uniform in [0, 1)."""
    range6, vs = geo
    rng = np.random.default_rng(seed)
    c = np.asarray(cells_xyz, np.int64).reshape(-1, 3)
    lo, v = np.asarray(range6[:3], np.float64), np.asarray(vs, np.float64)
    xyz = lo + (c + rng.uniform(0.25, 0.75, c.shape)) * v
    return np.concatenate([xyz, rng.uniform(0, 1, (len(c), features - 3))], 1).astype(np.float32)


def lin_cells(geo, lin):
    gx, gy, gz = (int(v) for v in grid_of(*geo))
    lin = np.asarray(lin, np.int64)
    assert ((lin >= 0) & (lin < gx * gy * gz)).all()
    return np.stack([lin % gx, (lin // gx) % gy, lin // (gx * gy)], 1)


def mixed_cloud(geo, n, cells, seed, features=4):
    """n points over `cells` cells drawn at random (revisits everywhere), every tenth point out of range."""
    rng = np.random.default_rng(seed)
    total = int(np.prod(grid_of(*geo)))
    pool = rng.permutation(total)[:cells]
    pts = cell_points(geo, lin_cells(geo, pool[rng.integers(0, cells, n)]), seed + 1, features)
    pts[9::10, 0] += np.float32(2 * (geo[0][3] - geo[0][0]))
    return pts


def distinct_cloud(geo, n, seed, features=4):
    """n points in n distinct cells."""
    total = int(np.prod(grid_of(*geo)))
    assert n <= total
    return cell_points(geo, lin_cells(geo, np.random.default_rng(seed).permutation(total)[:n]), seed + 1, features)


def _recip_f64_disagree(vals, lo, vs):
    """Which fp32 coordinates change cell under multiply-by-reciprocal / under float64 arithmetic on the configuration's decimal
    constants (what a loop that promotes to double computes), against the fp32 divide."""
    vals, lo32, vs32 = np.asarray(vals, np.float32), np.float32(lo), np.float32(vs)
    with np.errstate(all="ignore"):
        d = vals - lo32
        q = np.floor(d / vs32)
        qr = np.floor(d * (np.float32(1) / vs32))
        q64 = np.floor((vals.astype(np.float64) - float(lo)) / float(vs))
    return qr != q, q64 != q.astype(np.float64)


def boundary_points(geo, stride=1):
    """Per axis: the fp32 values fl(lo + fl(k vs)) for k = 0 .. grid with their two fp32 neighbours, hi and its neighbour below, lo's
    neighbour below, +-0.0 and the smallest subnormal; the other two coordinates sit mid-cell (cell grid // 2).  ``stride`` > 1
    keeps every stride-th k, k = 0, grid - 1, grid and every k of which one of the three values changes cell under a reciprocal
    multiply or under float64 arithmetic.
    -> (points [N, 4], info): info[axis] = dict(rows = slice of the axis's k-values (three per k), recip / f64 = disagreeing rows
    of that slice, full_rows / full_recip / full_f64 = the same counts at stride 1)."""
    range6, vs = geo
    r, v = np.asarray(range6, np.float32), np.asarray(vs, np.float32)
    grid = grid_of(range6, vs)
    mid = np.asarray(r[:3], np.float64) + (grid // 2 + 0.5) * np.asarray(v, np.float64)
    rows, info, at = [], {}, 0
    for j in range(3):
        k = np.arange(int(grid[j]) + 1)
        e = r[j] + k.astype(np.float32) * v[j]                                 # fp32 product and sum, as voxel_coords.npz places its borders
        tri = np.stack([np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))], 1)     # [K, 3]
        rc, f6 = _recip_f64_disagree(tri.reshape(-1), range6[j], vs[j])
        keep = (k % stride == 0) | (k == 0) | (k >= grid[j] - 1) | rc.reshape(-1, 3).any(1) | f6.reshape(-1, 3).any(1)
        vals = tri[keep].reshape(-1)
        rc_k, f6_k = _recip_f64_disagree(vals, range6[j], vs[j])
        extra = np.array([r[3 + j], np.nextafter(r[3 + j], np.float32(-np.inf)), np.nextafter(r[j], np.float32(-np.inf)), 0.0, -0.0,
                          np.float32(2.0 ** -149)], np.float32)
        allv = np.concatenate([vals, extra])
        p = np.tile(mid.astype(np.float32), (len(allv), 1))
        p[:, j] = allv
        rows.append(p)
        info[j] = dict(rows=slice(at, at + len(vals)), recip=int(rc_k.sum()), f64=int(f6_k.sum()),
                       full_rows=int(tri.size), full_recip=int(rc.sum()), full_f64=int(f6.sum()))
        at += len(allv)
    xyz = np.concatenate(rows)
    w = (np.arange(len(xyz)) % 97 / np.float32(97)).astype(np.float32)
    return np.concatenate([xyz, w[:, None]], 1).astype(np.float32), info


def tile_lengths(tile, B):
    """Cloud lengths that put cloud starts at tile - 1, tile, tile + 1 and 2 tile, an empty cloud first, three in a row in the middle
    and one last, and a cloud of more than three tiles (B >= 12; smaller batches keep what fits: B = 1 the long cloud, B = 2 a start
    at tile - 1 and the long cloud)."""
    long_ = 3 * tile + 5
    if B == 1:
        return [long_]
    if B == 2:
        return [tile - 1, long_]
    assert B >= 12
    head = [0, tile - 1, 1, 1, tile - 1, 7, 0, 0, 0, long_]
    fill = [(3, 0, 11, 1, 0, 29)[i % 6] for i in range(B - len(head) - 1)]
    return head + fill + [0]


def tile_clouds(tile, B, pattern, geo=None, seed=0):
    """-> (clouds, props).  ``pattern``: "shared" (a few hundred cells revisited within and across clouds and tiles), "distinct"
    (every point of a cloud opens a voxel), "one" (B clouds of which only one, in the middle, is non-empty: three tiles and five)."""
    geo = geo or grid_geometry(64, 64, 4)
    if pattern == "one":
        lens = [0] * B
        lens[B // 2] = 3 * tile + 5
    else:
        lens = tile_lengths(tile, B)
    clouds = []
    for b, n in enumerate(lens):
        if pattern == "distinct":
            clouds.append(distinct_cloud(geo, n, seed + 17 * b))
        else:
            clouds.append(mixed_cloud(geo, n, 300, seed + 17 * b))
    starts = np.concatenate([[0], np.cumsum(lens)])
    props = dict(lengths=lens, starts=[int(s) for s in starts[:-1]], n=int(starts[-1]), tile=tile)
    return clouds, props


def revisit_cloud(tile, cells, tiles=4, geo=None, seed=3):
    """`cells` voxels opened by the first `cells` points (tile 0); every later tile -- the last one, of three points, included --
    holds only later points of those voxels, and the cloud's last point is one."""
    geo = geo or grid_geometry(64, 64, 4)
    assert cells <= tile
    rng = np.random.default_rng(seed)
    total = int(np.prod(grid_of(*geo)))
    pool = rng.permutation(total)[:cells]
    n = tiles * tile + 3
    lin = np.concatenate([pool, pool[rng.integers(0, cells, n - cells)]])
    return cell_points(geo, lin_cells(geo, lin), seed + 1), dict(n=n, cells=cells, tile=tile)


def pillar_runs(lengths, interleave=True, geo=None, seed=5, min_points=3 * 1024 + 100):
    """A few pillars of the given point counts, their points interleaved at random over the whole cloud (``interleave``; otherwise
    pillar after pillar), padded with single-point pillars to at least three 1 024-point groups of k_vox_group_rank.
    -> (cloud, props): props["labels"] = pillar of every point (-1: filler)."""
    geo = geo or grid_geometry(64, 64, 1)
    rng = np.random.default_rng(seed)
    total = int(np.prod(grid_of(*geo)))
    filler = max(min_points - int(np.sum(lengths)), 64)
    pool = rng.permutation(total)[:len(lengths) + filler]
    labels = np.concatenate([np.full(n, i) for i, n in enumerate(lengths)] + [-np.ones(filler, np.int64)]).astype(np.int64)
    lin = np.concatenate([np.full(n, pool[i]) for i, n in enumerate(lengths)] + [pool[len(lengths):]])
    if interleave:
        perm = rng.permutation(len(lin))
        labels, lin = labels[perm], lin[perm]
    return cell_points(geo, lin_cells(geo, lin), seed + 1), dict(labels=labels, lengths=list(lengths), n=len(lin))


def model_run_order(indices, group=1024):
    """A run as k_vox_group_rank + k_vox_run_scatter may lay it out: the points of one 1 024-point group stay together, the groups in
    the order their atomicAdd on the counter lands -- here LAST group first (any order but ascending leaves small indices behind)."""
    indices = np.asarray(indices)
    g = indices // group
    return np.concatenate([indices[g == k] for k in sorted(set(g.tolist()), reverse=True)])


def cap_clouds(v, open_last_at=None, tail=40, geo=None, seed=7, quiet=8):
    """Exactly `v` distinct voxels: v - 1 opened by the first v - 1 points, revisits of them (the first `quiet` ones excepted) up to
    position ``open_last_at`` (default v + 20) where the LAST voxel opens -- the `break` position at max_voxels = v - 1 --, then
    `tail` revisits of the quiet early voxels (one point each so far: `break` or `continue` shows in their counts and slots) and
    revisits of the last voxel behind it."""
    geo = geo or grid_geometry(64, 64, 4)
    rng = np.random.default_rng(seed)
    total = int(np.prod(grid_of(*geo)))
    pool = rng.permutation(total)[:v]
    at = v + 20 if open_last_at is None else int(open_last_at)
    assert at >= v - 1 and v >= quiet + 2
    lin = np.concatenate([pool[:v - 1], pool[rng.integers(quiet, v - 1, at - (v - 1))], pool[v - 1:], pool[rng.integers(0, quiet, tail)],
                          pool[v - 1:], pool[:1], pool[v - 1:], pool[:1]])
    return cell_points(geo, lin_cells(geo, lin), seed + 1), dict(v=v, break_at=at, n=len(lin))


# ----------------------------------------------------------------------------------------------------------------- forms
DEFAULT_CONSTANTS = dict(kBlock=256, kFusedItems=2, kFusedFrames=64, kCascadeMaxPoints=8, kFlagItems=4, kFlagItemsBig=16, kStageDiv=8,
                         kVoxMaxPoints=256, big_scan_from=512 * 1024, staged_from=256 * 1024, small_table=1024, small_table_upto=512)


def read_constants():
    """The same numbers, read from the sources (a changed threshold must make the case table fail, not test one side only)."""
    src = open(VOXELIZE_HIP).read()
    out = {}
    for name in ("kFusedItems", "kFusedFrames", "kCascadeMaxPoints", "kFlagItems", "kFlagItemsBig", "kStageDiv", "kVoxMaxPoints"):
        out[name] = int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    out["kBlock"] = int(re.search(r"constexpr int kBlock = (\d+);", open(COMMON_HPP).read()).group(1))
    a, b = re.search(r"if \(num_points >= (\d+) \* (\d+)\)\s*\n\s*hipLaunchKernelGGL\(k_vox_flag_scan<kFlagItemsBig>", src).groups()
    out["big_scan_from"] = int(a) * int(b)
    a, b = re.search(r"staged_first = dense && num_points >= (\d+) \* (\d+);", src).groups()
    out["staged_from"] = int(a) * int(b)
    a, b, c = re.search(r"w\.table = next_pow2\(\(uint32_t\)\(n > (\d+) \? (\d+) \* \(size_t\)n : (\d+)\)\);", src).groups()
    assert int(b) == 2
    out["small_table_upto"], out["small_table"] = int(a), int(c)
    return out


def next_pow2(x):
    return 1 << max(int(x) - 1, 0).bit_length()


def forms(n, B, max_points, max_voxels, cells, fill=True, features=4, mean=True, aligned=True, k=DEFAULT_CONSTANTS):
    """The five choices of voxelize_impl / carve_vox for one call (n = points.shape[0], cells = cells of one cloud's grid)."""
    if max_points > k["kVoxMaxPoints"]:
        return dict(refused=True)
    table = k["small_table"] if n <= k["small_table_upto"] else next_pow2(2 * n)
    run = max_points > k["kCascadeMaxPoints"] and n > 0
    dense = run and not fill and B * cells <= table
    staged = dense and n >= k["staged_from"]
    peek = n > 2 * B * max_voxels
    fused = n > 0 and B <= k["kFusedFrames"] and max_points <= k["kCascadeMaxPoints"]
    if n == 0:
        first, scan = "none", "none"
    else:
        first = "dense+staged" if staged else "dense" if dense else "hash+peek" if peek else "hash"
        scan = "fused" if fused else "flag16" if n >= k["big_scan_from"] else "flag4"
    frames = "lds" if (n > 0 and B <= k["kFusedFrames"]) else "k_vox_frames"
    slots = "none" if n == 0 else "cascade" if not run else "select<%d>" % (1 if max_points <= 64 else 2 if max_points <= 128 else 4)
    if not fill:
        epi = "counts"
    elif mean and features == 4 and max_points <= k["kCascadeMaxPoints"] and aligned:
        epi = "fill_mean4"
    else:
        epi = "fill+mean" if mean else "fill"
    tile = k["kBlock"] * (k["kFusedItems"] if scan == "fused" else k["kFlagItemsBig"] if scan == "flag16" else k["kFlagItems"])
    return dict(first=first, scan=scan, frames=frames, slots=slots, epilogue=epi, table=table, tile=tile, keys=not dense, refused=False)


# ----------------------------------------------------------------------------------------------------------------- case table
class Case:
    """One GPU input: ``build()`` -> list of clouds; the other fields are the arguments of ops.voxelize and the forms it must take."""

    def __init__(self, name, geo, build, max_points, max_voxels, cap_mode="break", fill=True, nf=None, dtype="float32",
                 encoder="SimpleVoxel", expect=None, features=4, spare_rows=0, host=True):
        self.name, self.geo, self._build = name, geo, build
        self.max_points, self.max_voxels, self.cap_mode, self.fill = max_points, max_voxels, cap_mode, fill
        self.features = features
        self.nf = (features if fill else 0) if nf is None else nf
        self.dtype, self.encoder, self.expect = dtype, encoder, dict(expect or {})
        self.spare_rows = spare_rows       # in-range rows behind point_offsets[B] that must open no voxel
        self.host = host                   # small enough for the sequential statements on the CPU
        self._clouds = None

    def clouds(self):
        if self._clouds is None:
            self._clouds = [np.ascontiguousarray(c, np.float32) for c in self._build()]
            for c in self._clouds:
                c.setflags(write=False)
        return self._clouds

    def spare(self):
        return mixed_cloud(self.geo, self.spare_rows, 50, 991, self.features) if self.spare_rows else None

    def forms(self, k=DEFAULT_CONSTANTS):
        n = sum(len(c) for c in self.clouds()) + self.spare_rows
        return forms(n, len(self.clouds()), self.max_points, self.max_voxels, int(np.prod(grid_of(*self.geo))), self.fill,
                     self.features, bool(self.nf), True, k)

    def reference(self):
        return ref_voxelize(self.clouds(), self.geo[1], self.geo[0], self.max_points, self.max_voxels, self.cap_mode)


def _cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    G = grid_geometry(64, 64, 4)
    # --- cell arithmetic: every border of five geometries, fused path, run path with and without the voxel tensor
    for g in BOUNDARY_GEOMETRIES:
        geo = geometry(g)
        b = (lambda geo=geo: [boundary_points(geo)[0]])
        add(f"cells/{g}/fused", geo, b, 5, 100000, expect=dict(scan="fused", slots="cascade", epilogue="fill_mean4"))
        add(f"cells/{g}/run", geo, b, 60, 100000, expect=dict(scan="flag4", slots="select<1>", first="hash"))
        add(f"cells/{g}/run-nofill", geo, b, 60, 100000, fill=False, expect=dict(slots="select<1>", epilogue="counts"))
    # --- fused scan tiles (512 points)
    for n in (1, 2, 3, 511, 512, 513, 1023, 1024, 1025, 2571):
        add(f"fused/n{n}", G, (lambda n=n: [mixed_cloud(G, n, max(n // 3, 1), n)]), 5, 100000, expect=dict(scan="fused", tile=512))
    for B, pat in ((1, "shared"), (2, "shared"), (63, "shared"), (64, "shared"), (64, "distinct"), (64, "one")):
        for cap in ("break", "continue"):
            add(f"fused/tiles/B{B}/{pat}/{cap}", G, (lambda B=B, pat=pat: tile_clouds(512, B, pat)[0]), 3, 150, cap,
                expect=dict(scan="fused", frames="lds"))
    add("fused/revisit", G, lambda: [revisit_cloud(512, 200)[0]], 8, 100000, expect=dict(scan="fused"))
    for T in (1, 2, 8):
        add(f"fused/T{T}", G, lambda: [revisit_cloud(512, 37)[0], mixed_cloud(G, 700, 90, 4)], T, 100000, expect=dict(scan="fused"))
    for at in (511, 512):
        for V in (59, 60, 61, 1):
            for cap in ("break", "continue"):
                add(f"fused/cap/at{at}/V{V}/{cap}", G, (lambda at=at: [cap_clouds(60, at)[0], cap_clouds(60, at, seed=8)[0]]), 5, V, cap,
                    expect=dict(scan="fused"))
    # --- unfused scan: 1 024-point tiles, k_vox_frames at 65 clouds, 4 096-point tiles from 524 288 points
    for pat in ("shared", "distinct"):
        for cap in ("break", "continue"):
            add(f"flag4/tiles/B65/{pat}/{cap}", G, (lambda pat=pat: tile_clouds(1024, 65, pat)[0]), 3, 150, cap,
                expect=dict(scan="flag4", frames="k_vox_frames", slots="cascade"))
            add(f"flag4/tiles/B12/T9/{pat}/{cap}", G, (lambda pat=pat: tile_clouds(1024, 12, pat)[0]), 9, 150, cap,
                expect=dict(scan="flag4", frames="lds", slots="select<1>"))
    add("flag4/revisit/T9", G, lambda: [revisit_cloud(1024, 300)[0]], 9, 100000, expect=dict(scan="flag4"))
    add("flag4/revisit/B65", G, lambda: [revisit_cloud(1024, 300)[0]] + [mixed_cloud(G, 5, 3, s) for s in range(64)], 4, 100000,
        expect=dict(scan="flag4", frames="k_vox_frames"))
    for at in (1023, 1024):
        for V in (59, 60, 61, 1):
            for cap in ("break", "continue"):
                add(f"flag4/cap/at{at}/V{V}/{cap}", G, (lambda at=at: [cap_clouds(60, at)[0], cap_clouds(60, at, seed=8)[0]]), 9, V, cap,
                    expect=dict(scan="flag4"))
            add(f"flag4/cap/at{at}/V{V}/B65", G, (lambda at=at: [cap_clouds(60, at)[0]] * 65), 3, V, "break",
                expect=dict(scan="flag4", frames="k_vox_frames"))
    GB = grid_geometry(128, 128, 1)
    for n, scan in ((524287, "flag4"), (524288, "flag16")):
        add(f"big/n{n}", GB, (lambda n=n: [mixed_cloud(GB, n - 200000, 3000, 21), mixed_cloud(GB, 200000, 2500, 22)]), 9, 5000,
            expect=dict(scan=scan, slots="select<1>", first="hash+peek"), host=False)
    # --- hash: table-size switch, peek switch, load factor 1/2, one cell
    for n in (512, 513):
        for T in (5, 9):
            add(f"hash/table/n{n}/T{T}", G, (lambda n=n: [distinct_cloud(G, n, n)]), T, 100000, expect=dict(table=1024 if n == 512 else 2048, first="hash"))
    for n, first in ((600, "hash"), (601, "hash+peek")):
        for T in (5, 9):
            add(f"hash/peek/n{n}/T{T}", G, (lambda n=n: [mixed_cloud(G, n, 350, n)]), T, 300, expect=dict(first=first))
    for T in (5, 9):
        add(f"hash/full/T{T}", G, lambda: [distinct_cloud(G, 1024, 77)], T, 100000, expect=dict(table=2048, first="hash"))
        add(f"hash/onecell/T{T}", G, lambda: [cell_points(G, np.tile([[5, 6, 1]], (1024, 1)), 78)], T, 100000, expect=dict(table=2048))
    # --- slots
    GP = grid_geometry(64, 64, 1)
    for T, slots in ((8, "cascade"), (9, "select<1>"), (64, "select<1>"), (65, "select<2>"), (128, "select<2>"), (129, "select<4>"),
                     (256, "select<4>")):
        add(f"slots/T{T}/edges", GP, (lambda T=T: [pillar_runs([T - 1, T, T + 1])[0]]), T, 100000, expect=dict(slots=slots))
    for T in (60, 100, 200, 256):
        add(f"slots/T{T}/runs", GP, lambda: [pillar_runs([63, 64, 65, 127, 128, 129, 255, 256, 257, 1000])[0]], T, 100000,
            expect=dict(slots="select<%d>" % (1 if T <= 64 else 2 if T <= 128 else 4)))
        if T <= 200:       # (the PillarFeatureNet that reads the lists is held to 200 slots by its own edge suite)
            add(f"slots/T{T}/runs/nofill", GP, lambda: [pillar_runs([63, 64, 65, 127, 128, 129, 255, 256, 257, 1000])[0]], T, 100000,
                fill=False, expect=dict(first="dense"))
    # --- dense numbering (no voxel tensor, max_points > 8): B * cells on both sides of the table size
    for gx, first in ((32, "dense"), (34, "hash")):
        g = grid_geometry(gx, 32, 1)
        add(f"dense/n500/{gx}x32", g, (lambda g=g: [mixed_cloud(g, 500, 200, 31)]), 20, 100000, fill=False, expect=dict(first=first, table=1024))
        add(f"dense/n500/{gx}x32/B2", g, (lambda g=g: [mixed_cloud(g, 250, 200, 31), mixed_cloud(g, 250, 100, 32)]), 20, 100000, fill=False,
            expect=dict(first="hash", table=1024))
    for gx, first in ((128, "dense"), (129, "hash")):
        g = grid_geometry(gx, 64, 1)
        for cap, V in (("break", 100000), ("break", 700), ("continue", 700)):
            add(f"dense/n3000/{gx}x64/{cap}{V}", g, (lambda g=g: [mixed_cloud(g, 3000, 1500, 33)]), 20, V, cap, fill=False,
                expect=dict(first=first if first == "dense" or V > 1500 else "hash+peek", table=8192))
    GS = grid_geometry(256, 256, 1)
    for n, first in ((262143, "dense"), (262144, "dense+staged")):
        add(f"dense/staged/n{n}", GS, (lambda n=n: [mixed_cloud(GS, 150000, 20000, 41), mixed_cloud(GS, 0, 1, 42), mixed_cloud(GS, n - 150000 - 16, 9000, 43),
                                                    mixed_cloud(GS, 16, 16, 44)]), 12, 15000, "break", fill=False, expect=dict(first=first), host=False)
    # --- capacity rows behind point_offsets[B] on the four first-point forms (the spare rows count into n)
    add("spare/hash", G, lambda: [mixed_cloud(G, 400, 120, 51), mixed_cloud(G, 300, 80, 52)], 5, 100000, spare_rows=333, expect=dict(first="hash", scan="fused"))
    add("spare/peek", G, lambda: [mixed_cloud(G, 400, 120, 51), mixed_cloud(G, 300, 80, 52)], 9, 150, spare_rows=333, expect=dict(first="hash+peek"))
    add("spare/dense", grid_geometry(32, 32, 1), lambda: [mixed_cloud(grid_geometry(32, 32, 1), 700, 300, 53)], 12, 100000, fill=False,
        spare_rows=333, expect=dict(first="dense"))
    add("spare/staged", GS, lambda: [mixed_cloud(GS, 140000, 20000, 54), mixed_cloud(GS, 120000, 9000, 55)], 12, 100000, fill=False,
        spare_rows=3000, expect=dict(first="dense+staged"), host=False)
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


# ----------------------------------------------------------------------------------------------------------------- emulation
MISTAKES = ("reciprocal", "trunc", "le_grid", "neg_zero", "break_as_continue", "continue_as_break", "batch_cap", "by_cell",
            "slots_reversed", "last_points", "uncapped_count", "div_max_points", "reverse_sum", "truncate16")


def emulate(clouds, geo, max_points, max_voxels, cap_mode, nf=0, dtype="float32", encoder="SimpleVoxel", mistake=None):
    """The voxeliser as its kernels state it, sequentially: cells by fp32 subtract / divide / floor (k_vox_hash), a voxel per first
    touch, the first max_points arrivals, the cap per cloud, means by T fp32 additions from +0.0 and one division, one rounding to a
    16-bit type.  ``mistake``: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    range6, vs = geo
    r, v = np.asarray(range6, np.float32), np.asarray(vs, np.float32)
    grid = grid_of(range6, vs)
    gf = grid.astype(np.float32)
    T, V = int(max_points), int(max_voxels)
    brk = cap_mode == "break"
    if (mistake, cap_mode) in (("break_as_continue", "break"), ("continue_as_break", "continue")):
        brk = not brk
    vox, coo, npv, offs, made = [], [], [], [0], 0
    F = clouds[0].shape[1]
    for b, pts in enumerate(clouds):
        with np.errstate(all="ignore"):
            d = pts[:, :3] - r[:3]
            q = d * (np.float32(1) / v) if mistake == "reciprocal" else d / v
            q = np.trunc(q) if mistake == "trunc" else np.floor(q)
            ok = (q >= 0) & ((q <= gf) if mistake == "le_grid" else (q < gf))
            if mistake == "neg_zero":
                ok &= ~np.signbit(q)
        ok = ok.all(1)
        cells = np.where(ok[:, None], q, 0).astype(np.int64)
        table, members, first_cell = {}, [], []
        for i in np.nonzero(ok)[0]:
            key = (int(cells[i, 2]), int(cells[i, 1]), int(cells[i, 0]))
            vid = table.get(key)
            if vid is None:
                if (made + len(members) if mistake == "batch_cap" else len(members)) >= V:
                    if brk:
                        break
                    continue
                vid = table[key] = len(members)
                members.append([])
                first_cell.append(key)
            members[vid].append(i)
        made += len(members)
        order = sorted(range(len(members)), key=lambda j: first_cell[j]) if mistake == "by_cell" else range(len(members))
        voxels = np.zeros((len(members), T, F), np.float32)
        for row, j in enumerate(order):
            m = members[j][-T:] if mistake == "last_points" else members[j][:T]
            if mistake == "slots_reversed":
                m = m[::-1]
            voxels[row, :len(m)] = pts[m]
            npv.append(len(members[j]) if mistake == "uncapped_count" else min(len(members[j]), T))
            coo.append((b,) + first_cell[j])
        vox.append(voxels)
        offs.append(offs[-1] + len(members))
    out = {"voxels": np.concatenate(vox), "coordinates": np.asarray(coo, np.int32).reshape(-1, 4),
           "num_points_per_voxel": np.asarray(npv, np.int32), "voxel_offsets": np.asarray(offs, np.int32)}
    if nf:
        k = 4 if encoder == "SimpleVoxelRadius" else nf
        x, cnt = out["voxels"], out["num_points_per_voxel"]
        s = np.zeros((x.shape[0], k), np.float32)
        with np.errstate(all="ignore"):
            if mistake == "reverse_sum":
                for row in range(x.shape[0]):
                    for t in range(min(int(cnt[row]), T) - 1, -1, -1):
                        s[row] = s[row] + x[row, t, :k]
            else:
                for t in range(T):
                    s = s + x[:, t, :k]
            m = s / (np.float32(T) if mistake == "div_max_points" else cnt.astype(np.float32)[:, None])
            if encoder == "SimpleVoxelRadius":
                m = np.stack([np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]), m[:, 2], m[:, 3], np.zeros_like(m[:, 0])], 1)
        if dtype != "float32" and mistake == "truncate16":
            bits = m.astype(np.float32).view(np.int32) & (~0xffff if dtype == "bfloat16" else ~0x1fff)
            m = bits.view(np.float32)
        out["mean"] = round_to(m, dtype)
    return out
