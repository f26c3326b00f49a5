"""Produces tests/golden/voxel_edges.npz by EXECUTING the reference's own voxelisation loop
(second/utils/simplevis.py:8-60, ``_points_to_bevmap_reverse_kernel``: the in-repo copy of spconv's points_to_voxel) on CPU.
Build container only (needs the reference checkout; execution shims of make_golden.py, no reference text is copied):

    python tests/golden/make_golden_voxel_edges.py

Inputs: ``voxel_ref_helpers.boundary_points`` of five geometries -- kitti/car.fhd, nuscenes/all.pp.largea, kitti/pointpillars,
nuscenes/all.fhd (``models.ALL_FHD_NUSC``) and the coarse cap geometry of voxel_coords.npz: every cell border fl(lo + fl(k vs)) of
every axis with its two fp32 neighbours, hi and its neighbour below, lo's neighbour below, +-0.0 and the smallest subnormal.  The
full sets fit the size limit of a committed file (160 kB compressed), so STRIDE is 1 everywhere; a larger stride would keep
k = 0, grid - 1, grid and every k at which a reciprocal multiply or float64 arithmetic changes a cell.  Per geometry ``<g>``: ``<g>_points``, ``<g>_range``, ``<g>_voxel_size``; the loop run without a cap
(``<g>_coors``: voxel coordinates (z, y, x) in voxel order; ``<g>_density``: rows (y, x, count) of the non-zero columns of
``bev[-1]``, the points counted per column) and with a cap reached in the middle of the set (``<g>_cap``, ``<g>_cap_coors``,
``<g>_cap_density``)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "second.pytorch_amd"), ROOT]

STRIDE = {"kitti": 1, "nusc_pp": 1, "kitti_pp": 1, "nusc_fhd": 1, "coarse": 1}


def run_loop(simplevis, pts, vs, pr, cap):
    grid = np.round((pr[3:] - pr[:3]) / vs).astype(np.int32)
    lookup = -np.ones(tuple(int(g) for g in grid[::-1]), np.int32)
    bev = np.zeros((int(grid[2]) + 2, int(grid[1]), int(grid[0])), np.float32)
    lowers = np.linspace(pr[2], pr[5], int(grid[2]), endpoint=False).astype(np.float32)
    simplevis._points_to_bevmap_reverse_kernel(pts, vs, pr, lookup, bev, lowers, False, cap)
    zyx = np.argwhere(lookup >= 0)
    order = np.argsort(lookup[lookup >= 0])
    yx = np.argwhere(bev[-1] > 0)
    density = np.concatenate([yx, bev[-1][bev[-1] > 0].astype(np.int64)[:, None]], 1).astype(np.int32)
    return zyx[order].astype(np.int32), density


def main():
    import voxel_ref_helpers as H
    geos = {g: H.geometry(g) for g in H.BOUNDARY_GEOMETRIES}       # (before the shims replace `spconv`)
    import make_golden
    make_golden.install_shims()
    from second.utils import simplevis
    out = {}
    for g, geo in geos.items():
        pts, _ = H.boundary_points(geo, STRIDE[g])
        pr, vs = np.asarray(geo[0], np.float32), np.asarray(geo[1], np.float32)
        coors, density = run_loop(simplevis, pts, vs, pr, 1 << 30)
        cap = len(coors) // 2
        cap_coors, cap_density = run_loop(simplevis, pts, vs, pr, cap)
        assert len(cap_coors) == cap
        out.update({f"{g}_points": pts, f"{g}_range": pr, f"{g}_voxel_size": vs, f"{g}_stride": np.int64(STRIDE[g]), f"{g}_coors": coors,
                    f"{g}_density": density, f"{g}_cap": np.int64(cap), f"{g}_cap_coors": cap_coors, f"{g}_cap_density": cap_density})
        print(g, "points", len(pts), "voxels", len(coors), "cap", cap)
    path = os.path.join(HERE, "voxel_edges.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
