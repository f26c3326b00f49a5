"""CPU replay of the RPN's live-tile lists on the bench's eight clouds: fixed 8 x 16 grid against the per-band cover.

    python tools/rpn_tile_cover_replay.py [--frames 8] [--scene open]

numpy only, no GPU.  syn_kitti_cloud(0..7) -> occupied car.fhd voxel cells -> the three k3 / s2 / p1 levels of the sparse middle
(projected on the BEV plane: every level keeps at least one z output per input) -> for conv j = 0..5 the pixels within Chebyshev
distance j + 1 of a site.  Per conv it prints
  * the tiles of the fixed 8 x 16 grid that hold such a pixel (what sec_rpn_tile_live lists), and
  * the tiles of the greedy cover of sec_rpn_tile_cover: per 8-row band, walk x from 0; at a reachable column emit a tile and
    advance by 16, otherwise advance by 1,
summed over the frames, plus the share of the grid tiles' pixels that are reachable and the share of their 16-pixel rows that are.
"""
import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _synthetic():
    # loaded by path: the package's __init__ imports torch, this tool must not need it
    spec = importlib.util.spec_from_file_location("sec_synthetic", os.path.join(HERE, "..", "second.pytorch_amd", "second_amd", "synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bev_sites(cloud, rng_, vox):
    """[H, W] bool: cells of the RPN's input map (after three stride-2 levels) that hold a site."""
    lo = np.array(rng_[:3], np.float32)
    grid = np.round((np.array(rng_[3:]) - np.array(rng_[:3])) / np.array(vox)).astype(np.int64)       # (x, y, z) cells
    cells = np.floor((cloud[:, :3] - lo) / np.array(vox, np.float32)).astype(np.int64)
    m = np.zeros((grid[1], grid[0]), bool)
    m[cells[:, 1], cells[:, 0]] = True
    for _ in range(3):            # k3 / s2 / p1: output o sees inputs 2 o - 1 .. 2 o + 1
        h, w = m.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        p = np.zeros((2 * ho + 1, 2 * wo + 1), bool)
        p[1:h + 1, 1:w + 1] = m
        rows = p[0:2 * ho:2] | p[1:2 * ho + 1:2] | p[2:2 * ho + 2:2]
        m = rows[:, 0:2 * wo:2] | rows[:, 1:2 * wo + 1:2] | rows[:, 2:2 * wo + 2:2]
    return m


def dilate(m, k):
    """Pixels within Chebyshev distance k of a set pixel."""
    h, w = m.shape
    p = np.zeros((h + 2 * k, w + 2 * k), bool)
    p[k:k + h, k:k + w] = m
    rows = np.zeros((h, w + 2 * k), bool)
    for d in range(2 * k + 1):
        rows |= p[d:d + h]
    out = np.zeros((h, w), bool)
    for d in range(2 * k + 1):
        out |= rows[:, d:d + w]
    return out


def cover_band(r):
    """x0 of the greedy cover's tiles for one band's reachable-column row ``r`` [W] bool."""
    xs, x, w = [], 0, r.shape[0]
    while x < w:
        if r[x]:
            xs.append(x)
            x += 16
        else:
            x += 1
    return xs


def replay(sites, convs=6):
    """Per conv: (grid tiles, cover tiles, reachable pixels in the grid's live tiles, their pixels, live 16-pixel rows, their rows)."""
    h, w = sites.shape
    out = []
    for j in range(convs):
        reach = dilate(sites, j + 1)
        grid = cover = px = rows = 0
        for y0 in range(0, h, 8):
            band = reach[y0:y0 + 8]
            cover += len(cover_band(band.any(0)))
            for x0 in range(0, w, 16):
                t = band[:, x0:x0 + 16]
                if t.any():
                    grid += 1
                    px += int(t.sum())
                    rows += int(t.any(1).sum())
        out.append((grid, cover, px, grid * 128, rows, grid * 8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--scene", default="open")
    args = ap.parse_args()
    syn = _synthetic()
    tot = np.zeros((6, 6), np.int64)
    for s in range(args.frames):
        tot += np.array(replay(bev_sites(syn.syn_kitti_cloud(s, scene=args.scene), syn.CAR_FHD_RANGE, syn.CAR_FHD_VOXEL)))
    fmt = lambda v: " ".join(f"{x:>6}" for x in v)
    print("conv j                                 " + fmt(range(6)) + "      sum")
    print("live tiles, fixed 8x16 grid            " + fmt(tot[:, 0]) + f" {tot[:, 0].sum():>8}")
    print("reachable share of those tiles' pixels " + fmt(f"{a / b:.2f}" for a, b in zip(tot[:, 2], tot[:, 3])))
    print("tiles, per-band cover at free x        " + fmt(tot[:, 1]) + f" {tot[:, 1].sum():>8}")
    print("live 16-pixel rows in the grid's tiles " + fmt(f"{a / b:.2f}" for a, b in zip(tot[:, 4], tot[:, 5])))


if __name__ == "__main__":
    main()
