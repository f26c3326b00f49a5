"""Cover lists of the RPN (sec_rpn_tile_cover): per conv l, frame and 8-row band the pixels within Chebyshev distance l + 1 of a site
are covered by tiles placed at free x -- walk x from 0, at a reachable column emit tile (band, x) and advance by 16, otherwise by 1.
The device's lists, counts, coverage masks C_l and halo masks (rank-indexed and grid-indexed) against a numpy implementation of that
rule, on maps ragged in both directions, empty and full frames and single sites in the corners and the last column."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dilate(m, k):
    """[H, W] bool -> pixels within Chebyshev distance k of a set one"""
    h, w = m.shape
    p = np.zeros((h + 2 * k, w + 2 * k), bool)
    p[k:k + h, k:k + w] = m
    out = np.zeros((h, w), bool)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def cover_reference(sites, layers):
    """sites [B, H, W] bool -> per layer: lists [l][b] of (band, x0), cols [l, B, bands, W] bool, grid-live tiles per band [l, B, bands]"""
    b, h, w = sites.shape
    bands = (h + 7) // 8
    lists = [[[] for _ in range(b)] for _ in range(layers)]
    cols = np.zeros((layers, b, bands, w), bool)
    grid = np.zeros((layers, b, bands), np.int64)
    for l in range(layers):
        for f in range(b):
            reach = dilate(sites[f], l + 1)
            for ty in range(bands):
                r = reach[8 * ty:8 * ty + 8].any(0)
                grid[l, f, ty] = sum(bool(r[x:x + 16].any()) for x in range(0, w, 16))
                x = 0
                while x < w:
                    if r[x]:
                        lists[l][f].append((ty, x))
                        cols[l, f, ty, x:x + 16] = True
                        x += 16
                    else:
                        x += 1
                assert not (r & ~cols[l, f, ty]).any()            # C is a superset of R
    return lists, cols, grid


def halo_reference(cols_prev, ty, x0):
    """three 18-bit masks of tile (ty, x0) from the producing layer's coverage [bands, W] bool; outside the image counts as written"""
    bands, w = cols_prev.shape
    out = []
    for ry in range(3):
        yb, m = ty - 1 + ry, 0
        for hx in range(18):
            x = x0 - 1 + hx
            if not (0 <= yb < bands) or not (0 <= x < w) or cols_prev[yb, x]:
                m |= 1 << hx
        out.append(m)
    return out


def unpack_cols(words, w):
    """[..., ceil(W / 32)] int32 words -> [..., W] bool"""
    u = words.astype(np.int64) & 0xffffffff
    bits = (u[..., :, None] >> np.arange(32)) & 1
    return bits.reshape(*u.shape[:-1], -1)[..., :w].astype(bool), bits.reshape(*u.shape[:-1], -1)[..., w:]


def site_maps(kind, h, w):
    """[2, H, W] bool"""
    rng = np.random.default_rng(h * 131 + w)
    s = np.zeros((2, h, w), bool)
    if kind == "random":                                  # a few blobs and lone sites: most bands hold gaps, some straddle grid lines
        for f in range(2):
            n = 5 + 3 * f
            s[f, rng.integers(0, h, n), rng.integers(0, w, n)] = True
    elif kind == "empty_full":
        s[1] = True
    elif kind == "corners":
        s[0, [0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
        s[1, h // 2, w - 1] = True
    return s


@pytest.mark.parametrize("kind", ["random", "empty_full", "corners"])
@pytest.mark.parametrize("h,w", [(24, 40), (40, 48), (17, 21)])
def test_cover_lists_follow_the_greedy_rule(h, w, kind):
    from second_amd import ops
    sites = site_maps(kind, h, w)
    smap = np.zeros((2, 2, h, w), np.int32)
    smap[:, 0][sites] = 7                                  # either plane marks a site
    smap[:, 1][sites & (np.arange(w) % 2 == 0)] = 3
    smap[:, 0][sites & (np.arange(w) % 2 == 0)] = 0
    dev = torch.from_numpy(smap).cuda()
    bands, tx = (h + 7) // 8, (w + 15) // 16
    tiles = bands * tx
    assert ops.rpn_tile_cover_supported(h, w, 7)
    for layers in range(1, 8):
        order_g, counts_g, cv = ops.rpn_tile_live(dev, layers, cover=True)
        order_p, counts_p = ops.rpn_tile_live(dev, layers)                   # the grid lists beside them are sec_rpn_tile_live's
        assert torch.equal(counts_g, counts_p)
        for l in range(layers):
            for f in range(2):
                c = int(counts_p[l, f])
                assert torch.equal(order_g[l, f, :c], order_p[l, f, :c])
        lists, cols, grid = cover_reference(sites, layers)
        order = cv.order.cpu().numpy().astype(np.int64) & 0xffff
        counts = cv.counts.cpu().numpy()
        got_cols, beyond = unpack_cols(cv.cols.cpu().numpy(), w)
        halo = cv.halo.cpu().numpy().astype(np.int64) & 0xffffffff
        assert tuple(cv.order.shape) == (layers, 2, tiles) and tuple(cv.halo.shape) == (layers, 2, 2, tiles, 3)
        assert not beyond.any()
        np.testing.assert_array_equal(got_cols, cols)
        for l in range(layers):
            for f in range(2):
                want = lists[l][f]
                assert counts[l, f] == len(want) <= int(counts_p[l, f])
                np.testing.assert_array_equal(order[l, f, :len(want)], [ty * w + x0 for ty, x0 in want])
                per_band = np.bincount([ty for ty, _ in want], minlength=bands)
                assert (per_band <= grid[l, f]).all()                         # never more tiles than the grid has live ones in a band
                assert grid[l, f].sum() == int(counts_p[l, f])
                if l >= 1:
                    ranked = np.array([halo_reference(cols[l - 1, f], ty, x0) for ty, x0 in want], np.int64).reshape(-1, 3)
                    np.testing.assert_array_equal(halo[l, 0, f, :len(want)], ranked)
                    np.testing.assert_array_equal(halo[l, 1, f], [halo_reference(cols[l - 1, f], t // tx, (t % tx) * 16) for t in range(tiles)])
    if kind == "empty_full":
        assert counts[:, 0].sum() == 0 and (counts[:, 1] == tiles).all()
    if kind == "corners" and w % 16:
        assert any(x0 + 16 > w for _, x0 in lists[0][1]), "the site in the last column must give a tile that sticks out past the edge"


def test_cover_lists_are_refused_where_an_entry_does_not_fit_16_bits():
    from second_amd import ops
    assert not ops.rpn_tile_cover_supported(4096, 129, 6)        # 512 bands x 129 columns > 65535
    assert ops.rpn_tile_cover_supported(200, 176, 6) and ops.rpn_tile_cover_supported(160, 132, 6)
