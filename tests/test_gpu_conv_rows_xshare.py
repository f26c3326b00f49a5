"""The x-share forms of k_conv_rows_buf (csrc/indice_conv.hip, FL bit 13): a lane whose neighbour row at (dz, dy, -1) or (dz, dy, +1) is the
row the lane beside it gathers at (dz, dy, 0) issues no memory request for it and takes that lane's centre fragment through a DPP wave
shift.  Same operand, same MFMA, same position in the k = 0..26 sequence: the output must equal the old form's BIT FOR BIT, and both
must agree with the fp64-accumulating oracle within one rounding of the 16-bit store (the tolerance of tests/test_gpu_parity.py).

Forms (sec_indice_conv_set_variant: 80 / 82 = old, 81 / 83 = sharing; 80 / 81 keep the automatic choice, 82 / 83 force the kernel like 22):
  64w8  k_conv_rows_buf<T, 64, 64, 27, 3, 8, 3, 2689 | 10881>   the 56 k-row layers        (forced: any row count)
  64w4  k_conv_rows_buf<T, 64, 64, 27, 3, 4, 2, 2689 | 10881>   the 23 k-row layers        (automatic choice, 8192 <= rows < 40000)
  32    k_conv_rows_buf<T, 32, 32, 27, 6, 8, 2, 2115 | 10307>   the 32 -> 32 layers        (forced: any row count)

The CPU test at the end models the rule in numpy on the oracle's rulebooks of one synthetic cloud.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc  # noqa: E402  (test infrastructure only)

gpu = pytest.mark.gpu

#        cin, cout, old variant, sharing variant, waves, FL old, FL sharing
FORMS = {"64w8": (64, 64, 82, 83, 8, 2689, 10881),
         "64w4": (64, 64, 80, 81, 4, 2689, 10881),
         "32": (32, 32, 82, 83, 8, 2115, 10307)}
K_BAL_WGS = 256


def slab_rows(n, waves):
    """Rows per wave (`rw` of k_conv_rows_buf, FL bit 11): the launch fills 256 workgroups once; a multiple of 4 in 4..32."""
    per_wg = -(-n // K_BAL_WGS)
    rw = (-(-per_wg // waves) + 3) & ~3
    return min(max(rw, 4), 32)


def share_model(nbr, n_live, rw):
    """numpy model of the kernel's share rule on a gather table [n, 27] whose first n_live rows are live, slabs of rw rows per wave.
    Returns (left[n_live, 9], right[n_live, 9]): offset 3g of the row comes from the lane on its left / offset 3g + 2 from its right."""
    t = nbr[:n_live].reshape(n_live, 9, 3)
    lane = np.arange(n_live) % rw
    left = np.zeros((n_live, 9), bool)
    right = np.zeros((n_live, 9), bool)
    has_l = lane > 0                                         # same slab (a slab is at most 32 lanes = one half-wave), lane live
    has_r = (lane < rw - 1) & (np.arange(n_live) + 1 < n_live)
    left[1:] = has_l[1:, None] & (t[1:, :, 0] >= 0) & (t[1:, :, 0] == t[:-1, :, 1])
    right[:-1] = has_r[:-1, None] & (t[:-1, :, 2] >= 0) & (t[:-1, :, 2] == t[1:, :, 1])
    return left, right


def sort_cells(idx, shape):
    lin = ((idx[:, 0].astype(np.int64) * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
    return np.ascontiguousarray(idx[np.argsort(lin, kind="stable")])


def subm_table(idx, batch, shape):
    _, pairs, pair_num = orc.rulebook_subm(idx, batch, shape, 3)
    nbr = -np.ones((len(idx), 27), np.int32)
    for k in range(27):
        p = pairs[k, :, :pair_num[k]]
        nbr[p[1], k] = p[0]
    return nbr


def pairs_of(nbr, n_feat):
    """Rulebook (pairs[27, 2, n_feat], pair_num) of a gather table, for the oracle."""
    n = len(nbr)
    width = max(n, n_feat)
    pairs = -np.ones((27, 2, width), np.int32)
    pair_num = np.zeros(27, np.int32)
    for k in range(27):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        pairs[k, 0, :len(o)], pairs[k, 1, :len(o)], pair_num[k] = nbr[o, k], o, len(o)
    return pairs, pair_num


# ------------------------------------------------------------------ the cases: (gather table, feature rows, live rows or None)
def case_cloud():
    """Level-1 rulebook (the 32 -> 32 layers) of two bench clouds in sorted numbering: ~30 k rows, about half of all pairs shareable."""
    from second_amd import synthetic as syn
    idx = []
    for b in range(2):
        r = orc.points_to_voxel(syn.syn_kitti_cloud(b), syn.CAR_FHD_VOXEL, syn.CAR_FHD_RANGE, 5, 40000)
        idx.append(np.concatenate([np.full((r["voxel_num"], 1), b, np.int32), r["coordinates"]], 1))
    idx, shape = np.concatenate(idx), [41, 1600, 1408]
    idx, _, _, shape = orc.rulebook_conv(idx, 2, shape, 3, 2, 1)
    shape = [int(s) for s in shape]
    idx = sort_cells(idx, shape)
    nbr = subm_table(idx, 2, shape)
    return nbr, len(nbr), None


def case_cloud_static():
    """The same table as a static-capacity launch: the live count on the device, 517 rows short of the table -- the rows behind it are
    REAL rows of the same cloud, so the first dead lane holds exactly the centre index its live neighbour would share."""
    nbr, n, _ = case_cloud()
    return nbr, n, n - 517


def case_dense():
    """A fully dense 8 x 24 x 48 block: every interior dx = +-1 pair is shareable; 48-cell x-runs meet every slab phase."""
    shape = [8, 24, 48]
    z, y, x = np.meshgrid(np.arange(8), np.arange(24), np.arange(48), indexing="ij")
    idx = np.stack([np.zeros(z.size, np.int64), z.ravel(), y.ravel(), x.ravel()], 1).astype(np.int32)
    nbr = subm_table(sort_cells(idx, shape), 1, shape)
    return nbr, len(nbr), None


def case_isolated():
    """Every other x: the cells have y / z neighbours but no x-adjacent one, nothing is shareable."""
    shape = [8, 24, 96]
    z, y, x = np.meshgrid(np.arange(8), np.arange(24), np.arange(0, 96, 2), indexing="ij")
    idx = np.stack([np.zeros(z.size, np.int64), z.ravel(), y.ravel(), x.ravel()], 1).astype(np.int32)
    nbr = subm_table(sort_cells(idx, shape), 1, shape)
    return nbr, len(nbr), None


def _runs(n_target, seed):
    """x-runs of random length 1..70 with gaps of 1..3 cells on consecutive (z, y) lines, sorted numbering."""
    rng = np.random.default_rng(seed)
    shape = [40, 64, 400]
    cells = []
    total = 0
    for z in range(shape[0]):
        for y in range(shape[1]):
            x = int(rng.integers(0, 3))
            while True:
                ln = int(rng.integers(1, 71))
                if x + ln > shape[2]:
                    break
                cells.append(np.stack([np.zeros(ln, np.int64), np.full(ln, z), np.full(ln, y), np.arange(x, x + ln)], 1))
                total += ln
                x += ln + int(rng.integers(1, 4))
            if total >= n_target:
                break
        if total >= n_target:
            break
    idx = np.concatenate(cells).astype(np.int32)[:n_target]
    return subm_table(np.ascontiguousarray(idx), 1, shape)


def case_runs_small():
    """9 001 rows: slabs of 8 (eight-wave forms) or 12 rows (four-wave form), ragged last workgroup."""
    nbr = _runs(9001, 3)
    return nbr, len(nbr), None


def case_runs_mid():
    """33 003 rows: the four-wave form runs full 32-row slabs (lanes 0 and 31)."""
    nbr = _runs(33003, 4)
    return nbr, len(nbr), None


def case_runs_large():
    """60 005 rows: the eight-wave forms run full 32-row slabs (lanes 0 and 31)."""
    nbr = _runs(60005, 5)
    return nbr, len(nbr), None


def case_equal_indices():
    """Hand-made table: the lane beside holds the SAME index at its centre offset although the cells have nothing to do with each other
    (rows of a 500-row feature matrix drawn at random) -- legal, equal index = equal bytes, must share."""
    rng = np.random.default_rng(21)
    n, n_feat = 9003, 500
    t = rng.integers(-1, n_feat, (n, 9, 3)).astype(np.int32)
    t[rng.random((n, 9, 3)) < 0.3] = -1
    take_r = rng.random((n - 1, 9)) < 0.5
    t[:-1, :, 2] = np.where(take_r, t[1:, :, 1], t[:-1, :, 2])
    take_l = rng.random((n - 1, 9)) < 0.5
    t[1:, :, 0] = np.where(take_l, t[:-1, :, 1], t[1:, :, 0])
    return t.reshape(n, 27), n_feat, None


def case_minus_one():
    """Hand-made table: neighbouring lanes hold -1 at the compared offsets (equal, but no row), every other compared pair differs: the
    model shares nothing and the result must not change.  (A kernel that wrongly "shared" a -1 would take the other lane's centre
    fragment, which is an out-of-range gather = zeros, so that mistake would not show in the output: what this case pins down is that
    tables full of -1 beside live entries give the old form's bits, not that no request is made.)"""
    rng = np.random.default_rng(22)
    n, n_feat = 9005, 700
    t = (2 * rng.integers(0, n_feat // 2, (n, 9, 3)) + 1).astype(np.int32)     # odd rows at dx = -1 / +1, even rows at dx = 0: never equal
    t[:, :, 1] -= 1
    hole = rng.random((n, 9)) < 0.6
    t[:, :, 1] = np.where(hole, -1, t[:, :, 1])
    t[:-1, :, 2] = np.where(hole[1:], -1, t[:-1, :, 2])
    t[1:, :, 0] = np.where(hole[:-1], -1, t[1:, :, 0])
    return t.reshape(n, 27), n_feat, None


CASES = {"cloud": case_cloud, "cloud_static": case_cloud_static, "dense": case_dense, "isolated": case_isolated,
         "runs_small": case_runs_small, "runs_mid": case_runs_mid, "runs_large": case_runs_large,
         "equal_indices": case_equal_indices, "minus_one": case_minus_one}
_case_cache = {}


def get_case(name):
    if name not in _case_cache:
        _case_cache[name] = CASES[name]()
    return _case_cache[name]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    ops.indice_conv_set_variant(-1)
    yield ops
    ops.indice_conv_set_variant(-1)


def _forms_for(n_live):
    """The forms a launch of this many rows can be sent to (the four-wave form only through the automatic choice)."""
    return [f for f in FORMS if f != "64w4" or 8192 <= n_live < 40000]


def _expect_shares(name, nbr, n_live, rw):
    """What each case is there for, checked on the numpy model of the rule at this slab width."""
    left, right = share_model(nbr, n_live, rw)
    shared = int(left.sum() + right.sum())
    lane = np.arange(n_live) % rw
    if name in ("isolated", "minus_one"):
        assert shared == 0
    else:
        assert shared > 0
    if name == "dense":
        t = nbr[:n_live].reshape(n_live, 9, 3)
        inner = (lane > 0) & (lane < rw - 1) & (np.arange(n_live) + 1 < n_live)
        assert np.array_equal(left[inner], t[inner][:, :, 0] >= 0) and np.array_equal(right[inner], t[inner][:, :, 2] >= 0)
    if name.startswith("runs"):
        # centre line g = 4: a row with a +x neighbour but none at -x starts a run, the reverse ends one
        t = nbr[:n_live, 12:15]
        start, end = (t[:, 0] < 0) & (t[:, 2] >= 0), (t[:, 0] >= 0) & (t[:, 2] < 0)
        for ln in (0, rw - 1):
            assert (start & (lane == ln)).any() and (end & (lane == ln)).any(), (name, rw, ln)
        assert ((t[:, 2] >= 0) & (lane == rw - 1)).any()     # a run that crosses a slab (= wave or workgroup) boundary
    return shared


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CASES))
def test_xshare_bit_identical_and_vs_oracle(ops, name, dtype):
    nbr, n_feat, n_live = get_case(name)
    n = len(nbr)
    live = n if n_live is None else n_live
    tol = 2 ** -7 if dtype == torch.bfloat16 else 2 ** -10    # one rounding of the 16-bit store (tests/test_gpu_parity.py)
    full_slabs = set()
    for form in _forms_for(n):
        cin, cout, v_old, v_new, waves, fl_old, fl_new = FORMS[form]
        rw = slab_rows(live, waves)
        _expect_shares(name, nbr, live, rw)
        full_slabs.add(rw == 32)
        rng = np.random.default_rng(cin + len(name))
        f_t = dev(rng.standard_normal((n_feat, cin)).astype(np.float32), dtype)
        w_t = dev((rng.standard_normal((3, 3, 3, cin, cout)) / (5 * np.sqrt(cin))).astype(np.float32), dtype)
        scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        shift = rng.uniform(-0.2, 0.2, cout).astype(np.float32)
        packed, tbl = ops.pack_weight(w_t), dev(nbr)
        count = None if n_live is None else dev(np.array([n_live], np.int32))
        outs = {}
        for tag, variant, fl in (("old", v_old, fl_old), ("new", v_new, fl_new)):
            ops.indice_conv_set_variant(variant)
            assert ops.indice_conv_plan(cin, cout, 27, n, dtype) == 11
            plain = ops.indice_conv(f_t, w_t, tbl, n, packed=packed, num_out_dev=count)
            kname = ops.last_kernel_name()
            assert kname.startswith("k_conv_rows_buf<") and kname.endswith(f", {waves}, {3 if waves == 8 and cin == 64 else 2}, {fl}>"), kname
            fused = ops.indice_conv(f_t, w_t, tbl, n, packed=packed, scale=dev(scale), shift=dev(shift), relu=True, num_out_dev=count)
            outs[tag] = (plain[:live].cpu(), fused[:live].cpu())
        ops.indice_conv_set_variant(-1)
        for i, what in enumerate(("plain", "fused")):
            a, b = outs["old"][i], outs["new"][i]
            assert a.dtype == dtype and torch.equal(a.view(torch.int16), b.view(torch.int16)), \
                f"{form} {what}: {(a.view(torch.int16) != b.view(torch.int16)).sum().item()} elements differ"
        pairs, pair_num = pairs_of(nbr[:live], n_feat)
        f_np = np.zeros((pairs.shape[2], cin), np.float32)
        f_np[:n_feat] = f_t.float().cpu().numpy()
        ref = orc.indice_conv(f_np, w_t.float().cpu().numpy(), pairs, pair_num, live, acc64=True)
        ref_plain = torch.from_numpy(ref).to(dtype).float().numpy()
        ref_fused = torch.from_numpy(np.maximum(ref * scale + shift, 0)).to(dtype).float().numpy()
        np.testing.assert_allclose(outs["new"][0].float().numpy(), ref_plain, rtol=tol, atol=tol * np.abs(ref).max(), err_msg=form)
        np.testing.assert_allclose(outs["new"][1].float().numpy(), ref_fused, rtol=tol, atol=tol * np.abs(ref_fused).max(), err_msg=form)
    if name in ("runs_mid", "runs_large"):
        assert True in full_slabs                            # lanes 0 and 31 of a full slab were run ends somewhere


def test_share_rule_model_on_oracle_rulebooks(capsys):
    """CPU: the rule on the oracle's SubM rulebooks of one synthetic cloud, levels 0..3 in sorted numbering.  The pairing the rule finds
    by comparing row indices is compared with the pairing computed from CELL COORDINATES alone (rows i, i + 1 x-adjacent and the cell
    at that offset occupied): the two must be the same set, i.e. the rule never pairs two different rows and misses no shareable pair;
    x-adjacent consecutive rows really hold the indices the rule looks for (the offsets of a (dz, dy) line are k = 3g + dx); the
    shareable fraction of all pairs is printed per level."""
    from second_amd import synthetic as syn
    r = orc.points_to_voxel(syn.syn_kitti_cloud(0), syn.CAR_FHD_VOXEL, syn.CAR_FHD_RANGE, 5, 40000)
    idx = np.concatenate([np.zeros((r["voxel_num"], 1), np.int32), r["coordinates"]], 1)
    shape = [41, 1600, 1408]
    lines = []
    for level in range(4):
        idx = sort_cells(idx, shape)
        nbr = subm_table(idx, 1, shape)
        n = len(nbr)
        left, right = share_model(nbr, n, n)               # one endless slab: the count without slab edges
        t = nbr.reshape(n, 9, 3)
        adj = np.all(idx[1:, :3] == idx[:-1, :3], 1) & (idx[1:, 3] == idx[:-1, 3] + 1)
        # the pairing from coordinates alone: offset vector of every k from the cells the table joins (one constant vector per k, x
        # fastest), then "rows i, i + 1 are x-adjacent and the cell of row i at (dz, dy, +1) / of row i + 1 at (dz, dy, -1) is occupied"
        zyx = idx[:, 1:].astype(np.int64)
        dvec = np.zeros((27, 3), np.int64)
        for k in range(27):
            o = np.nonzero(nbr[:, k] >= 0)[0]
            d = zyx[nbr[o, k]] - zyx[o]
            assert len(o) and (d == d[0]).all() and (idx[nbr[o, k], 0] == idx[o, 0]).all(), k
            dvec[k] = d[0]
        step = dvec[1::3] - dvec[0::3]
        assert (step == dvec[2::3] - dvec[1::3]).all() and (step[:, :2] == 0).all() and (np.abs(step[:, 2]) == 1).all() and (step == step[0]).all()
        key = lambda c: (c[..., 0] * shape[1] + c[..., 1]) * shape[2] + c[..., 2]
        inside = lambda c: np.all((c >= 0) & (c < np.array(shape)), -1)
        occupied = np.sort(key(zyx))                         # (one frame: the batch index plays no part)
        has = lambda c: inside(c) & (occupied[np.minimum(np.searchsorted(occupied, key(c)), n - 1)] == key(c))
        assert int(step[0, 2]) == 1                           # offset 3g + 2 is the +x neighbour: row i + 1 of an x-run lies at (dz, dy, +1)
        geo_right = np.zeros((n, 9), bool)
        geo_left = np.zeros((n, 9), bool)
        geo_right[:-1] = adj[:, None] & has(zyx[:-1, None, :] + dvec[None, 2::3, :])
        geo_left[1:] = adj[:, None] & has(zyx[1:, None, :] + dvec[None, 0::3, :])
        assert np.array_equal(geo_right, right) and np.array_equal(geo_left, left), level
        # geometry: if rows i, i + 1 are x-adjacent, (dz, dy, +1) of i IS (dz, dy, 0) of i + 1, and the reverse
        assert np.array_equal(t[:-1, :, 2][adj], t[1:, :, 1][adj]) and np.array_equal(t[1:, :, 0][adj], t[:-1, :, 1][adj])
        assert np.array_equal(right[:-1][adj], t[1:, :, 1][adj] >= 0) and np.array_equal(left[1:][adj], t[:-1, :, 1][adj] >= 0)
        npairs = int((nbr >= 0).sum())
        shared = int(left.sum() + right.sum())
        assert 0 < shared < npairs
        lines.append(f"level {level}: {n} rows, {npairs} pairs, shareable {shared} = {100.0 * shared / npairs:.1f} %")
        if level < 3:
            idx, _, _, shape = orc.rulebook_conv(idx, 1, shape, 3, 2, 1)
            shape = [int(s) for s in shape]
    with capsys.disabled():
        print("\nx-share rule, syn_kitti_cloud(0):\n  " + "\n  ".join(lines))
