"""fp64 reference, per-element error bounds, geometries and exact-integer cases for the sparse convolution BACKWARD
(sec_indice_conv_bwd, csrc/indice_conv.hip).  numpy on the CPU; shared by tests/test_indice_conv_bwd_host.py (which proves that the
bounds bite) and tests/test_gpu_indice_conv_bwd.py (which holds the kernels to them).

Everything is expressed on the gather table alone: nbr_out[o][k] = input row that output row o reads at kernel offset k, or -1.
    dW[k]    = sum_o feat[nbr_out[o][k]]^T dout[o]
    dfeat[i] += dout[o] W[k]^T            for every pair (i = nbr_out[o][k], o)
"""
import numpy as np

from oracle import oracle as orc  # noqa: E402  (test infrastructure only)
from test_gpu_conv_rows_xshare import case_dense, sort_cells, subm_table  # noqa: F401  (re-exported to the tests)

U24 = 2.0 ** -24          # unit roundoff of fp32
U_STORE = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # unit roundoff of the 16-bit stores (8 / 11 significant bits, round to nearest)


# ------------------------------------------------------------------------------------------------ reference
def _w3(w):
    w = np.asarray(w)
    return w.reshape(-1, w.shape[-2], w.shape[-1])


def reference(feat, w, nbr_out, dout):
    """(dfeat64, dw64, mag_dfeat, mag_dw, terms_dw[k]) in float64 from the gather table alone.  feat [n_in, cin], w [..., cin, cout],
    nbr_out [n_out, K], dout [n_out, cout] are the ALREADY ROUNDED operands (float32 or float64).  mag_* are the same sums over
    |feat|, |w|, |dout| (the sum of the magnitudes of the products of that element), terms_dw[k] the number of pairs of offset k."""
    f64, d64, w64 = np.asarray(feat, np.float64), np.asarray(dout, np.float64), _w3(w).astype(np.float64)
    K, cin, cout = w64.shape
    assert nbr_out.shape == (len(d64), K) and f64.shape[1] == cin and d64.shape[1] == cout
    fa, da, wa = np.abs(f64), np.abs(d64), np.abs(w64)
    dfeat, mag_f = np.zeros_like(f64), np.zeros_like(f64)
    dw, mag_w = np.zeros_like(w64), np.zeros_like(w64)
    terms = np.zeros(K, np.int64)
    inv = np.full((len(f64), K), len(d64), np.int64)       # the table read from the input side; row n_out of d0 below is zero
    twice = False
    for k in range(K):
        o = np.nonzero(nbr_out[:, k] >= 0)[0]
        terms[k] = len(o)
        if not len(o):
            continue
        i = nbr_out[o, k]
        dw[k] = f64[i].T @ d64[o]
        mag_w[k] = fa[i].T @ da[o]
        twice = twice or np.bincount(i, minlength=len(f64)).max() > 1
        inv[i, k] = o
    if not twice:
        # a rulebook: an input row meets an offset once, so dfeat[i] = [dout[inv[i][0]] | ... | dout[inv[i][K-1]]] @ [W[0]^T; ...; W[K-1]^T]:
        # one matmul per block of rows (a matmul per offset is four times slower at 52 k rows)
        d0 = np.concatenate([d64, np.zeros((1, cout))])
        wc = np.ascontiguousarray(w64.transpose(0, 2, 1)).reshape(K * cout, cin)
        wca = np.abs(wc)
        for r0 in range(0, len(f64), 8192):
            g = d0[inv[r0:r0 + 8192]].reshape(-1, K * cout)
            dfeat[r0:r0 + 8192] = g @ wc
            mag_f[r0:r0 + 8192] = np.abs(g, out=g) @ wca
    else:                                                  # a hand-made table that names an input row twice at one offset
        for k in range(K):
            o = np.nonzero(nbr_out[:, k] >= 0)[0]
            np.add.at(dfeat, nbr_out[o, k], d64[o] @ w64[k].T)
            np.add.at(mag_f, nbr_out[o, k], da[o] @ wa[k].T)
    return dfeat, dw, mag_f, mag_w, terms


# ------------------------------------------------------------------------------------------------ bounds
def bound_dw(mag_dw, terms_dw):
    """|dW - ref| per element, fp32 accumulator, ANY summation order (MFMA steps, chunks, atomics across chunks).
    Summing n numbers t_i in fp32 in any order errs by at most gamma_(n-1) sum |t_i| (Higham, Accuracy and Stability, 4.2), and
    gamma_(n-1) <= n * 2^-24 while n^2 2^-24 <= 3, i.e. up to 7 000 pairs; the + 2 leaves room for the second-order term there.  For more
    pairs the kernels' own summation is shallower than n: a chunk of at most 1 024 rows is summed first, the chunk sums are combined
    by atomics, so no partial sum has seen more than chunk + chunks additions -- the first-order form in n holds a fortiori.
    The t_i themselves are exact for 16-bit operands (8 + 8 or 11 + 11 significant bits fit the 24 of fp32, the exponents its range);
    fp32 operands go through fmaf (k_conv_wgrad_tiled, k_conv_wgrad): one rounding per term, which is the same n roundings.
    `tiny` keeps an element whose every product is zero from failing on 0 <= 0 written with a -0."""
    return (np.asarray(terms_dw, np.float64)[:, None, None] + 2) * U24 * mag_dw + 1e-30


def bound_dfeat(ref, mag, kvol, cout, kind):
    """|dfeat - ref| per element; T = kvol * cout terms per element.  kind:
    "fp32_exact"  IEEE products and sums (v_mfma_f32_32x32x2_f32 / fmaf): gamma_T, as in bound_dw: (T + 2) 2^-24 mag.
    "fp32_split"  operands carried as two bf16 halves, lo * lo dropped: every product within 3 * 2^-18 of exact; the forward
                  test (test_indice_conv_fp32) grants 4 * 2^-18 mag on top of the accumulation, and so does this.
    "bf16"/"fp16" exact products, fp32 accumulation a = ref + e with |e| <= (T + 2) 2^-24 mag, then ONE round-to-nearest store
                  (the comment above pack2_16): |rn(a) - ref| <= u |a| + |e| <= u |ref| + (1 + u) |e|, u = 2^-8 / 2^-11.
                  fp16 results below 2^-14 are subnormal, spaced 2^-24: half a spacing, 2^-25, as an absolute floor."""
    t = kvol * cout
    acc = (t + 2) * U24 * mag
    if kind == "fp32_exact":
        return acc + 1e-30
    if kind == "fp32_split":
        return acc + 4 * 2.0 ** -18 * mag + 1e-30
    u = U_STORE[kind]
    return u * np.abs(ref) + (1 + u) * acc + (2.0 ** -25 if kind == "fp16" else 1e-30)


def bounds(ref, kvol, cout, kind):
    """(bound_dfeat, bound_dw) for the tuple `ref` = reference(...)."""
    dfeat, _, mag_f, mag_w, terms = ref
    return bound_dfeat(dfeat, mag_f, kvol, cout, kind), bound_dw(mag_w, terms)


def worst(x, ref, bound):
    """Largest error / bound over ALL elements (no element is excluded), nan-safe: a NaN or Inf in x counts as infinitely wrong."""
    err = np.abs(np.asarray(x, np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / bound).max()) if err.size else 0.0


def old_check(x, ref, tol):
    """The check of tests/test_gpu_parity.py::test_indice_conv_backward_shapes_and_dtypes: relative to the tensor's maximum."""
    return bool(np.allclose(x, ref, rtol=tol, atol=tol * np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------ geometries: (idx, shape, batch)
def _run_cells(rng, shape, batch, max_run, keep_line=1.0, n_target=None):
    """x-runs of random length 1..max_run with gaps of 1..3 cells on (z, y) lines (a line is kept with probability keep_line), x
    fastest: sorted cell order by construction.  n_target: stop (and cut) there."""
    cells, total = [], 0
    for b in range(batch):
        for z in range(shape[0]):
            for y in range(shape[1]):
                if keep_line < 1.0 and rng.random() >= keep_line:
                    continue
                x = int(rng.integers(0, 3))
                while True:
                    ln = int(rng.integers(1, max_run + 1))
                    if x + ln > shape[2]:
                        break
                    cells.append(np.stack([np.full(ln, b), np.full(ln, z), np.full(ln, y), np.arange(x, x + ln)], 1))
                    total += ln
                    x += ln + int(rng.integers(1, 4))
                if n_target is not None and total >= n_target:
                    return np.concatenate(cells).astype(np.int32)[:n_target]
    assert n_target is None, (total, n_target)
    return np.concatenate(cells).astype(np.int32)


def geom_runs():
    """About 1 100 rows in two frames: x-runs with gaps on a random half of the lines of 5 x 6 x 44 -- the x-share forms have rows to
    share, runs start and end inside slabs, and every one of the 27 offsets has pairs."""
    shape, batch = [5, 6, 44], 2
    idx = _run_cells(np.random.default_rng(11), shape, batch, 14, keep_line=0.6)
    return sort_cells(idx, shape), shape, batch


RAGGED_COUNTS = (63, 64, 65, 511, 512, 513, 577)
RAGGED_ISOLATED = 6


def geom_ragged(count):
    """Exactly `count` rows: runs in the planes z = 0..3 of 8 x 12 x 40 and RAGGED_ISOLATED cells in the plane z = 7, three cells apart.
    Those have no neighbour but themselves under a 3 x 3 x 3 SubM, and no pair AT ALL under the (3, 1, 1) / (2, 1, 1) conv without
    padding, whose three output planes end at z = 6.  (tables(keep_out=...) makes pair-less input rows for any strided mode.)"""
    shape = [8, 12, 40]
    assert count > RAGGED_ISOLATED
    body = _run_cells(np.random.default_rng(100 + count), [4, 12, 40], 1, 9, n_target=count - RAGGED_ISOLATED)
    iso = np.array([[0, 7, 3 * (j % 3) + 1, 3 * j + 1] for j in range(RAGGED_ISOLATED)], np.int32)
    idx = sort_cells(np.concatenate([body, iso]), shape)
    assert len(idx) == count
    return idx, shape, 1


def geom_empty_offset():
    """One z-plane (z = 1 of 3 x 20 x 40): the 18 offsets with dz != 0 have no pair at all."""
    shape = [3, 20, 40]
    idx = _run_cells(np.random.default_rng(12), [1, 20, 40], 1, 10)
    idx[:, 1] = 1
    return sort_cells(idx, shape), shape, 1


BIG_ROWS = 52300


def geom_big():
    """52 300 rows of x-runs (1..70 cells, gaps 1..3) on consecutive lines of 40 x 64 x 400: past the 40 000 rows from which the data
    gradient runs k_conv_rows_buf / the eight-wave fp32 kernel, and past the 52 225 from which a 1 024-row wgrad chunk survives."""
    shape = [40, 64, 400]
    idx = _run_cells(np.random.default_rng(13), shape, 1, 70, n_target=BIG_ROWS)
    return idx, shape, 1


def geom_dense():
    """The fully dense 8 x 24 x 48 block of the forward x-share tests: every interior dx = +-1 pair is shareable."""
    shape = [8, 24, 48]
    z, y, x = np.meshgrid(np.arange(8), np.arange(24), np.arange(48), indexing="ij")
    idx = np.stack([np.zeros(z.size, np.int64), z.ravel(), y.ravel(), x.ravel()], 1).astype(np.int32)
    return sort_cells(idx, shape), shape, 1


# ------------------------------------------------------------------------------------------------ rulebooks -> tables
def tables_from_pairs(pairs, pair_num, n_in, n_out):
    K = pairs.shape[0]
    nbr_out = -np.ones((n_out, K), np.int32)
    nbr_in = -np.ones((n_in, K), np.int32)
    for k in range(K):
        i, o = pairs[k, 0, :pair_num[k]], pairs[k, 1, :pair_num[k]]
        nbr_out[o, k] = i
        nbr_in[i, k] = o
    return nbr_out, nbr_in


MODES = {"subm": None, "s2": (3, 2, 1), "k3": ((3, 1, 1), (2, 1, 1), 0)}     # (ksize, stride, padding) of the strided modes


def tables(geom, mode, keep_out=None):
    """Gather tables of one geometry: dict(nbr_out [n_out, K], nbr_in [n_in, K], n_in, n_out, kvol, subm, pairs, pair_num).
    "subm": 3 x 3 x 3 SubM (oracle.rulebook_subm; nbr_in is there for the mirror identity, the kernels get None).
    "s2":   3 x 3 x 3 stride 2 padding 1;  "k3": (3, 1, 1) stride (2, 1, 1) no padding -- both in sorted output numbering
            (oracle.rulebook_conv_sorted), the numbering the served networks run.
    keep_out: keep only the first keep_out output rows of a strided table (a sub-rulebook: the pairs of the other outputs go, which
              leaves input rows without any pair)."""
    idx, shape, batch = geom
    n_in = len(idx)
    if mode == "subm":
        assert keep_out is None
        _, pairs, pair_num = orc.rulebook_subm(idx, batch, shape, 3)
        n_out = n_in
    else:
        ks, st, pd = MODES[mode]
        out_idx, pairs, pair_num, _ = orc.rulebook_conv_sorted(idx, batch, shape, ks, st, pd)
        n_out = len(out_idx)
    nbr_out, nbr_in = tables_from_pairs(pairs, pair_num, n_in, n_out)
    if keep_out is not None:
        assert 0 <= keep_out <= n_out
        n_out = keep_out
        nbr_out = np.ascontiguousarray(nbr_out[:n_out])
        nbr_in = np.where(nbr_in >= n_out, -1, nbr_in).astype(np.int32)
    return dict(nbr_out=nbr_out, nbr_in=nbr_in, n_in=n_in, n_out=n_out, kvol=nbr_out.shape[1], subm=mode == "subm",
                pairs=pairs, pair_num=pair_num)


def pad_dead(tb, dead):
    """Static capacity: `dead` rows appended to both tables, all -1 (a SubM table stays square)."""
    K = tb["kvol"]
    out = dict(tb)
    out["nbr_out"] = np.concatenate([tb["nbr_out"], -np.ones((dead, K), np.int32)])
    out["nbr_in"] = np.concatenate([tb["nbr_in"], -np.ones((dead, K), np.int32)])
    out["n_in"], out["n_out"] = tb["n_in"] + dead, tb["n_out"] + dead
    return out


# ------------------------------------------------------------------------------------------------ operands
def random_case(cin, cout, tb, seed):
    """(feat, w [K, cin, cout], dout) float32, unrounded: unit-variance rows, weights scaled as the forward tests scale them."""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((tb["n_in"], cin)).astype(np.float32)
    w = (rng.standard_normal((tb["kvol"], cin, cout)) / np.sqrt(tb["kvol"] * cin)).astype(np.float32)
    dout = rng.standard_normal((tb["n_out"], cout)).astype(np.float32)
    return feat, w, dout


def exact_case(cin, cout, tb, seed=0):
    """Small integers, every sum exact in every dtype and in any order: feat in {-3..3}, w in {-1, 0, 1} (random: asymmetric in k and
    in (ci, co)), dout rows with ONE non-zero channel of +-1.  Then an element of dfeat is a sum of at most kvol weights (one per
    offset): |dfeat| <= 27 and every partial sum is an integer below 2^8 (exact in bf16, fp16, fp32, and in the bf16 hi half of the split
    mode, whose lo half is zero); an element of dW[k] is a sum of at most pairs_k features: |dW| <= 3 pairs_k < 2^24.  Both conditions
    are asserted here on the fp64 reference.  Returns (feat, w, dout, dfeat_ref, dw_ref) with float32 operands and float64 results."""
    rng = np.random.default_rng(seed + 7 * cin + cout)
    feat = rng.integers(-3, 4, (tb["n_in"], cin)).astype(np.float32)
    w = rng.integers(-1, 2, (tb["kvol"], cin, cout)).astype(np.float32)
    dout = np.zeros((tb["n_out"], cout), np.float32)
    if tb["n_out"]:
        dout[np.arange(tb["n_out"]), rng.integers(0, cout, tb["n_out"])] = rng.choice([-1.0, 1.0], tb["n_out"])
    dfeat, dw, mag_f, mag_w, terms = reference(feat, w, tb["nbr_out"], dout)
    assert mag_f.max(initial=0) <= tb["kvol"] <= 27 and np.array_equal(dfeat, np.round(dfeat))
    assert (mag_w <= 3 * terms[:, None, None]).all() and 3 * terms.max(initial=0) < 2 ** 24 and np.array_equal(dw, np.round(dw))
    return feat, w, dout, dfeat, dw
