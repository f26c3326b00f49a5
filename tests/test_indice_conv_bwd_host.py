"""CPU: the fp64 reference, the geometries and the per-element bounds of tests/indice_conv_bwd_helpers.py, before the GPU tests rely on
them -- the reference against the oracle, the identity the SubM data gradient rests on, what every geometry promises, and that the
bounds BITE: a numpy model of a correct kernel passes them, six seeded wrong kernels do not."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc  # noqa: E402  (test infrastructure only)

import indice_conv_bwd_helpers as H

TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16}
_cache = {}


def geom(name):
    if name not in _cache:
        _cache[name] = (getattr(H, "geom_" + name)() if isinstance(name, str) else H.geom_ragged(name))
    return _cache[name]


def rnd(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH[kind]).float().numpy() if kind in TORCH else np.asarray(a, np.float32)


# ------------------------------------------------------------------------------------------------ reference == oracle
@pytest.mark.parametrize("mode", ["subm", "s2", "k3"])
@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 7)])
def test_reference_equals_oracle(mode, cin, cout):
    """The oracle accumulates in fp64 over the rulebook's pairs and returns the float32 of the sums: the gap to the table-built fp64
    reference is that one rounding (2^-24 relative; 2^-150 absolute for a result below the smallest fp32 normal)."""
    tb = H.tables(geom("runs"), mode)
    assert tb["kvol"] == (3 if mode == "k3" else 27)
    feat, w, dout = H.random_case(cin, cout, tb, 3)
    dfeat, dw, _, _, terms = H.reference(feat, w, tb["nbr_out"], dout)
    o_dfeat, o_dw = orc.indice_conv_backward(feat, w, tb["pairs"], tb["pair_num"], dout)
    assert np.array_equal(terms, tb["pair_num"])
    # (the oracle adds the pairs one by one in fp64 where the reference runs matmuls: 2^-53-sized differences before the rounding)
    assert np.all(np.abs(o_dfeat - dfeat) <= 2.0 ** -24 * np.abs(dfeat) * (1 + 1e-6) + 2.0 ** -150)
    assert np.all(np.abs(o_dw - dw) <= 2.0 ** -24 * np.abs(dw) * (1 + 1e-6) + 2.0 ** -150)


def test_reference_handles_a_table_that_names_a_row_twice():
    """Hand-made table (two output rows read the same input row at one offset): the indexed-add path equals the per-pair definition."""
    rng = np.random.default_rng(0)
    nbr = rng.integers(-1, 40, (90, 27)).astype(np.int32)
    feat, w, dout = rng.standard_normal((40, 8)), rng.standard_normal((27, 8, 6)), rng.standard_normal((90, 6))
    dfeat, dw, mag_f, mag_w, terms = H.reference(feat, w, nbr, dout)
    e_dfeat, e_dw = np.zeros((40, 8)), np.zeros((27, 8, 6))
    for o in range(90):
        for k in range(27):
            if nbr[o, k] >= 0:
                e_dw[k] += np.outer(feat[nbr[o, k]], dout[o])
                e_dfeat[nbr[o, k]] += w[k] @ dout[o]
    assert np.allclose(dfeat, e_dfeat, rtol=1e-12, atol=1e-12) and np.allclose(dw, e_dw, rtol=1e-12, atol=1e-12)
    assert np.array_equal(terms, (nbr >= 0).sum(0)) and (mag_f >= np.abs(dfeat) - 1e-12).all() and (mag_w >= np.abs(dw) - 1e-12).all()


# ------------------------------------------------------------------------------------------------ geometries
SUBM_GEOMS = ["runs", "empty_offset", "dense", "big"] + list(H.RAGGED_COUNTS)


@pytest.mark.parametrize("name", SUBM_GEOMS)
def test_subm_mirror_identity(name):
    """nbr_in[j][k] == nbr_out[j][K-1-k]: the SubM data gradient reads nbr_out through mirrored offsets instead of an input-major table."""
    idx, shape, batch = geom(name)
    lin = ((idx[:, 0].astype(np.int64) * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
    assert (np.diff(lin) > 0).all()                           # sorted cell order, x fastest, no cell twice
    tb = H.tables((idx, shape, batch), "subm")
    assert np.array_equal(tb["nbr_in"], tb["nbr_out"][:, ::-1])
    assert np.array_equal(tb["nbr_out"][:, 13], np.arange(len(idx)))


def test_geometries_meet_their_properties():
    idx, shape, batch = geom("runs")
    assert 1000 <= len(idx) <= 1250 and batch == 2 and set(idx[:, 0]) == {0, 1}
    tb = H.tables(geom("runs"), "subm")
    assert (tb["pair_num"] > 0).all()
    t = tb["nbr_out"][:, 12:15]                               # the centre line: runs that start, end and go on (something to share)
    assert ((t[:, 0] < 0) & (t[:, 2] >= 0)).any() and ((t[:, 0] >= 0) & (t[:, 2] < 0)).any() and ((t[:, 0] >= 0) & (t[:, 2] >= 0)).any()
    assert len(idx) % 64 not in (0, 63) and len(idx) > 1024 and len(idx) % 512 % 64 != 0       # a ragged last chunk with a ragged last step
    for mode, kvol in (("s2", 27), ("k3", 3)):
        ts = H.tables(geom("runs"), mode)
        assert ts["kvol"] == kvol and (ts["pair_num"] > 0).all() and 0 < ts["n_out"] < ts["n_in"]
        lo = ts["pairs"][:, 1]                                # sorted output numbering: per offset, pairs ascend in the input row
        assert all((np.diff(ts["pairs"][k, 0, :ts["pair_num"][k]]) > 0).all() for k in range(kvol)) and lo.max() == ts["n_out"] - 1
    for count in H.RAGGED_COUNTS:
        g = geom(count)
        assert len(g[0]) == count
        tb = H.tables(g, "subm")
        assert ((tb["nbr_out"] >= 0).sum(1) == 1).sum() == H.RAGGED_ISOLATED                # no neighbour but themselves
        t3 = H.tables(g, "k3")
        assert ((t3["nbr_in"] >= 0).sum(1) == 0).sum() == H.RAGGED_ISOLATED                 # strided: input rows with no pair at all
        t2 = H.tables(g, "s2", keep_out=min(64, count // 4))
        assert t2["n_out"] == min(64, count // 4) and ((t2["nbr_in"] >= 0).sum(1) == 0).any() and t2["nbr_in"].max() == t2["n_out"] - 1
    tb = H.tables(geom("empty_offset"), "subm")
    assert (tb["pair_num"][:9] == 0).all() and (tb["pair_num"][18:] == 0).all() and (tb["pair_num"][9:18] > 0).all()
    idx, _, _ = geom("big")
    assert len(idx) == H.BIG_ROWS == 52300
    # the thresholds the case is sized for (launch_wgrad_tiled: the chunk halves from 8192 while ceil(n / chunk) * 27 < 1400)
    chunk = 8192
    while chunk > 512 and -(-len(idx) // chunk) * 27 < 1400:
        chunk >>= 1
    assert chunk == 1024 and len(idx) >= 40000
    d = H.tables(geom("dense"), "subm")
    assert np.array_equal(d["nbr_out"], H.case_dense()[0])


@pytest.mark.parametrize("mode", ["subm", "s2", "k3"])
def test_exact_case_is_exact(mode):
    tb = H.tables(geom("runs"), mode)
    feat, w, dout, dfeat, dw = H.exact_case(32, 32, tb)
    assert set(np.unique(feat)) == set(range(-3, 4)) and set(np.unique(w)) == {-1, 0, 1}
    assert ((dout != 0).sum(1) == 1).all() and set(np.unique(dout)) == {-1, 0, 1}
    assert np.abs(dfeat).max() <= tb["kvol"] and dfeat.any() and dw.any()
    # asymmetric: neither the offset mirror nor the transpose leaves the weights unchanged
    assert not np.array_equal(w, w[::-1]) and not np.array_equal(w, w.transpose(0, 2, 1))
    for kind in ("bf16", "fp16"):                             # representable: the 16-bit store changes nothing
        assert np.array_equal(rnd(dfeat, kind), dfeat) and np.array_equal(rnd(feat, kind), feat)


# ------------------------------------------------------------------------------------------------ the bounds bite
FAULTS = {"a": "one pair dropped in the weakest offset", "b": "SubM data gradient without the offset mirror",
          "c": "W[k] used untransposed in the data gradient (square shape)", "d": "the last n_out % 64 rows of a chunk skipped",
          "e": "dfeat truncated instead of rounded to nearest", "f": "two 16-channel halves of dW swapped"}


OLD_PASSES = "e"             # which of FAULTS the old max-relative check lets through (test_bounds_bite)


def _fma(acc, prod64):
    """fp32 accumulator + exact (fp64) product, one rounding: fmaf."""
    return (acc.astype(np.float64) + prod64).astype(np.float32)


def _store(x, kind, truncate):
    x = np.asarray(x, np.float32)
    if not truncate:
        return rnd(x, kind)
    if kind == "bf16":
        return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def model_kernel(feat, w, tb, dout, kind, seed, fault=None):
    """numpy model of sec_indice_conv_bwd on 16-bit operands (float32 arrays holding the rounded values).
    dW: one fp32 accumulator per (offset, 512-row chunk) over that chunk's pairs in a shuffled order, chunk sums combined in a shuffled
    order (the atomics).  dfeat: SubM reads nbr_out with the weights of the mirrored offset, a strided conv its input-major table; the
    kvol * cout terms of an element are added in a shuffled order in fp32, then ONE round-to-nearest store.  `fault`: a key of FAULTS."""
    rng = np.random.default_rng(seed)
    K, cin, cout = w.shape
    nbr_out, nbr_in = tb["nbr_out"].copy(), tb["nbr_in"].copy()
    f64, d64, w64 = feat.astype(np.float64), dout.astype(np.float64), w.astype(np.float64)
    if fault == "a":
        cnt = (nbr_out >= 0).sum(0)
        k = int(np.argmin(np.where(cnt > 0, cnt, cnt.max() + 1)))
        o = int(np.nonzero(nbr_out[:, k] >= 0)[0][0])
        nbr_in[nbr_out[o, k], k] = -1
        nbr_out[o, k] = -1
    dw = np.zeros((K, cin, cout), np.float32)
    for k in range(K):
        sums = []
        for o0 in range(0, len(nbr_out), 512):
            o1 = min(o0 + 512, len(nbr_out))
            if fault == "d":
                o1 = o0 + (o1 - o0) // 64 * 64
            o = o0 + np.nonzero(nbr_out[o0:o1, k] >= 0)[0]
            rng.shuffle(o)
            acc = np.zeros((cin, cout), np.float32)
            for oo in o:
                acc = _fma(acc, np.outer(f64[nbr_out[oo, k]], d64[oo]))
            sums.append(acc)
        for j in rng.permutation(len(sums)):
            dw[k] = dw[k] + sums[j]
    if fault == "f":
        dw[:, :32] = np.concatenate([dw[:, 16:32], dw[:, :16]], 1)
    tbl = nbr_out if tb["subm"] else nbr_in
    acc = np.zeros((len(tbl), cin), np.float32)
    d0 = np.concatenate([d64, np.zeros((1, cout))])          # row -1: no neighbour, exact zeros
    for t in rng.permutation(K * cout):
        k, co = divmod(int(t), cout)
        wk = w64[K - 1 - k if tb["subm"] and fault != "b" else k]
        col = wk[co, :] if fault == "c" else wk[:, co]
        acc = _fma(acc, d0[tbl[:, k], co][:, None] * col[None, :])
    return _store(acc, kind, fault == "e"), dw


@pytest.fixture(scope="module")
def bite_case():
    tb = H.tables(geom("runs"), "subm")
    out = {}
    for kind in ("bf16", "fp16"):
        feat, w, dout = (rnd(a, kind) for a in H.random_case(32, 32, tb, 5))
        out[kind] = (feat, w, dout, H.reference(feat, w, tb["nbr_out"], dout))
    out["exact"] = H.exact_case(32, 32, tb)
    return tb, out


def _ratios(tb, ops, kind, fault, seed=1):
    feat, w, dout, ref = ops
    dfeat, dw = model_kernel(feat, w, tb, dout, kind, seed, fault)
    b_dfeat, b_dw = H.bounds(ref, tb["kvol"], w.shape[2], kind)
    tol = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -9}[kind]
    old = H.old_check(dfeat, ref[0], tol) and H.old_check(rnd(dw, kind), ref[1], tol)      # the old test sees dW in the weight's dtype
    return H.worst(dfeat, ref[0], b_dfeat), H.worst(dw, ref[1], b_dw), old


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_bounds_pass_a_correct_kernel(bite_case, kind):
    tb, cases = bite_case
    r_dfeat, r_dw, old = _ratios(tb, cases[kind], kind, None)
    assert r_dfeat <= 1.0 and r_dw <= 1.0 and old, (r_dfeat, r_dw, old)
    feat, w, dout, e_dfeat, e_dw = cases["exact"]
    dfeat, dw = model_kernel(feat, w, tb, dout, kind, 2)
    assert np.array_equal(dfeat, e_dfeat) and np.array_equal(dw, e_dw)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_bounds_bite(bite_case, fault, capsys):
    """Each wrong kernel of FAULTS, modelled in numpy on `runs` (1 143 rows, SubM, 32 -> 32, bf16), misses the per-element bounds, and
    the exact-integer case differs by np.array_equal -- with ONE exception that arithmetic forces: (e), truncation, cannot show on
    integers that the 16-bit format represents exactly (truncation and rounding agree on them); only the bounds on random operands
    catch it, so that is what is asserted for (e).

    What the OLD check lets through (tests/test_gpu_parity.py::test_indice_conv_backward_shapes_and_dtypes: rtol = atol / max|ref| =
    2^-7 for bf16, dW seen after rounding to bf16), measured here on the same operands (error / new bound in brackets):
        (e) truncated store             PASSES the old check           (dfeat 1.8)
        (a) one dropped pair            fails it                       (dfeat 330, dW 1 500)
        (d) 55 skipped rows of 1 143    fails it                       (dW 5 000)
        (b) no offset mirror, (c) untransposed W[k], (f) swapped channel halves: fail it (dfeat 6 000 / 7 600, dW 24 000)
    (a) and (d) were expected to slip through the old check as well.  With unit-variance rows they do not: one product is ~1 against
    an allowance of 2^-7 max|dW| ~ 1, and it changes dfeat by ~0.2 against 2^-7 max|dfeat| ~ 0.035.  A dropped pair whose product is
    a few times smaller than typical does slip through; the per-element bounds catch it by a factor of hundreds either way.
    """
    tb, cases = bite_case
    r_dfeat, r_dw, old = _ratios(tb, cases["bf16"], "bf16", fault)
    with capsys.disabled():
        print(f"\n  ({fault}) {FAULTS[fault]}: dfeat error / bound {r_dfeat:.3g}, dW error / bound {r_dw:.3g}, old check {'passes' if old else 'fails'}")
    assert max(r_dfeat, r_dw) > 1.0, (fault, r_dfeat, r_dw)
    assert {"a": r_dw > 1 and r_dfeat > 1, "b": r_dfeat > 1 and r_dw <= 1, "c": r_dfeat > 1 and r_dw <= 1, "d": r_dw > 1 and r_dfeat <= 1,
            "e": r_dfeat > 1 and r_dw <= 1, "f": r_dw > 1 and r_dfeat <= 1}[fault], (fault, r_dfeat, r_dw)
    assert old == (fault in OLD_PASSES), (fault, old)
    feat, w, dout, e_dfeat, e_dw = cases["exact"]
    dfeat, dw = model_kernel(feat, w, tb, dout, "bf16", 2, fault)
    same = np.array_equal(dfeat, e_dfeat) and np.array_equal(dw, e_dw)
    assert same == (fault == "e"), fault
