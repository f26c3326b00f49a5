"""-m gpu: the sparse convolution BACKWARD (sec_indice_conv_bwd / run_bwd, csrc/indice_conv.hip) element by element against the fp64
reference and the per-element bounds of tests/indice_conv_bwd_helpers.py (derived there; tests/test_indice_conv_bwd_host.py shows on the
CPU that they catch a dropped pair, a missing mirror, a transposed weight, a skipped chunk tail, a truncating store and swapped
channel halves).  Every call goes through ops.indice_conv_backward with the UNROUNDED fp32 weight gradient (dweight_dtype=float32: what
training takes), operands are rounded to the dtype first and the reference sees the rounded values, no element is excluded, and every
test asserts the kernel it meant to reach: the data gradient by ops.indice_conv_plan on the swapped shape and, where the kernel
reports itself, by ops.last_kernel_name(); the weight gradient by the name launch_wgrad_tiled reports, chunk included.

  A  bounds on the trained layer shapes x SubM / stride 2 / (3,1,1)-stride-(2,1,1) x bf16 / fp16 / fp32 exact / fp32 split, with the
     call packing its own data-gradient image and with the production arguments (packed_dgrad, dweight_out of pack_weight_train)
  B  small integers on the same grid: np.array_equal
  C  the data-gradient kernels of the training sizes forced at small size (variants 22, 82, 83, 30, 31) and the compacting wgrad (41)
  D  edges: row counts around the 64-row step and the 512-row chunk, offsets without pairs, n_out = 0, need_* flags, static capacity
     with NaN / Inf behind the live rows, a second backward through one autograd node
  E  52 300 rows: the automatic thresholds (k_conv_rows_buf, the eight-wave fp32 kernel, 1 024-row wgrad chunks)
"""
import contextlib

import numpy as np
import pytest
import torch

import indice_conv_bwd_helpers as H

pytestmark = pytest.mark.gpu

KINDS = {"bf16": (torch.bfloat16, None), "fp16": (torch.float16, None),
         "fp32_exact": (torch.float32, "exact"), "fp32_split": (torch.float32, "split16")}
TNAME = {"bf16": "__hip_bfloat16", "fp16": "__half", "fp32_exact": "float", "fp32_split": "float"}
LAYER_SHAPES = [(4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64)]
GRID = [(ci, co, m) for ci, co in LAYER_SHAPES for m in ("subm", "s2")] + [(64, 64, "k3")]
RATIOS = {}                                                     # kernel family -> largest error / bound seen (test_report_ratios)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    ops.indice_conv_set_variant(-1)
    mode = ops.get_fp32_mode()
    yield ops
    ops.indice_conv_set_variant(-1)
    ops.set_fp32_mode(mode)


@contextlib.contextmanager
def forced(ops, variant=-1, fp32=None):
    """A kernel variant and an fp32 arithmetic for the calls inside; both restored whatever happens."""
    prev = ops.get_fp32_mode()
    try:
        ops.indice_conv_set_variant(variant)
        if fp32 is not None:
            ops.set_fp32_mode(fp32)
        yield
    finally:
        ops.indice_conv_set_variant(-1)
        ops.set_fp32_mode(prev)


# ------------------------------------------------------------------------------------------------ what the dispatch is expected to do
MFMA_SHAPES = {(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (16, 64), (64, 32), (32, 16), (128, 64)}
X3_SHAPES = {(16, 32), (32, 32), (32, 64), (64, 32), (64, 64)}       # fp32 matrix-core kernels (split operands / fp32 MFMA)
WGRAD_TR = {(32, 32), (32, 64), (64, 32), (64, 64)}
WGRAD_MFMA = {(4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64)}
WGRAD_TILED = WGRAD_MFMA | {(64, 128), (128, 128)}


def buf_shape(ci, co, kvol):
    return (ci, co) == (64, 64) if kvol == 3 else kvol == 27 and (ci, co) in {(16, 16), (16, 32), (32, 32), (32, 64), (64, 64)}


def dgrad_plan(cin, cout, kvol, n_in, variant=-1):
    """Plan id of the 16-bit data gradient = the forward decision on the SWAPPED shape (include/second_hip.h): 0 none of the
    packed-weight kernels (k_conv_tiled / k_conv_dgrad), 4 split-K, 5 sliced split-K, 11 k_conv_rows_buf."""
    ci, co = cout, cin
    if (ci, co) not in MFMA_SHAPES:
        return 0
    auto = variant in (-1, 80, 81)
    if buf_shape(ci, co, kvol) and (variant in (22, 82, 83) or (auto and (n_in >= 40000 or ((ci, co) == (64, 64) and kvol == 27 and n_in >= 8192)))):
        return 11
    return 5 if auto and co <= 32 else 4


def rows_buf_name(kind, cin, cout, kvol, variant):
    """k_conv_rows_buf instantiation of a FORCED data gradient (or one of >= 40 000 rows) on the swapped shape."""
    ci, co = cout, cin
    xsh = variant != 82
    if kvol == 3:
        form = "3, 3, 8, 2, 3"
    elif (ci, co) == (64, 64):
        form = f"27, 3, 8, 3, {10881 if xsh else 2689}"
    elif (ci, co) == (32, 64):
        form = "27, 4, 8, 2, 2051"
    else:
        form = f"27, 6, 8, 2, {10307 if xsh and ci == 32 else 2115}"
    return f"k_conv_rows_buf<{TNAME[kind]}, {ci}, {co}, {form}>"


def f32_dgrad_name(kind, cin, cout, n_in, variant=-1):
    """Name the fp32 data gradient reports, or None for the kernels that do not report (k_conv_tiled, k_conv_dgrad)."""
    ci, co = cout, cin
    if (ci, co) not in X3_SHAPES or variant == 30:
        return None
    if kind == "fp32_split" and variant != 31:
        return f"void sec::k_conv_rows_x3_f32<{ci}, {co}, {8 if n_in >= 40000 else 4}>"
    return f"void sec::k_conv_mfma_f32<{ci}, {co}>"


def f32_bound_kind(kind, cin, cout, variant=-1):
    """The arithmetic that runs: split operands only in k_conv_rows_x3_f32; every other fp32 kernel multiplies and adds in IEEE fp32."""
    name = f32_dgrad_name(kind, cin, cout, 0, variant)
    return "fp32_split" if name and "x3_f32" in name else "fp32_exact"


def wgrad_name(kind, cin, cout, kvol, n_out, variant=-1):
    chunk = 8192
    while chunk > 512 and -(-n_out // chunk) * kvol < 1400:
        chunk >>= 1
    t = TNAME[kind]
    if kind in ("bf16", "fp16"):
        if (cin, cout) in WGRAD_TR and variant != 41:
            return f"k_conv_wgrad_tr<{t}, {cin}, {cout}> chunk={chunk}"
        if (cin, cout) in WGRAD_MFMA:
            return f"k_conv_wgrad_mfma<{t}, {cin}, {cout}> chunk={chunk}"
    if (cin, cout) in WGRAD_TILED:
        return f"k_conv_wgrad_tiled<{t}, {cin}, {cout}> chunk={chunk}"
    return f"k_conv_wgrad<{t}> chunk=512"


# ------------------------------------------------------------------------------------------------ cases (computed once, never modified)
_tables, _cases = {}, {}


def tables(geom, mode, keep_out=None):
    key = (geom, mode, keep_out)
    if key not in _tables:
        g = H.geom_ragged(geom) if isinstance(geom, int) else getattr(H, "geom_" + geom)()
        _tables[key] = H.tables(g, mode, keep_out=keep_out)
    return _tables[key]


def rnd(a, dtype):
    return torch.from_numpy(a).to(dtype).float().numpy()


class Case:
    def __init__(self, cin, cout, tb, kind, exact, seed=0):
        dtype = KINDS[kind][0]
        self.cin, self.cout, self.tb, self.kind, self.dtype = cin, cout, tb, kind, dtype
        if exact:
            self.feat, self.w, self.dout, dfeat, dw = H.exact_case(cin, cout, tb)
            assert all(np.array_equal(rnd(a, dtype), a) for a in (self.feat, self.w, self.dout))
            self.ref = (dfeat, dw)
        else:
            self.feat, self.w, self.dout = (rnd(a, dtype) for a in H.random_case(cin, cout, tb, 1000 * cin + cout + seed))
            self.ref = H.reference(self.feat, self.w, tb["nbr_out"], self.dout)
        self.f_t, self.w_t, self.d_t = dev(self.feat, dtype), dev(self.w, dtype), dev(self.dout, dtype)
        self.nbr_out_t = dev(tb["nbr_out"])
        self.nbr_in_t = None if tb["subm"] else dev(tb["nbr_in"])

    def run(self, ops, **kw):
        kw.setdefault("dweight_dtype", torch.float32)
        dfeat, dw = ops.indice_conv_backward(self.f_t, self.w_t, self.nbr_out_t, self.nbr_in_t, self.d_t, **kw)
        assert dfeat is None or (dfeat.dtype == self.dtype and dfeat.shape == self.f_t.shape)
        assert dw is None or (dw.dtype == torch.float32 and dw.shape == self.w_t.shape)
        return dfeat, dw


def case(cin, cout, geom, mode, kind, exact=False, keep_out=None):
    key = (cin, cout, geom, mode, kind, exact, keep_out)
    if key not in _cases:
        _cases[key] = Case(cin, cout, tables(geom, mode, keep_out), kind, exact)
    return _cases[key]


def npf(t):
    return t.float().cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"error / bound  {family}: {ratio:.3f}")


def check_dfeat(c, dfeat, family, bound_kind=None):
    b = H.bound_dfeat(c.ref[0], c.ref[2], c.tb["kvol"], c.cout, bound_kind or c.kind)
    r = H.worst(npf(dfeat), c.ref[0], b)
    note(family, r)
    assert r <= 1.0, (family, r)


def check_dw(c, dw, family):
    r = H.worst(npf(dw), c.ref[1], H.bound_dw(c.ref[3], c.ref[4]))
    note(family, r)
    assert r <= 1.0, (family, r)


def dgrad_family(c, plan, name):
    if name:
        return name.replace("void sec::", "").split("<")[0]
    if c.kind.startswith("fp32"):
        return "k_conv_tiled / k_conv_dgrad (fp32)"
    return {0: "k_conv_tiled / k_conv_dgrad (16-bit)", 4: "k_conv_mfma_sk", 5: "k_conv_mfma_sks"}[plan]


def paths(ops, c, variant=-1):
    """Run the weight gradient alone, then the data gradient alone, and assert both paths.  Returns (dfeat, dw, dgrad family, bound kind).
    The order matters: a data-gradient kernel that reports itself replaces the weight gradient's name, one that does not leaves it."""
    tb, n_in = c.tb, c.tb["n_in"]
    none, dw = c.run(ops, need_dfeat=False)
    assert none is None
    wname = ops.last_kernel_name()
    assert wname == wgrad_name(c.kind, c.cin, c.cout, tb["kvol"], tb["n_out"], variant), wname
    dfeat, none = c.run(ops, need_dweight=False)
    assert none is None
    got = ops.last_kernel_name()
    if c.kind.startswith("fp32"):
        plan, bkind = None, f32_bound_kind(c.kind, c.cin, c.cout, variant)
        want = f32_dgrad_name(c.kind, c.cin, c.cout, n_in, variant)
    else:
        plan, bkind = dgrad_plan(c.cin, c.cout, tb["kvol"], n_in, variant), c.kind
        assert ops.indice_conv_plan(c.cout, c.cin, tb["kvol"], n_in, c.dtype) == plan
        want = rows_buf_name(c.kind, c.cin, c.cout, tb["kvol"], variant) if plan == 11 else None
    assert got == (want or wname), (got, want)
    return dfeat, dw, dgrad_family(c, plan, want), bkind


# ------------------------------------------------------------------------------------------------ A, B: the trained layer shapes
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cin,cout,mode", GRID)
def test_a_bounds_on_trained_layer_shapes(ops, cin, cout, mode, kind):
    c = case(cin, cout, "runs", mode, kind)
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw, fam, bkind = paths(ops, c)
        check_dfeat(c, dfeat, fam, bkind)
        check_dw(c, dw, wgrad_name(kind, cin, cout, c.tb["kvol"], c.tb["n_out"]).split("<")[0])
        both_dfeat, both_dw = c.run(ops)                       # one call, both gradients: what the autograd function issues
        assert same_bits(both_dfeat, dfeat)
        check_dw(c, both_dw, "both gradients in one call")
        if kind in ("bf16", "fp16"):
            # the production arguments: the images of the forward's one pack launch (the fp32 master weight holds the rounded values)
            w16, _, pkt, dw0 = ops.pack_weight_train(dev(c.w), c.dtype, c.tb["subm"], zero_grad=True)
            assert same_bits(w16, c.w_t) and dw0.dtype == torch.float32 and not dw0.any()
            assert (pkt is not None) == (cout % 16 == 0)
            p_dfeat, p_dw = ops.indice_conv_backward(c.f_t, w16, c.nbr_out_t, c.nbr_in_t, c.d_t, dweight_dtype=torch.float32,
                                                     packed_dgrad=pkt, dweight_out=dw0)
            assert p_dw is dw0                                 # accumulated in place, no copy, no cast
            assert same_bits(p_dfeat, dfeat)
            check_dw(c, p_dw, "dweight_out of pack_weight_train")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cin,cout,mode", GRID)
def test_b_exact_integers_on_trained_layer_shapes(ops, cin, cout, mode, kind):
    c = case(cin, cout, "runs", mode, kind, exact=True)
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw, _, _ = paths(ops, c)
        assert np.array_equal(npf(dfeat), c.ref[0]) and np.array_equal(npf(dw), c.ref[1])
        if kind in ("bf16", "fp16"):
            w16, _, pkt, dw0 = ops.pack_weight_train(dev(c.w), c.dtype, c.tb["subm"], zero_grad=True)
            p_dfeat, p_dw = ops.indice_conv_backward(c.f_t, w16, c.nbr_out_t, c.nbr_in_t, c.d_t, dweight_dtype=torch.float32,
                                                     packed_dgrad=pkt, dweight_out=dw0)
            assert np.array_equal(npf(p_dfeat), c.ref[0]) and np.array_equal(npf(p_dw), c.ref[1])


# ------------------------------------------------------------------------------------------------ C: forced kernels
ROWS_CASES = [(ci, co, m) for ci, co in ((32, 32), (16, 16), (32, 16), (64, 64)) for m in ("subm", "s2")] + [(64, 64, "k3")]


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,mode", ROWS_CASES)
def test_c_rows_buf_data_gradient_forced(ops, cin, cout, mode, kind):
    """Variant 22: k_conv_rows_buf on the swapped shape (32 -> 16 forward = its 16 -> 32 form; the swapped 16 -> 32 forward has none)
    through the mirrored image (SubM) and the input-major table (stride 2, three offsets)."""
    assert buf_shape(cout, cin, 3 if mode == "k3" else 27)
    for exact in (False, True):
        c = case(cin, cout, "runs", mode, kind, exact=exact)
        with forced(ops, 22):
            assert dgrad_plan(cin, cout, c.tb["kvol"], c.tb["n_in"], 22) == 11
            dfeat, _, fam, _ = paths(ops, c, 22)
        assert fam == "k_conv_rows_buf"
        if exact:
            assert np.array_equal(npf(dfeat), c.ref[0])
        else:
            check_dfeat(c, dfeat, fam)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", ["runs", "dense"])
@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("ch", [32, 64])
def test_c_xshare_data_gradient_forced(ops, ch, mode, geom, kind):
    """Variants 82 / 83: the row-split kernel without / with the x-share loads, on a mirrored SubM image and on the input-major table of
    a stride-2 conv over sorted input rows: bit-identical to each other, within the bounds, exact on integers."""
    for exact in (False, True):
        c = case(ch, ch, geom, mode, kind, exact=exact)
        out = {}
        for variant in (82, 83):
            with forced(ops, variant):
                assert ops.indice_conv_plan(ch, ch, 27, c.tb["n_in"], c.dtype) == 11
                out[variant], _ = c.run(ops, need_dweight=False)
                name = ops.last_kernel_name()
            assert name == rows_buf_name(kind, ch, ch, 27, variant), name
            assert name.endswith({(32, 82): ", 2115>", (32, 83): ", 10307>", (64, 82): ", 2689>", (64, 83): ", 10881>"}[(ch, variant)])
        assert same_bits(out[82], out[83])
        if exact:
            assert np.array_equal(npf(out[83]), c.ref[0])
        else:
            check_dfeat(c, out[83], "k_conv_rows_buf")


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", [(32, 32), (32, 64), (64, 64)])
@pytest.mark.parametrize("mode", ["subm", "s2"])
def test_c_compacting_wgrad_forced(ops, cin, cout, mode, kind):
    """Variant 41: k_conv_wgrad_mfma on the shapes that k_conv_wgrad_tr serves by default."""
    for exact in (False, True):
        c = case(cin, cout, "runs", mode, kind, exact=exact)
        with forced(ops, 41):
            _, dw = c.run(ops, need_dfeat=False)
            name = ops.last_kernel_name()
        assert name == f"k_conv_wgrad_mfma<{TNAME[kind]}, {cin}, {cout}> chunk=512", name
        if exact:
            assert np.array_equal(npf(dw), c.ref[1])
        else:
            check_dw(c, dw, "k_conv_wgrad_mfma")


@pytest.mark.parametrize("variant", [30, 31])
@pytest.mark.parametrize("cin,cout,mode", [(32, 32, "subm"), (32, 32, "s2"), (64, 64, "subm"), (64, 64, "k3"), (32, 64, "s2"), (16, 32, "subm")])
def test_c_fp32_data_gradient_forced(ops, cin, cout, mode, variant):
    """Variants 30 / 31 under the DEFAULT split mode: the register-tiled VALU kernel and the fp32-MFMA kernel, both IEEE fp32."""
    for exact in (False, True):
        c = case(cin, cout, "runs", mode, "fp32_split", exact=exact)
        with forced(ops, variant, "split16"):
            dfeat, _, fam, bkind = paths(ops, c, variant)
        assert bkind == "fp32_exact"
        assert fam == ("k_conv_mfma_f32" if variant == 31 and (cout, cin) in X3_SHAPES else "k_conv_tiled / k_conv_dgrad (fp32)")
        if exact:
            assert np.array_equal(npf(dfeat), c.ref[0])
        else:
            check_dfeat(c, dfeat, fam, bkind)


# ------------------------------------------------------------------------------------------------ D: edges
@pytest.mark.parametrize("kind", ["bf16", "fp32_split"])
@pytest.mark.parametrize("ch", [64, 16])
@pytest.mark.parametrize("count", H.RAGGED_COUNTS)
def test_d_ragged_row_counts(ops, count, ch, kind):
    """n_out just around the 64-row step and the 512-row chunk of the weight gradient, with rows that have no neighbour but themselves."""
    c = case(ch, ch, count, "subm", kind)
    assert c.tb["n_out"] == count
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw, fam, bkind = paths(ops, c)
        check_dfeat(c, dfeat, fam, bkind)
        check_dw(c, dw, wgrad_name(kind, ch, ch, 27, count).split("<")[0])
        if kind == "bf16" and ch == 64:                        # the row-split data gradient on the same ragged tails
            with forced(ops, 22):
                d22, _ = c.run(ops, need_dweight=False)
                assert ops.last_kernel_name() == rows_buf_name(kind, ch, ch, 27, 22)
            check_dfeat(c, d22, "k_conv_rows_buf")


@pytest.mark.parametrize("kind", ["bf16", "fp32_split"])
@pytest.mark.parametrize("ch,mode,keep_out", [(64, "k3", None), (64, "s2", 65), (16, "s2", 65), (64, "s2", 63)])
def test_d_strided_rows_without_any_pair(ops, ch, mode, keep_out, kind):
    """Input rows no output reads: their dfeat is exactly zero, everything else within the bounds."""
    c = case(ch, ch, 577, mode, kind, keep_out=keep_out)
    lonely = (c.tb["nbr_in"] >= 0).sum(1) == 0
    assert lonely.any() and (keep_out is None or c.tb["n_out"] == keep_out)
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw, fam, bkind = paths(ops, c)
    assert not npf(dfeat)[lonely].any()
    check_dfeat(c, dfeat, fam, bkind)
    check_dw(c, dw, wgrad_name(kind, ch, ch, c.tb["kvol"], c.tb["n_out"]).split("<")[0])


@pytest.mark.parametrize("cin,cout,kind", [(32, 32, "bf16"), (16, 16, "fp16"), (32, 32, "fp32_split"), (5, 7, "fp32_exact"), (5, 7, "bf16")])
def test_d_offsets_without_pairs(ops, cin, cout, kind):
    c = case(cin, cout, "empty_offset", "subm", kind)
    empty = c.ref[4] == 0
    assert empty.sum() == 18
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw = c.run(ops)
    assert not npf(dw)[empty].any()
    check_dw(c, dw, wgrad_name(kind, cin, cout, 27, c.tb["n_out"]).split("<")[0])
    check_dfeat(c, dfeat, "empty offsets", f32_bound_kind(kind, cin, cout) if kind.startswith("fp32") else kind)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cin,cout,kvol", [(64, 64, 27), (16, 16, 27), (4, 16, 27), (5, 7, 27), (64, 64, 3)])
def test_d_no_output_rows(ops, cin, cout, kvol, kind):
    """A strided conv whose input rows produce no output (n_out = 0, n_in > 0; empty tensors carry null pointers): the call succeeds,
    dW is all zero, and so is dfeat.  run_bwd skips the packed-weight kernels and runs k_conv_tiled / the fp32 kernels / k_conv_dgrad
    on a table of -1, which never touch dout."""
    dtype, n_in = KINDS[kind][0], 130
    rng = np.random.default_rng(1)
    feat = dev(rng.standard_normal((n_in, cin)).astype(np.float32), dtype)
    w = dev(rng.standard_normal((kvol, cin, cout)).astype(np.float32), dtype)
    nbr_out, nbr_in = dev(np.zeros((0, kvol), np.int32)), dev(-np.ones((n_in, kvol), np.int32))
    dout = torch.empty((0, cout), dtype=dtype, device="cuda")
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw = ops.indice_conv_backward(feat, w, nbr_out, nbr_in, dout, dweight_dtype=torch.float32)
        assert dfeat.shape == feat.shape and dw.dtype == torch.float32 and not dfeat.any() and not dw.any()
        none, dw = ops.indice_conv_backward(feat, w, nbr_out, nbr_in, dout, need_dfeat=False, dweight_dtype=torch.float32)
        assert none is None and not dw.any()
        sentinel = torch.full(w.shape, 7.0, device="cuda")
        _, dw = ops.indice_conv_backward(feat, w, nbr_out, nbr_in, dout, need_dfeat=False, dweight_dtype=torch.float32,
                                         dweight_out=sentinel)
        assert dw is sentinel and bool((sentinel == 7.0).all())     # `dweight_out` is zeroed by its maker; nothing is added to it


@pytest.mark.parametrize("kind", ["bf16", "fp32_exact"])
def test_d_need_flags(ops, kind):
    c = case(32, 32, "runs", "s2", kind)
    with forced(ops, -1, KINDS[kind][1]):
        full_dfeat, full_dw = c.run(ops)
        sentinel = torch.full(c.w_t.shape, 7.0, device="cuda")
        dfeat, none = c.run(ops, need_dweight=False, dweight_out=sentinel)
        assert none is None and same_bits(dfeat, full_dfeat) and bool((sentinel == 7.0).all())       # not touched
        none, dw = c.run(ops, need_dfeat=False)
        assert none is None
        check_dw(c, dw, "need_dfeat=False")
        check_dw(c, full_dw, "need_dfeat=False")
        none, none2 = c.run(ops, need_dfeat=False, need_dweight=False)
        assert none is None and none2 is None


DEAD = 300


@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("cin,cout,kind,variant,wgrad", [
    (64, 64, "bf16", -1, "k_conv_wgrad_tr"), (32, 32, "fp16", -1, "k_conv_wgrad_tr"), (32, 64, "bf16", 41, "k_conv_wgrad_mfma"),
    (16, 16, "bf16", -1, "k_conv_wgrad_mfma"), (4, 16, "fp16", -1, "k_conv_wgrad_mfma"), (32, 32, "fp32_split", -1, "k_conv_wgrad_tiled"),
    (16, 16, "fp32_exact", -1, "k_conv_wgrad_tiled"), (5, 7, "fp32_exact", -1, "k_conv_wgrad"), (5, 7, "bf16", -1, "k_conv_wgrad"),
    (64, 64, "bf16", 22, "k_conv_wgrad_tr"), (32, 32, "bf16", 83, "k_conv_wgrad_tr")])
def test_d_static_capacity_dead_rows(ops, cin, cout, kind, variant, wgrad, mode):
    """Static capacities: 300 rows behind the live ones in feat, dout and both tables, table rows all -1, contents NaN and Inf.  A
    gradient row without a neighbour must not be READ (0 x NaN would poison the sum): dW within the bound, dfeat of the live rows bit
    for bit what the un-padded call gives, dfeat of the dead rows exactly zero."""
    c = case(cin, cout, "runs", mode, kind)
    tb, dtype = c.tb, c.dtype
    junk = np.tile(np.array([np.nan, np.inf, -np.inf, np.nan], np.float32), 16)
    pad = lambda a: dev(np.concatenate([a, np.resize(junk, (DEAD, a.shape[1]))]), dtype)
    f_p, d_p = pad(c.feat), pad(c.dout)
    tp = H.pad_dead(tb, DEAD)
    assert torch.isnan(f_p[tb["n_in"]:]).any() and torch.isinf(d_p[tb["n_out"]:]).any() and (tp["nbr_out"][tb["n_out"]:] == -1).all()
    with forced(ops, variant, KINDS[kind][1]):
        live_dfeat, _ = c.run(ops, need_dweight=False)
        dfeat, dw = ops.indice_conv_backward(f_p, c.w_t, dev(tp["nbr_out"]), None if tb["subm"] else dev(tp["nbr_in"]), d_p,
                                             dweight_dtype=torch.float32)
        none, dw_only = ops.indice_conv_backward(f_p, c.w_t, dev(tp["nbr_out"]), None if tb["subm"] else dev(tp["nbr_in"]), d_p,
                                                 need_dfeat=False, dweight_dtype=torch.float32)
        name = ops.last_kernel_name()
    assert name == wgrad_name(kind, cin, cout, 27, tp["n_out"], variant) and name.startswith(wgrad + "<"), name
    assert same_bits(dfeat[:tb["n_in"]], live_dfeat)
    assert not dfeat[tb["n_in"]:].float().abs().sum().item() and not torch.isnan(dfeat).any()
    check_dw(c, dw, wgrad)
    check_dw(c, dw_only, wgrad)


@pytest.mark.parametrize("mode", ["subm", "s2"])
def test_d_second_backward_through_one_autograd_node(ops, mode):
    """spconv.functional.indice_conv with an fp32 master weight and bf16 features: the first backward consumes the accumulator that the
    forward's pack launch zeroed; a second one (retain_graph) must zero its own -- its increment of weight.grad is one more dW, not
    dW on top of the first.  weight.grad is fp32 and unrounded: within the dW bound."""
    from spconv import functional as F
    from spconv.tensor import Rulebook
    c = case(32, 64, "runs", mode, "bf16")
    tb = c.tb
    rb = Rulebook(None, None, c.nbr_out_t, c.nbr_in_t, tb["n_out"], None, None, tb["subm"])
    feat = c.f_t.clone().requires_grad_(True)
    weight = dev(c.w).requires_grad_(True)                     # fp32 master weight holding the rounded values
    out = F.indice_conv(feat, weight, rb)
    assert out.dtype == torch.bfloat16 and out.shape == (tb["n_out"], 64)
    out.backward(c.d_t, retain_graph=True)
    g1, f1 = weight.grad.clone(), feat.grad.clone()
    assert g1.dtype == torch.float32
    check_dw(c, g1, "autograd weight.grad")
    check_dfeat(c, f1, "autograd features.grad")
    out.backward(c.d_t, retain_graph=True)
    total = weight.grad.double().cpu().numpy()
    inc = total - g1.double().cpu().numpy()                    # the second increment, up to the rounding of grad += dW
    bound = H.bound_dw(c.ref[3], c.ref[4]) + 2.0 ** -24 * np.abs(total)
    r = H.worst(inc, c.ref[1], bound)
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ E: the automatic thresholds
@pytest.mark.parametrize("kind", ["bf16", "fp32_split"])
def test_e_automatic_thresholds_at_52300_rows(ops, kind):
    """No variant forced: from 40 000 rows the data gradient runs k_conv_rows_buf (32 -> 32: the x-share form on the mirrored image) /
    the eight-wave split-operand fp32 kernel, and from 52 225 rows a 1 024-row weight-gradient chunk survives the halving."""
    c = case(32, 32, "big", "subm", kind)
    assert c.tb["n_out"] == 52300
    with forced(ops, -1, KINDS[kind][1]):
        dfeat, dw, fam, bkind = paths(ops, c)
        wname = wgrad_name(kind, 32, 32, 27, 52300)
    assert wname.endswith("chunk=1024") and wname.startswith("k_conv_wgrad_tr<" if kind == "bf16" else "k_conv_wgrad_tiled<")
    assert fam == ("k_conv_rows_buf" if kind == "bf16" else "k_conv_rows_x3_f32") and (kind == "bf16" or bkind == "fp32_split")
    check_dfeat(c, dfeat, fam + " (52 300 rows)", bkind)
    check_dw(c, dw, wname.split("<")[0] + " chunk=1024")


def test_report_ratios(capsys):
    """The record: largest error / bound per kernel family over this run (nothing above 1 can reach this line: the tests above assert)."""
    with capsys.disabled():
        print("\nlargest error / bound per kernel family:")
        for fam in sorted(RATIOS):
            print(f"  {RATIOS[fam]:.3f}  {fam}")
    assert all(r <= 1.0 for r in RATIOS.values())
