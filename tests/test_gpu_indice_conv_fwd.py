"""-m gpu: the sparse convolution FORWARD (sec_indice_conv_fwd, csrc/indice_conv.hip) element by element against the fp64 reference
and the per-element bounds of tests/indice_conv_fwd_helpers.py (derived there; tests/test_indice_conv_fwd_host.py shows on the CPU that
they are sound and that they catch a dropped contribution, mirrored offsets, a transposed weight, swapped channel halves, rotated
output channels, a misplaced ReLU or shift, a truncating store and a row computed past the live count).  Every call goes through
ops.indice_conv, operands are rounded to the dtype first and the reference sees the rounded values, no element is excluded, and
every test asserts the kernel it meant to reach: the 16-bit forms by ops.indice_conv_plan, the kernels that report themselves by
ops.last_kernel_name(), the fp32 kernels that do not by the name of a priming launch still standing.

  A  bounds (Gaussian operands, error / bound <= 1) and small integers (np.array_equal) on every shipped form
  B  the epilogue flags one by one
  C  edges, on integers: row counts around the 32-row tile / the 128-row workgroup / the 8-tile XCD order, static capacity with garbage
     behind the live rows, rows / tiles / workgroups without a neighbour, offsets without a pair, 1-5 offsets, strided sub-rulebooks,
     n_out = 0, n_in = 0, a one-hot identity at offsets 0, 13 and 26
  D  the row-count thresholds of the automatic choice: 8 192 and 40 000 rows
  E  the record: largest error / bound per kernel form
"""
import contextlib

import numpy as np
import pytest
import torch

import indice_conv_fwd_helpers as H

pytestmark = pytest.mark.gpu

TNAME = {"bf16": "__hip_bfloat16", "fp16": "__half"}
MFMA_SHAPES = [(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (16, 64), (64, 32), (32, 16), (128, 64)]
X3_SHAPES = [(16, 32), (32, 32), (32, 64), (64, 32), (64, 64)]
ROWS_SHAPES = [(16, 16, "subm"), (16, 32, "subm"), (32, 32, "s2"), (32, 64, "subm"), (64, 64, "s2"), (64, 64, "k3")]
RATIOS = {}                                                     # kernel form -> largest error / bound seen (test_report_ratios)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def npf(t):
    return t.float().cpu().numpy()


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


# ------------------------------------------------------------------------------------------------ tables and cases (made once)
_tables = {}


def table(name, mode="subm", keep_out=None, rows=None):
    """name: a geometry of the helpers ("runs", "empty_offset", "big"), a ragged row count, or ("kvol", k); rows: the first `rows` outputs."""
    key = (name, mode, keep_out, rows)
    if key not in _tables:
        if rows is not None:
            _tables[key] = H.cut(table(name, mode, keep_out)[1], rows)
        elif isinstance(name, tuple):
            _tables[key] = H.table_kvol(name[1], 200, 150)
        else:
            g = H.geom_ragged(name) if isinstance(name, int) else getattr(H, "geom_" + name)()
            _tables[key] = H.tables(g, mode, keep_out=keep_out)
    return key, _tables[key]


def case(cin, cout, kind, exact, name="runs", mode="subm", keep_out=None, rows=None):
    key, tb = table(name, mode, keep_out, rows)
    return H.case(cin, cout, key, tb, kind, exact)


def both(cin, cout, kind, **kw):
    return [case(cin, cout, kind, False, **kw), case(cin, cout, kind, True, **kw)]


# ------------------------------------------------------------------------------------------------ forms: what a launch must reach
PRIMED = "void sec::k_conv_rows_x3_f32<64, 32, 4>"


def prime(ops):
    """One tiny launch of a kernel that reports itself, so that a kernel that does NOT report leaves a known name standing."""
    with forced(ops, -1, "split16"):
        ops.indice_conv(dev(np.ones((1, 64), np.float32)), dev(np.ones((1, 64, 32), np.float32)), dev(np.zeros((1, 1), np.int32)), 1)
        assert ops.last_kernel_name() == PRIMED


class Form:
    """family: the key of RATIOS; kind: feature arithmetic; variant: the number forced; plan: what ops.indice_conv_plan must say;
    name: what the kernel reports ({ci}, {co}, {kv}, {w} = waves); silent: an fp32 kernel that does not report (PRIMED must stand)."""

    def __init__(self, family, kind, variant=-1, plan=None, name=None, packed=True, out_dtype=None, silent=False):
        self.family, self.kind, self.variant, self.plan, self.name = family, kind, variant, plan, name
        self.packed, self.out_dtype, self.silent = packed, out_dtype, silent
        self.store = "fp32" if (out_dtype == torch.float32 or kind.startswith("fp32")) else kind
        self.bound_kind = ("fp32_split" if "x3" in family else "fp32_exact") if kind.startswith("fp32") else kind
        self.key = family + (" -> fp32" if out_dtype == torch.float32 else "")


def launch(ops, form, c, epi="none", **kw):
    assert c.kind == form.kind
    n = kw.get("n_out", c.tb["n_out"])
    if form.silent:
        prime(ops)
    with forced(ops, form.variant, H.KINDS[form.kind][1]):
        if form.plan is not None:
            got = ops.indice_conv_plan(c.cin, c.cout, c.tb["kvol"], n, c.dtype, form.out_dtype, packed=bool(form.packed))
            assert got == form.plan, (form.family, got, form.plan)
        out = c.run(ops, epi, packed=form.packed, out_dtype=form.out_dtype, **kw)
        got = ops.last_kernel_name()
    if form.name:
        assert got == form.name.format(ci=c.cin, co=c.cout, kv=c.tb["kvol"], w=8 if n >= 40000 else 4), got
    elif form.plan == 11:
        assert got.startswith(f"k_conv_rows_buf<{TNAME[form.kind]}, {c.cin}, {c.cout}, {c.tb['kvol']}, "), got
    elif form.silent:
        assert got == PRIMED, got
    return out


def note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"error / bound  {key}: {ratio:.3f}")


def check(form, c, out, epi, rows=None, key=None):
    """Integers: bit for bit.  Gaussian operands: every element within its bound.  rows: only the first `rows` rows are compared."""
    got, y = npf(out)[:rows], c.y(epi)[:rows]
    if c.exact:
        bad = np.argwhere(got != y)
        assert not len(bad), (form.family, epi, "first wrong element", tuple(bad[0]), got[tuple(bad[0])], y[tuple(bad[0])], len(bad))
        assert np.array_equal(got, y)
    else:
        r = H.worst(got, y, c.bound(epi, form.bound_kind, form.store)[:rows])
        note(key or form.key, r)
        assert r <= 1.0, (form.family, epi, r)


def hold(ops, form, cases, epis=("none", "full")):
    outs = {}
    for c in cases:
        for epi in epis:
            outs[(c.exact, epi)] = launch(ops, form, c, epi)
            check(form, c, outs[(c.exact, epi)], epi)
    return outs


def f16(family, kind, variant, plan, **kw):
    return Form(family, kind, variant, plan, **kw)


def wave(kind, **kw):
    return f16("k_conv_mfma", kind, 0, 3, **kw)


def split_k(kind, cout, **kw):
    """Plan 4: the automatic choice for cout > 32, a documented number (30: split-K on 16-bit features) for the narrow shapes."""
    return f16("k_conv_mfma_sk", kind, -1 if cout > 32 else 30, 4, **kw)


def sliced(kind, cout, **kw):
    """Plan 5: the automatic choice for cout <= 32, variant 8 for the wide shapes (grid.y = cout / 32 > 1)."""
    return f16("k_conv_mfma_sks", kind, -1 if cout <= 32 else 8, 5, **kw)


def x3(w="{w}"):
    return Form("k_conv_rows_x3_f32 (%s waves)" % w, "fp32_split", name="void sec::k_conv_rows_x3_f32<{ci}, {co}, %s>" % w, packed=None)


def x3p(w="{w}"):
    return Form("k_conv_rows_x3p_f32 (%s waves)" % w, "fp32_split", name="void sec::k_conv_rows_x3p_f32<{ci}, {co}, %s, {kv}>" % w)


MFMA_F32 = "void sec::k_conv_mfma_f32<{ci}, {co}>"


# ------------------------------------------------------------------------------------------------ A: 16-bit features
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("cin,cout", MFMA_SHAPES)
def test_a_one_wave_per_tile(ops, cin, cout, mode, kind):
    """Variant 0, plan 3, k_conv_mfma: features first into the MFMA, the untransposed C/D store layout."""
    hold(ops, wave(kind), both(cin, cout, kind, mode=mode))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("cin,cout", MFMA_SHAPES)
def test_a_split_k(ops, cin, cout, mode, kind):
    hold(ops, split_k(kind, cout), both(cin, cout, kind, mode=mode))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("cin,cout", MFMA_SHAPES)
def test_a_sliced_split_k(ops, cin, cout, mode, kind):
    hold(ops, sliced(kind, cout), both(cin, cout, kind, mode=mode))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["subm", "s2"])
def test_a_first_layer(ops, mode, kind):
    """4 -> 16: plan 12 (k_conv_c4_mfma); under variant 29 the same call runs the VALU kernel k_conv_c4 (plan 2).  Both within
    their bounds, exact on integers, and within the sum of their bounds of each other."""
    cases = both(4, 16, kind, mode=mode)
    mfma, valu = f16("k_conv_c4_mfma", kind, -1, 12), f16("k_conv_c4", kind, 29, 2)
    a, b = hold(ops, mfma, cases), hold(ops, valu, cases)
    for epi in ("none", "full"):
        assert torch.equal(a[(True, epi)], b[(True, epi)])
        gap = np.abs(npf(a[(False, epi)]).astype(np.float64) - npf(b[(False, epi)]))
        assert (gap <= 2 * cases[0].bound(epi, kind, kind)).all()


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", [22, 82, 83])
@pytest.mark.parametrize("cin,cout,mode", ROWS_SHAPES)
def test_a_row_split_forced(ops, cin, cout, mode, variant, kind):
    """Plan 11 at small size: the per-element bound with the negative-scale epilogue, next to the bit-exact tests these forms have."""
    hold(ops, f16("k_conv_rows_buf", kind, variant, 11), both(cin, cout, kind, mode=mode))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,plan,family", [(5, 7, 0, "k_conv_generic"), (32, 32, 1, "k_conv_tiled (16-bit)"),
                                                  (64, 64, 1, "k_conv_tiled (16-bit)"), (4, 16, 2, "k_conv_c4")])
def test_a_plain_weight(ops, cin, cout, plan, family, kind):
    """packed=None: the kernels that read the weight itself."""
    hold(ops, f16(family, kind, -1, plan, packed=None), both(cin, cout, kind))


F32 = torch.float32


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,make", [
    (16, 16, lambda k, co: wave(k, out_dtype=F32)), (64, 128, lambda k, co: wave(k, out_dtype=F32)),
    (16, 32, lambda k, co: split_k(k, co, out_dtype=F32)), (64, 64, lambda k, co: split_k(k, co, out_dtype=F32)),
    (32, 32, lambda k, co: sliced(k, co, out_dtype=F32)), (64, 128, lambda k, co: sliced(k, co, out_dtype=F32)),
    # the row-split kernel stores the feature dtype only: forced, the plan must fall back to split-K
    (64, 64, lambda k, co: f16("k_conv_mfma_sk", k, 22, 4, out_dtype=F32)),
    # and so does the Cin = 4 MFMA kernel: the VALU first layer
    (4, 16, lambda k, co: f16("k_conv_c4", k, -1, 2, out_dtype=F32))],
    ids=["wave-16-16", "wave-64-128", "sk-16-32", "sk-64-64", "sks-32-32", "sks-64-128", "rows-falls-back-64-64", "c4-falls-back"])
def test_a_fp32_output_from_16_bit_input(ops, cin, cout, make, kind):
    hold(ops, make(kind, cout), both(cin, cout, kind))


# ------------------------------------------------------------------------------------------------ A: fp32 features
@pytest.mark.parametrize("mode", ["subm", "s2"])
@pytest.mark.parametrize("cin,cout", X3_SHAPES)
def test_a_fp32_split_on_the_fly(ops, cin, cout, mode):
    hold(ops, x3(4), both(cin, cout, "fp32_split", mode=mode))


@pytest.mark.parametrize("cin,cout,mode", [(16, 16, "subm"), (16, 32, "s2"), (32, 32, "subm"), (32, 64, "s2"), (64, 32, "subm"),
                                           (64, 64, "subm"), (64, 64, "k3")])
def test_a_fp32_split_prepacked(ops, cin, cout, mode):
    """The seven instantiations of k_conv_rows_x3p_f32; bit for bit the on-the-fly form where both exist; variant 32 ignores the image."""
    cases = both(cin, cout, "fp32_split", mode=mode)
    pre = hold(ops, x3p(4), cases)
    if (cin, cout) in X3_SHAPES:
        fly = hold(ops, x3(4), cases)
        ignoring = Form("k_conv_rows_x3_f32 (4 waves)", "fp32_split", 32, name=x3(4).name, packed=True)
        ign = hold(ops, ignoring, cases)
        for k in pre:
            assert torch.equal(pre[k], fly[k]) and torch.equal(ign[k], fly[k]), k


@pytest.mark.parametrize("cin,cout", X3_SHAPES)
def test_a_fp32_mfma(ops, cin, cout):
    """k_conv_mfma_f32: the `exact` mode, and variant 31 under the split mode (the packed image ignored)."""
    hold(ops, Form("k_conv_mfma_f32", "fp32_exact", name=MFMA_F32), both(cin, cout, "fp32_exact", mode="s2"))
    hold(ops, Form("k_conv_mfma_f32", "fp32_split", 31, name=MFMA_F32), both(cin, cout, "fp32_split"))


@pytest.mark.parametrize("cin,cout,variant,packed,family", [
    (32, 32, 30, True, "k_conv_tiled (fp32)"), (64, 64, 30, None, "k_conv_tiled (fp32)"), (16, 16, -1, None, "k_conv_tiled (fp32)"),
    (32, 16, -1, True, "k_conv_tiled (fp32)"), (4, 16, -1, True, "k_conv_c4 (fp32)"), (5, 7, -1, True, "k_conv_generic (fp32)")])
def test_a_fp32_valu(ops, cin, cout, variant, packed, family):
    """Variant 30 and the shapes without a matrix form: IEEE fp32 on the VALU under the default split mode."""
    hold(ops, Form(family, "fp32_split", variant, packed=packed, silent=True), both(cin, cout, "fp32_split"))


# ------------------------------------------------------------------------------------------------ B: the epilogue flags
def edge_forms():
    """One form per family for the sections B and C: (form, cin, cout)."""
    return [(wave("bf16"), 32, 64), (split_k("bf16", 64), 64, 64), (sliced("fp16", 32), 16, 32), (f16("k_conv_c4_mfma", "bf16", -1, 12), 4, 16),
            (x3(4), 32, 32), (x3p(4), 32, 64)]


@pytest.mark.parametrize("epi", ["scale", "shift", "affine", "relu"])
def test_b_epilogue_flags(ops, epi):
    """scale only, shift only, both without ReLU, ReLU alone: load_affine4 / epilogue_v carry a flag for each."""
    for form, cin, cout in edge_forms():
        hold(ops, form, both(cin, cout, form.kind), epis=(epi,))


# ------------------------------------------------------------------------------------------------ C: edges, on integers
SMALL_COUNTS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("count", SMALL_COUNTS + H.RAGGED_COUNTS)
def test_c_row_counts(ops, count):
    """The 32-row tile, the 128-row workgroup, and 1 / 8 / 9 tiles under the XCD order with the grid padded to a multiple of 8."""
    kw = dict(name=count) if count in H.RAGGED_COUNTS else dict(rows=count)
    for form, cin, cout in edge_forms():
        c = case(cin, cout, form.kind, True, **kw)
        assert c.tb["n_out"] == count
        check(form, c, launch(ops, form, c, "full"), "full")


CAPACITY_FORMS = [(f16("k_conv_rows_buf", "bf16", 22, 11), 64, 64), (f16("k_conv_c4", "bf16", 29, 2), 4, 16),
                  (f16("k_conv_generic", "bf16", -1, 0, packed=None), 5, 7), (f16("k_conv_tiled (16-bit)", "fp16", -1, 1, packed=None), 32, 32),
                  (Form("k_conv_mfma_f32", "fp32_exact", name=MFMA_F32), 32, 32)]


@pytest.mark.parametrize("live", [0, 1, 33, -1])
def test_c_static_capacity(ops, live):
    """The row count on the device is below the capacity and the table rows behind it hold 0x3fffffff: never read, never gathered.
    Only [:live] is compared (the rows behind are uninitialised memory of the output)."""
    for form, cin, cout in edge_forms() + CAPACITY_FORMS:
        c = case(cin, cout, form.kind, True)
        cap = c.tb["n_out"]
        m = cap - 1 if live < 0 else live
        assert 0 <= m < cap
        nbr = c.tb["nbr_out"].copy()
        nbr[m:] = H.GARBAGE
        out = launch(ops, form, c, "full", nbr=dev(nbr), num_out_dev=dev(np.array([m], np.int32)))
        assert out.shape[0] == cap
        check(form, c, out, "full", rows=m)


def test_c_rows_without_a_neighbour(ops):
    """Single rows, a whole 32-row tile and a whole 128-row workgroup with no neighbour at all: act(shift), exactly."""
    key, tb = table("runs")
    lonely = np.r_[5, 100, 1001, 64:96, 256:384]
    tl = H.with_lonely_rows(tb, lonely)
    for form, cin, cout in edge_forms() + CAPACITY_FORMS:
        c = H.case(cin, cout, (key, "lonely"), tl, form.kind, True)
        for epi in ("none", "shift", "full"):
            out = launch(ops, form, c, epi)
            check(form, c, out, epi)
            want = {"none": np.zeros(cout), "shift": c.shift, "full": np.maximum(c.shift, 0)}[epi]
            assert np.array_equal(npf(out)[lonely], np.broadcast_to(want, (len(lonely), cout))), (form.family, epi)


def test_c_offsets_without_a_pair(ops):
    for form, cin, cout in edge_forms() + CAPACITY_FORMS:
        c = case(cin, cout, form.kind, True, name="empty_offset")
        assert ((c.tb["nbr_out"] >= 0).sum(0) == 0).sum() == 18
        check(form, c, launch(ops, form, c, "full"), "full")


@pytest.mark.parametrize("kvol", [1, 2, 3, 5])
def test_c_few_offsets(ops, kvol):
    """Hand-built tables of 1-5 offsets: with 1-3 some of the four waves that split the offsets have none."""
    for form, cin, cout in [(split_k("bf16", 64), 64, 64), (split_k("fp16", 16), 32, 16), (sliced("bf16", 32), 32, 32),
                            (sliced("fp16", 128), 64, 128), (wave("bf16"), 16, 32)]:
        c = case(cin, cout, form.kind, True, name=("kvol", kvol))
        assert c.tb["kvol"] == kvol
        for epi in ("none", "full"):
            check(form, c, launch(ops, form, c, epi), epi)


@pytest.mark.parametrize("keep_out", [65, 63])
def test_c_strided_sub_rulebooks(ops, keep_out):
    """A stride-2 table cut to 65 / 63 outputs: several output rows read one input row, and input rows exist that no output reads."""
    for form, cin, cout in edge_forms() + CAPACITY_FORMS:
        c = case(cin, cout, form.kind, True, name=577, mode="s2", keep_out=keep_out)
        used = np.bincount(c.tb["nbr_out"][c.tb["nbr_out"] >= 0], minlength=c.tb["n_in"])
        assert c.tb["n_out"] == keep_out and used.max() > 1 and (used == 0).any()
        check(form, c, launch(ops, form, c, "full"), "full")


@pytest.mark.parametrize("kind", list(H.KINDS))
@pytest.mark.parametrize("cin,cout", [(64, 64), (16, 16), (4, 16), (5, 7)])
def test_c_no_output_rows(ops, cin, cout, kind):
    dtype = H.KINDS[kind][0]
    with forced(ops, -1, H.KINDS[kind][1]):
        w = dev(np.ones((27, cin, cout), np.float32), dtype)
        out = ops.indice_conv(dev(np.ones((130, cin), np.float32), dtype), w, dev(np.zeros((0, 27), np.int32)), 0, packed=ops.pack_weight(w),
                              scale=dev(np.ones(cout, np.float32)), shift=dev(np.ones(cout, np.float32)), relu=True)
    assert out.shape == (0, cout) and out.dtype == dtype


def test_c_no_input_rows(ops):
    """n_in = 0 and a table of -1: every row is act(shift)."""
    tb = dict(nbr_out=-np.ones((130, 27), np.int32), nbr_in=None, n_in=0, n_out=130, kvol=27, subm=False)
    for form, cin, cout in edge_forms() + CAPACITY_FORMS[1:]:           # (the row-split kernel needs features: the plan gives way)
        c = H.case(cin, cout, "no input rows", tb, form.kind, True)
        for epi in ("none", "full"):
            out = launch(ops, form, c, epi)
            want = np.zeros(cout) if epi == "none" else np.maximum(c.shift, 0)
            assert np.array_equal(npf(out), np.broadcast_to(want, (130, cout))), (form.family, epi)


@pytest.mark.parametrize("k", [0, 13, 26])
@pytest.mark.parametrize("cin,cout", [(16, 32), (64, 128)])
def test_c_one_hot_identity_at_an_offset(ops, cin, cout, k):
    """One-hot rows and an asymmetric W[k] at the first, the centre and the last offset (every other W[j] is all 3, and never used):
    catches transposed operand or output layouts, and the weights of another offset."""
    n = 70
    nbr = -np.ones((n, 27), np.int32)
    nbr[:, k] = np.arange(n)[::-1]
    feat = np.zeros((n, cin), np.float32)
    feat[np.arange(n), np.arange(n) % cin] = 1.0
    w = np.full((27, cin, cout), 3.0, np.float32)
    w[k] = np.arange(cin)[:, None] * 2 + np.arange(cout)[None, :] % 2
    want = w[k][np.arange(n)[::-1] % cin]
    f_t, w_t = dev(feat, torch.bfloat16), dev(w, torch.bfloat16)
    packed = ops.pack_weight(w_t)
    for variant, plan in ((0, 3), (30 if cout <= 32 else -1, 4), (-1 if cout <= 32 else 8, 5)):
        with forced(ops, variant):
            assert ops.indice_conv_plan(cin, cout, 27, n, torch.bfloat16) == plan
            out = ops.indice_conv(f_t, w_t, dev(nbr), n, packed=packed)
        assert np.array_equal(npf(out), want), (plan, k)


# ------------------------------------------------------------------------------------------------ D: the row-count thresholds
def test_d_8192_rows(ops):
    """Exactly kRowsMinSmall rows, bf16, automatic choice: 64 -> 64 runs the four-wave row-split form (kRows64W4), 8 191 rows do not."""
    form = f16("k_conv_rows_buf (8 192 rows)", "bf16", -1, 11)
    with forced(ops):
        assert ops.indice_conv_plan(64, 64, 27, 8191, torch.bfloat16) == 4
        assert ops.indice_conv_plan(32, 64, 27, 8192, torch.bfloat16) == 4
    for c in both(64, 64, "bf16", name="big", rows=8192):
        assert c.tb["n_out"] == 8192
        out = launch(ops, form, c, "full")
        assert ops.last_kernel_name() == "k_conv_rows_buf<__hip_bfloat16, 64, 64, 27, 3, 4, 2, 2689>", ops.last_kernel_name()
        check(form, c, out, "full")


@pytest.mark.parametrize("which", ["bf16", "x3", "x3p"])
def test_d_40000_rows(ops, which):
    """Exactly kRowsMin rows, automatic choice: the row-split kernel (bf16 32 -> 64), k_conv_rows_x3_f32<32, 64, 8> and
    k_conv_rows_x3p_f32<64, 64, 8, 27>; one row less keeps split-K / the four-wave forms."""
    form, cin, cout = {"bf16": (f16("k_conv_rows_buf (40 000 rows)", "bf16", -1, 11), 32, 64), "x3": (x3(), 32, 64), "x3p": (x3p(), 64, 64)}[which]
    for c in both(cin, cout, form.kind, name="big", rows=40000):
        assert c.tb["n_out"] == 40000
        out = launch(ops, form, c, "full")
        name = ops.last_kernel_name()
        assert name == {"bf16": "k_conv_rows_buf<__hip_bfloat16, 32, 64, 27, 4, 8, 2, 2051>", "x3": "void sec::k_conv_rows_x3_f32<32, 64, 8>",
                        "x3p": "void sec::k_conv_rows_x3p_f32<64, 64, 8, 27>"}[which], name
        check(form, c, out, "full", key=form.family.replace("{w}", "8"))
        if c.exact:                                              # 39 999 rows of the same table: the other side of the threshold
            below = f16("k_conv_mfma_sk", "bf16", -1, 4) if which == "bf16" else form
            out = launch(ops, below, c, "full", n_out=39999)         # (asserts plan 4 / the name of the four-wave form)
            check(below, c, out, "full", rows=39999)


# ------------------------------------------------------------------------------------------------ E: the record
EXPECTED_FORMS = ["k_conv_mfma", "k_conv_mfma_sk", "k_conv_mfma_sks", "k_conv_c4_mfma", "k_conv_c4", "k_conv_rows_buf", "k_conv_generic",
                  "k_conv_tiled (16-bit)", "k_conv_mfma -> fp32", "k_conv_mfma_sk -> fp32", "k_conv_mfma_sks -> fp32", "k_conv_c4 -> fp32",
                  "k_conv_rows_x3_f32 (4 waves)", "k_conv_rows_x3p_f32 (4 waves)", "k_conv_rows_x3_f32 (8 waves)", "k_conv_rows_x3p_f32 (8 waves)",
                  "k_conv_mfma_f32", "k_conv_tiled (fp32)", "k_conv_c4 (fp32)", "k_conv_generic (fp32)", "k_conv_rows_buf (8 192 rows)",
                  "k_conv_rows_buf (40 000 rows)"]


def test_report_ratios(capsys, request):
    """The record: largest error / bound per kernel form over this run (nothing above 1 can reach this line: the tests above assert).
    When no test was selected away (-k, a node id), every form named above must be in it."""
    with capsys.disabled():
        print("\nlargest error / bound per kernel form:")
        for fam in sorted(RATIOS):
            print(f"  {RATIOS[fam]:.3f}  {fam}")
    assert all(r <= 1.0 for r in RATIOS.values())
    if not request.config.option.keyword and not any("::" in a for a in request.config.args):
        assert not [f for f in EXPECTED_FORMS if f not in RATIOS]
