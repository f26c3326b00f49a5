"""fp64 reference, per-element error bounds, exact-integer operands and the case builder for the sparse convolution FORWARD
(sec_indice_conv_fwd, csrc/indice_conv.hip).  numpy on the CPU; shared by tests/test_indice_conv_fwd_host.py (which proves that the
bounds are sound and that they bite) and tests/test_gpu_indice_conv_fwd.py (which holds every shipped kernel form to them).

Everything is expressed on the gather table alone: nbr_out[o][k] = input row that output row o reads at kernel offset k, or -1.
    a[o] = sum_k feat[nbr_out[o][k]] @ W[k]          y = relu?(a * scale + shift)
The geometries and table builders are those of the backward suite (indice_conv_bwd_helpers), imported, not copied.
"""
import numpy as np
import torch

from indice_conv_bwd_helpers import (MODES, RAGGED_COUNTS, U24, U_STORE, geom_big, geom_dense, geom_empty_offset,  # noqa: F401
                                     geom_ragged, geom_runs, old_check, pad_dead, tables, worst)

GARBAGE = 0x3fffffff                                     # table entries behind the live rows of a static-capacity launch
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# name -> (scale?, shift?, relu?): the four of every case, and the two more of the epilogue-flag section
EPILOGUES = {"none": (False, False, False), "shift": (False, True, False), "scale": (True, False, False), "full": (True, True, True),
             "affine": (True, True, False), "relu": (False, False, True)}


# ------------------------------------------------------------------------------------------------ reference
def _w3(w):
    w = np.asarray(w)
    return w.reshape(-1, w.shape[-2], w.shape[-1])


def accumulate(feat, w, nbr_out):
    """(a, mag, terms) in float64: a[o] = sum_k feat[nbr_out[o][k]] @ W[k], mag the same sum over |feat| and |W| (the sum of the
    magnitudes of the products of that element), terms[o] = cin * live offsets of row o.  One matmul per block of rows:
    [feat[nbr[o][0]] | ... | feat[nbr[o][K-1]]] @ [W[0]; ...; W[K-1]], a zero row standing in for -1."""
    f64, w64 = np.asarray(feat, np.float64), _w3(w).astype(np.float64)
    K, cin, cout = w64.shape
    n_in, n_out = len(f64), len(nbr_out)
    assert nbr_out.shape == (n_out, K) and f64.shape[1:] == (cin,) and (n_out == 0 or nbr_out.max() < n_in)
    f0 = np.concatenate([f64, np.zeros((1, cin))])
    idx = np.where(nbr_out >= 0, nbr_out, n_in)
    wc = w64.reshape(K * cin, cout)
    wca = np.abs(wc)
    a, mag = np.zeros((n_out, cout)), np.zeros((n_out, cout))
    for r0 in range(0, n_out, 4096):
        g = f0[idx[r0:r0 + 4096]].reshape(-1, K * cin)
        a[r0:r0 + 4096] = g @ wc
        mag[r0:r0 + 4096] = np.abs(g, out=g) @ wca
    return a, mag, cin * (nbr_out >= 0).sum(1).astype(np.int64)


def epilogue(a, scale=None, shift=None, relu=False):
    y = np.array(a, np.float64)
    if scale is not None:
        y = y * np.asarray(scale, np.float64)
    if shift is not None:
        y = y + np.asarray(shift, np.float64)
    return np.maximum(y, 0.0) if relu else y


def reference(feat, w, nbr_out, scale=None, shift=None, relu=False):
    """(y, a, mag, terms) in float64 from the gather table alone; feat [n_in, cin], w [..., cin, cout], scale / shift [cout] are the
    ALREADY ROUNDED operands.  y = relu?(a * scale + shift)."""
    a, mag, terms = accumulate(feat, w, nbr_out)
    return epilogue(a, scale, shift, relu), a, mag, terms


# ------------------------------------------------------------------------------------------------ bounds
def bound(y, a, mag, terms, scale, shift, kind, store):
    """|out - y| per element, for a kernel that accumulates in fp32, applies epilogue_v and stores once.

    Accumulation.  The products of 16-bit operands are exact in fp32 (8 + 8 or 11 + 11 significant bits fit its 24).  Summing n
    numbers t_i in fp32 in ANY order (MFMA steps, four split-K partial sums reduced pairwise, fmaf chains) errs by at most
    gamma_(n-1) sum |t_i| (Higham, Accuracy and Stability, 4.2), gamma_(n-1) <= n 2^-24 to first order; n = terms[o] = cin x the live
    offsets of the row (offsets without a neighbour add exact zeros: no rounding), at most 27 * 128 = 3 456 here, so the + 2 covers the
    second-order term (n^2 2^-24 < 1).  fp32 operands through fmaf round once per term: the same n roundings.
        acc = (terms + 2) 2^-24 mag
    kind "fp32_exact": nothing more.  kind "fp32_split": operands carried as two bf16 halves, lo * lo dropped -- every product within
    3 * 2^-18 of exact; tests/test_gpu_parity.py::test_indice_conv_fp32 grants 4 * 2^-18 mag, and so does this.

    Epilogue (epilogue_v: __fmul_rn, then __fadd_rn; a flag that is off skips its operation, no rounding).  With c = a + e, |e| <= acc:
        p = fl(c s)   |p - a s|         <= |s| acc + 2^-24 |c s|     <= |s| acc (1 + 2^-24) + 2^-24 |a s|        =: e1
        q = fl(p + h) |q - (a s + h)|   <= e1 + 2^-24 |p + h|        <= e1 (1 + 2^-24) + 2^-24 |a s + h|         =: e2
    ReLU is 1-Lipschitz: |max(q, 0) - max(a s + h, 0)| <= e2.

    Store.  fp32: nothing.  16 bit: ONE round-to-nearest of v = y + e2: |rn(v) - y| <= u |v| + e2 <= u |y| + (1 + u) e2, u = 2^-8 (bf16)
    / 2^-11 (fp16); fp16 results below 2^-14 are subnormal, spaced 2^-24: half a spacing, 2^-25, as an absolute floor.
    The 1e-30 floor keeps 0 <= 0 from failing on a -0."""
    e = (np.asarray(terms, np.float64)[:, None] + 2) * U24 * mag
    if kind == "fp32_split":
        e = e + 4 * 2.0 ** -18 * mag
    else:
        assert kind == "fp32_exact" or kind in U_STORE, kind
    pre = np.asarray(a, np.float64)
    if scale is not None:
        s = np.abs(np.asarray(scale, np.float64))
        pre = pre * np.asarray(scale, np.float64)
        e = s * e * (1 + U24) + U24 * np.abs(pre)
    if shift is not None:
        pre = pre + np.asarray(shift, np.float64)
        e = e * (1 + U24) + U24 * np.abs(pre)
    if store == "fp32":
        return e + 1e-30
    u = U_STORE[store]
    return u * np.abs(y) + (1 + u) * e + (2.0 ** -25 if store == "fp16" else 1e-30)


def old_forward_check(x, ref, store):
    """The check of tests/test_gpu_parity.py::test_indice_conv_half_mfma on the fused 16-bit output: relative to the tensor's maximum."""
    return old_check(x, ref, 2.0 ** -7 if store == "bf16" else 2.0 ** -10)


# ------------------------------------------------------------------------------------------------ tables made by hand
def table_kvol(kvol, n_in, n_out, seed=0, holes=0.3):
    """A table of `kvol` offsets: column k is a random permutation of the input rows (cut or cycled to n_out) with `holes` of it -1."""
    rng = np.random.default_rng(1000 + 31 * kvol + seed)
    nbr = np.stack([np.resize(rng.permutation(n_in), n_out) for _ in range(kvol)], 1).astype(np.int32)
    nbr[rng.random(nbr.shape) < holes] = -1
    return dict(nbr_out=nbr, nbr_in=None, n_in=n_in, n_out=n_out, kvol=kvol, subm=False)


def with_lonely_rows(tb, rows):
    """The table with every offset of `rows` (output rows) set to -1: rows with no neighbour at all."""
    out = dict(tb)
    out["nbr_out"] = tb["nbr_out"].copy()
    out["nbr_out"][rows] = -1
    return out


def cut(tb, n_out):
    """The first n_out output rows of a table (a SubM table keeps all its input rows: the cut rows stay as inputs)."""
    assert 0 <= n_out <= tb["n_out"]
    out = dict(tb)
    out["nbr_out"], out["n_out"] = np.ascontiguousarray(tb["nbr_out"][:n_out]), n_out
    return out


# ------------------------------------------------------------------------------------------------ operands
def rnd(a, kind):
    """`a` rounded to the feature dtype of `kind` (bf16 / fp16: round to nearest even; fp32_*: float32), as float32."""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a).to(TORCH[kind]).float().numpy() if kind in ("bf16", "fp16") else a


def random_case(cin, cout, tb, seed, decay=8.0):
    """(feat, w [K, cin, cout], scale, shift) float32, unrounded.  Unit-variance rows times 2^(-decay * row / n_in): rows are numbered
    in cell order, so neighbours have similar magnitudes and the outputs span `decay` binades -- a check relative to the tensor's
    maximum is blind to the lower ones, the per-element bound is not.  scale: magnitudes in [0.5, 1.5], about half of them NEGATIVE;
    shift in [-0.2, 0.2] times the typical magnitude of the last rows."""
    rng = np.random.default_rng(seed)
    n_in = tb["n_in"]
    feat = rng.standard_normal((n_in, cin)) * 2.0 ** (-decay * np.arange(n_in) / max(n_in, 1))[:, None]
    w = rng.standard_normal((tb["kvol"], cin, cout)) / np.sqrt(tb["kvol"] * cin)
    scale = rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)
    scale[:2] = (-1.25, 0.75)                             # both signs whatever the draw
    shift = rng.uniform(-0.2, 0.2, cout) * 2.0 ** -decay
    return feat.astype(np.float32), w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32)


def exact_case(cin, cout, tb, seed=0):
    """Small integers, every sum exact in every dtype and in any order.  Each feature row has two non-zero channels (at random
    positions) with values in {-2, -1, 1, 2}; weights in {-1, 0, 1}, random: asymmetric in k and in (ci, co); scale in {-2, -1, 1, 2}
    per channel, shift an integer in -4 .. 4.  A row meets at most 27 offsets x 2 channels x |2| x |1|: mag <= 108, and
    |a scale + shift| <= 2 * 108 + 4 <= 256 -- both ASSERTED here on the fp64 reference.  Every partial sum in any order, the product
    with the scale and the sum with the shift are then integers of magnitude <= 256, which bf16 (8 bits), fp16, fp32 and the bf16 "hi"
    half of the split mode (lo = 0) all hold exactly.  Returns (feat, w, scale, shift, a, mag, terms)."""
    rng = np.random.default_rng(seed + 7 * cin + cout)
    n_in = tb["n_in"]
    feat = np.zeros((n_in, cin), np.float32)
    if n_in:
        first = rng.integers(0, cin, n_in)
        second = (first + rng.integers(1, cin, n_in)) % cin
        feat[np.arange(n_in), first] = rng.choice([-2.0, -1.0, 1.0, 2.0], n_in)
        feat[np.arange(n_in), second] = rng.choice([-2.0, -1.0, 1.0, 2.0], n_in)
    w = rng.integers(-1, 2, (tb["kvol"], cin, cout)).astype(np.float32)
    scale = rng.choice([-2.0, -1.0, 1.0, 2.0], cout).astype(np.float32)
    scale[:2] = (-2.0, 1.0)
    shift = rng.integers(-4, 5, cout).astype(np.float32)
    a, mag, terms = accumulate(feat, w, tb["nbr_out"])
    assert mag.max(initial=0) <= 108 and np.abs(a * scale + shift).max(initial=0) <= 256
    assert np.array_equal(a, np.round(a))
    return feat, w, scale, shift, a, mag, terms


# ------------------------------------------------------------------------------------------------ cases
KINDS = {"bf16": (torch.bfloat16, None), "fp16": (torch.float16, None),
         "fp32_exact": (torch.float32, "exact"), "fp32_split": (torch.float32, "split16")}


class Case:
    """One table with its rounded operands and fp64 accumulation.  `kind` is the FEATURE arithmetic (a key of KINDS); the reference
    of an epilogue and the bound of a (bound kind, store) are made on demand and kept.  Nothing here is modified after it is made."""

    def __init__(self, cin, cout, tb, kind, exact, seed=0):
        self.cin, self.cout, self.tb, self.kind, self.exact, self.dtype = cin, cout, tb, kind, exact, KINDS[kind][0]
        if exact:
            self.feat, self.w, self.scale, self.shift, self.a, self.mag, self.terms = exact_case(cin, cout, tb, seed)
            assert np.array_equal(rnd(self.feat, kind), self.feat) and np.array_equal(rnd(self.w, kind), self.w)
        else:
            feat, w, self.scale, self.shift = random_case(cin, cout, tb, 1000 * cin + cout + seed)
            self.feat, self.w = rnd(feat, kind), rnd(w, kind)
            self.a, self.mag, self.terms = accumulate(self.feat, self.w, tb["nbr_out"])
        self._y, self._dev = {}, None

    def vectors(self, epi):
        has_scale, has_shift, relu = EPILOGUES[epi]
        return (self.scale if has_scale else None), (self.shift if has_shift else None), relu

    def y(self, epi):
        if epi not in self._y:
            self._y[epi] = epilogue(self.a, *self.vectors(epi))
        return self._y[epi]

    def bound(self, epi, bound_kind, store):
        scale, shift, _ = self.vectors(epi)
        return bound(self.y(epi), self.a, self.mag, self.terms, scale, shift, bound_kind, store)

    def device(self):
        if self._dev is None:
            to = lambda a, dt=None: (torch.from_numpy(np.ascontiguousarray(a)).to(dt) if dt else torch.from_numpy(np.ascontiguousarray(a))).cuda()
            self._dev = dict(f=to(self.feat, self.dtype), w=to(self.w, self.dtype), nbr=to(self.tb["nbr_out"]),
                             scale=to(self.scale), shift=to(self.shift), packed={})
        return self._dev

    def run(self, ops, epi="none", packed=True, out_dtype=None, nbr=None, n_out=None, num_out_dev=None):
        """ops.indice_conv on the case.  packed=True: the image ops.pack_weight makes under the fp32 mode in force (None where the
        shape has none); packed=None: the kernels that read the plain weight.  nbr / n_out / num_out_dev: a static-capacity table."""
        d = self.device()
        pk = None
        if packed:
            mode = ops.get_fp32_mode()
            if mode not in d["packed"]:
                d["packed"][mode] = ops.pack_weight(d["w"])
            pk = d["packed"][mode]
        has_scale, has_shift, relu = EPILOGUES[epi]
        out = ops.indice_conv(d["f"], d["w"], d["nbr"] if nbr is None else nbr, self.tb["n_out"] if n_out is None else n_out, packed=pk,
                              scale=d["scale"] if has_scale else None, shift=d["shift"] if has_shift else None, relu=relu,
                              out_dtype=out_dtype, num_out_dev=num_out_dev)
        assert out.dtype == (out_dtype or self.dtype) and out.shape == (self.tb["n_out"] if n_out is None else n_out, self.cout)
        return out


_cases = {}


def case(cin, cout, tb_key, tb, kind, exact=False):
    """The Case of (shape, table, kind, exact), made once; `tb_key` names the table (any hashable), `tb` is a table or makes one."""
    key = (cin, cout, tb_key, kind, exact)
    if key not in _cases:
        _cases[key] = Case(cin, cout, tb() if callable(tb) else tb, kind, exact)
    return _cases[key]
