"""fp64 reference, per-element error bound, exact-integer cases and the case table of the 16-bit dense conv2d FORWARD (csrc/dense.hip,
csrc/dense_patch.hpp: k_conv2d_halo_reg, k_conv2d_patch, k_conv1x1_nhwc, k_conv2d_nhwc_dma, k_conv1x1_chain and the fused tail of
k_conv2d_halo_reg<..., TAIL>).  numpy on the CPU; shared by tests/test_dense_fwd_ref_host.py (which proves on the CPU that the
reference is the convolution and that the checks bite) and tests/test_gpu_dense_fwd_fp64.py (which holds every instantiation to them).
Activations are [B, H, W, C] arrays (channels-last memory as the kernels see it), already rounded to the 16-bit type; weights are
torch's [Cout, Cin, k, k]."""
import numpy as np

from dense_train_ref_helpers import U_STORE, gamma_n, round16, store_floor, worst  # noqa: F401  (the same constants and `worst`)

KINDS = ("bf16", "fp16")
TYPE_NAME = {"bf16": "__hip_bfloat16", "fp16": "__half"}


def out_size(n, ksize, stride, pad):
    return (n + 2 * pad - ksize) // stride + 1


# ------------------------------------------------------------------------------------------------ reference
def _ringed(a, pad):
    if pad == 0:
        return a
    b, h, w, c = a.shape
    p = np.zeros((b, h + 2 * pad, w + 2 * pad, c), a.dtype)
    p[:, pad:pad + h, pad:pad + w] = a
    return p


def _tap(xp, ky, kx, stride, ho, wo):
    """The input pixel of tap (ky, kx) of every output pixel: a strided slice of the zero-ringed tensor, as [B ho wo, C] rows."""
    v = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
    return np.ascontiguousarray(v).reshape(-1, xp.shape[3])


def conv2d_terms(h, w, cin, ksize, stride, pad):
    """[ho, wo] int64: the number of taps of an output pixel that fall inside the image, times cin -- the products of that element that
    are not an exact zero from the padding."""
    ho, wo = out_size(h, ksize, stride, pad), out_size(w, ksize, stride, pad)
    ones = _ringed(np.ones((1, h, w, 1), np.int64), pad)
    t = np.zeros((ho * wo, 1), np.int64)
    for ky in range(ksize):
        for kx in range(ksize):
            t += _tap(ones, ky, kx, stride, ho, wo)
    return t.reshape(ho, wo) * cin


def conv2d_reference(x, w16, bias, ksize, stride, pad, dtype=np.float64, want_mag=True):
    """y[b][oy][ox][co] = sum_{ky, kx, ci} x[b][oy s - p + ky][ox s - p + kx][ci] w16[co][ci][ky][kx] (+ bias[co]), pixels outside the
    image zero; rows / columns that no full window reaches are dropped (torch's floor rule).  x [B,H,W,Cin] and w16 [Cout,Cin,k,k] are
    the operands ALREADY ROUNDED to 16 bit.  One GEMM per tap over a strided slice of the zero-ringed tensor.
    -> (ref [B,ho,wo,Cout], mag, terms): mag the same sum over magnitudes, |bias| included (None without want_mag); terms [ho,wo] the
    per-element count of conv2d_terms.  dtype = np.float32 is for the exact-integer cases only: every partial sum an integer below
    2^24, so float32 sgemm is exact in any order."""
    b, h, w, cin = x.shape
    cout = w16.shape[0]
    assert w16.shape == (cout, cin, ksize, ksize)
    ho, wo = out_size(h, ksize, stride, pad), out_size(w, ksize, stride, pad)
    assert ho > 0 and wo > 0
    xp = _ringed(np.asarray(x, dtype), pad)
    wt = np.asarray(w16, dtype)
    ref = np.zeros((b * ho * wo, cout), dtype)
    mag = np.zeros_like(ref) if want_mag else None
    for ky in range(ksize):
        for kx in range(ksize):
            a = _tap(xp, ky, kx, stride, ho, wo)
            wk = np.ascontiguousarray(wt[:, :, ky, kx].T)
            ref += a @ wk
            if want_mag:
                mag += np.abs(a) @ np.abs(wk)
    if bias is not None:
        ref += np.asarray(bias, dtype)
        if want_mag:
            mag += np.abs(np.asarray(bias, dtype))
    shape = (b, ho, wo, cout)
    return ref.reshape(shape), (mag.reshape(shape) if want_mag else None), conv2d_terms(h, w, cin, ksize, stride, pad)


# ------------------------------------------------------------------------------------------------ bounds
def bound_fwd(ref, mag, terms, kind, bias):
    """dense_train_ref_helpers.bound_conv with the PER-ELEMENT term count: |y - ref| <= u16 |ref| + (1 + u16) gamma_T mag + floor,
    T = terms (+ 1 with a bias), u16 = 2^-8 (bf16) / 2^-11 (fp16), floor the fp16 subnormal half-spacing.  Derivation there: exact
    products (8 + 8 / 11 + 11 bits fit fp32's 24), fp32 accumulation in whatever order the MFMA loop has -- Higham's gamma_T covers
    every order -- one fp32 bias addition, ONE round-to-nearest store.  ReLU is 1-Lipschitz: the same bound holds against relu(ref).
    ref, mag [B,ho,wo,C]; terms [ho,wo]."""
    u = U_STORE[kind]
    t = np.asarray(terms, np.float64)[None, :, :, None] + (1 if bias else 0)
    return u * np.abs(ref) + (1 + u) * gamma_n(t) * mag + store_floor(kind)


def bound_next_stage(ref2, mag2, terms2, w2, b1, kind, bias):
    """The bound of a 1x1 stage that reads a ROUNDED intermediate m with |m - ref1| <= b1 per element (ref1 the float64 reference of
    the stage before, after its activation): the stage's exact sum moves by at most sum_c |w2[co][c]| b1[c], its fp32 accumulation
    errs by gamma_T2 mag2 (mag2 from ref1), then one store:  u16 |ref2| + (1 + u16) (gamma_T2 mag2 + sum |w2| b1) + floor.
    (The accumulation error on the moved part, gamma_T2 sum |w2| b1 <= 8e-6 of that term, is second order and not carried.)
    ref2, mag2 [..., Cout]; w2 [Cout, Cmid] (float64 of the 16-bit weights); b1 [..., Cmid]; terms2 a scalar."""
    u = U_STORE[kind]
    moved = b1.reshape(-1, b1.shape[-1]) @ np.abs(np.asarray(w2, np.float64)).T
    t = terms2 + (1 if bias else 0)
    return u * np.abs(ref2) + (1 + u) * (gamma_n(t) * mag2 + moved.reshape(ref2.shape)) + store_floor(kind)


def stage1x1(a, w, bias):
    """A 1x1 stage in float64 on [..., Cin] values: (ref, mag)."""
    w = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1])
    flat = np.asarray(a, np.float64).reshape(-1, w.shape[1])
    ref, mag = flat @ w.T, np.abs(flat) @ np.abs(w).T
    if bias is not None:
        ref, mag = ref + np.asarray(bias, np.float64), mag + np.abs(np.asarray(bias, np.float64))
    shape = a.shape[:-1] + (w.shape[0],)
    return ref.reshape(shape), mag.reshape(shape)


def chain_reference(x, w1, b1, relu1, w2, b2, kind, x_ref=None, x_bound=None):
    """y = W2 act(W1 x + b1) + b2, the two 1x1 convs of k_conv1x1_chain and of the fused tail of k_conv2d_halo_reg<..., TAIL>, in
    float64 with the propagated bound.  -> (ref2, bound2).
    WHERE THE KERNELS ROUND (read in csrc/dense.hip): k_conv1x1_chain and the TAIL epilogue accumulate stage 1 in fp32 MFMA
    accumulators, add bias1 in fp32, apply the ReLU in fp32 and then pack2<T> the intermediate to the 16-bit type into the LDS tile
    (`put_mid`) -- ONE round-to-nearest of act(W1 x + b1), after the activation; stage 2 reads those 16-bit values, accumulates in
    fp32, adds bias2 and rounds once at the store (store_tile_t).  In the TAIL form the 3x3 conv before them is rounded the same
    way: put_tile packs act(conv + bias) to 16 bit into the LDS tile the first 1x1 GEMM reads -- three stages, two rounded
    intermediates.  x_ref / x_bound: x is itself such a rounded intermediate with float64 reference x_ref and bound x_bound (the
    tail); without them x is exact input."""
    w1m = np.asarray(w1, np.float64).reshape(w1.shape[0], w1.shape[1])
    w2m = np.asarray(w2, np.float64).reshape(w2.shape[0], w2.shape[1])
    src = x if x_ref is None else x_ref
    r1, m1 = stage1x1(src, w1m, b1)
    if x_ref is None:
        bd1 = (U_STORE[kind] * np.abs(r1) + (1 + U_STORE[kind]) * gamma_n(w1m.shape[1] + (b1 is not None)) * m1 + store_floor(kind))
    else:
        bd1 = bound_next_stage(r1, m1, w1m.shape[1], w1m, x_bound, kind, b1 is not None)
    if relu1:
        r1 = np.maximum(r1, 0.0)                      # 1-Lipschitz: bd1 holds against relu(r1)
    r2, m2 = stage1x1(r1, w2m, b2)
    return r2, bound_next_stage(r2, m2, w2m.shape[1], w2m, bd1, kind, b2 is not None)


# ------------------------------------------------------------------------------------------------ the two existing checks
def old_check_max(y, ref, kind):
    """tests/test_gpu_parity.py::test_conv2d_nhwc_mfma_vs_torch: assert_allclose with rtol = atol / max|ref| = 2^-7 (bf16) / 2^-9 (fp16)."""
    tol = 2.0 ** -7 if kind == "bf16" else 2.0 ** -9
    ref32 = np.asarray(ref, np.float32).astype(np.float64)
    return bool(np.allclose(np.asarray(y, np.float64), ref32, rtol=tol, atol=tol * np.abs(ref32).max(initial=0)))


def old_check_per_element(y, ref_nobias, mag_nobias, cin, ksize, kind):
    """conv2d_per_element_bound of tests/test_gpu_parity.py (and tests/test_gpu_conv2d_plan.py) against an fp32 reference: it runs
    WITHOUT bias and ReLU, so y here is the output of that launch; u |ref| + 2 (cin k^2 + 2) 2^-24 mag + 1e-30."""
    ref32 = np.asarray(ref_nobias, np.float32).astype(np.float64)
    bound = U_STORE[kind] * np.abs(ref32) + 2 * (cin * ksize * ksize + 2) * 2.0 ** -24 * mag_nobias + 1e-30
    return bool((np.abs(np.asarray(y, np.float64) - ref32) <= bound).all())


# ------------------------------------------------------------------------------------------------ exact-integer cases
def integer_case(cin, cout, k, shape, seed, stride=1, pad=None, density=1.0):
    """x in [-4, 4] [B,H,W,cin], w in [-2, 2] [cout,cin,k,k], integer bias in [-8, 8] (int8 / int8 / int16), and `pre` = the integer
    convolution + bias as float32 [B,ho,wo,cout].  Every product is an integer of magnitude <= 8 and every partial sum one of
    magnitude <= 8 cin k^2 + 8 <= 18 440 < 2^24: exact in fp32 in ANY order (and within fp16's range), so a kernel must equal `pre`
    (after the ReLU where asked) rounded ONCE to the output type, bit for bit.  The bias of a channel is the value in [-8, 8] that
    makes most of its pre-activations exactly 0 (ties and channels without a candidate: seeded at random), so that the ReLU edge
    -- exact zeros and negative values -- is part of every case; both shares are asserted non-zero.  density < 1: that share of the
    input values is kept, the others are 0 (the tail cases: sums small enough to stay exact through two more 16-bit roundings)."""
    b, h, w = shape
    pad = (k // 2 if stride < k else 0) if pad is None else pad
    assert 8 * cin * k * k + 8 < 2 ** 24
    rng = np.random.default_rng(seed + 1009 * cin + 31 * cout + 7 * k + 3 * stride + 131 * h + w + b)
    x = rng.integers(-4, 5, (b, h, w, cin), dtype=np.int8)
    if density < 1.0:
        x = (x * (rng.random(x.shape) < density)).astype(np.int8)
    wt = rng.integers(-2, 3, (cout, cin, k, k), dtype=np.int8)
    bias = rng.integers(-8, 9, cout).astype(np.int16)
    return (x, wt) + integer_bias(x, wt, bias, k, stride, pad)


def integer_bias(x, wt, bias, k, stride, pad):
    """(bias, pre) of integer_case for the image x: `bias` where no value in [-8, 8] makes a zero in the channel."""
    cout, cin = wt.shape[:2]
    s, _, _ = conv2d_reference(x, wt, None, k, stride, pad, dtype=np.float32, want_mag=False)
    flat = s.reshape(-1, cout)
    cand = np.arange(-8, 9)
    hits = np.stack([(flat == -v).sum(0) for v in cand])                        # [17, cout]: zeros a bias of v would make
    best = hits.argmax(0)
    bias = np.where(hits.max(0) > 0, cand[best], bias).astype(np.int16)
    pre = s + bias.astype(np.float32)
    assert np.array_equal(pre, np.round(pre)) and np.abs(pre).max() <= 8 * cin * k * k + 8
    assert (pre == 0).any() and (pre < 0).any(), "the ReLU edge must be part of the case"
    return bias, pre


def rounded_bits(pre, relu, kind):
    """relu?(pre) rounded ONCE to the 16-bit type, as its int16 bit pattern (what test_gpu_conv2d_mfma16._rounded / _bits compare)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.maximum(pre, 0) if relu else pre, np.float32))
    return t.to(torch.bfloat16 if kind == "bf16" else torch.float16).view(torch.int16).numpy()


def bits_of(a, kind):
    """float32 array of 16-bit values -> int16 bit patterns."""
    return rounded_bits(a, False, kind)


def integer_chain_case(seed, cmid=128, cout2=64):
    """Integer 1x1 pair for the tail and the chain, kept EXACT through both roundings: W1 picks ONE input channel per mid channel with weight +-1 (a signed selection: mid = +-x[c] + b1, |b1| <= 2), so the
    16-bit intermediate is exact whenever x is; W2 has four entries of +-1 per head channel.  The caller asserts on the reference
    that the intermediate is representable in bf16 and the result is of magnitude <= 256."""
    rng = np.random.default_rng(seed)
    w1 = np.zeros((cmid, 128), np.int8)
    w1[np.arange(cmid), rng.permutation(128)[:cmid]] = rng.choice([-1, 1], cmid)
    b1 = rng.integers(-2, 3, cmid).astype(np.int16)
    w2 = np.zeros((cout2, cmid), np.int8)
    for co in range(cout2):
        w2[co, rng.choice(cmid, 4, replace=False)] = rng.choice([-1, 1], 4)
    b2 = rng.integers(-8, 9, cout2).astype(np.int16)
    return w1.reshape(cmid, 128, 1, 1), b1, w2.reshape(cout2, cmid, 1, 1), b2


def gaussian_case(cin, cout, k, shape, kind, seed=0):
    """x ~ N(0, 1) [B,H,W,cin], w ~ N(0, 1 / (cin k^2)), bias ~ N(0, 1) (fp32, as the kernels take it), x and w rounded to `kind`."""
    b, h, w = shape
    rng = np.random.default_rng(seed + 1000 * b + 10 * h + w + cin + 3 * cout + k)
    x = round16(rng.standard_normal((b, h, w, cin), np.float32), kind)
    wt = round16(rng.standard_normal((cout, cin, k, k), np.float32) / np.float32((cin * k * k) ** 0.5), kind)
    bias = rng.standard_normal(cout).astype(np.float32)
    return x, wt, bias


# ------------------------------------------------------------------------------------------------ case table
HALO128 = "k_conv2d_halo_reg<%s, 128, 8, 3, false>"
# call form, cin, cout, ksize, stride, pad, (batch, h, w), the instantiation (%s = element type), Gaussian run too (False: the
# threshold cases, integers only -- their maps are as large as the limit they land on needs)
FORM_CASES = [
    # ---- k_conv2d_halo_reg
    ("plain", 128, 128, 3, 1, 1, (2, 9, 17), HALO128, True),                                          # four tiles, ragged bottom and right
    ("plain", 128, 256, 3, 1, 1, (2, 1, 1), HALO128, True),                                           # one pixel, two channel blocks
    ("tiles", 128, 128, 3, 1, 1, (2, 9, 33), HALO128, True),
    ("tiles_lazy", 128, 256, 3, 1, 1, (2, 9, 33), HALO128, True),
    ("tail", 128, 128, 3, 1, 1, (2, 9, 33), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, false, true>", True),
    ("x3", 128, 128, 3, 1, 1, (2, 9, 17), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>", True),
    ("x3_tiles", 128, 256, 3, 1, 1, (2, 9, 33), "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>", True),
    ("gather", 128, 128, 3, 1, 1, (2, 9, 33), "k_conv2d_halo_reg<%s, 128, 8, 3, true>", True),
    ("plain", 64, 128, 3, 1, 1, (2, 13, 21), "k_conv2d_halo_reg<%s, 64, 8, 0, false>", True),
    ("plain", 64, 256, 3, 1, 1, (2, 1, 1), "k_conv2d_halo_reg<%s, 64, 8, 0, false>", True),
    ("plain", 256, 256, 3, 1, 1, (2, 1, 4097), "k_conv2d_halo_reg<%s, 256, 4, 0, false>", True),     # 257 x 2 x 2 = 1 028 workgroups
    ("plain", 256, 128, 3, 1, 1, (2, 65, 497), "k_conv2d_halo_reg<%s, 256, 4, 0, false>", False),    # 17 x 32 x 2 = 1 088
    ("plain", 64, 64, 3, 1, 1, (2, 2, 8209), "k_conv2d_halo_reg<%s, 64, 8, 0, false, 2>", True),     # 514 x 2 = 1 028 tiles of 16 x 16
    ("plain", 64, 64, 3, 1, 1, (2, 241, 513), "k_conv2d_halo_reg<%s, 64, 8, 0, false, 2>", False),   # 16 x 33 x 2 = 1 056
    # ---- k_conv2d_patch
    ("plain", 64, 64, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>", True),
    ("plain", 64, 64, 3, 2, 1, (2, 1, 1), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>", True),
    ("plain", 64, 64, 3, 2, 1, (2, 497, 1249), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>", False),     # 32 x 40 x 2 = 2 560 tiles: the last
    ("plain", 64, 128, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1>", True),
    ("plain", 128, 128, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 128, 3, 2, 4, 16, 1>", True),
    ("plain", 128, 256, 3, 2, 1, (2, 24, 20), "k_conv2d_patch<%s, 128, 3, 2, 4, 16, 1>", True),
    ("plain", 64, 64, 3, 1, 1, (2, 13, 21), "k_conv2d_patch<%s, 64, 3, 1, 16, 16, 2>", True),
    ("plain", 64, 64, 3, 1, 1, (2, 241, 497), "k_conv2d_patch<%s, 64, 3, 1, 16, 16, 2>", False),      # 16 x 32 x 2 = 1 024: the last
    ("plain", 256, 128, 3, 1, 1, (2, 9, 17), "k_conv2d_patch<%s, 256, 3, 1, 4, 16, 1>", True),
    ("plain", 256, 256, 3, 1, 1, (2, 1, 1), "k_conv2d_patch<%s, 256, 3, 1, 4, 16, 1>", True),
    ("plain", 256, 128, 3, 1, 1, (2, 61, 497), "k_conv2d_patch<%s, 256, 3, 1, 4, 16, 1>", False),     # 16 x 32 x 2 = 1 024: the last
    ("plain", 64, 128, 4, 4, 0, (2, 37, 53), "k_conv2d_patch<%s, 64, 4, 4, 2, 16, 1>", True),
    ("plain", 128, 128, 2, 2, 0, (2, 23, 19), "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>", True),
    ("plain", 128, 128, 2, 2, 0, (2, 63, 995), "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>", False),     # 16 x 32 x 2 = 1 024: the last
    ("plain", 128, 128, 2, 2, 0, (2, 7, 8195), "k_conv2d_patch<%s, 128, 2, 2, 4, 16, 1>", True),      # 2 x 257 x 2 = 1 028 tiles of 2 x 16
    ("plain", 128, 128, 2, 2, 0, (2, 67, 995), "k_conv2d_patch<%s, 128, 2, 2, 4, 16, 1>", False),     # 17 x 32 x 2 = 1 088
    ("plain", 256, 128, 1, 1, 0, (2, 9, 17), "k_conv2d_patch<%s, 256, 1, 1, 2, 16, 1>", True),
    ("plain", 384, 256, 1, 1, 0, (2, 13, 21), "k_conv2d_patch<%s, 384, 1, 1, 2, 16, 1>", True),
    ("plain", 384, 128, 1, 1, 0, (2, 1, 1), "k_conv2d_patch<%s, 384, 1, 1, 2, 16, 1>", True),
    ("into", 128, 128, 2, 2, 0, (2, 23, 19), "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>", True),
    ("into", 64, 64, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>", True),
    ("into", 256, 128, 1, 1, 0, (2, 9, 17), "k_conv2d_patch<%s, 256, 1, 1, 2, 16, 1>", True),
    ("rows", 64, 64, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true>", True),
    ("rows", 64, 64, 3, 2, 1, (2, 241, 993), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true>", False),  # 16 x 32 x 2 = 1 024: the last
    ("rows", 64, 64, 3, 2, 1, (2, 3, 16417), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true, true>", True),   # 514 x 2 = 1 028
    ("rows", 64, 64, 3, 2, 1, (2, 257, 993), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true, true>", False),  # 17 x 32 x 2 = 1 088
    ("rows", 64, 128, 3, 2, 1, (2, 23, 19), "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1, true>", True),
    # ---- k_conv1x1_nhwc: 306 pixels (no multiple of 128 * 4), 126 (below one tile), 2
    ("plain", 128, 128, 1, 1, 0, (2, 9, 17), "k_conv1x1_nhwc<%s, 128, 4>", True),
    ("plain", 128, 256, 1, 1, 0, (2, 7, 9), "k_conv1x1_nhwc<%s, 128, 4>", True),
    ("plain", 128, 64, 1, 1, 0, (2, 9, 17), "k_conv1x1_nhwc<%s, 64, 4>", True),
    ("plain", 128, 192, 1, 1, 0, (2, 7, 9), "k_conv1x1_nhwc<%s, 64, 4>", True),
    ("plain", 128, 64, 1, 1, 0, (2, 1, 1), "k_conv1x1_nhwc<%s, 64, 4>", True),
    # ---- k_conv2d_nhwc_dma: 64-wide below kGenericSmallMap = 384 workgroups of 128-wide tiles, 128-wide from it on
    ("plain", 192, 128, 3, 1, 1, (2, 13, 21), "k_conv2d_nhwc_dma<%s, 64>", True),
    ("plain", 192, 256, 3, 1, 1, (2, 80, 147), "k_conv2d_nhwc_dma<%s, 64>", False),                  # 184 x 2 = 368
    ("plain", 192, 256, 3, 1, 1, (2, 80, 150), "k_conv2d_nhwc_dma<%s, 128>", False),                 # 192 x 2 = 384: the first
    ("plain", 64, 256, 1, 1, 0, (2, 80, 150), "k_conv2d_nhwc_dma<%s, 128>", True),
    ("plain", 64, 64, 3, 2, 1, (2, 321, 1921), "k_conv2d_nhwc_dma<%s, 64>", False),                  # 21 x 61 x 2 = 2 562 tiles: past the patch form
]

# every instantiation launch_conv2d_plan_t's switch holds in a default process (ROLL == 3, no SEC_PATCH_S1); x3 exists on bf16 only
INSTANTIATIONS = [
    "k_conv2d_halo_reg<%s, 128, 8, 3, false>",
    "k_conv2d_halo_reg<%s, 128, 8, 3, true>",
    "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, false, true>",
    "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>",
    "k_conv2d_halo_reg<%s, 64, 8, 0, false>",
    "k_conv2d_halo_reg<%s, 256, 4, 0, false>",
    "k_conv2d_halo_reg<%s, 64, 8, 0, false, 2>",
    "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2>",
    "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1>",
    "k_conv2d_patch<%s, 128, 3, 2, 4, 16, 1>",
    "k_conv2d_patch<%s, 64, 3, 1, 16, 16, 2>",
    "k_conv2d_patch<%s, 256, 3, 1, 4, 16, 1>",
    "k_conv2d_patch<%s, 64, 4, 4, 2, 16, 1>",
    "k_conv2d_patch<%s, 128, 2, 2, 4, 16, 1>",
    "k_conv2d_patch<%s, 128, 2, 2, 2, 16, 1>",
    "k_conv2d_patch<%s, 256, 1, 1, 2, 16, 1>",
    "k_conv2d_patch<%s, 384, 1, 1, 2, 16, 1>",
    "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true, true>",
    "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true>",
    "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1, true>",
    "k_conv1x1_nhwc<%s, 128, 4>",
    "k_conv1x1_nhwc<%s, 64, 4>",
    "k_conv2d_nhwc_dma<%s, 128>",
    "k_conv2d_nhwc_dma<%s, 64>",
]
# decision thresholds: (what, the case ON the limit, the first case past it) as indices are not stable -- the rows are found by value
THRESHOLDS = [
    ("64->64 3x3/s1: 1 024 | 1 056 workgroups of 16 x 16", ("plain", 64, 64, 3, 1, 1, (2, 241, 497)), ("plain", 64, 64, 3, 1, 1, (2, 241, 513))),
    ("256->128 3x3/s1: 1 024 | 1 088 workgroups of 4 x 16", ("plain", 256, 128, 3, 1, 1, (2, 61, 497)), ("plain", 256, 128, 3, 1, 1, (2, 65, 497))),
    ("128->128 2x2/s2: 1 024 | 1 088 tiles of 2 x 16", ("plain", 128, 128, 2, 2, 0, (2, 63, 995)), ("plain", 128, 128, 2, 2, 0, (2, 67, 995))),
    ("rows 64->64 3x3/s2: 1 024 | 1 088 workgroups", ("rows", 64, 64, 3, 2, 1, (2, 241, 993)), ("rows", 64, 64, 3, 2, 1, (2, 257, 993))),
    ("64->64 3x3/s2: 2 560 | 2 562 tiles of 8 x 16", ("plain", 64, 64, 3, 2, 1, (2, 497, 1249)), ("plain", 64, 64, 3, 2, 1, (2, 321, 1921))),
    ("192->256 3x3/s1 generic: 368 | 384 workgroups", ("plain", 192, 256, 3, 1, 1, (2, 80, 147)), ("plain", 192, 256, 3, 1, 1, (2, 80, 150))),
]


def case_id(c):
    return "%s-%d-%d-k%ds%d-%dx%dx%d" % (c[0], c[1], c[2], c[3], c[4], *c[6])


def case_kinds(form):
    return ("bf16",) if form.startswith("x3") else KINDS


def workgroup_count(c, th, tw, cout_per_wg):
    """batch x tiles of th x tw OUTPUT pixels x channel blocks: what several_rounds (csrc/dense.hip) compares with 1 024."""
    _, _, cout, k, s, p, (b, h, w) = c[:7]
    ho, wo = out_size(h, k, s, p), out_size(w, k, s, p)
    return b * -(-ho // th) * -(-wo // tw) * (cout // cout_per_wg)


# ------------------------------------------------------------------------------------------------ site maps and tile lists
def border_site_map(shape, frames, planes=None, seed=0, density=0.3):
    """int32 site map [B, (planes,) H, W] of row + 1 (0: no site), one entry of `frames` per frame: "busy" = sites on all four
    borders, the four corners (the ragged one among them) and a random share inside; "single" = one site; "none" = no site.  Rows
    are numbered frame by frame: a frame's rows start where the frame before ends.  -> (site_map, rows in all)."""
    b, h, w = shape
    assert len(frames) == b
    rng = np.random.default_rng(seed + 17 * h + w)
    dims = (h, w) if planes is None else (planes, h, w)
    occ = np.zeros((b,) + dims, bool)
    for f, what in enumerate(frames):
        if what == "busy":
            o = rng.random(dims) < density
            o[..., 0, :] |= rng.random(dims[:-2] + (w,)) < 0.5
            o[..., -1, :] |= rng.random(dims[:-2] + (w,)) < 0.5
            o[..., :, 0] |= rng.random(dims[:-1]) < 0.5
            o[..., :, -1] |= rng.random(dims[:-1]) < 0.5
            o[..., 0, 0] = o[..., 0, -1] = o[..., -1, 0] = o[..., -1, -1] = True
            occ[f] = o
        elif what == "single":
            occ[(f,) + (() if planes is None else (planes - 1,)) + (h // 2, w // 3)] = True
        else:
            assert what == "none"
    site_map = np.zeros((b,) + dims, np.int32)
    n = int(occ.sum())
    site_map[occ] = np.arange(1, n + 1, dtype=np.int32)
    return site_map, n


def dense_from_rows(rows, site_map):
    """[..., C]: rows gathered through a map of row + 1 (0: zeros)."""
    z = np.concatenate([np.zeros_like(rows[:1]), rows])
    return z[site_map]


def tile_lists(shape, live, th=8, tw=16):
    """order [B, tiles] int16 / counts [B] int32 of sec_rpn_tile_live's format for the given live tiles per frame: live first, the
    others from the END backwards."""
    b, h, w = shape
    tiles = -(-h // th) * -(-w // tw)
    order = np.zeros((b, tiles), np.int16)
    for f, lv in enumerate(live):
        rest = [t for t in range(tiles) if t not in lv]
        order[f, :len(lv)] = lv
        order[f, len(lv):] = rest[::-1]
    return order, np.array([len(lv) for lv in live], np.int32)


def tile_slices(t, shape, th=8, tw=16):
    tx = -(-shape[2] // tw)
    return slice((t // tx) * th, (t // tx) * th + th), slice((t % tx) * tw, (t % tx) * tw + tw)


def neighbour_masks(shape, order, written, th=8, tw=16):
    """nbr_masks [2, B, tiles] int16 of sec_rpn_tile_live_masks: bit (dy + 1) * 3 + dx + 1 of a tile = that neighbour was WRITTEN by the
    producer (or lies outside the image); half 0 in the order of the list, half 1 by tile index."""
    b, h, w = shape
    ty, tx = -(-h // th), -(-w // tw)
    by_tile = np.zeros((b, ty * tx), np.int16)
    for f in range(b):
        for t in range(ty * tx):
            m = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = t // tx + dy, t % tx + dx
                    if not (0 <= yy < ty and 0 <= xx < tx) or (yy * tx + xx) in written[f]:
                        m |= 1 << ((dy + 1) * 3 + dx + 1)
            by_tile[f, t] = m
    by_rank = np.take_along_axis(by_tile, order.astype(np.int64), axis=1)
    return np.stack([by_rank, by_tile])
