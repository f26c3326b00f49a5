"""fp64 references, per-element error bounds, exact-integer cases and the case tables of the dense RPN TRAINING kernels
(csrc/dense_train.hip: k_conv2d_wgrad3x3, k_conv2d_wgrad3x3_row, k_conv2d_wgrad_reduce, k_bn_partial, k_bn_*_finalize, k_bn_apply,
k_bn_apply_small, k_conv2d_pack_train; and the forward / data gradient on k_conv2d_halo_reg).  numpy on the CPU; shared by
tests/test_dense_train_ref_host.py (which proves on the CPU that the bounds bite) and tests/test_gpu_dense_train_fp64.py (which holds
the kernels to them).  Activations are [B, H, W, C] arrays (channels-last memory as the kernels see it), already rounded to the 16-bit
type; weights are torch's [Cout, Cin, k, k]."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from indice_conv_bwd_helpers import U24, U_STORE, worst  # noqa: F401  (same constants, same `worst`: no element excluded, NaN = inf)

TINY = 1e-30                  # keeps 0 <= 0 from failing on a -0.0
FP16_SUB = 2.0 ** -25         # half the spacing of the fp16 subnormals: absolute floor of an fp16 store


def gamma_n(n, u=U24):
    """Higham's gamma_n = n u / (1 - n u) (Accuracy and Stability, 3.1): n roundings compound to at most this, no first-order
    shortcut."""
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


def store_floor(kind):
    return FP16_SUB if kind == "fp16" else TINY


# ------------------------------------------------------------------------------------------------ weight gradient
def _taps(ksize):
    return [(ky, kx) for ky in range(3) for kx in range(3)] if ksize == 3 else [(1, 1)]


def _padded_flat(a):
    """[B,H,W,C] -> the flat rows of the tensor with a ring of one zero pixel around every image, [B (H+2) (W+2), C].  On this layout
    the pixel at offset (dy, dx) of pixel p is row p + dy (W + 2) + dx, and a pixel outside the image reads zeros: a tap of the
    convolution is ONE contiguous slice."""
    b, h, w, c = a.shape
    p = np.zeros((b, h + 2, w + 2, c), a.dtype)
    p[:, 1:-1, 1:-1] = a
    return p.reshape(-1, c)


def wgrad_terms(shape, ksize):
    """terms[tap] = number of pixel pairs (p, p + offset(tap)) with the shifted pixel inside the image."""
    b, h, w = shape
    return np.array([b * (h - abs(ky - 1)) * (w - abs(kx - 1)) for ky, kx in _taps(ksize)], np.int64)


def wgrad_reference(x, dy, ksize, dtype=np.float64, want_mag=True):
    """dW[co][ci][ky][kx] = sum over pixels p of x[p + (ky - 1, kx - 1)][ci] * dy[p][co]  (stride 1, padding k // 2; k = 3 or 1).
    x [B,H,W,Cin], dy [B,H,W,Cout]: the operands ALREADY ROUNDED to 16 bit.  -> (dw64 [Cout,Cin,k,k], mag, terms[tap]): mag is the
    same sum over |x| |dy|, terms[tap] the number of pixel pairs of that tap whose shifted pixel lies inside the image.
    dtype = np.float32 is for the exact-integer cases only (every partial sum an integer below 2^24: float32 sgemm is exact)."""
    b, h, w, cin = x.shape
    cout = dy.shape[3]
    assert dy.shape[:3] == x.shape[:3] and ksize in (1, 3)
    xp, dp = _padded_flat(np.asarray(x, dtype)), _padded_flat(np.asarray(dy, dtype))
    s, e = w + 3, len(xp) - (w + 3)                          # every real pixel, and every shifted row stays inside the array
    taps = _taps(ksize)
    dw = np.zeros((cout, cin, ksize, ksize), np.float64)
    mag = np.zeros_like(dw) if want_mag else None
    xa, da = (np.abs(xp), np.abs(dp)) if want_mag else (None, None)
    for i, (ky, kx) in enumerate(taps):
        off = (ky - 1) * (w + 2) + (kx - 1)
        oy, ox = (ky, kx) if ksize == 3 else (0, 0)
        dw[:, :, oy, ox] = dp[s:e].T @ xp[s + off:e + off]
        if want_mag:
            mag[:, :, oy, ox] = da[s:e].T @ xa[s + off:e + off]
    return dw, mag, wgrad_terms((b, h, w), ksize)


def bound_wgrad(mag, terms):
    """|dW - ref| per element <= gamma_n * mag, n = terms[tap], gamma_n = n u / (1 - n u), u = 2^-24.
    The kernel adds the products of an element in fp32: inside an MFMA (v_mfma_f32_32x32x16: 16 pixels per instruction, the order
    inside it is the hardware's), over the steps of a slice into one accumulator, then over the slices in k_conv2d_wgrad_reduce (four
    chains, fixed order).  Whatever the order, a sum of n numbers t_i in fp32 errs by at most gamma_(n-1) sum |t_i| (Higham 4.2) -- every
    t_i passes at most n - 1 additions -- and n is what is used here.  The t_i themselves are EXACT: the product of two bf16 values
    has 8 + 8, of two fp16 values 11 + 11 significant bits, both fit the 24 of fp32, and the exponents fit its range -- with one
    caveat: fp16 operands below 2^-14 are subnormal; their products (down to 2^-48) are still normal fp32 numbers, so nothing
    underflows, but the bound grants nothing to an implementation that flushes subnormal INPUTS (dy = N(0,1) / 8 rounds to a subnormal a few
    hundred times per case; each would lose up to 2^-14 |x|).  bf16 has fp32's exponent range: a product underflows only below
    2^-126.  Pixels
    whose shifted pixel is outside the image add an exact zero and are not counted.  `terms` is indexed [ky * k + kx]."""
    k = mag.shape[2]
    g = gamma_n(np.asarray(terms, np.float64)).reshape(k, k)
    return g[None, None] * mag + TINY


def old_check_wgrad(dw, ref):
    """tests/test_gpu_train_dense.py::test_conv2d_wgrad_vs_torch: the largest error relative to the tensor's maximum < 2e-3."""
    return bool(np.abs(dw - ref).max() / np.abs(ref).max() < 2e-3)


# ------------------------------------------------------------------------------------------------ forward / data gradient
def conv_reference(x, w16, transposed_dgrad=False, bias=None):
    """y[p][co] = sum_{tap, ci} x[p + offset(tap)][ci] w16[co][ci][tap] (+ bias[co]): x [B,H,W,Cin], w16 [Cout,Cin,k,k] rounded to the
    16-bit type, k = 3 (padding 1) or 1.  transposed_dgrad: the data gradient instead -- x is dY [B,H,W,Cout] and the result is
    dX[p][ci] = sum_{tap, co} dY[p - offset(tap)][co] w16[co][ci][tap].  -> (ref64, mag, T): mag the same sum over magnitudes (|bias|
    included), T = k * k * C_contracted the number of products of an element."""
    w = np.asarray(w16, np.float64)
    if transposed_dgrad:
        w = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))      # W'[ci][co][ky][kx] = W[co][ci][k-1-ky][k-1-kx]
    cout, cin, k, _ = w.shape
    b, h, wd, c = x.shape
    assert c == cin
    xp = _padded_flat(np.asarray(x, np.float64))
    xa = np.abs(xp)
    s, e = wd + 3, len(xp) - (wd + 3)
    ref = np.zeros((len(xp), cout))
    mag = np.zeros_like(ref)
    for ky, kx in _taps(k):
        off = (ky - 1) * (wd + 2) + (kx - 1)
        wt = w[:, :, ky if k == 3 else 0, kx if k == 3 else 0].T
        ref[s:e] += xp[s + off:e + off] @ wt
        mag[s:e] += xa[s + off:e + off] @ np.abs(wt)
    ref = ref.reshape(b, h + 2, wd + 2, cout)[:, 1:-1, 1:-1]
    mag = mag.reshape(b, h + 2, wd + 2, cout)[:, 1:-1, 1:-1]
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)
        mag = mag + np.abs(np.asarray(bias, np.float64))
    return np.ascontiguousarray(ref), np.ascontiguousarray(mag), k * k * cin


def bound_conv(ref, mag, terms, kind, bias=False):
    """|y - ref| per element of a 16-bit output of k_conv2d_halo_reg: exact products (see bound_wgrad), fp32 accumulation of T = k k C
    of them in the MFMA order (+ one fp32 addition of the bias), a = ref + e with |e| <= gamma_T mag, then ONE round-to-nearest store:
    |rn(a) - ref| <= u16 |a| + |e| <= u16 |ref| + (1 + u16) gamma_T mag, u16 = 2^-8 (bf16) / 2^-11 (fp16); fp16 results below 2^-14
    are subnormal, spaced 2^-24: 2^-25 as an absolute floor.  The shape of bound_dfeat in indice_conv_bwd_helpers, with gamma_T
    written out."""
    u = U_STORE[kind]
    return u * np.abs(ref) + (1 + u) * gamma_n(terms + (1 if bias else 0)) * mag + store_floor(kind)


def bound_sum32(mag, n):
    """A plain fp32 sum of n exact terms in any order (the bias gradient of the heads: dy.float().sum): gamma_n * sum |t|."""
    return gamma_n(n) * mag + TINY


# ------------------------------------------------------------------------------------------------ exact-integer cases
def integer_case(shape, cout=128, seed=0):
    """x in {-2..2} [B,H,W,128] and dy in {-1,0,1} [B,H,W,cout] as int8: exact in bf16 and fp16, every product an integer of magnitude
    <= 2, every partial sum an integer of magnitude <= 2 P < 2^24 -- exact in fp32 in ANY order, so the kernel must equal the
    integer reference bit for bit (np.array_equal)."""
    b, h, w = shape
    assert 2 * b * h * w < 2 ** 24
    rng = np.random.default_rng(seed + 31 * b + 7 * h + w + cout)
    x = rng.integers(-2, 3, (b, h, w, 128), dtype=np.int8)
    dy = rng.integers(-1, 2, (b, h, w, cout), dtype=np.int8)
    return x, dy


def integer_reference(x, dy, ksize):
    """The integer weight gradient as float32 [Cout,Cin,k,k]: one float32 sgemm per tap over contiguous slices of the zero-ringed
    tensors (exact here, see integer_case; fast enough for the 692 224-pixel case)."""
    dw, _, _ = wgrad_reference(x, dy, ksize, dtype=np.float32, want_mag=False)
    assert np.array_equal(dw, np.round(dw)) and np.abs(dw).max(initial=0) < 2 ** 24
    return dw.astype(np.float32)


# ------------------------------------------------------------------------------------------------ what the host code decides
WGRAD_ROW_FROM = 160000       # pixels from which the 3x3 weight gradient takes the row form by itself
WGRAD_ROW_SLICES = 80
WGRAD_RESLICE_ABOVE = 256 * 42 * 64     # 688 128 pixels: above it the tap form has more than 256 slices of 42 steps and re-slices


def wgrad_plan(pixels, width, ntaps, row):
    """(form, steps per slice, slices) of run_wgrad for a request `row` (True / False: SEC_WGRAD_ROW=1 / 0, None: unset)."""
    total = (pixels + 63) // 64
    if row is None:
        row = pixels >= WGRAD_ROW_FROM
    if ntaps == 9 and width >= 16 and row:
        steps = max(3, (-(-total // WGRAD_ROW_SLICES) + 2) // 3 * 3)
        return "row", steps, -(-total // steps)
    steps = 6 if ntaps == 1 else 42
    gx = -(-total // steps)
    if gx > 256:
        steps = (-(-total // 256) + 2) // 3 * 3
        gx = -(-total // steps)
    return "tap", steps, max(gx, 1)


# ------------------------------------------------------------------------------------------------ BatchNorm + ReLU
BN_SMALL_ROWS = 1 << 17
BN_GROUPS = {True: 128, False: 512}       # small path / three-launch path


def bn_chain(capacity, live, c):
    """(groups, d): the workgroup count of k_bn_partial and the length d of the longest fp32 chain behind one of its partial sums.
    A workgroup of 256 threads covers ppi = 256 / (C / 8) pixels per trip and the grid `groups * ppi` pixels per round, so a thread
    adds at most ceil(live / (groups * ppi)) values (its first addition, to 0.0f, is exact but counted), and the LDS pass adds the ppi
    thread sums of a channel one after the other: d = ceil(live / (groups * ppi)) + ppi.  The path (128 or 512 groups) follows the
    CAPACITY of the buffer (the host cannot see the live count), the chain the live rows."""
    groups = BN_GROUPS[capacity <= BN_SMALL_ROWS]
    ppi = 256 // (c // 8)
    return groups, -(-max(live, 1) // (groups * ppi)) + ppi


def bn_live(p, live):
    """bn_live_rows of the kernel: None -> P; otherwise clamped to [0, P]."""
    return p if live is None else min(max(int(live), 0), p)


class BnRef:
    """Training BatchNorm (+ ReLU) of y [P, C] in float64, its backward for dz [P, C], and the bounds of every output.

    Statistics over the first `live` rows (None: all).  THE KERNEL'S DOCUMENTED RULE, not torch's, for degenerate counts: the divisor
    is max(live, 1) (k_bn_fwd_finalize: `if (P < 1) P = 1`), so live = 0 gives mean 0, variance 0, invstd 1 / sqrt(eps) and running
    statistics that decay towards 0; a single row has the BIASED variance (0) in the running update too (torch would divide by
    zero).  eps and momentum are the fp32 roundings of the arguments (they cross the C ABI as float).

    Arithmetic the bounds rest on (dense_train.hip): sums in fp32 within a thread and within the workgroup's LDS pass (chain length d,
    bn_chain), in double from the group partials on (G additions in double: (G + 6) 2^-53 relative, carried as `dbl`); one float cast
    each of mean and invstd; every element operation in fp32, one rounding each (a contracted fma has fewer: the bounds hold for both).
    With u = 2^-24, sy = sum |y|, syy = sum y^2 over the live rows, n = max(live, 1):
      err_mean   <= gamma_d sy / n + dbl + u (|mean| + that)                           (fp32 chains; the float cast)
      err_var    <= gamma_(d+1) syy / n + 2 |mean| e + e^2, e = gamma_d sy / n + dbl    (y * y is exact in fp32 for 16-bit y; the + 1
                    covers a product that is rounded; var = s1 / n - m^2 in double with the DOUBLE mean: no cast error in it;
                    clamping var at 0 moves it towards the true value)
      err_invstd <= err_var / (2 (max(var - err_var, 0) + eps)^1.5) + u (invstd + that)  (|d/dv (v + eps)^-1/2| is largest at the low end)
      running    <= momentum * err + the roundings of the fp32 update (1 - momentum, two products, one sum; see _running)
    Element chain, t = y - mean, xh = t * invstd, zp = xh * gamma + beta:
      e_t  = err_mean + u (|t| + err_mean)
      e_xh = e_t (invstd + err_invstd) + |t| err_invstd + u (|xh| + the former)
      e_zp = A + u (|zp| + A),  A = e_xh |gamma| + u (|xh| + e_xh) |gamma|              = bound_zp
      z    : e_zp + u16 (|ref| + e_zp) + the fp16 subnormal floor
    ReLU mask: an element is AMBIGUOUS iff |zp64| <= bound_zp; it may take either branch (z is then within the same bound of
    max(zp64, 0) either way; dy is accepted against either branch).  Every other element must take the reference's branch: a
    negative one must be exactly 0 in z.
    Backward, g = dz * mask:
      dbeta  <= gamma_d sum |g| + dbl + sum_ambiguous |dz| + u |.|
      dgamma <= gamma_(d+1) sum |g| (|xh| + e_xh) + sum |g| e_xh + dbl + sum_ambiguous |dz xh| + u |.|
      dy = k (g - dbeta inv - xh dgamma inv), k = gamma invstd, inv = fl(1 / n):
        e_k = |gamma| err_invstd + u (|k| + that);  B = dbeta / n: e_B = e_db / n + gamma_2 (|B| + e_db / n);
        Cc = xh dgamma / n: e_C = (e_xh |dgamma| + |xh| e_dg + e_xh e_dg) / n + gamma_3 (|Cc| + that);
        I = g - B - Cc: e_I = e_B + e_C + gamma_2 (|g| + |B| + |Cc| + e_B + e_C);
        dy: e_k (|I| + e_I) + |k| e_I + u (|dy| + those), then the 16-bit store as for z."""

    def __init__(self, y, dz, gamma, beta, eps, momentum, relu, live=None, running_mean=None, running_var=None, kind="bf16",
                 capacity=None):
        self.y, self.dz = y, dz
        p_cap, c = y.shape
        self.c, self.kind, self.relu = c, kind, bool(relu)
        self.live = bn_live(p_cap, live)
        self.capacity = p_cap if capacity is None else capacity
        n = max(self.live, 1)
        self.n = n
        self.eps = float(np.float32(eps))
        self.mom = float(np.float32(momentum))
        self.gamma, self.beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
        self.groups, self.d = bn_chain(self.capacity, self.live, c)
        u = U24
        dblrel = (self.groups + 6) * 2.0 ** -53
        # ---- statistics (blocked: the elementwise temporaries of 131 073 x 256 in float64 would not fit a test's budget)
        s0 = np.zeros(c); sy = np.zeros(c); syy = np.zeros(c)
        for r0, r1 in self.blocks():
            yb = np.asarray(y[r0:r1], np.float64)
            s0 += yb.sum(0); sy += np.abs(yb).sum(0); syy += (yb * yb).sum(0)
        self.mean = s0 / n
        # two-pass variance: the reference itself must not cancel
        v = np.zeros(c)
        for r0, r1 in self.blocks():
            t = np.asarray(y[r0:r1], np.float64) - self.mean
            v += (t * t).sum(0)
        self.var = v / n if self.live > 0 else np.zeros(c)
        if self.live == 0:
            self.mean = np.zeros(c)
        self.invstd = 1.0 / np.sqrt(self.var + self.eps)
        e = gamma_n(self.d) * sy / n + dblrel * sy / n
        self.err_mean = e + u * (np.abs(self.mean) + e)
        self.err_var = gamma_n(self.d + 1) * syy / n + dblrel * syy / n + 2 * np.abs(self.mean) * e + e * e
        lo = np.maximum(self.var - self.err_var, 0.0) + self.eps
        ei = self.err_var / (2 * lo ** 1.5)
        self.err_invstd = ei + u * (self.invstd + ei)
        # ---- running statistics: torch's convention (unbiased variance), the kernel's rule for a single row
        self.var_unb = self.var * n / (n - 1) if n > 1 else self.var
        self.err_var_unb = (self.err_var * n / (n - 1) if n > 1 else self.err_var)
        self.err_var_unb = self.err_var_unb + u * (self.var_unb + self.err_var_unb)            # the float cast of the unbiased variance
        self.running_mean = self.running_var = self.bound_running_mean = self.bound_running_var = None
        if running_mean is not None:
            self.running_mean, self.bound_running_mean = self._running(running_mean, self.mean, self.err_mean)
        if running_var is not None:
            self.running_var, self.bound_running_var = self._running(running_var, self.var_unb, self.err_var_unb)
        # ---- backward sums (need the masks: one more blocked pass), then their bounds
        self.dbeta = self.dgamma = None
        if dz is not None:
            sg = np.zeros(c); sgx = np.zeros(c); ag = np.zeros(c); agx = np.zeros(c); agex = np.zeros(c); amb_g = np.zeros(c); amb_gx = np.zeros(c)
            n_amb = 0

            def sums(rr):
                f = self._forward_block(*rr)
                dzb = np.asarray(dz[rr[0]:rr[1]], np.float64)
                g = dzb * f["mask"]
                a = f["amb"]
                return (g.sum(0), (g * f["xh"]).sum(0), np.abs(g).sum(0), (np.abs(g) * (np.abs(f["xh"]) + f["e_xh"])).sum(0),
                        (np.abs(g) * f["e_xh"]).sum(0), (np.abs(dzb) * a).sum(0), (np.abs(dzb * f["xh"]) * a).sum(0), int(a.sum()))
            for t in self._map(sums):                           # block order: the float64 sums do not depend on the thread schedule
                sg += t[0]; sgx += t[1]; ag += t[2]; agx += t[3]; agex += t[4]; amb_g += t[5]; amb_gx += t[6]; n_amb += t[7]
            self.dbeta, self.dgamma = sg, sgx
            eb = gamma_n(self.d) * ag + dblrel * ag + amb_g
            self.bound_dbeta = eb + u * (np.abs(sg) + eb) + TINY
            eg = gamma_n(self.d + 1) * agx + agex + dblrel * agx + amb_gx
            self.bound_dgamma = eg + u * (np.abs(sgx) + eg) + TINY
            self.n_ambiguous = n_amb
        else:
            self.n_ambiguous = sum(self._map(lambda rr: int(self._forward_block(*rr)["amb"].sum())))
        self.ambiguous_fraction = self.n_ambiguous / max(self.live * c, 1)

    def blocks(self, rows=8192):
        return [(r0, min(r0 + rows, self.live)) for r0 in range(0, self.live, rows)]

    def _map(self, fn):
        """fn over the row blocks, results in block order; eight threads where there is enough to share (numpy's elementwise loops
        release the interpreter lock) -- the 131 073 x 256 cases are 34 M elements of float64 arithmetic."""
        bl = self.blocks()
        if len(bl) < 4:
            return [fn(b) for b in bl]
        with ThreadPoolExecutor(8) as ex:
            return list(ex.map(fn, bl))

    def _running(self, r, val, err):
        """fp32 update r' = fl(fl(fl(1 - m) r) + fl(m v_f)), v_f the float of the statistic (its error `err` includes that cast):
        m err for the statistic, u |(1 - m) r| twice (the rounding of 1 - m, of the product), u |m v| for the other product, u |r'| for
        the sum -- and the propagated pieces once more to second order."""
        r = np.asarray(r, np.float64)
        a, b = (1.0 - self.mom) * r, self.mom * val
        new = a + b
        e = self.mom * err
        return new, e + U24 * (2 * np.abs(a) + np.abs(b) + e + np.abs(new)) * (1 + 3 * U24) + TINY

    def _forward_block(self, r0, r1):
        u = U24
        yb = np.asarray(self.y[r0:r1], np.float64)
        t = yb - self.mean
        xh = t * self.invstd
        zp = xh * self.gamma + self.beta
        e_t = self.err_mean + u * (np.abs(t) + self.err_mean)
        e_xh = e_t * (self.invstd + self.err_invstd) + np.abs(t) * self.err_invstd
        e_xh = e_xh + u * (np.abs(xh) + e_xh)
        a = e_xh * np.abs(self.gamma) + u * (np.abs(xh) + e_xh) * np.abs(self.gamma)
        e_zp = a + u * (np.abs(zp) + a)
        if self.relu:
            amb = np.abs(zp) <= e_zp
            mask = (zp > 0).astype(np.float64)
        else:
            amb = np.zeros(zp.shape, bool)
            mask = np.ones(zp.shape)
        return dict(t=t, xh=xh, zp=zp, e_xh=e_xh, e_zp=e_zp, amb=amb, mask=mask)

    def elem(self, r0, r1):
        """Rows r0..r1 (live ones): dict(zp, bound_zp, ambiguous, z, bound_z, and with dz: dy, dy_other, bound_dy, bound_dy_other).
        dy_other is the gradient of the OTHER ReLU branch, a legal answer for an ambiguous element only."""
        u, u16 = U24, U_STORE[self.kind]
        f = self._forward_block(r0, r1)
        zp, e_zp, amb = f["zp"], f["e_zp"], f["amb"]
        z = np.maximum(zp, 0.0) if self.relu else zp
        bz = e_zp + u16 * (np.abs(z) + e_zp) + store_floor(self.kind)
        if self.relu:
            bz = np.where((zp < 0) & ~amb, TINY, bz)            # a clearly negative pre-activation is exactly 0
        out = dict(zp=zp, bound_zp=e_zp, ambiguous=amb, z=z, bound_z=bz)
        if self.dz is None:
            return out
        n = self.n
        dzb = np.asarray(self.dz[r0:r1], np.float64)
        k = self.gamma * self.invstd
        e_k = np.abs(self.gamma) * self.err_invstd
        e_k = e_k + u * (np.abs(k) + e_k)
        bq = self.dbeta / n
        e_b = self.bound_dbeta / n
        e_b = e_b + gamma_n(2) * (np.abs(bq) + e_b)
        cc = f["xh"] * self.dgamma / n
        e_c = (f["e_xh"] * np.abs(self.dgamma) + np.abs(f["xh"]) * self.bound_dgamma + f["e_xh"] * self.bound_dgamma) / n
        e_c = e_c + gamma_n(3) * (np.abs(cc) + e_c)

        def one(g):
            inner = g - bq - cc
            e_i = e_b + e_c + gamma_n(2) * (np.abs(g) + np.abs(bq) + np.abs(cc) + e_b + e_c)
            dy = k * inner
            e = e_k * (np.abs(inner) + e_i) + np.abs(k) * e_i
            e = e + u * (np.abs(dy) + e)
            return dy, e + u16 * (np.abs(dy) + e) + store_floor(self.kind)
        out["dy"], out["bound_dy"] = one(dzb * f["mask"])
        # the other branch matters at ambiguous elements only (a handful): elsewhere it is a copy, never consulted
        out["dy_other"], out["bound_dy_other"] = out["dy"], out["bound_dy"]
        if amb.any():
            oth, both = one(dzb * (1.0 - f["mask"]))
            out["dy_other"], out["bound_dy_other"] = np.where(amb, oth, out["dy"]), np.where(amb, both, out["bound_dy"])
        return out

    def worst_elements(self, z=None, dy=None):
        """Largest error / bound of the kernel's z and dy [>= live rows, C] over the live rows, blocked; ambiguous elements of dy are
        held to the better of the two branches.  -> dict(z=..., dy=...)."""
        def block(rr):
            r0, r1 = rr
            e = self.elem(r0, r1)
            wz = worst(z[r0:r1], e["z"], e["bound_z"]) if z is not None else 0.0
            wd = 0.0
            if dy is not None:
                d64 = np.asarray(dy[r0:r1], np.float64)
                r = np.abs(d64 - e["dy"]) / e["bound_dy"]
                if e["ambiguous"].any():
                    r = np.where(e["ambiguous"], np.minimum(r, np.abs(d64 - e["dy_other"]) / e["bound_dy_other"]), r)
                r = np.where(np.isfinite(r), r, np.inf)
                wd = float(r.max()) if r.size else 0.0
            return wz, wd
        per = self._map(block)
        res = {}
        if z is not None:
            res["z"] = max((w[0] for w in per), default=0.0)
        if dy is not None:
            res["dy"] = max((w[1] for w in per), default=0.0)
        return res

    def channel_ratios(self, mean=None, invstd=None, running_mean=None, running_var=None, dbeta=None, dgamma=None):
        """error / bound of the per-channel outputs that are given."""
        out = {}
        for name, got, ref, bound in (("mean", mean, self.mean, self.err_mean + TINY), ("invstd", invstd, self.invstd, self.err_invstd + TINY),
                                      ("running_mean", running_mean, self.running_mean, self.bound_running_mean),
                                      ("running_var", running_var, self.running_var, self.bound_running_var),
                                      ("dbeta", dbeta, self.dbeta, getattr(self, "bound_dbeta", None)),
                                      ("dgamma", dgamma, self.dgamma, getattr(self, "bound_dgamma", None))):
            if got is not None:
                out[name] = worst(got, ref, bound)
        return out


def bn_reference(y, dz, gamma, beta, eps, momentum, relu, live=None, running_mean=None, running_var=None, kind="bf16", capacity=None):
    """The whole reference at once (small cases): dict(mean, var, invstd, running_mean, running_var, z, dbeta, dgamma, dy, zp64, ref)
    in float64; `ref` is the BnRef that holds the bounds.  See BnRef for the rule at live = 0 / 1."""
    r = BnRef(y, dz, gamma, beta, eps, momentum, relu, live, running_mean, running_var, kind, capacity)
    e = r.elem(0, r.live)
    return dict(mean=r.mean, var=r.var, invstd=r.invstd, running_mean=r.running_mean, running_var=r.running_var, z=e["z"], dbeta=r.dbeta,
                dgamma=r.dgamma, dy=e.get("dy"), zp64=e["zp"], ref=r)


def old_check_bn(kind, z, ref_z, rm, ref_rm, rv, ref_rv, dgamma, ref_dgamma, dbeta, ref_dbeta, dy, ref_dy):
    """tests/test_gpu_train_dense.py::test_bn_relu_forward_backward_vs_torch, assertion by assertion."""
    tol = 2.0 ** -7 if kind == "bf16" else 2.0 ** -10
    ok = np.allclose(z, ref_z, rtol=tol, atol=tol * np.abs(ref_z).max())
    ok = ok and np.allclose(rm, ref_rm, rtol=1e-5, atol=1e-6) and np.allclose(rv, ref_rv, rtol=1e-5, atol=1e-6)
    ok = ok and np.allclose(dgamma, ref_dgamma, rtol=1e-3, atol=1e-3 * np.abs(ref_dgamma).max())
    ok = ok and np.allclose(dbeta, ref_dbeta, rtol=1e-3, atol=1e-3 * np.abs(ref_dbeta).max())
    bad = np.abs(dy - ref_dy) > tol * np.abs(ref_dy).max() + tol * np.abs(ref_dy)
    return bool(ok and bad.mean() < 1e-3)


# ------------------------------------------------------------------------------------------------ case tables
WGRAD_SMALL = [(1, 1, 16), (1, 3, 16), (1, 13, 17), (2, 21, 12), (3, 5, 7), (2, 9, 16), (3, 11, 19), (1, 63, 1), (2, 40, 48)]
WGRAD_ONE_TAP = [(2, 21, 12), (3, 11, 19)]
WGRAD_INT_TAP_LAST = (1, 399, 401)        # 159 999 pixels: the last size that takes the tap form by itself
WGRAD_INT_ROW_FIRST = (1, 400, 400)       # 160 000: the first that takes the row form
WGRAD_INT_RESLICE = (1, 832, 832)         # 692 224 > 688 128: the tap form re-slices (gx > 256)
WGRAD_INT_TRAIN = (4, 200, 176)           # car.fhd training
FUNCTION_SHAPE = (2, 19, 23)
PACK_SHAPES = [(128, 128, 3), (128, 128, 1), (64, 128, 1), (128, 256, 1)]
BN_CHANNELS = [8, 16, 32, 64, 128, 256]
BN_SMALL_P = [1, 2, 255, 2325]
BN_SWITCH_P = [BN_SMALL_ROWS, BN_SMALL_ROWS + 1]
BN_SWITCH_C = [8, 128, 256]
BN_OFFSET_P = [2325, BN_SMALL_ROWS + 1]
BN_OFFSET_C = 16
BN_CAP_P = [4096, BN_SMALL_ROWS + 1]
BN_CAP_C = 16
BN_ROWS_N, BN_ROWS_C = 5003, [16, 32, 64]
BN_EPS, BN_MOMENTUM = 1e-3, 0.01
AMBIGUOUS_CAP = 1e-3


def bn_cap_lives(p):
    return [0, 1, 1000, p, p + 5]


def round16(a, kind):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float16)
    return t.float().numpy()


def wgrad_case(shape, kind, cout=128, seed=0):
    """x [B,H,W,128] unit variance, dy [B,H,W,cout] / 8 (the scales of the existing test), rounded to `kind`; float32 arrays."""
    b, h, w = shape
    rng = np.random.default_rng(1000 * b + 10 * h + w + cout + seed)
    x = round16(rng.standard_normal((b, h, w, 128), np.float32), kind)
    dy = round16(rng.standard_normal((b, h, w, cout), np.float32) / 8, kind)
    return x, dy


def bn_case(p, c, kind, variant="plain", seed=0):
    """dict(y, dz [P,C] rounded float32; gamma, beta, running_mean, running_var float32 [C]).  Running statistics start from
    non-trivial values.  beta keeps away from 0 (|beta| >= 1/16) so that a channel whose normalised values are all 0 (a constant or
    all-zero channel, a single row) is not ambiguous wholesale.
    "plain":  y = 2 N(0,1) + a per-channel offset N(0,1).
    "offset": every channel's mean is 8 x (fp16) / 4 x (bf16) its standard deviation (what loads the E[y^2] - E[y]^2 cancellation),
              except channel 1 = one constant (variance exactly 0: invstd = 1 / sqrt(eps)) and channel 2 = all zeros."""
    rng = np.random.default_rng(seed + 17 * c + p % 1000003)
    if variant == "plain":
        y = rng.standard_normal((p, c), np.float32) * 2 + rng.standard_normal((1, c), np.float32)
    else:
        ratio = 8.0 if kind == "fp16" else 4.0
        sd = (0.5 + rng.random((1, c), np.float32))
        y = rng.standard_normal((p, c), np.float32) * sd + ratio * sd * np.where(np.arange(c) % 2, -1.0, 1.0).astype(np.float32)
        y[:, 1] = 3.703125
        y[:, 2] = 0.0
    beta = rng.standard_normal(c).astype(np.float32) / 4
    beta = np.where(np.abs(beta) < 1 / 16, np.copysign(1 / 16, beta + 1e-9), beta).astype(np.float32)
    return dict(y=round16(y, kind), dz=round16(rng.standard_normal((p, c), np.float32), kind),
                gamma=(rng.random(c, np.float32) + 0.5), beta=beta,
                running_mean=(rng.standard_normal(c).astype(np.float32) * 0.3), running_var=(rng.random(c, np.float32) + 0.5))
