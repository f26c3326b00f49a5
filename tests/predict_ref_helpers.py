"""Plain references and input generators for the predict chain (csrc/predict.hip: select -> decode -> finalize).

Nothing here calls a project kernel or a second_amd.models function: torch and numpy only, on whatever device the inputs live on.
tests/test_predict_ref_host.py pins these references to the recorded outputs of the executed reference (tests/golden) and shows that
the comparison used on the GPU catches planted mistakes; tests/test_gpu_predict_edges.py applies them to the kernels.

select_reference      the selection the kernels document: NaN-propagating maximum over classes, first class attaining it, descending
                      by the integer image of the fp32 bit pattern (so +0.0 ranks before -0.0), ties by ascending global anchor index,
                      NaN maxima and masked anchors removed, sigmoid in float64, counts = min(k, N, #{score64 >= float32(thr)}).
decode_reference64    second_box_decode in float64 on the fp32 values, with the per-output bounds derived in decode_bounds().
standup_reference64   the axis-aligned NMS rows in float64 from the device's own decoded fp32 values.
finalize_reference32  the finalize kernel's documented order restated in numpy float32, one IEEE operation per line: bit equality.

The threshold comparison is exact by construction: every generated input keeps |score64 - float32(thr)| >= BAND = 2^-20 for every
anchor that is not exactly on the threshold (the device sigmoid 1 / (1 + expf(-x)) is within 2^-22 of a value <= 1: expf within 1 ulp,
the add and the divide half an ulp each), and logits exactly on a threshold occur only as +-0.0 with thr = 0.5, where both sides are exact.
"""
import math

import numpy as np
import torch

BAND = 2.0 ** -20            # no score closer than this to the threshold unless it is exactly on it
SCORE_RTOL = 2.0 ** -21      # device score vs score64: the 2 ulp of the sigmoid's three operations, doubled
SEL_CHUNK = 8192             # anchors per first-stage workgroup of the chunked select (kSelChunk)
SEL_CHUNK_LARGE = 73728      # ... for heads above 72 * 8192 anchors (the KP = 36 chunks)
REG_CAP = 72 * 1024          # keys one second-stage / direct workgroup holds; also the number of candidate slots


# ---------------------------------------------------------------------------------------------------------------- the select
def select_form(n, dtype):
    """The form the select takes for n anchors per frame: a name and the number of first-stage chunks.  An independent restatement of
    predict_select_decide (csrc/predict.hip); test_predict_ref_host.py holds it equal to ops.predict_select_plan."""
    if dtype == torch.float32:
        return "radix32", 0
    c4 = -(-n // SEL_CHUNK)
    if c4 >= 2 and c4 * 1024 <= REG_CAP:
        pairs = -(-(c4 * 1024 // 2) // 1024)
        return "chunk4+kp%d" % (5 if pairs <= 5 else 10 if pairs <= 10 else 20 if pairs <= 20 else 36), c4
    c36 = -(-n // REG_CAP)
    if n > REG_CAP and c36 * 1024 <= REG_CAP:
        pairs = -(-(c36 * 1024 // 2) // 1024)
        return "chunk36+kp%d" % (5 if pairs <= 5 else 10 if pairs <= 10 else 20 if pairs <= 20 else 36), c36
    if n <= REG_CAP:
        return "direct", 0
    return "radix16", 0


def concat_views(cls_views):
    """[B, N, C] float32 of one [B, A, H, W, C] (or [B, N, C]) tensor or of a list of them (anchors of view s follow those of s - 1)."""
    if isinstance(cls_views, torch.Tensor):
        cls_views = [cls_views]
    return torch.cat([v.reshape(v.shape[0], -1, v.shape[-1]).float() for v in cls_views], 1)


def order_key(x):
    """Monotone int64 image of fp32 bit patterns: a < b as floats (and -0.0 < +0.0) <=> key(a) < key(b).  NaN must be removed by the caller."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)


def first_max(x):
    """(value, index, any-NaN) of the FIRST class attaining the maximum of x [..., C] under float comparison (-0.0 == +0.0)."""
    nan = torch.isnan(x).any(-1)
    clean = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    top = clean.max(-1, keepdim=True).values
    c = x.shape[-1]
    ids = torch.arange(c, device=x.device).expand_as(x)
    label = torch.where(clean == top, ids, torch.full_like(ids, c)).min(-1).values
    best = torch.gather(clean, -1, label.unsqueeze(-1)).squeeze(-1)
    best = torch.where(nan, torch.full_like(best, math.nan), best)
    return best, label, nan


def select_reference(cls_views, k, thr, mask=None):
    """-> dict(idx, score64, label: per-frame lists of the first counts[b] entries; counts [B] int64; margin: min |score64 - float32(thr)|
    over the anchors that are not exactly on the threshold)."""
    x = concat_views(cls_views)
    b, n, _ = x.shape
    best, label, nan = first_max(x)
    thr32 = float(np.float32(thr))
    score64 = torch.sigmoid(best.double())
    alive = ~nan
    if mask is not None:
        alive = alive & (mask.reshape(b, n) != 0)
    key = torch.where(alive, order_key(torch.where(nan, torch.zeros_like(best), best)), torch.full((b, n), -1, dtype=torch.int64, device=x.device))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    passing = (alive & (score64 >= thr32)).sum(1)
    counts = torch.clamp(passing, max=min(int(k), n))
    off = (~nan) & (score64 != thr32)
    dist = torch.where(off, (score64 - thr32).abs(), torch.full_like(score64, math.inf))
    out = {"idx": [], "score64": [], "label": [], "counts": counts, "margin": float(dist.min())}
    for f in range(b):
        i = order[f, :int(counts[f])]
        out["idx"].append(i)
        out["score64"].append(score64[f, i])
        out["label"].append(label[f, i])
    return out


def check_selection(got, ref, score_rtol=SCORE_RTOL):
    """The comparison of every select test: counts equal, rows [0, counts[b]) of top_idx / top_label equal to the reference's, top_score
    within score_rtol (relative) of score64.  -> the largest relative score error seen.  ``got`` = (top_idx, top_score, top_label, counts)."""
    top_idx, top_score, top_label, counts = got
    assert counts.long().tolist() == ref["counts"].tolist(), (counts.tolist(), ref["counts"].tolist())
    worst = 0.0
    for f in range(counts.shape[0]):
        c = int(ref["counts"][f])
        if c == 0:
            continue
        gi, ri = top_idx[f, :c].long(), ref["idx"][f]
        if not torch.equal(gi, ri):
            j = int((gi != ri).nonzero()[0])
            raise AssertionError(f"frame {f}: row {j} of {c} is anchor {int(gi[j])}, the reference has {int(ri[j])}")
        assert torch.equal(top_label[f, :c].long(), ref["label"][f]), f"frame {f}: labels"
        s64 = ref["score64"][f]
        rel = ((top_score[f, :c].double() - s64).abs() / s64).max().item()
        worst = max(worst, rel)
        assert rel <= score_rtol, f"frame {f}: score off by {rel:.3e} relative (bound {score_rtol:.3e})"
    return worst


# ---------------------------------------------------------------------------------------------------------------- select inputs
def factor_ahw(n):
    """(A, H, W) with A * H * W = n and W not a power of two wherever n allows it (W odd > 1, then the rest split once more); (1, 1, n) otherwise."""
    m, two = n, 1
    while m % 2 == 0:
        m //= 2
        two *= 2
    if m == 1:                                   # a power of two (1 included): nothing else to choose
        return (1, 1, n)
    for p in (3, 5, 7, 11, 13):                  # a small odd factor as A when there is one, the odd rest as W
        if m % p == 0 and m // p > 1:
            return (p, two, m // p)
    return (1, two, m)


def thr_logit(thr):
    """The logit whose sigmoid is thr (a stand-in for thr <= 0, where every finite logit passes)."""
    return math.log(thr / (1.0 - thr)) if 0.0 < thr < 1.0 else -4.0


def redraw_band(x, thr):
    """Re-draw (one unit down, repeatedly) every logit of x (already rounded to its dtype) whose float64 sigmoid lies within 2 * BAND of
    float32(thr) without being exactly on it.  Exactly-on-threshold values are left alone: the generators only make them for thr = 0.5."""
    thr32 = float(np.float32(thr))
    for _ in range(8):
        s = torch.sigmoid(x.double())
        bad = (s != thr32) & ((s - thr32).abs() < 2 * BAND)
        if not bool(bad.any()):
            return x
        x = torch.where(bad, (x.float() - 1.0).to(x.dtype), x)
    raise AssertionError("redraw_band did not converge")


def _chunk_len(n):
    return SEL_CHUNK if n <= REG_CAP * SEL_CHUNK // 1024 else SEL_CHUNK_LARGE


def make_logits(pattern, b, n, nc, thr, dtype, seed):
    """[b, n, nc] class logits of ``dtype`` on the CPU, frame f drawn from seed + 1000 f.
    tie      5 levels around the threshold's logit (two above it), every anchor and class on one of them
    trained  background 6 below the threshold's logit, 300 hot anchors around it: all in the last chunk (even frames), spread (odd frames)
    crowd    more than 1024 anchors above the threshold inside ONE chunk, about 200 in every other chunk
    empty    no candidate        level    every anchor on one value above the threshold"""
    lt = thr_logit(thr)
    chunk = _chunk_len(n)
    frames = []
    for f in range(b):
        g = torch.Generator().manual_seed(seed + 1000 * f)
        if pattern == "tie":
            levels = torch.tensor([lt - 1.0, lt - 0.5, lt - 0.25, lt + 0.25, lt + 0.5])   # thr = 0.3: all negative (keys of negative logits)
            x = levels[torch.randint(0, 5, (n, nc), generator=g)]
        elif pattern == "level":
            x = torch.full((n, nc), lt + 0.75)
        else:
            x = torch.rand(n, nc, generator=g) + (lt - 6.0)
            if pattern == "trained":
                start = ((n - 1) // chunk) * chunk if f % 2 == 0 else 0
                hot = torch.randperm(n - start, generator=g)[:300] + start
                cols = torch.randint(0, nc, (hot.numel(),), generator=g)
                vals = lt + 0.3 + torch.randn(hot.numel(), generator=g) * 0.5
                vals[0] = lt + 1.0                                   # at least one candidate, also when the last chunk holds one anchor
                x[hot, cols] = vals
            elif pattern == "crowd":
                chunks = -(-n // chunk)
                big = (chunks // 2 + f) % chunks
                for c in range(chunks):
                    lo, hi = c * chunk, min(n, (c + 1) * chunk)
                    m = min(hi - lo, 1500 if c == big else 200)
                    hot = torch.randperm(hi - lo, generator=g)[:m] + lo
                    cols = torch.randint(0, nc, (m,), generator=g)
                    x[hot, cols] = lt + 0.5 + torch.rand(m, generator=g) * 4.0
            else:
                assert pattern == "empty", pattern
        frames.append(x)
    return redraw_band(torch.stack(frames).to(dtype), thr)


BOUNDARY_N = [1, 2, 999, 1000, 1001, 8191, 8192, 8193, 16385, 81920, 81921, 163840, 163841, 327680, 327681, 589824, 589825]
BOUNDARY_N_FP32 = [1, 2, 999, 1000, 1001, 8191, 8192, 8193, 16385, 70401]
BOUNDARY_N_HUGE = [5308416, 5308417]
PATTERNS = ["tie", "trained", "crowd"]


def boundary_cases():
    """(dtype, n, nc, batch) of the form-boundary test, in the order the GPU test runs them."""
    out = []
    for dtype in (torch.bfloat16, torch.float16):
        out += [(dtype, n, nc, 2) for n in BOUNDARY_N for nc in (1, 3)]
        out += [(dtype, n, 1, 1) for n in BOUNDARY_N_HUGE]
    out += [(torch.float32, n, nc, 2) for n in BOUNDARY_N_FP32 for nc in (1, 3)]
    return out


def k_thr_logits(n, thr, dtype, seed):
    """[4, n, 1]: two hot frames (different seeds; for thr = 0.5 with exact +0.0 and -0.0 among the hot logits), a frame without a
    candidate (for thr = 0 every anchor is one), a frame with every anchor on one value."""
    lt = thr_logit(thr)
    frames = []
    for f in range(2):
        g = torch.Generator().manual_seed(seed + 1000 * f)
        x = torch.rand(n, 1, generator=g) + (lt - 6.0)
        hot = torch.randperm(n, generator=g)[:700]
        x[hot, 0] = lt + 0.2 + torch.randn(700, generator=g) * 0.5
        if thr == 0.5:
            x[hot[:40:2], 0] = 0.0
            x[hot[1:40:2], 0] = -0.0
        frames.append(x)
    frames.append(make_logits("empty", 1, n, 1, thr, torch.float32, seed + 7)[0])
    frames.append(make_logits("level", 1, n, 1, thr, torch.float32, seed + 8)[0])
    return redraw_band(torch.stack(frames).to(dtype), thr)


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_reference64(e, anchors):
    """second_box_decode (box_torch_ops.py:56-101) in float64 on the fp32 values of e [..., 7] and anchors [..., 7] = (x, y, z, w, l, h, r)."""
    e, a = e.double(), anchors.double()
    xa, ya, za, wa, la, ha, ra = a.unbind(-1)
    xt, yt, zt, wt, lt, ht, rt = e.unbind(-1)
    diag = torch.sqrt(la * la + wa * wa)
    return torch.stack([xt * diag + xa, yt * diag + ya, zt * ha + za, torch.exp(wt) * wa, torch.exp(lt) * la, torch.exp(ht) * ha, rt + ra], -1)


def decode_bounds(e, anchors, ref):
    """Per-output |device - ref| bound of the fp32 decode kernel.
    o0, o1, o2   2^-23 (|e s| + |ref|): one rounding for s (diag: sqrtf of a rounded sum of rounded squares, folded into the first term),
                 one for the product, one for the sum
    o3, o4, o5   2^-22 |ref|: expf within 1 ulp (HIP device-math documentation), half an ulp for the product, doubled
    o6           2^-24 |ref|: one addition"""
    e, a = e.double(), anchors.double()
    diag = torch.sqrt(a[..., 4] * a[..., 4] + a[..., 3] * a[..., 3])
    es = torch.stack([e[..., 0] * diag, e[..., 1] * diag, e[..., 2] * a[..., 5]], -1).abs()
    r = ref.abs()
    return torch.cat([2.0 ** -23 * (es + r[..., :3]), 2.0 ** -22 * r[..., 3:6], 2.0 ** -24 * r[..., 6:7]], -1)


def standup_reference64(dec):
    """(rows [..., 4] = x1, y1, x2, y2 in float64, bound [..., 4]) of the axis-aligned NMS input from the device's own decoded fp32 rows.
    Bound 2^-21 (|centre| + (|o3| + |o4|) / 2), the centre being o0 for the x rows and o1 for the y rows: sinf / cosf within 2 ulp as
    documented, two products and two sums."""
    o = dec.double()
    hx, hy = o[..., 3] * 0.5, o[..., 4] * 0.5
    cs, sn = torch.cos(o[..., 6]).abs(), torch.sin(o[..., 6]).abs()
    ex, ey = hx * cs + hy * sn, hx * sn + hy * cs
    rows = torch.stack([o[..., 0] - ex, o[..., 1] - ey, o[..., 0] + ex, o[..., 1] + ey], -1)
    half = (o[..., 3].abs() + o[..., 4].abs()) * 0.5
    bx, by = 2.0 ** -21 * (o[..., 0].abs() + half), 2.0 ** -21 * (o[..., 1].abs() + half)
    return rows, torch.stack([bx, by, bx, by], -1)


def direction_reference(d):
    """First bin attaining the maximum of the direction logits d [..., bins]."""
    return first_max(d.float())[1]


def within(got, ref, bound):
    """|got - ref| <= bound elementwise, NaN matching NaN.  -> (ok, largest |got - ref| / bound over the finite entries with bound > 0)."""
    got, ref = got.double(), ref.double()
    both_nan = torch.isnan(got) & torch.isnan(ref)
    err = (got - ref).abs()
    ok = both_nan | (err <= bound)
    fin = torch.isfinite(err) & (bound > 0)
    ratio = float((err[fin] / bound[fin]).max()) if bool(fin.any()) else 0.0
    return bool(ok.all()), ratio


# ---------------------------------------------------------------------------------------------------------------- finalize
def limit_period_f32(val, offset, period):
    """box_torch_ops.limit_period in float32, one operation per line (div, add, floor, mul, sub)."""
    val, offset, period = np.asarray(val, np.float32), np.float32(offset), np.float32(period)
    q = val / period
    q = q + offset
    fl = np.floor(q)
    m = fl * period
    return val - m


def limit_period_quotient(o6, dir_offset, dir_limit_offset, bins):
    """val / period + limit_offset as finalize computes it (float32): the tests construct rotations around its integer values."""
    period = np.float32(6.283185307179586) / np.float32(bins)
    val = np.asarray(o6, np.float32) - np.float32(dir_offset)
    q = val / period
    return q + np.float32(dir_limit_offset)


def finalize_reference32(dec, top_score, top_label, dir_label, keep, num_keep, post_max, use_direction, dir_offset, dir_limit_offset,
                         bins, range6):
    """k_predict_finalize restated in numpy float32 (every operation an IEEE basic operation or floorf; the build uses -ffp-contract=off):
    dec [B, K, 7] f32, top_score / top_label / dir_label [B, K], keep [B, K] int, num_keep [B], range6 6 floats or None.
    -> dict(boxes [B, P, 7] f32, scores [B, P] f32, labels [B, P] i32, valid [B, P] bool), P = min(post_max, K)."""
    dec = np.asarray(dec, np.float32)
    b, k, _ = dec.shape
    p = min(int(post_max), k)
    j = np.arange(p)[None, :]
    ok = j < np.asarray(num_keep).reshape(b, 1)
    sel = np.where(ok, np.asarray(keep)[:, :p], 0).astype(np.int64)
    rows = np.arange(b)[:, None]
    o = dec[rows, sel].copy()
    if use_direction:
        period = np.float32(6.283185307179586) / np.float32(bins)
        off, lim = np.float32(dir_offset), np.float32(dir_limit_offset)
        val = o[..., 6] - off
        q = val / period
        q = q + lim
        fl = np.floor(q)
        m = fl * period
        rot = val - m
        r2 = rot + off
        dl = period * np.asarray(dir_label)[rows, sel].astype(np.float32)
        o[..., 6] = r2 + dl
    if range6 is not None:
        r = np.asarray(range6, np.float32)
        with np.errstate(invalid="ignore"):
            ok = ok & (o[..., 0] >= r[0]) & (o[..., 1] >= r[1]) & (o[..., 2] >= r[2]) & (o[..., 0] <= r[3]) & (o[..., 1] <= r[4]) & (o[..., 2] <= r[5])
    return {"boxes": o, "scores": np.asarray(top_score, np.float32)[rows, sel], "labels": np.asarray(top_label)[rows, sel].astype(np.int32),
            "valid": ok}


def same_bits_f32(a, b):
    """float32 arrays equal bit for bit, any NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
