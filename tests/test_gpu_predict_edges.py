"""-m gpu: the predict chain (csrc/predict.hip: select -> decode -> finalize) against exact references at the boundaries of every select
form, on ties, thresholds, segments, lazy / cover / masked addressing, NaN and infinities, and at the edges of decode and finalize.

References: tests/predict_ref_helpers.py (torch / numpy only, float64 or bit-exact float32; pinned to the executed reference's recorded
outputs and to planted mistakes by tests/test_predict_ref_host.py).  Inputs are generated on the CPU by the helpers' seeded generators --
the host test checks the very same inputs for the threshold band -- and copied to the device.

Bounds (derived in the helpers, none taken from a measurement):
  top_score            relative 2^-21 of the float64 sigmoid
  decode o0..o2        2^-23 (|e s| + |ref|)       o3..o5  relative 2^-22       o6  relative 2^-24
  standup rows         2^-21 (|centre| + (|o3| + |o4|) / 2)
  finalize             bit equality with the float32 restatement
  indices, labels, counts, valid: equality.
Measured on an MI355X (largest error / bound over every case of this file; each test prints its own with -s): top_score 0.25 (1.2e-7
relative, one ulp of the result), decode o0..o2 0.83, o3..o5 0.51, o6 1.00 (one correctly rounded addition), standup rows 0.23.

Two defects these cases exposed are fixed in csrc/predict.hip: a NaN maximum sorted to row 0 uncounted and pushed a detection out of
rows [0, counts) (test_select_with_nan_and_infinite_logits); the two-pass radix select of bf16 heads above 5 308 416 anchors kept
arbitrary ties when the k-th logit was negative (test_select_at_the_form_boundaries[bfloat16-N5308417-nc1]).
"""
import math

import numpy as np
import pytest
import torch

import predict_ref_helpers as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
MEASURED = {}          # name -> largest error / bound seen in this process


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


def _note(name, value):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(value))
    print(f"[predict-edges] {name}: {value:.4g} (largest so far {MEASURED[name]:.4g})")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _select_twice(ops, cls, k, thr, ref, **kw):
    """ops.predict_select on ``cls`` (a view or a list of views), twice: both runs against ``ref``; rows up to counts identical."""
    got = ops.predict_select(cls, k, thr, **kw)
    again = ops.predict_select(cls, k, thr, **kw)
    assert ref["margin"] >= R.BAND, ref["margin"]
    worst = R.check_selection(got, ref)
    assert torch.equal(got[3], again[3])
    for f in range(got[3].shape[0]):
        c = int(got[3][f])
        assert all(torch.equal(_bits(g[f, :c]), _bits(a[f, :c])) for g, a in zip(got[:3], again[:3])), f"frame {f}: the second run differs"
    _note("score rel err / 2^-21", worst / R.SCORE_RTOL)
    return got


def _check_logits(ops, x, ahw, k, thr):
    """x [B, N, C] on the CPU -> the [B, A, H, W, C] head on the device, selected and compared."""
    b, n, nc = x.shape
    a, h, w = ahw
    assert a * h * w == n
    cls = x.cuda().reshape(b, a, h, w, nc)
    ref = R.select_reference(cls, k, thr)
    got = _select_twice(ops, cls, k, thr, ref)
    assert got[0].shape[1] == min(k, n, 1024)
    return got, ref


# ---------------------------------------------------------------------------------------------------------------- 1. form boundaries
_BOUNDARY = [(i, c) for i, c in enumerate(R.boundary_cases())]


@pytest.mark.parametrize("i,case", _BOUNDARY, ids=[f"{str(c[0]).split('.')[-1]}-N{c[1]}-nc{c[2]}" for _, c in _BOUNDARY])
def test_select_at_the_form_boundaries(ops, i, case):
    """N on both sides of every edge of predict_select_launch's decision (select_form(); the host test pins the list to the table):
    direct / 8192-anchor chunks with the KP2 = 5, 10, 20, 36 second stage / 73 728-anchor chunks / the two 32-bit forms for 16-bit
    heads above 5 308 416 anchors / the fp32 radix select; odd N, a last chunk of one anchor, W not a power of two."""
    dtype, n, nc, b = case
    k, thr = 1000, 0.3
    form = R.select_form(n, dtype)
    assert ops.predict_select_plan(n, dtype) == form
    seen = 0
    for p, pattern in enumerate(R.PATTERNS):
        x = R.make_logits(pattern, b, n, nc, thr, dtype, 100 * i + p)
        got, ref = _check_logits(ops, x, R.factor_ahw(n), k, thr)
        seen = max(seen, int(ref["counts"].max()))
        if pattern == "crowd" and n >= 1500:
            assert int(ref["counts"].max()) == k                     # more than k candidates: bisection / radix, not the shortcut
        if pattern == "trained" and n >= 1000:
            assert 0 < int(ref["counts"].min()) <= int(ref["counts"].max()) < k, ref["counts"]    # the threshold shortcut's case
    assert seen > 0 or n < 3
    print(f"[predict-edges] form {form[0]} (chunks {form[1]}) ran at N = {n}, {dtype}, nc = {nc}")


# ---------------------------------------------------------------------------------------------------------------- 2. k and threshold
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n", [8193, 1001])
@pytest.mark.parametrize("thr", [0.0, 0.05, 0.5, 0.9])
def test_select_k_and_threshold(ops, thr, n, dtype):
    """k = 1, 7, 64, 1023, 1024 against thresholds 0 (counts == min(k, N): no logit is below it), 0.05, 0.5 (exact +0.0 and -0.0 among
    the hot logits: both score exactly 0.5, both count, every +0.0 ranks before every -0.0) and 0.9; a frame without a candidate and a
    frame with every anchor on one value."""
    x = R.k_thr_logits(n, thr, dtype, 17)
    for k in (1, 7, 64, 1023, 1024):
        got, ref = _check_logits(ops, x, R.factor_ahw(n), k, thr)
        kk = min(k, n)
        if thr == 0.0:
            assert got[3].tolist() == [kk] * 4
        else:
            assert int(ref["counts"][2]) == 0 and int(ref["counts"][3]) == kk
            assert ref["idx"][3].tolist() == list(range(kk))                      # all tied: ascending anchor index
    if thr == 0.5:
        ref = R.select_reference(x.cuda(), 1024, thr)
        for f in range(2):
            v = x[f, ref["idx"][f].cpu(), 0].float()
            zero = (v == 0).nonzero().squeeze(1)
            assert zero.numel() == 40 and int(zero[-1]) == int(ref["counts"][f]) - 1, "the +-0.0 logits are the last counted rows"
            sign = torch.signbit(v[zero])
            assert not bool(sign[:20].any()) and bool(sign[20:].all()), "every +0.0 before every -0.0"


# ---------------------------------------------------------------------------------------------------------------- 3. ties in fp32
@pytest.mark.parametrize("ahw", [(2, 37, 29), (2, 100, 88)])
@pytest.mark.parametrize("levels,k", [(1, 1000), (3, 1000), (40, 1000), (700, 1000)])
def test_select_tie_ranking_fp32(ops, levels, k, ahw):
    """test_predict_select_tie_ranking's levels for fp32 heads (the 32-bit radix select's ordered tie ranking across its 1024-key rounds
    and inside its last histogram bin), at a one-block and a multi-round size."""
    a, h, w = ahw
    n, b, thr = a * h * w, 2, 0.3
    g = torch.Generator().manual_seed(levels)
    vals = R.redraw_band(torch.randn(levels, generator=g) * 2.0 - 1.0, thr)
    x = vals[torch.randint(0, levels, (b, n, 1), generator=g)]
    _check_logits(ops, x, ahw, k, thr)


# ---------------------------------------------------------------------------------------------------------------- 4. class ties, strides
def _packed_views(x, box, dirs, ahw, pad_to=1):
    """cls / box / dir [B, A, H, W, code] views into ONE channels-last head tensor [B, A * (7 + nc + 2) (+ padding), H, W], as the RPN hands
    them out (test_fused_predict_matches_torch_formulation): non-contiguous, channel stride H * W-free, anchor stride = code."""
    b, n, nc = x.shape
    a, h, w = ahw
    parts = [t.reshape(b, a, h, w, c).permute(0, 1, 4, 2, 3).reshape(b, a * c, h, w) for t, c in ((box, 7), (x, nc), (dirs, 2))]
    packed = torch.cat(parts, 1)
    tot = packed.shape[1]
    if tot % pad_to:
        packed = torch.cat([packed, torch.zeros(b, pad_to - tot % pad_to, h, w, dtype=x.dtype, device=x.device)], 1)
    packed = packed.contiguous(memory_format=torch.channels_last)
    c0, views = 0, {}
    for name, code in (("box", 7), ("cls", nc), ("dir", 2)):
        views[name] = packed[:, c0:c0 + a * code].reshape(b, a, code, h, w).permute(0, 1, 3, 4, 2)
        c0 += a * code
    assert torch.equal(views["cls"].reshape(b, n, nc), x)
    return views


def _random_box_dir(b, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, n, 7, generator=g) * 0.2).to(dtype), torch.randn(b, n, 2, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("ahw", [(3, 37, 73), (20, 13, 37)])
@pytest.mark.parametrize("nc", [2, 10])
def test_select_class_ties_on_a_packed_channels_last_head(ops, nc, ahw, dtype):
    """Equal maxima in two classes (the first wins), the head a strided view of the packed channels-last tensor; N = 8 103 takes the
    direct form, N = 9 620 the chunk form."""
    a, h, w = ahw
    n, b, thr = a * h * w, 2, 0.3
    box, dirs = _random_box_dir(b, n, dtype, 5)
    for p, pattern in enumerate(("tie", "trained")):
        x = R.make_logits(pattern, b, n, nc, thr, dtype, 40 + p)
        g = torch.Generator().manual_seed(p)
        rows = torch.randperm(n, generator=g)[:200]
        lo, hi = sorted(torch.randperm(nc, generator=g)[:2].tolist())
        x[:, rows, :] = torch.tensor(-8.0).to(dtype)
        x[:, rows, lo] = x[:, rows, hi] = torch.tensor(1.25).to(dtype)            # two classes share the maximum
        views = _packed_views(x.cuda(), box.cuda(), dirs.cuda(), ahw)
        assert not views["cls"].is_contiguous()
        ref = R.select_reference(views["cls"], 1000, thr)
        got = _select_twice(ops, views["cls"], 1000, thr, ref)
        for f in range(b):
            c = int(got[3][f])
            picked = torch.isin(got[0][f, :c].long().cpu(), rows)
            assert int(picked.sum()) >= 100 and bool((got[2][f, :c].cpu()[picked] == lo).all())
        contiguous = ops.predict_select(views["cls"].contiguous(), 1000, thr)
        assert _same(got, contiguous)


# ---------------------------------------------------------------------------------------------------------------- decode comparison
def _check_decode(e, anchors, dirs, top_idx, top_score, dec, dets, dlab, rotate, rows=None):
    """dec / dets / dlab [B, K, ...] of the rows top_idx [B, K] (``rows`` [B]: how many of them to compare; all by default) against
    decode_reference64, standup_reference64 and direction_reference on e [B, N, 7], anchors [N, 7], dirs [B, N, bins] or None."""
    b, k = top_idx.shape
    for f in range(b):
        c = k if rows is None else int(rows[f])
        idx = top_idx[f, :c].long()
        ef, af = e[f, idx].float(), anchors[idx]
        ref = R.decode_reference64(ef, af)
        ok, ratio = R.within(dec[f, :c], ref, R.decode_bounds(ef, af, ref))
        for col, name in ((slice(0, 3), "decode o0..o2 err / bound"), (slice(3, 6), "decode o3..o5 err / bound"), (slice(6, 7), "decode o6 err / bound")):
            _note(name, R.within(dec[f, :c, col], ref[:, col], R.decode_bounds(ef, af, ref)[:, col])[1])
        assert ok, (f, ratio)
        if rotate:
            want = torch.cat([dec[f, :c][:, [0, 1, 3, 4, 6]], top_score[f, :c, None]], 1)
            assert torch.equal(_bits(dets[f, :c].contiguous()), _bits(want.contiguous())) or \
                bool(((dets[f, :c] == want) | (torch.isnan(dets[f, :c]) & torch.isnan(want))).all())
        else:
            rows64, bound = R.standup_reference64(dec[f, :c])
            ok, ratio = R.within(dets[f, :c, :4], rows64, bound)
            _note("standup err / bound", ratio)
            assert ok, (f, ratio)
            assert torch.equal(dets[f, :c, 4], top_score[f, :c]) and bool((dets[f, :c, 5] == 0).all())
        want_dir = R.direction_reference(dirs[f, idx]) if dirs is not None else torch.zeros(c, dtype=torch.long, device=dec.device)
        assert torch.equal(dlab[f, :c].long(), want_dir), f


# ---------------------------------------------------------------------------------------------------------------- 5. segments
SEGMENT_LISTS = [[(3, 37, 73), (5, 11, 13), (1, 1, 1)],
                 [(3, 37, 73), (1, 1, 1), (5, 11, 13), (7, 9, 5)],
                 [(1, 1, 1), (3, 37, 73)],
                 [(1, 1, 8191), (1, 1, 1), (1, 1, 3)]]


def _segment_views(x, box, dirs, maps):
    """Per map the packed, channel-padded channels-last head tensor holding its slice of the global anchor list."""
    out, start = [], 0
    for a, h, w in maps:
        m = a * h * w
        out.append(_packed_views(x[:, start:start + m].contiguous(), box[:, start:start + m].contiguous(), dirs[:, start:start + m].contiguous(),
                                 (a, h, w), pad_to=16))
        start += m
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("maps", SEGMENT_LISTS, ids=lambda m: "+".join("x".join(map(str, s)) for s in m))
def test_select_and_decode_over_three_and_four_segments(ops, maps, nc, dtype):
    """seg_pick with s = 2 and 3, odd segment sizes with a total above 8 192 (the chunk kernel's pair-straddles-a-border branch), a
    border one anchor into a chunk and one anchor before its end; ties across every border rank by global index."""
    n = sum(a * h * w for a, h, w in maps)
    b, k, thr = 2, 1000, 0.3
    assert ops.predict_select_plan(n, dtype) == R.select_form(n, dtype)          # the segments select decides on the summed anchor count
    starts = np.cumsum([a * h * w for a, h, w in maps])[:-1].tolist()
    box, dirs = _random_box_dir(b, n, dtype, 6)
    g = torch.Generator().manual_seed(8)
    anchors = torch.cat([torch.rand(n, 3, generator=g) * 40, torch.rand(n, 3, generator=g) * 3 + 0.5, torch.rand(n, 1, generator=g) * 3], 1).cuda()
    for p, pattern in enumerate(("tie", "trained", "border")):
        x = R.make_logits("trained" if pattern == "border" else pattern, b, n, nc, thr, dtype, 60 + p)
        if pattern == "border":
            for s in starts:                                # the last anchor of a segment and the first of the next: equal logits
                x[:, s - 1, :] = x[:, s, :] = torch.tensor(2.5).to(dtype)
        views = _segment_views(x.cuda(), box.cuda(), dirs.cuda(), maps)
        cls = [v["cls"] for v in views]
        ref = R.select_reference(cls, k, thr)
        got = _select_twice(ops, cls, k, thr, ref)
        if pattern == "border":
            for f in range(b):
                top = sorted({i for s in starts for i in (s - 1, s)})
                assert got[0][f, :len(top)].tolist() == top
        for rotate in (True, False):
            dec, dets, dlab = ops.predict_decode([v["box"] for v in views], [v["dir"] for v in views], anchors, got[0], got[1], rotate=rotate)
            _check_decode(box.cuda(), anchors, dirs.cuda(), got[0], got[1], dec, dets, dlab, rotate, rows=got[3])


# ---------------------------------------------------------------------------------------------------------------- 6. lazy / cover / mask
def _ragged_lazy_inputs(form, ahw, dtype, b=2, nc=3, thr=0.3):
    """A lazily written head on a map ragged against the tile grid / the cover words: the written-tile table (``form`` "tiles") or cover
    words ("cover"), the pixel mask they stand for, and per head tensor ("cls", "box", "dir") the triple (the head with junk in its
    unwritten elements, the background map, where(written, head, background)), all on the device; anchors; the generator, for more draws."""
    a, h, w = ahw
    n = a * h * w
    g = torch.Generator().manual_seed(21)
    x = R.make_logits("trained", b, n, nc, thr, dtype, 70).reshape(b, a, h, w, nc)
    bg = R.redraw_band((torch.randn(1, a, h, w, nc, generator=g) * 0.8 - 2.5).to(dtype), thr)       # a few percent of the background anchors pass 0.3
    box, dirs = _random_box_dir(b, n, dtype, 7)
    bgbox, bgdir = _random_box_dir(1, n, dtype, 9)
    anchors = (torch.rand(n, 7, generator=g) + 0.5).cuda()
    if form == "tiles":
        ty, tx = (h + 7) // 8, (w + 15) // 16
        live = torch.rand(b, ty * tx, generator=g) < 0.6
        written = live.reshape(b, ty, 1, tx, 1).expand(b, ty, 8, tx, 16).reshape(b, ty * 8, tx * 16)[:, :h, :w]
        table = (live.to(torch.int16) << 4).contiguous().cuda()
    else:
        bands, words = (h + 7) // 8, (w + 31) // 32
        cover = torch.randint(-2 ** 31, 2 ** 31, (b, bands, words), generator=g, dtype=torch.int64)
        ys, xs = torch.arange(h), torch.arange(w)
        written = ((cover[:, ys // 8][:, :, xs // 32] >> (xs % 32)) & 1).bool()
        table = cover.to(torch.int32).contiguous().cuda()
    assert 0.2 < written.float().mean() < 0.8
    wr = written.reshape(b, 1, h, w, 1)
    heads = {}
    for name, t, back, code, junk in (("cls", x, bg, nc, 30.0), ("box", box, bgbox, 7, 5.0), ("dir", dirs, bgdir, 2, 9.0)):
        t, back = t.reshape(b, a, h, w, code), back.reshape(1, a, h, w, code)
        heads[name] = (torch.where(wr, t, torch.full_like(t, junk)).contiguous().cuda(),         # unwritten elements hold junk
                       back.contiguous().cuda(), torch.where(wr, t, back.expand(b, -1, -1, -1, -1)).contiguous().cuda())
    return table, written, heads, anchors, g


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("ahw", [(20, 13, 37), (2, 13, 37)])
@pytest.mark.parametrize("form", ["tiles", "cover"])
def test_lazy_cover_and_masked_addressing_on_ragged_maps(ops, form, ahw, dtype):
    """Written-tile bits (8 x 16 grid) / cover words (8-row bands, 32-column words) on a map ragged against both, a background map with
    scores above the threshold, an anchor mask on top: select and decode equal the plain entry points on where(written, head, background)
    bit for bit, and the reference (with mask=) entry for entry.  (20, 13, 37) takes the chunk form, (2, 13, 37) the direct one."""
    a, h, w = ahw
    n, b, nc, k, thr = a * h * w, 2, 3, 1000, 0.3
    table, written, heads, anchors, g = _ragged_lazy_inputs(form, ahw, dtype, b, nc, thr)
    holes, bgc, full = heads["cls"]
    ref = R.select_reference(full, k, thr)
    got = _select_twice(ops, holes, k, thr, ref, lazy=(table, bgc))
    plain = ops.predict_select(full, k, thr)
    assert _same(got, plain) and int(ref["counts"].min()) > 0
    on_bg = [int((~written.reshape(b, -1)[f][(ref["idx"][f].cpu() % (h * w))]).sum()) for f in range(b)]
    assert min(on_bg) > 0, "the selection must include anchors read from the background map"
    for rotate in (True, False):
        lz = ops.predict_decode(heads["box"][0], heads["dir"][0], anchors, got[0], got[1], rotate=rotate, lazy=(table, (heads["box"][1], heads["dir"][1])))
        pl = ops.predict_decode(heads["box"][2], heads["dir"][2], anchors, got[0], got[1], rotate=rotate)
        assert _same(lz, pl)
        _check_decode(heads["box"][2].reshape(b, n, 7), anchors, heads["dir"][2].reshape(b, n, 2), got[0], got[1], *lz, rotate, rows=got[3])
    mask = torch.rand(b, n, generator=g) < 0.5
    for f in range(b):
        mask[f, ref["idx"][f].cpu()[::2]] = False                                      # half of the unmasked selection is masked out
    mask = mask.cuda()
    refm = R.select_reference(full, k, thr, mask=mask)
    gotm = _select_twice(ops, holes, k, thr, refm, lazy=(table, bgc), anchor_mask=mask)
    assert _same(gotm, ops.predict_select(full, k, thr, anchor_mask=mask)) and 0 < int(refm["counts"].max()) < int(ref["counts"].max())
    none = torch.zeros_like(mask)
    for cls_, kw in ((holes, {"lazy": (table, bgc)}), (full, {})):
        assert ops.predict_select(cls_, k, thr, anchor_mask=none, **kw)[3].tolist() == [0] * b


def _select_through(entry, cls, k, thr, tail=()):
    """sec_predict_select / sec_predict_select_lazy through ctypes (ops.predict_select itself calls sec_predict_select_masked), with the
    allocations of ops.predict_select; ``tail`` = the tensors the entry point takes between the dtype and the stream."""
    import ctypes
    from second_amd import runtime as rt
    b, a, h, w, nc = cls.shape
    k = min(k, a * h * w, 1024)
    out = (torch.empty((b, k), dtype=torch.int32, device=cls.device), torch.empty((b, k), dtype=torch.float32, device=cls.device),
           torch.empty((b, k), dtype=torch.int32, device=cls.device), torch.empty((b,), dtype=torch.int32, device=cls.device))
    keys = torch.empty((b * a * h * w,), dtype=torch.int32, device=cls.device)
    rc = getattr(rt.lib(), entry)(rt.ptr(cls), (ctypes.c_int64 * 5)(*cls.stride()), b, a, h, w, nc, k, float(thr), rt.ptr(keys),
                                  *[rt.ptr(t) for t in out], rt.dtype_code(cls.dtype), *[rt.ptr(t) for t in tail], rt.stream())
    assert rc == 0, (entry, rc)
    return out


def _same_up_to_counts(got, want):
    assert torch.equal(got[3], want[3]) and int(want[3].max()) > 0
    for f in range(want[3].shape[0]):
        c = int(want[3][f])
        assert all(torch.equal(_bits(g[f, :c]), _bits(w[f, :c])) for g, w in zip(got[:3], want[:3])), f"frame {f}"


@pytest.mark.parametrize("dtype,ahw,nc,form", [(torch.bfloat16, (2, 13, 37), 3, "direct"), (torch.float32, (2, 13, 37), 3, "radix32"),
                                               (torch.bfloat16, (3, 1, 2731), 1, "chunk4+kp5")],
                         ids=["bf16-direct", "fp32-radix32", "bf16-chunked"])
def test_the_eager_and_lazy_entry_points_equal_the_masked_route(ops, dtype, ahw, nc, form):
    """ops.predict_select reaches every head form but the cover one through sec_predict_select_masked; sec_predict_select and
    sec_predict_select_lazy stay in the C API for callers without a mask.  Both, through ctypes, give ops.predict_select's four
    outputs bit for bit up to counts: a [2, 2, 13, 37, 3] head (direct / radix32) and an 8193-anchor one (chunked); the lazy entry
    point on the ragged tile table and background of test_lazy_cover_and_masked_addressing_on_ragged_maps."""
    a, h, w = ahw
    n, b, k, thr = a * h * w, 2, 1000, 0.3
    assert ops.predict_select_plan(n, dtype) == R.select_form(n, dtype) and R.select_form(n, dtype)[0] == form
    cls = R.make_logits("trained", b, n, nc, thr, dtype, 90).cuda().reshape(b, a, h, w, nc)
    _same_up_to_counts(_select_through("sec_predict_select", cls, k, thr), ops.predict_select(cls, k, thr))
    lazy_ahw = (20, 13, 37) if form.startswith("chunk") else (2, 13, 37)
    assert ops.predict_select_plan(lazy_ahw[0] * 13 * 37, dtype)[0] == form
    table, _, heads, _, _ = _ragged_lazy_inputs("tiles", lazy_ahw, dtype)
    holes, bgc, full = heads["cls"]
    want = ops.predict_select(holes, k, thr, lazy=(table, bgc))
    _same_up_to_counts(_select_through("sec_predict_select_lazy", holes, k, thr, tail=(table, bgc)), want)
    _same_up_to_counts(_select_through("sec_predict_select", full, k, thr), want)


# ---------------------------------------------------------------------------------------------------------------- 7. NaN and infinities
def _nan(dtype, negative):
    """A quiet NaN of ``dtype`` with the given sign bit, built from its bits (conversions canonicalise the sign away)."""
    if dtype == torch.float32:
        return torch.tensor([0xFFC00000 - 2 ** 32 if negative else 0x7FC00000], dtype=torch.int32).view(torch.float32)[0]
    quiet = 0x7FC0 if dtype == torch.bfloat16 else 0x7E00
    return torch.tensor([quiet + 0x8000 - 2 ** 16 if negative else quiet], dtype=torch.int16).view(dtype)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n", [1001, 8193])
@pytest.mark.parametrize("nc", [1, 3])
def test_select_with_nan_and_infinite_logits(ops, nc, n, dtype):
    """+inf scores 1.0 and ranks first, -inf scores 0; an anchor whose maximum over classes is NaN (either sign; in class 0, and for three
    classes in class 2 alone -- torch.max propagates it and `>= thresh` drops the anchor, voxelnet.py:558-562) never appears in rows
    [0, counts): counts and the rows are those of the NaN-free anchors.  k = 7: a NaN ranked first would push a detection out."""
    thr, b = 0.3, 2
    x = R.make_logits("trained", b, n, nc, thr, dtype, 80)
    g = torch.Generator().manual_seed(n + nc)
    spots = torch.randperm(n, generator=g)[:40]
    x[:, spots[0:3], 0] = math.inf
    x[:, spots[3:6], :] = -math.inf
    x[0, spots[6:10], 0] = _nan(dtype, False)
    x[1, spots[10:14], 0] = _nan(dtype, True)
    x[:, spots[6:14], 1:] = torch.tensor(4.0).to(dtype)                       # a finite, passing logit next to the NaN: still dropped
    if nc == 3:
        x[0, spots[14:18], 2] = _nan(dtype, True)
        x[1, spots[18:22], 2] = _nan(dtype, False)
        x[:, spots[14:22], 0] = torch.tensor(4.0).to(dtype)
    x[:, spots[24:40], 0] = torch.linspace(0.5, 2.0, 16).to(dtype)            # sixteen finite candidates in every frame
    signs = torch.signbit(x[torch.isnan(x)].float())
    assert bool(signs.any()) and not bool(signs.all()), "NaN of both signs"
    bad = torch.isnan(x.float()).any(-1)
    for k in (7, 1000):
        got, ref = _check_logits(ops, x, R.factor_ahw(n), k, thr)
        for f in range(b):
            c = int(got[3][f])
            assert c >= min(k, 19) and not bool(bad[f, got[0][f, :c].long().cpu()].any())
            assert got[0][f, :3].sort().values.tolist() == spots[0:3].sort().values.tolist() and got[1][f, :3].tolist() == [1.0] * 3


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_select_classes_drops_nan_columns(ops, dtype):
    """The (frame, class) select scores one column at a time: a NaN there fails its threshold and is no candidate, whatever the other
    columns hold; every item equals select_reference on its one-class column."""
    ahw, nc, b, k, thr = (4, 13, 37), 3, 2, 200, 0.3
    n = ahw[0] * ahw[1] * ahw[2]
    x = R.make_logits("trained", b, n, nc, thr, dtype, 90)
    x[:, 5:900:7, 1] = _nan(dtype, False)
    x[:, 6:900:7, 2] = _nan(dtype, True)
    cls = x.cuda().reshape(b, *ahw, nc)
    top_idx, top_score, counts = ops.predict_select_classes(cls, [(0, ahw[0])] * nc, [k] * nc, [thr] * nc)
    for c in range(nc):
        ref = R.select_reference(cls[..., c:c + 1], k, thr)
        assert ref["margin"] >= R.BAND
        R.check_selection((top_idx[:, c], top_score[:, c], torch.zeros_like(top_idx[:, c]), counts[:, c]), ref)


# ---------------------------------------------------------------------------------------------------------------- decode edges
def _decode_inputs(dtype, with_nan=True):
    a, h, w, b, k = 2, 13, 37, 2, 64
    n = a * h * w
    g = torch.Generator().manual_seed(31)
    e = torch.cat([torch.randn(b, n, 3, generator=g) * 0.5, torch.rand(b, n, 3, generator=g) * 8 - 4, torch.rand(b, n, 1, generator=g) * 80 - 40], 2)
    anchors = torch.cat([torch.rand(n, 3, generator=g) * 40, torch.rand(n, 3, generator=g) * 3 + 0.5, torch.rand(n, 1, generator=g) * 3], 1)
    dirs = torch.randn(b, n, 2, generator=g)
    top_idx = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(b)]).to(torch.int32)
    sq, tied, nanrow = int(top_idx[0, 0]), int(top_idx[0, 1]), int(top_idx[1, 2])
    anchors[sq, 4] = anchors[sq, 3]                                   # an anchor with w == l
    dirs[:, tied, :] = 0.375                                          # direction logits tied: the first bin wins
    if with_nan:
        e[1, nanrow, :] = math.nan                                    # one NaN box row
    top_score = torch.rand(b, k, generator=g)
    return (a, h, w), e.to(dtype), anchors, dirs.to(dtype), top_idx, top_score, (1, 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("with_dir", [True, False])
def test_decode_against_float64_with_derived_bounds(ops, with_dir, rotate, dtype):
    """Size residuals in [-4, 4] (expf over its working range), angles in [-40, 40] (the standup rows' sinf / cosf far outside
    [-pi, pi]), an anchor with w == l, tied direction logits, a NaN box row (NaN out; finalize turns it into valid == 0)."""
    (a, h, w), e, anchors, dirs, top_idx, top_score, nan_at = _decode_inputs(dtype)
    b, n = e.shape[0], a * h * w
    box = e.cuda().reshape(b, a, h, w, 7)
    dd = dirs.cuda().reshape(b, a, h, w, 2) if with_dir else None
    anchors, top_idx, top_score = anchors.cuda(), top_idx.cuda(), top_score.cuda()
    dec, dets, dlab = ops.predict_decode(box, dd, anchors, top_idx, top_score, rotate=rotate)
    _check_decode(e.cuda(), anchors, dirs.cuda() if with_dir else None, top_idx, top_score, dec, dets, dlab, rotate)
    assert bool(torch.isnan(dec[nan_at]).all()) and int(torch.isnan(dec).sum()) == 7
    if with_dir:
        assert int(dlab[0, 1]) == 0
    # the NaN row through finalize: never valid, with or without the direction fix and the range test
    keep = torch.arange(64, dtype=torch.int32).repeat(b, 1).cuda()
    num_keep = torch.full((b,), 64, dtype=torch.int32).cuda()
    lab = torch.zeros(b, 64, dtype=torch.int32).cuda()
    r6 = torch.tensor([-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]).cuda()
    fin = ops.predict_finalize(dec, top_score, lab, dlab, keep, num_keep, 64, with_dir, 0.0, 1.0, 2, r6)
    assert not bool(fin["valid"][nan_at]) and int(fin["valid"].sum()) == b * 64 - 1


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_decode_classes_against_float64(ops, dtype):
    """The same bounds through ops.predict_decode_classes: [B, C, K] rows of (frame, class) items are one list of C * K rows per frame."""
    (a, h, w), e, anchors, dirs, top_idx, top_score, _ = _decode_inputs(dtype, with_nan=False)
    b, nc, k = e.shape[0], 4, 16
    box, dd = e.cuda().reshape(b, a, h, w, 7), dirs.cuda().reshape(b, a, h, w, 2)
    anchors = anchors.cuda()
    idx3, score3 = top_idx.cuda().reshape(b, nc, k).contiguous(), top_score.cuda().reshape(b, nc, k).contiguous()
    for rotate in (True, False):
        dec, dets, dlab = ops.predict_decode_classes(box, dd, anchors, idx3, score3, rotate=rotate)
        assert dec.shape == (b, nc, k, 7) and dets.shape == (b, nc, k, 6) and dlab.shape == (b, nc, k)
        _check_decode(e.cuda(), anchors, dirs.cuda(), idx3.reshape(b, -1), score3.reshape(b, -1), dec.reshape(b, -1, 7), dets.reshape(b, -1, 6),
                      dlab.reshape(b, -1), rotate)


# ---------------------------------------------------------------------------------------------------------------- finalize edges
RANGE6 = np.array([0.0, -40.0, -3.0, 70.4, 40.0, 1.0], np.float32)


def _finalize_table(dir_offset, dir_limit_offset, bins):
    """64 decoded rows: rotations whose quotient val / period + limit_offset is an integer, and one and two floats to either side of it
    (12 integers x 5); centres exactly on each face of RANGE6 (rows 0, 2, .., 10) and one float outside it (rows 1, 3, .., 11); row 12 NaN."""
    period = np.float32(6.283185307179586) / np.float32(bins)
    t = np.zeros((64, 7), np.float32)
    t[:, :3] = np.array([35.0, 0.5, -1.0], np.float32)
    t[:, 3:6] = np.array([1.6, 3.9, 1.5], np.float32)
    r = 0
    for m in range(-6, 6):
        mid = np.float32(np.float32(m) * period) + np.float32(dir_offset)
        for cand in [mid] + [np.nextafter(mid, np.float32(s * np.inf)) for s in (-1, 1)]:     # a float whose quotient IS the integer
            if R.limit_period_quotient(cand, dir_offset, dir_limit_offset, bins) == np.float32(m) + np.float32(dir_limit_offset):
                mid = cand
                break
        lo1 = np.nextafter(mid, np.float32(-np.inf)); lo2 = np.nextafter(lo1, np.float32(-np.inf))
        hi1 = np.nextafter(mid, np.float32(np.inf)); hi2 = np.nextafter(hi1, np.float32(np.inf))
        t[r:r + 5, 6] = [lo2, lo1, mid, hi1, hi2]
        r += 5
    t[60:, 6] = [0.0, 1e-30, 40.0, -40.0]
    for face in range(6):
        axis, sign = face % 3, (-1.0 if face < 3 else 1.0)
        t[2 * face, axis] = RANGE6[face]
        t[2 * face + 1, axis] = np.nextafter(RANGE6[face], np.float32(sign * np.inf))
    t[12, :] = np.nan
    return t


@pytest.mark.parametrize("setting", [(0.0, 1.0, 2), (0.78539, 0.0, 2)])
def test_finalize_is_the_float32_restatement_bit_for_bit(ops, setting):
    """limit_period around integer quotients, the inclusive post_center_range comparisons at equality, num_keep of 0, 1, post_max and k
    with post_max = 16 < k = 64, use_direction = 0, a NaN row."""
    dir_offset, dir_limit_offset, bins = setting
    table = _finalize_table(*setting)
    with np.errstate(invalid="ignore"):
        q = R.limit_period_quotient(table[:60, 6], *setting).reshape(12, 5)
    exact = q[:, 2] == np.floor(q[:, 2])
    assert int(exact.sum()) >= 6, "quotients that land on an integer"
    assert int((exact & (np.floor(q[:, 0]) < q[:, 2])).sum()) >= 6 and int((exact & (q[:, 4] > q[:, 2])).sum()) >= 6, "and floats on either side of it"
    b, k, p = 6, 64, 16
    g = torch.Generator().manual_seed(3)
    dec = np.repeat(table[None], b, 0)
    keep = np.stack([np.roll(np.arange(k), -16 * (f % 4)) for f in range(b)]).astype(np.int32)
    num_keep = np.array([p, k, p, k, 0, 1], np.int32)
    top_score = torch.rand(b, k, generator=g).numpy()
    top_label = torch.randint(0, 10, (b, k), generator=g).to(torch.int32).numpy()
    dir_label = torch.randint(0, bins, (b, k), generator=g).to(torch.int32).numpy()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for use_dir in (1, 0):
        for r6 in (RANGE6, None):
            want = R.finalize_reference32(dec, top_score, top_label, dir_label, keep, num_keep, p, use_dir, dir_offset, dir_limit_offset, bins, r6)
            got = ops.predict_finalize(dev(dec), dev(top_score), dev(top_label), dev(dir_label) if use_dir else None, dev(keep), dev(num_keep), p,
                                       use_dir, dir_offset, dir_limit_offset, bins, dev(r6) if r6 is not None else None)
            assert got["boxes"].shape == (b, p, 7)
            assert np.array_equal(got["valid"].cpu().numpy(), want["valid"])
            assert R.same_bits_f32(got["boxes"].cpu().numpy(), want["boxes"])
            assert R.same_bits_f32(got["scores"].cpu().numpy(), want["scores"])
            assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
            valid = got["valid"].cpu().numpy()
            assert valid[4].sum() == 0 and valid[5].sum() == 1
            if r6 is not None:                                                    # frame 0's first rows: the face rows, then the NaN row
                assert valid[0, :13].tolist() == [True, False] * 6 + [False]
            else:                                                                 # without a range nothing is compared: every kept row is valid
                assert valid[0].sum() == p and valid[1].sum() == p
            if use_dir:                                                           # the direction fix moved the rotations
                assert not R.same_bits_f32(got["boxes"][1, :, 6].cpu().numpy(), dec[1, keep[1, :p], 6])
