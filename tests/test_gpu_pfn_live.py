"""The PillarFeatureNet training kernels on static-capacity pillars with the count on the device (sec_pfn_train_fwd_live / _bwd_live
and their radius forms, ops.PFNTrainFunction / PFNRadiusTrainFunction with ``num_dev``, PillarScatterFunction with ``num_dev``):
  a. the training case table of tests/pfn_ref_helpers.py at a capacity above its pillar count, with a garbage tail, against the float64
     reference of the live rows (that file's per-element bounds and decision-aware comparison, unchanged);
  b. the count edges: n in {0, 1, 3, 4, 5} at capacities {n, n + 1, n + 7, 4100}, n = 4097 at 4100, counts above the capacity and
     negative ones;
  c. num_dev = NULL and num_dev == capacity bit-equal to the entry points without a count;
  d. one hipGraph of forward and backward replayed on three counts, bit-equal to the eager calls;
  e. the pillar scatter under autograd with a count.
Every garbage tail is in range but wrong (tests/pfn_live_helpers.py): a kernel that read it would compute wrong numbers, not fault.
tests/test_pfn_live_host.py proves on the CPU that the comparison passes a float32 emulation and fails the planted mistakes."""
import ctypes

import numpy as np
import pytest
import torch

import pfn_live_helpers as L
import pfn_ref_helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ids(c):
    return "-".join(str(v) for v in c)


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _train(cc, radius, num_dev="none"):
    """ops.PFN(Radius)TrainFunction on the case's arrays (forward and backward); ``num_dev``: an int for the device count, "none" for
    the call without one.  Returns every result as numpy, ``stats`` whole as well."""
    from second_amd import ops
    cls = ops.PFNRadiusTrainFunction if radius else ops.PFNTrainFunction
    wt = H._wt(cc, radius)
    c = wt.shape[1]
    w, ga, be = dev(wt.T.copy()).requires_grad_(), dev(cc["gamma"]).requires_grad_(), dev(cc["beta"]).requires_grad_()
    rm, rv = dev(np.asarray(cc["rm0"], np.float32)), dev(np.asarray(cc["rv0"], np.float32))
    extra = () if num_dev == "none" else (_count(num_dev),)
    out = cls.apply(dev(cc["vox"]), dev(cc["num"]), dev(cc["coords"]), w, ga, be, rm, rv, cc["eps"], cc["momentum"], cc["geom"], *extra)
    saved = out.grad_fn.saved_tensors                              # voxels, num_points, coords, wt, gamma, stats, out, argmax
    stats, arg = saved[5], saved[7]
    out.backward(dev(cc["grad_out"]))
    got = dict(mean=stats[:c], invstd=stats[c:2 * c], out=out.detach(), argmax=arg, running_mean=rm, running_var=rv, stats=stats,
               d_linear_weight=w.grad, d_norm_weight=ga.grad, d_norm_bias=be.grad)
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


def _checked(got):
    return {k: v for k, v in got.items() if k != "stats"}


# ---- (a) the case table at a capacity above its pillar count --------------------------------------------------------------------
@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
@pytest.mark.parametrize("case_id", H.TRAIN_CASES, ids=_ids)
def test_case_table_with_a_garbage_tail_against_float64(case_id, radius):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    cc = L.with_tail(case, p + 7)
    assert L.tail_is_in_range(cc, p)
    got = _train(cc, radius, p)
    res = L.check_live(_checked(got), cc, p, radius, ref_case=case)
    print("live", case_id, "radius" if radius else "nine", {k: f"{v:.3f}" for k, v in res.items()})
    assert set(res) == set(H.FWD_KEYS + H.BWD_KEYS + ("argmax", "gate", "tail"))
    if t == 127:
        assert (got["argmax"][:p] == 126).any()
    assert max(res.values()) <= 1.0, res


# ---- (b) count edges ------------------------------------------------------------------------------------------------------------
def _run_c(cc, radius, num_dev, cap=None):
    """The C entry points on the case's arrays with ``cap`` as the capacity argument (default: the arrays' rows; 0 is passed with
    arrays of one row, so that no pointer is NULL) and the device count ``num_dev`` (None: NULL).  Guard values behind every output."""
    from second_amd import runtime as rt
    l = rt.lib()
    rows, t = cc["vox"].shape[:2]
    cap = rows if cap is None else cap
    wt = H._wt(cc, radius)
    k, c = wt.shape
    a = {n: dev(cc[n]) for n in ("vox", "num", "coords", "gamma", "beta", "grad_out")}
    a["wt"] = dev(wt)
    rm, rv = dev(np.asarray(cc["rm0"], np.float32)), dev(np.asarray(cc["rv0"], np.float32))
    out = torch.full((rows + 1, c), 7.5, device="cuda")
    arg = torch.full((rows + 1, c), 99, dtype=torch.int8, device="cuda")
    stats = torch.full((c * (2 + k) + k + 4,), float("nan"), device="cuda")
    dw, dg, db = (torch.full((n + 4,), float("nan"), device="cuda") for n in (k * c, c, c))
    ws = rt.workspace(l.sec_pfn_train_workspace_bytes(cap, c), "cuda")
    nd = None if num_dev is None else _count(num_dev)
    fwd = l.sec_pfn_radius_train_fwd_live if radius else l.sec_pfn_train_fwd_live
    bwd = l.sec_pfn_radius_train_bwd_live if radius else l.sec_pfn_train_bwd_live
    geom = [ctypes.c_float(v) for v in cc["geom"]]
    rc = fwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), cap, rt.ptr(nd), t, 4, rt.ptr(a["wt"]), rt.ptr(a["gamma"]),
             rt.ptr(a["beta"]), float(cc["eps"]), float(cc["momentum"]), rt.ptr(rm), rt.ptr(rv), c, *geom, rt.ptr(out), rt.ptr(arg),
             rt.ptr(stats), rt.ptr(ws), ws.numel(), rt.stream())
    assert rc == 0
    rc = bwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), cap, rt.ptr(nd), t, 4, rt.ptr(a["wt"]), rt.ptr(a["gamma"]),
             rt.ptr(stats), c, *geom, rt.ptr(a["grad_out"]), rt.ptr(out), rt.ptr(arg), rt.ptr(dw), rt.ptr(dg), rt.ptr(db), rt.ptr(ws),
             ws.numel(), rt.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out[cap:] == 7.5).all()) and bool((arg[cap:] == 99).all())                  # nothing behind the capacity is written
    assert all(bool(torch.isnan(x[-4:]).all()) for x in (stats, dw, dg, db))
    got = dict(mean=stats[:c], invstd=stats[c:2 * c], out=out[:cap], argmax=arg[:cap], running_mean=rm, running_var=rv, stats=stats[:-4],
               d_linear_weight=dw[:k * c].view(k, c).t(), d_norm_weight=dg[:c], d_norm_bias=db[:c])
    return {k_: v.cpu().numpy() for k_, v in got.items()}


@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
@pytest.mark.parametrize("c", L.C_EDGES)
@pytest.mark.parametrize("t", L.T_EDGES)
def test_count_edges(t, c, radius):
    worst = {}
    for n in L.N_EDGES:
        case = L.edge_case(n, t, c) if n else L.empty_case(t, c)
        for cap in L.caps_of(n):
            cc = L.with_tail(case, cap)
            assert L.tail_is_in_range(cc, n)
            if cap == 0:                       # a capacity of zero: arrays of one (garbage) row, so that no pointer is NULL
                got = _run_c(L.with_tail(case, 1), radius, 0, cap=0)
            else:
                got = _run_c(cc, radius, n)
            res = L.check_live(_checked(got), cc, n, radius, ref_case=case if n else None)
            worst[(n, cap)] = max(res.values())
            assert max(res.values()) <= 1.0, (n, cap, res)
            assert np.isfinite(got["stats"]).all()
    print("count edges", t, c, "radius" if radius else "nine", {k: f"{v:.3f}" for k, v in worst.items()})
    # a count above the capacity is the capacity: bit-equal to the call without a count on the same rows
    full = L.edge_case(5, t, c)
    want, got = _run_c(full, radius, None), _run_c(full, radius, 5 + 1000)
    assert all(np.array_equal(want[k], got[k]) for k in want)
    # a negative count is zero
    cc = L.with_tail(full, 12)
    zero, neg = _run_c(cc, radius, 0), _run_c(cc, radius, -3)
    assert all(np.array_equal(zero[k], neg[k]) for k in zero)
    assert max(L.check_live(_checked(neg), cc, -3, radius).values()) == 0.0


@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
@pytest.mark.parametrize("c", L.C_EDGES)
@pytest.mark.parametrize("t", L.T_EDGES)
def test_count_above_the_grid_stride_threshold(t, c, radius):
    """n = 4097 at capacity 4100: the grids (1024 blocks of four waves) run their grid-stride loop over live pillars only.  The float64
    reference runs on slot-trimmed pillars (at most three points each; the zero rows that were cut count in the statistics)."""
    case = L.sparse_case(4097, t, c)
    cc = L.with_tail(case, L.BIG_CAP)
    assert L.tail_is_in_range(cc, 4097)
    got = _run_c(cc, radius, 4097)
    res = L.check_live(_checked(got), cc, 4097, radius, ref_case=H.trim_slots(case))
    print("n = 4097", t, c, "radius" if radius else "nine", {k: f"{v:.3f}" for k, v in res.items()})
    assert max(res.values()) <= 1.0, res


# ---- (c) no count, and a count equal to the capacity ----------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
@pytest.mark.parametrize("case_id", [(33, 5, 16, "plain", (-0.3, 0.3)), (700, 60, 33, "plain", (-0.3, 0.3)), (4100, 20, 64, "plain", (-0.3, 0.3))], ids=_ids)
def test_null_count_and_full_count_are_bit_equal_to_the_forms_without_one(case_id, radius):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    want = _train(case, radius)                                        # sec_pfn_train_fwd / _bwd (or the radius forms), as before
    null, full = _run_c(case, radius, None), _run_c(case, radius, p)   # the _live forms with NULL and with num_dev == capacity
    through_ops = _train(case, radius, p)
    for name, got in (("NULL", null), ("count == capacity", full), ("ops, count == capacity", through_ops)):
        for k in want:
            assert np.array_equal(want[k], got[k]), (name, k)


# ---- (d) the count is read when the kernels run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
def test_one_captured_graph_follows_the_count(radius):
    """Forward and backward captured ONCE at capacity 47, replayed with 40, 3 and 0 in the device int: each replay is bit-equal to the
    eager call with that count (same grid, same partition of the sums), and differs from the other counts' results."""
    from second_amd import runtime as rt
    l = rt.lib()
    case = H.train_case(40, 9, 64, "plain", seed=3)
    cc = L.with_tail(case, 47)
    cap, t = cc["vox"].shape[:2]
    wt = H._wt(cc, radius)
    k, c = wt.shape
    a = {n: dev(cc[n]) for n in ("vox", "num", "coords", "gamma", "beta", "grad_out")}
    a["wt"] = dev(wt)
    rm0, rv0 = dev(np.asarray(cc["rm0"], np.float32)), dev(np.asarray(cc["rv0"], np.float32))
    rm, rv = rm0.clone(), rv0.clone()
    out, arg = torch.empty((cap, c), device="cuda"), torch.empty((cap, c), dtype=torch.int8, device="cuda")
    stats = torch.empty((c * (2 + k) + k,), device="cuda")
    dw, dg, db = (torch.empty((n,), device="cuda") for n in (k * c, c, c))
    ws = rt.workspace(l.sec_pfn_train_workspace_bytes(cap, c), "cuda")
    nd = _count(cap)
    fwd = l.sec_pfn_radius_train_fwd_live if radius else l.sec_pfn_train_fwd_live
    bwd = l.sec_pfn_radius_train_bwd_live if radius else l.sec_pfn_train_bwd_live
    geom = [ctypes.c_float(v) for v in cc["geom"]]

    def both():
        rc = fwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), cap, rt.ptr(nd), t, 4, rt.ptr(a["wt"]), rt.ptr(a["gamma"]),
                 rt.ptr(a["beta"]), float(cc["eps"]), float(cc["momentum"]), rt.ptr(rm), rt.ptr(rv), c, *geom, rt.ptr(out), rt.ptr(arg),
                 rt.ptr(stats), rt.ptr(ws), ws.numel(), rt.stream())
        assert rc == 0
        rc = bwd(rt.ptr(a["vox"]), rt.ptr(a["num"]), rt.ptr(a["coords"]), cap, rt.ptr(nd), t, 4, rt.ptr(a["wt"]), rt.ptr(a["gamma"]),
                 rt.ptr(stats), c, *geom, rt.ptr(a["grad_out"]), rt.ptr(out), rt.ptr(arg), rt.ptr(dw), rt.ptr(dg), rt.ptr(db), rt.ptr(ws),
                 ws.numel(), rt.stream())
        assert rc == 0

    results = (out, arg, stats, dw, dg, db, rm, rv)

    def reset(n):
        nd.fill_(n)
        rm.copy_(rm0)
        rv.copy_(rv0)
        for x in (out, stats, dw, dg, db):
            x.fill_(-3.0)
        arg.fill_(55)

    eager = {}
    for n in (40, 3, 0):
        reset(n)
        both()
        torch.cuda.synchronize()
        eager[n] = [x.clone() for x in results]
    assert not torch.equal(eager[40][2], eager[3][2]) and not torch.equal(eager[3][3], eager[0][3])      # the counts do differ
    reset(cap)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with rt.capture_guard(), torch.cuda.graph(g, stream=side):
        both()
    for n in (3, 40, 0, 40):
        reset(n)
        g.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(("out", "argmax", "stats", "dw", "dgamma", "dbeta", "running_mean", "running_var"), results, eager[n]):
            assert torch.equal(x, y), (n, name)
    # and the eager results themselves are right: the float64 comparison on the last replay (count 40)
    got = dict(mean=stats[:c], invstd=stats[c:2 * c], out=out, argmax=arg, running_mean=rm, running_var=rv,
               d_linear_weight=dw.view(k, c).t(), d_norm_weight=dg, d_norm_bias=db)
    res = L.check_live({k_: v.cpu().numpy() for k_, v in got.items()}, cc, 40, radius, ref_case=case)
    assert max(res.values()) <= 1.0, res


# ---- (e) the scatter under autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", list(H.KINDS))
def test_pillar_scatter_function_with_a_count(kind, channels_last):
    from spconv.functional import PillarScatterFunction
    dt = H.KINDS[kind]
    p, c = 40, 65
    feat, coords, batch, ny, nx = H.scatter_case(p, c)
    rng = np.random.default_rng(c)
    g = torch.from_numpy((rng.integers(-64, 64, (batch, c, ny, nx)) / 4).astype(np.float32)).to(dt).cuda()
    if channels_last:
        g = g.contiguous(memory_format=torch.channels_last)
    for n in (0, 1, 17, 40):
        # the tail carries live cells and large values: landing it, or gathering for it, shows
        f = feat.copy()
        f[n:] = 4096.0
        co_n = coords.copy()
        if n:
            co_n[n:] = coords[np.arange(p - n) % n]
        x = dev(f).to(dt).requires_grad_()
        img = PillarScatterFunction.apply(x, dev(co_n), batch, ny, nx, channels_last, _count(n))
        assert img.dtype == dt and img.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        want = H.scatter64(dev(f).to(dt).float().cpu().numpy()[:n], co_n[:n], batch, ny, nx)
        assert np.array_equal(img.detach().float().cpu().numpy(), want), (n, "forward")
        img.backward(g)
        assert x.grad.shape == (p, c) and not x.grad[n:].any(), (n, "tail gradient")
        if n:
            xd = dev(f[:n]).to(dt).requires_grad_()
            PillarScatterFunction.apply(xd, dev(co_n[:n]), batch, ny, nx, channels_last).backward(g)
            assert torch.equal(x.grad[:n], xd.grad), (n, "live gradient")


# ---- the modules hand the count on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
def test_modules_pass_the_count_on_in_training_mode(radius):
    """PillarFeatureNet(.Radius).forward(..., num_dev=) and PointPillarsScatter.forward(..., num_dev=) in training mode: the live rows,
    the gradients and the running statistics are bit-equal to the modules on the first n rows alone (below 4 096 pillars a block sums
    the same four pillars in both calls, and the blocks past the count add exact zeros), the tail is zero, nothing lands for it."""
    from second_amd import models as M
    n, cap, t, c = 40, 47, 9, 64
    case = H.train_case(n, t, c, "plain", seed=4)
    cc = L.with_tail(case, cap)
    assert L.tail_is_in_range(cc, n)
    g_img = torch.from_numpy(np.random.default_rng(1).standard_normal((1, c, 400, 400)).astype(np.float32)).cuda()
    res = {}
    for live in (False, True):
        torch.manual_seed(0)
        pfn = (M.PillarFeatureNetRadius if radius else M.PillarFeatureNet)(4, (c,), (0.25, 0.25, 8), (-50, -50, -5, 50, 50, 3)).cuda().train()
        scat = M.PointPillarsScatter([1, 1, 400, 400], c)
        src = cc if live else case
        kw = dict(num_dev=_count(n)) if live else {}
        feats = pfn(dev(src["vox"]), dev(src["num"]), dev(src["coords"]), **kw)
        img = scat(feats, dev(src["coords"]), 1, **kw)
        img.backward(g_img)
        torch.cuda.synchronize()
        l = pfn.pfn_layers[0]
        res[live] = [feats.detach()[:n], img.detach(), l.linear.weight.grad, l.norm.weight.grad, l.norm.bias.grad, l.norm.running_mean,
                     l.norm.running_var, l.norm.num_batches_tracked]
        if live:
            assert feats.shape == (cap, c) and not feats.detach()[n:].any()
    for name, a, b in zip(("features", "image", "d linear.weight", "d norm.weight", "d norm.bias", "running_mean", "running_var", "batches"),
                          res[True], res[False]):
        assert torch.equal(a, b), name
    assert res[True][2].abs().max() > 0 and int(res[True][7]) == 1
    # a count the training kernels cannot serve is an error, not a quiet walk through the torch formulation over the garbage rows
    pfn.train_backend = "torch"
    with pytest.raises(RuntimeError, match="num_dev"):
        pfn(dev(cc["vox"]), dev(cc["num"]), dev(cc["coords"]), num_dev=_count(n))
