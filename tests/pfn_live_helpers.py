"""The PillarFeatureNet training kernels on STATIC-CAPACITY pillars (sec_pfn_train_fwd_live / _bwd_live and their radius forms: the
arrays hold ``cap`` rows, live = min(max(*num_dev, 0), cap) of them are pillars): capacity cases with a garbage tail, a float32
emulation of the kernels with a live count and planted mistakes, and the comparison -- the float64 reference, per-element bounds and
decision-aware checks of tests/pfn_ref_helpers.py on the live rows, unchanged, plus what the entry points promise about the rest.
Shared by tests/test_pfn_live_host.py (CPU: the emulation passes, every planted mistake fails) and tests/test_gpu_pfn_live.py.

The garbage tail is IN RANGE but WRONG: coords copied from live pillars (the grid's centre cell where there is none), num_points = T,
points and grad_out finite but large (1e6).  A kernel that wrongly reads a tail row produces wrong numbers, never a fault."""
import numpy as np

import pfn_ref_helpers as H

GARBAGE = np.float32(1e6)
GRID = 400                                     # cells per side of the 0.25 m grids of H.GEOM (offset case: up to 480)
T_EDGES, C_EDGES = (1, 60, 100), (33, 64)
N_EDGES = (0, 1, 3, 4, 5)
BIG_CAP = 4100                                 # above kPfnMaxBlocks x four waves = 4096 pillars: the grid-stride loop runs
LIVE_BUGS = {"rows_cap": ("mean", "invstd"), "tail_in_stats": ("mean",), "tail_grad_in_dbeta": ("d_norm_bias",),
             "rv_cap_factor": ("running_var",)}


def live_count(num_dev, cap):
    return min(max(int(num_dev), 0), int(cap))


def caps_of(n):
    return (n, n + 1, n + 7, BIG_CAP)


def edge_case(n, t, c, seed=0):
    """A training case of n >= 1 pillars for the count edges (pfn_ref_helpers.train_case, plain)."""
    return H.train_case(n, t, c, "plain", seed=seed)


def sparse_case(n, t, c, keep=3, seed=0):
    """Many pillars cheaply: at most ``keep`` points each, so that the float64 reference can run on slot-trimmed pillars
    (H.trim_slots: the cut zero rows still count in the statistics)."""
    case = H.train_case(n, t, c, "plain", seed=seed)
    case["num"] = np.minimum(case["num"], keep).astype(np.int32)
    case["vox"] = (case["vox"] * (np.arange(t)[None, :] < case["num"][:, None])[..., None]).astype(np.float32)
    return case


def with_tail(case, cap):
    """The case at capacity ``cap``: its n rows (n = 0: :func:`empty_case`) followed by cap - n garbage rows (see the module text)."""
    n, t = case["vox"].shape[:2]
    c = case["grad_out"].shape[1]
    assert cap >= n
    pad = cap - n
    src = case["coords"][np.arange(pad) % n] if n else np.tile(np.array([[0, 0, GRID // 2, GRID // 2]], np.int32), (pad, 1))
    cc = dict(case,
              vox=np.concatenate([case["vox"], np.full((pad, t, 4), GARBAGE, np.float32)]),
              num=np.concatenate([case["num"], np.full(pad, t, np.int32)]).astype(np.int32),
              coords=np.concatenate([case["coords"], src.astype(np.int32)]).astype(np.int32),
              grad_out=np.concatenate([case["grad_out"], np.full((pad, c), GARBAGE, np.float32)]))
    return {k: v for k, v in cc.items() if not isinstance(k, tuple)}


def empty_case(t, c, seed=0):
    """No pillar at all (n = 0) with the parameters of a real case: what :func:`with_tail` pads to a capacity."""
    case = H.train_case(1, t, c, "plain", seed=seed)
    return {k: (v[:0] if k in ("vox", "num", "coords", "grad_out") else v) for k, v in case.items() if not isinstance(k, tuple)}


def tail_is_in_range(cc, n):
    """The property every generated tail has: reading it cannot fault -- counts within 1 .. T, cells on the grid and taken from the
    live pillars where there are any, finite points and gradients -- and cannot go unnoticed (large values)."""
    cap, t = cc["vox"].shape[:2]
    tail = slice(n, cap)
    ok = bool(((cc["num"][tail] >= 1) & (cc["num"][tail] <= t)).all())
    co = cc["coords"][tail]
    ok &= bool((co[:, :2] == 0).all() and (co[:, 2:] >= 0).all() and (co[:, 2:] < 2 * GRID).all())
    if n and cap > n:
        live = {tuple(r) for r in cc["coords"][:n]}
        ok &= all(tuple(r) in live for r in co)
    ok &= bool(np.isfinite(cc["vox"][tail]).all() and np.isfinite(cc["grad_out"][tail]).all())
    ok &= bool((np.abs(cc["vox"][tail]) >= 1e5).all() and (np.abs(cc["grad_out"][tail]) >= 1e5).all())
    return ok


def head_of(cc, n):
    """The first n rows as a case of pfn_ref_helpers (what the float64 reference sees)."""
    return {k: (v[:n] if k in ("vox", "num", "coords", "grad_out") else v) for k, v in cc.items() if not isinstance(k, tuple)}


# ------------------------------------------------------------------------------------------------ float32 emulation with a live count
def emulate32_live(cc, num_dev, radius, bug=None):
    """The arithmetic of the five kernels in float32 numpy (fp64 sums, another summation order) on a capacity case with the live
    count ``num_dev``; H.emulate32's train branch with the count threaded through.  Planted mistakes: rows_cap (BatchNorm's N is
    cap * T), tail_in_stats (one tail pillar summed into the statistics), tail_grad_in_dbeta (one tail row of grad_out summed into
    dbeta), rv_cap_factor (running_var with the capacity's unbiased factor), zero_div (no guard for live == 0)."""
    f = np.float32
    cap, t, _ = cc["vox"].shape
    n = live_count(num_dev, cap)
    use = min(n + 1, cap)                                              # the rows this emulation (with its mistakes) can touch
    v = np.asarray(cc["vox"][:use], f)
    num = np.asarray(cc["num"][:use], np.int64)
    vx, vy, xo, yo = (f(g) for g in cc["geom"])
    slot_live = np.arange(t)[None, :] < num[:, None]
    xyz = v[..., :3]
    with np.errstate(all="ignore"):
        mean_p = xyz.sum(1, dtype=f) / num.astype(f)[:, None]
        co = np.asarray(cc["coords"][:use])
        cx, cy = co[:, 3].astype(f) * vx + xo, co[:, 2].astype(f) * vy + yo
        head = np.concatenate([np.sqrt(v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2], dtype=f), v[..., 2:]], -1) if radius else v
        dec = np.concatenate([head, xyz - mean_p[:, None, :], (v[..., 0] - cx[:, None])[..., None], (v[..., 1] - cy[:, None])[..., None]], -1)
        dec = (dec * slot_live[..., None]).astype(f)
        wt = np.asarray(H._wt(cc, radius), f)
        x = (dec @ wt).astype(f)
    k, c = dec.shape[2], x.shape[2]
    stat = min(n + 1, cap) if bug == "tail_in_stats" else n            # the pillars that enter the sums
    rows = float((cap if bug == "rows_cap" else n) * t)
    eps, mom = float(cc["eps"]), float(cc["momentum"])
    ga, be = np.asarray(cc["gamma"], f), np.asarray(cc["beta"], f)
    rm0, rv0 = np.asarray(cc["rm0"], np.float64), np.asarray(cc["rv0"], np.float64)
    xs64 = x[:stat].astype(np.float64)
    with np.errstate(all="ignore"):
        if rows > 0 or bug == "zero_div":
            mean64 = xs64.sum((0, 1)) / rows
            # two-pass over the summed rows; the rows of N that were not summed are zero rows, (0 - mean)^2 each
            var = np.maximum((((xs64 - mean64) ** 2).sum((0, 1)) + (rows - stat * t) * mean64 ** 2) / rows, 0.0)
            urows = float(cap * t) if bug == "rv_cap_factor" else rows
            var_u = var * (urows / (urows - 1.0) if urows > 1 else 1.0)
            rm = ((1 - mom) * rm0 + mom * mean64).astype(f)
            rv = ((1 - mom) * rv0 + mom * var_u).astype(f)
        else:                                                          # no live pillar: mean 0, variance 0, running statistics kept
            mean64, var = np.zeros(c), np.zeros(c)
            rm, rv = np.asarray(cc["rm0"], f).copy(), np.asarray(cc["rv0"], f).copy()
        mean = mean64.astype(f)
        inv = (1.0 / np.sqrt(var + eps)).astype(f)
        xhat = ((x - mean) * inv).astype(f)
        y = np.maximum(xhat * ga + be, f(0)).astype(f)
    ym = np.where(np.ones_like(slot_live)[..., None], y, -np.inf)
    out, arg = np.zeros((cap, c), f), np.full((cap, c), -1, np.int64)  # rows past the count: defined, nothing of them computed
    out[:n] = ym.max(1).astype(f)[:n]
    arg[:n] = np.where(ym.argmax(1) >= num[:, None], -1, ym.argmax(1))[:n]
    got = dict(mean=mean, invstd=inv, out=out, argmax=arg, running_mean=rm, running_var=rv)
    g = np.asarray(cc["grad_out"], f)
    dz = (g * (out > 0))[:n]
    slot = np.where(arg < 0, t - 1, arg)[:n]
    fs = dec[np.arange(n)[:, None], slot]
    xs = np.take_along_axis(xhat[:n], slot[:, None, :], 1)[:, 0, :]
    db = dz.sum(0, dtype=np.float64)
    if bug == "tail_grad_in_dbeta" and n < cap:
        db = db + g[n].astype(np.float64)
    dg = (dz * xs).sum(0, dtype=np.float64)
    a = np.einsum("pc,pck->ck", dz, fs).astype(np.float64)
    s1 = dec[:stat].sum((0, 1), dtype=np.float64).astype(f).astype(np.float64)
    m = np.einsum("ptc,ptk->ck", x[:stat], dec[:stat]).astype(f).astype(np.float64)
    i64, m64 = inv.astype(np.float64), mean.astype(np.float64)
    with np.errstate(all="ignore"):
        if rows > 0 or bug == "zero_div":
            dw = ga.astype(np.float64)[:, None] * i64[:, None] * (a - db[:, None] / rows * s1[None, :]
                                                                   - dg[:, None] / rows * i64[:, None] * (m - m64[:, None] * s1[None, :]))
        else:
            dw = np.zeros((c, k))
    got.update(d_linear_weight=dw.astype(f), d_norm_weight=dg.astype(f), d_norm_bias=db.astype(f))
    return got


# ------------------------------------------------------------------------------------------------ the comparison
def check_live(got, cc, num_dev, radius, ref_case=None):
    """{quantity: worst error / bound} of a run at capacity against the float64 reference of the live rows (H.check_train on the
    first ``live`` rows, bounds and decisions unchanged), plus ``tail``: 0.0 when every ``out`` row past the count is exactly zero
    and every ``argmax`` there -1, else inf.  live == 0: :func:`check_empty`.  ``ref_case``: the case the reference runs on where it
    is not simply the head (slot-trimmed pillars); it is kept by the caller so that its float64 results are computed once."""
    cap = cc["vox"].shape[0]
    n = live_count(num_dev, cap)
    g = {k: np.asarray(v) for k, v in got.items()}
    tail_ok = g["out"].shape[0] == cap and not g["out"][n:].any() and bool((g["argmax"][n:] == -1).all())
    if n == 0:
        res = check_empty(g, cc)
    else:
        head = ref_case if ref_case is not None else head_of(cc, n)
        res = H.check_train(dict(g, out=g["out"][:n], argmax=g["argmax"][:n]), head, radius)
    res["tail"] = 0.0 if tail_ok else float("inf")
    return res


def check_empty(got, cc):
    """No live pillar: nothing may be NaN or infinite, the running statistics keep their bits, the three gradients are exactly zero,
    the statistics are those of no row (mean 0, invstd = 1 / sqrt(eps))."""
    g = {k: np.asarray(v) for k, v in got.items()}
    finite = all(bool(np.isfinite(np.asarray(v, np.float64)).all()) for v in g.values())
    same = np.array_equal(np.asarray(g["running_mean"], np.float32), np.asarray(cc["rm0"], np.float32)) and \
        np.array_equal(np.asarray(g["running_var"], np.float32), np.asarray(cc["rv0"], np.float32))
    zero = all(not np.asarray(g[k]).any() for k in H.BWD_KEYS)
    stats = not g["mean"].any() and np.allclose(g["invstd"], 1.0 / np.sqrt(float(cc["eps"])), rtol=1e-6, atol=0)
    inf = float("inf")
    return dict(finite=0.0 if finite else inf, running=0.0 if same else inf, gradients=0.0 if zero else inf, stats=0.0 if stats else inf)
