"""Float64 references, per-element error bounds, exact cases, input generators and the case tables of the PillarFeatureNet kernels
(csrc/pillars.hip: k_pfn_fwd in its tensor and slots forms, k_pfn_stats, k_pfn_finalize, k_pfn_fwd_train, k_pfn_bwd,
k_pfn_bwd_finalize, each on the nine-entry row and on the eight-entry radius row) and of the pillar scatter (csrc/scatter.hip).
numpy / torch on the CPU; shared by tests/test_pfn_ref_host.py (which proves on the CPU that the comparison bites) and
tests/test_gpu_pfn_edges.py (which holds the kernels to it).  The references are written from the reference's formulation
(second/pytorch/models/pointpillars.py:51-65 PFNLayer, :203-237 PillarFeatureNet.forward, :290-325 PillarFeatureNetRadius.forward),
not imported from second_amd.models.

Bounds (u = 2^-24, gamma_n of dense_train_ref_helpers; every product below is taken with the perturbed magnitudes, so there is no
first-order shortcut).  For one decorated row f[0..K-1] of a point (x, y, z, w) of pillar p:
  raw entries          exact.
  r = sqrt(x^2 + y^2)  two products, one sum, one square root, each correctly rounded: |dr| <= gamma_3 r.
  pillar mean m        a sum over the T slots in ANY order and one division: |dm| <= gamma_T sum|x_t| / n.
  x - m                one more rounding: |d| <= dm + u (|x - m| + dm).
  pillar centre c      c = fl(fl(i * v) + o): two roundings, |dc| <= gamma_2 (|i v| + |o|); x - c as x - m.
  linear x_c           K fmas: |dx| <= gamma_K sum_j (|f_j| + df_j) |w_j| + sum_j df_j |w_j|.
  eval                 y = relu(fl(x * scale + shift)): |dy| <= dx |scale| + u (|x scale + shift| + dx |scale|); relu is 1-Lipschitz.
  train                y = relu(fma(fl(fl(x - mean) * invstd), gamma, beta)) with the bounds of mean and invstd propagated.
  max over the slots   1-Lipschitz: the element's bound is the largest bound among its slots; the padded slot's value relu(shift)
                       (eval) is exact, in training it carries the bounds of mean and invstd.
  16-bit outputs       one storage rounding on top (u16 |ref| + (1 + u16) bound), fp16 with its subnormal floor 2^-25.
Statistics (mean, invstd, running_mean, running_var): the propagated error of the rows (derived) plus the accumulation, whose
constant cannot be derived for an unknown order over P * T rows: FOUR times the error the float32 torch formulation shows against
float64 on the same inputs (torch_f32_constants; measured on the CPU, never on the kernel under test).  Gradients: the sum of term
magnitudes times gamma_(P + 4) (any order over the pillars, four waves), plus the propagated bounds of the rows, mean and invstd,
through the closed form k_pfn_bwd_finalize evaluates.

Decisions: no element is excluded.  The kernel's argmax is accepted when its slot's float64 value is within twice the element's
bound of the float64 maximum (-1 = the padded slot, which must exist), its ReLU gate (out > 0) when |y64| of that slot is within
the bound wherever it disagrees with float64; the float64 backward is then evaluated with the kernel's own argmax and gate."""
import numpy as np
import torch

from dense_train_ref_helpers import FP16_SUB, TINY, gamma_n, store_floor  # noqa: F401
from indice_conv_bwd_helpers import U24, U_STORE, worst  # noqa: F401

GEOM = (0.25, 0.25, -49.875, -49.875)        # vx, vy, x_offset, y_offset of the 0.25 m grids (all.pp.largea, all.pp.mhead)
EPS, MOMENTUM = 1e-3, 0.01
KINDS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _k(radius):
    return 8 if radius else 9


def _wt(case, radius):
    """[K, C] weights of the row: cases made for both rows carry the nine-entry ``wt9`` (the radius row drops its first line: r takes
    the place of x and y), the others their own ``wt``."""
    return np.ascontiguousarray(case["wt9"][1:] if radius else case["wt9"]) if "wt9" in case else case["wt"]


def _cached(case, key, make):
    if key not in case:
        case[key] = make()
    return case[key]


def _f32geom(geom):
    return [float(np.float32(v)) for v in geom]


# ------------------------------------------------------------------------------------------------ decorated rows
def decorate64(vox, num, coords, geom, radius, mean_div=None, centre_cols=(3, 2), radius_x=False, slots=None):
    """(dec [P, T, K], ddec [P, T, K], live [P, T]) in float64: the decorated, masked rows and the bound of each entry as a float32
    kernel may compute it.  mean_div / centre_cols / radius_x plant mistakes (the host test)."""
    v = np.asarray(vox, np.float64)
    p, t, _ = v.shape
    n = np.asarray(num, np.int64)
    vx, vy, xo, yo = _f32geom(geom)
    live = np.arange(t)[None, :] < n[:, None]
    div = (n if mean_div is None else np.full(p, mean_div)).astype(np.float64)[:, None]
    xyz = v[..., :3]
    mean = xyz.sum(1) / div                                                        # over all T slots (the padded ones are zero)
    dmean = gamma_n(slots or t) * np.abs(xyz).sum(1) / div
    co = np.asarray(coords, np.float64)
    ix, iy = co[:, centre_cols[0]], co[:, centre_cols[1]]
    cen = np.stack([ix * vx + xo, iy * vy + yo], 1)
    dcen = gamma_n(2) * np.stack([np.abs(ix * vx) + abs(xo), np.abs(iy * vy) + abs(yo)], 1)
    d_m = xyz - mean[:, None, :]
    dd_m = dmean[:, None, :] + U24 * (np.abs(d_m) + dmean[:, None, :])
    d_c = v[..., :2] - cen[:, None, :]
    dd_c = dcen[:, None, :] + U24 * (np.abs(d_c) + dcen[:, None, :])
    if radius:
        r = v[..., 0:1] if radius_x else np.sqrt(v[..., 0:1] ** 2 + v[..., 1:2] ** 2)
        head, dhead = np.concatenate([r, v[..., 2:]], -1), np.concatenate([gamma_n(3) * np.abs(r), np.zeros_like(v[..., 2:])], -1)
    else:
        head, dhead = v, np.zeros_like(v)
    dec = np.concatenate([head, d_m, d_c], -1) * live[..., None]
    ddec = np.concatenate([dhead, dd_m, dd_c], -1) * live[..., None]
    return dec, ddec, live


def linear64(dec, ddec, wt):
    """x [P, T, C] = dec @ W and its bound after K fmas."""
    w = np.asarray(wt, np.float64)
    k = w.shape[0]
    x = dec @ w
    prop = ddec @ np.abs(w)
    dx = gamma_n(k) * ((np.abs(dec) + ddec) @ np.abs(w)) + prop
    return x, dx


def store_bound(ref, bound, kind):
    """One storage rounding of a 16-bit output on top of the fp32 bound."""
    if kind == "fp32":
        return bound + TINY
    u = U_STORE[kind]
    return u * np.abs(ref) + (1 + u) * bound + store_floor(kind)


# ------------------------------------------------------------------------------------------------ eval layer
def eval64(case, radius, pad_in_max=True, **plant):
    """(out [P, C], bound [P, C]) of the eval layer (Linear, folded BatchNorm, ReLU, max over the slots) in float64."""
    dec, ddec, live = decorate64(case["vox"], case["num"], case["coords"], case["geom"], radius, **plant)
    x, dx = linear64(dec, ddec, _wt(case, radius))
    sc, sh = np.asarray(case["scale"], np.float64), np.asarray(case["shift"], np.float64)
    pre = x * sc + sh
    dy = dx * np.abs(sc) + U24 * (np.abs(pre) + dx * np.abs(sc))
    y = np.maximum(pre, 0.0)
    t = live.shape[1]
    use = live if not pad_in_max else np.ones_like(live)      # a padded slot is a zero row: y = relu(shift), exactly (dy = 0 there)
    y = np.where(use[..., None], y, -np.inf)
    dy = np.where(live[..., None], dy, 0.0)
    assert t > 0
    return y.max(1), dy.max(1)


def check_eval(got, case, radius, kind):
    """Worst error / bound over every element of an inference output (torch tensor or array) of dtype ``kind``."""
    ref, b = _cached(case, ("eval64", radius), lambda: eval64(case, radius))
    g = got.detach().float().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return worst(g, ref, store_bound(ref, b, kind))


# ------------------------------------------------------------------------------------------------ train-mode layer
def torch_f32_constants(case, radius):
    """The accumulation constants of the statistics: relative error of the FLOAT32 torch formulation (decorate, F.linear,
    torch.native_batch_norm in training mode, all on the CPU) against float64 on the case's inputs, as the maximum over the
    channels: mean against the channel's mean |x|, invstd and the unbiased variance against their own values.  torch's CPU BatchNorm
    sums float32 within each thread's chunk of the rows, so its error follows the thread count (offset case, invstd: 2.8e-6 with one
    thread, 2.2e-7 with sixteen); it is measured with MEASURE_THREADS threads wherever it runs, so the bar is the same everywhere."""
    threads = torch.get_num_threads()
    torch.set_num_threads(MEASURE_THREADS)
    try:
        return _torch_f32_constants(case, radius)
    finally:
        torch.set_num_threads(threads)


MEASURE_THREADS = 16


def _torch_f32_constants(case, radius):
    res = {}
    for dt in (torch.float64, torch.float32):
        v = torch.as_tensor(np.asarray(case["vox"])).to(dt)
        n = torch.as_tensor(np.asarray(case["num"])).long()
        co = torch.as_tensor(np.asarray(case["coords"])).to(dt)
        vx, vy, xo, yo = _f32geom(case["geom"])
        if case.get("slots", v.shape[1]) > v.shape[1]:
            v = torch.nn.functional.pad(v, (0, 0, 0, case["slots"] - v.shape[1]))
        p, t, _ = v.shape
        xyz = v[..., :3]
        mean = xyz.sum(1, keepdim=True) / n.to(dt).view(-1, 1, 1)
        cx, cy = co[:, 3].view(-1, 1) * vx + xo, co[:, 2].view(-1, 1) * vy + yo
        tail = [xyz - mean, (v[..., 0] - cx).unsqueeze(-1), (v[..., 1] - cy).unsqueeze(-1)]
        head = [torch.linalg.vector_norm(v[..., :2], ord=2, dim=2, keepdim=True), v[..., 2:]] if radius else [v]
        mask = (torch.arange(t).view(1, -1) < n.view(-1, 1)).to(dt).unsqueeze(-1)
        x = torch.nn.functional.linear(torch.cat(head + tail, -1) * mask, torch.as_tensor(np.asarray(_wt(case, radius))).to(dt).t())
        _, m, inv = torch.native_batch_norm(x.reshape(p * t, -1), None, None, None, None, True, MOMENTUM, float(case["eps"]))
        rows = p * t
        var_u = x.reshape(rows, -1).var(0, unbiased=True) if rows > 1 else x.reshape(rows, -1).var(0, unbiased=False)
        res[dt] = (m.double().numpy(), inv.double().numpy(), var_u.double().numpy(), x.abs().double().mean((0, 1)).numpy())
    (m64, i64, v64, mabs), (m32, i32, v32, _) = res[torch.float64], res[torch.float32]
    tiny = 1e-300
    return dict(mean=float((np.abs(m32 - m64) / np.maximum(mabs, tiny)).max()), invstd=float((np.abs(i32 - i64) / i64).max()),
                var=float((np.abs(v32 - v64) / np.maximum(v64, tiny)).max()))


def train64(case, radius, rows_live=False, unbiased_norm=False, rv_biased=False, pad_in_max=True, **plant):
    """The train-mode layer in float64 with every bound the comparison needs.  Batch statistics over ALL P * T rows (the zero rows
    of the padded slots included); biased variance for normalising, unbiased (N / (N - 1)) for running_var; momentum update; ReLU;
    max over the slots (first maximum; -1 = a padded slot won).  case["slots"] = T where ``vox`` holds only the first slots of
    a [P, T, 4] tensor (trim_slots): the zero rows that were cut off count in the statistics as the rows they are."""
    slots = int(case.get("slots", np.shape(case["vox"])[1]))
    dec, ddec, live = decorate64(case["vox"], case["num"], case["coords"], case["geom"], radius, slots=slots, **plant)
    x, dx = linear64(dec, ddec, _wt(case, radius))
    p, t, c = x.shape
    cut = float(p * (slots - t))
    rows = float(live.sum()) if rows_live else float(p * slots)
    eps, mom = float(case["eps"]), float(case["momentum"])
    ga, be = np.asarray(case["gamma"], np.float64), np.asarray(case["beta"], np.float64)
    mean = x.sum((0, 1)) / rows
    var = (((x - mean) ** 2).sum((0, 1)) + cut * mean ** 2) / rows if not rows_live else (x ** 2).sum((0, 1)) / rows - mean ** 2
    var_u = var * (rows / (rows - 1.0) if rows > 1 else 1.0)
    invstd = 1.0 / np.sqrt((var_u if unbiased_norm else var) + eps)
    rm = (1 - mom) * np.asarray(case["rm0"], np.float64) + mom * mean
    rv = (1 - mom) * np.asarray(case["rv0"], np.float64) + mom * (var if rv_biased else var_u)
    # bounds of the statistics: propagated row errors + 4 x the float32 torch formulation's own error (accumulation)
    k4 = _cached(case, ("consts", radius), lambda: torch_f32_constants(case, radius))
    mabs = np.abs(x).sum((0, 1)) / rows
    dmean = dx.sum((0, 1)) / rows + 4 * k4["mean"] * mabs
    dvar = 2.0 * ((np.abs(x - mean) * (dx + dmean)).sum((0, 1)) + cut * np.abs(mean) * dmean) / rows
    dinv = 0.5 * invstd ** 3 * dvar * 1.001 + 4 * k4["invstd"] * invstd
    drm = mom * dmean + U24 * np.abs(rm) * 2
    drv = mom * (dvar * 1.001 * (rows / (rows - 1.0) if rows > 1 else 1.0) + 4 * k4["var"] * var_u) + U24 * np.abs(rv) * 2
    # normalise, ReLU, max
    d = x - mean
    dd = dx + dmean + U24 * (np.abs(d) + dx + dmean)
    xhat = d * invstd
    dxhat = dd * (invstd + dinv) + np.abs(d) * dinv + U24 * (np.abs(xhat) + dd * (invstd + dinv) + np.abs(d) * dinv)
    pre = xhat * ga + be
    dy = dxhat * np.abs(ga)
    dy = dy + U24 * (np.abs(pre) + dy)
    y = np.maximum(pre, 0.0)
    use = np.ones_like(live) if pad_in_max else live
    ymax = np.where(use[..., None], y, -np.inf)
    out = ymax.max(1)
    arg = ymax.argmax(1)                                        # first maximum; a padded slot sits after every live one
    arg = np.where(arg >= np.asarray(case["num"], np.int64)[:, None], -1, arg)
    return dict(dec=dec, ddec=ddec, live=live, x=x, dx=dx, rows=rows, mean=mean, var=var, invstd=invstd, running_mean=rm, running_var=rv,
                d_mean=dmean + TINY, d_invstd=dinv, d_running_mean=drm + TINY, d_running_var=drv, xhat=xhat, dxhat=dxhat, pre=pre, y=y,
                dy=dy, out=out, d_out=dy.max(1) + TINY, argmax=arg, gamma=ga, beta=be, consts=k4)


def accept_decisions(ref, case, arg, gate):
    """(argmax accepted [P, C], gate accepted [P, C]) for the kernel's argmax (int, -1 = padded slot) and gate (bool, out > 0)."""
    n = np.asarray(case["num"], np.int64)[:, None]
    t = ref["live"].shape[1]
    arg = np.asarray(arg, np.int64)
    valid = ((arg >= 0) & (arg < np.minimum(n, t))) | ((arg == -1) & (n < t))
    slot = np.where(arg < 0, t - 1, np.clip(arg, 0, t - 1))       # a padded slot exists only where n < t: slot t - 1 is then one
    y_sel = np.take_along_axis(ref["y"], slot[:, None, :], 1)[:, 0, :]
    pre_sel = np.take_along_axis(ref["pre"], slot[:, None, :], 1)[:, 0, :]
    ok_arg = valid & (y_sel >= ref["out"] - 2 * ref["d_out"])
    gate = np.asarray(gate, bool)
    ok_gate = (gate == (pre_sel > 0)) | (np.abs(pre_sel) <= ref["d_out"])
    return ok_arg, ok_gate


def backward64(ref, case, arg, gate, grad_out):
    """dW [C, K], dgamma, dbeta in float64 from the reference's formulation (autograd of max, ReLU, BatchNorm over all rows,
    Linear), evaluated with the GIVEN argmax and gate, and their per-element bounds through the kernel's closed form."""
    dec, ddec, live = ref["dec"], ref["ddec"], ref["live"]
    p, t, k = dec.shape
    c = ref["x"].shape[2]
    rows, mean, inv, ga = ref["rows"], ref["mean"], ref["invstd"], ref["gamma"]
    arg = np.asarray(arg, np.int64)
    dz = np.asarray(grad_out, np.float64) * np.asarray(gate, bool)
    pad = arg < 0
    slot = np.where(pad, t - 1, arg)
    dzf = np.zeros((p, t, c))
    np.put_along_axis(dzf, slot[:, None, :], dz[:, None, :], 1)
    xhat = ref["xhat"]
    dbeta = dzf.sum((0, 1))
    dgamma = (dzf * xhat).sum((0, 1))
    dx_rows = ga * inv * (dzf - dbeta / rows - xhat * dgamma / rows)
    dw = np.einsum("ptc,ptk->ck", dx_rows, dec)
    # bounds: the closed form dW = ga inv (A - db / N S1 - dg / N inv (M - mean S1)) piece by piece
    g_sum = gamma_n(p + 4)
    adz = np.abs(dz)
    idx = slot                                                         # [P, C]
    fs = dec[np.arange(p)[:, None], idx]                               # [P, C, K]
    dfs = ddec[np.arange(p)[:, None], idx]
    xh_s = np.take_along_axis(xhat, idx[:, None, :], 1)[:, 0, :]
    dxh_s = np.take_along_axis(ref["dxhat"], idx[:, None, :], 1)[:, 0, :]
    b_db = g_sum * adz.sum(0) + TINY
    b_dg = g_sum * (adz * (np.abs(xh_s) + dxh_s)).sum(0) + (adz * dxh_s).sum(0) + U24 * np.abs(dgamma) + TINY
    a = np.einsum("pc,pck->ck", dz, fs)
    b_a = g_sum * np.einsum("pc,pck->ck", adz, np.abs(fs) + dfs) + np.einsum("pc,pck->ck", adz, dfs)
    n_sum = gamma_n(rows + 4)                                          # S1 and M run over every live row
    s1 = dec.sum((0, 1))
    b_s1 = n_sum * (np.abs(dec) + ddec).sum((0, 1)) + ddec.sum((0, 1)) + U24 * np.abs(s1)
    x, dx = ref["x"], ref["dx"]
    m = np.einsum("ptc,ptk->ck", x, dec)
    b_m = (n_sum * np.einsum("ptc,ptk->ck", np.abs(x) + dx, np.abs(dec) + ddec) + np.einsum("ptc,ptk->ck", dx, np.abs(dec) + ddec)
           + np.einsum("ptc,ptk->ck", np.abs(x), ddec) + U24 * np.abs(m))
    q = m - mean[:, None] * s1[None, :]
    b_q = b_m + ref["d_mean"][:, None] * (np.abs(s1) + b_s1)[None, :] + np.abs(mean)[:, None] * b_s1[None, :]
    dinv = ref["d_invstd"]
    t2 = dbeta[:, None] / rows * s1[None, :]
    b_t2 = (b_db[:, None] * (np.abs(s1) + b_s1)[None, :] + np.abs(dbeta)[:, None] * b_s1[None, :]) / rows
    t3 = dgamma[:, None] / rows * inv[:, None] * q
    b_t3 = (b_dg[:, None] * (inv + dinv)[:, None] * (np.abs(q) + b_q) + np.abs(dgamma)[:, None] * dinv[:, None] * (np.abs(q) + b_q)
            + np.abs(dgamma)[:, None] * inv[:, None] * b_q) / rows
    br = a - t2 - t3
    b_br = b_a + b_t2 + b_t3
    b_dw = np.abs(ga)[:, None] * (dinv[:, None] * (np.abs(br) + b_br) + inv[:, None] * b_br) + 4 * U24 * np.abs(dw) + TINY
    return dict(d_linear_weight=dw, d_norm_weight=dgamma, d_norm_bias=dbeta, b_d_linear_weight=b_dw, b_d_norm_weight=b_dg, b_d_norm_bias=b_db)


FWD_KEYS = ("mean", "invstd", "out", "running_mean", "running_var")
BWD_KEYS = ("d_linear_weight", "d_norm_weight", "d_norm_bias")


def check_train(got, case, radius, ref=None):
    """The shared comparison of the training kernels.  ``got``: mean, invstd, out, argmax, running_mean, running_var and (with
    case["grad_out"]) d_linear_weight [C, K], d_norm_weight, d_norm_bias, as arrays.  Returns {quantity: worst error / bound} with
    the decisions as 0.0 (every element accepted) or inf; a run passes when every value is <= 1."""
    ref = ref or _cached(case, ("train64", radius), lambda: train64(case, radius))
    g = {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    res = {}
    for k in FWD_KEYS:
        if k in g:
            res[k] = worst(g[k], ref[k], ref["d_" + k])
    if "argmax" in g:
        gate = np.asarray(g["out"], np.float64) > 0
        ok_arg, ok_gate = accept_decisions(ref, case, g["argmax"], gate)
        res["argmax"] = 0.0 if bool(ok_arg.all()) else float("inf")
        res["gate"] = 0.0 if bool(ok_gate.all()) else float("inf")
        if "d_norm_bias" in g and res["argmax"] == 0.0:
            bw = backward64(ref, case, g["argmax"], gate, case["grad_out"])
            for k in BWD_KEYS:
                res[k] = worst(g[k], bw[k], bw["b_" + k])
    return res


def check_train_undecided(got, case, radius):
    """check_train for a recorded node that kept neither argmax nor statistics (the training-step audit): out and the running
    statistics as above; the gradients against the float64 backward with the float64 argmax and the node's own gate, where every
    (pillar, channel) whose maximum is contested within twice its bound widens the bounds by |dz| times the spread of the contested
    rows -- the decision the node may legitimately have taken otherwise."""
    ref = _cached(case, ("train64", radius), lambda: train64(case, radius))
    g = {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float64) for k, v in got.items()}
    res = {k: worst(g[k], ref[k], ref["d_" + k]) for k in ("out", "running_mean", "running_var") if k in g}
    if "d_norm_bias" not in g:
        return res
    gate = g["out"] > 0
    arg = ref["argmax"]
    pre_sel = np.take_along_axis(ref["pre"], np.where(arg < 0, ref["live"].shape[1] - 1, arg)[:, None, :], 1)[:, 0, :]
    res["gate"] = 0.0 if bool(((gate == (pre_sel > 0)) | (np.abs(pre_sel) <= ref["d_out"])).all()) else float("inf")
    bw = backward64(ref, case, arg, gate, case["grad_out"])
    near = (ref["y"] >= (ref["out"] - 2 * ref["d_out"])[:, None, :]) & np.ones_like(ref["live"])[..., None]       # [P, T, C] contested slots
    adz = np.abs(np.asarray(case["grad_out"], np.float64)) * gate
    dec, xhat = ref["dec"], ref["xhat"]
    p = dec.shape[0]
    slot = np.where(arg < 0, ref["live"].shape[1] - 1, arg)
    fs = dec[np.arange(p)[:, None], slot]                               # [P, C, K]
    xs = np.take_along_axis(xhat, slot[:, None, :], 1)[:, 0, :]
    spread_f = np.zeros_like(fs)
    spread_x = np.zeros_like(xs)
    for pi, ci in zip(*np.nonzero(near.sum(1) > 1)):
        ts = np.nonzero(near[pi, :, ci])[0]
        spread_f[pi, ci] = np.abs(dec[pi, ts] - fs[pi, ci]).max(0)
        spread_x[pi, ci] = np.abs(xhat[pi, ts, ci] - xs[pi, ci]).max()
    # another contested row moves A[c][j] by |dz| spread_f and dgamma by |dz| spread_xhat; dgamma enters dW through
    # dgamma / N invstd (M - mean S1), and |M - mean S1| / N <= mean|x - mean| max|f_j|
    extra_dg = (adz * spread_x).sum(0)
    scale = np.abs(ref["gamma"]) * ref["invstd"]
    extra_dw = scale[:, None] * (np.einsum("pc,pck->ck", adz, spread_f)
                                 + extra_dg[:, None] * ref["invstd"][:, None] * np.abs(ref["x"] - ref["mean"]).mean((0, 1))[:, None]
                                 * np.abs(dec).max((0, 1))[None, :])
    res["d_norm_bias"] = worst(g["d_norm_bias"], bw["d_norm_bias"], bw["b_d_norm_bias"])
    res["d_norm_weight"] = worst(g["d_norm_weight"], bw["d_norm_weight"], bw["b_d_norm_weight"] + extra_dg)
    res["d_linear_weight"] = worst(g["d_linear_weight"], bw["d_linear_weight"], bw["b_d_linear_weight"] + extra_dw)
    return res


def trim_slots(case):
    """The case with ``vox`` cut to the slots that can matter -- the live ones and one padded slot (all padded slots are the same zero
    row) -- and case["slots"] = T: the float64 arrays are [P, T', C] instead of [P, T, C]."""
    t = case["vox"].shape[1]
    keep = min(t, int(np.max(case["num"], initial=0)) + 1)
    return dict({k: v for k, v in case.items() if not isinstance(k, tuple)}, vox=np.ascontiguousarray(case["vox"][:, :keep]), slots=t)


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernels
def emulate32(case, radius, mode, bug=None):
    """The kernels' arithmetic in float32 numpy (another summation order, the same formulas), with one planted mistake ``bug``.
    mode "eval" -> out [P, C]; "train" -> the dict check_train takes (gradients included when the case has grad_out)."""
    f = np.float32
    v = np.asarray(case["vox"], f)
    n = np.asarray(case["num"], np.int64)
    p, t, _ = v.shape
    vx, vy, xo, yo = (f(g) for g in case["geom"])
    live = np.arange(t)[None, :] < n[:, None]
    xyz = v[..., :3]
    mean_p = xyz.sum(1, dtype=f) / (f(t) if bug == "mean_div_T" else n.astype(f)[:, None])
    co = np.asarray(case["coords"])
    cx = co[:, 2 if bug == "centre_col" else 3].astype(f) * vx + xo
    cy = co[:, 2].astype(f) * vy + yo
    if radius:
        r = v[..., 0:1] if bug == "radius_x" else np.sqrt(v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2], dtype=f)
        head = np.concatenate([r, v[..., 2:]], -1)
    else:
        head = v
    dec = np.concatenate([head, xyz - mean_p[:, None, :], (v[..., 0] - cx[:, None])[..., None], (v[..., 1] - cy[:, None])[..., None]], -1)
    dec = (dec * live[..., None]).astype(f)
    wt = np.asarray(_wt(case, radius), f)
    x = (dec @ wt).astype(f)
    use = live if bug == "pad_out_of_max" else np.ones_like(live)
    if mode == "eval":
        y = np.maximum(x * np.asarray(case["scale"], f) + np.asarray(case["shift"], f), f(0))
        out = np.where(use[..., None], y, -np.inf).max(1).astype(f)
        live_rows = case.get("num_dev")
        if live_rows is not None:
            keep = out.copy()
            out = np.full_like(out, case["sentinel"])
            m = p if bug == "num_dev_ignored" else min(int(live_rows), p)
            out[:m] = keep[:m]
        return out
    rows = f(live.sum()) if bug == "n_live" else f(p * t)
    k = dec.shape[2]
    c = x.shape[2]
    mean = (x.sum((0, 1), dtype=np.float64) / rows).astype(f)
    var = (((x - mean) ** 2).sum((0, 1), dtype=np.float64) / rows)
    if bug == "n_live":
        var = (x.astype(np.float64) ** 2).sum((0, 1)) / rows - mean.astype(np.float64) ** 2
    var_u = var * (rows / (rows - 1) if rows > 1 else 1.0)
    eps, mom = float(case["eps"]), float(case["momentum"])
    inv = (1.0 / np.sqrt((var_u if bug == "unbiased_norm" else var) + eps)).astype(f)
    ga, be = np.asarray(case["gamma"], f), np.asarray(case["beta"], f)
    rm = ((1 - mom) * np.asarray(case["rm0"], np.float64) + mom * mean).astype(f)
    rv = ((1 - mom) * np.asarray(case["rv0"], np.float64) + mom * (var if bug == "rv_biased" else var_u)).astype(f)
    xhat = ((x - mean) * inv).astype(f)
    y = np.maximum(xhat * ga + be, f(0)).astype(f)
    ym = np.where(use[..., None], y, -np.inf)
    out = ym.max(1).astype(f)
    arg = ym.argmax(1)
    arg = np.where(arg >= n[:, None], -1, arg)
    got = dict(mean=mean, invstd=inv, out=out, argmax=arg, running_mean=rm, running_var=rv)
    if case.get("grad_out") is None:
        return got
    g = np.asarray(case["grad_out"], f)
    dz = g * ((g > 0) if bug == "gate_from_grad" else (out > 0))
    slot = np.where(arg < 0, t - 1, arg)
    fs = dec[np.arange(p)[:, None], slot]
    xs = np.take_along_axis(xhat, slot[:, None, :], 1)[:, 0, :]
    db = dz.sum(0, dtype=np.float64)
    dg = (dz * xs).sum(0, dtype=np.float64)
    a = np.einsum("pc,pck->ck", dz, fs).astype(np.float64)
    s1 = dec.sum((0, 1), dtype=np.float64).astype(f).astype(np.float64)
    m = np.einsum("ptc,ptk->ck", x, dec).astype(f).astype(np.float64)
    if bug == "m_transposed":
        m = m.reshape(-1).reshape(k, c).T.copy()                   # M[c][j] read at [j * C + c]
    if bug == "no_s1":
        s1 = np.zeros_like(s1)
    i64, m64 = inv.astype(np.float64), mean.astype(np.float64)
    dw = ga.astype(np.float64)[:, None] * i64[:, None] * (a - db[:, None] / rows * s1[None, :]
                                                           - dg[:, None] / rows * i64[:, None] * (m - m64[:, None] * s1[None, :]))
    got.update(d_linear_weight=dw.astype(f), d_norm_weight=dg.astype(f), d_norm_bias=db.astype(f))
    return got


# ------------------------------------------------------------------------------------------------ input generators
POINT_SETS = ("centred", "far", "axis", "single", "duplicated", "intensity255", "full")
PARAM_SETS = ("plain", "negative_scale", "pad_wins", "dead_channel")


def pillars(p, t, kind="far", seed=0):
    """[P, T, 4] float32 pillars, counts [P] and coords [P, 4] (b, z, y, x) on the 0.25 m grid of GEOM.
    centred: points in +-3 m around the sensor;  far: pillars anywhere on the +-50 m grid (|x|, |y| up to 50 m: x - mean cancels);
    axis: far, pillar 0 at the sensor axis with its first point at x = y = 0 (r = 0);  single: every pillar holds one point
    (x - mean is exactly 0);  duplicated: every pillar repeats one point;  intensity255: far with the fourth feature in 0 .. 255;
    full: far with n = T everywhere (no padded slot).  Every other kind: counts 1 .. T, every seventh pillar full, pillar 1 (where
    there is one) a single point."""
    rng = np.random.default_rng(seed * 7919 + p * 131 + t)
    n = rng.integers(1, t + 1, p)
    n[::7] = t
    if p > 1:
        n[1] = 1
    if kind == "single":
        n[:] = 1
    if kind == "full":
        n[:] = t
    lo, hi = (188, 212) if kind == "centred" else (0, 400)
    cy, cx = rng.integers(lo, hi, p), rng.integers(lo, hi, p)
    if kind == "far" and p > 1:
        cy[-1], cx[-1] = 399, 0                                          # a corner pillar: |x|, |y| ~ 50 m
    if kind == "axis":
        cy[0], cx[0] = 200, 200
    coords = np.stack([np.zeros(p, np.int64), np.zeros(p, np.int64), cy, cx], 1).astype(np.int32)
    vox = np.zeros((p, t, 4), np.float32)
    vox[..., 0] = -50.0 + (cx[:, None] + rng.uniform(0.02, 0.98, (p, t))) * 0.25
    vox[..., 1] = -50.0 + (cy[:, None] + rng.uniform(0.02, 0.98, (p, t))) * 0.25
    vox[..., 2] = rng.uniform(-3, 1, (p, t))
    vox[..., 3] = rng.uniform(0, 255, (p, t)) if kind == "intensity255" else rng.uniform(0, 1, (p, t))
    if kind == "axis":
        vox[0, 0, 0] = vox[0, 0, 1] = 0.0
    if kind == "duplicated":
        vox[:] = vox[:, :1]
    vox *= (np.arange(t)[None, :] < n[:, None])[..., None]
    return vox, n.astype(np.int32), coords


def eval_case(p, t, c, points="far", params="plain", seed=0):
    """An inference case.  params: plain (scale 0.5 .. 1.5, shift +-0.3); negative_scale (every third channel's scale negated);
    pad_wins (channel 0: shift high enough that relu(shift) of the padded slot beats every live point); dead_channel (channel
    C - 1: shift low enough that every slot is exactly 0)."""
    vox, num, coords = pillars(p, t, points, seed)
    rng = np.random.default_rng(seed + 1000 * c + t)
    k_w = 3.0 * (40.0 if points == "intensity255" else 1.0)
    wt9 = (rng.standard_normal((9, c)) / 3).astype(np.float32)
    wt9[3] /= np.float32(k_w / 3.0)
    scale, shift = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
    if params == "negative_scale":
        scale[::3] *= -1
    if params == "pad_wins":
        wt9[:, 0] = 0
        wt9[3, 0] = 0.3                                 # x = 0.3 w >= 0 (w is row 3 of the nine-entry and row 2 of the radius row)
        scale[0], shift[0] = -abs(scale[0]), 2.0        # y = shift - |scale| x <= shift = the padded slot's value
    case = dict(vox=vox, num=num, coords=coords, geom=GEOM, scale=scale, shift=shift, wt9=wt9, params=params, points=points)
    if params == "dead_channel":
        hi = max(float(np.abs(linear64(*decorate64(vox, num, coords, GEOM, r)[:2], _wt(case, r))[0][..., c - 1]).max()) for r in (False, True))
        shift[c - 1] = -(hi * abs(scale[c - 1]) * 1.5 + 1.0)        # below every slot's -x * scale: the whole channel is exactly 0
    return case


# (P, T, C, points, params): every T, C and P of the kernel's boundaries at least once -- T on both sides of the one / two pass mean
# loop (64), C on both sides of one / two channel passes (64, 65, 128) and lanes idle (1, 16, 48), P around the four waves of a
# workgroup (3, 4, 5) -- with every point set and parameter set
EVAL_CASES = [
    (1, 1, 1, "single", "plain"), (3, 5, 16, "centred", "plain"), (4, 63, 48, "far", "negative_scale"), (5, 64, 64, "axis", "pad_wins"),
    (33, 65, 65, "far", "dead_channel"), (33, 100, 96, "intensity255", "plain"), (4, 127, 128, "duplicated", "negative_scale"),
    (5, 128, 64, "full", "plain"), (3, 200, 65, "far", "pad_wins"), (700, 60, 64, "far", "plain"), (700, 5, 16, "single", "dead_channel"),
    (33, 64, 128, "full", "pad_wins"), (33, 63, 1, "axis", "plain"), (5, 65, 48, "centred", "dead_channel"), (33, 200, 128, "intensity255", "negative_scale"),
]
EVAL_T = (1, 5, 63, 64, 65, 100, 127, 128, 200)
EVAL_C = (1, 16, 48, 64, 65, 96, 128)
EVAL_P = (1, 3, 4, 5, 33, 700)
SLOT_T = (5, 8, 9, 64, 65, 100, 200)


def train_case(p, t, c, variant="plain", seed=0, bias=(-0.3, 0.3)):
    """A training case: pillars, weights, gamma 0.5 .. 1.5, beta in ``bias``, running statistics, grad_out.  variant:
    full (n = T everywhere), zero_weight (channel 0 has no weight: var = 0, invstd = eps ** -0.5), gamma0 (gamma[1] = 0), pad_wins
    (channel 2: gamma < 0 on an always-positive x far above its mean ... the padded zero row wins in every ragged pillar),
    zero_grad_rows (every third row of grad_out zero), offset (the cloud sits in x in [60, 70], intensity in 200 .. 255, every
    pillar full; channel 0 weighs x only, channel 1 the intensity only)."""
    kind = "full" if variant in ("full", "offset") else "axis"
    vox, num, coords = pillars(p, t, kind, seed + 17)
    rng = np.random.default_rng(seed + 31 * c + t + p)
    geom = GEOM
    if variant == "offset":
        cx = rng.integers(440, 480, p)                               # x in [60, 70] on the same 0.25 m grid (the kernels take any cell)
        coords[:, 3] = cx
        vox[..., 0] = (-50.0 + (cx[:, None] + rng.uniform(0.02, 0.98, (p, t))) * 0.25).astype(np.float32)
        vox[..., 3] = rng.uniform(200, 255, (p, t)).astype(np.float32)
    if t == 127:
        vox[0, t - 1, 2] = 6.0                                       # pillar 0 is full: its last slot, 126, the end of the int8 argmax, wins where z weighs in
    wt9 = rng.uniform(-0.35, 0.35, (9, c)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(*bias, c).astype(np.float32)
    if variant == "offset":
        wt9[3] /= 64
        wt9[:, 0] = 0
        wt9[0, 0] = 0.3
        wt9[:, 1] = 0
        wt9[3, 1] = 0.01
    if variant == "zero_weight":
        wt9[:, 0] = 0
    if variant == "gamma0":
        gamma[1] = 0
    if variant == "pad_wins":
        wt9[:, 2] = 0
        wt9[2, 2], wt9[3, 2] = 0.0, -0.3                             # x = -0.3 w <= 0 with w in [0, 1]: the zero row is the largest
        gamma[2], beta[2] = 1.0, 0.5
    g = rng.standard_normal((p, c)).astype(np.float32)
    if variant == "zero_grad_rows":
        g[::3] = 0
    return dict(vox=vox, num=num, coords=coords, geom=geom, wt9=wt9, gamma=gamma, beta=beta, eps=EPS, momentum=MOMENTUM,
                rm0=rng.uniform(-0.5, 0.5, c).astype(np.float32), rv0=rng.uniform(0.5, 2.0, c).astype(np.float32), grad_out=g, variant=variant)


# the CASES of tests/test_gpu_mhead_train.py, then: the smallest P above 1024 blocks x 4 waves (grid-stride loop), C = 33, all full,
# a zero-weight channel, a gamma = 0 channel, a channel the padded slot always wins, zero rows in grad_out, the offset cloud
TRAIN_CASES = [(1, 2, 64, "plain", (-0.3, 0.3)), (33, 5, 64, "plain", (-0.3, 0.3)), (3, 127, 64, "plain", (-0.3, 0.3)),
               (700, 60, 64, "plain", (-0.3, 0.3)), (5000, 20, 64, "plain", (-0.3, 0.3)), (700, 60, 16, "plain", (-0.3, 0.3)),
               (33, 5, 16, "plain", (-0.3, 0.3)), (33, 5, 64, "plain", (2.0, 4.0)), (4100, 20, 64, "plain", (-0.3, 0.3)),
               (700, 60, 33, "plain", (-0.3, 0.3)), (33, 8, 64, "full", (-0.3, 0.3)), (33, 5, 64, "zero_weight", (-0.3, 0.3)),
               (33, 5, 64, "gamma0", (-0.3, 0.3)), (65, 9, 64, "pad_wins", (-0.3, 0.3)), (33, 5, 64, "zero_grad_rows", (-0.3, 0.3)),
               (700, 32, 64, "offset", (-0.3, 0.3))]


# ------------------------------------------------------------------------------------------------ exact cases
PYTHAGOREAN = ((3, 4), (4, 3), (5, 12), (12, 5), (8, 15), (15, 8), (0, 0), (6, 8), (9, 12), (0, 5), (7, 24), (20, 21))


def exact_eval_case(p=9, t=12, c=64, seed=0):
    """Every fp32 intermediate exact: points on a 1/8 m lattice with Pythagorean (x, y) pairs (so the radius is an integer multiple
    of 1/8 too), counts powers of two, integer weights in -2 .. 2, scale +-2^k, integer shift: out must be bit-equal to float64."""
    rng = np.random.default_rng(seed)
    num = np.array([1, 2, 4, 8][: min(4, p)] * p, np.int32)[:p]
    num = np.minimum(num, 1 << int(np.log2(t))).astype(np.int32)
    if p > 4:
        num[4] = 1 << int(np.log2(t))
    coords = np.stack([np.zeros(p, np.int64), np.zeros(p, np.int64), rng.integers(0, 400, p), rng.integers(0, 400, p)], 1).astype(np.int32)
    vox = np.zeros((p, t, 4), np.float32)
    pick = rng.integers(0, len(PYTHAGOREAN), (p, t))
    sign = rng.choice([-1.0, 1.0], (p, t, 2))
    xy = np.array(PYTHAGOREAN, np.float32)[pick] * sign / 8
    vox[..., :2] = xy
    vox[..., 2] = rng.integers(-16, 8, (p, t)) / 8
    vox[..., 3] = rng.integers(0, 8, (p, t))
    vox *= (np.arange(t)[None, :] < num[:, None])[..., None]
    wt9 = rng.integers(-2, 3, (9, c)).astype(np.float32)
    scale = (rng.choice([-1.0, 1.0], c) * 2.0 ** rng.integers(-2, 3, c)).astype(np.float32)
    shift = rng.integers(-4, 5, c).astype(np.float32)
    return dict(vox=vox, num=num, coords=coords, geom=GEOM, wt9=wt9, scale=scale, shift=shift)


def exact_train_fwd_case(radius, p=8, t=8, c=64):
    """k_pfn_stats / _finalize / _fwd_train with every intermediate exact: all pillars full and in ONE cell, each point offset by
    +-1 (nine-entry row) from the cell centre in x, y, z and by +-1 in w in balanced patterns, so that every decorated column takes
    two values, half the rows each; channel c weighs one column by +-1 (+-0.5 where the column moves by +-2).  Then mean_c is
    dyadic, var_c = 1 exactly, and with eps = 3 invstd = 0.5; gamma = +-2^k, beta integer."""
    k = _k(radius)
    coords = np.tile(np.array([[0, 0, 180, 220]], np.int32), (p, 1))          # centre (5.125, -4.875)
    cx, cy = 220 * 0.25 - 49.875, 180 * 0.25 - 49.875
    ts = np.arange(t)
    ps = np.arange(p)[:, None]
    s = lambda d: (1.0 - 2.0 * (((ts[None, :] >> d) + ps) & 1))               # balanced within every pillar (t a multiple of 8)
    vox = np.zeros((p, t, 4), np.float32)
    if radius:
        # (x, y) in {(5, 12), (9, 12)}: r in {13, 15}; x - mean = -+2, x - cx = x - 5.125
        vox[..., 0] = 7 + 2 * s(0)
        vox[..., 1] = 12
        step = np.array([1, 1, 1, 2, 0, 1, 2, 0], np.float64)                # movement of each column: 0 = constant (unused)
    else:
        vox[..., 0] = cx + s(0)
        vox[..., 1] = cy + s(1)
        step = np.ones(9)
    vox[..., 2] = -1 + s(2)
    vox[..., 3] = 3 + s(1 if radius else 0) * s(2)
    cols = [j for j in range(k) if step[j] > 0]
    wt = np.zeros((k, c), np.float32)
    for ch in range(c):
        j = cols[ch % len(cols)]
        wt[j, ch] = (1.0 if (ch // len(cols)) % 2 == 0 else -1.0) / step[j]
    gamma = (np.where(np.arange(c) % 3 == 0, -1.0, 1.0) * 2.0 ** (np.arange(c) % 4 - 1)).astype(np.float32)
    beta = ((np.arange(c) % 5) - 2).astype(np.float32)
    return dict(vox=vox, num=np.full(p, t, np.int32), coords=coords, geom=GEOM, wt=wt, gamma=gamma, beta=beta, eps=3.0, momentum=0.25,
                rm0=np.arange(c, dtype=np.float32) % 4, rv0=np.full(c, 4.0, np.float32), grad_out=None)


def exact_train_bwd_case(radius, p=8, t=8, c=64, seed=3):
    """sec_pfn_train_bwd / sec_pfn_radius_train_bwd on hand-made stats, argmax and out: points on the 1/8 lattice (Pythagorean
    pairs), integer weights, integer mean[c], invstd[c] = 2^-k, distinct integers M[c][j] and S1[j], integer grad_out, N = P * T a
    power of two: dbeta, dgamma and every dW[c][j] are exact.  Returns the case with ``stats`` (mean[C], invstd[C], M[C][K], S1[K],
    flat), ``argmax`` int8 [P, C] (-1 where the pillar is ragged, slots otherwise), ``out`` (its sign is the gate) and the float64
    results ``want``."""
    k = _k(radius)
    e = exact_eval_case(p, t, c, seed)
    rng = np.random.default_rng(seed + 5)
    num = e["num"].astype(np.int64)
    wt = (e["wt9"][1:] if radius else e["wt9"]).copy()
    mean = rng.integers(-3, 4, c).astype(np.float64)
    inv = 2.0 ** -rng.integers(0, 3, c).astype(np.float64)
    m = (rng.permutation(c * k).reshape(c, k) - c * k // 2).astype(np.float64) * 8
    s1 = (rng.permutation(k) + 1).astype(np.float64) * 16
    gamma = (rng.choice([-1.0, 1.0], c) * 2.0 ** rng.integers(-1, 2, c))
    arg = rng.integers(0, 1 << 20, (p, c)) % num[:, None]
    arg = np.where((rng.random((p, c)) < 0.2) & (num[:, None] < t), -1, arg)
    out = np.where(rng.random((p, c)) < 0.3, 0.0, 1.5)
    g = rng.integers(-3, 4, (p, c)).astype(np.float64)
    dec = decorate64(e["vox"], e["num"], e["coords"], GEOM, radius)[0]
    rows = float(p * t)
    dz = g * (out > 0)
    slot = np.where(arg < 0, 0, arg)
    fs = dec[np.arange(p)[:, None], slot] * (arg >= 0)[..., None]
    xs = np.einsum("pck,kc->pc", fs, wt.astype(np.float64))
    db = dz.sum(0)
    dg = (dz * (xs - mean) * inv).sum(0)
    a = np.einsum("pc,pck->ck", dz, fs)
    dw = gamma[:, None] * inv[:, None] * (a - db[:, None] / rows * s1[None, :] - dg[:, None] / rows * inv[:, None] * (m - mean[:, None] * s1[None, :]))
    stats = np.concatenate([mean, inv, m.reshape(-1), s1]).astype(np.float32)
    want = dict(d_linear_weight=dw, d_norm_weight=dg, d_norm_bias=db)
    for v in want.values():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)      # representable: bit-equality is meaningful
    return dict(vox=e["vox"], num=e["num"], coords=e["coords"], geom=GEOM, wt=wt, gamma=gamma.astype(np.float32), stats=stats,
                argmax=arg.astype(np.int8), out=out.astype(np.float32), grad_out=g.astype(np.float32), want=want)


# ------------------------------------------------------------------------------------------------ pillar scatter
def scatter64(feat, coords, batch, ny, nx, live=None):
    """PointPillarsScatter restated: out[b, :, y, x] = feat[i] for the first ``live`` pillars, zero elsewhere (dtype kept)."""
    f = np.asarray(feat)
    n = f.shape[0] if live is None else max(0, min(int(live), f.shape[0]))
    out = np.zeros((batch, f.shape[1], ny, nx), f.dtype)
    co = np.asarray(coords)
    out[co[:n, 0], :, co[:n, 2], co[:n, 3]] = f[:n]
    return out


def gather64(dense, coords, live=None):
    d = np.asarray(dense)
    co = np.asarray(coords)
    n = co.shape[0] if live is None else max(0, min(int(live), co.shape[0]))
    return d[co[:n, 0], :, co[:n, 2], co[:n, 3]]


def scatter_case(p, c, batch=2, ny=12, nx=10, seed=0):
    """Distinct cells for p pillars of c channels (values exactly representable in bf16 and fp16: small integers / 4)."""
    rng = np.random.default_rng(seed + p + c)
    cells = rng.permutation(batch * ny * nx)[:p]
    coords = np.stack([cells // (ny * nx), np.zeros(p, np.int64), cells // nx % ny, cells % nx], 1).astype(np.int32)
    feat = (rng.integers(-64, 64, (p, c)) / 4).astype(np.float32)
    feat[feat == 0] = 0.25                                     # so that a landed row differs from the zero fill everywhere
    return feat, coords, batch, ny, nx
