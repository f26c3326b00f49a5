"""Produces tests/golden/train_metrics.npz by EXECUTING the reference's ``VoxelNet.update_metrics``
(second/pytorch/models/voxelnet.py:654-679) on CPU tensors.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_train_metrics.py [path to the reference checkout]

The method runs unbound on a small holder object that carries the two attributes it reads (``_num_class``,
``_encode_background_as_zeros``) and REAL torchplus.metrics modules, built as VoxelNet.__init__ builds them (voxelnet.py:172-183).

Each case is a sequence of three updates on one set of modules with B = 2; the state buffers and the returned dict are recorded
after every update.  Cases (C, N, label dtype, thresholds):
  A   1  4099  int32  default seven   plain; a zero cls loss in the middle (skipped); plain              logits stored as float16
  B   2   255  int64  default         both losses zero first (value NaN); every label -1; plain
  C   2   256  int32  sixteen         no positives; plain; every score below 0.1
  D  10   257  int64  default         NaN logits (alone, beside a class above 0.5, a whole row); logits of exactly 0; plain
  E   1     1  int32  one (0.5)       a positive above the threshold; label -1; a negative with logit 0
  F  10     1  int64  default         plain
  G   1   257  int64  default         ``cared`` differs from labels >= 0; NaN and zero logits with one class; a NaN loss
Labels: about 10 % -1, 5 % positive (their class gets +2.5), the rest 0.  Logits N(0, 2).

Admission: every sigmoid is taken in float64; a logit whose sigmoid lies within 2^-20 of a threshold in use (Accuracy's 0.5 included)
is REPLACED by a fresh draw, and so is a logit that ties the maximum of a multi-class row; the logits placed at exactly 0 on purpose
are exempt (their sigmoid is exactly 0.5 in any arithmetic, and ``> 0.5`` is false).  The number replaced is recorded and has to
stay below 1 % of all logits -- expected share about 1e-5.  The numpy restatement and the torch stand-in of
tests/train_metrics_helpers.py are checked against what was just recorded."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
B = 2
SIXTEEN = [round(0.05 * (i + 1), 2) for i in range(16)]


def draw(rng, n, c, half):
    x = rng.normal(0.0, 2.0, (B, n, c)).astype(np.float32)
    return x.astype(np.float16).astype(np.float32) if half else x


def make_labels(rng, n, c, x):
    u = rng.uniform(size=(B, n))
    lab = np.zeros((B, n), np.int64)
    lab[u < 0.10] = -1
    posm = u > 0.95
    lab[posm] = rng.integers(1, c + 1, int(posm.sum()))
    b, i = np.nonzero(posm)
    x[b, i, lab[b, i] - 1] += np.float32(2.5)
    return lab


def admit(rng, x, thresholds, keep_zero, half, counter):
    """Replace in place what the admission rule refuses; -> number replaced."""
    import train_metrics_helpers as H
    thr = np.array(sorted(set([np.float64(np.float32(t)) for t in thresholds] + [0.5])))
    for _ in range(100):
        s = H.sigmoid64(x)
        near = (np.abs(s[..., None] - thr) < H.MARGIN).any(-1) & ~np.isnan(x)
        if keep_zero is not None:
            near &= ~(keep_zero & (x == 0))
        tie = np.zeros_like(near)
        if x.shape[-1] > 1:
            real = np.where(np.isnan(x), -np.inf, x)
            mx = real.max(-1, keepdims=True)
            at = (real == mx) & np.isfinite(mx)
            if keep_zero is not None:
                at &= ~keep_zero                                  # rows placed at 0 on purpose tie on purpose only where stated below
            many = at.sum(-1, keepdims=True) > 1
            first = np.cumsum(at, -1) == 1
            tie = at & many & ~first                              # every tied entry but the first is redrawn
        bad = near | tie
        if not bad.any():
            return
        counter[0] += int(bad.sum())
        fresh = rng.normal(0.0, 2.0, int(bad.sum())).astype(np.float32)
        x[bad] = fresh.astype(np.float16).astype(np.float32) if half else fresh
    raise AssertionError("admission did not settle")


def build_cases():
    rng = np.random.default_rng(20261019)
    f = np.float32
    cases, counter, total = {}, [0], 0

    def update(n, c, kind, thresholds, half=False):
        x = draw(rng, n, c, half)
        lab = make_labels(rng, n, c, x)
        keep_zero, cared = None, None
        if kind == "all_ignored":
            lab[:] = -1
        elif kind == "no_positives":
            lab[lab > 0] = 0
        elif kind == "low_scores":
            x[:] = -np.abs(x) - f(3.0)                               # sigmoid(-3) = 0.047
        elif kind == "nan":
            rows = rng.choice(n, size=min(n, 24), replace=False)
            keep_zero = np.zeros(x.shape, bool)
            for j, r in enumerate(rows):
                if c == 1 or j % 3 == 0:
                    x[j % B, r, rng.integers(0, c)] = np.nan             # alone: the other classes as drawn
                elif j % 3 == 1:
                    k = int(rng.integers(0, c))                          # a NaN right behind / in front of a class far above 0.5
                    k2 = (k + 1) % c if j % 2 else (k - 1) % c
                    x[j % B, r, k], x[j % B, r, k2] = np.nan, f(4.0)
                    lab[j % B, r] = (k + 1, k2 + 1, 0, -1)[(j // 3) % 4]
                    continue
                else:
                    x[j % B, r, :] = np.nan                              # a whole row
                lab[j % B, r] = (0, 1, min(2, c), -1)[j % 4]
        elif kind == "zeros":
            keep_zero = np.zeros(x.shape, bool)
            rows = rng.choice(n, size=min(n, 24), replace=False)
            for j, r in enumerate(rows):
                if c == 1 or j % 2 == 0:
                    k = int(rng.integers(0, c))
                    x[j % B, r, :] = -np.abs(x[j % B, r, :]) - f(0.5)    # the maximum is the one logit at exactly 0
                    x[j % B, r, k] = 0.0
                    keep_zero[j % B, r, k] = True
                    lab[j % B, r] = (0, k + 1, -1)[j % 3]
        if kind == "cared":
            cared = rng.uniform(size=(B, n)) < 0.7                       # not labels >= 0: ignored anchors counted, cared ones left out
            x[0, :8, 0] = np.nan
            keep_zero = np.zeros(x.shape, bool)
            x[1, :8, 0] = 0.0
            keep_zero[1, :8, 0] = True
            lab[1, :8] = (0, 1, 0, 1, -1, 0, 1, 0)
        if half:
            x[:] = x.astype(np.float16).astype(np.float32)
        admit(rng, x, thresholds, keep_zero, half, counter)
        return x, lab, cared

    def case(name, c, n, dtype, thresholds, kinds, losses, half=False):
        nonlocal total
        ups = []
        for kind, (cl, ll) in zip(kinds, losses):
            x, lab, cared = update(n, c, kind, thresholds, half)
            total += x.size
            ups.append(dict(logits=x, labels=lab.astype(dtype), cared=cared, cls_loss=f(cl), loc_loss=f(ll)))
        cases[name] = dict(C=c, N=n, B=B, label_dtype=dtype, thresholds=list(thresholds), half=half, updates=ups)

    D7 = [0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95]
    case("A", 1, 4099, "int32", D7, ("plain", "plain", "plain"), ((0.8125, 1.7), (0.0, 1.3), (0.61, 0.9)), half=True)
    case("B", 2, 255, "int64", D7, ("plain", "all_ignored", "plain"), ((0.0, 0.0), (0.0, 0.4), (0.3, 0.0)))
    case("C", 2, 256, "int32", SIXTEEN, ("no_positives", "plain", "low_scores"), ((1.1, 2.2), (0.9, 1.8), (0.7, 1.4)))
    case("D", 10, 257, "int64", D7, ("nan", "zeros", "plain"), ((0.5, 0.25), (0.125, 3.0), (1e-3, 1e3)))
    case("E", 1, 1, "int32", [0.5], ("plain", "plain", "plain"), ((0.2, 0.3), (0.4, 0.0), (0.1, 0.6)))
    cases["E"]["updates"][0]["logits"][:] = np.float32([[[1.5]], [[-0.75]]]); cases["E"]["updates"][0]["labels"][:] = [[1], [0]]
    cases["E"]["updates"][1]["logits"][:] = np.float32([[[2.0]], [[2.0]]]); cases["E"]["updates"][1]["labels"][:] = [[-1], [-1]]
    cases["E"]["updates"][2]["logits"][:] = np.float32([[[0.0]], [[0.25]]]); cases["E"]["updates"][2]["labels"][:] = [[0], [1]]
    case("F", 10, 1, "int64", D7, ("plain", "plain", "plain"), ((0.2, 0.3), (0.4, 0.5), (0.1, 0.6)))
    case("G", 1, 257, "int64", D7, ("cared", "cared", "zeros"), ((0.5, 0.5), (float("nan"), 0.25), (0.75, 0.5)))
    return cases, counter[0], total


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT, os.path.join(ROOT, "tests")]
    import torch
    import train_metrics_helpers as H
    from second_amd import compat
    compat.install(ref)
    from second.pytorch.models.voxelnet import VoxelNet
    from torchplus import metrics

    cases, replaced, total = build_cases()
    share = replaced / total
    print("logits", total, "replaced", replaced, "share", share)
    assert share < 0.01, "the admission rule replaced 1 % of the logits or more: a bug in the generator"

    out = {}
    meta = {"cases": {}, "replaced": replaced, "logits": total, "margin": H.MARGIN, "state_order": list(H.STATE)}
    for name, c in cases.items():
        thr, t = c["thresholds"], len(c["thresholds"])

        def ref_modules():
            return {"rpn_acc": metrics.Accuracy(dim=-1, encode_background_as_zeros=True),
                    "rpn_metrics": metrics.PrecisionRecall(dim=-1, thresholds=thr, use_sigmoid_score=True, encode_background_as_zeros=True),
                    "rpn_cls_loss": metrics.Scalar(), "rpn_loc_loss": metrics.Scalar()}
        real = H.holder(c["C"], thr, ref_modules())               # real modules; the method below is the reference's, unbound
        standin = H.holder(c["C"], thr)
        mine = H.zero_state(t)
        for k, u in enumerate(c["updates"]):
            cared = (u["labels"] >= 0) if u["cared"] is None else u["cared"]
            args = lambda: (torch.tensor(u["cls_loss"]), torch.tensor(u["loc_loss"]), torch.from_numpy(u["logits"].copy()),
                            torch.from_numpy(u["labels"].copy()), torch.from_numpy(cared.copy()))
            ret = VoxelNet.update_metrics(real, *args())
            state = H.state_vector({kk: v.numpy() for kk, v in H.net_state(real).items()})
            vec = H.ret_vector(ret, thr)
            p = f"{name}/u{k}/"
            out[p + "logits"] = u["logits"].astype(np.float16) if c["half"] else u["logits"]
            assert np.array_equal(out[p + "logits"].astype(np.float32), u["logits"], equal_nan=True)
            out[p + "labels"] = u["labels"].astype(np.int8)
            if u["cared"] is not None:
                out[p + "cared"] = u["cared"].astype(np.uint8)
            out[p + "losses"] = np.array([u["cls_loss"], u["loc_loss"]], np.float32)
            out[p + "state"], out[p + "ret"] = state, vec
            # the two restatements against what was just recorded
            r2 = H.restate(mine, u["cls_loss"], u["loc_loss"], u["logits"], u["labels"], u["cared"], thr)
            assert H.same(H.state_vector(mine), state) and H.same(H.ret_vector(r2, thr), vec), (name, k, "numpy restatement")
            r3 = standin.update_metrics(*args())
            s3 = H.state_vector({kk: v.numpy() for kk, v in H.net_state(standin).items()})
            assert H.same(s3, state) and H.same(H.ret_vector(r3, thr), vec), (name, k, "torch stand-in")
            print(name, k, "acc", ret["rpn_acc"], "cls", ret["loss"]["cls_loss"], "prec/rec", vec[5:5 + t][:3], vec[5 + t:][:3])
        meta["cases"][name] = {kk: c[kk] for kk in ("C", "N", "B", "label_dtype", "thresholds")}
        meta["cases"][name]["updates"] = len(c["updates"])
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "train_metrics.npz")
    H.save_npz(path, out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
