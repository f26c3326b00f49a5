"""Helpers for the training-metrics tests (tests/golden/train_metrics.npz, sec_train_metrics_f32).

* ``restate`` -- VoxelNet.update_metrics (voxelnet.py:654-679) with torchplus/metrics.py Accuracy, PrecisionRecall and Scalar, restated
  in numpy from their formulas: decisions from float64 sigmoids (the fixture keeps every one of them 2^-20 from a threshold, so
  float32 and float64 decide alike), the state arithmetic in float32 in the reference's order.  tests/test_train_metrics_host.py
  holds it to the fixture exactly, so the GPU tests can use it where no fixture exists (a tied maximum, the grid-stride sizes).
* ``attach_metrics`` -- gives a network object (the stand-in VoxelNet of tests/reference_standin.py, or the bare ``Holder``) metric
  modules under the reference's attribute and buffer names, plus ``update_metrics`` / ``clear_metrics`` written from the same
  formulas in torch, with the reference's host reads (the GPU box has no reference checkout).  The host test holds that
  formulation to the fixture exactly as well, on the CPU.
* the fixture's layout: ``load_fixture``.
"""
import json
import os

import numpy as np

STATE = ("acc_total", "acc_count", "prec_total", "prec_count", "rec_total", "rec_count", "cls_total", "cls_count", "loc_total", "loc_count")
DEFAULT_THRESHOLDS = [0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95]
MARGIN = 2.0 ** -20            # admission: no sigmoid (float64) closer than this to a threshold in use
HOST_READS_REFERENCE = 23      # counted in voxelnet.py:654-679 + torchplus/metrics.py: 1 (Accuracy .cpu()) + 14 (if rec_count > 0 / if prec_count > 0,
#                                seven thresholds) + 2 (PrecisionRecall.value .cpu() x 2) + 2 x (1 `if not scalar.eq(0.0)` + 1 .cpu()) + 2 float(loss.cpu())
HOST_READS_DEVICE = 1


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def zero_state(num_thresholds):
    return {k: np.zeros(num_thresholds if k.startswith(("prec", "rec")) else 1, np.float32) for k in STATE}


def state_vector(state):
    return np.concatenate([np.asarray(state[k], np.float32).reshape(-1) for k in STATE])


def ret_keys(thresholds):
    """The returned dict flattened in the kernel's output order: rpn_acc, the four losses, prec per threshold, rec per threshold."""
    return (["rpn_acc", "loss/cls_loss", "loss/cls_loss_rt", "loss/loc_loss", "loss/loc_loss_rt"]
            + [f"pr/prec@{int(t*100)}" for t in thresholds] + [f"pr/rec@{int(t*100)}" for t in thresholds])


def ret_vector(ret, thresholds):
    flat = {"rpn_acc": ret["rpn_acc"]}
    flat.update({"loss/" + k: v for k, v in ret["loss"].items()})
    flat.update({"pr/" + k: v for k, v in ret["pr"].items()})
    keys = ret_keys(thresholds)
    assert sorted(flat) == sorted(keys), (sorted(flat), sorted(keys))
    assert all(type(v) is float for v in flat.values())
    return np.array([flat[k] for k in keys], np.float64)


def counts(cls_preds, labels, cared, thresholds, acc_threshold=0.5):
    """The integers of one update: matches (pred == label over all anchors), cared, and tp / fp / fn per threshold."""
    x = np.asarray(cls_preds, np.float32)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    x = x.reshape(lab.size, -1)
    w = (lab >= 0) if cared is None else np.asarray(cared).reshape(-1) != 0
    nan = np.isnan(x)
    has_nan = nan.any(1)
    real = np.where(nan, -np.inf, x)
    m = real.max(1) if lab.size else np.zeros(0)
    arg = np.where(has_nan, nan.argmax(1), real.argmax(1))            # torch.max: the first NaN, else the lowest index of the maximum
    s = sigmoid64(m)
    any_real = ~nan.all(1)
    pred = np.where(any_real & (s > np.float64(np.float32(acc_threshold))), arg + 1, 0)
    out = {"matches": int((pred == lab).sum()), "cared": int(w.sum()), "tp": [], "fp": [], "fn": []}
    pos, neg = w & (lab > 0), w & (lab == 0)
    for t in thresholds:
        hit = ~has_nan & (s > np.float64(np.float32(t)))
        out["tp"].append(int((pos & hit).sum()))
        out["fp"].append(int((neg & hit).sum()))
        out["fn"].append(int((pos & ~hit).sum()))
    return out


def restate(state, cls_loss, loc_loss, cls_preds, labels, cared, thresholds, acc_threshold=0.5):
    """One update: ``state`` (dict of float32 arrays, see ``zero_state``) is updated in place -> the returned dict."""
    f = np.float32
    c = counts(cls_preds, labels, cared, thresholds, acc_threshold)
    with np.errstate(invalid="ignore", divide="ignore"):
        state["acc_count"][0] = state["acc_count"][0] + max(f(c["cared"]), f(1.0))
        state["acc_total"][0] = state["acc_total"][0] + f(c["matches"])
        rpn_acc = state["acc_total"][0] / state["acc_count"][0]
        for i in range(len(thresholds)):
            tp, fp, fn = f(c["tp"][i]), f(c["fp"][i]), f(c["fn"][i])
            if tp + fn > 0:
                state["rec_count"][i] += tp + fn
                state["rec_total"][i] += tp
            if tp + fp > 0:
                state["prec_count"][i] += tp + fp
                state["prec_total"][i] += tp
        prec = state["prec_total"] / np.maximum(state["prec_count"], f(1.0))
        rec = state["rec_total"] / np.maximum(state["rec_count"], f(1.0))
        rt = {}
        for name, v in (("cls", f(cls_loss)), ("loc", f(loc_loss))):
            if not v == 0.0:
                state[name + "_count"][0] += f(1.0)
                state[name + "_total"][0] += v
            rt[name] = (state[name + "_total"][0] / state[name + "_count"][0], v)
    ret = {"loss": {"cls_loss": float(rt["cls"][0]), "cls_loss_rt": float(rt["cls"][1]), "loc_loss": float(rt["loc"][0]),
                    "loc_loss_rt": float(rt["loc"][1])}, "rpn_acc": float(rpn_acc), "pr": {}}
    for i, t in enumerate(thresholds):
        ret["pr"][f"prec@{int(t*100)}"] = float(prec[i])
        ret["pr"][f"rec@{int(t*100)}"] = float(rec[i])
    return ret


def same(a, b):
    """Bit-equal float arrays, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ------------------------------------------------------------------------------------------------ torch stand-in of the metric modules
def _buffers_module(names_sizes, **attrs):
    import torch
    from torch import nn

    class Metric(nn.Module):
        def clear(self):
            for b in self.buffers():
                b.zero_()
    m = Metric()
    for name, size in names_sizes:
        m.register_buffer(name, torch.zeros(size, dtype=torch.float32))
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _standin_update_metrics(self, cls_loss, loc_loss, cls_preds, labels, sampled):
    """voxelnet.py:654-679 for sigmoid scores with the background encoded as all zeros, from the formulas -- including the places
    where the reference reads a device value on the host (23 per call with seven thresholds)."""
    import torch
    if not self._encode_background_as_zeros or not self.rpn_metrics._use_sigmoid_score:
        raise NotImplementedError("the stand-in restates the sigmoid / background-as-zeros form only")
    self.standin_calls = getattr(self, "standin_calls", 0) + 1
    x = cls_preds.view(cls_preds.shape[0], -1, self._num_class)
    w = sampled.float()
    scores = torch.sigmoid(x)
    acc, pr = self.rpn_acc, self.rpn_metrics
    top = torch.max(x, dim=-1)[1] + 1
    pred = torch.where((scores > acc._threshold).any(-1), top, torch.zeros_like(top))
    acc.count += torch.clamp(w.sum(), min=1.0)
    acc.total += (pred == labels.long()).float().sum()
    rpn_acc = (acc.total / acc.count).cpu().numpy()[0]
    best = torch.max(scores, dim=-1)[0]
    pos, neg = labels > 0, labels == 0
    for i, t in enumerate(pr.thresholds):
        hit = best > t
        tp, fp, fn = (w * (pos & hit).float()).sum(), (w * (neg & hit).float()).sum(), (w * (pos & ~hit).float()).sum()
        if tp + fn > 0:
            pr.rec_count[i] += tp + fn
            pr.rec_total[i] += tp
        if tp + fp > 0:
            pr.prec_count[i] += tp + fp
            pr.prec_total[i] += tp
    prec = (pr.prec_total / torch.clamp(pr.prec_count, min=1.0)).cpu().numpy()
    rec = (pr.rec_total / torch.clamp(pr.rec_count, min=1.0)).cpu().numpy()
    vals = []
    for m, s in ((self.rpn_cls_loss, cls_loss), (self.rpn_loc_loss, loc_loss)):
        if not s.eq(0.0):
            m.count += 1
            m.total += s.data.float()
        vals.append(float((m.total / m.count).cpu().numpy()[0]))
    ret = {"loss": {"cls_loss": vals[0], "cls_loss_rt": float(cls_loss.data.cpu().numpy()), "loc_loss": vals[1],
                    "loc_loss_rt": float(loc_loss.data.cpu().numpy())}, "rpn_acc": float(rpn_acc), "pr": {}}
    for i, t in enumerate(pr.thresholds):
        ret["pr"][f"prec@{int(t*100)}"] = float(prec[i])
        ret["pr"][f"rec@{int(t*100)}"] = float(rec[i])
    return ret


def _standin_clear_metrics(self):
    for m in (self.rpn_acc, self.rpn_metrics, self.rpn_cls_loss, self.rpn_loc_loss):
        m.clear()


def attach_metrics(net, thresholds=None, modules=None):
    """``net`` (an nn.Module with ``_num_class`` and ``_encode_background_as_zeros``) gets rpn_acc / rpn_metrics / rpn_cls_loss /
    rpn_loc_loss, ``update_metrics`` and ``clear_metrics`` as methods of its class -- as on the reference's VoxelNet, where they are
    class attributes that an instance attribute can shadow.  ``modules``: the reference's own metric modules (the fixture's
    generator), else the stand-in ones."""
    thresholds = list(DEFAULT_THRESHOLDS if thresholds is None else thresholds)
    t = len(thresholds)
    if modules is None:
        modules = {
            "rpn_acc": _buffers_module((("total", 1), ("count", 1)), _threshold=0.5, _encode_background_as_zeros=True),
            "rpn_metrics": _buffers_module((("prec_total", t), ("prec_count", t), ("rec_total", t), ("rec_count", t)), _thresholds=thresholds,
                                           thresholds=thresholds, _use_sigmoid_score=True, _encode_background_as_zeros=True),
            "rpn_cls_loss": _buffers_module((("total", 1), ("count", 1))),
            "rpn_loc_loss": _buffers_module((("total", 1), ("count", 1))),
        }
    for k, m in modules.items():
        setattr(net, k, m)
    cls = type(net)
    net.__class__ = type(cls.__name__, (cls,), {"update_metrics": _standin_update_metrics, "clear_metrics": _standin_clear_metrics})
    return net


def holder(num_class, thresholds=None, modules=None):
    """The smallest object update_metrics runs on: the two attributes it reads and the metric modules."""
    from torch import nn

    class Holder(nn.Module):
        pass
    h = Holder()
    h._num_class, h._encode_background_as_zeros = int(num_class), True
    return attach_metrics(h, thresholds, modules)


def net_state(net):
    a, m, c, l = net.rpn_acc, net.rpn_metrics, net.rpn_cls_loss, net.rpn_loc_loss
    return dict(zip(STATE, (a.total, a.count, m.prec_total, m.prec_count, m.rec_total, m.rec_count, c.total, c.count, l.total, l.count)))


# ------------------------------------------------------------------------------------------------ fixture
def load_fixture(path=None):
    """-> (meta, cases): ``cases[name]`` = dict(C, N, B, label_dtype, thresholds, updates=[dict(logits f32 [B, N, C], labels [B, N],
    cared bool [B, N] or None, cls_loss, loc_loss (float32 scalars), state (float32 vector in STATE order AFTER the update), ret
    (float64 vector in ret_keys order), keys)])."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_metrics.npz")
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    cases = {}
    for name, c in meta["cases"].items():
        ups = []
        for k in range(c["updates"]):
            p = f"{name}/u{k}/"
            lab = z[p + "labels"].astype(c["label_dtype"]).reshape(c["B"], c["N"])
            ups.append(dict(logits=z[p + "logits"].astype(np.float32).reshape(c["B"], c["N"], c["C"]), labels=lab,
                            cared=(z[p + "cared"].astype(bool).reshape(c["B"], c["N"]) if p + "cared" in z.files else None),
                            cls_loss=z[p + "losses"][0], loc_loss=z[p + "losses"][1], state=z[p + "state"], ret=z[p + "ret"]))
        cases[name] = dict(c, updates=ups)
    return meta, cases


def split_state(vec, num_thresholds):
    out, o = {}, 0
    for k in STATE:
        n = num_thresholds if k.startswith(("prec", "rec")) else 1
        out[k] = np.asarray(vec[o:o + n], np.float32)
        o += n
    return out


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)
