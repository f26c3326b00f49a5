"""``VoxelNet.update_metrics`` (second/pytorch/models/voxelnet.py:654-679) on the device.

The last call of the reference's training iteration (train.py:327) runs torchplus/metrics.py ``Accuracy``, ``PrecisionRecall``
(seven thresholds) and two ``Scalar`` modules: about 150 small launches and 23 device-to-host reads per optimisation step -- the 14
``if rec_count > 0`` / ``if prec_count > 0`` branches on device values, the two ``if not scalar.eq(0.0)``, five ``.cpu()`` of
values and two ``float(x.data.cpu().numpy())``.  Here: two launches (``sec_train_metrics_f32``) that write the SAME ten state
buffers, and one copy into pinned memory behind one event for the returned dict.

    m = DeviceTrainMetrics.from_net(net)        # binds net.rpn_acc / rpn_metrics / rpn_cls_loss / rpn_loc_loss buffers
    m.accumulate(cls_loss, loc_loss, cls_preds, labels, cared)      # no host read; may be captured in a hipGraph
    ret = m.read()                              # the reference's dict; one copy, one event wait
    ret = m.update(...)                         # both

``install(net)`` (``compat.accelerate_model(net, train_metrics=True)`` or SEC_TRAIN_METRICS=1) shadows ``net.update_metrics`` on the
instance.  Calls outside the kernel's contract go to the reference's own method, unchanged, and are counted with their reason in
``stats``: CPU tensors, logits that are not float32 (the reference takes the sigmoid in the logits' own dtype), a background column
or softmax scores, a ``sampled`` that is not bool / uint8 (its values would be weights), metric buffers on another device, more than
2^24 anchors (the reference's float32 sums stop being exact there).
"""
import os

import torch

from . import ops

DEFAULT_THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95)         # voxelnet.py:178


def env_enabled():
    return os.environ.get("SEC_TRAIN_METRICS", "0") == "1"


def _net_state(net):
    a, m, c, l = net.rpn_acc, net.rpn_metrics, net.rpn_cls_loss, net.rpn_loc_loss
    return (a.total, a.count, m.prec_total, m.prec_count, m.rec_total, m.rec_count, c.total, c.count, l.total, l.count)


class DeviceTrainMetrics:
    def __init__(self, thresholds=DEFAULT_THRESHOLDS, acc_threshold=0.5, device="cuda", _state_of=None):
        self.thresholds = [float(t) for t in thresholds]
        if len(self.thresholds) > ops.TRAIN_METRICS_MAX_THRESHOLDS:
            raise ValueError(f"{len(self.thresholds)} thresholds: at most {ops.TRAIN_METRICS_MAX_THRESHOLDS}")
        self.acc_threshold = float(acc_threshold)
        self._state_of = _state_of
        self._own = None
        self._dev = None
        if _state_of is None:
            t = len(self.thresholds)
            self._own = tuple(torch.zeros(t if 2 <= k < 6 else 1, dtype=torch.float32, device=device) for k in range(10))

    @classmethod
    def from_net(cls, net):
        """Bound to the network's OWN metric buffers (looked up at every call: ``net.cuda()`` replaces them), so ``clear_metrics()``,
        ``state_dict()``, checkpoints and a later call of the reference's method all see the same numbers."""
        return cls(thresholds=net.rpn_metrics.thresholds, acc_threshold=net.rpn_acc._threshold, _state_of=lambda: _net_state(net))

    def state(self):
        """The ten float32 buffers in the order of ``ops.TRAIN_METRICS_STATE``."""
        return self._own if self._state_of is None else self._state_of()

    def clear(self):
        for s in self.state():
            s.zero_()

    def _buffers(self, device):
        if self._dev != device:                      # first call, or the metrics moved: counters (zero), result row, pinned mirror, event
            t = len(self.thresholds)
            self._ws = ops.train_metrics_workspace(t, device)
            self._out = torch.zeros(5 + 2 * t, dtype=torch.float32, device=device)
            self._host = torch.zeros(5 + 2 * t, dtype=torch.float32).pin_memory()
            self._event = torch.cuda.Event()
            self._dev = device
        return self._ws, self._out

    def accumulate(self, cls_loss, loc_loss, cls_preds, labels, cared=None):
        """One update of the state; no host read.  ``cls_preds`` float32 [B, ..., C] contiguous, ``labels`` int32 / int64 [B, N],
        ``cared`` bool / uint8 [B, N] or None (labels >= 0), the losses float32 tensors of one element."""
        ws, out = self._buffers(cls_preds.device)
        f32 = lambda x: x.detach() if x.dtype == torch.float32 else x.detach().float()
        ops.train_metrics(cls_preds.detach(), labels, cared, self.thresholds, self.acc_threshold, f32(cls_loss), f32(loc_loss),
                          self.state(), out, ws)

    def read(self):
        """The reference's dict for the state as the last ``accumulate`` left it: one copy into pinned memory, one event wait."""
        self._host.copy_(self._out, non_blocking=True)
        self._event.record()
        self._event.synchronize()
        v = self._host.tolist()
        t = len(self.thresholds)
        ret = {"loss": {"cls_loss": v[1], "cls_loss_rt": v[2], "loc_loss": v[3], "loc_loss_rt": v[4]}, "rpn_acc": v[0], "pr": {}}
        for i, thresh in enumerate(self.thresholds):
            ret["pr"][f"prec@{int(thresh*100)}"] = v[5 + i]
            ret["pr"][f"rec@{int(thresh*100)}"] = v[5 + t + i]
        return ret

    def update(self, cls_loss, loc_loss, cls_preds, labels, cared=None):
        self.accumulate(cls_loss, loc_loss, cls_preds, labels, cared)
        return self.read()


def fallback_reason(net, cls_loss, loc_loss, cls_preds, labels, sampled):
    """None when the device form serves this call, else why the reference's method has to (module docstring)."""
    tensors = (cls_loss, loc_loss, cls_preds, labels, sampled)
    if not all(torch.is_tensor(t) for t in tensors):
        return "an argument that is not a tensor"
    if not getattr(net, "_encode_background_as_zeros", False):
        return "background column (encode_background_as_zeros is off)"
    if not getattr(net.rpn_metrics, "_use_sigmoid_score", False) or not getattr(net.rpn_acc, "_encode_background_as_zeros", False):
        return "softmax scores"
    if sampled.dtype not in (torch.bool, torch.uint8):
        return f"sampled in {sampled.dtype}, not bool / uint8"
    if labels.dtype not in (torch.int32, torch.int64):
        return f"labels in {labels.dtype}, not int32 / int64"
    if not all(t.is_cuda for t in tensors):
        return "CPU tensors"
    if cls_preds.dtype != torch.float32:
        return f"logits in {cls_preds.dtype}, not float32"
    if any(t.device != cls_preds.device for t in tensors) or any(s.device != cls_preds.device or s.dtype != torch.float32
                                                                 for s in _net_state(net)):
        return "metric buffers or arguments on another device than the predictions (or not float32)"
    total = labels.numel()
    if total > ops.TRAIN_METRICS_MAX_ANCHORS:
        return f"{total} anchors: more than 2^24"
    num_class = int(net._num_class)
    if total == 0 or cls_preds.numel() != total * num_class or sampled.numel() != total or cls_preds.shape[0] != labels.shape[0]:
        return "shapes that are not [B, ..., C] logits with [B, N] labels and sampled"
    if len(net.rpn_metrics.thresholds) > ops.TRAIN_METRICS_MAX_THRESHOLDS:
        return "more than 16 thresholds"
    return None


def install(net, stats=None):
    """Shadow ``net.update_metrics`` on the instance (idempotent).  ``stats`` (the fused engine's dict when there is one) receives
    ``train_metrics_calls``, ``train_metrics_fallbacks`` and ``train_metrics_fallback_reason``.  -> the :class:`DeviceTrainMetrics`,
    also kept as ``net._second_amd_train_metrics``; the reference's bound method as ``net._second_amd_original_update_metrics``."""
    if getattr(net, "_second_amd_train_metrics", None) is not None:
        return net._second_amd_train_metrics
    for name in ("rpn_acc", "rpn_metrics", "rpn_cls_loss", "rpn_loc_loss", "update_metrics"):
        if not hasattr(net, name):
            raise AttributeError(f"train metrics hook: the network has no `{name}` (not the reference's VoxelNet)")
    stats = {} if stats is None else stats
    stats.setdefault("train_metrics_calls", 0)
    stats.setdefault("train_metrics_fallbacks", 0)
    stats.setdefault("train_metrics_fallback_reason", None)
    original = net.update_metrics
    dev = DeviceTrainMetrics.from_net(net)
    dev.stats = stats

    def update_metrics(cls_loss, loc_loss, cls_preds, labels, sampled):
        reason = fallback_reason(net, cls_loss, loc_loss, cls_preds, labels, sampled)
        if reason is not None:
            stats["train_metrics_fallbacks"] += 1
            stats["train_metrics_fallback_reason"] = reason
            return original(cls_loss, loc_loss, cls_preds, labels, sampled)
        stats["train_metrics_calls"] += 1
        return dev.update(cls_loss, loc_loss, cls_preds.contiguous(), labels.contiguous(), sampled.contiguous())
    net.update_metrics = update_metrics
    net._second_amd_train_metrics, net._second_amd_original_update_metrics = dev, original
    return dev
