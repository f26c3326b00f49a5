"""``KittiDataset.convert_detection_to_kitti_annos`` of second/data/kitti_dataset.py (:38-107) on the device.

The reference turns the detections of a val pass into KITTI annotation dicts frame by frame on the host: three device->host copies,
about twenty small numpy calls (lidar -> camera box, eight corners, projection, min / max) and a Python loop with nine list appends
per detection; ``kitti_eval.pack`` then concatenates the dicts again and uploads them, once per ``eval_class_v3`` call.  Here the
frames' tensors are concatenated on the device, ``sec_kitti_annos_f64`` (three launches) converts, drops and compacts all rows, ONE
copy brings the result to the host and the reference's list of dicts is built as views of it.  The list that comes back
(:class:`DeviceAnnoList`) also keeps the device arrays ``kitti_eval.run_stages`` wants, so the evaluation that follows neither
re-concatenates nor re-uploads the detections.

``compat.accelerate_eval(annos=True)`` (or SEC_EVAL_ANNOS=1) installs :func:`convert_detection_to_kitti_annos` on ``KittiDataset``;
the original stays at ``KittiDataset._second_amd_original_convert_detection_to_kitti_annos`` and serves every call outside the
kernel's contract (counted in ``stats['fallback']``).  The reference's quirks the kernel repeats are listed in DESIGN.md section 9e.
"""
import numpy as np

ORIGINAL = "_second_amd_original_convert_detection_to_kitti_annos"

# calls converted on the device, and calls handed to the reference's own method because they are outside the kernel's contract
stats = {"device": 0, "fallback": 0}
last_fallback_reason = None         # why the latest fallback call was outside the contract


class DeviceAnnoList(list):
    """The list of annotation dicts :func:`convert_detection_to_kitti_annos` returns, plus the device tensors of the ``dt_*`` entries
    ``kitti_eval.pack`` would build from it (dt_bbox, dt_alpha, dt_score as float64, dt_box3d, dt_name, dt_off; max_dt and the
    per-image counts on the host).  ``kitti_eval.pack`` uses them while :meth:`handoff` finds the list as it was built: the same
    length, and every dict still holding the very ``name`` array object put there (an identity check per image).  A dict that was
    replaced, or whose ``name`` was, sends the evaluation down the plain-dict route.  Edits of array CONTENTS in place are not
    detected: whoever changes annotation values in place has to pass ``list(annos)`` on.
    The gt side of a pack is cached here as well (``pack_cache``), keyed by the identity and length of ``gt_annos``.
    Pickles and copies as a plain list."""

    def __init__(self, annos=(), names=None, device=None):
        super().__init__(annos)
        self._names = names
        self._device = device
        self.pack_cache = None

    def handoff(self):
        """The device entries, or None when the list is not what was built any more."""
        if self._device is None or self._names is None or len(self) != len(self._names):
            return None
        for a, name in zip(self, self._names):
            if not isinstance(a, dict) or a.get("name") is not name:
                return None
        return self._device

    def __reduce__(self):
        return (list, (list(self),))


def _empty_anno():
    """kitti_common.empty_result_anno (:700-713): float64 (0,) arrays -- name included -- and (0, 4) / (0, 3) zeros."""
    return {"name": np.array([]), "truncated": np.array([]), "occluded": np.array([]), "alpha": np.array([]), "bbox": np.zeros([0, 4]),
            "dimensions": np.zeros([0, 3]), "location": np.zeros([0, 3]), "rotation_y": np.array([]), "score": np.array([])}


def annos_from_packed(packed, class_names, metadata):
    """The reference's list of dicts from the kernel's compacted arrays (numpy): ``packed`` holds bbox [>= n, 4], alpha, box3d
    [>= n, 7] = location, dimensions, rotation_y (float64), score (float32), label (int32) and out_off int32 [images + 1] with
    n = out_off[-1]; rows behind n are ignored.  Keys, dtypes and shapes as np.stack gives them in the reference (name kind U, truncated
    float64 zeros, occluded int64 zeros, score float32); an image with nothing kept gets empty_result_anno's layout; ``metadata[i]`` is
    attached as the reference attaches ``det['metadata']``.  A label outside ``class_names`` raises IndexError (a negative one counts
    from the end), as the reference's list indexing does.  -> (annos, names): names[i] is the ``name`` array object of annos[i]."""
    off = np.asarray(packed["out_off"]).astype(np.int64)
    images, n = len(off) - 1, int(off[-1])
    assert len(metadata) == images
    uniq, inverse = np.unique(np.asarray(packed["label"])[:n], return_inverse=True)
    table = [class_names[int(u)] for u in uniq]
    name = np.array(table)[inverse.reshape(-1)] if n else np.zeros(0, "U1")
    box3d = np.asarray(packed["box3d"])[:n]
    whole = {"name": name, "truncated": np.zeros(n), "occluded": np.zeros(n, np.int64), "alpha": np.asarray(packed["alpha"])[:n],
             "bbox": np.asarray(packed["bbox"])[:n], "dimensions": np.ascontiguousarray(box3d[:, 3:6]),
             "location": np.ascontiguousarray(box3d[:, 0:3]), "rotation_y": np.ascontiguousarray(box3d[:, 6]),
             "score": np.asarray(packed["score"])[:n]}
    annos, names = [], []
    for i in range(images):
        a, b = int(off[i]), int(off[i + 1])
        anno = {k: v[a:b] for k, v in whole.items()} if b > a else _empty_anno()
        anno["metadata"] = metadata[i]
        annos.append(anno)
        names.append(anno["name"])
    return annos, names


def _calibration(infos, images):
    """(lidar2cam [images, 4, 4], P2 [images, 4, 4] float64, image_hw [images, 2] int32) of infos[0 .. images) BY POSITION, or None
    when an info is outside the contract.  lidar2cam = R0_rect @ Tr_velo_to_cam with numpy's ``@``, as box_np_ops.lidar_to_camera."""
    l2c, p2, hw = np.empty((images, 4, 4)), np.empty((images, 4, 4)), np.empty((images, 2), np.int32)
    for i in range(images):
        info = infos[i]
        try:
            calib, shape = info["calib"], info["image"]["image_shape"]
            rect, trv2c, p = np.asarray(calib["R0_rect"]), np.asarray(calib["Tr_velo_to_cam"]), np.asarray(calib["P2"])
        except (KeyError, TypeError, IndexError):
            return None
        if rect.shape != (4, 4) or trv2c.shape != (4, 4) or p.shape != (4, 4) or np.shape(shape) != (2,):
            return None
        if any(m.dtype.kind != "f" for m in (rect, trv2c, p)) or np.asarray(shape).dtype.kind not in "iu":
            return None
        l2c[i], p2[i], hw[i] = rect @ trv2c, p, shape
    return l2c, p2, hw


def _frames_reason(frames):
    """Why the frames are outside the kernel's contract (None: they are inside): types and shapes first, the device last."""
    import torch
    if not frames:
        return "no frames"
    for boxes, scores, labels in frames:
        if not all(torch.is_tensor(t) for t in (boxes, scores, labels)):
            return "not tensors"
        if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 7:
            return "boxes not float32 [*, 7]"
        if scores.dtype != torch.float32 or tuple(scores.shape) != (boxes.shape[0],):
            return "scores not float32 [*]"
        if labels.dtype not in (torch.int32, torch.int64) or tuple(labels.shape) != (boxes.shape[0],):
            return "labels not int32 / int64 [*]"
    return None


def _device_reason(frames):
    dev = frames[0][0].device
    if any(not t.is_cuda for f in frames for t in f):
        return "detections on the CPU"
    if any(t.device != dev for f in frames for t in f):
        return "frames on different devices"
    return None


def convert_detection_to_kitti_annos(dataset, detection):
    """Drop-in for ``KittiDataset.convert_detection_to_kitti_annos(self, detection)``: the same list of dicts (a
    :class:`DeviceAnnoList`).  ``dataset._kitti_infos[i]`` is read by position and ``dataset._class_names`` by label, as the
    reference does.  The frames' row counts come from tensor shapes, so nothing synchronises before the one device->host copy (a
    DeferredDetection fills itself when first read, as for the reference).  The detections are not written: the reference lowers
    ``box3d_lidar[:, 2]`` by half the height in place on what ``.cpu().numpy()`` returned, which for CPU tensors is the caller's tensor.
    Outside the kernel's contract -- a frame on the CPU, boxes not float32 [*, 7], scores not float32, labels not int32 / int64,
    frames on different devices, a calibration matrix not 4 x 4, an info without ``calib`` / ``image_shape``, no frame at all -- the
    reference's own method serves the call (``stats['fallback']``)."""
    import torch
    from . import kitti_eval, ops
    images = len(detection)
    frames = [(det["box3d_lidar"], det["scores"], det["label_preds"]) for det in detection]
    global last_fallback_reason
    reason, calib = _frames_reason(frames), None
    if reason is None:
        calib = _calibration(dataset._kitti_infos, images)
        reason = "calibration not 4 x 4 float matrices / no calib or image_shape" if calib is None else _device_reason(frames)
    if reason is not None:
        stats["fallback"] += 1
        last_fallback_reason = reason
        return getattr(dataset, ORIGINAL)(detection)
    stats["device"] += 1
    class_names = dataset._class_names
    dev = frames[0][0].device
    counts = np.array([f[0].shape[0] for f in frames], np.int64)
    det_off = np.zeros(images + 1, np.int64)
    np.cumsum(counts, out=det_off[1:])
    assert det_off[-1] < 2 ** 31, "int32 offsets"
    n = int(det_off[-1])
    boxes = torch.cat([f[0].detach() for f in frames], 0).contiguous()
    scores = torch.cat([f[1].detach() for f in frames], 0).contiguous()
    labels = torch.cat([f[2].detach() for f in frames], 0).to(torch.int32).contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.kitti_annos(boxes, scores, labels, up(det_off.astype(np.int32)), up(calib[0]), up(calib[1]), up(calib[2]))
    host = ops.kitti_annos_views(out["packed"].cpu().numpy(), n, images)          # the one device->host copy
    annos, names = annos_from_packed(host, class_names, [det["metadata"] for det in detection])
    kept = int(host["out_off"][-1])
    # what kitti_eval.pack builds from the dicts, already on the device (names through the same table, lower-cased)
    ids = kitti_eval._name_ids(class_names)
    label = out["label"][:kept].long()
    device = {
        "dt_bbox": out["bbox"][:kept], "dt_alpha": out["alpha"][:kept], "dt_score": out["score"][:kept].double(), "dt_box3d": out["box3d"][:kept],
        "dt_name": (up(ids)[label] if len(ids) else label.to(torch.int32)).contiguous(), "dt_off": out["out_off"],
        "dt_num": np.diff(host["out_off"].astype(np.int64)),
    }
    device["max_dt"] = int(device["dt_num"].max(initial=0))
    return DeviceAnnoList(annos, names, device)
