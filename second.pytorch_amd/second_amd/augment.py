"""Training augmentation on the device: the geometric stages of the reference's ``prep_pointcloud``
(second/data/preprocess.py:250-286) for a whole batch, producing what :meth:`DeviceTrainer.step` consumes.

    aug = DeviceAugmenter.from_config(config.train_input_reader.preprocess, voxel_generator)
    aug.draw(num_boxes=gt_boxes.shape[0], batch_size=B)              # fresh noise, on the device
    trainer.step(*aug(points, point_offsets, gt_boxes, gt_offsets, gt_classes)[:5])

Stages, in the reference's order: per-object noise (noise_per_object_v3_: up to ``num_try`` tries per box, each checked for
collision against every other box of the frame), flip, global rotation, global scaling, global translation, dropping boxes
whose centre left the range, yaw wrapped to [-pi, pi).  Four launches (ops.points_in_boxes, ops.noise_per_box,
ops.augment_points_, ops.augment_boxes); every count stays on the device, so a call captures into a hipGraph next to the
training step.  What stays on the CPU: database sampling, remove_points_after_sample, point shuffling, the frustum crop.
"""

import torch

from . import ops
from . import runtime as rt


def _pair(v, name):
    v = [float(x) for x in (v if isinstance(v, (list, tuple)) or hasattr(v, "__len__") else (-v, v))]
    if len(v) != 2:
        raise ValueError(f"{name}: expected (low, high), got {v}")
    return tuple(v)


def _triple(v, name):
    v = [float(x) for x in (v if isinstance(v, (list, tuple)) or hasattr(v, "__len__") else (v, v, v))]
    if len(v) != 3:
        raise ValueError(f"{name}: expected three values, got {v}")
    return tuple(v)


class DeviceAugmenter:
    """``gt_rotation_noise`` (low, high) rad and ``gt_loc_noise_std`` (x, y, z) m: the per-object noise; ``global_rotation_noise`` /
    ``global_scaling_noise`` (low, high); ``global_translate_noise_std`` (x, y, z); ``point_cloud_range`` (6 values, its BEV part
    filters the boxes); ``num_try`` tries per box (the reference uses 100; at most 128); ``max_boxes_per_frame`` (at most 512): a
    frame with more boxes gets no per-object noise.  The noise lives in static device tensors -- ``loc_noises`` [G, T, 3],
    ``rot_noises`` [G, T], ``frame_params`` [B, 8] = (flip_x, flip_y, angle, scale, tx, ty, tz, 0) -- that :meth:`draw` refills in
    place, so a captured call sees each new draw."""

    def __init__(self, gt_rotation_noise, gt_loc_noise_std, global_rotation_noise, global_scaling_noise, global_translate_noise_std,
                 random_flip_x, random_flip_y, point_cloud_range, num_try=100, max_boxes_per_frame=ops.AUG_MAX_BOXES_PER_FRAME,
                 device="cuda"):
        self.gt_rotation_noise = _pair(gt_rotation_noise, "gt_rotation_noise")
        self.gt_loc_noise_std = _triple(gt_loc_noise_std, "gt_loc_noise_std")
        self.global_rotation_noise = _pair(global_rotation_noise, "global_rotation_noise")
        self.global_scaling_noise = _pair(global_scaling_noise, "global_scaling_noise")
        self.global_translate_noise_std = _triple(global_translate_noise_std, "global_translate_noise_std")
        self.random_flip_x, self.random_flip_y = bool(random_flip_x), bool(random_flip_y)
        rng = [float(v) for v in point_cloud_range]
        if len(rng) != 6:
            raise ValueError(f"point_cloud_range: expected 6 values, got {rng}")
        self.bev_range = (rng[0], rng[1], rng[3], rng[4])
        self.num_try, self.max_boxes_per_frame = int(num_try), int(max_boxes_per_frame)
        if not 1 <= self.num_try <= ops.AUG_MAX_TRY:
            raise ValueError(f"num_try: 1..{ops.AUG_MAX_TRY} tries per box are supported, got {num_try}")
        if not 1 <= self.max_boxes_per_frame <= ops.AUG_MAX_BOXES_PER_FRAME:
            raise ValueError(f"max_boxes_per_frame: 1..{ops.AUG_MAX_BOXES_PER_FRAME} are supported, got {max_boxes_per_frame}")
        self.device = torch.device(device)
        self.loc_noises = self.rot_noises = self.frame_params = None

    @classmethod
    def from_config(cls, preprocess_proto, voxel_generator, **kwargs):
        """From the reference's ``input_reader.preprocess`` message (second/protos/input_reader.proto, read the way
        second/builder/dataset_builder.py:84-103 does) and the voxel generator (or its 6-value point_cloud_range).  Raises ValueError
        naming the field for ``use_group_id`` and for a non-zero ``global_random_rotation_range_per_object``: neither is
        implemented.  The ``database_sampler`` of the message is not run and never was by this project -- sampled objects have to be
        in the boxes and points handed to the call."""
        p = preprocess_proto
        if p.use_group_id:
            raise ValueError("use_group_id: group ids are not supported by the device augmentation")
        grot = [float(v) for v in p.global_random_rotation_range_per_object]
        if grot and abs(grot[0] - grot[1]) >= 1e-3:       # the reference's own test for "enabled" (second/core/preprocess.py:604-605)
            raise ValueError(f"global_random_rotation_range_per_object: {grot} is not supported by the device augmentation (every shipped "
                             "config uses [0, 0])")
        rng = getattr(voxel_generator, "point_cloud_range", voxel_generator)
        return cls(list(p.groundtruth_rotation_uniform_noise), list(p.groundtruth_localization_noise_std),
                   list(p.global_rotation_uniform_noise), list(p.global_scaling_uniform_noise), list(p.global_translate_noise_std),
                   p.random_flip_x, p.random_flip_y, rng, **kwargs)

    @property
    def per_object_skipped(self):
        """True when the per-object stage does nothing: all noise zero, the reference's early return (second/core/preprocess.py:611-612)."""
        return all(v == 0 for v in self.gt_loc_noise_std) and all(v == 0 for v in self.gt_rotation_noise)

    # ------------------------------------------------------------------------------------------------ noise
    def _require_device(self):
        rt.require_gpu(torch.empty(0, device=self.device))

    def _alloc(self, num_boxes, batch_size):
        g, b = int(num_boxes), int(batch_size)
        if self.frame_params is None or self.frame_params.shape[0] != b or self.loc_noises.shape[0] != g:
            self.loc_noises = torch.zeros((g, self.num_try, 3), dtype=torch.float32, device=self.device)
            self.rot_noises = torch.zeros((g, self.num_try), dtype=torch.float32, device=self.device)
            self.frame_params = torch.zeros((b, 8), dtype=torch.float32, device=self.device)

    def draw(self, generator=None, num_boxes=None, batch_size=None):
        """Fill the noise tensors from ``generator`` (a torch.Generator of this device; None = the device's default), eagerly, on the
        device.  ``num_boxes`` (rows of gt_boxes) / ``batch_size`` size the tensors at the first call and may be left out afterwards;
        the same sizes reuse the same storage.  loc_noises ~ N(0, std) per axis, rot_noises ~ U(low, high) (noise_per_object_v3_,
        second/core/preprocess.py:616-621); frame_params: each flip flag with p = 0.5 where enabled (random_flip), angle and scale
        uniform, translation normal -- z with the x entry of the std, as global_translate_ draws it (preprocess.py:894-896)."""
        self._require_device()
        if generator is not None and generator.device.type != self.device.type:
            raise ValueError(f"draw: the generator lives on {generator.device}, the noise on {self.device}")
        if self.frame_params is None and (num_boxes is None or batch_size is None):
            raise ValueError("draw: the first call needs num_boxes and batch_size")
        self._alloc(self.loc_noises.shape[0] if num_boxes is None else num_boxes,
                    self.frame_params.shape[0] if batch_size is None else batch_size)
        dev, b = self.device, self.frame_params.shape[0]
        if not self.per_object_skipped:
            self.loc_noises.normal_(0.0, 1.0, generator=generator).mul_(torch.tensor(self.gt_loc_noise_std, device=dev))
            lo, hi = self.gt_rotation_noise
            self.rot_noises.uniform_(0.0, 1.0, generator=generator).mul_(hi - lo).add_(lo)
        u = torch.rand((b, 4), generator=generator, device=dev)
        n = torch.randn((b, 3), generator=generator, device=dev)
        fp = self.frame_params
        fp[:, 0] = (u[:, 0] < 0.5).float() * float(self.random_flip_x)
        fp[:, 1] = (u[:, 1] < 0.5).float() * float(self.random_flip_y)
        (lo, hi), (slo, shi), std = self.global_rotation_noise, self.global_scaling_noise, self.global_translate_noise_std
        fp[:, 2] = u[:, 2] * (hi - lo) + lo
        fp[:, 3] = u[:, 3] * (shi - slo) + slo
        fp[:, 4:7] = n * torch.tensor([std[0], std[1], std[0]], device=dev) if any(std) else 0.0
        return self

    def set_noise(self, loc_noises=None, rot_noises=None, frame_params=None):
        """Inject given noise (tests, reproducing a run): copied into the static tensors when the shapes match them, adopted otherwise."""
        rt.require_gpu(loc_noises, rot_noises, frame_params)
        for name, t in (("loc_noises", loc_noises), ("rot_noises", rot_noises), ("frame_params", frame_params)):
            if t is None:
                continue
            t = t.to(torch.float32)
            cur = getattr(self, name)
            if cur is not None and cur.shape == t.shape:
                cur.copy_(t)
            else:
                setattr(self, name, t.contiguous().clone())
        return self

    # ------------------------------------------------------------------------------------------------ the call
    def __call__(self, points, point_offsets, gt_boxes, gt_offsets, gt_classes=None, gt_mask=None, gt_importance=None, inplace=False):
        """points [N, 4 or 5] fp32 and gt_boxes [G, 7] fp32, frames concatenated with [B+1] int32 offsets; ``gt_mask`` [G] bool: the
        reference's gt_boxes_mask (boxes of other classes: they block per-object moves, never move, and are dropped).
        -> (points, point_offsets, gt_boxes, gt_offsets, gt_classes[, gt_importance]): the arguments of DeviceTrainer.step.  The
        points are a copy unless ``inplace``; their count and offsets do not change.  The box tensors keep G rows: survivors first,
        in order, frame boundaries in the new gt_offsets, zero rows behind."""
        rt.require_gpu(points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance)
        b, g = gt_offsets.numel() - 1, gt_boxes.shape[0]
        if self.frame_params is None or self.frame_params.shape[0] != b:
            raise ValueError(f"no noise for a batch of {b}: call draw(num_boxes={g}, batch_size={b}) or set_noise first")
        if not inplace:
            points = points.clone()
        first = loc_t = rot_t = None
        if not self.per_object_skipped and g > 0:
            if self.loc_noises is None or self.loc_noises.shape[0] != g or tuple(self.rot_noises.shape) != tuple(self.loc_noises.shape[:2]):
                raise ValueError(f"no per-object noise for {g} boxes: call draw(num_boxes={g}, batch_size={b}) or set_noise first")
            first = ops.points_in_boxes(points, point_offsets, gt_boxes, gt_offsets, valid=gt_mask)
            _, loc_t, rot_t = ops.noise_per_box(gt_boxes, gt_offsets, gt_mask, self.loc_noises, self.rot_noises,
                                                max_boxes_per_frame=self.max_boxes_per_frame)
        ops.augment_points_(points, point_offsets, self.frame_params, first, gt_boxes, gt_mask, loc_t, rot_t)
        boxes, offsets, classes, importance = ops.augment_boxes(gt_boxes, gt_offsets, self.frame_params, self.bev_range, valid=gt_mask,
                                                                classes=gt_classes, importance=gt_importance, loc_transform=loc_t,
                                                                rot_transform=rot_t)
        out = (points, point_offsets, boxes, offsets, classes)
        return out + (importance,) if gt_importance is not None else out
