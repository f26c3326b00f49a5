"""Training augmentation on the device: the geometric stages of the reference's ``prep_pointcloud``
(second/data/preprocess.py:250-286) for a whole batch, producing what :meth:`DeviceTrainer.step` consumes.

    aug = DeviceAugmenter.from_config(config.train_input_reader.preprocess, voxel_generator)
    aug.draw(num_boxes=gt_boxes.shape[0], batch_size=B)              # fresh noise, on the device
    trainer.step(*aug(points, point_offsets, gt_boxes, gt_offsets, gt_classes)[:5])

Stages, in the reference's order: per-object noise (noise_per_object_v3_: up to ``num_try`` tries per box, each checked for
collision against every other box of the frame), flip, global rotation, global scaling, global translation, dropping boxes
whose centre left the range, yaw wrapped to [-pi, pi).  Four launches (ops.points_in_boxes, ops.noise_per_box,
ops.augment_points_, ops.augment_boxes); every count stays on the device, so a call captures into a hipGraph next to the
training step.

Ground-truth database sampling (DataBaseSamplerV2.sample_all, second/core/sample_ops.py:95-216, and the merge of
second/data/preprocess.py:210-249) runs in front of those stages when the augmenter has a sampler:

    db = DeviceGtDatabase.from_config(preprocess.database_sampler, root_path, num_point_features=4, class_names=["Car"])
    aug = DeviceAugmenter.from_config(preprocess, voxel_generator, database=db)
    aug.draw(num_boxes=..., batch_size=B)                            # noise and fresh candidates
    trainer.step(*aug(points, point_offsets, gt_boxes, gt_offsets, gt_classes)[:5])

:class:`DeviceGtDatabase` is the pool on the device, :class:`DeviceDatabaseSampler` the six launches (ops.db_sample_select: two,
ops.points_in_boxes on the accepted boxes, ops.db_sample_merge_points: three).  What stays on the CPU: point shuffling, the frustum
crop (random_crop), group sampling (multi-class sample groups, use_group_id) and the sampler's per-object rotation.
"""

import os
import pickle

import numpy as np
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
                 device="cuda", sampler=None):
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
        self.sampler = sampler          # a DeviceDatabaseSampler run in front of the stages above, or None

    @classmethod
    def from_config(cls, preprocess_proto, voxel_generator, database=None, **kwargs):
        """From the reference's ``input_reader.preprocess`` message (second/protos/input_reader.proto, read the way
        second/builder/dataset_builder.py:84-103 does) and the voxel generator (or its 6-value point_cloud_range).  Raises ValueError
        naming the field for ``use_group_id`` and for a non-zero ``global_random_rotation_range_per_object``: neither is
        implemented.  With ``database`` (a :class:`DeviceGtDatabase`, e.g. from DeviceGtDatabase.from_config on the message's
        ``database_sampler``) the augmenter gets a :class:`DeviceDatabaseSampler` with the database's groups and rate and the
        message's ``remove_points_after_sample`` / ``sample_importance``; without one the ``database_sampler`` of the message is
        not run -- sampled objects then have to be in the boxes and points handed to the call."""
        p = preprocess_proto
        if p.use_group_id:
            raise ValueError("use_group_id: group ids are not supported by the device augmentation")
        grot = [float(v) for v in p.global_random_rotation_range_per_object]
        if grot and abs(grot[0] - grot[1]) >= 1e-3:       # the reference's own test for "enabled" (second/core/preprocess.py:604-605)
            raise ValueError(f"global_random_rotation_range_per_object: {grot} is not supported by the device augmentation (every shipped "
                             "config uses [0, 0])")
        rng = getattr(voxel_generator, "point_cloud_range", voxel_generator)
        if database is not None and "sampler" not in kwargs:
            kwargs["sampler"] = DeviceDatabaseSampler(database, remove_points_after_sample=bool(getattr(p, "remove_points_after_sample", True)),
                                                      sample_importance=float(getattr(p, "sample_importance", 1.0)))
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
        if self.sampler is not None:
            self.sampler.draw(generator, batch_size=b)
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
    def __call__(self, points, point_offsets, gt_boxes, gt_offsets, gt_classes=None, gt_mask=None, gt_importance=None, inplace=False,
                 out_point_capacity=None):
        """points [N, 4 or 5] fp32 and gt_boxes [G, 7] fp32 -- or [G, 9], columns 7 and 8 a velocity (NuScenesDatasetVelo) that the
        flips, the rotation and the scaling transform (ops.augment_boxes); the stages that only read boxes take a contiguous copy of
        columns 0-6 -- frames concatenated with [B+1] int32 offsets; ``gt_mask`` [G] bool: the
        reference's gt_boxes_mask (boxes of other classes: they block per-object moves, never move, and are dropped).
        -> (points, point_offsets, gt_boxes, gt_offsets, gt_classes[, gt_importance]): the arguments of DeviceTrainer.step.  The
        points are a copy unless ``inplace``; their count and offsets do not change.  The box tensors keep G rows: survivors first,
        in order, frame boundaries in the new gt_offsets, zero rows behind.  With a sampler the database sampling runs first: the
        boxes then have G + B*C*K rows, the points ``out_point_capacity`` rows (default: enough for every draw) with new offsets,
        and ``num_boxes`` of :meth:`draw` is that larger row count (``sampler.box_rows(G, B)``)."""
        if gt_boxes.dim() != 2 or gt_boxes.shape[1] not in (7, 9):
            raise ValueError(f"DeviceAugmenter: gt_boxes {tuple(gt_boxes.shape)}; rows of 7 values, or of 9 with a velocity in columns 7 and 8")
        if self.sampler is not None and gt_boxes.shape[1] != 7:
            raise ValueError("DeviceAugmenter: database sampling with 9-column gt_boxes (velocities) is not supported: the database "
                             "holds 7-column boxes (the reference's concatenation fails on them too)")
        rt.require_gpu(points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance)
        if self.sampler is not None:
            want_importance = gt_importance is not None
            points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance = self.sampler(
                points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance, out_point_capacity=out_point_capacity)
            inplace = True                                          # the merged cloud is already a fresh tensor
            if not want_importance:
                gt_importance = None
        b, g = gt_offsets.numel() - 1, gt_boxes.shape[0]
        if self.frame_params is None or self.frame_params.shape[0] != b:
            raise ValueError(f"no noise for a batch of {b}: call draw(num_boxes={g}, batch_size={b}) or set_noise first")
        if not inplace:
            points = points.clone()
        first = loc_t = rot_t = None
        boxes7 = gt_boxes if gt_boxes.shape[1] == 7 else gt_boxes[:, :7].contiguous()     # what the box-reading stages take
        if not self.per_object_skipped and g > 0:
            if self.loc_noises is None or self.loc_noises.shape[0] != g or tuple(self.rot_noises.shape) != tuple(self.loc_noises.shape[:2]):
                raise ValueError(f"no per-object noise for {g} boxes: call draw(num_boxes={g}, batch_size={b}) or set_noise first")
            first = ops.points_in_boxes(points, point_offsets, boxes7, gt_offsets, valid=gt_mask)
            _, loc_t, rot_t = ops.noise_per_box(boxes7, gt_offsets, gt_mask, self.loc_noises, self.rot_noises,
                                                max_boxes_per_frame=self.max_boxes_per_frame)
        ops.augment_points_(points, point_offsets, self.frame_params, first, boxes7, gt_mask, loc_t, rot_t)
        boxes, offsets, classes, importance = ops.augment_boxes(gt_boxes, gt_offsets, self.frame_params, self.bev_range, valid=gt_mask,
                                                                classes=gt_classes, importance=gt_importance, loc_transform=loc_t,
                                                                rot_transform=rot_t)
        out = (points, point_offsets, boxes, offsets, classes)
        return out + (importance,) if gt_importance is not None else out


# ---------------------------------------------------------------------------------------------------- database sampling
class DeviceGtDatabase:
    """The ground-truth database as one pool on the device: ``boxes`` [N, 7] fp32 (box3d_lidar of every object), ``pool_points``
    [P, F] fp32 (the objects' points, relative to their box centre as the database's .bin files store them), ``pool_offsets``
    [N+1] int32, ``names`` (one per row) and ``class_rows`` {name: int64 rows, in the database's order}.  ``groups`` [(name,
    max_num)] and ``rate`` are the sampler settings read by :meth:`from_config` (None / 1.0 otherwise).  ``info_index`` [N]: the
    position of each row's info in its class's unfiltered list."""

    def __init__(self, boxes, pool_points, pool_offsets, names, class_names, groups=None, rate=1.0, info_index=None, device="cuda"):
        self.device = torch.device(device)
        boxes = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 7))
        pool_points = np.ascontiguousarray(np.asarray(pool_points, np.float32))
        pool_offsets = np.ascontiguousarray(np.asarray(pool_offsets, np.int64))
        self.names = [str(n) for n in names]
        if len(self.names) != len(boxes) or len(pool_offsets) != len(boxes) + 1 or pool_points.ndim != 2:
            raise ValueError("DeviceGtDatabase: boxes [N, 7], names [N], pool_offsets [N+1], pool_points [P, F]")
        if pool_offsets[0] != 0 or (np.diff(pool_offsets) < 0).any() or pool_offsets[-1] != len(pool_points) or len(pool_points) >= 2 ** 31:
            raise ValueError("DeviceGtDatabase: pool_offsets must rise from 0 to the number of pool points")
        self.class_names = [str(n) for n in class_names]
        self.num_point_features = int(pool_points.shape[1])
        self.point_counts = np.diff(pool_offsets)
        order = {}
        for r, n in enumerate(self.names):
            order.setdefault(n, []).append(r)
        self.class_rows = {n: np.asarray(r, np.int64) for n, r in order.items()}
        self.info_index = None if info_index is None else np.asarray(info_index, np.int64)
        self.groups = None if groups is None else [(str(n), int(m)) for n, m in groups]
        self.rate = float(rate)
        self.boxes = torch.from_numpy(boxes).to(self.device)
        self.pool_points = torch.from_numpy(pool_points).to(self.device)
        self.pool_offsets = torch.from_numpy(pool_offsets.astype(np.int32)).to(self.device)

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_infos(cls, db_infos, root_path, num_point_features, class_names, min_num_points=None, removed_difficulties=(),
                   only=None, **kwargs):
        """``db_infos`` {name: [info]} as the reference's create_groundtruth_database pickles it (info: ``path`` relative to
        ``root_path``, ``box3d_lidar``, ``difficulty``, ``num_points_in_gt``).  Filters, in this order: DBFilterByMinNumPoint with
        ``min_num_points`` {name: least num_points_in_gt}, DBFilterByDifficulty with ``removed_difficulties``
        (second/core/preprocess.py:67-95; both drop infos one by one, so their order does not change the result).  ``only``: the
        class names to load (None = all).  The .bin files are read with numpy, once, here."""
        removed = set(int(d) for d in removed_difficulties)
        mins = {str(n): int(v) for n, v in dict(min_num_points or {}).items()}
        boxes, names, index, chunks, offsets = [], [], [], [], [0]
        for name, infos in db_infos.items():
            if only is not None and name not in only:
                continue
            for i, info in enumerate(infos):
                if mins.get(name, 0) > 0 and info["num_points_in_gt"] < mins[name]:
                    continue
                if info["difficulty"] in removed:
                    continue
                pts = np.fromfile(os.path.join(str(root_path), str(info["path"])), dtype=np.float32).reshape(-1, int(num_point_features))
                boxes.append(np.asarray(info["box3d_lidar"], np.float32))
                names.append(name)
                index.append(i)
                chunks.append(pts)
                offsets.append(offsets[-1] + len(pts))
        pool = np.concatenate(chunks) if chunks else np.zeros((0, int(num_point_features)), np.float32)
        return cls(np.stack(boxes) if boxes else np.zeros((0, 7), np.float32), pool, offsets, names, class_names, info_index=index, **kwargs)

    @classmethod
    def from_config(cls, database_sampler_proto, root_path, num_point_features, class_names, random_crop=False, **kwargs):
        """From the reference's ``database_sampler`` message (second/protos/sampler.proto, read the way
        second/builder/dbsampler_builder.py does): loads the pickle named by ``database_info_path`` (relative paths are taken from
        ``root_path``) and reads ``sample_groups``, ``database_prep_steps`` and ``rate``.  Raises ValueError naming the field for a
        sample group with more than one class, a non-zero ``global_random_rotation_range_per_object`` and ``random_crop``."""
        s = database_sampler_proto
        if random_crop:
            raise ValueError("random_crop: the frustum crop of sampled objects is not supported by the device sampler")
        grot = [float(v) for v in s.global_random_rotation_range_per_object]
        if grot and abs(grot[0] - grot[1]) >= 1e-3:           # the reference's own test for "enabled" (second/core/sample_ops.py:87)
            raise ValueError(f"global_random_rotation_range_per_object: {grot} of the database sampler is not supported on the device "
                             "(every shipped config uses [0, 0])")
        groups = _single_class_groups([dict(g.name_to_max_num) for g in s.sample_groups])
        mins, removed = {}, []
        for step in s.database_prep_steps:
            kind = step.WhichOneof("database_preprocessing_step")
            if kind == "filter_by_difficulty":
                removed += [int(d) for d in step.filter_by_difficulty.removed_difficulties]
            elif kind == "filter_by_min_num_points":
                for n, v in dict(step.filter_by_min_num_points.min_num_point_pairs).items():
                    mins[n] = max(mins.get(n, 0), int(v))
            else:
                raise ValueError(f"database_prep_steps: unknown step {kind}")
        path = str(s.database_info_path)
        with open(path if os.path.isabs(path) else os.path.join(str(root_path), path), "rb") as f:
            db_infos = pickle.load(f)
        return cls.from_infos(db_infos, root_path, num_point_features, class_names, min_num_points=mins, removed_difficulties=removed,
                              only=[n for n, _ in groups], groups=groups, rate=float(s.rate), **kwargs)

    @classmethod
    def synthetic(cls, seed, class_names=("Car",), objects_per_class=40, max_points=60, num_point_features=4, groups=None, rate=1.0,
                  point_cloud_range=(0.0, -40.0, -3.0, 70.4, 40.0, 1.0), **kwargs):
        """A seeded pool for tests and probes (no KITTI database exists on the machines this project is built on): per class
        ``objects_per_class`` car-sized boxes anywhere in the range with 0..``max_points`` points each inside the box."""
        rs = np.random.RandomState(seed)
        r = point_cloud_range
        boxes, names, chunks, offsets = [], [], [], [0]
        for name in class_names:
            for _ in range(int(objects_per_class)):
                box = np.array([rs.uniform(r[0] + 3, r[3] - 3), rs.uniform(r[1] + 3, r[4] - 3), rs.uniform(-1.2, -0.6), rs.uniform(1.5, 1.9),
                                rs.uniform(3.4, 4.4), rs.uniform(1.4, 1.8), rs.uniform(-np.pi, np.pi)], np.float32)
                n = rs.randint(0, int(max_points) + 1)
                local = rs.uniform(-0.45, 0.45, (n, 3)) * box[3:6]
                c, s = np.cos(box[6]), np.sin(box[6])
                pts = np.concatenate([np.stack([local[:, 0] * c + local[:, 1] * s, -local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1),
                                      rs.uniform(0, 1, (n, int(num_point_features) - 3))], 1).astype(np.float32)
                boxes.append(box)
                names.append(name)
                chunks.append(pts)
                offsets.append(offsets[-1] + n)
        return cls(np.stack(boxes), np.concatenate(chunks), offsets, names, class_names, groups=groups, rate=rate, **kwargs)


def _single_class_groups(groups):
    """[{name: max_num}] or [(name, max_num)] -> [(name, max_num)]; a group with more than one class is refused by name."""
    out = []
    for g in groups:
        items = list(g.items()) if hasattr(g, "items") else [tuple(g)]
        if len(items) != 1:
            raise ValueError(f"sample_groups: a group with more than one class ({sorted(n for n, _ in items)}) needs group sampling, which "
                             "is not supported by the device sampler")
        out.append((str(items[0][0]), int(items[0][1])))
    return out


def sample_num_table(groups, rate):
    """[C, T] int32: row c, column n = the number sample_all draws for a frame with n gt boxes of group c's class,
    np.round(rate * (max_num - n)) in float64, half to even (second/core/sample_ops.py:107-109), never negative; T = the largest
    max_num + 1, so a column past the end means 0."""
    t = max([m for _, m in groups] + [0]) + 1
    table = np.zeros((len(groups), t), np.int32)
    for c, (_, m) in enumerate(groups):
        for n in range(t):
            table[c, n] = max(int(np.round(rate * int(m - n)).astype(np.int64)), 0)
    return table


class DeviceDatabaseSampler:
    """DataBaseSamplerV2.sample_all + the merge of prep_pointcloud (second/data/preprocess.py:210-249) on a
    :class:`DeviceGtDatabase`.  ``groups`` [(class name, max_num)] or [{name: max_num}] in sample order and ``rate`` default to the
    database's; every sample class has to be one of ``class_names`` (the target classes: class id = index + 1).  The candidates
    live in a static int32 tensor ``candidates`` [B, C, K] that :meth:`draw` refills in place, so a captured call follows each draw.

    The one intended difference from the reference in how a class's permutation is consumed: the reference draws exactly
    ``sampled_num`` infos per frame, which depends on the frame's gt boxes -- a count this class never reads back.  :meth:`draw`
    takes K_c = the largest entry of the class's row of ``num_table`` per frame instead, and the device uses the first
    ``sampled_num`` of them; the rest of the K_c are skipped, not returned to the permutation."""

    def __init__(self, database, groups=None, rate=None, class_names=None, remove_points_after_sample=True, sample_importance=1.0):
        self.database = database
        groups = database.groups if groups is None else groups
        if not groups:
            raise ValueError("sample_groups: no sample groups given (pass groups=[(class name, max_num)] or build the database from_config)")
        self.groups = _single_class_groups(groups)
        self.rate = float(database.rate if rate is None else rate)
        self.class_names = [str(n) for n in (database.class_names if class_names is None else class_names)]
        for name, _ in self.groups:
            if name not in self.class_names:
                raise ValueError(f"sample_groups: {name!r} is not one of the target classes {self.class_names}")
        if len(self.groups) > ops.DB_MAX_GROUPS:
            raise ValueError(f"sample_groups: at most {ops.DB_MAX_GROUPS} groups are supported, got {len(self.groups)}")
        self.remove_points_after_sample, self.sample_importance = bool(remove_points_after_sample), float(sample_importance)
        self.num_table_host = sample_num_table(self.groups, self.rate)
        self.per_class = [int(v) for v in self.num_table_host.max(1)]                # K_c
        self.k = max(self.per_class + [1])
        if self.k > ops.DB_MAX_CANDIDATES:
            raise ValueError(f"sample_groups: at most {ops.DB_MAX_CANDIDATES} candidates per frame and class are supported, "
                             f"round(rate * max_num) = {self.k}")
        dev = self.device = database.device
        self.num_table = torch.from_numpy(self.num_table_host).to(dev)
        self.class_of_group = torch.tensor([self.class_names.index(n) + 1 for n, _ in self.groups], dtype=torch.int32, device=dev)
        self.rows = [torch.from_numpy(database.class_rows.get(n, np.zeros(0, np.int64)).astype(np.int32)).to(dev) for n, _ in self.groups]
        # the most points one frame can receive: per class the K_c largest objects
        self.max_sampled_points = sum(int(np.sort(database.point_counts[database.class_rows.get(n, np.zeros(0, np.int64))])[::-1][:kc].sum())
                                      for (n, _), kc in zip(self.groups, self.per_class))
        self.perms, self.cursors = [None] * len(self.groups), [0] * len(self.groups)
        self.candidates = None
        self.overflow = None
        self.last = None             # the dict of ops.db_sample_select of the last call (accepted rows, counts): for inspection

    def box_rows(self, num_boxes, batch_size):
        """Rows of the box tensors a call returns for ``num_boxes`` rows of gt boxes."""
        k = self.k if self.candidates is None else self.candidates.shape[2]
        return int(num_boxes) + int(batch_size) * len(self.groups) * k

    def _shuffle(self, c, generator):
        n = self.rows[c].numel()
        self.perms[c] = self.rows[c][torch.randperm(n, generator=generator, device=self.device)]
        self.cursors[c] = 0

    def draw(self, generator=None, batch_size=None):
        """Refill ``candidates`` for ``batch_size`` frames (remembered after the first call), eagerly: per frame and class the
        next K_c rows of the class's permutation (torch.randperm from ``generator``, on the database's device; the cursor is a
        host integer).  As BatchSampler._sample (second/core/preprocess.py:36-50): when cursor + K_c reaches the end, the remainder
        is taken -- fewer than asked, the slots behind are -1 -- and the permutation is shuffled anew."""
        if generator is not None and generator.device.type != self.device.type:
            raise ValueError(f"draw: the generator lives on {generator.device}, the database on {self.device}")
        if batch_size is None:
            if self.candidates is None:
                raise ValueError("draw: the first call needs batch_size")
            batch_size = self.candidates.shape[0]
        b = int(batch_size)
        if self.candidates is None or self.candidates.shape[0] != b:
            self.candidates = torch.full((b, len(self.groups), self.k), -1, dtype=torch.int32, device=self.device)
        self.candidates.fill_(-1)
        for c, kc in enumerate(self.per_class):
            if kc == 0:
                continue
            if self.perms[c] is None:
                self._shuffle(c, generator)
            n = self.rows[c].numel()
            if self.cursors[c] + b * kc < n:                   # no frame of this batch reaches the end: one strided copy
                cur = self.cursors[c]
                self.candidates[:, c, :kc] = self.perms[c][cur:cur + b * kc].view(b, kc)
                self.cursors[c] = cur + b * kc
                continue
            for f in range(b):
                cur = self.cursors[c]
                if cur + kc >= n:
                    self.candidates[f, c, :n - cur] = self.perms[c][cur:]
                    self._shuffle(c, generator)
                else:
                    self.candidates[f, c, :kc] = self.perms[c][cur:cur + kc]
                    self.cursors[c] = cur + kc
        return self

    def set_candidates(self, candidates):
        """Inject given candidates [B, C, K'] (K' <= 64; tests, reproducing a run): copied into the static tensor when the shapes
        match, adopted otherwise."""
        rt.require_gpu(candidates)
        t = candidates.to(torch.int32).contiguous()
        if t.dim() != 3 or t.shape[1] != len(self.groups) or not 1 <= t.shape[2] <= ops.DB_MAX_CANDIDATES:
            raise ValueError(f"set_candidates: expected [B, {len(self.groups)}, 1..{ops.DB_MAX_CANDIDATES}], got {tuple(t.shape)}")
        if self.candidates is not None and self.candidates.shape == t.shape:
            self.candidates.copy_(t)
        else:
            self.candidates = t.clone()
        return self

    def point_capacity(self, num_points, batch_size):
        """Rows that hold every possible outcome of a call on ``num_points`` rows of scene points."""
        return int(num_points) + int(batch_size) * self.max_sampled_points

    def __call__(self, points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask=None, gt_importance=None, out_point_capacity=None):
        """-> (points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance): the arguments of
        DeviceAugmenter.__call__.  Per frame the accepted objects' boxes follow the frame's gt boxes (G + B*C*K rows, zero rows
        behind), their points precede the scene points, and the scene points inside an accepted box are dropped when
        ``remove_points_after_sample``.  ``out_point_capacity`` rows are allocated for the points (default: point_capacity);
        if a batch needs more its tail is cut and :meth:`overflowed` says so.  A frame with more than 512 gt boxes + candidates
        in use accepts nothing."""
        rt.require_gpu(points, point_offsets, gt_boxes, gt_offsets, gt_classes, gt_mask, gt_importance, self.database.boxes)
        b = gt_offsets.numel() - 1
        if self.candidates is None or self.candidates.shape[0] != b:
            raise ValueError(f"no candidates for a batch of {b}: call draw(batch_size={b}) or set_candidates first")
        if points.shape[1] != self.database.num_point_features:
            raise ValueError(f"points have {points.shape[1]} features, the database's {self.database.num_point_features}")
        db = self.database
        sel = ops.db_sample_select(gt_boxes, gt_offsets, gt_classes, db.boxes, self.candidates, self.class_of_group, self.num_table,
                                   gt_valid=gt_mask, gt_importance=gt_importance, sample_importance=self.sample_importance)
        first = None
        if self.remove_points_after_sample:
            first = ops.points_in_boxes(points, point_offsets, sel["boxes"], sel["box_offsets"], valid=sel["sampled"])
        cap = self.point_capacity(points.shape[0], b) if out_point_capacity is None else int(out_point_capacity)
        if self.overflow is None:
            self.overflow = torch.zeros((1,), dtype=torch.int32, device=points.device)
        out, offsets, _ = ops.db_sample_merge_points(points, point_offsets, first, db.pool_points, db.pool_offsets, db.boxes, sel["accepted"],
                                                     sel["accepted_count"], out_capacity=cap, overflow=self.overflow)
        self.last = sel
        return out, offsets, sel["boxes"], sel["box_offsets"], sel["classes"], sel["valid"], sel["importance"]

    def overflowed(self):
        """True if the last call's points did not fit ``out_point_capacity`` (reads one word from the device)."""
        return self.overflow is not None and bool(self.overflow.item())
