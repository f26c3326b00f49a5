"""The fused MI355X pipeline BEHIND the reference's own ``VoxelNet.forward(example)``.

The reference evaluates with ``net(example)`` (second/pytorch/train.py:524) where ``net`` is the ``VoxelNet`` that
``build_network`` assembled from ``spconv.SubMConv3d / SparseConv3d / SparseSequential`` modules
(second/pytorch/models/voxelnet.py:142-171, middle.py:145-210, rpn.py:202-420) and ``example`` is the collated batch of
``merge_second_batch`` after ``example_convert_to_torch`` (voxels [N, T, F], num_points [N], coordinates [N, 4] with the batch
index prepended, anchors [B, A, 7]; voxelnet.py:339-375).  Eager execution of that module graph pays a host round trip per
strided layer, three modules per layer, the dense [B, 128, 200, 176] image and per-frame torch glue in ``predict``.

:class:`FusedVoxelNet` adopts such a network instead of re-running it:

  * :func:`model_config` reads everything the fused pipeline needs from the network object itself (voxel grid, layer plan of
    the RPN, anchor count, the NMS / score / direction settings of ``predict``) -- no config file, no edit of the reference;
  * the parameters move by state-dict key into :class:`second_amd.models.SecondDetector` (same keys as the reference), the
    BatchNorms are folded, the RPN is repacked for the hand-written MFMA convs; adoption is redone whenever a parameter of the
    network changes (``load_state_dict`` after acceleration, ``net.half()``, ``.to(device)``);
  * one call = copy the example into static-capacity buffers, ONE hipGraph replay (SimpleVoxel mean | SimpleVoxelRadius | PillarFeatureNet ->
    fused rulebook chain -> 14 sparse convs -> RPN on live tiles -> select / decode / NMS / finalize), ONE device -> host copy of
    the padded detections, and the reference's return value (voxelnet.py:616-643: a list of
    ``{box3d_lidar [k, 7 + custom_ndim] float32, scores [k] float32, label_preds [k] int64, metadata}`` on the input's device);
  * precision follows the caller: ``net.half()`` (train.py:470) runs the fp16 pipeline, ``dtype=torch.bfloat16`` may be forced; fp32
    networks run the fp32-storage pipeline whose products are, by default, three bf16 MFMA passes on split operands ("bf16x3": 16
    significant bits per operand, fp32 accumulation -- inside the 1e-4 of the parity rule, NOT the reference's fp32 arithmetic);
    ``fp32_exact=True`` computes IEEE fp32 products (sparse convs on the fp32 MFMA, RPN on torch's fp32 convolutions or, with
    SEC_FP32_RPN=hip, on the fp32-MFMA kernels);
  * training mode: opt-in (``train_dtype``), served by :mod:`second_amd.dropin_train`; otherwise the original forward;
  * examples that carry ``anchors_mask`` (the KITTI PointPillars configs: ``anchor_area_threshold: 1``, preprocess.py:345-357) are
    served: the example's uint8 / bool mask is copied into a static [B, A] buffer of the session and the captured select drops the
    masked-out anchors before the score threshold (voxelnet.py:397-439; sec_predict_select_masked) -- the mask is taken from the
    example, not recomputed;
  * DataParallel-padded examples (``num_points`` 2-D, voxelnet.py:346), a mask whose shape is not [B, A] (or that is not on the
    GPU) and per-frame anchor sets keep the original forward.

There is no CPU fallback inside the fused path: static capacities and graphs need the HIP library; a CPU network is served
in the dynamic-shape eager mode only when a test installs the oracle backend.
"""
import numpy as np
import torch

from . import ops
from .models import PILLAR_VFES, VFES, SecondDetector, box_ndim_of


class NotAccelerable(NotImplementedError):
    """The network is outside what the fused pipeline reproduces exactly; the message says which property."""


# (y, x) stride of the sparse middles the fused pipeline mirrors (second_amd.models.MIDDLES; middle.py:111-210, 213-300, 418-483)
SPARSE_MIDDLE_STRIDE = {"SpMiddleFHD": 8, "SpMiddleFHDLite": 8, "SpMiddleFHDPeople": 4}


def _seq(v):
    return [float(x) for x in np.asarray(v).reshape(-1)]


def head_weight(net):
    """A classification-head weight of the network: its dtype / device are the network's (``net.half()``, ``.to(device)``).  RPNV2 carries
    the heads itself; the multi-head network keeps them beside its head-less RPN (net_multi_head.py:131-148)."""
    owner = net.rpn if hasattr(net.rpn, "conv_cls") else net.large_head
    return owner.conv_cls.weight


def _multi_head_config(net, why):
    """The ``heads`` entry of a VoxelNetNuscenesMultiHead (net_multi_head.py:121-176): large_head on the trunk's concatenated map,
    small_head on block 0's cropped output; appends to ``why`` what the fused pipeline does not reproduce."""
    small, large = getattr(net, "small_head", None), getattr(net, "large_head", None)
    if type(small).__name__ != "SmallObjectHead" or type(large).__name__ != "DefaultHead":
        why.append(f"rpn RPNNoHead with heads {type(large).__name__} / {type(small).__name__} (DefaultHead on 'out' + SmallObjectHead on 'stage0' only)")
        return None
    ta = net.target_assigner
    classes, sizes = list(ta.classes), [[int(v) for v in f] for f in (ta._feature_map_sizes or [])]
    if len(sizes) != len(classes) or not all(len(f) == 3 for f in sizes):
        why.append("multi-head network without a feature_map_size per class")
        return None
    on_small = [c in net.small_classes for c in classes]
    unknown = [c for c in classes if c not in net.small_classes and c not in net.large_classes]
    if unknown:
        why.append(f"classes {unknown} belong to neither head")
        return None
    # predictions are concatenated large first, then small (:170-176): the anchors (class order of the config) must be laid out the same
    if on_small != sorted(on_small):
        first_small = classes[on_small.index(True)]
        late = [c for c, s_ in zip(classes, on_small) if not s_ and classes.index(c) > on_small.index(True)]
        why.append(f"class order: {late} (large_head, the 'out' map) come after {first_small} (small_head, the 'stage0' map); predictions are "
                   "concatenated large first")
        return None
    heads = []
    for name, head, pick in (("large_head", large, False), ("small_head", small, True)):
        fms = [f for f, s_ in zip(sizes, on_small) if s_ == pick]
        if not fms or any(f != fms[0] for f in fms):
            why.append(f"{name}: its classes' feature_map_size differ ({fms})")
            return None
        heads.append(dict(name=name, source="stage0" if pick else "out", num_anchor_per_loc=int(head._num_anchor_per_loc), feature_map_size=fms[0]))
    return heads


def _env_multiclass_nms():
    import os
    return os.environ.get("SEC_ACCELERATE_MULTICLASS_NMS", "0") == "1"


def _custom_values(net, coder, why):
    """The anchor generators' custom_values of a network whose box coder is the ground coder with ``custom_ndim`` extra values
    (box_coders.py:31-46; code_size = 7 + custom_ndim), one list per generator; [] for the plain 7-value coder.  Any other coder is
    named in ``why``."""
    custom_ndim = int(getattr(coder, "custom_ndim", 0) or 0)
    if (type(coder).__name__ == "BevBoxCoder" or getattr(coder, "vec_encode", False) or getattr(coder, "linear_dim", False)
            or int(coder.code_size) != 7 + custom_ndim):
        why.append("box coder other than the ground coder of 7 + custom_ndim values (vec_encode, linear_dim and the BEV coder are not served)")
        return []
    if custom_ndim == 0:
        return []
    if custom_ndim > ops.BOX_MAX_NDIM - 7:
        why.append(f"box coder with {custom_ndim} custom values (at most {ops.BOX_MAX_NDIM - 7})")
        return []
    gens = list(getattr(net.target_assigner, "_anchor_generators", []))
    values = [[float(v) for v in getattr(g, "custom_values", getattr(g, "_custom_values", ()))] for g in gens]
    if not values or any(len(v) != custom_ndim for v in values):
        why.append(f"anchor generators whose custom_values do not match the box coder's custom_ndim {custom_ndim}")
        return []
    return values


def model_config(net, multiclass_nms=False):
    """The ``SecondDetector`` configuration of a reference-built VoxelNet (attribute names of voxelnet.py:100-171, rpn.py:202-300,
    spconv.utils.VoxelGeneratorV2).  Raises :class:`NotAccelerable` for networks outside the fused path.
    ``multiclass_nms=True``: a network built with ``use_multi_class_nms`` is taken -- its per-class lists, ``_nms_class_agnostic`` and
    ``target_assigner.anchors_range`` are read.  Opt-in (as training is): the device path answers a frame on which no class keeps
    anything with no detections where the reference raises; without it such a network is refused by name, as before."""
    why = []
    vfe, mid, rpn = net.voxel_feature_extractor, net.middle_feature_extractor, net.rpn
    vfe_t, mid_t, rpn_t = type(vfe).__name__, type(mid).__name__, type(rpn).__name__
    pillar_vfes = PILLAR_VFES
    if vfe_t not in ("SimpleVoxel", "SimpleVoxelRadius") + pillar_vfes:
        why.append(f"voxel feature extractor {vfe_t}")
    if mid_t not in SPARSE_MIDDLE_STRIDE and mid_t != "PointPillarsScatter":
        why.append(f"middle feature extractor {mid_t}")
    if vfe_t == "SimpleVoxelRadius" and int(getattr(net, "_num_input_features", 4)) != 4:
        why.append(f"SimpleVoxelRadius on {int(net._num_input_features)} point features (x, y, z and one more only)")
    if (vfe_t in pillar_vfes) != (mid_t == "PointPillarsScatter"):
        why.append(f"{vfe_t} with {mid_t}")
    if rpn_t not in ("RPNV2", "RPNNoHead") or getattr(rpn, "_use_groupnorm", False) or not getattr(rpn, "_use_norm", True):
        why.append(f"rpn {rpn_t} (BatchNorm RPNV2 / RPNNoHead only)")
    heads = _multi_head_config(net, why) if rpn_t == "RPNNoHead" else None
    multiclass = bool(getattr(net, "_multiclass_nms", False))
    if multiclass and not multiclass_nms:
        why.append("multiclass_nms (served on request: accelerate_model(net, multiclass_nms=True) or SEC_ACCELERATE_MULTICLASS_NMS=1)")
    elif multiclass:
        # (what the device path does not reproduce, each by name; SecondDetector refuses the same configurations)
        if heads or rpn_t == "RPNNoHead":
            why.append("multiclass_nms on a multi-head network")
        if min((float(t) for t in net._nms_score_thresholds), default=1.0) <= 0.0:
            why.append("multiclass_nms with a score threshold <= 0")
    if not getattr(net, "_use_sigmoid_score", True) or not getattr(net, "_encode_background_as_zeros", True):
        why.append("softmax scores / background class")
    coder = getattr(net, "_box_coder", None) or net.target_assigner.box_coder
    custom = _custom_values(net, coder, why)
    if multiclass and multiclass_nms and custom:
        why.append("multiclass_nms with custom box values")
    if why:
        raise NotAccelerable("accelerate_model: not reproducible by the fused pipeline: " + "; ".join(why))
    vg = net.voxel_generator
    pillars = vfe_t in pillar_vfes
    ups = [float(u) for u in rpn._upsample_strides]
    use_dir = bool(net._use_direction_classifier if heads else rpn._use_direction_classifier)
    mid_stride = 1 if pillars else SPARSE_MIDDLE_STRIDE[mid_t]
    # input channels of the sparse middle: what its first conv takes (SimpleVoxelRadius feeds 3 of the 4 point features' means)
    first = next((m for m in mid.modules() if hasattr(m, "in_channels") and hasattr(m, "indice_key")), None)
    mid_in = 64 if pillars else int(first.in_channels if first is not None else net._num_input_features)
    want_in = int(net._num_input_features) - (1 if vfe_t == "SimpleVoxelRadius" else 0)
    if not pillars and mid_in != want_in:
        raise NotAccelerable(f"accelerate_model: {mid_t} takes {mid_in} input channels, {vfe_t} produces {want_in}")
    factor = mid_stride * float(np.prod([float(s) for s in rpn._layer_strides[:rpn._upsample_start_idx + 1]])) / ups[0]
    if abs(factor - round(factor)) > 1e-6:
        raise NotAccelerable(f"accelerate_model: non-integer feature map factor {factor}")
    cfg = dict(
        name="adopted:" + (getattr(net, "name", None) or type(net).__name__),
        point_cloud_range=_seq(vg.point_cloud_range), voxel_size=_seq(vg.voxel_size),
        max_points_per_voxel=int(vg.max_num_points_per_voxel), max_voxels=int(getattr(vg, "_max_voxels", 20000)),
        num_point_features=int(net._num_input_features),
        middle=mid_t, middle_in=mid_in,
        rpn=dict(layer_nums=[int(v) for v in rpn._layer_nums], layer_strides=[int(v) for v in rpn._layer_strides],
                 num_filters=[int(v) for v in rpn._num_filters], upsample_strides=ups,
                 num_upsample_filters=[int(v) for v in rpn._num_upsample_filters], num_input_features=int(rpn._num_input_features),
                 use_direction_classifier=use_dir),
        downsample_factor=int(round(factor)),
        num_anchor_per_loc=sum(h["num_anchor_per_loc"] for h in heads) if heads else int(rpn._num_anchor_per_loc),
        num_class=int(net._num_class), num_direction_bins=int(net._num_direction_bins),
        direction_offset=float(net._dir_offset), direction_limit_offset=float(net._dir_limit_offset),
        nms_score_threshold=float(net._nms_score_thresholds[0]), nms_pre_max_size=int(net._nms_pre_max_sizes[0]),
        nms_post_max_size=int(net._nms_post_max_sizes[0]), nms_iou_threshold=float(net._nms_iou_thresholds[0]),
        use_rotate_nms=bool(net._use_rotate_nms),
        post_center_range=_seq(net._post_center_range) if len(net._post_center_range) else [-1e30] * 3 + [1e30] * 3,
    )
    if custom:                                   # GroundBox3dCoder.custom_ndim > 0 (nuScenes velocity): box rows of 7 + custom_ndim values
        cfg.update(anchor_custom_values=custom)
    if multiclass:
        nc = int(net._num_class)
        lists = {k: list(getattr(net, a)) for k, a in (("nms_score_thresholds", "_nms_score_thresholds"), ("nms_pre_max_sizes", "_nms_pre_max_sizes"),
                                                        ("nms_post_max_sizes", "_nms_post_max_sizes"), ("nms_iou_thresholds", "_nms_iou_thresholds"))}
        if any(len(v) != nc for v in lists.values()):
            raise NotAccelerable(f"accelerate_model: multiclass_nms needs one threshold / size per class ({nc}), got "
                                 f"{ {k: len(v) for k, v in lists.items()} }")
        agnostic = bool(getattr(net, "_nms_class_agnostic", False))
        cfg.update(multiclass_nms=True, nms_class_agnostic=agnostic,
                   nms_score_thresholds=[float(v) for v in lists["nms_score_thresholds"]],
                   nms_pre_max_sizes=[int(v) for v in lists["nms_pre_max_sizes"]],
                   nms_post_max_sizes=[int(v) for v in lists["nms_post_max_sizes"]],
                   nms_iou_thresholds=[float(v) for v in lists["nms_iou_thresholds"]])
        if not agnostic:
            cfg.update(class_anchor_ranges=[tuple(int(v) for v in net.target_assigner.anchors_range(c)) for c in range(nc)])
    if vfe_t == "SimpleVoxelRadius":
        cfg.update(vfe="SimpleVoxelRadius")
    if pillars:
        lin = vfe.pfn_layers[0].linear
        # the decorated row of the module's kind beyond the four point features (PillarFeatureNetRadius: (x, y) -> r; RadiusHeight:
        # + h; with_distance: one more).  PillarFeatureNetOld centres the caller's voxels in place; the device path never writes them
        with_distance = bool(getattr(vfe, "_with_distance", False))
        extra = ops.pfn_row_width(VFES[vfe_t].kind, with_distance) - 4
        if len(vfe.pfn_layers) != 1 or lin.in_features != int(net._num_input_features) + extra:
            raise NotAccelerable(f"accelerate_model: {vfe_t} other than one layer on (x, y, z, r) + {extra} decorations")
        cfg.update(vfe=vfe_t, vfe_filters=[int(lin.out_features)], vfe_with_distance=with_distance)
    if heads:
        cfg.update(rpn_class="RPNNoHead", heads=heads)
    if not use_dir:
        raise NotAccelerable("accelerate_model: networks without the direction classifier")   # (every shipped config has it)
    return cfg


class _Pending:
    """One asynchronous ``net(example)`` call in flight: the clones of its outputs, the pinned host copies of its validity mask and
    counters, the event that says they have arrived, and the example itself (kept until the call is resolved: the inputs are read on
    a side stream, and a call whose counters report an overflow / other anchors / changed weights is redone synchronously)."""

    def __init__(self, eng, sess, slot, example, packed, batch, meta):
        self.eng, self.sess, self.slot, self.example = eng, sess, slot, example
        self.packed, self.batch, self.meta = packed, batch, meta
        self.results = None

    def resolve(self):
        if self.results is not None:
            return self.results
        eng, sess, slot = self.eng, self.sess, self.slot
        slot["event"].synchronize()
        nc = sess.outs["counters"].numel()
        cnt = slot["host_counters"].numpy()
        over = any(int(r) > c for r, c in zip(cnt[:nc], sess.outs["limits"]))
        if cnt[nc] or cnt[nc + 1] or over:               # rare: settle it through the synchronous path (it adopts / recaptures / falls back)
            eng.stats["deferred_redone"] += 1
            res = eng._static(eng.refresh(), self.example)
            if over:                                     # the lanes' own sessions take the capacities the synchronous session settled on
                sync = eng._session(eng._det, self.example, self.batch, -1)
                for other in eng._sessions.values():
                    if other is not sync and other.batch == sync.batch and other.caps and len(other.caps) == len(sync.caps):
                        other.grow_to = [max(a, b) for a, b in zip(other.caps, sync.caps)]
            if res is None:
                eng.stats["original_calls"] += 1
                with torch.no_grad():
                    res = eng.net._second_amd_original_forward(self.example)
        else:
            cur = torch.cuda.current_stream()
            self.packed.record_stream(cur)                # produced on the lane's stream, consumed wherever the caller is
            p = sess.outs["post"]
            nd = eng.box_ndim
            valid = slot["host_packed"].numpy()[:, (nd + 2) * p:(nd + 3) * p] > 0.5
            res = eng._results(self.packed, valid, p, self.batch, self.meta, nd)
            eng.stats["fused_calls"] += 1
        self.results = res
        slot["busy"] = None
        self.example = self.packed = None
        if self in eng._pending:
            eng._pending.remove(self)
        return res


class DeferredDetection(dict):
    """What an asynchronous ``net(example)`` returns per frame: a dict that fills itself with the reference's entries
    (voxelnet.py:616-643: box3d_lidar, scores, label_preds, metadata) the first time anything reads it -- the reference's evaluate()
    only collects the dicts in a list while it loops (train.py:519-524) and first looks inside after the loop (train.py:537-539).
    Pickles as a plain dict."""

    def __init__(self, pending, frame):
        super().__init__()
        self._pending, self._frame = pending, frame

    def _fill(self):
        pend = self.__dict__.get("_pending")
        if pend is not None:
            self.__dict__["_pending"] = None
            super().update(pend.resolve()[self._frame])
        return self

    def __getitem__(self, k):
        self._fill()
        return super().__getitem__(k)

    def get(self, k, default=None):
        self._fill()
        return super().get(k, default)

    def __contains__(self, k):
        self._fill()
        return super().__contains__(k)

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __len__(self):
        self._fill()
        return super().__len__()

    def keys(self):
        self._fill()
        return super().keys()

    def items(self):
        self._fill()
        return super().items()

    def values(self):
        self._fill()
        return super().values()

    def __eq__(self, other):
        self._fill()
        return super().__eq__(other)

    __hash__ = None

    def __repr__(self):
        self._fill()
        return super().__repr__()

    def copy(self):
        self._fill()
        return dict(super().items())

    def __reduce__(self):
        self._fill()
        return (dict, (dict(super().items()),))


class _Session:
    """Static buffers + captured graph for one (batch size, row capacity, voxel tensor layout)."""

    def __init__(self, eng, batch, cap, vox_shape, vox_dtype, anchors0, has_mask=False):
        self.eng, self.batch, self.cap = eng, batch, cap
        dev = anchors0.device
        # the example's anchors_mask [B, A] (uint8; a bool mask is converted by the copy): read by the captured select
        self.mask = torch.ones((batch, anchors0.shape[0]), dtype=torch.uint8, device=dev) if has_mask else None
        self.voxels = torch.zeros((cap,) + tuple(vox_shape), dtype=vox_dtype, device=dev)
        self.num_points = torch.ones((cap,), dtype=torch.int32, device=dev)      # rows past the live count: 0 / 1, never 0 / 0
        self.coors = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.n_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.anchors = anchors0.detach().float().contiguous().clone()
        # 1 when the anchors of the example in flight differ from the session's table: written by ONE compare launch per call
        # (ops.rows_differ_, outside the graph: the example's tensor has no fixed address), read -- and cleared -- by the graph
        self.anchor_flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.caps = None            # static_out_rows of the strided layers, in module order
        self.graph = self.outs = None
        self.event = torch.cuda.Event()
        from .models import lane_stream
        self.stream = lane_stream(dev) if eng.deferred else None     # asynchronous calls: this lane's own (high-priority: own hardware queue) stream
        self.slots, self.grow_to = [], None

    def take_slot(self):
        """Pinned host landing buffers + event for one asynchronous call; a slot is free again once its call has been resolved."""
        for sl in self.slots:
            if sl["busy"] is None:
                return sl
        if len(self.slots) >= 2:                        # both in flight: the older call is (long) done on the device -- settle it
            oldest = min(self.slots, key=lambda sl: sl["serial"])
            oldest["busy"].resolve()
            return oldest
        sl = {"host_packed": torch.empty(self.outs["packed"].shape, dtype=torch.float32, pin_memory=True),
              "host_counters": torch.empty((self.outs["flags"].numel(),), dtype=torch.int32, pin_memory=True),
              "event": torch.cuda.Event(), "busy": None, "serial": 0}
        self.slots.append(sl)
        return sl

    def _strided(self):
        import spconv
        return [m for m in self.eng._det.middle_feature_extractor.modules()
                if isinstance(m, spconv.SparseConvolution) and not m.subm]

    def body(self):
        det, b = self.eng._det, self.batch
        for m, c in zip(self._strided(), self.caps or []):
            m.static_out_rows = c
        dt = det._infer_dtype
        # the content check of the network's tensors (FusedVoxelNet._checksum) at the head of the graph.  (Its first form, ~45 us of small
        # torch launches, was tried on a side branch of the captured graph -- fork / join on a second stream: the synchronous call
        # gained nothing and three asynchronous lanes LOST a fifth of their throughput, 16.8 k -> 13.2 k frames/s -- a branched hipGraph
        # serialises against the other lanes' graphs.  Kept linear; the check itself became one launch instead.)
        stale = self.eng.weights_changed_flag()
        pitch = None
        if det.pillars:
            feats = det.voxel_feature_extractor(self.voxels, self.num_points, self.coors, out_dtype=dt, num_dev=self.n_dev)
        else:
            nf = det.cfg["num_point_features"]      # SimpleVoxel (voxel_encoder.py:207-225), summed in fp32 whatever the storage type
            if det.encoder == "SimpleVoxelRadius":  # (:228-255) rows [r, z, w, 0] for the zero-padded first conv: one launch
                vox32 = self.voxels if self.voxels.dtype == torch.float32 else self.voxels.float()
                feats = det.voxel_feature_extractor.rows4(vox32, self.num_points, out_dtype=dt or torch.float32, num_dev=self.n_dev)
                pitch = det.voxel_feature_extractor.ROW_PITCH
            elif self.voxels.dtype == torch.float32 and self.voxels.is_cuda:
                feats = ops.simple_voxel(self.voxels, self.num_points, nf, out_dtype=dt or torch.float32, num_dev=self.n_dev)   # one launch
            else:
                feats = self.voxels[:, :, :nf].float().sum(1) / self.num_points.float().unsqueeze(1)
                if dt is not None:
                    feats = feats.to(dt)
        with det.lazy_heads():          # the head tensor's background tiles stay unwritten: predict_device reads them from the empty frame's map
            preds = det.network_forward(feats, self.coors, b, num_active_dev=self.n_dev, in_pitch=pitch)
        out = det.predict_device(preds, b, self.anchors, anchors_mask=self.mask)
        checks = list(getattr(det.middle_feature_extractor, "last_overflow_checks", [])) if not det.pillars else []
        packed = torch.cat([out["boxes"].reshape(b, -1).float(), out["scores"].float(), out["labels"].float(),
                            out["valid"].float()], 1)
        counters = torch.stack([num[1] for num, _ in checks]).int() if checks else torch.zeros((1,), dtype=torch.int32, device=packed.device)
        # (the content check above: in-place updates that bump no version counter -- `p.data.copy_()`, `p.data.mul_()` -- show up in it)
        # (the anchors: compared by content, every call -- a freed-and-reallocated tensor can reuse an address and a version counter)
        flags = torch.cat([counters.reshape(-1), self.anchor_flag, stale])      # [overflow counters..., anchors differ, weights changed]
        self.anchor_flag.zero_()                                                # ready for the next call's compare
        # packed [B, (box_ndim + 3) * post]: the boxes' rows, then scores, labels and validity
        return {"packed": packed, "counters": counters, "limits": [int(c) for _, c in checks], "post": int(out["scores"].shape[1]), "flags": flags}

    def build(self, graph):
        prev = ops.set_rulebook_numbering("sorted")
        try:
            with torch.no_grad():
                if not graph:
                    self.graph, self.outs = None, self.body()
                else:
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        for _ in range(2):
                            self.body()
                    torch.cuda.current_stream().wait_stream(s)
                    torch.cuda.synchronize()
                    self.graph = torch.cuda.CUDAGraph()
                    with ops.rt.capture_guard(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                        self.outs = self.body()
                    self.eng.stats["captures"] += 1
        finally:
            ops.set_rulebook_numbering(prev)
        self.host_packed = torch.empty(self.outs["packed"].shape, dtype=torch.float32, pin_memory=True)
        self.host_counters = torch.empty((self.outs["flags"].numel(),), dtype=torch.int32, pin_memory=True)

    def launch(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            prev = ops.set_rulebook_numbering("sorted")
            try:
                with torch.no_grad():
                    self.outs = self.body()
            finally:
                ops.set_rulebook_numbering(prev)


class FusedVoxelNet:
    """See the module docstring.  ``graph=False``: the same static-capacity launches issued one by one (debugging, profiling);
    ``static=False``: dynamic shapes, eager (what a CPU network under the tests' oracle backend gets)."""

    def __init__(self, net, dtype=None, graph=True, static=None, margin=1.25, row_bucket=16384, train_dtype=None, fp32_exact=False,
                 deferred=False, lanes=3, multiclass_nms=False):
        self.net, self.cfg = net, model_config(net, multiclass_nms=multiclass_nms)
        self.box_ndim = box_ndim_of(self.cfg)        # values per anchor / box row: 7 + the coder's custom_ndim
        # deferred: eval-mode calls return at once with self-filling dicts (DeferredDetection); consecutive calls alternate between
        # `lanes` sessions on their own streams, so call k + 1's copies and graph overlap call k's tail (see _static_deferred)
        import os
        self.deferred, self.lanes = bool(deferred) and bool(graph), max(1, int(os.environ.get("SEC_ACCELERATE_LANES", lanes)))
        self._pending, self._lane, self._serial = [], 0, 0
        self.fp32_exact = bool(fp32_exact)      # fp32 networks: IEEE fp32 products instead of the split-operand bf16 passes (prepare_inference)
        self.forced_dtype, self.graph, self.static = dtype, bool(graph), static
        # training-mode calls (second_amd.dropin_train): opt-in, because the captured step computes with 16-bit features where the
        # reference's default training arithmetic is fp32 (its own enable_mixed_precision mode makes the same trade)
        self.train_dtype, self.trainer = train_dtype, None
        self.margin, self.row_bucket = float(margin), int(row_bucket)
        self._det = self._wkey = self._watch = None
        self._sessions = {}
        self.stats = {"content_readoptions": 0, "deferred_calls": 0, "deferred_redone": 0, "fused_calls": 0, "original_calls": 0, "adoptions": 0, "captures": 0, "overflow_recaptures": 0,
                      "anchor_refreshes": 0, "train_fallback_reason": None}

    # ------------------------------------------------------------------ adoption
    def _tensors(self):
        net = self.net
        out = []
        for m in (net.voxel_feature_extractor, net.middle_feature_extractor, net.rpn) + self._head_modules():
            out += list(m.parameters()) + list(m.buffers())
        return out

    def _head_modules(self):
        """The multi-head network's heads, which live beside its RPN (net_multi_head.py:131-148); () for every other network."""
        return (self.net.small_head, self.net.large_head) if self.cfg.get("heads") else ()

    def _weights_key(self):
        """Host-side fingerprint of the three sub-modules' parameters and buffers, per call: every tensor's version counter
        (in-place updates through the tensor: load_state_dict, torch optimizers) and storage address / dtype (`.half()`, `.to()`,
        `p.data = other`).  Updates through ``.data``
        (`p.data.copy_()`, `p.data.mul_()`: the reference's torchplus optimizers, EMA swap-ins) bump no counter -- those are caught
        by the CONTENT check that rides with every call (:meth:`weights_changed_flag`)."""
        w = self._watch
        return (sum(t._version for t in w), len(w), tuple(t.data_ptr() for t in w), w[0].dtype, head_weight(self.net).dtype,
                w[0].device)

    def _checksum(self):
        """Content fingerprint of every non-empty tensor of the three sub-modules, on the device: a position-weighted 64-bit sum of the
        bytes (ops.tensors_checksum: ONE launch over all ~140 tensors; the first form -- a multi-tensor L2 norm per dtype, stacked and
        compared -- cost ~45 us of small launches per call).  Tensors whose byte size is not a multiple of 4 are padded views no network
        here has; they fall back to their fp32 sum."""
        ts, odd = [], []
        for t in self._watch:
            if t.numel() == 0:
                continue
            t = t.detach()
            if t.is_cuda and t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0 and t.data_ptr() % 4 == 0:
                ts.append(t)
            else:
                odd.append(t)
        parts = []
        if ts:
            parts.append(ops.tensors_checksum(ts).reshape(-1))
        if odd:
            parts.append(torch.stack([t.double().sum() for t in odd]).view(torch.int64))
        return torch.cat(parts) if len(parts) != 1 else parts[0]

    def weights_changed_flag(self):
        """int32[1] on the device: 1 when any tensor's fingerprint differs from its fingerprint at adoption."""
        return (self._checksum() != self._ref_sum).any().int().reshape(1)

    def run_dtype(self):
        """None = fp32 pipeline; torch.float16 / torch.bfloat16 = 16-bit features (BatchNorm statistics, biases, box decode and
        NMS stay fp32 either way, as after the reference's ``convert_norm_to_float``)."""
        if self.forced_dtype is not None:
            return None if self.forced_dtype == torch.float32 else self.forced_dtype
        wd = head_weight(self.net).dtype
        return None if wd == torch.float32 else wd

    def refresh(self, force=False):
        """(Re-)adopt the network's parameters when any of them changed since the last call (``force``: unconditionally)."""
        if self._watch is None:
            self._watch = self._tensors()
        key = self._weights_key()
        if self._det is not None and key == self._wkey and not force:
            return self._det
        self._watch = self._tensors()          # (parameters may have been replaced as objects: re-enumerate, then fingerprint again)
        key = self._weights_key()
        net = self.net
        dev = head_weight(net).device
        det = SecondDetector(self.cfg).eval()
        mine = det.state_dict()
        theirs = net.state_dict()
        absent = [k for k in mine if k not in theirs and k != "global_step"]
        parts = ("voxel_feature_extractor", "middle_feature_extractor", "rpn") + (("small_head", "large_head") if self.cfg.get("heads") else ())
        extra = [k for k in theirs if k.split(".")[0] in parts and k not in mine
                 and not k.endswith("num_batches_tracked")]
        if absent or extra:
            raise NotAccelerable(f"accelerate_model: state dict differs from the fused pipeline's (missing {absent[:4]}, unknown {extra[:4]})")
        state = {}
        for k, v in mine.items():
            if k in theirs:
                t = theirs[k].detach()
                if tuple(t.shape) != tuple(v.shape):
                    raise NotAccelerable(f"accelerate_model: {k} has shape {tuple(t.shape)}, the fused pipeline expects {tuple(v.shape)}")
                state[k] = t.float() if t.is_floating_point() else t
        det.load_state_dict(state, strict=False)
        det = det.to(dev)
        dt = self.run_dtype()
        if dev.type == "cuda":       # fp32: BatchNorms folded, the RPN's 3x3 convs on sec_conv2d_nhwc_x3 (split-bf16 operands, fp32 accumulation)
            det.prepare_inference(dt if dt is not None else torch.float32, exact=self.fp32_exact and dt is None)
        det.eval()
        self._det, self._wkey = det, key
        self._ref_sum = self._checksum().clone()
        self._sessions.clear()
        self.stats["adoptions"] += 1
        return det

    # ------------------------------------------------------------------ dispatch
    def accepts(self, example):
        if self.net.training:
            return self._accepts_training(example)
        for k in ("voxels", "num_points", "coordinates", "anchors"):
            if not isinstance(example.get(k), torch.Tensor):
                return False
        return example["num_points"].dim() == 1 and self._mask_ok(example) and example["voxels"].shape[0] > 0

    def _mask_ok(self, example):
        """No ``anchors_mask``, or one the fused select takes: a bool / uint8 CUDA tensor of [B, A] entries beside the anchors (the
        masked select is a device kernel; the CPU mode of the tests' oracle backend keeps refusing masks) and a score threshold
        above 0 (a masked-out anchor must not pass it).  Anything else keeps the original forward."""
        if "anchors_mask" not in example:
            return True
        if self.cfg.get("multiclass_nms"):           # refused by name: the reference indexes the masked arrays with unmasked ranges
            self.stats["fallback_reason"] = "multiclass_nms with anchors_mask"
            return False
        m, anc =example["anchors_mask"], example["anchors"]
        if not isinstance(m, torch.Tensor) or m.dtype not in (torch.bool, torch.uint8) or not m.is_cuda or m.device != anc.device or anc.dim() < 2:
            return False
        batch = anc.shape[0]
        n_anchor = anc.numel() // (batch * self.box_ndim) if batch else 0
        return m.dim() >= 2 and m.shape[0] == batch and m.numel() == batch * n_anchor and self.cfg["nms_score_threshold"] > 0

    def _accepts_training(self, example):
        if self.train_dtype is None or self.trainer is False:
            return False
        if self.trainer is None:
            from . import dropin_train as T
            try:
                self.trainer = T.FusedTrainStep(self.net, self.cfg, self.train_dtype)
                self.stats.update(self.trainer.stats)
                self.trainer.stats = self.stats
            except T.NotTrainable as e:
                self.trainer = False
                self.stats["train_fallback_reason"] = str(e)
                return False
        return self.trainer.accepts(example)

    def __call__(self, example):
        if self.net.training:
            from . import dropin_train as T
            try:
                return self.trainer(example)
            except T.NotTrainable as e:            # found out at adoption / capture time: keep the original forward from now on
                self.trainer = False
                self.stats["train_fallback_reason"] = str(e)
                return None
        det = self.refresh()
        voxels = example["voxels"]
        static = voxels.is_cuda if self.static is None else self.static
        if not static:
            return self._dynamic(det, example)
        if self.deferred:
            return self._static_deferred(det, example)
        return self._static(det, example)

    def flush(self):
        """Resolve every asynchronous call still in flight (their dicts fill themselves when read; this only forces it now)."""
        for pend in list(self._pending):
            pend.resolve()

    def _meta(self, example, batch):
        meta = example.get("metadata")
        return list(meta) if meta is not None and len(meta) else [None] * batch

    def _dynamic(self, det, example):
        if bool(self.weights_changed_flag().item()):     # (this mode syncs per layer anyway)
            det = self.refresh(force=True)
        batch = example["anchors"].shape[0]
        anchors = example["anchors"].reshape(batch, -1, self.box_ndim).float()
        with torch.no_grad():
            voxels = example["voxels"]
            pitch = None
            if det.encoder == "SimpleVoxelRadius":
                feats, pitch = det.voxel_feature_extractor.encode(voxels.float(), example["num_points"])
            else:
                feats = det.voxel_feature_extractor(voxels.float(), example["num_points"], example["coordinates"])
            preds = det.network_forward(feats, example["coordinates"], batch, in_pitch=pitch)
            mask = example.get("anchors_mask")
            out = det.predict_device(preds, batch, anchors, anchors_mask=None if mask is None else mask.reshape(batch, -1))
        self.stats["fused_calls"] += 1
        res = []
        for b, meta in zip(range(batch), self._meta(example, batch)):
            m = out["valid"][b]
            res.append({"box3d_lidar": out["boxes"][b][m].float(), "scores": out["scores"][b][m].float(),
                        "label_preds": out["labels"][b][m].long(), "metadata": meta})
        return res

    def _session(self, det, example, batch, lane=0):
        voxels = example["voxels"]
        n = voxels.shape[0]
        anchors0 = example["anchors"].reshape(batch, -1, self.box_ndim)[0]
        has_mask = "anchors_mask" in example
        key = (batch, tuple(voxels.shape[1:]), voxels.dtype, voxels.device, int(anchors0.shape[0]), lane, has_mask)
        sess = self._sessions.get(key)
        if sess is not None and sess.cap >= n:
            return sess
        cap = -(-int(n * (1.0 if sess is None else self.margin)) // self.row_bucket) * self.row_bucket
        new = _Session(self, batch, cap, voxels.shape[1:], voxels.dtype, anchors0, has_mask)
        new.caps = self._calibrate(det, example, batch)
        self._fill(new, example)
        new.build(self.graph)
        self._sessions[key] = new
        return new

    def _calibrate(self, det, example, batch):
        """Capacities of the strided layers from one dynamic-shape forward of this example (live outputs x margin, 256-row
        granules), like SecondDetector.calibrate."""
        import spconv
        if det.pillars:
            return []
        prev = ops.set_rulebook_numbering("sorted")
        try:
            with torch.no_grad():
                nf = det.cfg["num_point_features"]
                pitch = None
                if det.encoder == "SimpleVoxelRadius":
                    feats, pitch = det.voxel_feature_extractor.encode(example["voxels"].float(), example["num_points"].int())
                else:
                    feats = example["voxels"][:, :, :nf].float().sum(1) / example["num_points"].float().unsqueeze(1)
                det.network_forward(feats, example["coordinates"].int(), batch, in_pitch=pitch)
        finally:
            ops.set_rulebook_numbering(prev)
        caps = []
        for m in det.middle_feature_extractor.modules():
            if isinstance(m, spconv.SparseConvolution) and not m.subm:
                caps.append(int(-(-int(m.last_num_out * self.margin) // 256) * 256))
        return caps

    @staticmethod
    def _fill(sess, example):
        n = example["voxels"].shape[0]
        sess.voxels[:n].copy_(example["voxels"], non_blocking=True)
        sess.num_points[:n].copy_(example["num_points"], non_blocking=True)
        sess.coors[:n].copy_(example["coordinates"], non_blocking=True)
        sess.n_dev.fill_(n)
        anc = example["anchors"]
        if anc.dtype != torch.float32 or not anc.is_contiguous():
            anc = anc.float().contiguous()
        ops.rows_differ_(sess.anchor_flag, anc, sess.anchors)
        if sess.mask is not None:
            sess.mask.copy_(example["anchors_mask"].reshape(sess.mask.shape), non_blocking=True)

    def _static(self, det, example):
        batch = example["anchors"].shape[0]
        anchors = example["anchors"].reshape(batch, -1, self.box_ndim)
        lane = -1 if self.deferred else 0           # beside asynchronous lanes the synchronous path owns a session of its own
        for attempt in range(4):
            sess = self._session(det, example, batch, lane)
            self._fill(sess, example)
            nc = sess.outs["counters"].numel()
            sess.launch()
            sess.host_packed.copy_(sess.outs["packed"], non_blocking=True)
            sess.host_counters.copy_(sess.outs["flags"], non_blocking=True)
            packed = sess.outs["packed"].clone()          # the session's buffers are overwritten by the next call
            sess.event.record()
            sess.event.synchronize()
            cnt = sess.host_counters.numpy()
            if cnt[nc + 1]:                               # the network's tensors changed under the adopted copy: adopt again, redo
                det = self.refresh(force=True)
                self.stats["content_readoptions"] += 1
                continue
            if cnt[nc]:
                same = bool((anchors == anchors[:1]).all().item())
                if not same:                              # per-frame anchor sets: the reference's own path handles them
                    return None
                sess.anchors.copy_(anchors[0])
                self.stats["anchor_refreshes"] += 1
                continue
            over = [int(r) for r, c in zip(cnt[:nc], sess.outs["limits"]) if int(r) > c]
            if over:                                      # a strided layer outgrew its capacity: size it from the raw counts, recapture
                caps = [max(c, int(-(-int(int(r) * self.margin) // 256) * 256)) for r, c in zip(cnt[:nc], sess.caps)]
                sess.caps = caps
                sess.build(self.graph)
                self.stats["overflow_recaptures"] += 1
                continue
            break
        else:
            raise RuntimeError("accelerate_model: static capacities did not settle after four attempts")
        self.stats["fused_calls"] += 1
        p = sess.outs["post"]
        hp = sess.host_packed.numpy()
        nd = self.box_ndim
        valid = hp[:, (nd + 2) * p:(nd + 3) * p] > 0.5
        return self._results(packed, valid, p, batch, self._meta(example, batch), nd)

    def _static_deferred(self, det, example):
        """The asynchronous form of :meth:`_static`: nothing waits.  Lane ``k % lanes`` (its own session: buffers, graph, stream) takes
        call k -- copies, replay, clones of the outputs, the two small device -> host copies and an event, all on the lane's stream
        after the caller's stream -- and the call returns dicts that resolve themselves when read (:class:`DeferredDetection`).  What
        the synchronous path checks after its sync (overflow counters, anchor equality, weight content) is checked when the call is
        resolved; a call that fails a check is redone synchronously from the example it still holds."""
        batch = example["anchors"].shape[0]
        anchors = example["anchors"].reshape(batch, -1, self.box_ndim)
        lane = self._lane
        self._lane = (lane + 1) % self.lanes
        sess = self._session(det, example, batch, lane)          # (first call of a lane: calibrates and captures, synchronously)
        if sess.grow_to is not None:                             # an earlier call overflowed a strided layer: larger capacities, recapture
            for sl in sess.slots:
                if sl["busy"] is not None:
                    sl["busy"].resolve()
            torch.cuda.current_stream().wait_stream(sess.stream)
            sess.caps, sess.grow_to = sess.grow_to, None
            sess.build(self.graph)
            self.stats["overflow_recaptures"] += 1
        slot = sess.take_slot()
        nc = sess.outs["counters"].numel()
        cur = torch.cuda.current_stream()
        sess.stream.wait_stream(cur)
        with torch.cuda.stream(sess.stream):
            self._fill(sess, example)
            sess.launch()
            slot["host_packed"].copy_(sess.outs["packed"], non_blocking=True)
            slot["host_counters"].copy_(sess.outs["flags"], non_blocking=True)
            packed = sess.outs["packed"].clone()
            slot["event"].record()
        self._serial += 1
        pend = _Pending(self, sess, slot, example, packed, batch, self._meta(example, batch))
        slot["busy"], slot["serial"] = pend, self._serial
        self._pending.append(pend)
        self.stats["deferred_calls"] += 1
        return [DeferredDetection(pend, b) for b in range(batch)]

    @staticmethod
    def _results(packed, valid, p, batch, metas, nd=7):
        boxes = packed[:, :nd * p].view(batch, p, nd)
        scores = packed[:, nd * p:(nd + 1) * p]
        labels = packed[:, (nd + 1) * p:(nd + 2) * p].long()          # (the packed copy carries them as floats: exact for class indices)
        res = []
        for b, meta in zip(range(batch), metas):
            idx = np.flatnonzero(valid[b])
            k = len(idx)
            if k == 0 or idx[-1] == k - 1:                # the usual case: the kept detections are a prefix
                res.append({"box3d_lidar": boxes[b, :k], "scores": scores[b, :k], "label_preds": labels[b, :k], "metadata": meta})
            else:
                sel = torch.from_numpy(idx).to(packed.device)
                res.append({"box3d_lidar": boxes[b][sel], "scores": scores[b][sel], "label_preds": labels[b][sel], "metadata": meta})
        return res


def accelerate_model(net, dtype=None, graph=True, static=None, strict=True, train_dtype=None, fp32_exact=False, deferred=None,
                     train_metrics=None, multiclass_nms=None):
    """Serve ``net(example)`` (eval mode) from the fused pipeline; see the module docstring.  ``multiclass_nms=True``
    (SEC_ACCELERATE_MULTICLASS_NMS=1): networks built with ``use_multi_class_nms`` are served too (:func:`model_config`).  ``train_dtype`` (torch.bfloat16 /
    torch.float16, or SEC_ACCELERATE_TRAIN=bf16|fp16 in the environment): training-mode calls are served too -- loss dict out of one
    graph replay, ``loss.backward()`` a second one that leaves the gradients on the network's own parameters (dropin_train).  Returns ``net`` (its ``forward`` is
    shadowed on the instance; ``net._second_amd_engine`` is the :class:`FusedVoxelNet`, ``net._second_amd_original_forward`` the
    reference's method).  ``strict=False``: a network outside the fused path is returned unchanged instead of raising.
    ``train_metrics=True`` (SEC_TRAIN_METRICS=1): ``net.update_metrics`` (train.py:327) from two launches and one host read
    (:mod:`second_amd.train_metrics`) -- fused forward or not; its counters land in the engine's ``stats`` when there is one."""
    want_metrics = _env_train_metrics() if train_metrics is None else bool(train_metrics)
    if getattr(net, "_second_amd_engine", None) is not None:
        if want_metrics:
            _hook_train_metrics(net, net._second_amd_engine.stats, explicit=train_metrics is not None)
        return net
    train_dtype = train_dtype if train_dtype is not None else _env_train_dtype()
    try:
        import os
        deferred = (os.environ.get("SEC_ACCELERATE_DEFERRED", "0") == "1") if deferred is None else bool(deferred)
        multiclass_nms = _env_multiclass_nms() if multiclass_nms is None else bool(multiclass_nms)
        eng = FusedVoxelNet(net, dtype=dtype, graph=graph, static=static, train_dtype=train_dtype, fp32_exact=fp32_exact, deferred=deferred,
                            multiclass_nms=multiclass_nms)
    except NotAccelerable:
        if strict:
            raise
        if want_metrics:
            _hook_train_metrics(net, None, explicit=train_metrics is not None)
        return net
    if want_metrics:
        _hook_train_metrics(net, eng.stats, explicit=train_metrics is not None)
    original = net.forward

    def forward(example):
        if eng.accepts(example):
            res = eng(example)
            if res is not None:
                return res
        eng.stats["original_calls"] += 1
        return original(example)
    net.forward = forward
    net._second_amd_engine, net._second_amd_original_forward = eng, original
    return net


def _env_train_dtype():
    import os
    v = os.environ.get("SEC_ACCELERATE_TRAIN", "").lower()
    return {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16, "half": torch.float16}.get(v)


def _env_train_metrics():
    import os
    return os.environ.get("SEC_TRAIN_METRICS", "0") == "1"          # unset: second_amd.train_metrics is never imported


def _hook_train_metrics(net, stats, explicit):
    """``explicit``: asked for by argument -- a network without the reference's metric modules is an error then; through the
    environment such a network is left alone."""
    from . import train_metrics
    if not explicit and not all(hasattr(net, n) for n in ("rpn_acc", "rpn_metrics", "rpn_cls_loss", "rpn_loc_loss", "update_metrics")):
        return None
    return train_metrics.install(net, stats)


def accelerate_class(cls):
    """Class-level form of :func:`accelerate_model`: every instance of ``cls`` (the reference's ``VoxelNet``) builds its engine
    lazily at its first eval-mode call; instances outside the fused path keep the original forward.  Idempotent."""
    if getattr(cls, "_second_amd_class_accelerated", False):
        return cls
    original = cls.forward

    def forward(self, example):
        eng = self.__dict__.get("_second_amd_engine")
        if eng is None and (not self.training or _env_train_dtype() is not None):
            try:
                eng = FusedVoxelNet(self, train_dtype=_env_train_dtype(), multiclass_nms=_env_multiclass_nms())
            except NotAccelerable:
                eng = False
            self.__dict__["_second_amd_engine"] = eng
            self.__dict__["_second_amd_original_forward"] = lambda ex: original(self, ex)
        if eng and eng.accepts(example):
            res = eng(example)
            if res is not None:
                return res
        if eng:
            eng.stats["original_calls"] += 1
        return original(self, example)
    forward.__doc__ = original.__doc__
    cls.forward = forward
    cls._second_amd_class_accelerated = True
    return cls


def install_import_hook(module_name="second.pytorch.models.voxelnet", class_name="VoxelNet"):
    """The zero-edit, zero-call route (SEC_ACCELERATE_MODEL=1 with a bare ``import spconv``): when the reference's
    ``second.pytorch.models.voxelnet`` is imported, its ``VoxelNet`` is passed through :func:`accelerate_class`.  If the module
    is already imported it is patched at once."""
    import importlib.abc
    import importlib.util
    import sys
    if module_name in sys.modules:
        accelerate_class(getattr(sys.modules[module_name], class_name))
        return
    if any(getattr(f, "_second_amd_hook", None) == module_name for f in sys.meta_path):
        return

    class Finder(importlib.abc.MetaPathFinder):
        _second_amd_hook = module_name

        def find_spec(self, name, path, target=None):
            if name != module_name:
                return None
            sys.meta_path.remove(self)
            spec = importlib.util.find_spec(name)
            if spec is None or spec.loader is None:
                return spec
            inner = spec.loader

            class Loader(importlib.abc.Loader):
                def create_module(self, spec_):
                    return inner.create_module(spec_)

                def exec_module(self, module):
                    inner.exec_module(module)
                    accelerate_class(getattr(module, class_name))
            spec.loader = Loader()
            return spec
    sys.meta_path.insert(0, Finder())
