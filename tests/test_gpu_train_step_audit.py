"""The 16-bit training step, node by node against fp64 on its own inputs (tests/train_step_audit_helpers.py): two real
``DeviceTrainer.step`` calls on two different batches are recorded -- every call of the project's autograd functions with inputs,
outputs, arriving and produced gradients, the kernel-level arguments below them, the sparse layers' coordinates -- and then

  * every node is held to the fp64 reference and the per-element bound of its kernel's own test, on the tensors the step gave it;
  * the wiring is asserted: weight images are the images of the master weights as they are in THAT step, every strided layer's
    backward got its own tables, the gradient arriving at a node is bit for bit what its consumer produced, every parameter's bucket
    slot is its node's weight gradient (nothing of the step before), the record covers the autograd graph, the master weights follow
    fp64 AdamW on the recorded gradients, the running statistics follow the recurrence.

car.fhd runs at a reduced x / y range (full z extent: the middle extractor's depth chain 41 -> 21 -> 11 -> 5 -> 2 is the shipped one)
whose feature map is 28 x 36 -- neither side a multiple of 16 or of anything the dense kernels tile by -- with two frames of ~2 600
voxels; no sparse level's live row count is a multiple of 128 or next to one.  ``graph_rpn`` is off so that the dense segment's nodes
are visible; the captured forms are tied to the eager one by tests/test_gpu_train_dense.py.  tests/test_train_step_audit_host.py
proves on the CPU that each check fails on the mistake it is there for."""
import numpy as np
import pytest
import torch

import train_step_audit_helpers as A
from mhead_train_helpers import small_batch, small_cfg

pytestmark = pytest.mark.gpu

CAR_RANGE = [0, -5.6, -3, 14.4, 5.6, 1]          # 288 x 224 x 40 voxels of 0.05 x 0.05 x 0.1 m: feature map 28 x 36
# (cloud seeds, voxels of the first frame): sparse level rows 5291 / 8673 / 4847 / 1651 / 1425 and 5491 / 8084 / 4402 / 1491 / 1423
BATCHES = (((0, 1), 2600), ((4, 5), 2700))


def car_cfg():
    """car.fhd with only point_cloud_range, anchor_ranges, post_center_range and max_voxels changed (as mhead_train_helpers.small_cfg
    reduces all.pp.mhead)."""
    from second_amd.models import CAR_FHD
    x0, y0, _, x1, y1, _ = CAR_RANGE
    return dict(CAR_FHD, point_cloud_range=list(CAR_RANGE), anchor_ranges=[[x0, y0, -1.0, x1, y1, -1.0]],
                post_center_range=[x0, y0, -2.2, x1, y1, 0.8], max_voxels=8000)


def car_batch(det, seeds, voxels, boxes=10):
    """(points, point_offsets, gt_boxes, gt_offsets): two clouds with ``voxels`` and ``voxels`` + 91 occupied voxels, and per frame ten
    boxes that are anchors of the map (centres at least 2 m inside the range) nudged by a few centimetres -- so every box has a
    positive anchor -- and turned by 0.2 .. 0.4 rad, which keeps the direction target off the bin edge an axis-parallel box sits on."""
    from second_amd import synthetic as syn
    rng = np.random.default_rng(1000 + seeds[0])
    clouds = [syn.syn_kitti_cloud(s, num_points=voxels + 400 + 37 * i, num_voxels=voxels + 91 * i, point_cloud_range=tuple(float(v) for v in CAR_RANGE))
              for i, s in enumerate(seeds)]
    pts, offs = syn.batch_clouds(clouds)
    anc = det.anchors.cpu().numpy()
    x0, y0, _, x1, y1, _ = CAR_RANGE
    inner = anc[(anc[:, 0] > x0 + 2) & (anc[:, 0] < x1 - 2) & (anc[:, 1] > y0 + 2) & (anc[:, 1] < y1 - 2)]
    gts = []
    for _ in seeds:
        b = inner[rng.choice(len(inner), boxes, replace=False)].astype(np.float32)
        b[:, :2] += rng.normal(0, 0.03, (boxes, 2)).astype(np.float32)
        b[:, 6] += rng.uniform(0.2, 0.4, boxes).astype(np.float32)
        gts.append(b)
    goffs = np.arange(len(seeds) + 1, dtype=np.int32) * boxes
    return [torch.from_numpy(a).cuda() for a in (pts, offs, np.concatenate(gts), goffs)]


def perturb_norms(det, seed=7):
    """Affine parameters and running statistics off their initial 1 / 0 / 0 / 1: a gamma read as 1 or a running statistic overwritten
    instead of blended would otherwise not show."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in det.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)


def device_packers(ops):
    """The expected weight images: the project's packers on the master weight a node recorded, cross-checked against the plain cast
    and the separate pack (ops.pack_weight)."""
    def sparse(w, dt, subm):
        w16, pk, pkt = ops.pack_weight_train(w.contiguous(), dt, subm)
        ref = ops.pack_weight(w.to(dt).contiguous())
        assert torch.equal(w16, w.to(dt)) and (pk is None) == (ref is None) and (pk is None or torch.equal(pk, ref))
        return w16, pk, pkt
    return dict(sparse=sparse, dense=lambda w, dt: ops.conv2d_pack_weight_train(w.contiguous(), dt))


def project_functions():
    import spconv.functional as Fsp
    from second_amd import ops
    return [getattr(Fsp, n) if hasattr(Fsp, n) else getattr(ops, n) for n in A.PROJECT_FUNCTIONS]


def run_steps(monkeypatch, tr, batches):
    import spconv.conv
    from second_amd import ops
    assert ops._op_hook is None
    steps = []
    with A.Recorder(monkeypatch, project_functions(), ops, spconv.conv.SparseConvolution) as rec:
        for k, ins in enumerate(batches):
            rec.step = k
            steps.append(A.audited_step(rec, tr, ins, native_params=getattr(tr, "_audit_native", ())))
        torch.cuda.synchronize()
    assert ops._op_hook is None and not ops._PREPACK
    return rec, steps


def audit_steps(rec, steps, tr, stacked, label):
    from second_amd import ops
    audit = A.Audit()
    packers = device_packers(ops)
    for k, got in enumerate(steps):
        nodes = rec.nodes_of(k)
        # step 2 (after an optimizer update, on another batch) is about wiring and state: its convolutions keep their wiring checks,
        # the fp64 references of the same kernels on a second batch are left out (they are two thirds of the audit's time)
        A.audit_nodes(nodes, audit, packers, conv_numerics=k == 0)
        got["graph"] = A.audit_graph(got["loss"], nodes, audit)
        A.audit_bucket(tr, nodes, got["before"], audit, stacked=stacked)
        A.audit_adamw(tr, got["before"], got["after"], audit, f"AdamW step {k + 1}")
    for call in rec.free_calls:
        if call.name == "voxelize":
            A.audit_voxel_means(call, audit, f"voxel means step {call.step + 1}")
    bns = [(n, m) for n, m in tr.det.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    A.audit_running_statistics([rec.nodes_of(k) for k in range(len(steps))], bns, audit)
    print()
    print(audit.report(label))
    return audit


CAR_NODES = {"IndiceConvFunction": 14, "BatchNormReluFunction": 14 + 6 + 1, "SparseToDenseFunction": 1, "Conv3x3Function": 6,
             "ConvTranspose1x1Function": 1, "HeadsLossFunction": 1}


@pytest.mark.parametrize("mode", ["bf16-dynamic", "bf16-static", "fp16-loss-scale"])
def test_car_fhd_step_every_node_against_fp64_on_its_own_inputs(monkeypatch, mode):
    """Measured worst error / bound per node kind: DESIGN.md 9h-a."""
    import spconv
    from second_amd.models import SecondDetector
    from second_amd.training import DeviceTrainer
    dtype = torch.float16 if mode.startswith("fp16") else torch.bfloat16
    torch.manual_seed(0)
    det = SecondDetector(car_cfg()).cuda()
    assert det.feature_map_size == [1, 28, 36]
    perturb_norms(det)
    tr = DeviceTrainer(det, amp_dtype=dtype)
    tr.graph_rpn = False
    batches = [car_batch(det, seeds, voxels) for seeds, voxels in BATCHES]
    if mode == "bf16-static":
        # static-capacity rows (what capture_step captures, run eagerly here): capacities from a dynamic pass per batch, the state put back
        state = {k: v.clone() for k, v in det.state_dict().items()}
        rows = {}
        for ins in batches:
            with torch.no_grad():
                tr.forward_loss(*ins)
            for m in det.middle_feature_extractor.modules():
                if isinstance(m, spconv.SparseConvolution) and not m.subm:
                    rows[m] = max(rows.get(m, 0), int(m.last_num_out))
        for m, n in rows.items():
            m.static_out_rows = int(-(-int(n * 1.25) // 256) * 256)
        det.load_state_dict(state)
        tr.static = True
    rec, steps = run_steps(monkeypatch, tr, batches)
    if tr.static:
        tr.check_overflow()
    heads = [det.rpn.conv_box, det.rpn.conv_cls, det.rpn.conv_dir_cls]
    stacked = [("HeadsLossFunction", arg, [getattr(m, name) for m in heads]) for arg, name in ((1, "weight"), (2, "bias"))]
    audit = audit_steps(rec, steps, tr, stacked, f"car.fhd 28 x 36, {mode}")
    assert not audit.failures(), audit.describe_failures()
    for k, got in enumerate(steps):
        nodes = rec.nodes_of(k)
        kinds = [n.kind for n in nodes]
        assert {kd: kinds.count(kd) for kd in set(kinds)} == CAR_NODES
        # one chain of 44 nodes: (nearly) every edge runs from one recorded node straight to the next and was compared bit for bit
        assert got["graph"]["project_nodes"] == len(nodes) == 44 and got["graph"]["links"] >= 40, got["graph"]
        # the conditions on the inputs
        for n in nodes:
            if n.kind == "IndiceConvFunction":
                live = (A.live_count(n.layer["in_dev"], n.args[0].shape[0]), A.live_count(n.layer["out_dev"], n.outputs[0].shape[0]))
                assert all(v % 128 not in (0, 1, 127) for v in live), live
                assert (n.args[0].shape[0] > live[0]) == (mode == "bf16-static")           # static: capacity rows behind the live ones
        loss_node = nodes[-1]
        labels = loss_node.args[3]
        assert loss_node.kind == "HeadsLossFunction" and int((labels > 0).sum(1).min()) >= 10
        # the sparse stack reads the voxeliser's 16-bit means, the first layer's input IS that tensor
        vox = [c for c in rec.free_calls if c.name == "voxelize" and c.step == k]
        assert len(vox) == 1 and vox[0].result["mean"].dtype == dtype
        assert A.same_bits(nodes[0].args[0], vox[0].result["mean"][:nodes[0].args[0].shape[0]])
        # the loss scale is what arrived at the loss: every gradient below it carries exactly that factor, the update divides it out
        scale = got["before"]["scale"]
        assert float(loss_node.grad_out[0]) == scale == (2.0 ** 12 if dtype == torch.float16 else 1.0)
    assert max(r["exempt"] for r in audit.rows) <= A.EXEMPT_CAP
    assert tr.steps == 2 and (tr.skipped_steps == 0)


def test_all_pp_mhead_step_hand_written_nodes_against_fp64_on_their_own_inputs(monkeypatch):
    """all.pp.mhead at mhead_train_helpers.small_cfg, bf16: PFNRadiusTrainFunction, PillarScatterFunction, the hand-written 128-channel
    3x3 convolutions and BatchNorms of the trunk's block 1, its 128 -> 128 1x1 deblock, SecondLossFunction on both heads' concatenated
    predictions.  The 64-channel convolutions, the strided ones, the other deblocks and the 1x1 heads stay on torch: allow-listed in
    the graph walk, not audited."""
    from second_amd.models import SecondDetector
    from second_amd.training import MultiHeadDeviceTrainer
    torch.manual_seed(0)
    det = SecondDetector(small_cfg()).cuda()
    perturb_norms(det)
    tr = MultiHeadDeviceTrainer(det, amp_dtype=torch.bfloat16)
    tr.graph_rpn = False
    tr._audit_native = list(det.parameters())         # parameters no recorded node produced a gradient for belong to torch's layers
    batches = [tuple(torch.from_numpy(a).cuda() for a in small_batch(det, seed=s)) for s in (0, 1)]
    rec, steps = run_steps(monkeypatch, tr, batches)
    audit = audit_steps(rec, steps, tr, (), "all.pp.mhead small_cfg, bf16")
    assert not audit.failures(), audit.describe_failures()
    for k in range(2):
        kinds = [n.kind for n in rec.nodes_of(k)]
        assert kinds[0] == "PFNRadiusTrainFunction" and kinds[1] == "PillarScatterFunction" and kinds[-1] == "SecondLossFunction"
        assert kinds.count("Conv3x3Function") == 5 and kinds.count("BatchNormReluFunction") >= 5, kinds        # block 1's 128 -> 128 layers
        assert steps[k]["graph"]["project_nodes"] == len(kinds)
        loss_node = rec.nodes_of(k)[-1]
        assert loss_node.args[0].shape[1] == 4800 + 8192            # both heads' anchors
    assert max(r["exempt"] for r in audit.rows) <= A.EXEMPT_CAP
