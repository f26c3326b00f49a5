"""-m gpu: the RPN convolutions in IEEE fp32 on v_mfma_f32_32x32x2_f32 (csrc/dense_f32.hip: sec_conv2d_nhwc_f32, sec_conv2d_nhwc_f32_tiles,
sec_conv1x1_chain_f32), ``RPNInference(backend="hip_f32")`` and ``prepare_inference(float32, exact=True, exact_rpn="hip")``.

Forward bounds are derived, not measured: an fp32 fma / sum chain of K terms is within (K + 2) * 2^-24 * (sum |x||w| + |b|) of the
exact value for ANY evaluation order (K = 9 * 128 = 1152 for the 3x3 conv); the integer case is exact in any order and tells fp32
products from the split-operand (bf16x3) ones with no tolerance at all."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_x3 import _sites
from test_gpu_heads_fp64 import BOUNDS, fp64_heads, setup  # noqa: F401  (setup: the module fixture of the whole-network test)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("batch,h,w,cout,relu", [(2, 200, 176, 128, True), (1, 37, 45, 128, False), (3, 8, 16, 256, True),
                                                 (2, 9, 17, 128, True), (1, 1, 1, 128, False)])
def test_conv2d_f32_is_within_the_fma_chain_bound_of_the_fp64_convolution(batch, h, w, cout, relu):
    from second_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 128, h, w, generator=g).mul_(3.0)
    x = torch.where(torch.rand(x.shape, generator=g) < 0.3, torch.zeros(()), x)       # ReLU-like inputs
    wt = torch.randn(cout, 128, 3, 3, generator=g) * 0.05
    bias = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1)
    mag = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), 1, 1)      # sum |x||w| + |b|
    y = ops.conv2d_nhwc_f32(_cl(x), ops.conv2d_pack_weight_f32(wt.cuda()), bias.cuda(), cout, relu=relu)
    assert y.dtype == torch.float32 and y.shape == (batch, cout, h, w) and y.is_contiguous(memory_format=torch.channels_last)
    y = y.cpu().double()
    if relu:
        ref = ref.clamp_min(0)
    err = (y - ref).abs()
    print(f"conv2d_f32 {batch}x{h}x{w}->{cout}: max|err|/max|ref| = {float(err.max()) / float(ref.abs().max()):.3e}   "
          f"worst share of the bound = {float((err / ((1152 + 2) * U * mag)).max()):.4f}")
    assert bool((err <= (1152 + 2) * U * mag).all())


def test_conv2d_f32_is_exact_on_integers_where_the_split_operand_form_is_not():
    """Odd integers below 512 on four input channels and every tap: products have <= 18 bits and every partial sum stays below
    2^24, so any fp32 evaluation order is exact -- while x_hi w_hi + x_hi w_lo + x_lo w_hi drops the x_lo w_lo terms.  Asymmetric
    weights: a transposed write or a permuted k order against the packed weights cannot pass."""
    from second_amd import ops
    g = torch.Generator().manual_seed(5)
    b, h, w = 2, 37, 45

    def odd(shape):
        return (torch.randint(-256, 256, shape, generator=g) * 2 + 1).float()
    x = torch.zeros(b, 128, h, w)
    chans = [3, 64, 65, 127]
    x[:, chans] = odd((b, 4, h, w)) * (torch.rand(b, 1, h, w, generator=g) >= 0.3)
    wt = odd((128, 128, 3, 3))
    bias = torch.randint(-999, 1000, (128,), generator=g).float()
    ref = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1)
    assert float(ref.abs().max()) < 2 ** 24
    y = ops.conv2d_nhwc_f32(_cl(x), ops.conv2d_pack_weight_f32(wt.cuda()), bias.cuda(), 128, relu=False)
    assert torch.equal(y.cpu().double(), ref)
    hi, lo = ops.split_bf16x2(_cl(x))
    y3 = ops.merge_bf16x2(*ops.conv2d_nhwc_x3(hi, lo, ops.conv2d_pack_weight_x3(wt.cuda()), bias.cuda(), 128, relu=False))
    assert not torch.equal(y3.cpu().double(), ref), "the split-operand conv is exact here too: the test cannot tell the arithmetics apart"


def test_conv2d_f32_all_zero_tiles_write_the_bias_and_match_the_full_form():
    from second_amd import ops
    g = torch.Generator().manual_seed(2)
    x = torch.zeros(2, 128, 64, 96)
    x[:, :, 10:14, 20:30] = torch.randn(2, 128, 4, 10, generator=g)
    x[1, :, 60:, 90:] = torch.randn(128, 4, 6, generator=g)
    wt = torch.randn(128, 128, 3, 3, generator=g) * 0.05
    bias = torch.randn(128, generator=g)
    pk = ops.conv2d_pack_weight_f32(wt.cuda())
    neg = torch.zeros(2, 128, 64, 96)
    neg[0, 5, 40, 50] = -0.0
    for inp in (x, torch.zeros(2, 128, 64, 96), neg):
        a = ops.conv2d_nhwc_f32(_cl(inp), pk, bias.cuda(), 128, relu=True, sparse_input=True)
        b = ops.conv2d_nhwc_f32(_cl(inp), pk, bias.cuda(), 128, relu=True, sparse_input=False)
        assert torch.equal(a, b)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))              # signs of zeros too
    ref = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1).clamp_min(0)
    y = ops.conv2d_nhwc_f32(_cl(x), pk, bias.cuda(), 128, relu=True, sparse_input=True).cpu().double()
    assert float((y - ref).abs().max()) / float(ref.abs().max()) <= 1e-5


def _bn_rpn(seed, bias=False):
    from second_amd.models import RPNV2
    torch.manual_seed(0)
    rpn = RPNV2().eval()
    g = torch.Generator().manual_seed(seed)
    for m in rpn.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            if bias:
                m.running_mean.copy_(torch.empty_like(m.running_mean).uniform_(-0.3, 0.1, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
                m.bias.data.uniform_(-0.1, 0.3, generator=g)                   # a non-zero background and border imprint
            else:
                m.running_mean.copy_(torch.empty_like(m.running_mean).uniform_(-0.1, 0.1, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
                m.weight.data.uniform_(0.8, 1.6, generator=g)
    return rpn, g


@pytest.mark.parametrize("batch,h,w,n", [(3, 200, 176, 700), (2, 37, 50, 12), (2, 120, 97, 4000)])
def test_fp32_mfma_rpn_on_live_tiles_is_bit_identical_to_the_full_convolutions(batch, h, w, n):
    """RPNInference(float32, backend="hip_f32") fed the sparse middle's rows: the list forms (lazy convs, last conv copying its
    background) against every-tile convolutions, on a network whose background is not zero, unwritten tiles poisoned with NaN."""
    import spconv
    from second_amd import ops
    from second_amd.models import RPNInference, SparseBEV
    rpn, g = _bn_rpn(4, bias=True)
    inf = RPNInference(rpn.cuda(), torch.float32, backend="hip_f32")
    assert inf.fp32 is not None and inf.fp32.name == "fp32" and len(inf.fp32_packed) == 6 and inf.fp32_chain is not None
    assert inf.background_convs == 6
    idx = _sites(batch, h, w, n, seed=h + n).cuda()
    feats = torch.randn(idx.shape[0], 64, generator=g).abs().cuda()
    sp = spconv.SparseConvTensor(feats, idx, [2, h, w], batch)
    last = []            # the map behind the last 3x3 conv (what the 1x1 tail reads)

    def run(x):
        ops.set_op_hook(lambda name, fn, a, kw, res: last.append(a[0].clone()) if name == "conv1x1_chain_f32" else None)
        try:
            with torch.no_grad():
                return {k: v.float().clone() for k, v in inf(x).items()}
        finally:
            ops.set_op_hook(None)
    inf.skip_background = False
    want = run(SparseBEV(sp))
    dense = run(sp.dense_channels_last_2d())
    inf.skip_background = True
    ops.POISON_LAZY_OUTPUTS = True
    try:
        got = run(SparseBEV(sp))
    finally:
        ops.POISON_LAZY_OUTPUTS = False
    live = inf.last_live_counts.cpu().numpy()
    tiles = ((h + 7) // 8) * ((w + 15) // 16)
    assert live.shape == (6, batch) and (batch == 1 or (live[:, -1] == 0).all())
    if n <= 3000:
        assert live[0].sum() < batch * tiles                       # the lists do leave tiles out: not a vacuous pass
    assert len(last) == 3 and torch.equal(last[0], last[1])
    assert torch.isfinite(last[2]).all(), "an unwritten (NaN-poisoned) tile reached the last conv's output"
    assert torch.equal(last[2], last[0])
    for k in want:
        assert torch.equal(dense[k], want[k]), k
        assert torch.equal(got[k], want[k]), k


def test_conv1x1_chain_f32_matches_fp64():
    """y = W2 relu(W1 x + b1) + b2: two chained K = 128 fp32 chains (ReLU is 1-Lipschitz), pixel count not a multiple of the
    128-pixel workgroup tile; both head widths."""
    from second_amd import ops
    g = torch.Generator().manual_seed(7)
    b, h, w = 2, 37, 45
    x = torch.randn(b, 128, h, w, generator=g).clamp_min(0) * 2.0
    w1 = torch.randn(128, 128, 1, 1, generator=g) * 0.1
    b1 = torch.randn(128, generator=g) * 0.3
    w2 = torch.randn(64, 128, 1, 1, generator=g) * 0.1
    w2[20:] = 0                                                   # padded head channels
    b2 = torch.randn(64, generator=g)
    w2b = torch.randn(128, 128, 1, 1, generator=g) * 0.1
    b2b = torch.randn(128, generator=g)
    gamma = 130 * U
    for wt2, bb2, cout2 in ((w2, b2, 64), (w2b, b2b, 128)):
        mid = F.conv2d(x.double(), w1.double(), b1.double())
        ref = F.conv2d(mid.clamp_min(0), wt2.double(), bb2.double())
        mag1 = F.conv2d(x.double().abs(), w1.double().abs(), b1.double().abs())
        bound = gamma * (2 * F.conv2d(mag1, wt2.double().abs()) + bb2.double().abs().view(1, -1, 1, 1))
        y = ops.conv1x1_chain_f32(_cl(x), ops.conv2d_pack_weight_f32(w1.cuda()), b1.cuda(), ops.conv2d_pack_weight_f32(wt2.cuda()), bb2.cuda(), cout2)
        assert y.dtype == torch.float32 and y.shape == (b, cout2, h, w) and y.is_contiguous(memory_format=torch.channels_last)
        err = (y.cpu().double() - ref).abs()
        print(f"conv1x1_chain_f32 cout2={cout2}: max|err|/max|ref| = {float(err.max()) / float(ref.abs().max()):.3e}")
        assert bool((err <= bound).all())


def test_fp32_mfma_rpn_inference_matches_the_torch_block():
    from second_amd.models import RPNInference
    rpn, g = _bn_rpn(3)
    rpn = rpn.cuda()
    x = torch.randn(2, 128, 200, 176, generator=g).clamp_min(0).cuda()
    with torch.no_grad():
        want = rpn(x)
        inf = RPNInference(rpn, torch.float32, backend="hip_f32")
        assert inf.fp32 is not None and inf.fp32.name == "fp32" and len(inf.fp32_packed) == 6 and inf.fp32_chain is not None
        got = inf(x.contiguous(memory_format=torch.channels_last))
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        a, b = got[k].float().cpu().numpy(), want[k].float().cpu().numpy()
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * float(np.abs(b).max()), err_msg=k)


def _detector(state, exact_rpn):
    from second_amd.models import SecondDetector, CAR_FHD
    det = SecondDetector(CAR_FHD)
    det.load_state_dict(state)
    det = det.eval().cuda()
    return det.prepare_inference(torch.float32, exact=True, exact_rpn=exact_rpn)


def test_head_tensors_of_the_exact_mode_on_the_fp32_mfma_rpn(setup):
    """The whole car.fhd network against the float64 chain, inside the project's existing fp32 bound (measured on the MI355X, worst
    head: see DESIGN.md section 2; torch's fp32 convolutions give 2.6e-6 / 2.5e-6)."""
    state, feats, coors, ref = setup
    det = _detector(state, "hip")
    assert det.arithmetic() == "fp32" and det.rpn.fp32 is not None and det.rpn.fp32.name == "fp32"
    with torch.no_grad():
        got = {k: v.double().contiguous() for k, v in det.network_forward(feats, coors, 2).items()}
    bmax, brms = BOUNDS["fp32"]
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        r, g = ref[k], got[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        emax = ((g - r).abs().max() / r.abs().max()).item()
        erms = ((g - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item()
        print(f"[fp32, exact_rpn=hip] {k}: max|err|/max|ref| = {emax:.3e}   rms(err)/rms(ref) = {erms:.3e}")
        assert emax <= bmax and erms <= brms, (k, emax, erms)


def test_exact_mode_on_the_fp32_mfma_rpn_calls_no_vendor_convolution(setup, monkeypatch):
    state, feats, coors, _ = setup
    det_hip, det_torch = _detector(state, "hip"), _detector(state, "torch")
    with torch.no_grad():
        want = det_hip.network_forward(feats, coors, 2)

    def refuse(*a, **k):
        raise AssertionError("vendor convolution / GEMM called")
    monkeypatch.setattr(torch.nn.functional, "conv2d", refuse)
    monkeypatch.setattr(torch, "conv2d", refuse)
    monkeypatch.setattr(torch, "addmm", refuse)
    with torch.no_grad():
        got = det_hip.network_forward(feats, coors, 2)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        with pytest.raises(AssertionError, match="vendor convolution"):          # the torch RPN does call them: the patch bites
            det_torch.network_forward(feats, coors, 2)


def test_exact_mode_on_the_fp32_mfma_rpn_is_capturable(setup):
    """One eager forward (sizes the empty-frame maps), then network_forward captured on a single stream and replayed on refreshed inputs."""
    from second_amd import ops
    state, feats, coors, _ = setup
    det = _detector(state, "hip")
    n = feats.shape[0]
    nd = torch.tensor([n], dtype=torch.int32, device="cuda")
    s_feats, s_coors = feats.clone(), coors.clone()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in det.network_forward(s_feats, s_coors, 2, num_active_dev=nd).items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.rt.capture_guard(), torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = det.network_forward(s_feats, s_coors, 2, num_active_dev=nd)
    for _ in range(2):
        s_feats.zero_()
        s_coors.zero_()
        for v in out.values():
            v.zero_()
        s_feats.copy_(feats)
        s_coors.copy_(coors)
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(out[k], eager[k]), k


def test_load_state_dict_into_the_prepared_exact_detector_repacks_the_fp32_images(setup):
    """Perturbed RPN weights loaded into a prepared detector give exactly what a detector prepared from those weights gives: the
    packed fp32 images follow the parameters and the empty-frame maps are rebuilt."""
    state, feats, coors, _ = setup
    det = _detector(state, "hip")
    with torch.no_grad():
        before = {k: v.clone() for k, v in det.network_forward(feats, coors, 2).items()}
    g = torch.Generator().manual_seed(11)
    raw = {k: (v * (1 + 0.05 * torch.randn(v.shape, generator=g).to(v.device)) if k.startswith("rpn.") and v.dim() == 4 else v)
           for k, v in state.items()}
    assert sum(1 for k in raw if not torch.equal(raw[k], state[k])) >= 8         # six 3x3 convs, the deblock, the heads
    fresh = _detector(raw, "hip")
    with torch.no_grad():
        want = {k: v.clone() for k, v in fresh.network_forward(feats, coors, 2).items()}
    det.load_state_dict(fresh.state_dict())
    with torch.no_grad():
        after = det.network_forward(feats, coors, 2)
    for k in want:
        assert not torch.equal(want[k], before[k]), k
        assert torch.equal(after[k], want[k]), k
