"""Teacher-forced audit of one 16-bit training step: record every node of a real step, then hold each node to its fp64 reference ON THE
INPUTS THE STEP ITSELF GAVE IT, and assert the wiring between the nodes.

Why node by node: a free-running fp64 chain cannot be compared with the 16-bit step (the two chains differ in the last bit
before a 16-bit store, a ReLU mask flips, twenty train-mode BatchNorm layers amplify it).  With every node's inputs taken from the
recording nothing compounds, the ReLU masks are those of the recorded activations, and the per-element bounds the kernel tests already
state apply unchanged:

    sparse convolution      indice_conv_bwd_helpers.reference / bounds / bound_dfeat     (the gather table is REBUILT here from the
                            recorded coordinates and the layer's kernel / stride / padding, not taken from the step)
    dense convolutions      dense_train_ref_helpers.conv_reference / wgrad_reference / bound_conv / bound_wgrad / bound_sum32
    BatchNorm + ReLU        dense_train_ref_helpers.BnRef  (rows and NHWC; its own rule for mask-ambiguous elements)
    losses                  train_ref_helpers.loss_ref in float64, tolerances of tests/test_gpu_train_edges.py
    AdamW                   train_ref_helpers.adamw_ref, tolerance of tests/test_gpu_train_edges.py::_adam_steps
    pillar layer            the module's own float64 formulation, bounds of tests/test_gpu_mhead_train.py; and per element
                            pfn_ref_helpers.check_train_undecided
    scatter / gather        bit equality

"Every node within its bound on its own inputs" + "every node's inputs are the tensors they should be" (the wiring assertions: weight
images, backward tables, gradient flow, gradient bucket, loss scale, completeness of the record against the autograd graph) pins the
step.  Nothing here knows whether the recorded functions are the project's (tests/test_gpu_train_step_audit.py) or the CPU emulation of
tests/test_train_step_audit_host.py, which proves that every check bites.
"""
import numpy as np
import torch

from indice_conv_bwd_helpers import U24, U_STORE, bound_dfeat, bound_dw, reference as sparse_bwd_reference, worst
from dense_train_ref_helpers import (TINY, BnRef, bound_conv, bound_sum32, bound_wgrad, conv_reference, gamma_n, store_floor,
                                     wgrad_reference)
import train_ref_helpers as TR

EXEMPT_CAP = 0.01            # share of a node's elements that may be mask-ambiguous (a condition on the inputs, not a measurement)

# torch-native autograd nodes a step may contain besides the project's functions: casts, views, copies, concatenations, the slices of
# the multi-head network, and the convolutions / BatchNorms the 16-bit step leaves on torch (other widths, strides, deblocks, heads).
NATIVE_ALLOWED = frozenset("""AccumulateGrad ToCopyBackward0 CloneBackward0 CatBackward0 SliceBackward0 ViewBackward0 ReshapeAliasBackward0
UnsafeViewBackward0 PermuteBackward0 TBackward0 TransposeBackward0 MulBackward0 AliasBackward0 CopySlices AsStridedBackward0
ConvolutionBackward0 MiopenConvolutionBackward0 MiopenConvolutionTransposeBackward0 CudnnConvolutionBackward0
CudnnConvolutionTransposeBackward0 NativeBatchNormBackward0 MiopenBatchNormBackward0 CudnnBatchNormBackward0 ReluBackward0
ConstantPadNdBackward0 SelectBackward0 ExpandBackward0 UnsqueezeBackward0 SqueezeBackward1 AddBackward0 NoneType""".split())

PROJECT_FUNCTIONS = ("IndiceConvFunction", "SparseToDenseFunction", "PillarScatterFunction", "BatchNormReluFunction", "Conv3x3Function",
                     "ConvTranspose1x1Function", "Heads1x1Function", "HeadsLossFunction", "SecondLossFunction", "PFNTrainFunction",
                     "PFNRadiusTrainFunction")
# kernel-level entry points of second_amd.ops that the op hook does not report: wrapped as module attributes
UNTRACED_OPS = ("pack_weight_train", "indice_conv_backward", "dense_to_sparse", "bn_relu_forward", "bn_relu_backward", "conv2d_wgrad",
                "conv2d_pack_weight_train")
TRACED_OPS = ("indice_conv", "sparse_to_dense", "pillar_scatter", "conv2d_nhwc", "voxelize", "second_loss")


# ------------------------------------------------------------------------------------------------------------------ small tools
def kind_of(dtype):
    assert dtype in (torch.bfloat16, torch.float16), dtype
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def a64(t):
    return t.detach().to("cpu").double().numpy()


def same_bits(a, b):
    """Bit equality of two tensors (shape, dtype and every bit; -0.0 is not 0.0, a NaN equals itself)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().to("cpu").contiguous(), b.detach().to("cpu").contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.view(view), b.view(view)))


def nhwc(t):
    """[B,C,H,W] tensor -> float64 [B,H,W,C] array."""
    return np.ascontiguousarray(a64(t).transpose(0, 2, 3, 1))


def rows_of(t):
    """The [P, C] float64 view a BatchNorm kernel has of its input: feature rows as they are, an image pixel-major."""
    return a64(t) if t.dim() == 2 else nhwc(t).reshape(-1, t.shape[1])


def live_count(num_dev, default):
    return int(default) if num_dev is None else min(int(num_dev.detach().reshape(-1)[0].item()), int(default))


# ------------------------------------------------------------------------------------------------------------------ the recorder
class Call:
    __slots__ = ("name", "phase", "step", "args", "kwargs", "result")

    def __init__(self, name, phase, step, args, kwargs, result):
        self.name, self.phase, self.step, self.args, self.kwargs, self.result = name, phase, step, args, kwargs, result

    def arg(self, index, key):
        return self.args[index] if len(self.args) > index else self.kwargs.get(key)


class Node:
    """One call of a project autograd function.  args: the inputs (tensors detached; parameters and small tensors cloned, because the
    optimizer and the BatchNorm kernels change them in place later); outputs; grad_out[i]: the gradient that arrived at output i;
    grad_in[i]: the gradient produced for input i; calls: the kernel-level calls made inside forward ("fwd") and backward ("bwd");
    layer: the sparse convolution module's geometry and coordinates; after: in-place results (running statistics) after forward."""

    def __init__(self, kind, index, step):
        self.kind, self.index, self.step = kind, index, step
        self.args, self.arg_refs, self.outputs, self.out_refs = [], [], [], ()
        self.grad_out, self.grad_in, self.calls, self.grad_fn = None, None, [], None
        self.layer, self.after = None, {}

    def __repr__(self):
        return f"node {self.index} ({self.kind}, step {self.step})"

    def tensor_slots(self):
        """Argument index of every input slot of the autograd node (its next_functions): the tensor arguments, in order."""
        return [i for i, a in enumerate(self.arg_refs) if isinstance(a, torch.Tensor)]

    def calls_of(self, name, phase):
        return [c for c in self.calls if c.name == name and c.phase == phase]

    def one_call(self, name, phase):
        c = self.calls_of(name, phase)
        assert len(c) == 1, f"{self!r}: {len(c)} {phase} calls of {name}, expected one"
        return c[0]


def _keep(a):
    if not isinstance(a, torch.Tensor):
        return a
    if (a.is_leaf and a.requires_grad) or a.numel() <= 65536:
        return a.detach().clone()
    return a.detach()


class Recorder:
    """with Recorder(monkeypatch, functions, ops_module, conv_class) as rec: ... -- records every ``apply`` of the given autograd
    function classes (see :class:`Node`), the kernel-level calls of ``ops_module`` made inside them (through ``ops.set_op_hook`` for the
    traced entry points, by wrapping the module attribute for the others) and, per sparse convolution module, coordinates and geometry.
    ``rec.step`` labels the nodes recorded from now on.  The hook is reset and the attributes are restored on exit, whatever happened."""

    def __init__(self, monkeypatch, functions, ops_module, conv_class=None):
        self.mp, self.functions, self.ops, self.conv_class = monkeypatch, list(functions), ops_module, conv_class
        self.nodes, self.free_calls, self.step = [], [], 0
        self._stack, self._bwd = [], None

    # -- installation
    def __enter__(self):
        self._ctx = self.mp.context()
        m = self._ctx.__enter__()
        try:
            origs = [(cls, cls.apply) for cls in self.functions]        # all of them first: a subclass must not pick up its base's wrapper
            for cls, orig in origs:
                m.setattr(cls, "apply", staticmethod(self._wrap_apply(cls, orig)))
            for name in UNTRACED_OPS + TRACED_OPS:
                fn = getattr(self.ops, name, None)
                if fn is None or hasattr(fn, "__wrapped_op__"):        # absent in an emulation / reported by the op hook
                    continue
                m.setattr(self.ops, name, self._wrap_op(name, fn))
            if self.conv_class is not None:
                m.setattr(self.conv_class, "forward", self._wrap_conv(self.conv_class.forward))
            self.ops.set_op_hook(lambda name, fn, args, kwargs, res: self._on_call(name, args, kwargs, res))
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        try:
            self.ops.set_op_hook(None)
        finally:
            self._ctx.__exit__(*exc)
        return False

    # -- what the wrappers do
    def _on_call(self, name, args, kwargs, res):
        node = self._stack[-1] if self._stack else self._bwd
        phase = "fwd" if self._stack else ("bwd" if node is not None else "free")
        (node.calls if node is not None else self.free_calls).append(Call(name, phase, self.step, args, dict(kwargs), res))

    def _wrap_op(self, name, fn):
        def wrapped(*args, **kwargs):
            res = fn(*args, **kwargs)
            self._on_call(name, args, kwargs, res)
            return res
        return wrapped

    def _wrap_conv(self, forward):
        rec = self

        def wrapped(mod, x):
            first = len(rec.nodes)
            in_idx, in_shape, in_dev = x.indices, list(x.spatial_shape), x.num_active_dev
            out = forward(mod, x)
            for node in rec.nodes[first:]:
                if node.kind == "IndiceConvFunction":
                    node.layer = dict(module=mod, in_indices=in_idx, out_indices=out.indices, in_shape=in_shape, in_dev=in_dev,
                                      out_dev=out.num_active_dev, ksize=list(mod.kernel_size), stride=list(mod.stride),
                                      padding=list(mod.padding), subm=bool(mod.subm))
            return out
        return wrapped

    def _wrap_apply(self, cls, orig):
        rec = self

        def apply(*args):
            node = Node(cls.__name__, len(rec.nodes), rec.step)
            node.args, node.arg_refs = [_keep(a) for a in args], list(args)
            rec.nodes.append(node)
            rec._stack.append(node)
            try:
                out = orig(*args)
            finally:
                rec._stack.pop()
            outs = out if isinstance(out, tuple) else (out,)
            node.out_refs = outs
            node.outputs = [o.detach() if isinstance(o, torch.Tensor) else o for o in outs]
            if cls.__name__ == "BatchNormReluFunction":
                node.after = dict(running_mean=args[3].detach().clone(), running_var=args[4].detach().clone())
            elif cls.__name__ in ("PFNTrainFunction", "PFNRadiusTrainFunction"):
                node.after = dict(running_mean=args[6].detach().clone(), running_var=args[7].detach().clone())
            node.grad_fn = next((o.grad_fn for o in outs if isinstance(o, torch.Tensor) and o.grad_fn is not None), None)
            if node.grad_fn is not None:
                node.grad_fn.register_prehook(lambda grad_outputs, node=node: rec._enter_backward(node))
                node.grad_fn.register_hook(lambda grad_inputs, grad_outputs, node=node: rec._leave_backward(node, grad_inputs, grad_outputs))
            return out
        return apply

    def _enter_backward(self, node):
        self._bwd = node

    def _leave_backward(self, node, grad_inputs, grad_outputs):
        keep = lambda g: None if g is None else g.detach()
        # autograd keeps one input slot per TENSOR argument: spread them over the argument list (None for everything else)
        slots = node.tensor_slots()
        assert len(slots) == len(grad_inputs), (node, len(slots), len(grad_inputs))
        node.grad_in = [None] * len(node.arg_refs)
        for i, g in zip(slots, grad_inputs):
            node.grad_in[i] = keep(g)
        node.grad_out = [keep(g) for g in grad_outputs]
        self._bwd = None

    def nodes_of(self, step):
        return [n for n in self.nodes if n.step == step]


# ------------------------------------------------------------------------------------------------------------------ the findings
class Audit:
    """Rows of (node, kind, check, error / bound, exempt share).  A row fails when its ratio exceeds 1 (a NaN or a wiring mismatch is
    infinite) or when more than EXEMPT_CAP of the node's elements had to be exempted as mask-ambiguous."""

    def __init__(self):
        self.rows, self.audited, self.seconds, self.numerics = [], set(), {}, True

    def add(self, node, check, ratio, exempt=0.0, note=""):
        ratio = float(ratio)
        is_node = isinstance(node, Node)
        self.rows.append(dict(node=node.index if is_node else node, kind=node.kind if is_node else str(node), step=node.step if is_node else None,
                              check=check, ratio=ratio if np.isfinite(ratio) else float("inf"), exempt=float(exempt), note=note))

    def require(self, node, check, ok, note=""):
        self.add(node, check, 0.0 if ok else float("inf"), note=note)

    def failures(self):
        return [r for r in self.rows if not r["ratio"] <= 1.0 or r["exempt"] > EXEMPT_CAP]

    def failed_nodes(self):
        return {r["node"] for r in self.failures()}

    def summary(self):
        """{node kind: (worst ratio, largest exempt share, nodes)}."""
        out = {}
        for r in self.rows:
            w, e, nodes = out.get(r["kind"], (0.0, 0.0, set()))
            out[r["kind"]] = (max(w, r["ratio"]), max(e, r["exempt"]), nodes | {r["node"]})
        return {k: (w, e, len(n)) for k, (w, e, n) in sorted(out.items())}

    def report(self, title):
        lines = [f"{title}: worst error / bound and mask-ambiguous share per node kind"]
        for k, (w, e, n) in self.summary().items():
            lines.append(f"  {k:28s} nodes {n:3d}   worst ratio {w:8.4f}   exempt {100 * e:7.4f} %" +
                         (f"   reference {self.seconds[k]:5.2f} s" if k in self.seconds else ""))
        return "\n".join(lines)

    def describe_failures(self):
        return "\n".join(f"node {r['node']} {r['kind']} step {r['step']} [{r['check']}] ratio {r['ratio']:.4g} exempt {r['exempt']:.4g} {r['note']}"
                         for r in self.failures())


# ------------------------------------------------------------------------------------------------------------------ sparse convolution
def geometry_table(in_idx, out_idx, shape, ksize, stride, padding):
    """nbr[o][k] = the input row at cell out[o] * stride - padding + k, k = (kz * kH + ky) * kW + kx, or -1: the gather table of a
    sparse convolution from coordinates and layer geometry alone ([n, 4] rows of (batch, z, y, x), ``shape`` of the INPUT grid)."""
    ii, oo = np.asarray(in_idx, np.int64), np.asarray(out_idx, np.int64)
    d, h, w = (int(s) for s in shape)
    lin = lambda b, z, y, x: ((b * d + z) * h + y) * w + x
    keys = lin(ii[:, 0], ii[:, 1], ii[:, 2], ii[:, 3])
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    assert len(sk) == 0 or (np.diff(sk) > 0).all(), "duplicate input coordinates"
    assert len(ii) == 0 or ((ii[:, 1:] >= 0).all() and (ii[:, 1] < d).all() and (ii[:, 2] < h).all() and (ii[:, 3] < w).all())
    kvol = int(np.prod(ksize))
    nbr = -np.ones((len(oo), kvol), np.int32)
    k = 0
    for kz in range(ksize[0]):
        for ky in range(ksize[1]):
            for kx in range(ksize[2]):
                z = oo[:, 1] * stride[0] - padding[0] + kz
                y = oo[:, 2] * stride[1] - padding[1] + ky
                x = oo[:, 3] * stride[2] - padding[2] + kx
                ok = (z >= 0) & (z < d) & (y >= 0) & (y < h) & (x >= 0) & (x < w)
                q = lin(oo[:, 0], z, y, x)
                pos = np.clip(np.searchsorted(sk, q), 0, max(len(sk) - 1, 0))
                hit = ok & (sk[pos] == q) if len(sk) else np.zeros(len(oo), bool)
                nbr[hit, k] = order[pos[hit]]
                k += 1
    return nbr


def sparse_forward_reference(feat, w16, nbr):
    """(ref64, mag) of out[o] = sum_k feat[nbr[o][k]] @ w16[k] with the ALREADY ROUNDED operands."""
    f = np.asarray(feat, np.float64)
    w = np.asarray(w16, np.float64)
    w = w.reshape(-1, w.shape[-2], w.shape[-1])
    kvol, cin, cout = w.shape
    f0 = np.concatenate([f, np.zeros((1, cin))])
    idx = np.where(nbr < 0, len(f), nbr)
    wf, wa = w.reshape(kvol * cin, cout), np.abs(w).reshape(kvol * cin, cout)
    ref, mag = np.zeros((len(nbr), cout)), np.zeros((len(nbr), cout))
    for r0 in range(0, len(nbr), 4096):
        g = f0[idx[r0:r0 + 4096]].reshape(-1, kvol * cin)
        ref[r0:r0 + 4096] = g @ wf
        mag[r0:r0 + 4096] = np.abs(g) @ wa
    return ref, mag


def audit_indice_conv(node, audit, packers):
    feat, master = node.args[0], node.args[1]
    kind = kind_of(feat.dtype)
    L = node.layer
    if L is None:
        return audit.require(node, "layer geometry recorded", False)
    fwd = node.one_call("indice_conv", "fwd")
    w16_used, nbr_out_used, packed_used = fwd.args[1], fwd.args[2], fwd.kwargs.get("packed")
    rb = node.arg_refs[2]
    # ---- weight images: what the kernels received is the image of the master weight as it is NOW
    w16, pk, pkt = packers["sparse"](master, feat.dtype, L["subm"])
    audit.require(node, "16-bit weight = round16(master)", same_bits(w16, master.to(feat.dtype)) and same_bits(w16_used, w16))
    audit.require(node, "forward weight image = pack(round16(master))", same_bits(packed_used, pk))
    # ---- tables: rebuilt from the coordinates; the step's own must agree on the live rows
    n_in, n_out = live_count(L["in_dev"], feat.shape[0]), live_count(L["out_dev"], node.outputs[0].shape[0])
    in_idx, out_idx = L["in_indices"].detach().cpu().numpy()[:n_in], L["out_indices"].detach().cpu().numpy()[:n_out]
    pad = [k // 2 for k in L["ksize"]] if L["subm"] else L["padding"]
    nbr = geometry_table(in_idx, out_idx, L["in_shape"], L["ksize"], [1, 1, 1] if L["subm"] else L["stride"], pad)
    audit.require(node, "forward table is the rulebook's", nbr_out_used is rb.nbr_out)
    audit.require(node, "nbr_out = table of the coordinates", np.array_equal(nbr_out_used.detach().cpu().numpy()[:n_out], nbr))
    # ---- forward
    f64, w64 = a64(feat)[:n_in], a64(w16_used)
    kvol, cin, cout = int(np.prod(L["ksize"])), w64.shape[-2], w64.shape[-1]
    if audit.numerics:
        ref, mag = sparse_forward_reference(f64, w64, nbr)
        audit.add(node, "forward", worst(a64(node.outputs[0])[:n_out], ref, bound_dfeat(ref, mag, kvol, cin, kind)))
    if node.grad_in is None:
        return
    # ---- backward: its own arguments, then the gradients
    bwd = node.one_call("indice_conv_backward", "bwd")
    audit.require(node, "backward got this layer's nbr_out", bwd.args[2] is rb.nbr_out)
    audit.require(node, "backward got this layer's nbr_in", bwd.args[3] is rb.nbr_in and (rb.nbr_in is None) == L["subm"])
    if not L["subm"] and bwd.args[3] is not None:
        inv = -np.ones((n_in, kvol), np.int32)
        for k in range(kvol):
            o = np.nonzero(nbr[:, k] >= 0)[0]
            inv[nbr[o, k], k] = o
        got = bwd.args[3].detach().cpu().numpy()[:n_in]
        audit.require(node, "nbr_in = inverse table of the coordinates", np.array_equal(np.where(got >= n_out, -1, got), inv))
    audit.require(node, "backward 16-bit weight = round16(master)", same_bits(bwd.args[1], w16))
    audit.require(node, "data-gradient weight image = pack^T(round16(master))", same_bits(bwd.kwargs.get("packed_dgrad"), pkt))
    audit.require(node, "backward features are the forward's", same_bits(bwd.args[0], feat))
    audit.require(node, "backward dout is the arriving gradient", same_bits(bwd.args[4], node.grad_out[0].contiguous()))
    if not audit.numerics:
        return
    dout = a64(node.grad_out[0])[:n_out]
    r = sparse_bwd_reference(f64, w64, nbr, dout)
    dfeat, dw = node.grad_in[0], node.grad_in[1]
    if dfeat is not None:
        audit.add(node, "data gradient", worst(a64(dfeat)[:n_in], r[0], bound_dfeat(r[0], r[2], kvol, cout, kind)))
    if dw is not None:
        audit.require(node, "weight gradient is fp32", dw.dtype == torch.float32)
        audit.add(node, "weight gradient", worst(a64(dw).reshape(r[1].shape), r[1], bound_dw(r[3], r[4])))


# ------------------------------------------------------------------------------------------------------------------ BatchNorm + ReLU
def audit_bn(node, audit, packers):
    y, gamma, beta, rm0, rv0, eps, mom, relu, rows_dev = (node.args + [None])[:9]
    kind = kind_of(y.dtype)
    yr = rows_of(y)
    live = live_count(rows_dev, yr.shape[0])
    dz = None if node.grad_out is None else rows_of(node.grad_out[0])
    ref = BnRef(yr, dz, a64(gamma), a64(beta), eps, mom, relu, live=live, running_mean=a64(rm0), running_var=a64(rv0), kind=kind,
                capacity=yr.shape[0])
    exempt = ref.ambiguous_fraction
    fwd = node.one_call("bn_relu_forward", "fwd")
    audit.require(node, "kernel got eps / momentum / relu of the module", (float(fwd.args[3]), float(fwd.args[4]), bool(fwd.arg(7, "relu"))) ==
                  (float(eps), float(mom), bool(relu)))
    z = rows_of(node.outputs[0])
    dy = None if node.grad_in is None or node.grad_in[0] is None else rows_of(node.grad_in[0])
    w = ref.worst_elements(z=z, dy=dy)
    audit.add(node, "z", w["z"], exempt)
    _, mean, invstd = fwd.result
    ch = ref.channel_ratios(mean=a64(mean), invstd=a64(invstd), running_mean=a64(node.after["running_mean"]),
                            running_var=a64(node.after["running_var"]))
    for k, v in ch.items():
        audit.add(node, k, v)
    if node.grad_in is None:
        return
    bwd = node.one_call("bn_relu_backward", "bwd")
    rows_ref = node.arg_refs[8] if len(node.arg_refs) > 8 else None
    audit.require(node, "backward got the forward's y, statistics, relu flag and row count",
                  same_bits(bwd.args[1], y) and same_bits(bwd.args[4], mean) and same_bits(bwd.args[5], invstd)
                  and bool(bwd.arg(6, "relu")) == bool(relu) and bwd.kwargs.get("rows_dev") is rows_ref)
    audit.require(node, "backward dz is the arriving gradient", same_bits(bwd.args[0], node.grad_out[0]))
    if dy is not None:
        audit.add(node, "dy", w["dy"], exempt)
    for k, v in ref.channel_ratios(dgamma=a64(node.grad_in[1]), dbeta=a64(node.grad_in[2])).items():
        audit.add(node, k, v, exempt)


# ------------------------------------------------------------------------------------------------------------------ dense convolutions
def _conv_weight_views(node, master):
    """(forward conv weight [Cout,Cin,k,k], k, index of the forward image, index of the backward image, dW from the [co][ci] form)."""
    if node.kind == "ConvTranspose1x1Function":         # weight [Cin, Cout, 1, 1]: the forward is the 1x1 conv with the transposed matrix
        return master.transpose(0, 1).contiguous(), 1, 1, 0, lambda d: d.transpose(0, 1)
    return master, master.shape[2], 0, 1, lambda d: d


def audit_dense_conv(node, audit, packers):
    """Conv3x3Function, ConvTranspose1x1Function, Heads1x1Function and the convolution inside HeadsLossFunction."""
    x, master = node.args[0], node.args[1]
    bias = node.args[2] if node.kind in ("Heads1x1Function", "HeadsLossFunction") else None
    kind = kind_of(x.dtype)
    wconv, k, i_f, i_b, dw_form = _conv_weight_views(node, master)
    images = packers["dense"](master, x.dtype)
    convs = node.calls_of("conv2d_nhwc", "fwd")
    audit.require(node, "one forward convolution", len(convs) == 1)
    fwd = convs[0]
    audit.require(node, "forward weight image = pack(round16(master))", same_bits(fwd.args[1], images[i_f]))
    audit.require(node, "forward geometry", (int(fwd.args[4]), int(fwd.arg(5, "stride")), int(fwd.arg(6, "pad")), bool(fwd.kwargs.get("relu", False))) ==
                  (k, 1, k // 2, False))
    audit.require(node, "forward input is the node's", same_bits(fwd.args[0], x))
    w16 = a64(wconv.to(x.dtype))
    x64 = nhwc(x)
    y = fwd.result
    if audit.numerics:
        ref, mag, terms = conv_reference(x64, w16, bias=None if bias is None else a64(bias.float()))
        audit.add(node, "forward", worst(nhwc(y), ref, bound_conv(ref, mag, terms, kind, bias=bias is not None)))
    if node.kind != "HeadsLossFunction":
        audit.require(node, "output is the convolution's", same_bits(node.outputs[0], y))
    if node.grad_in is None:
        return y, None
    if node.kind == "HeadsLossFunction":
        dy_t = node.one_call("conv2d_wgrad", "bwd").args[1]
    else:
        dy_t = node.grad_out[0]
    dy = nhwc(dy_t)
    dx, dw = node.grad_in[0], node.grad_in[1]
    if dx is not None:
        bconv = node.one_call("conv2d_nhwc", "bwd")
        audit.require(node, "data-gradient weight image = pack(flip^T(round16(master)))", same_bits(bconv.args[1], images[i_b]))
        audit.require(node, "data gradient reads the arriving gradient", same_bits(bconv.args[0], dy_t.contiguous(memory_format=torch.channels_last)))
        if audit.numerics:
            r, m, t = conv_reference(dy, w16, transposed_dgrad=True)
            audit.add(node, "data gradient", worst(nhwc(dx), r, bound_conv(r, m, t, kind)))
    if dw is not None:
        wg = node.one_call("conv2d_wgrad", "bwd")
        audit.require(node, "weight gradient reads the forward's input and the arriving gradient",
                      same_bits(wg.args[0], x) and same_bits(wg.args[1], dy_t.contiguous(memory_format=torch.channels_last)))
        audit.require(node, "weight gradient is fp32", dw.dtype == torch.float32)
        if audit.numerics:
            r, m, t = wgrad_reference(x64, dy, k)
            got = a64(dw)
            if node.kind == "ConvTranspose1x1Function":
                got = got.transpose(1, 0, 2, 3)
            audit.add(node, "weight gradient", worst(got, r, bound_wgrad(m, t)))
    if bias is not None and node.grad_in[2] is not None:
        s, sa = dy.sum((0, 1, 2)), np.abs(dy).sum((0, 1, 2))
        n = dy.shape[0] * dy.shape[1] * dy.shape[2]
        if node.kind == "HeadsLossFunction":       # tests/test_gpu_train_edges.py: the column sums of the RETURNED gradient within 1e-5 of their mass
            audit.add(node, "bias gradient", worst(a64(node.grad_in[2]), s, 1e-5 * sa + TINY))
        else:
            audit.add(node, "bias gradient", worst(a64(node.grad_in[2]), s, bound_sum32(sa, n)))
    return y, dy_t


# ------------------------------------------------------------------------------------------------------------------ losses
def _scalar_ratio(got, want):
    """tests/test_gpu_train_edges.py::_check_scalars: 1e-4 relative; a term whose reference is exactly zero may be off by 1e-7."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return worst(got, want, np.where(want == 0, 1e-7, 1e-4 * np.abs(want)))


def loss_reference(cls, box, dirp, labels, reg, anchors, imp, **kw):
    """train_ref_helpers.loss_ref with class logits that are EXACTLY zero moved to 1e-300.
    The reference writes the cross entropy as clamp(x, min=0) - x t + log1p(exp(-|x|)) and differentiates it by autograd.  The
    function is smooth (softplus(x) - x t, derivative sigmoid(x) - t), but that FORMULA has a kink in both of its pieces at x = 0,
    where autograd's conventions (clamp passes the gradient at its bound, sign(0) = 0) return 1 - t instead of sigmoid(0) - t = 1/2 - t.
    In fp32 an exact zero does not occur; 16-bit logits hit it (56 of 259 840 class logits of the first all.pp.mhead step), and the
    kernels, which evaluate p - t, are right there.  At 1e-300 both pieces are differentiable, and every value and derivative of the
    smooth function moves by less than 1e-300 -- nothing a float64 comparison sees."""
    cls = np.asarray(cls, np.float64)
    return TR.loss_ref(np.where(cls == 0.0, 1e-300, cls), box, dirp, labels, reg, anchors, imp, **kw)


def _split_heads(y, a, nc, bins):
    """[B, HW, 64] stacked head rows (box | cls | dir | padding, anchor-major inside a head) -> the loss's [B, a HW, code] tensors."""
    b, hw, _ = y.shape
    out, c0 = [], 0
    for code in (7, nc, bins):
        if code:
            out.append(np.ascontiguousarray(y[..., c0:c0 + a * code].reshape(b, hw, a, code).transpose(0, 2, 1, 3)).reshape(b, a * hw, code))
        else:
            out.append(None)
        c0 += a * code
    return out, c0


def _stack_heads(parts, b, hw, a, width):
    want, c0 = np.zeros((b, hw, width)), 0
    for p in parts:
        if p is None:
            continue
        code = p.shape[-1]
        want[..., c0:c0 + a * code] = p.reshape(b, a, hw, code).transpose(0, 2, 1, 3).reshape(b, hw, a * code)
        c0 += a * code
    return want


def audit_heads_loss(node, audit, packers):
    y, dy_t = audit_dense_conv(node, audit, packers)
    labels, reg, anchors, imp, a, nc, bins, cfg = node.args[3:11]
    kind = kind_of(y.dtype)
    b, hc, h, w = y.shape
    yr = nhwc(y).reshape(b, h * w, hc)
    (box, cls, dirp), tot = _split_heads(yr, int(a), int(nc), int(bins))
    lcfg = {k: v for k, v in cfg.items() if k in TR.LOSS_KEYS}
    ref6, r_cls, r_box, r_dir = loss_reference(cls, box, dirp, labels.cpu().numpy(), reg.cpu().numpy(), anchors.cpu().numpy(), imp.cpu().numpy(),
                                               num_class=int(nc), num_direction_bins=int(bins), **lcfg)
    audit.add(node, "loss scalars", _scalar_ratio(a64(node.outputs[1]), ref6))
    audit.require(node, "loss is out6[0]", same_bits(node.outputs[0], node.outputs[1][0]))
    if dy_t is None:
        return
    g = float(node.grad_out[0].double().item())
    want = _stack_heads([r_box, r_cls, r_dir], b, h * w, int(a), hc) * g
    got = nhwc(dy_t).reshape(b, h * w, hc)
    rel, sub = (2.0 ** -8, 0.0) if kind == "bf16" else (2.0 ** -10, 2.0 ** -24)      # test_heads_loss_against_the_float64_loss
    audit.add(node, "head gradient", worst(got, want, rel * np.abs(want) + 1e-6 * np.abs(want).max() + sub + TINY))
    audit.require(node, "channels behind the heads are zero", bool(np.all(got[..., tot:] == 0)))


def audit_second_loss(node, audit, packers):
    cls, box, dirp, labels, reg, anchors, imp, cfg = node.args[:8]
    b = cls.shape[0]
    nc, bins = int(cfg.get("num_class", 1)), (0 if dirp is None else int(cfg.get("num_direction_bins", 2)))
    f = lambda t, k: a64(t.reshape(b, -1, k).float())
    lcfg = {k: v for k, v in cfg.items() if k in TR.LOSS_KEYS}
    ref6, r_cls, r_box, r_dir = loss_reference(f(cls, nc), f(box, 7), None if dirp is None else f(dirp, bins), labels.cpu().numpy(),
                                               reg.cpu().numpy(), anchors.cpu().numpy(), imp.cpu().numpy(), num_class=nc,
                                               num_direction_bins=bins, **lcfg)
    audit.add(node, "loss scalars", _scalar_ratio(a64(node.outputs[1]), ref6))
    if node.grad_in is None:
        return
    g = float(node.grad_out[0].double().item())
    for name, got, want, src in (("cls", node.grad_in[0], r_cls, cls), ("box", node.grad_in[1], r_box, box), ("dir", node.grad_in[2], r_dir, dirp)):
        if want is None or got is None:
            continue
        want = want * g
        # tests/test_gpu_train_edges.py::_check_grad (rtol 1e-4, atol 1e-6 of the largest entry) for the fp32 kernel result, then the
        # ONE rounding of `.to(dtype)` when the predictions are 16-bit
        u16 = 0.0 if src.dtype == torch.float32 else U_STORE[kind_of(src.dtype)]
        floor = store_floor(kind_of(src.dtype)) if u16 else 0.0
        tol = (1e-4 + u16) * np.abs(want) + 1e-6 * np.abs(want).max() + 1e-9 + floor
        audit.add(node, f"d_{name}", worst(a64(got.reshape(b, -1, want.shape[-1]).float()), want, tol))


# ------------------------------------------------------------------------------------------------------------------ data movement
def audit_sparse_to_dense(node, audit, packers):
    feat, idx, batch, shape, num_dev, cl2d = (node.args + [None, False])[:6]
    n = live_count(num_dev, feat.shape[0])
    f, ix = feat.detach().cpu()[:n], idx.detach().cpu().long()[:n]
    d, h, w = (int(s) for s in shape)
    c = feat.shape[1]
    dense = torch.zeros((int(batch), c, d, h, w), dtype=feat.dtype)
    dense[ix[:, 0], :, ix[:, 1], ix[:, 2], ix[:, 3]] = f
    want = dense.reshape(int(batch), c * d, h, w) if cl2d else dense
    audit.require(node, "forward: rows at their cells, zero elsewhere", same_bits(node.outputs[0], want))
    if cl2d:
        audit.require(node, "forward: channels-last image", node.outputs[0].is_contiguous(memory_format=torch.channels_last))
    if node.grad_in is None or node.grad_in[0] is None:
        return
    g = node.grad_out[0].detach().cpu()
    g5 = g.reshape(int(batch), c, d, h, w) if cl2d else g
    rows = g5[ix[:, 0], :, ix[:, 1], ix[:, 2], ix[:, 3]]
    audit.require(node, "backward: every row gathered from its own cell and depth slice", same_bits(node.grad_in[0].detach().cpu()[:n], rows))
    call = node.one_call("dense_to_sparse", "bwd")
    dev_ref = node.arg_refs[4] if len(node.arg_refs) > 4 else None
    audit.require(node, "backward: depth and live count of the forward",
                  int(call.kwargs.get("depth", 0)) == (d if cl2d else 0) and call.kwargs.get("num_dev") is dev_ref)


def audit_pillar_scatter(node, audit, packers):
    feat, coords, batch, ny, nx = node.args[:5]
    f, ix = feat.detach().cpu(), coords.detach().cpu().long()
    want = torch.zeros((int(batch), feat.shape[1], int(ny), int(nx)), dtype=feat.dtype)
    want[ix[:, 0], :, ix[:, 2], ix[:, 3]] = f
    audit.require(node, "forward: pillars at their cells, zero elsewhere", same_bits(node.outputs[0], want))
    if node.grad_in is None or node.grad_in[0] is None:
        return
    g = node.grad_out[0].detach().cpu()
    audit.require(node, "backward: every pillar gathered from its own cell", same_bits(node.grad_in[0], g[ix[:, 0], :, ix[:, 2], ix[:, 3]]))


# ------------------------------------------------------------------------------------------------------------------ pillar layer
PFN_TOL = {"out": 2e-4, "d_linear_weight": 2e-3, "d_norm_weight": 2e-3, "d_norm_bias": 2e-3, "running_mean": 1e-5, "running_var": 1e-5}


def pfn_module(kind, channels, eps, momentum, geom):
    """The pillar layer's module (torch formulation off the GPU) for a recorded node's geometry (vx, vy, x_offset, y_offset)."""
    from second_amd import models
    vx, vy, xo, yo = (float(v) for v in geom)
    cls = models.PillarFeatureNetRadius if kind == "PFNRadiusTrainFunction" else models.PillarFeatureNet
    net = cls(4, (int(channels),), (vx, vy, 1.0), (xo - vx / 2, yo - vy / 2, 0.0, 0.0, 0.0, 0.0)).train()
    net.x_offset, net.y_offset = xo, yo
    net.pfn_layers[0].norm.eps, net.pfn_layers[0].norm.momentum = float(eps), float(momentum)
    return net


def pfn_factory(node):
    return lambda: pfn_module(node.kind, node.args[3].shape[0], node.args[8], node.args[9], node.args[10])


def audit_pfn(node, audit, packers):
    """The float64 formulation of tests/test_gpu_mhead_train.py: the layer's own torch formulation on the CPU in float64; per
    quantity max-abs error over max-abs value within the larger of the project tolerance and four times the error of a float32
    run of the same formulation.  Then every element against the float64 reference and bounds of tests/pfn_ref_helpers.py."""
    vfe = packers.get("pfn", pfn_factory)(node)                 # fresh module (train mode, torch formulation) for this node's geometry and channel count
    vox, num, coords, weight, gamma, beta, rm0, rv0 = node.args[:8]
    w = None if node.grad_out is None else node.grad_out[0]
    res = {}
    for dt in (torch.float64, torch.float32):
        net = vfe().to(dt)
        layer = net.pfn_layers[0]
        with torch.no_grad():
            layer.linear.weight.copy_(weight.cpu()); layer.norm.weight.copy_(gamma.cpu()); layer.norm.bias.copy_(beta.cpu())
            layer.norm.running_mean.copy_(rm0.cpu()); layer.norm.running_var.copy_(rv0.cpu())
        out = net(vox.cpu().to(dt), num.cpu(), coords.cpu())
        r = dict(out=out.detach(), running_mean=layer.norm.running_mean, running_var=layer.norm.running_var)
        if w is not None:
            (out * w.cpu().to(dt)).sum().backward()
            r.update(d_linear_weight=layer.linear.weight.grad, d_norm_weight=layer.norm.weight.grad, d_norm_bias=layer.norm.bias.grad)
        res[dt] = {k: v.detach().double() for k, v in r.items()}
    got = dict(out=node.outputs[0], running_mean=node.after["running_mean"], running_var=node.after["running_var"])
    if node.grad_in is not None:
        got.update(d_linear_weight=node.grad_in[3], d_norm_weight=node.grad_in[4], d_norm_bias=node.grad_in[5])
    rel = lambda x, ref: float((x - ref).abs().max() / max(float(ref.abs().max()), 1e-30))
    for k, v in got.items():
        ref = res[torch.float64][k]
        bound = max(PFN_TOL[k], 4 * rel(res[torch.float32][k], ref))
        audit.add(node, k, rel(v.detach().double().cpu(), ref) / bound)
    # and per element (tests/pfn_ref_helpers.py: float64 written from the reference's formulation, every element inside its own
    # derived bound; the node kept neither argmax nor statistics, so contested maxima widen the gradient bounds by their spread)
    import pfn_ref_helpers as P
    f32 = lambda t: t.detach().float().cpu().numpy()
    case = P.trim_slots(dict(vox=f32(vox), num=num.detach().cpu().numpy(), coords=coords.detach().cpu().numpy(), geom=tuple(float(g) for g in node.args[10]),
                             wt=np.ascontiguousarray(f32(weight).T), gamma=f32(gamma), beta=f32(beta), eps=float(node.args[8]),
                             momentum=float(node.args[9]), rm0=f32(rm0), rv0=f32(rv0), grad_out=None if w is None else f32(w)))
    per = P.check_train_undecided({k: v.detach().double().cpu() for k, v in got.items()}, case, node.kind == "PFNRadiusTrainFunction")
    for k, ratio in per.items():
        audit.add(node, k + " per element", ratio)


# ------------------------------------------------------------------------------------------------------------------ voxel means
def audit_voxel_means(call, audit, label="voxel means"):
    """A recorded ``voxelize`` call with 16-bit means: every mean within ONE rounding of the float64 mean of the voxel's points --
    the fp32 sum of at most T points and one division ((T + 1) roundings) under the 16-bit store."""
    res = call.result
    mean = res.get("mean")
    if mean is None or mean.dtype == torch.float32:
        return
    kind = kind_of(mean.dtype)
    n = int(res["voxel_offsets"][-1].item())
    vox, npv = a64(res["voxels"])[:n], res["num_points_per_voxel"].detach().cpu().numpy()[:n].astype(np.int64)
    t = vox.shape[1]
    live = (np.arange(t)[None, :] < npv[:, None])[..., None]
    c = mean.shape[1]
    ref = (vox[..., :c] * live).sum(1) / np.maximum(npv, 1)[:, None]
    mag = (np.abs(vox[..., :c]) * live).sum(1) / np.maximum(npv, 1)[:, None]
    u = U_STORE[kind]
    bound = u * np.abs(ref) + (1 + u) * gamma_n(t + 1) * mag + store_floor(kind)
    audit.add(label, "16-bit mean", worst(a64(mean)[:n], ref, bound))


AUDITS = {"IndiceConvFunction": audit_indice_conv, "BatchNormReluFunction": audit_bn, "Conv3x3Function": audit_dense_conv,
          "ConvTranspose1x1Function": audit_dense_conv, "Heads1x1Function": audit_dense_conv, "HeadsLossFunction": audit_heads_loss,
          "SecondLossFunction": audit_second_loss, "SparseToDenseFunction": audit_sparse_to_dense,
          "PillarScatterFunction": audit_pillar_scatter, "PFNTrainFunction": audit_pfn, "PFNRadiusTrainFunction": audit_pfn}


def audit_nodes(nodes, audit, packers, conv_numerics=True):
    """``conv_numerics=False``: the convolutions' fp64 references (most of the audit's time) are left out -- their wiring checks
    (weight images, tables, which tensors the kernels read) and every other node's full audit stay."""
    import time
    audit.numerics = bool(conv_numerics)
    for node in nodes:
        t0 = time.perf_counter()
        AUDITS[node.kind](node, audit, packers)
        audit.audited.add(node.index)
        audit.seconds[node.kind] = audit.seconds.get(node.kind, 0.0) + time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------------------------ wiring
def walk_graph(root):
    """Every autograd node reachable from ``root`` (a grad_fn): (list of nodes, {id(producer): [(consumer, input slot, output nr)]})."""
    seen, order, consumers = {}, [], {}
    stack = [root]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen[id(fn)] = fn
        order.append(fn)
        for slot, (nxt, nr) in enumerate(fn.next_functions):
            if nxt is not None:
                consumers.setdefault(id(nxt), []).append((fn, slot, nr))
                stack.append(nxt)
    return order, consumers


def audit_graph(loss, nodes, audit, function_names=PROJECT_FUNCTIONS, also_allowed=()):
    """Completeness and gradient flow.  Walk the graph from ``loss.grad_fn``: every node of a project function type was recorded and
    audited (counts equal), every other type is on NATIVE_ALLOWED.  Where the ONLY consumer of a recorded node's output is another
    recorded node, the gradient that arrived at the producer is bit for bit what the consumer produced for that input."""
    order, consumers = walk_graph(loss.grad_fn)
    by_fn = {id(n.grad_fn): n for n in nodes if n.grad_fn is not None}
    project = {name + "Backward" for name in function_names}
    in_graph = [fn for fn in order if type(fn).__name__ in project]
    missing = [type(fn).__name__ for fn in in_graph if id(fn) not in by_fn]
    audit.require("graph", "every project node of the graph was recorded", not missing, note=f"missing {missing}")
    rec_in_graph = [n for n in nodes if n.grad_fn is not None and id(n.grad_fn) in {id(f) for f in in_graph}]
    audit.require("graph", "counts: graph = recorded = audited",
                  len(in_graph) == len(rec_in_graph) == len([n for n in nodes if n.index in audit.audited and n.grad_fn is not None]),
                  note=f"graph {len(in_graph)} recorded {len(rec_in_graph)} audited {len(audit.audited)}")
    foreign = sorted({type(fn).__name__ for fn in order if type(fn).__name__ not in project and type(fn).__name__ not in NATIVE_ALLOWED
                      and type(fn).__name__ not in also_allowed})
    audit.require("graph", "every other node type is allow-listed", not foreign, note=f"not allow-listed: {foreign}")
    links = 0
    for n in nodes:
        if n.grad_fn is None or n.grad_out is None:
            continue
        cons = consumers.get(id(n.grad_fn), [])
        for nr in range(len(n.grad_out)):
            mine = [(c, slot) for c, slot, k in cons if k == nr]
            if len(mine) == 1 and id(mine[0][0]) in by_fn:
                m = by_fn[id(mine[0][0])]
                if m.grad_in is None:
                    continue
                slot = m.tensor_slots()[mine[0][1]]
                links += 1
                audit.require(n, f"arriving gradient = what node {m.index} ({m.kind}) produced for its input {slot}",
                              same_bits(n.grad_out[nr], m.grad_in[slot]))
    return dict(graph_nodes=len(order), project_nodes=len(in_graph), links=links)


def audit_bucket(tr, nodes, snap, audit, scale=1.0, stacked=()):
    """After backward + all-reduce, before the update (``snap`` taken there): every parameter's gradient equals its node's recorded
    weight gradient (for parameters stacked into one operand -- the heads -- the slice of the stacked gradient), every .grad is a
    view of the flat bucket, the slots of parameters no node used are zero, and the bucket holds nothing else (in particular nothing of
    an earlier step).  ``stacked``: [(node kind, argument index, [parameters in stacking order])]."""
    produced = {}
    where, off = {}, 0
    for p in tr.bucket.params:
        where[id(p)] = (off, p.numel())
        off += p.numel()
    # the master weight a node computed with is the parameter as the optimizer held it when this step's update began
    current = lambda p: snap["master"][where[id(p)][0]:where[id(p)][0] + where[id(p)][1]].view_as(p)
    for n in nodes:
        for i, ref in enumerate(n.arg_refs):
            if isinstance(ref, torch.nn.Parameter) and id(ref) in where:
                audit.require(n, f"argument {i} is the current master parameter", same_bits(n.args[i], current(ref)))
        for kind, arg, params in stacked:
            if n.kind == kind:
                rows = sum(p.shape[0] for p in params)
                audit.require(n, f"argument {arg} stacks the current master parameters, zeros behind them",
                              same_bits(n.args[arg][:rows], torch.cat([current(p) for p in params])) and bool((n.args[arg][rows:] == 0).all()))
        if n.grad_in is None:
            continue
        for i, ref in enumerate(n.arg_refs):
            if isinstance(ref, torch.nn.Parameter) and n.grad_in[i] is not None:
                produced.setdefault(id(ref), []).append((n, n.grad_in[i]))
        for kind, arg, params in stacked:
            if n.kind == kind and n.grad_in[arg] is not None:
                off = 0
                for p in params:
                    produced.setdefault(id(p), []).append((n, n.grad_in[arg][off:off + p.shape[0]]))
                    off += p.shape[0]
    off = 0
    for p, view in zip(tr.bucket.params, tr.bucket.views):
        slot = snap["flat"][off:off + p.numel()].view_as(p)
        off += p.numel()
        got = produced.get(id(p))
        name = snap["names"].get(id(p), "?")
        audit.require("bucket", f"{name}: .grad is a view of the flat bucket", snap["grad_ptr"].get(id(p)) == view.data_ptr())
        if got is None:
            if id(p) in snap["native"]:
                continue                  # a parameter of a torch-native layer: its gradient is torch's, not audited
            audit.require("bucket", f"{name}: unused parameter's slot is zero", bool((slot == 0).all()))
        elif len(got) == 1:
            audit.require(got[0][0], f"{name}: bucket slot = the node's weight gradient", same_bits(slot, got[0][1].reshape(p.shape).to(slot.dtype)),
                          note="(a stale or doubled gradient shows here)")
    return produced


def audit_adamw(tr, before, after, audit, label):
    """Master weights after the update within the AdamW tolerance (tests/test_gpu_train_edges.py: rtol 2e-6, atol 2e-7) of the float64
    formula on the recorded bucket, unscaled by the loss scale the step ran with."""
    f32 = lambda v: float(np.float32(v))
    g = tr.opt.param_groups[0]
    scale = float(before.get("scale", 1.0))
    p, m, v, _ = TR.adamw_ref(a64(before["master"]), a64(before["exp_avg"]), a64(before["exp_avg_sq"]), a64(before["flat"]) / scale,
                              int(before["step"]) + 1, f32(g["lr"]), f32(g["betas"][0]), f32(g["betas"][1]), f32(g["eps"]),
                              f32(g["weight_decay"]), f32(tr.opt.max_grad_norm))
    audit.add(label, "master weights = fp64 AdamW on the recorded gradients", worst(a64(after["master"]), p, 2e-6 * np.abs(p) + 2e-7))


def optimizer_state(tr):
    o = tr.opt
    scale = 1.0 if getattr(o, "loss_scale", None) is None else float(o.loss_scale[0].item())
    return dict(master=o.flat.detach().clone(), exp_avg=o.exp_avg.detach().clone(), exp_avg_sq=o.exp_avg_sq.detach().clone(),
                flat=tr.bucket.flat.detach().clone(), step=float(o.state[1].item()), scale=scale)


def audited_step(rec, tr, ins, native_params=()):
    """One ``tr.step(*ins)`` with the loss tensor kept (for the graph walk) and snapshots of bucket and optimizer taken between the
    all-reduce and the update, and after it.  -> dict(loss, before, after, out6)."""
    got = {}
    orig_fl, orig_up = tr.forward_loss, tr._step_update

    def forward_loss(*a, **k):
        out = orig_fl(*a, **k)
        got["loss"] = out[0]
        return out

    def step_update():
        got["before"] = optimizer_state(tr)
        got["before"]["grad_ptr"] = {id(p): (None if p.grad is None else p.grad.data_ptr()) for p in tr.bucket.params}
        got["before"]["names"] = {id(p): n for n, p in tr.det.named_parameters()}
        got["before"]["native"] = {id(p) for p in native_params}
        orig_up()
        got["after"] = optimizer_state(tr)
    tr.forward_loss, tr._step_update = forward_loss, step_update
    try:
        got["out6"] = tr.step(*ins)
    finally:
        del tr.forward_loss, tr._step_update
    return got


def audit_running_statistics(steps_nodes, bn_modules, audit):
    """BatchNorm running statistics over several steps follow the recurrence step by step: step k starts, bit for bit, from what
    step k - 1 left (each step's own update is held to BnRef's bound in audit_bn), the module ends on the last step's result and
    has counted every step."""
    per_module = {}
    for k, nodes in enumerate(steps_nodes):
        for n in nodes:
            if n.kind in ("BatchNormReluFunction", "PFNTrainFunction", "PFNRadiusTrainFunction"):
                buf = n.arg_refs[3 if n.kind == "BatchNormReluFunction" else 6]
                per_module.setdefault(id(buf), []).append(n)
    for name, bn in bn_modules:
        chain = per_module.get(id(bn.running_mean), [])
        if not chain:
            continue
        i0 = 3 if chain[0].kind == "BatchNormReluFunction" else 6
        audit.require(chain[0], f"{name}: one update per step", len(chain) == len(steps_nodes))
        for a, b in zip(chain[:-1], chain[1:]):
            audit.require(b, f"{name}: starts from the previous step's running statistics",
                          same_bits(b.args[i0], a.after["running_mean"]) and same_bits(b.args[i0 + 1], a.after["running_var"]))
        audit.require(chain[-1], f"{name}: the module holds the last step's running statistics",
                      same_bits(bn.running_mean, chain[-1].after["running_mean"]) and same_bits(bn.running_var, chain[-1].after["running_var"]))
        audit.require(chain[-1], f"{name}: num_batches_tracked = steps", int(bn.num_batches_tracked) == len(steps_nodes))
