"""The audit of tests/train_step_audit_helpers.py proved on the CPU: a tiny torch emulation of every node kind of the 16-bit training
step (same function names, same call structure, rounding where the kernels round) goes through the SAME recorder and the SAME checks as
the device step in tests/test_gpu_train_step_audit.py.  The clean emulation passes every check; each planted mistake -- the wiring
mistakes a suite of finite-gradient and cosine checks lets through -- is flagged, at the node it was planted in and nowhere else.

The emulation's rulebooks come from the CPU oracle (oracle.rulebook_subm / rulebook_conv_sorted); the audit rebuilds its tables from
coordinates and layer geometry (train_step_audit_helpers.geometry_table), so the two are independent here as they are on the device."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import indice_conv_bwd_helpers as SB
import train_ref_helpers as TR
import train_step_audit_helpers as A
from oracle import oracle as orc

GRID, BATCH = [3, 12, 10], 2              # input grid (z, y, x); the strided layer leaves depth 2, so the dense image has 2 x 8 channels
HEADS = (14, 2, 4)                        # box | cls | dir channels of two anchors per cell, one class, two direction bins
HEAD_PAD = 24
LOSS_CFG = dict(TR.LOSS_DEFAULTS, num_class=1, num_direction_bins=2)


# ------------------------------------------------------------------------------------------------ the emulated kernel layer
def make_ops(mutants=frozenset()):
    """A module object with the kernel-level entry points the recorder knows from second_amd.ops, in fp32 torch on the CPU."""
    E = types.ModuleType("emulated_ops")
    E.mutants = set(mutants)
    E.stale = {}
    E.set_op_hook = lambda hook: None

    def images(w16, subm):
        k = w16.reshape(-1, w16.shape[-2], w16.shape[-1])
        return k.transpose(1, 2).contiguous().reshape(-1), (k.flip(0) if subm else k).contiguous().reshape(-1) * 1

    def pack_weight_train(weight, dtype, subm, zero_grad=False):
        w16 = weight.detach().to(dtype)
        pk, pkt = images(w16, subm)
        return (w16, pk, pkt, torch.zeros_like(weight)) if zero_grad else (w16, pk, pkt)

    def indice_conv(features, weight, nbr_out, num_out, packed=None, num_out_dev=None):
        k = weight.reshape(-1, weight.shape[-2], weight.shape[-1]).float()
        f0 = torch.cat([features.float(), torch.zeros(1, features.shape[1])])
        idx = torch.where(nbr_out < 0, torch.full_like(nbr_out, features.shape[0]), nbr_out).long()
        out = torch.zeros(num_out, k.shape[2])
        for o in range(k.shape[0]):
            out += f0[idx[:num_out, o]] @ k[o]
        return out.to(features.dtype)

    def indice_conv_backward(features, weight, nbr_out, nbr_in, dout, need_dfeat=True, need_dweight=True, dweight_dtype=None,
                             packed_dgrad=None, dweight_out=None):
        k = weight.reshape(-1, weight.shape[-2], weight.shape[-1]).float()
        f, d = features.float(), dout.float()
        dfeat, dw = torch.zeros_like(f), torch.zeros_like(k)
        for o in range(k.shape[0]):
            rows = torch.nonzero(nbr_out[:, o] >= 0).flatten()
            src = nbr_out[rows, o].long()
            wk = k[o].t() if ("transposed weight in dgrad" in E.mutants and k.shape[1] == k.shape[2] and nbr_in is None) else k[o]
            dfeat.index_add_(0, src, d[rows] @ wk.t())
            dw[o] = f[src].t() @ d[rows]
        return (dfeat.to(features.dtype) if need_dfeat else None), (dw.reshape(weight.shape) if need_dweight else None)

    def sparse_to_dense(features, indices, batch_size, spatial_shape, channels_last_2d=False, num_dev=None):
        d, h, w = spatial_shape
        c, ix = features.shape[1], indices.long()
        dense = torch.zeros(batch_size, c, d, h, w, dtype=features.dtype)
        dense[ix[:, 0], :, ix[:, 1], ix[:, 2], ix[:, 3]] = features
        return dense.reshape(batch_size, c * d, h, w).contiguous(memory_format=torch.channels_last) if channels_last_2d else dense

    def dense_to_sparse(dense, indices, num_dev=None, depth=0):
        ix = indices.long()
        if dense.dim() == 4 and depth:
            b, cd, h, w = dense.shape
            z = torch.zeros_like(ix[:, 1]) if "dense_to_sparse reads depth slice 0" in E.mutants else ix[:, 1]
            return dense.reshape(b, cd // depth, depth, h, w)[ix[:, 0], :, z, ix[:, 2], ix[:, 3]].contiguous()
        return dense[ix[:, 0], :, ix[:, 2], ix[:, 3]].contiguous()

    def pillar_scatter(features, coords, batch_size, ny, nx, channels_last=False, num_dev=None):
        ix = coords.long()
        out = torch.zeros(batch_size, features.shape[1], ny, nx, dtype=features.dtype)
        out[ix[:, 0], :, ix[:, 2], ix[:, 3]] = features
        return out.contiguous(memory_format=torch.channels_last) if channels_last else out

    def _rows(t):
        return t if t.dim() == 2 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])

    def _like(rows, t):
        if t.dim() == 2:
            return rows.to(t.dtype)
        b, c, h, w = t.shape
        return rows.to(t.dtype).reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)

    def bn_relu_forward(y, gamma, beta, eps, momentum, running_mean=None, running_var=None, relu=True, rows_dev=None):
        r = _rows(y).double()
        n = r.shape[0]
        mean, var = r.mean(0), r.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
        mean32, invstd32 = mean.float(), invstd.float()
        z = ((r.float() - mean32) * invstd32) * gamma + beta
        if relu:
            z = z.clamp_min(0)
        m = np.float32(momentum)
        unb = var if "biased variance in the running update" in E.mutants or n < 2 else var * n / (n - 1)
        running_mean.copy_((1 - m) * running_mean + m * mean32)
        running_var.copy_((1 - m) * running_var + m * unb.float())
        return _like(z, y), mean32, invstd32

    def bn_relu_backward(dz, y, gamma, beta, save_mean, save_invstd, relu=True, rows_dev=None):
        r, g = _rows(y).float(), _rows(dz).float()
        n = r.shape[0]
        xh = (r - save_mean) * save_invstd
        if relu and "ReLU mask dropped" not in E.mutants:
            g = g * ((xh * gamma + beta) > 0)
        dbeta = g.double().sum(0).float()
        dgamma = (g.double().sum(0) if "dgamma without xhat" in E.mutants else (g * xh).double().sum(0)).float()
        inv = np.float32(1.0 / n)
        dy = (gamma * save_invstd) * (g - dbeta * inv - xh * dgamma * inv)
        return _like(dy, y), dgamma, dbeta

    def conv2d_pack_weight_train(weight, dtype):
        w16 = weight.detach().to(dtype)
        return w16.reshape(-1).clone(), w16.flip(2, 3).transpose(0, 1).contiguous().reshape(-1)

    def conv2d_nhwc(x, packed, bias, cout, ksize, stride=1, pad=0, relu=False, sparse_input=False):
        w = packed.reshape(cout, x.shape[1], ksize, ksize).float()
        y = F.conv2d(x.float(), w, None if bias is None else bias.float(), stride, pad)
        return y.to(x.dtype).contiguous(memory_format=torch.channels_last)

    def conv2d_wgrad(x, dy, ksize=3):
        return torch.nn.grad.conv2d_weight(x.float(), (dy.shape[1], x.shape[1], ksize, ksize), dy.float(), padding=ksize // 2)

    for fn in (pack_weight_train, indice_conv, indice_conv_backward, sparse_to_dense, dense_to_sparse, pillar_scatter, bn_relu_forward,
               bn_relu_backward, conv2d_pack_weight_train, conv2d_nhwc, conv2d_wgrad):
        setattr(E, fn.__name__, fn)
    return E


# ------------------------------------------------------------------------------------------------ the emulated autograd functions
def make_functions(E):
    """The project's autograd functions, by name, over the emulated kernel layer ``E`` (looked up at call time: the recorder wraps
    its attributes)."""
    M = E.mutants

    class IndiceConvFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, features, weight, rulebook, packed):
            subm = rulebook.nbr_in is None
            key = id(weight)
            if "weight image from before the AdamW step" in M and subm and weight.shape[-2] == weight.shape[-1] and key in E.stale:
                w16, pk, pkt, dw0 = E.stale[key]                                   # the cache that forgot to look at the weights
                E.pack_weight_train(weight.detach(), features.dtype, subm, zero_grad=True)
            else:
                w16, pk, pkt, dw0 = E.pack_weight_train(weight.detach(), features.dtype, subm, zero_grad=True)
                E.stale[key] = (w16, pk, pkt, dw0)
            ctx.rb, ctx.pkt = rulebook, pkt
            ctx.save_for_backward(features, w16)
            return E.indice_conv(features, w16, rulebook.nbr_out, rulebook.num_out, packed=pk, num_out_dev=rulebook.num_out_dev)

        @staticmethod
        def backward(ctx, grad_out):
            features, w16 = ctx.saved_tensors
            rb = ctx.rb
            nbr_in = rb.nbr_out if ("nbr_out where nbr_in belongs" in M and rb.nbr_in is not None) else rb.nbr_in
            dfeat, dw = E.indice_conv_backward(features, w16, rb.nbr_out, nbr_in, grad_out.contiguous(), ctx.needs_input_grad[0], True,
                                               dweight_dtype=torch.float32, packed_dgrad=ctx.pkt)
            return dfeat, dw, None, None

    class BatchNormReluFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y, gamma, beta, running_mean, running_var, eps, momentum, relu, rows_dev=None):
            if "momentum 0.1 for 0.01" in M and y.dim() == 4:
                momentum = 0.1
            z, mean, invstd = E.bn_relu_forward(y, gamma.detach(), beta.detach(), eps, momentum, running_mean, running_var, relu, rows_dev=rows_dev)
            ctx.save_for_backward(y, gamma, beta, mean, invstd)
            ctx.relu = relu
            return z

        @staticmethod
        def backward(ctx, dz):
            y, gamma, beta, mean, invstd = ctx.saved_tensors
            dy, dgamma, dbeta = E.bn_relu_backward(dz, y, gamma.detach(), beta.detach(), mean, invstd, ctx.relu, rows_dev=None)
            return dy, dgamma, dbeta, None, None, None, None, None, None

    class SparseToDenseFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, features, indices, batch_size, spatial_shape, num_dev=None, channels_last_2d=False):
            ctx.save_for_backward(indices)
            ctx.depth = int(spatial_shape[0]) if channels_last_2d else 0
            return E.sparse_to_dense(features, indices, batch_size, spatial_shape, channels_last_2d=channels_last_2d, num_dev=num_dev)

        @staticmethod
        def backward(ctx, grad):
            return E.dense_to_sparse(grad, ctx.saved_tensors[0], num_dev=None, depth=ctx.depth), None, None, None, None, None

    class PillarScatterFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, features, coords, batch_size, ny, nx, channels_last=False):
            ctx.save_for_backward(coords)
            return E.pillar_scatter(features, coords, batch_size, ny, nx, channels_last=channels_last)

        @staticmethod
        def backward(ctx, grad):
            return E.dense_to_sparse(grad, ctx.saved_tensors[0]), None, None, None, None, None

    def dense_conv(ctx, x, weight, bias, k, i_f, i_b):
        img = E.conv2d_pack_weight_train(weight.detach().contiguous(), x.dtype)
        cout = weight.shape[1] if i_f else weight.shape[0]
        y = E.conv2d_nhwc(x, img[i_f], None if bias is None else bias.detach().float(), cout, k, 1, k // 2, relu=False)
        ctx.k, ctx.img_b, ctx.cin = k, img[i_b], x.shape[1]
        return y

    def dense_conv_backward(ctx, x, dy, transposed=False):
        dy = dy.contiguous(memory_format=torch.channels_last)
        if "dy of another layer" in M and ctx.k == 3:
            dy = E.kept_dy
        elif ctx.k == 1 and not hasattr(ctx, "is_heads"):
            E.kept_dy = dy                                        # the deblock's arriving gradient: what the mistake hands to the 3x3 layer
        dx = E.conv2d_nhwc(dy, ctx.img_b, None, ctx.cin, ctx.k, 1, ctx.k // 2, relu=False)
        dw = E.conv2d_wgrad(x, dy, ctx.k)
        return dx, (dw.transpose(0, 1).contiguous() if transposed else dw), dy

    class Conv3x3Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight):
            ctx.save_for_backward(x)
            return dense_conv(ctx, x, weight, None, 3, 0, 1)

        @staticmethod
        def backward(ctx, dy):
            return dense_conv_backward(ctx, ctx.saved_tensors[0], dy)[:2]

    class ConvTranspose1x1Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight):
            ctx.save_for_backward(x)
            return dense_conv(ctx, x, weight, None, 1, 1, 0)

        @staticmethod
        def backward(ctx, dy):
            return dense_conv_backward(ctx, ctx.saved_tensors[0], dy, transposed=True)[:2]

    class Heads1x1Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight, bias):
            ctx.save_for_backward(x)
            ctx.is_heads = True
            return dense_conv(ctx, x, weight, bias, 1, 0, 1)

        @staticmethod
        def backward(ctx, dy):
            dx, dw, dy = dense_conv_backward(ctx, ctx.saved_tensors[0], dy)
            return dx, dw, dy.float().sum(dim=(0, 2, 3))

    def loss32(y, labels, reg, anchors, imp, a, nc, bins, cfg):
        b, hc, h, w = y.shape
        rows = y.detach().float().permute(0, 2, 3, 1).reshape(b, h * w, hc).double().numpy()
        (box, cls, dirp), tot = A._split_heads(rows, a, nc, bins)
        lcfg = {k: v for k, v in cfg.items() if k in TR.LOSS_KEYS}
        with torch.enable_grad():                        # (grad mode is off inside Function.forward)
            out6, d_cls, d_box, d_dir = TR.loss_ref(cls, box, dirp, labels.numpy(), reg.numpy(), anchors.numpy(), imp.numpy(), num_class=nc,
                                                    num_direction_bins=bins, dtype=torch.float32, **lcfg)
        return torch.from_numpy(out6).float(), d_cls, d_box, d_dir

    class HeadsLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight, bias, labels, reg_targets, anchors, importance, anchors_per_loc, num_class, num_dir_bins, cfg, want_terms=False):
            ctx.is_heads = True
            y = dense_conv(ctx, x, weight, bias, 1, 0, 1)
            out6, d_cls, d_box, d_dir = loss32(y, labels, reg_targets, anchors, importance, anchors_per_loc, num_class, num_dir_bins, cfg)
            b, hc, h, w = y.shape
            d = A._stack_heads([d_box, d_cls, d_dir], b, h * w, anchors_per_loc, hc)
            ctx.d_heads = torch.from_numpy(d).float().reshape(b, h, w, hc).permute(0, 3, 1, 2)
            ctx.save_for_backward(x)
            ctx.dtype = y.dtype
            ctx.mark_non_differentiable(out6)
            return out6[0].clone(), out6

        @staticmethod
        def backward(ctx, g_loss, _g_all):
            dy = (ctx.d_heads * g_loss.float()).to(ctx.dtype).contiguous(memory_format=torch.channels_last)
            dx, dw, dy = dense_conv_backward(ctx, ctx.saved_tensors[0], dy)
            return dx, dw, dy.float().sum(dim=(0, 2, 3)), None, None, None, None, None, None, None, None, None

    class SecondLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, cls_preds, box_preds, dir_preds, labels, reg_targets, anchors, importance, cfg):
            b = cls_preds.shape[0]
            f = lambda t, k: t.detach().reshape(b, -1, k).double().numpy()
            lcfg = {k: v for k, v in cfg.items() if k in TR.LOSS_KEYS}
            with torch.enable_grad():
                out6, d_cls, d_box, d_dir = TR.loss_ref(f(cls_preds, 1), f(box_preds, 7), f(dir_preds, 2), labels.numpy(), reg_targets.numpy(),
                                                        anchors.numpy(), importance.numpy(), num_class=1, num_direction_bins=2,
                                                        dtype=torch.float32, **lcfg)
            ctx.grads = [torch.from_numpy(g).float().reshape(t.shape) for g, t in ((d_cls, cls_preds), (d_box, box_preds), (d_dir, dir_preds))]
            ctx.dts = (cls_preds.dtype, box_preds.dtype, dir_preds.dtype)
            out6 = torch.from_numpy(out6).float()
            ctx.mark_non_differentiable(out6)
            return out6[0].clone(), out6

        @staticmethod
        def backward(ctx, g_loss, _g_all):
            return tuple((g * g_loss).to(dt) for g, dt in zip(ctx.grads, ctx.dts)) + (None,) * 5

    class PFNRadiusTrainFunction(torch.autograd.Function):
        """The layer's own torch formulation in float32, run under autograd inside forward."""

        @staticmethod
        def forward(ctx, voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, eps, momentum, geom):
            net = A.pfn_module("PFNRadiusTrainFunction", weight.shape[0], eps, momentum, geom).float()
            layer = net.pfn_layers[0]
            with torch.no_grad():
                layer.linear.weight.copy_(weight); layer.norm.weight.copy_(gamma); layer.norm.bias.copy_(beta)
                layer.norm.running_mean.copy_(running_mean); layer.norm.running_var.copy_(running_var)
            with torch.enable_grad():
                ctx.out = net(voxels, num_points, coords)
            ctx.layer = layer
            running_mean.copy_(layer.norm.running_mean); running_var.copy_(layer.norm.running_var)
            return ctx.out.detach().clone()

        @staticmethod
        def backward(ctx, grad_out):
            l = ctx.layer
            dw, dg, db = torch.autograd.grad(ctx.out, [l.linear.weight, l.norm.weight, l.norm.bias], grad_out)
            return None, None, None, dw, dg, db, None, None, None, None, None

    return types.SimpleNamespace(IndiceConvFunction=IndiceConvFunction, BatchNormReluFunction=BatchNormReluFunction,
                                 SparseToDenseFunction=SparseToDenseFunction, PillarScatterFunction=PillarScatterFunction,
                                 Conv3x3Function=Conv3x3Function, ConvTranspose1x1Function=ConvTranspose1x1Function,
                                 Heads1x1Function=Heads1x1Function, HeadsLossFunction=HeadsLossFunction, SecondLossFunction=SecondLossFunction,
                                 PFNRadiusTrainFunction=PFNRadiusTrainFunction)


def packers_for(E):
    """The expected images: the emulation's own packers, unwrapped, on the master weight the node recorded."""
    return dict(sparse=lambda w, dt, subm: E._pack0(w, dt, subm), dense=lambda w, dt: E._pack2d0(w, dt))


# ------------------------------------------------------------------------------------------------ the emulated network and trainer
class SparseTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, list(spatial_shape), batch_size
        self.num_active_dev, self.rulebooks = None, {}


class Rulebook:
    def __init__(self, nbr_out, nbr_in, num_out, subm):
        self.nbr_out, self.nbr_in, self.num_out, self.num_out_dev, self.subm = nbr_out, nbr_in, num_out, None, subm


class SparseConv(nn.Module):
    def __init__(self, fns, cin, cout, subm, key=None):
        super().__init__()
        self.fns, self.subm, self.key = fns, subm, key
        self.kernel_size, self.stride, self.padding = [3, 3, 3], ([1, 1, 1] if subm else [2, 2, 2]), [1, 1, 1]
        self.weight = nn.Parameter(torch.randn(3, 3, 3, cin, cout) / np.sqrt(27 * cin))

    def forward(self, x):
        idx = x.indices.numpy()
        if self.subm:
            rb = x.rulebooks.get(self.key)
            if rb is None:
                _, pairs, num = orc.rulebook_subm(idx, x.batch_size, x.spatial_shape, 3)
                nbr_out, _ = SB.tables_from_pairs(pairs, num, len(idx), len(idx))
                rb = x.rulebooks[self.key] = Rulebook(torch.from_numpy(nbr_out), None, len(idx), True)
            out_idx, out_shape = x.indices, x.spatial_shape
        else:
            out_np, pairs, num, out_shape = orc.rulebook_conv_sorted(idx, x.batch_size, x.spatial_shape, 3, 2, 1)
            nbr_out, nbr_in = SB.tables_from_pairs(pairs, num, len(idx), len(out_np))
            rb = Rulebook(torch.from_numpy(nbr_out), torch.from_numpy(nbr_in), len(out_np), False)
            out_idx = torch.from_numpy(out_np)
        feats = self.fns.IndiceConvFunction.apply(x.features, self.weight, rb, None)
        out = SparseTensor(feats, out_idx, [int(s) for s in out_shape], x.batch_size)
        out.rulebooks = x.rulebooks
        return out


def _bn(cls, c, seed):
    m = cls(c, eps=1e-3, momentum=0.01)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.weight.copy_(torch.rand(c, generator=g) + 0.5)
        m.bias.copy_(torch.randn(c, generator=g) / 4)
        m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
        m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return m


class Net(nn.Module):
    """SubM 4 -> 16, SubM 16 -> 16, stride-2 16 -> 8 (each + BatchNorm1d + ReLU), dense [B, 8 x 2, 6, 5], 3x3 conv + BatchNorm2d + ReLU,
    1x1 transposed conv + BatchNorm2d + ReLU, stacked heads + loss; ``spare`` is a parameter nothing uses."""

    def __init__(self, fns):
        super().__init__()
        torch.manual_seed(3)
        self.fns = fns
        self.convs = nn.ModuleList([SparseConv(fns, 4, 16, True, "s0"), SparseConv(fns, 16, 16, True, "s0"), SparseConv(fns, 16, 8, False)])
        self.norms = nn.ModuleList([_bn(nn.BatchNorm1d, 16, 1), _bn(nn.BatchNorm1d, 16, 2), _bn(nn.BatchNorm1d, 8, 3)])
        self.conv = nn.Conv2d(16, 16, 3, padding=1, bias=False)
        self.bn_a = _bn(nn.BatchNorm2d, 16, 4)
        self.deconv = nn.ConvTranspose2d(16, 16, 1, bias=False)
        self.bn_b = _bn(nn.BatchNorm2d, 16, 5)
        self.conv_box, self.conv_cls, self.conv_dir_cls = nn.Conv2d(16, 14, 1), nn.Conv2d(16, 2, 1), nn.Conv2d(16, 4, 1)
        self.spare = nn.Parameter(torch.ones(5))

    def bn(self, m, x, rows_dev=None):
        z = self.fns.BatchNormReluFunction.apply(x, m.weight, m.bias, m.running_mean, m.running_var, m.eps, m.momentum, True, rows_dev)
        m.num_batches_tracked += 1
        return z

    def forward(self, batch, dtype, fused_loss=True):
        x = SparseTensor(batch["rows"].to(dtype), batch["indices"], GRID, BATCH)
        for conv, norm in zip(self.convs, self.norms):
            x = conv(x)
            x.features = self.bn(norm, x.features)
        img = self.fns.SparseToDenseFunction.apply(x.features, x.indices, BATCH, x.spatial_shape, None, True)
        y = self.bn(self.bn_a, self.fns.Conv3x3Function.apply(img, self.conv.weight))
        y = self.bn(self.bn_b, self.fns.ConvTranspose1x1Function.apply(y, self.deconv.weight))
        heads = (self.conv_box, self.conv_cls, self.conv_dir_cls)
        pad = HEAD_PAD - sum(HEADS)
        wcat = torch.cat([c.weight for c in heads] + [torch.zeros(pad, 16, 1, 1)], 0)
        bcat = torch.cat([c.bias for c in heads] + [torch.zeros(pad)], 0)
        t = batch["targets"]
        if fused_loss:
            return self.fns.HeadsLossFunction.apply(y, wcat, bcat, t["labels"], t["reg"], t["anchors"], t["importance"], 2, 1, 2, LOSS_CFG, False)
        o = self.fns.Heads1x1Function.apply(y, wcat, bcat)
        b, _, h, w = o.shape
        part = lambda c0, code: o[:, c0:c0 + 2 * code].reshape(b, 2, code, h, w).permute(0, 1, 3, 4, 2).contiguous()
        return self.fns.SecondLossFunction.apply(part(14, 1), part(0, 7), part(16, 2), t["labels"], t["reg"], t["anchors"], t["importance"], LOSS_CFG)


class AdamW:
    """FlatAdamW's surface and formulas (csrc/train.hip: k_flat_sumsq, k_flat_adamw) in fp32 torch."""

    def __init__(self, params, grad_flat, lr=3e-3, weight_decay=0.01, loss_scale=None, mutants=frozenset()):
        self.params = list(params)
        self.flat = torch.cat([p.detach().reshape(-1) for p in self.params]).clone()
        off = 0
        for p in self.params:
            p.data = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.grad, self.exp_avg, self.exp_avg_sq = grad_flat, torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.state = torch.zeros(4)
        self.loss_scale = None if loss_scale is None else torch.tensor([float(loss_scale), 0.0, 200.0, 0.0])
        self.param_groups = [dict(lr=lr, betas=(0.9, 0.99), eps=1e-8, weight_decay=weight_decay)]
        self.max_grad_norm, self.mutants = 10.0, mutants

    def step(self):
        g = self.param_groups[0]
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        lr, b1, b2, eps, wd = f32(g["lr"]), f32(g["betas"][0]), f32(g["betas"][1]), f32(g["eps"]), f32(g["weight_decay"])
        scale = 1.0 if self.loss_scale is None else float(self.loss_scale[0])
        norm = (self.grad.double().pow(2).sum().sqrt() / scale).float()
        self.state[0], self.state[1], self.state[3] = norm, self.state[1] + 1, scale
        unscale = 1.0 if "loss scale left on" in self.mutants else np.float32(1.0 / scale)
        clip = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        t = float(self.state[1])
        gi = self.grad * unscale * clip
        self.flat.mul_(1 - lr * wd)
        self.exp_avg.add_((gi - self.exp_avg) * (1 - b1))
        self.exp_avg_sq.mul_(b2).add_(gi * gi * (1 - b2))
        step_size, rs2 = lr / (1 - b1 ** t), torch.sqrt(1 - b2 ** t)
        self.flat.sub_(step_size * (self.exp_avg / (self.exp_avg_sq.sqrt() / rs2 + eps)))


class Trainer:
    """training.DeviceTrainer's surface as the audit uses it: det, bucket, opt, forward_loss, step, _step_update."""

    def __init__(self, det, dtype, loss_scale=None, mutants=frozenset(), fused_loss=True):
        from second_amd.distributed import GradBucket
        self.det, self.dtype, self.fused_loss, self.mutants = det, dtype, fused_loss, mutants
        self.bucket = GradBucket(det)
        self.opt = AdamW(self.bucket.params, self.bucket.flat, loss_scale=loss_scale, mutants=mutants)

    def forward_loss(self, batch):
        loss, out6 = self.det(batch, self.dtype, self.fused_loss)
        return loss, out6, batch["targets"]["labels"]

    def step(self, batch):
        loss, out6, _ = self.forward_loss(batch)
        (loss if self.opt.loss_scale is None else loss * self.opt.loss_scale[0]).backward()
        self.bucket.allreduce(average=True)
        self._step_update()
        return out6

    def _step_update(self):
        self.opt.step()
        if "bucket not zeroed between steps" not in self.mutants:
            self.bucket.zero_grad()


def make_batch(seed, dtype):
    rng = np.random.default_rng(seed)
    cells = []
    for b in range(BATCH):
        lin = np.sort(rng.choice(int(np.prod(GRID)), 150 + 7 * b, replace=False))
        z, rem = np.divmod(lin, GRID[1] * GRID[2])
        y, x = np.divmod(rem, GRID[2])
        cells.append(np.stack([np.full_like(z, b), z, y, x], 1))
    idx = np.concatenate(cells).astype(np.int32)
    rows = torch.from_numpy(rng.standard_normal((len(idx), 4)).astype(np.float32))
    out_hw = 6 * 5
    c = TR.loss_case(seed + 11, BATCH, 2 * out_hw, 1, 2, empty_frame=None)
    targets = dict(labels=torch.from_numpy(c["labels"]), reg=torch.from_numpy(c["reg"]), anchors=torch.from_numpy(c["anchors"]),
                   importance=torch.from_numpy(c["importance"]))
    return dict(rows=rows, indices=torch.from_numpy(idx), targets=targets)


# ------------------------------------------------------------------------------------------------ running the audit on the emulation
def run(monkeypatch, mutants=(), dtype=torch.bfloat16, loss_scale=None, fused_loss=True, steps=2, drop_node=None):
    """``steps`` audited optimisation steps of the emulation on different batches -> (audit, recorder, per-step results)."""
    mutants = frozenset(mutants)
    E = make_ops(mutants)
    E._pack0, E._pack2d0 = E.pack_weight_train, E.conv2d_pack_weight_train          # the unwrapped packers, for the expected images
    fns = make_functions(E)
    det = Net(fns)
    tr = Trainer(det, dtype, loss_scale, mutants, fused_loss)
    audit = A.Audit()
    heads = [det.conv_box, det.conv_cls, det.conv_dir_cls]
    stacked = [(k, arg, [getattr(m, name) for m in heads]) for k in ("HeadsLossFunction", "Heads1x1Function")
               for arg, name in ((1, "weight"), (2, "bias"))]
    classes = [getattr(fns, n) for n in A.PROJECT_FUNCTIONS if hasattr(fns, n)]
    per_step = []
    with A.Recorder(monkeypatch, classes, E, SparseConv) as rec:
        for k in range(steps):
            rec.step = k
            per_step.append(A.audited_step(rec, tr, (make_batch(100 + k, dtype),)))
    for k, got in enumerate(per_step):
        nodes = rec.nodes_of(k)
        if drop_node is not None:
            nodes = [n for n in nodes if n.kind != drop_node or n.index != min(m.index for m in nodes if m.kind == drop_node)]
        A.audit_nodes(nodes, audit, packers_for(E))
        got["graph"] = A.audit_graph(got["loss"], nodes, audit)
        A.audit_bucket(tr, nodes, got["before"], audit, stacked=stacked)
        A.audit_adamw(tr, got["before"], got["after"], audit, f"AdamW step {k + 1}")
    bns = [(n, m) for n, m in det.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    A.audit_running_statistics([rec.nodes_of(k) for k in range(steps)], bns, audit)
    return audit, rec, per_step


def planted(rec, kind, nth=0, step=None):
    return [n.index for n in rec.nodes if n.kind == kind and (step is None or n.step == step)][nth]


@pytest.mark.parametrize("dtype,loss_scale", [(torch.bfloat16, None), (torch.float16, 2.0 ** 12)])
@pytest.mark.parametrize("fused_loss", [True, False])
def test_the_clean_emulation_passes_every_check(monkeypatch, dtype, loss_scale, fused_loss):
    audit, rec, steps = run(monkeypatch, dtype=dtype, loss_scale=loss_scale, fused_loss=fused_loss)
    print(audit.report(f"emulation {dtype} fused_loss={fused_loss}"))
    assert not audit.failures(), audit.describe_failures()
    kinds = {n.kind for n in rec.nodes}
    want = {"IndiceConvFunction", "BatchNormReluFunction", "SparseToDenseFunction", "Conv3x3Function", "ConvTranspose1x1Function"}
    assert kinds == want | ({"HeadsLossFunction"} if fused_loss else {"Heads1x1Function", "SecondLossFunction"})
    # the exempt share is a condition on the inputs: the fp64 reference alone leaves at most 1 % of a node's elements ambiguous
    assert max(r["exempt"] for r in audit.rows) <= A.EXEMPT_CAP
    assert all(s["graph"]["project_nodes"] == len(rec.nodes_of(k)) for k, s in enumerate(steps))
    assert steps[0]["graph"]["links"] >= len(rec.nodes_of(0)) - 2          # the chain is linked node to node
    if loss_scale:
        loss_node = [n for n in rec.nodes if n.kind in ("HeadsLossFunction", "SecondLossFunction")][0]
        assert float(loss_node.grad_out[0]) == loss_scale                  # every gradient below it carries exactly the scale


def test_the_recorder_on_cpu_tensors(monkeypatch):
    """Hooks fire (every node has its arriving and produced gradients and its kernel-level calls), counts match the graph walk, the
    wrapped attributes are restored and the op hook is reset on exit."""
    E = make_ops()
    hooks = []
    E.set_op_hook = hooks.append
    fns = make_functions(E)
    before = (fns.IndiceConvFunction.apply, E.indice_conv, SparseConv.forward)
    det = Net(fns)
    with A.Recorder(monkeypatch, [getattr(fns, n) for n in A.PROJECT_FUNCTIONS if hasattr(fns, n)], E, SparseConv) as rec:
        assert callable(hooks[-1]) and E.indice_conv is not before[1]
        loss, _ = det(make_batch(1, torch.bfloat16), torch.bfloat16)
        loss.backward()
    assert hooks[-1] is None and E.indice_conv is before[1] and SparseConv.forward is before[2]
    assert fns.IndiceConvFunction.apply == before[0]
    assert len(rec.nodes) == 3 + 5 + 1 + 1 + 1 + 1
    order, _ = A.walk_graph(loss.grad_fn)
    assert sum(type(f).__name__.endswith("FunctionBackward") for f in order) == len(rec.nodes)
    for n in rec.nodes:
        assert n.grad_out is not None and n.grad_in is not None and len(n.grad_in) == len(n.args), n
        assert n.calls and {c.phase for c in n.calls} == {"fwd", "bwd"}, n
    assert rec.nodes[0].grad_in[0] is None and rec.nodes[0].grad_in[1] is not None          # the voxel rows are data
    assert [n.layer is not None for n in rec.nodes if n.kind == "IndiceConvFunction"] == [True] * 3
    # and a forward without the recorder records nothing more
    det(make_batch(2, torch.bfloat16), torch.bfloat16)
    assert len(rec.nodes) == 12


def test_geometry_table_equals_the_oracle_rulebooks():
    """The audit's own gather table (coordinates + kernel / stride / padding) against the CPU oracle's rulebooks: SubM, 3x3x3 stride 2
    padding 1 and (3, 1, 1) stride (2, 1, 1) without padding, on the ragged geometry of the backward tests."""
    geom = SB.geom_runs()
    idx, shape, batch = geom
    for mode, (ks, st, pd) in (("subm", ([3, 3, 3], [1, 1, 1], [1, 1, 1])), ("s2", ([3, 3, 3], [2, 2, 2], [1, 1, 1])),
                               ("k3", ([3, 1, 1], [2, 1, 1], [0, 0, 0]))):
        tb = SB.tables(geom, mode)
        out_idx = idx if mode == "subm" else orc.rulebook_conv_sorted(idx, batch, shape, ks, st, pd)[0]
        assert np.array_equal(A.geometry_table(idx, out_idx, shape, ks, st, pd), tb["nbr_out"]), mode


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_voxel_means_within_one_rounding_and_a_mean_over_all_slots_is_flagged(dtype):
    """audit_voxel_means on a voxeliser result made by hand: ragged voxels of up to five points, the fp32 mean stored in 16 bits."""
    g = torch.Generator().manual_seed(4)
    n, t = 300, 5
    npv = torch.randint(1, t + 1, (n,), generator=g).int()
    vox = torch.randn(n + 20, t, 4, generator=g) * 10 * (torch.arange(t).view(1, -1, 1) < torch.cat([npv, torch.zeros(20).int()]).view(-1, 1, 1))
    mean = vox[:n].sum(1) / npv.view(-1, 1)
    res = dict(voxels=vox, num_points_per_voxel=torch.cat([npv, torch.zeros(20).int()]), voxel_offsets=torch.tensor([0, 140, n]).int())
    for name, m, ok in (("per live point", mean, True), ("over all slots", vox[:n].sum(1) / t, False)):
        audit = A.Audit()
        res["mean"] = torch.cat([m.to(dtype), torch.full((20, 4), float("nan"), dtype=dtype)])        # capacity rows behind the live ones
        A.audit_voxel_means(A.Call("voxelize", "free", 0, (), {}, res), audit)
        assert len(audit.rows) == 1 and (not audit.failures()) == ok, (name, audit.rows)


def test_loss_reference_at_a_logit_of_exactly_zero():
    """The one place where the audit does not hand the recorded tensor to train_ref_helpers.loss_ref as it is (see
    train_step_audit_helpers.loss_reference): at x = 0 the reference's formula returns autograd's 1 - t, the smooth function's
    derivative is 1/2 - t; every other value is untouched."""
    c = TR.loss_case(3, 2, 64, 1, 2, empty_frame=None)
    cls = c["cls"].astype(np.float64)
    zeros = [(0, 5), (1, 9), (1, 63)]                       # a negative, a negative, the positive the case puts last
    for i, n in zeros:
        cls[i, n, 0] = 0.0
    assert c["labels"][0, 5] == 0 and c["labels"][1, 63] > 0
    args = (c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"])
    raw = TR.loss_ref(cls, *args)
    fixed = A.loss_reference(cls, *args)
    near = TR.loss_ref(np.where(cls == 0, 1e-9, cls), *args)           # the smooth function a nanounit away
    np.testing.assert_allclose(fixed[0], raw[0], rtol=1e-15)
    mask = np.zeros(cls.shape, bool)
    for i, n in zeros:
        mask[i, n, 0] = True
    assert np.array_equal(fixed[1][~mask], raw[1][~mask]) and np.array_equal(fixed[2], raw[2]) and np.array_equal(fixed[3], raw[3])
    np.testing.assert_allclose(fixed[1][mask], near[1][mask], rtol=1e-8)
    assert np.all(np.abs(raw[1][mask] - fixed[1][mask]) > 0.2 * np.abs(fixed[1][mask]))        # the formula's kink is a 40 % matter
    # analytic value at a negative with logit 0, focal gamma 2, alpha 1/4: (1 - alpha) (2 p (1 - p) p softplus(0) + p^2 p), p = 1/2
    w = fixed[1][0, 5, 0] / (0.75 * (2 * 0.5 * 0.25 * np.log(2.0) + 0.125))
    assert w > 0 and abs(raw[1][0, 5, 0] / w - 0.75 * (2 * 0.5 * 0.25 * np.log(2.0) + 0.25)) < 1e-12


# ---- the planted mistakes: (mutant, node kind it is planted in, which of them, step) -----------------------------------------------
NODE_MUTANTS = [
    ("weight image from before the AdamW step", "IndiceConvFunction", 1, 1),
    ("transposed weight in dgrad", "IndiceConvFunction", 1, None),
    ("nbr_out where nbr_in belongs", "IndiceConvFunction", 2, None),
    ("dy of another layer", "Conv3x3Function", 0, None),
    ("ReLU mask dropped", "BatchNormReluFunction", None, None),
    ("biased variance in the running update", "BatchNormReluFunction", None, None),
    ("momentum 0.1 for 0.01", "BatchNormReluFunction", (3, 4), None),
    ("dgamma without xhat", "BatchNormReluFunction", None, None),
    ("dense_to_sparse reads depth slice 0", "SparseToDenseFunction", 0, None),
]


@pytest.mark.parametrize("mutant,kind,which,step", NODE_MUTANTS, ids=[m[0] for m in NODE_MUTANTS])
def test_a_planted_mistake_is_flagged_at_its_node_and_nowhere_else(monkeypatch, mutant, kind, which, step):
    audit, rec, _ = run(monkeypatch, mutants=[mutant])
    assert audit.failures(), f"{mutant}: not noticed"
    of_kind = [n for n in rec.nodes if n.kind == kind]
    if which is None:
        want = {n.index for n in of_kind}
    elif isinstance(which, tuple):
        want = {n.index for n in of_kind if of_kind.index(n) % 5 in which}
    else:
        want = {n.index for n in of_kind if n.step in ((step,) if step is not None else (0, 1)) and
                [m for m in of_kind if m.step == n.step].index(n) == which}
    print(audit.describe_failures())
    assert audit.failed_nodes() == want, (mutant, sorted(audit.failed_nodes(), key=str), sorted(want))
    if step is not None:           # the stale image: step 1's images were right
        assert all(r["step"] == step for r in audit.failures())


def test_bucket_not_zeroed_between_steps_shows_in_step_two(monkeypatch):
    audit, rec, _ = run(monkeypatch, mutants=["bucket not zeroed between steps"])
    bad = audit.failures()
    assert bad and all(r["step"] == 1 and "bucket slot" in r["check"] for r in bad if r["kind"] != "bucket"), audit.describe_failures()
    assert {r["node"] for r in bad} >= {n.index for n in rec.nodes_of(1) if n.kind == "IndiceConvFunction"}


def test_loss_scale_left_on_shows_in_the_update(monkeypatch):
    audit, _, _ = run(monkeypatch, mutants=["loss scale left on"], dtype=torch.float16, loss_scale=2.0 ** 12)
    bad = audit.failures()
    assert bad and {r["node"] for r in bad} == {"AdamW step 1", "AdamW step 2"}, audit.describe_failures()


def test_a_project_node_missing_from_the_record_is_named(monkeypatch):
    audit, _, _ = run(monkeypatch, drop_node="ConvTranspose1x1Function")
    bad = [r for r in audit.failures() if r["node"] == "graph"]
    assert any("ConvTranspose1x1FunctionBackward" in r["note"] for r in bad), audit.describe_failures()
    assert any(r["check"].startswith("counts") for r in bad)


def test_pillar_node_kinds_pass_and_a_wrong_gather_is_flagged(monkeypatch):
    """PFNRadiusTrainFunction and PillarScatterFunction (the all.pp.mhead front end) through recorder and audit."""
    from mhead_train_helpers import RANGE, VOXEL, ragged_pillars
    for mutant in ((), ("pillar gather from the wrong cell",)):
        E = make_ops()
        fns = make_functions(E)
        vox, num, coors = ragged_pillars(40, 6, seed=5)
        coors[:, 2], coors[:, 3] = torch.arange(40) // 8, torch.arange(40) % 8          # a 5 x 8 map for the scatter
        net = A.pfn_module("PFNRadiusTrainFunction", 16, 1e-3, 0.01, (VOXEL[0], VOXEL[1], VOXEL[0] / 2 + RANGE[0], VOXEL[1] / 2 + RANGE[1]))
        l = net.pfn_layers[0]
        if mutant:
            real = E.dense_to_sparse
            E.dense_to_sparse = lambda dense, indices, num_dev=None, depth=0: real(dense, indices.flip(0), num_dev, depth)
        audit = A.Audit()
        with A.Recorder(monkeypatch, [fns.PFNRadiusTrainFunction, fns.PillarScatterFunction], E) as rec:
            out = fns.PFNRadiusTrainFunction.apply(vox, num, coors, l.linear.weight, l.norm.weight, l.norm.bias, l.norm.running_mean,
                                                    l.norm.running_var, 1e-3, 0.01, (net.vx, net.vy, net.x_offset, net.y_offset))
            img = fns.PillarScatterFunction.apply(out.bfloat16(), coors, 1, 5, 8, True)
            w = torch.randn(img.shape, generator=torch.Generator().manual_seed(1))
            loss = (img.float() * w).sum()
            loss.backward()
        A.audit_nodes(rec.nodes, audit, dict(pfn=A.pfn_factory))
        A.audit_graph(loss, rec.nodes, audit, also_allowed=("SumBackward0",))         # this test's own stand-in for a loss
        assert [n.kind for n in rec.nodes] == ["PFNRadiusTrainFunction", "PillarScatterFunction"]
        if mutant:
            assert audit.failed_nodes() == {1}, audit.describe_failures()
        else:
            assert not audit.failures(), audit.describe_failures()
