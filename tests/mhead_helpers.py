"""Shared by tests/test_gpu_mhead.py and tools/mhead_probe.py: the all.pp.mhead stand-in (tests/reference_standin_mhead.py) with
weights of trained-network shape."""
import torch


def standin(cfg, seed=0):
    from reference_standin_mhead import build_voxelnet_mhead
    from second_amd import synthetic as syn
    torch.manual_seed(seed)
    net = build_voxelnet_mhead(cfg)
    syn.randomise_like_trained(net, seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for m in net.small_head.net:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(2.5)
            if isinstance(m, torch.nn.BatchNorm2d):
                # variances down to 1e-4: eps 1e-5 and eps 1e-3 then differ by a factor of up to 3 in the folded scale
                m.running_var.copy_(torch.empty(64).uniform_(1e-4, 2e-3, generator=g))
                m.weight.copy_(torch.empty(64).uniform_(0.01, 0.04, generator=g))
    return net


def sharpen(net, calib):
    """Head logits of trained-network shape for both heads (second_amd.synthetic.sharpen_heads, per head): empty regions score
    sigmoid(-4.5) < 0.05, the strongest anchor of the calibration frame logit 10; box residuals |delta| <= 0.5."""
    with torch.no_grad():
        empty = net.rpn(torch.zeros(1, 64, 192, 192, device="cuda"))
        large, small = calib
        for head, name, src, cal in ((net.large_head, "out", empty["out"], large), (net.small_head, "stage0", empty["stage0"], small)):
            e = head(src)["cls_preds"]
            a, nc = head._num_anchor_per_loc, head._num_class
            hw = e.shape[1] // a
            side = int(round(hw ** 0.5))
            c_empty = e.view(a, side, side, nc)[:, side // 2, side // 2].float()       # interior value per (anchor, class)
            d = cal["cls_preds"][0].view(a, -1, nc) - c_empty.view(a, 1, nc)
            s = 14.5 / float(d.max())
            head.conv_cls.weight.mul_(s)
            head.conv_cls.bias.copy_(s * (head.conv_cls.bias - c_empty.reshape(-1)) - 4.5)
            sb = 0.5 / float(cal["box_preds"].abs().max())
            head.conv_box.weight.mul_(sb)
            head.conv_box.bias.mul_(sb)



def trained_like_standin(cfg, calib_cloud, device="cuda"):
    """The stand-in on ``device`` in eval mode, heads sharpened on ``calib_cloud`` (distinct scores, empty regions below the threshold)."""
    from reference_standin import example_of
    from reference_standin_mhead import module_graph_dense
    net = standin(cfg).eval().to(device)
    ex = example_of(net, [calib_cloud], device)
    with torch.no_grad():
        feats = net.voxel_feature_extractor(ex["voxels"], ex["num_points"], ex["coordinates"])
        img = net.middle_feature_extractor(feats, ex["coordinates"], 1)
        sharpen(net, module_graph_dense(net, img))
    return net
