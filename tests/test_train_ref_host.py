"""The float64 references of tests/train_ref_helpers.py against what the reference project itself computed (the fixtures behind
tests/test_gpu_train.py), so that tests/test_gpu_train_edges.py compares the kernels with something pinned.  No GPU."""
import numpy as np
import pytest

import train_ref_helpers as H

SCALARS = ("loss", "cls_loss_reduced", "loc_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss")
LATTICE_SEEDS = (0, 1)          # what tests/test_gpu_train_edges.py uses


def test_loss_defaults_are_the_packages():
    from second_amd import ops
    assert H.LOSS_DEFAULTS == ops.LOSS_DEFAULTS and set(H.LOSS_KEYS) == set(ops.LOSS_DEFAULTS)


def test_assign_ref_reproduces_the_single_class_fixture(golden):
    g = golden("train_targets_losses")
    for f in range(3):
        labels, targets, imp, _ = H.assign_ref(g["anchors"], g[f"gt_{f}"], float(g["matched_threshold"]), float(g["unmatched_threshold"]))
        np.testing.assert_array_equal(labels, g["labels"][f])
        np.testing.assert_array_equal(imp, g["importance"][f])
        np.testing.assert_allclose(targets, g["bbox_targets"][f], rtol=0, atol=2e-6)
    assert (g["labels"] > 0).sum() >= 20 and (g["labels"] == -1).any()


@pytest.mark.parametrize("mode", ["per_class", "all"])
def test_assign_per_class_ref_reproduces_the_multiclass_fixture(golden, mode):
    g = golden("train_targets_multiclass")
    ids = [1, 2, 3] if mode == "per_class" else [0, 0, 0]
    for f in range(3):
        labels, targets, imp = H.assign_per_class_ref(g["anchors"], g[f"gt_{f}"], g[f"gt_classes_{f}"], g["class_anchor_begin"].tolist(), ids,
                                                      g["matched"].tolist(), g["unmatched"].tolist(), gt_importance=g[f"gt_importance_{f}"])
        np.testing.assert_array_equal(labels, g[f"labels_{mode}"][f])
        np.testing.assert_array_equal(imp, g[f"importance_{mode}"][f])
        np.testing.assert_allclose(targets, g[f"bbox_targets_{mode}"][f], rtol=0, atol=2e-6)
    assert (g[f"importance_{mode}"] != 1.0).any()


def _check_loss(g, got):
    out6, d_cls, d_box, d_dir = got
    np.testing.assert_allclose(out6, np.array([g[k] for k in SCALARS], np.float64), rtol=1e-4)
    for name, got_g, ref_g in (("cls", d_cls, g["d_cls"]), ("box", d_box, g["d_box"]), ("dir", d_dir, g["d_dir"])):
        np.testing.assert_allclose(got_g, ref_g, rtol=1e-4, atol=1e-6 * np.abs(ref_g).max() + 1e-9, err_msg=name)


def test_loss_ref_reproduces_the_single_class_fixture(golden):
    g = golden("train_targets_losses")
    _check_loss(g, H.loss_ref(g["cls_preds"], g["box_preds"], g["dir_preds"], g["labels"], g["bbox_targets"], g["anchors"], g["importance"]))


def test_loss_ref_reproduces_the_three_class_fixture(golden):
    g = golden("train_targets_multiclass")
    _check_loss(g, H.loss_ref(g["cls_preds"], g["box_preds"], g["dir_preds"], g["labels_per_class"], g["bbox_targets_per_class"], g["anchors"],
                              g["importance_per_class"], num_class=3, direction_offset=0.78))


@pytest.mark.parametrize("seed", LATTICE_SEEDS)
def test_lattice_case_meets_its_own_conditions(seed):
    """lattice_case asserts exactness and population itself; here for every seed and size the GPU tests use."""
    c = H.lattice_case(seed)
    assert [len(g) for g in c["gt"]] == [300, 256, 257, 0, 1] and c["anchors"].shape == (874, 7)
    assert 0 < int((c["classes"][0] == 2).sum()) < 10 and (np.nonzero(c["classes"][0] == 2)[0] >= 256).any()
    assert not (c["classes"][1] == 3).any() and (c["classes"][2] == 3).any()
    # ground truth beyond the first 256 of a frame is the best match of some anchors, and ties reach across the chunk border
    _, _, _, info = H.assign_ref(c["anchors"], c["gt"][0], 0.6, 0.45)
    assert (info["arg"] >= 256).sum() >= 20


def test_loss_case_keeps_direction_targets_off_the_bin_edges():
    for bins, off in ((2, 0.0), (4, 0.78)):
        c = H.loss_case(5, 3, 1000, 3, bins, direction_offset=off)
        assert H.dir_bin_margin(c["reg"], c["anchors"], np.ones_like(c["labels"]), off, bins) >= 1e-4
        assert not (c["labels"][1] > 0).any() and (c["labels"][0] > 0).sum() >= 20 and (c["labels"] == -1).sum() >= 20


def test_fp32_evaluation_of_the_loss_reference_sits_far_inside_the_kernel_tolerances():
    """The yardstick for the tolerances of test_gpu_train_edges.py (rtol 1e-4 scalars, 1e-6 of the largest entry for gradients):
    the same formulas in fp32 differ from fp64 by 2.7e-6 (scalars, relative) and 1.3e-6 (gradients, of the largest entry) on the edge
    inputs -- measured on a CPU."""
    import torch
    worst_s = worst_g = 0.0
    for cfg in ({}, H.LOSS_NONDEFAULT, dict(gamma=0.0)):
        for n, nc, bins in ((37, 1, 2), (1000, 3, 4), (1000, 1, 0)):
            c = H.loss_case(11, 3, n, nc, bins, direction_offset=cfg.get("direction_offset", 0.0))
            args = (c["cls"], c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"])
            r64 =H.loss_ref(*args, num_class=nc, num_direction_bins=bins, **cfg)
            r32 = H.loss_ref(*args, num_class=nc, num_direction_bins=bins, dtype=torch.float32, **cfg)
            nz = r64[0] != 0
            worst_s = max(worst_s, float(np.max(np.abs(r32[0][nz] - r64[0][nz]) / np.abs(r64[0][nz]))))
            for a, b in zip(r32[1:], r64[1:]):
                if b is not None:
                    worst_g = max(worst_g, float(np.abs(a - b).max() / np.abs(b).max()))
    assert worst_s < 2.5e-5 and worst_g < 2.5e-5, (worst_s, worst_g)      # a quarter of rtol 1e-4: four times fp32 rounding still fits


def test_adamw_ref_is_torch_adamw_with_clip_grad_norm():
    import torch
    g = torch.Generator().manual_seed(1)
    p = torch.nn.Parameter(torch.randn(500, generator=g, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=3e-3, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8)
    q, m, v = p.detach().numpy().copy(), np.zeros(500), np.zeros(500)
    for step, scale in enumerate((0.01, 3.0, 0.2), 1):
        gr = torch.randn(500, generator=g, dtype=torch.float64) * scale
        p.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_([p], 10.0)
        opt.step()
        q, m, v, n = H.adamw_ref(q, m, v, gr.numpy(), step, 3e-3, 0.9, 0.99, 1e-8, 0.01, 10.0)
        assert abs(n - float(norm)) <= 1e-12 * n
        np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert 3.0 * np.sqrt(500) > 10.0 > 0.2 * np.sqrt(500)          # clipped in one step, not in the others
