"""CPU-only: the SimpleVoxelRadius entry points (sec_voxelize_encode_f32, sec_simple_voxel_radius_f32) are exported, bound in
``runtime.SYMBOLS`` and validate their arguments on the host, before any launch; the ABI version stays 9 (additions only).  Plus
the host logic around them that needs no GPU: the zero-padded first-layer weight, the layer plans, the training refusal."""
import ctypes

import numpy as np
import pytest
import torch


def test_radius_symbols_are_exported_and_bound():
    from second_amd import runtime as rt
    l = rt.lib()
    for name in ("sec_voxelize_encode_f32", "sec_simple_voxel_radius_f32"):
        assert name in rt.SYMBOLS and hasattr(l, name), name
        assert getattr(l, name).argtypes, name
    assert l.sec_abi_version() == rt.ABI_VERSION == 9
    # the sibling takes sec_voxelize_f32's arguments plus (encoder, out_pitch)
    assert len(l.sec_voxelize_encode_f32.argtypes) == len(l.sec_voxelize_f32.argtypes) + 2


def test_radius_entry_points_validate_before_any_launch():
    """Status codes of include/second_hip.h, decided on the host (the pointers are never dereferenced: no GPU needed)."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)          # 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(4100)          # not a whole-row address
    rng, vs = rt.f_arr([0, -32, -3, 52.8, 32, 1]), rt.f_arr([0.05, 0.05, 0.1])
    inval, unsup = -1, -3

    def vox(mean, mean_features, dtype, encoder, pitch, max_points=1, num_features=4):
        return l.sec_voxelize_encode_f32(one, one, 1000, num_features, 1, rng, vs, max_points, 100, 0, one, one, one, one, mean, mean_features,
                                         dtype, encoder, pitch, one, 1 << 30, None)
    assert vox(one, 4, rt.SEC_F32, 2, 4) == inval and vox(one, 4, rt.SEC_F32, -1, 4) == inval          # encoder outside {0, 1}
    assert vox(one, 3, rt.SEC_F32, 1, 4) == unsup                                                      # radius: four features in only
    assert vox(one, 4, rt.SEC_BF16, 1, 3) == inval and vox(one, 4, rt.SEC_BF16, 1, 8) == inval         # radius rows have a pitch of 4
    assert vox(None, 0, rt.SEC_F32, 1, 4) == inval                                                     # nothing to encode into
    assert vox(odd, 4, rt.SEC_F16, 1, 4) == inval                                                      # rows are stored whole
    assert vox(one, 4, rt.SEC_F32, 0, 3) == inval and vox(one, 3, rt.SEC_F32, 0, 4) == inval           # SimpleVoxel: pitch = mean_features
    assert vox(one, 4, rt.SEC_F32, 1, 4, max_points=300) == unsup                                      # the voxeliser's own limits still hold
    assert vox(one, 5, rt.SEC_F32, 1, 4) in (inval, unsup)                                             # mean_features > num_features

    def rad(voxels, n, mean_features, out, pitch, dtype, num_features=4):
        return l.sec_simple_voxel_radius_f32(voxels, one, n, None, 5, num_features, mean_features, out, pitch, dtype, None)
    assert rad(one, 10, 4, None, 4, rt.SEC_F32) == inval and rad(None, 10, 4, one, 4, rt.SEC_F32) == inval
    assert rad(one, -1, 4, one, 4, rt.SEC_F32) == inval
    assert rad(one, 10, 3, one, 4, rt.SEC_F32) == unsup and rad(one, 10, 4, one, 4, 7) == unsup
    assert rad(one, 10, 4, one, 3, rt.SEC_F32) == inval and rad(one, 10, 4, odd, 4, rt.SEC_BF16) == inval
    assert rad(one, 10, 5, one, 4, rt.SEC_F32, num_features=4) == inval
    assert rad(None, 0, 4, one, 4, rt.SEC_F32) == 0                                                    # an empty batch is fine


def test_first_layer_weight_is_zero_padded_only_for_rows_declared_as_pitch_4():
    """SparseConvolution.pad_in_channels: the parameter keeps the reference's [3, 3, 3, 3, 16] shape and key; the zero-padded image is
    used only when the producer DECLARES pitch-4 rows on the tensor (SparseConvTensor.in_pitch, inference) -- never inferred from the
    column count: four columns of anything else meet the three-channel weight and fail loudly, as before."""
    import spconv
    from second_amd.models import ALL_FHD_KITTI, CAR_LITE, PEOPLE_FHD, SecondDetector
    det = SecondDetector(CAR_LITE)
    conv = det.middle_feature_extractor.middle_conv[0]
    assert tuple(conv.weight.shape) == (3, 3, 3, 3, 16) and conv.pad_in_channels == 4 and not conv.subm
    assert "middle_feature_extractor.middle_conv.0.weight" in det.state_dict()
    idx = torch.zeros((5, 4), dtype=torch.int32)

    def tensor(cols, pitch=None):
        x = spconv.SparseConvTensor(torch.zeros(5, cols), idx, [41, 1280, 1056], 1)
        if pitch is not None:
            x.in_pitch = pitch
        return x
    with torch.no_grad():
        assert conv.takes_padded_rows(tensor(4, 4)) and not conv.takes_padded_rows(tensor(4)) and not conv.takes_padded_rows(tensor(3))
        w4 = conv.kernel_weight(padded=True)
        assert tuple(w4.shape) == (3, 3, 3, 4, 16) and torch.equal(w4[..., :3, :], conv.weight) and not w4[..., 3, :].any()
        assert conv.kernel_weight() is conv.weight
        conv.weight.mul_(2.0)                                      # a changed parameter is padded again
        assert torch.equal(conv.kernel_weight(padded=True)[..., :3, :], conv.weight)
        with pytest.raises(ValueError, match="pitch of 4"):
            conv.takes_padded_rows(tensor(3, 4))                   # declared, but the rows are not that wide
        plain = spconv.SubMConv3d(3, 16, 3, bias=False)            # a user's own 3-channel layer was not built for it
        assert plain.pad_in_channels is None
        with pytest.raises(ValueError, match="pitch of 4"):
            plain.takes_padded_rows(tensor(4, 4))
    with pytest.raises(ValueError, match="grad on"):               # the padded form is inference only: no gradient through the pad
        conv.takes_padded_rows(tensor(4, 4))
    assert SecondDetector(PEOPLE_FHD).middle_feature_extractor.middle_conv[0].pad_in_channels is None
    first = SecondDetector(ALL_FHD_KITTI).middle_feature_extractor.middle_conv[0]          # KITTI all.fhd: SubMConv3d(3, 16), same route
    assert first.subm and tuple(first.weight.shape) == (3, 3, 3, 3, 16) and first.pad_in_channels == 4


def test_simple_voxel_radius_module_always_returns_three_columns():
    from second_amd.models import SimpleVoxelRadius
    vfe = SimpleVoxelRadius(4)
    v, n = torch.rand(7, 5, 4), torch.full((7,), 5, dtype=torch.int32)
    with torch.no_grad():
        assert vfe(v, n).shape == (7, 3)
        rows, pitch = vfe.encode(v, n)                             # no device kernel on the CPU: the formulation, no pitch declared
    assert rows.shape == (7, 3) and pitch is None and vfe(v, n).shape == (7, 3)


def test_device_trainer_refuses_the_radius_networks_before_touching_them():
    """DeviceTrainer's forward feeds the voxeliser's SimpleVoxel means to the middle: a network whose middle expects radius rows is
    refused in the constructor (no parameter broadcast, no mode change), naming the encoder."""
    from second_amd.models import ALL_FHD_KITTI, CAR_LITE, SecondDetector
    from second_amd.training import DeviceTrainer
    for cfg in (CAR_LITE, ALL_FHD_KITTI):
        det = SecondDetector(cfg).eval()
        with pytest.raises(NotImplementedError, match="SimpleVoxelRadius"):
            DeviceTrainer(det)
        assert not det.training


def test_layer_plans_and_map_sizes():
    import spconv
    from second_amd import ops
    from second_amd.models import CAR_LITE, PEOPLE_FHD, SecondDetector
    for cfg, fm, z, n_strided, n_subm in ((CAR_LITE, [1, 160, 132], [41, 21, 11, 5, 2], 4, 0), (PEOPLE_FHD, [1, 200, 240], [21, 11, 5, 2], 3, 7)):
        det = SecondDetector(cfg)
        assert det.feature_map_size == fm and type(det.middle_feature_extractor).__name__ == cfg["middle"]
        assert type(det.voxel_feature_extractor).__name__ == cfg.get("vfe", "SimpleVoxel")
        convs = [m for m in det.middle_feature_extractor.modules() if isinstance(m, spconv.SparseConvolution)]
        assert sum(not m.subm for m in convs) == n_strided and sum(m.subm for m in convs) == n_subm
        shape = list(det.middle_feature_extractor.sparse_shape)
        assert shape[0] == z[0]
        for m, zz in zip([m for m in convs if not m.subm], z[1:]):
            shape = ops.conv_output_shape(shape, m.kernel_size, m.stride, m.padding, m.dilation)
            assert shape[0] == zz, (cfg["name"], shape)
        assert shape == [2] + fm[1:] and convs[-1].out_channels == 64
        assert det.anchors.shape[0] == det.num_anchor_per_loc * fm[1] * fm[2]


def test_simple_voxel_radius_torch_formulation_matches_the_reference_fixture(golden):
    """tests/golden/simple_voxel_radius.npz was produced by executing the reference's SimpleVoxelRadius.forward on CPU
    (tests/golden/make_golden_lite.py); the mirror's torch formulation is the same arithmetic."""
    from second_amd.models import SimpleVoxelRadius
    z = golden("simple_voxel_radius")
    vfe = SimpleVoxelRadius(4)
    for t in (1, 5):
        out = vfe(torch.from_numpy(z[f"voxels_t{t}"]), torch.from_numpy(z[f"num_points_t{t}"]))
        assert out.shape[1] == 3
        np.testing.assert_array_equal(out.numpy(), z[f"out_t{t}"])


def test_training_of_the_new_networks_is_refused_before_any_forward():
    """dropin_train has a captured step for SimpleVoxel + SpMiddleFHD only: the other adoptable networks raise NotTrainable in the
    constructor, naming the VFE / middle, and the engine keeps the original forward for training-mode calls."""
    from reference_standin_lite import build_voxelnet_lite
    from second_amd import dropin, dropin_train as T
    from second_amd.models import CAR_LITE, PEOPLE_FHD
    for cfg, word in ((CAR_LITE, "SimpleVoxelRadius"), (PEOPLE_FHD, "SpMiddleFHDPeople"), (dict(PEOPLE_FHD, vfe="SimpleVoxel", middle="SpMiddleFHDLite", middle_in=4, downsample_factor=8), "SpMiddleFHDLite")):
        net = build_voxelnet_lite(cfg)
        calls = []
        net.network_forward = lambda *a, **k: calls.append(a)
        c = dropin.model_config(net)
        assert c["middle"] == cfg["middle"]
        with pytest.raises(T.NotTrainable, match=word):
            T.FusedTrainStep(net, c, torch.bfloat16)
        eng = dropin.FusedVoxelNet(net, train_dtype=torch.bfloat16)
        net.train()
        assert not eng.accepts({"voxels": torch.zeros(1, cfg["max_points_per_voxel"], 4)})
        assert eng.trainer is False and word in eng.stats["train_fallback_reason"] and not calls
