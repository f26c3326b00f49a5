"""CPU-only checks of the device augmentation's host side: the numpy restatement (tests/augment_helpers.py) against the fixture
recorded from the reference (tests/golden/augment.npz), the C ABI's argument validation (no launch), DeviceAugmenter.from_config
and the refusals.  The kernels themselves: tests/test_gpu_augment.py."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import augment_helpers as ah

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def cases():
    g = np.load(ah.GOLDEN)
    return {name: ah.load_case(name, g) for name in ah.CASES}


@pytest.fixture(scope="module")
def chains(cases):
    return {name: ah.chain(batch) for name, (batch, _) in cases.items()}


@pytest.mark.parametrize("name", list(ah.CASES))
def test_helper_equals_fixture(cases, chains, name):
    batch, ref = cases[name]
    mine = chains[name]
    assert np.array_equal(mine["selected"], ref["selected"])
    first, counts = ah.fixture_first_and_counts(batch, ref)
    assert np.array_equal(mine["first_box"], first) and np.array_equal(mine["counts"], counts)
    kept = np.nonzero(ref["keep"])[0]
    assert np.array_equal(mine["offsets"], ref["offsets"])
    assert np.array_equal(mine["classes"], batch["classes"][kept]) and np.array_equal(mine["importance"], batch["importance"][kept])
    assert mine["boxes"].shape == ref["boxes"].shape
    assert (np.abs(mine["points"] - ref["points"]) <= ah.point_bound(batch)).all()
    assert (np.abs(mine["boxes"][:, :6] - ref["boxes"][:, :6]) <= ah.box_bound(batch, kept)).all()
    dyaw = mine["boxes"][:, 6] - ref["boxes"][:, 6]
    assert (np.abs(dyaw - np.round(dyaw / (2 * np.pi)) * 2 * np.pi) <= 1e-5).all()


def test_fixture_covers_the_special_frames(cases):
    """What the issue asks the recorded frames to contain (the generator asserts the same when it records)."""
    b1, r1 = cases["b1_t5"]
    b5, r5 = cases["b5_t100"]
    assert np.array_equal(np.diff(b5["box_offsets"]), [0, 1, 3, 70, 12]) and np.array_equal(np.diff(b5["point_offsets"]), [257, 0, 1, 601, 150])
    assert r1["selected"][0] == -1 and b1["valid"][1]                       # a valid box failing every try ... (box 0 is invalid there)
    bo = b5["box_offsets"]
    assert r5["selected"][bo[4]] == -1 and b5["valid"][bo[4]]               # ... and one in the T = 100 batch
    assert r5["selected"].max() >= 64                                       # a success in the second wave of tries
    assert not b1["valid"][0] and not b1["valid"][3] and r1["selected"][4] > 0     # invalid boxes (the first among them) that block
    for batch, ref in ((b1, r1), (b5, r5)):
        assert (batch["valid"] & ~ref["keep"]).any()                        # a valid box whose centre left the range
    n, npts = 12, 257
    mask = np.unpackbits(r1["mask0"], count=npts * n).reshape(npts, n)
    assert (mask.sum(1) >= 2).any()                                         # a point inside two overlapping boxes
    flips = np.concatenate([r1["frame_params"][:, :2], r5["frame_params"][:, :2], cases["b1_t1"][1]["frame_params"][:, :2]])
    assert set(flips[:, 0]) == {0.0, 1.0} and set(flips[:, 1]) == {0.0, 1.0}


def test_contained_box_is_a_collision_both_ways():
    """The trap of box_collision_test: run as plain Python (numba stubbed) its `ret[i, j] is False` guard is never true and a box
    inside another is no collision; compiled, it is.  The specification -- helper and kernel -- is the compiled meaning."""
    big = ah.bev_corners(np.array([[10.0, 0, 0, 4, 4, 1, 0.3]]))[0]
    small = ah.bev_corners(np.array([[10.2, 0.1, 0, 1, 1, 1, -0.4]]))[0]
    assert not ah.edges_cross(big, small)
    assert ah.collide(big, small) and ah.collide(small, big)
    far = ah.bev_corners(np.array([[30.0, 0, 0, 1, 1, 1, 0.0]]))[0]
    assert not ah.collide(big, far)
    boxes = np.array([[10.0, 0, 0, 4, 4, 1, 0.3], [20.0, 0, 0, 1, 1, 1, 0.0]])
    loc = np.zeros((2, 2, 3))
    loc[1, 0, :2], loc[1, 1, :2] = (-9.8, 0.1), (0.5, 0.5)                  # first try: inside box 0; second: free
    assert list(ah.noise_per_box(boxes, [True, True], loc, np.zeros((2, 2)))) == [0, 1]


def test_entry_points_validate_before_any_launch():
    """Status codes of include/second_hip.h decided on the host, no GPU needed.  (None of the four entry points takes a workspace, so
    there is no *_workspace_bytes query to check.)"""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)                       # non-NULL, never dereferenced: validation fails first
    r4 = rt.f_arr([0, -40, 70.4, 40])
    assert l.sec_points_in_boxes_f32(one, 4, one, 10, one, one, 3, 1, None, None, None, None) == -1            # no first_box
    assert l.sec_points_in_boxes_f32(one, 4, None, 10, one, one, 3, 1, None, one, None, None) == -1            # no offsets
    assert l.sec_points_in_boxes_f32(one, 2, one, 10, one, one, 3, 1, None, one, None, None) == -3             # pitch < 3
    assert l.sec_points_in_boxes_f32(one, 4, one, 10, one, one, 3, 0, None, one, None, None) == -1             # batch 0
    npb = (one, one, 3, 1, None, one, one)
    assert l.sec_noise_per_box_f32(*npb, 100, 512, None, one, one, None) == -1                                 # no selected
    assert l.sec_noise_per_box_f32(*npb, 100, 512, one, None, one, None) == -1 and l.sec_noise_per_box_f32(*npb, 100, 512, one, one, None, None) == -1
    assert l.sec_noise_per_box_f32(*npb, 129, 512, one, one, one, None) == -3                                  # more than 128 tries
    assert l.sec_noise_per_box_f32(*npb, 100, 513, one, one, one, None) == -3                                  # more than 512 boxes per frame
    assert l.sec_noise_per_box_f32(*npb, 0, 512, one, one, one, None) == -1
    assert l.sec_augment_points_f32(None, 4, one, 10, 1, None, None, None, None, None, one, None) == -1        # no points
    assert l.sec_augment_points_f32(one, 4, one, 10, 1, None, None, None, None, None, None, None) == -1        # no frame_params
    assert l.sec_augment_points_f32(one, 4, one, 10, 1, one, one, None, None, one, one, None) == -1            # first_box without transforms
    assert l.sec_augment_points_f32(one, 2, one, 10, 1, None, None, None, None, None, one, None) == -3         # pitch < 3
    assert l.sec_augment_points_f32(one, 4, one, 0, 1, None, None, None, None, None, one, None) == 0           # nothing to do, nothing launched
    ab = (one, one, 3, 1, None, None, None)
    assert l.sec_augment_boxes_f32(*ab, None, None, one, r4, None, one, one, one, None) == -1                  # no out_boxes
    assert l.sec_augment_boxes_f32(*ab, None, None, one, r4, one, one, one, None, None) == -1                  # no out_offsets
    assert l.sec_augment_boxes_f32(*ab, one, None, one, r4, one, one, one, one, None) == -1                    # one transform without the other
    assert l.sec_augment_boxes_f32(*ab, None, None, one, None, one, one, one, one, None) == -1                 # no range


CAR = dict(gt_rotation_noise=(-0.78539816, 0.78539816), gt_loc_noise_std=(1.0, 1.0, 0.5), global_rotation_noise=(-0.78539816, 0.78539816),
           global_scaling_noise=(0.95, 1.05), global_translate_noise_std=(0.0, 0.0, 0.0), random_flip_x=False, random_flip_y=True)
CONFIGS = [
    ("car.fhd.config", dict(CAR, bev_range=(0.0, -40.0, 70.4, 40.0)), False),
    ("car.lite.config", dict(CAR, bev_range=(0.0, -32.0, 52.8, 32.0)), False),
    ("nuscenes/all.fhd.config", dict(gt_rotation_noise=(0.0, 0.0), gt_loc_noise_std=(0.0, 0.0, 0.0), global_rotation_noise=(0.0, 0.0),
                                     global_scaling_noise=(1.0, 1.0), global_translate_noise_std=(0.0, 0.0, 0.0), random_flip_x=True,
                                     random_flip_y=True, bev_range=(-49.6, -49.6, 49.6, 49.6)), True),
]


@pytest.mark.parametrize("rel, want, skipped", CONFIGS)
def test_from_config_reads_the_reference_configs(rel, want, skipped):
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    from google.protobuf import text_format
    from second_amd import compat
    from second_amd.augment import DeviceAugmenter
    compat.install(REF)
    from second.protos import pipeline_pb2
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(REF, "second/configs", rel)).read(), cfg)
    aug = DeviceAugmenter.from_config(cfg.train_input_reader.preprocess, list(cfg.model.second.voxel_generator.point_cloud_range))
    for k, v in want.items():
        assert getattr(aug, k) == pytest.approx(v, rel=1e-6), k
    assert aug.per_object_skipped is skipped and aug.num_try == 100


def _proto(**over):
    p = dict(use_group_id=False, global_random_rotation_range_per_object=[0, 0], groundtruth_rotation_uniform_noise=[-0.78539816, 0.78539816],
             groundtruth_localization_noise_std=[1.0, 1.0, 0.5], global_rotation_uniform_noise=[-0.78539816, 0.78539816],
             global_scaling_uniform_noise=[0.95, 1.05], global_translate_noise_std=[0, 0, 0], random_flip_x=False, random_flip_y=True)
    p.update(over)
    return types.SimpleNamespace(**p)


def test_from_config_on_a_message_shaped_object_and_the_two_refusals():
    from second_amd.augment import DeviceAugmenter
    vg = types.SimpleNamespace(point_cloud_range=np.array([0, -40, -3, 70.4, 40, 1], np.float32))
    aug = DeviceAugmenter.from_config(_proto(), vg, num_try=50)
    for k, v in dict(CAR, bev_range=(0.0, -40.0, 70.4, 40.0)).items():
        assert getattr(aug, k) == pytest.approx(v, rel=1e-6), k
    assert aug.num_try == 50 and not aug.per_object_skipped
    assert DeviceAugmenter.from_config(_proto(groundtruth_rotation_uniform_noise=[0, 0], groundtruth_localization_noise_std=[0, 0, 0]),
                                       vg).per_object_skipped
    with pytest.raises(ValueError, match="use_group_id"):
        DeviceAugmenter.from_config(_proto(use_group_id=True), vg)
    with pytest.raises(ValueError, match="global_random_rotation_range_per_object"):
        DeviceAugmenter.from_config(_proto(global_random_rotation_range_per_object=[0.78, 2.35]), vg)
    with pytest.raises(ValueError, match="num_try"):
        DeviceAugmenter.from_config(_proto(), vg, num_try=129)
    with pytest.raises(ValueError, match="max_boxes_per_frame"):
        DeviceAugmenter.from_config(_proto(), vg, max_boxes_per_frame=513)


def test_cpu_tensors_and_devices_are_refused():
    """draw needs the GPU to run: on the CPU only its refusals can be checked, like every op of the package."""
    from second_amd import ops
    from second_amd.augment import DeviceAugmenter
    from second_amd.runtime import SecondHipError
    aug = DeviceAugmenter(device="cpu", point_cloud_range=[0, -40, -3, 70.4, 40, 1], **CAR)
    with pytest.raises(SecondHipError):
        aug.draw(num_boxes=4, batch_size=1)
    with pytest.raises(SecondHipError):
        aug.set_noise(frame_params=torch.zeros(1, 8))
    pts, po = torch.zeros(5, 4), torch.tensor([0, 5], dtype=torch.int32)
    boxes, bo = torch.zeros(2, 7), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(SecondHipError):
        aug(pts, po, boxes, bo)
    with pytest.raises(SecondHipError):
        ops.points_in_boxes(pts, po, boxes, bo)
    with pytest.raises(SecondHipError):
        ops.noise_per_box(boxes, bo, None, torch.zeros(2, 5, 3), torch.zeros(2, 5))
    with pytest.raises(SecondHipError):
        ops.augment_points_(pts, po, torch.zeros(1, 8))
    with pytest.raises(SecondHipError):
        ops.augment_boxes(boxes, bo, torch.zeros(1, 8), (0, -40, 70.4, 40))
