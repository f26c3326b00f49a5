"""CPU-only checks of the device database sampling's host side: the numpy restatement (tests/dbsample_helpers.py) against the fixture
recorded from the reference (tests/golden/dbsample.npz), DeviceGtDatabase.from_infos / from_config and their refusals, the table of
numbers to draw, the draw cursor, and the C ABI's argument validation (no launch).  The kernels: tests/test_gpu_dbsample.py."""
import ctypes
import pickle
import types

import numpy as np
import pytest
import torch

import augment_helpers as ah
import dbsample_helpers as dh


@pytest.fixture(scope="module")
def cases():
    g = np.load(dh.GOLDEN)
    return {name: dh.load_case(name, g) for name in dh.CASES}


@pytest.mark.parametrize("name", list(dh.CASES))
def test_helper_equals_fixture(cases, name):
    case, _, db, batch, ref = cases[name]
    mine = dh.chain(batch, db, case, dh.candidates_of(ref))
    for k in ("accepted", "accepted_offsets", "accepted_per_group", "box_offsets", "classes", "mask", "point_offsets"):
        np.testing.assert_array_equal(mine[k], ref[k], err_msg=k)
    for k in ("boxes", "importance", "points"):
        np.testing.assert_array_equal(mine[k].view(np.int32), ref[k].view(np.int32), err_msg=k)
    np.testing.assert_array_equal(mine["removed"], np.unpackbits(ref["removed"], count=len(batch["points"])).astype(bool))


def _greedy(gt_boxes, db_boxes, rows):
    """What the acceptance rule is NOT: each candidate against the gt boxes and what was accepted so far."""
    avoid, out = list(ah.bev_corners(gt_boxes.astype(np.float64))), []
    for r in rows:
        c = ah.bev_corners(db_boxes[[r]].astype(np.float64))[0]
        if not any(ah.collide(c, a) for a in avoid):
            avoid.append(c)
            out.append(r)
    return out


def test_fixture_covers_the_special_frames(cases):
    """What the issue asks the recorded frames to contain (the generator asserts the same when it records)."""
    case, _, db, batch, ref = cases["ab"]
    cands, acc = dh.candidates_of(ref)[0][0], list(ref["accepted"])
    a, b = sorted((cands.index(0), cands.index(1)))                         # rows 0 and 1 are the overlapping pair A, B
    assert cands[a] not in acc and cands[b] in acc                          # the earlier one is rejected, the later one accepted
    greedy = _greedy(batch["boxes"], db["boxes"], cands)
    assert cands[a] in greedy and cands[b] not in greedy and greedy != acc  # ... which a greedy loop gets the other way round
    case, _, db, batch, ref = cases["multi"]
    table = dh.num_table(case["groups"], case["rate"])
    counts = [int((batch["classes"][:batch["box_offsets"][1]] == c + 1).sum()) for c in range(3)]
    assert counts == [2, 1, 2]
    assert case["rate"] * (7 - 2) == 2.5 and table[0][2] == 2               # .5 -> even, down
    assert case["rate"] * (4 - 1) == 1.5 and table[1][1] == 2               # .5 -> even, up
    assert table[2][2] == 0 and ref["accepted_per_group"][0][2] == 0 and (ref["candidates"][0, 2] < 0).all()    # the maximum is reached
    assert not batch["valid"][:batch["box_offsets"][1]].all()               # a gt box of no target class
    case, _, db, batch, ref = cases["car"]
    assert list(np.diff(batch["box_offsets"])) == [3, 0, 5, 12] and list(np.diff(batch["point_offsets"])) == [800, 600, 0, 1300]
    table = dh.num_table(case["groups"], case["rate"])
    got = (ref["candidates"][:, 0] >= 0).sum(1)
    asked = [table[0][int((batch["classes"][batch["box_offsets"][f]:batch["box_offsets"][f + 1]] == 1).sum())] for f in range(4)]
    assert any(0 < g < w for g, w in zip(got, asked))                       # the sampler returned fewer than asked
    assert any(ref["accepted_per_group"][f, 0] < got[f] for f in range(4))  # and some candidates are rejected
    assert np.unpackbits(ref["removed"], count=len(batch["points"])).sum() > 0


def _write_pool(root, infos):
    (root / "gt_database").mkdir(exist_ok=True)
    for v in infos.values():
        for info in v:
            info["points"].tofile(str(root / info["path"]))
    return {n: [{k: x for k, x in info.items() if k != "points"} for info in v] for n, v in infos.items()}


@pytest.mark.parametrize("name", ["car", "multi"])
def test_from_infos_applies_the_reference_filters(cases, tmp_path, name):
    from second_amd.augment import DeviceDatabaseSampler, DeviceGtDatabase
    from second_amd.runtime import SecondHipError
    case, infos, db, batch, ref = cases[name]
    plain = _write_pool(tmp_path, infos)
    d = DeviceGtDatabase.from_infos(plain, tmp_path, dh.NUM_POINT_FEATURES, case["class_names"], min_num_points=case["min_num_points"],
                                    removed_difficulties=case["removed_difficulties"], device="cpu")
    for n in infos:
        np.testing.assert_array_equal(d.info_index[d.class_rows[n]], ref[f"filtered/{n}"])
        assert len(ref[f"filtered/{n}"]) < len(infos[n])                    # the filters removed something
    assert d.names == db["names"] and d.boxes.dtype == torch.float32 and d.pool_offsets.dtype == torch.int32
    np.testing.assert_array_equal(d.boxes.numpy(), db["boxes"])
    np.testing.assert_array_equal(d.pool_points.numpy(), db["points"])
    np.testing.assert_array_equal(d.pool_offsets.numpy(), db["offsets"])
    only = DeviceGtDatabase.from_infos(plain, tmp_path, dh.NUM_POINT_FEATURES, case["class_names"], only=[case["groups"][0][0]], device="cpu")
    assert set(only.names) == {case["groups"][0][0]} and len(only) == len(infos[case["groups"][0][0]])
    # construction on the CPU is fine; a call is refused like every op of the package
    sampler = DeviceDatabaseSampler(d, groups=case["groups"], rate=case["rate"])
    sampler.draw(torch.Generator().manual_seed(0), batch_size=len(batch["box_offsets"]) - 1)
    with pytest.raises(SecondHipError):
        sampler(torch.from_numpy(batch["points"]), torch.from_numpy(batch["point_offsets"]), torch.from_numpy(batch["boxes"]),
                torch.from_numpy(batch["box_offsets"]), torch.from_numpy(batch["classes"]))
    with pytest.raises(SecondHipError):
        sampler.set_candidates(torch.zeros((1, len(case["groups"]), 4), dtype=torch.int32))


class _Step:
    def __init__(self, **kw):
        (self.kind, value), = kw.items()
        setattr(self, self.kind, value)

    def WhichOneof(self, _):
        return self.kind


def _sampler_proto(path, groups=({"Car": 15},), grot=(0.0, 0.0), rate=1.0):
    return types.SimpleNamespace(
        database_info_path=str(path), sample_groups=[types.SimpleNamespace(name_to_max_num=g) for g in groups],
        database_prep_steps=[_Step(filter_by_min_num_points=types.SimpleNamespace(min_num_point_pairs={"Car": 5})),
                             _Step(filter_by_difficulty=types.SimpleNamespace(removed_difficulties=[-1]))],
        global_random_rotation_range_per_object=list(grot), rate=rate)


def test_from_config_and_the_refusals_by_name(cases, tmp_path):
    from second_amd.augment import DeviceAugmenter, DeviceDatabaseSampler, DeviceGtDatabase
    case, infos, db, _, ref = cases["car"]
    plain = _write_pool(tmp_path, infos)
    with open(tmp_path / "dbinfos.pkl", "wb") as f:
        pickle.dump(plain, f)
    d = DeviceGtDatabase.from_config(_sampler_proto("dbinfos.pkl"), tmp_path, dh.NUM_POINT_FEATURES, ["Car"], device="cpu")
    np.testing.assert_array_equal(d.info_index, ref["filtered/Car"])
    assert d.groups == [("Car", 15)] and d.rate == 1.0
    np.testing.assert_array_equal(d.boxes.numpy(), db["boxes"])
    with pytest.raises(ValueError, match="sample_groups"):
        DeviceGtDatabase.from_config(_sampler_proto(tmp_path / "dbinfos.pkl", groups=({"Car": 15, "Van": 3},)), tmp_path, 4, ["Car"], device="cpu")
    with pytest.raises(ValueError, match="global_random_rotation_range_per_object"):
        DeviceGtDatabase.from_config(_sampler_proto(tmp_path / "dbinfos.pkl", grot=(0.78, 2.35)), tmp_path, 4, ["Car"], device="cpu")
    with pytest.raises(ValueError, match="random_crop"):
        DeviceGtDatabase.from_config(_sampler_proto(tmp_path / "dbinfos.pkl"), tmp_path, 4, ["Car"], random_crop=True, device="cpu")
    with pytest.raises(ValueError, match="sample_groups"):
        DeviceDatabaseSampler(d, groups=[{"Car": 15, "Van": 3}])
    with pytest.raises(ValueError, match="sample_groups"):
        DeviceDatabaseSampler(d, groups=[("Van", 3)])                       # no target class
    with pytest.raises(ValueError, match="candidates per frame"):
        DeviceDatabaseSampler(d, groups=[("Car", 65)])
    # the augmenter builds its sampler from the preprocess message when a database is given, and stays as it was without one
    p = types.SimpleNamespace(use_group_id=False, global_random_rotation_range_per_object=[0, 0], groundtruth_rotation_uniform_noise=[-0.78, 0.78],
                              groundtruth_localization_noise_std=[1.0, 1.0, 0.5], global_rotation_uniform_noise=[-0.78, 0.78],
                              global_scaling_uniform_noise=[0.95, 1.05], global_translate_noise_std=[0, 0, 0], random_flip_x=False,
                              random_flip_y=True, remove_points_after_sample=False, sample_importance=0.25)
    aug = DeviceAugmenter.from_config(p, [0, -40, -3, 70.4, 40, 1], database=d)
    assert aug.sampler.database is d and aug.sampler.groups == [("Car", 15)] and aug.sampler.sample_importance == 0.25
    assert aug.sampler.remove_points_after_sample is False
    assert DeviceAugmenter.from_config(p, [0, -40, -3, 70.4, 40, 1]).sampler is None


@pytest.mark.parametrize("rate", [0.5, 0.7, 1.0])
def test_num_table_is_the_reference_rounding(rate):
    from second_amd.augment import DeviceDatabaseSampler, DeviceGtDatabase, sample_num_table
    groups = [("Car", 15), ("Pedestrian", 8), ("Cyclist", 3)]
    table = sample_num_table(groups, rate)
    assert table.shape == (3, 16) and table.dtype == np.int32
    for c, (_, m) in enumerate(groups):
        for n in range(16):
            want = np.round(rate * int(m - n)).astype(np.int64)             # second/core/sample_ops.py:107-109
            assert table[c, n] == max(int(want), 0), (c, n)
    if rate == 0.5:
        assert table[0, 14] == 0 and table[0, 12] == 2 and table[0, 10] == 2 and table[0, 0] == 8      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 7.5 -> 8
    d = DeviceGtDatabase.synthetic(0, ("Car", "Pedestrian", "Cyclist"), 6, device="cpu")
    s = DeviceDatabaseSampler(d, groups=groups, rate=rate)
    np.testing.assert_array_equal(s.num_table.numpy(), table)
    assert s.per_class == list(table[:, 0]) and s.k == table.max() and s.class_of_group.tolist() == [1, 2, 3]


def test_draw_cursor_remainder_pad_and_reshuffle():
    """BatchSampler._sample on the device permutation: K_c rows per frame; when cursor + K_c reaches the end, the remainder, -1
    behind it, and a fresh shuffle."""
    from second_amd.augment import DeviceDatabaseSampler, DeviceGtDatabase
    d = DeviceGtDatabase.synthetic(1, ("Car", "Van"), 10, device="cpu")
    s = DeviceDatabaseSampler(d, groups=[("Car", 4), ("Van", 5)], rate=1.0)
    assert s.per_class == [4, 5] and s.k == 5 and s.max_sampled_points == sum(sorted(d.point_counts[:10])[-4:]) + sum(sorted(d.point_counts[10:])[-5:])
    gen = torch.Generator().manual_seed(3)
    s.draw(gen, batch_size=1)
    car, van = s.perms[0].clone(), s.perms[1].clone()
    assert sorted(car.tolist()) == list(range(10)) and sorted(van.tolist()) == list(range(10, 20))
    assert s.candidates.shape == (1, 2, 5) and s.candidates.dtype == torch.int32
    assert s.candidates[0, 0].tolist() == car[:4].tolist() + [-1] and s.candidates[0, 1].tolist() == van[:5].tolist()
    store = s.candidates.data_ptr()
    s.draw(gen)
    assert s.candidates[0, 0].tolist() == car[4:8].tolist() + [-1]
    assert s.candidates[0, 1].tolist() == van[5:].tolist()                  # 5 + 5 >= 10: the remainder is all five, then a reshuffle
    assert s.cursors == [8, 0] and not torch.equal(s.perms[1], van)
    van = s.perms[1].clone()
    s.draw(gen)
    assert s.candidates[0, 0].tolist() == car[8:].tolist() + [-1, -1, -1]   # 8 + 4 >= 10: two left, padded
    assert s.cursors == [0, 5] and not torch.equal(s.perms[0], car) and s.candidates[0, 1].tolist() == van[:5].tolist()
    assert s.candidates.data_ptr() == store
    # a batch that crosses the end inside one draw
    car = s.perms[0].clone()
    s.draw(gen, batch_size=3)
    new = s.perms[0]
    assert s.candidates[:, 0].tolist() == [car[:4].tolist() + [-1], car[4:8].tolist() + [-1], car[8:].tolist() + [-1] * 3]
    assert s.cursors[0] == 0 and sorted(new.tolist()) == list(range(10))
    # same seed, same draws
    a = DeviceDatabaseSampler(d, groups=[("Car", 4)]).draw(torch.Generator().manual_seed(5), batch_size=4).candidates
    b = DeviceDatabaseSampler(d, groups=[("Car", 4)]).draw(torch.Generator().manual_seed(5), batch_size=4).candidates
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="batch_size"):
        DeviceDatabaseSampler(d, groups=[("Car", 4)]).draw()


def test_entry_points_validate_before_any_launch():
    """Status codes of include/second_hip.h decided on the host, no GPU needed."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)                       # non-NULL, never dereferenced: validation fails first

    def select(k=15, groups=1, accepted=one, count=one, per_group=one, out_boxes=one, cap=1000, offsets=one, cands=one, table=one):
        return l.sec_db_sample_select_f32(one, one, 10, 2, one, None, None, one, 40, cands, groups, k, one, table, 16, 1.0, accepted, count,
                                          per_group, out_boxes, cap, one, one, one, one, offsets, None)
    assert select(accepted=None) == -1 and select(count=None) == -1 and select(per_group=None) == -1
    assert select(out_boxes=None) == -1 and select(offsets=None) == -1      # NULL outputs
    assert select(cands=None) == -1 and select(table=None) == -1
    assert select(k=65) == -3 and select(groups=17, cap=100000) == -3       # more than 64 candidates / 16 groups
    assert select(k=64, groups=16, cap=10 + 2 * 16 * 64 - 1) == -1          # the merged boxes might not fit

    ws = l.sec_db_sample_merge_points_workspace_bytes
    assert ws(17000, 8, 15) >= 4 * (67 + 3 * 8 + 1 + 8 * 15) and ws(0, 1, 1) > 0
    assert ws(17000, 0, 15) == 0 and ws(17000, 8, 0) == 0 and ws(17000, 8, 16 * 64 + 1) == 0 and ws(-1, 8, 15) == 0

    def merge(pitch=4, slots=15, out=one, offsets=one, overflow=one, wsp=one, nbytes=1 << 20, accepted=one):
        return l.sec_db_sample_merge_points_f32(one, pitch, one, 17000, 8, one, one, one, one, 40, accepted, one, slots, out, 30000, offsets,
                                                overflow, wsp, nbytes, None)
    assert merge(out=None) == -1 and merge(offsets=None) == -1 and merge(overflow=None) == -1 and merge(wsp=None) == -1
    assert merge(accepted=None) == -1
    assert merge(pitch=2) == -3 and merge(slots=16 * 64 + 1) == -3
    assert merge(nbytes=ws(17000, 8, 15) - 1) == -2 and merge(nbytes=0) == -2          # workspace too small
