"""One InFlightRunner step of car.lite (a 160 x 132 map: ragged against the 16-column tiles) with SEC_RPN_TILE_COVER=0 and =1, each in
its own process: the serving path follows the grid lists / the cover lists of the RPN, and the detections are equal element for
element."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _child(path):
    from second_amd import synthetic as syn
    from second_amd.models import CAR_LITE, InFlightRunner, SecondDetector
    torch.manual_seed(0)
    det = SecondDetector(CAR_LITE).cuda().eval()
    syn.randomise_like_trained(det)
    det.prepare_inference(torch.bfloat16)
    clouds = [syn.syn_kitti_cloud(s, num_points=6000, num_voxels=5000, point_cloud_range=tuple(CAR_LITE["point_cloud_range"]),
                                  voxel_size=tuple(CAR_LITE["voxel_size"])) for s in range(2)]
    pts, offs = syn.batch_clouds(clouds)
    pts, offs = torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda()
    with torch.no_grad():
        det.calibrate(pts, offs)
        runner = InFlightRunner(det, pts, offs, inflight=2, serialize_rpn=True)
        out, _ = runner.step()
        runner.synchronize()
    cover = det.rpn.last_cover_counts
    np.savez(path, cover=np.zeros(0) if cover is None else cover.cpu().numpy(), grid=det.rpn.last_live_counts.cpu().numpy(),
             **{k: v.float().cpu().numpy() if v.is_floating_point() else v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)})


def test_runner_step_with_cover_lists_gives_the_grid_lists_detections(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for mode in ("0", "1"):
        path = str(tmp_path / f"cover{mode}.npz")
        env = dict(os.environ, SEC_RPN_TILE_COVER=mode,
                   PYTHONPATH=os.pathsep.join([root, os.path.join(root, "second.pytorch_amd"), os.environ.get("PYTHONPATH", "")]))
        r = subprocess.run([sys.executable, __file__, "--runner-child", path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got[mode] = dict(np.load(path))
    assert got["0"]["cover"].size == 0 and got["1"]["cover"].size > 0, "SEC_RPN_TILE_COVER must select the form"
    convs = got["1"]["cover"].shape[0]                     # (the grid form asks for one layer more: the lazy heads' tile flags)
    np.testing.assert_array_equal(got["0"]["grid"][:convs], got["1"]["grid"][:convs])
    assert (got["1"]["cover"].sum(1) <= got["1"]["grid"][:convs].sum(1)).all()
    assert int(got["0"]["valid"].sum()) > 0
    m = got["0"]["valid"].astype(bool)
    np.testing.assert_array_equal(m, got["1"]["valid"].astype(bool))
    for k in got["0"]:                                     # (rows behind a frame's detections are unspecified)
        if k not in ("cover", "grid", "valid") and got["0"][k].shape[:2] == m.shape:
            np.testing.assert_array_equal(got["0"][k][m], got["1"][k][m], err_msg=k)


if __name__ == "__main__" and "--runner-child" in sys.argv:
    _child(sys.argv[sys.argv.index("--runner-child") + 1])
