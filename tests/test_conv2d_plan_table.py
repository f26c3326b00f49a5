"""The dispatch of the dense conv2d forward, pinned: ``sec_conv2d_fwd_plan_name`` of the built library must answer
tests/golden/conv2d_plan_table.json (recorded by tests/golden/make_conv2d_plan_table.py) entry for entry, under each setting of
SEC_CONV2D_PATCH / SEC_CONV2D_MFMA (one child process per setting: the switches are read once).  Host-only: no GPU."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_conv2d_plan_table_is_unchanged():
    from second_amd import runtime as rt
    spec = importlib.util.spec_from_file_location("make_conv2d_plan_table", os.path.join(GOLDEN, "make_conv2d_plan_table.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(GOLDEN, "conv2d_plan_table.json")) as f:
        t = json.load(f)
    # the grid the table was recorded on is the recorder's
    assert (t["layers"], t["maps"], t["dtype"], t["call_form"], t["env"]) == (rec.LAYERS, rec.MAPS, rec.DTYPES, rec.FORMS, rec.ENVS)
    grid = list(rec.grid())
    assert len(grid) == 20 * 27 * 3 * 8 and len(t["plans"]) == 3
    rt.lib()                                    # built and loadable
    got = rec.record(rt.LIB_PATH)
    for env, plans, names in zip(t["env"], t["plans"], got):
        want = [t["names"][int(i)] for i in plans.split()]
        assert len(want) == len(names) == len(grid)
        diff = [(q, w, g) for q, w, g in zip(grid, want, names) if w != g]
        assert not diff, "%s: %d of %d names differ; first (batch, h, w, cin, cout, ksize, stride, pad, dtype, form), want, got: %s" % (
            env, len(diff), len(want), diff[:8])
        fp32 = [g for q, g in zip(grid, names) if q[8] == 0]
        assert fp32 and not any(fp32)           # SEC_F32: no 16-bit kernel
