"""The dispatch of the sparse-conv forward, pinned: ``sec_indice_conv_fwd_plan`` of the built library must answer
tests/golden/conv_plan_table.json (recorded by tests/golden/make_conv_plan_table.py) entry for entry.  Host-only: no GPU."""
import itertools
import json
import os


def test_conv_plan_table_is_unchanged():
    from second_amd import runtime as rt
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")) as f:
        t = json.load(f)
    want = [int(t["plans"][i:i + 2]) for i in range(0, len(t["plans"]), 2)]
    grid = list(itertools.product(t["variants"], t["shapes"], t["kvol"], t["rows"], t["dtype"], t["out_f32"], t["has_packed"]))
    assert len(grid) == len(want) == 17 * 14 * 2 * 7 * 3 * 2 * 2
    lib = rt.lib()
    got, cur = [], None
    try:
        for v, (cin, cout), kvol, rows, dt, of32, packed in grid:
            if v != cur:
                lib.sec_indice_conv_set_variant(v)
                cur = v
            got.append(int(lib.sec_indice_conv_fwd_plan(cin, cout, kvol, rows, dt, 0 if of32 else dt, packed)))
    finally:
        lib.sec_indice_conv_set_variant(-1)
    diff = [(q, w, g) for q, w, g in zip(grid, want, got) if w != g]
    assert not diff, "%d of %d plans differ; first (variant, shape, kvol, rows, dtype, out_f32, packed), want, got: %s" % (
        len(diff), len(want), diff[:8])
