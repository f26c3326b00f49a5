"""CPU side of the static-capacity PillarFeatureNet training kernels (sec_pfn_train_fwd_live / _bwd_live and their radius forms):
the float32 emulation of the kernels with a live count (tests/pfn_live_helpers.py) passes the comparisons of
tests/test_gpu_pfn_live.py -- the float64 reference of tests/pfn_ref_helpers.py on the live rows, bounds and decisions unchanged --
each planted mistake fails them, every generated garbage tail is in range, and the new entry points validate their arguments before
anything is launched."""
import ctypes

import numpy as np
import pytest

import pfn_live_helpers as L
import pfn_ref_helpers as H

HOST_TRAIN = [c for c in H.TRAIN_CASES if c[0] * c[1] * c[2] <= 300000 or c[3] == "offset"]       # the sizes tests/test_pfn_ref_host.py runs


def _ids(c):
    return "-".join(str(v) for v in c)


# ---- (a) the case table at a capacity above its pillar count --------------------------------------------------------------------
@pytest.mark.parametrize("case_id", HOST_TRAIN, ids=_ids)
def test_emulation_with_a_garbage_tail_passes_the_float64_comparison(case_id):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    cc = L.with_tail(case, p + 7)
    assert L.tail_is_in_range(cc, p)
    for radius in (False, True):
        res = L.check_live(L.emulate32_live(cc, p, radius), cc, p, radius, ref_case=case)
        assert set(res) == set(H.FWD_KEYS + H.BWD_KEYS + ("argmax", "gate", "tail"))
        assert max(res.values()) <= 1.0, (radius, res)


# ---- (b) count edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", L.C_EDGES)
@pytest.mark.parametrize("t", L.T_EDGES)
def test_emulation_passes_the_count_edges(t, c):
    for n in L.N_EDGES:
        case = L.edge_case(n, t, c) if n else L.empty_case(t, c)
        for cap in L.caps_of(n):
            cc = L.with_tail(case, cap)
            assert L.tail_is_in_range(cc, n) and cc["vox"].shape[0] == cap
            for radius in (False, True):
                res = L.check_live(L.emulate32_live(cc, n, radius), cc, n, radius, ref_case=case if n else None)
                assert max(res.values()) <= 1.0, (n, cap, radius, res)
    # a count above the capacity is the capacity, a negative one is zero
    full = L.edge_case(5, t, c)
    for radius in (False, True):
        a, b = L.emulate32_live(full, 5, radius), L.emulate32_live(full, 5 + 1000, radius)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        cc = L.with_tail(full, 12)
        a, b = L.emulate32_live(cc, 0, radius), L.emulate32_live(cc, -3, radius)
        assert all(np.array_equal(a[k], b[k]) for k in a) and max(L.check_live(b, cc, -3, radius).values()) == 0.0


def test_emulation_passes_above_the_grid_stride_threshold():
    """n = 4097 at capacity 4100 on slot-trimmed pillars (at most three points each; the zero rows that were cut count)."""
    t, c = 60, 33
    case = L.sparse_case(4097, t, c)
    cc = L.with_tail(case, L.BIG_CAP)
    assert L.tail_is_in_range(cc, 4097)
    small = H.trim_slots(case)
    assert small["vox"].shape[1] == 4 and small["slots"] == t
    for radius in (False, True):
        res = L.check_live(L.emulate32_live(cc, 4097, radius), cc, 4097, radius, ref_case=small)
        assert max(res.values()) <= 1.0, (radius, res)


# ---- planted mistakes -----------------------------------------------------------------------------------------------------------
def _planted():
    case = H.train_case(5, 9, 64, "plain", seed=5, bias=(0.5, 1.5))
    return case, L.with_tail(case, 12)


@pytest.mark.parametrize("bug", sorted(L.LIVE_BUGS))
def test_planted_mistakes_fail_the_comparison(bug):
    case, cc = _planted()
    for radius in (False, True):
        good = L.check_live(L.emulate32_live(cc, 5, radius), cc, 5, radius, ref_case=case)
        assert max(good.values()) <= 1.0, good
        res = L.check_live(L.emulate32_live(cc, 5, radius, bug), cc, 5, radius, ref_case=case)
        for k in L.LIVE_BUGS[bug]:
            assert res.get(k, float("inf")) > 1.0, (bug, radius, k, res)


def test_an_output_tail_left_alone_fails_the_tail_check():
    case, cc = _planted()
    got = L.emulate32_live(cc, 5, False)
    for k, v in (("out", 0.5), ("argmax", 0)):
        bad = dict(got, **{k: got[k].copy()})
        bad[k][7] = v
        assert L.check_live(bad, cc, 5, False, ref_case=case)["tail"] > 1.0


def test_dividing_by_no_rows_fails_the_empty_check():
    cc = L.with_tail(L.empty_case(9, 64), 8)
    assert L.tail_is_in_range(cc, 0)
    for radius in (False, True):
        assert max(L.check_live(L.emulate32_live(cc, 0, radius), cc, 0, radius).values()) == 0.0
        res = L.check_live(L.emulate32_live(cc, 0, radius, "zero_div"), cc, 0, radius)
        assert res["finite"] > 1.0 and res["gradients"] > 1.0 and res["running"] > 1.0, res


# ---- garbage tails --------------------------------------------------------------------------------------------------------------
def test_a_tail_out_of_range_is_recognised():
    """tail_is_in_range is asserted on every generated tail above; here it is shown to bite."""
    case, cc = _planted()
    assert L.tail_is_in_range(cc, 5)
    for k, i, v in (("num", 6, 10), ("num", 6, 0), ("coords", 6, -1), ("coords", 6, 100000), ("vox", 6, np.nan), ("grad_out", 6, np.inf),
                    ("vox", 6, 0.0)):
        bad = dict(cc, **{k: cc[k].copy()})
        bad[k][i] = v
        assert not L.tail_is_in_range(bad, 5), (k, v)
    moved = dict(cc, coords=cc["coords"].copy())
    moved["coords"][6] = [0, 0, 7, 7]                           # on the grid, but no live pillar's cell
    assert not L.tail_is_in_range(moved, 5)


# ---- host validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [False, True], ids=["nine", "radius"])
def test_live_entry_points_validate_before_any_launch(radius):
    """The status codes of sec_pfn_train_fwd / _bwd, decided on the host before anything is enqueued (no device is touched: the
    pointers are never dereferenced on these paths)."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)
    big = 1 << 30
    f_fwd = l.sec_pfn_radius_train_fwd_live if radius else l.sec_pfn_train_fwd_live
    f_bwd = l.sec_pfn_radius_train_bwd_live if radius else l.sec_pfn_train_bwd_live

    def fwd(t=60, f=4, c=64, wt=one, ga=one, be=one, out=one, arg=one, stats=one, ws=one, wsb=big, p=100, nd=one):
        return f_fwd(one, one, one, p, nd, t, f, wt, ga, be, 1e-3, 0.01, one, one, c, 0.25, 0.25, 0.0, 0.0, out, arg, stats, ws, wsb, None)

    def bwd(t=60, f=4, c=64, wt=one, ga=one, stats=one, g=one, out=one, arg=one, dw=one, dg=one, db=one, ws=one, wsb=big, p=100, nd=one):
        return f_bwd(one, one, one, p, nd, t, f, wt, ga, stats, c, 0.25, 0.25, 0.0, 0.0, g, out, arg, dw, dg, db, ws, wsb, None)
    for nd in (one, None):
        for name in ("wt", "ga", "be", "out", "arg", "stats"):
            assert fwd(nd=nd, **{name: None}) == -1, name                # SEC_E_INVALID
        for name in ("wt", "ga", "stats", "g", "out", "arg", "dw", "dg", "db"):
            assert bwd(nd=nd, **{name: None}) == -1, name
        assert fwd(nd=nd, t=128) == -1 and bwd(nd=nd, t=128) == -1 and fwd(nd=nd, t=0) == -1 and fwd(nd=nd, p=-1) == -1 and bwd(nd=nd, p=-1) == -1
        assert fwd(nd=nd, c=65) == -3 and bwd(nd=nd, c=65) == -3 and fwd(nd=nd, f=5) == -3 and bwd(nd=nd, f=5) == -3      # the limits, unchanged
        need = l.sec_pfn_train_workspace_bytes(100, 64)
        assert need > 0
        assert fwd(nd=nd, wsb=need - 1) == -2 and bwd(nd=nd, wsb=need - 1) == -2 and fwd(nd=nd, ws=None) == -2 and bwd(nd=nd, ws=None) == -2
        assert fwd(nd=nd, p=0, t=128) == -1 and fwd(nd=nd, p=0, c=65) == -3
    assert fwd(nd=None, p=0) == 0                                     # no count, no pillar: the no-op of the forms without a count


def test_header_and_bindings_declare_the_live_forms():
    import os
    import re
    from second_amd import runtime
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "second_hip.h")).read()
    for name in ("sec_pfn_train_fwd_live", "sec_pfn_train_bwd_live", "sec_pfn_radius_train_fwd_live", "sec_pfn_radius_train_bwd_live"):
        assert re.search(rf"\bint {name}\(", header) and name in runtime.SYMBOLS
        assert re.search(rf"int {name}\([^;]*int num_pillars, const int \*num_dev,\s+int max_points", header), name
    assert re.search(r"#define\s+SEC_ABI_VERSION\s+9\b", header) and runtime.ABI_VERSION == 9           # additions only
