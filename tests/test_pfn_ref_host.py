"""CPU proof that the comparison of tests/test_gpu_pfn_edges.py bites (tests/pfn_ref_helpers.py): the float64 references agree with
the executed reference (fixtures recorded from its own modules), a float32 emulation of each kernel's arithmetic passes every
comparison, each planted mistake fails it, every generator delivers what it claims, the exact cases are exact, and the measured
4x constants are printed so that a change in them is visible without a GPU."""
import numpy as np
import pytest
import torch

import pfn_ref_helpers as H


def _folded(g, prefix="pfn_sd.pfn_layers.0."):
    w = g[prefix + "linear.weight"]
    bw, bb, rm, rv = [g[prefix + "norm." + k].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var")]
    scale = bw / np.sqrt(rv + 1e-3)
    return w, scale, bb - rm * scale


# ---- the references against the executed reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,radius", [("torch_modules", False), ("mhead", True)])
def test_eval_reference_matches_the_reference_module(golden, fixture, radius):
    g = golden(fixture)
    w, scale, shift = _folded(g)
    assert w.shape[1] == (8 if radius else 9)
    case = dict(vox=g["pfn_voxels"], num=g["pfn_num_points"], coords=g["pfn_coords"], geom=H.GEOM, wt=w.T.copy(), scale=scale, shift=shift)
    ref, bound = H.eval64(case, radius)
    np.testing.assert_allclose(ref, g["pfn_out"], rtol=3e-6, atol=3e-6)               # the reference ran in float32
    # its float32 result, with float32-folded parameters, also sits inside the per-element bound (plus the folding's own rounding)
    case32 = dict(case, scale=scale.astype(np.float32), shift=shift.astype(np.float32))
    assert H.check_eval(H.emulate32(case32, radius, "eval"), case32, radius, "fp32") <= 1.0


def _train_fixture(g):
    c = g["linear_weight"].shape[0]
    vs, rg = g["voxel_size"], g["pc_range"]
    geom = (vs[0], vs[1], vs[0] / 2 + rg[0], vs[1] / 2 + rg[1])
    return dict(vox=g["voxels"], num=g["num_points"], coords=g["coords"], geom=geom, wt=g["linear_weight"].T.copy(), gamma=g["norm_weight"],
                beta=g["norm_bias"], eps=float(g["eps"]), momentum=float(g["momentum"]), rm0=np.zeros(c), rv0=np.ones(c), grad_out=g["w"])


@pytest.mark.parametrize("fixture,radius", [("pfn_train", False), ("mhead_train", True)])
def test_train_reference_matches_the_reference_layer_in_float64(golden, fixture, radius):
    g = golden(fixture)
    case = _train_fixture(g)
    ref = H.train64(case, radius)
    bw = H.backward64(ref, case, ref["argmax"], ref["out"] > 0, case["grad_out"])
    for k in ("out", "running_mean", "running_var"):
        np.testing.assert_allclose(ref[k], g[k], rtol=1e-11, atol=1e-13, err_msg=k)
    for k in H.BWD_KEYS:
        np.testing.assert_allclose(bw[k], g[k], rtol=1e-9, atol=1e-12, err_msg=k)
    # and the recorded float64 results pass the shared comparison as a kernel's would
    got = dict(mean=ref["mean"], invstd=ref["invstd"], out=g["out"], argmax=ref["argmax"], running_mean=g["running_mean"],
               running_var=g["running_var"], d_linear_weight=g["d_linear_weight"], d_norm_weight=g["d_norm_weight"], d_norm_bias=g["d_norm_bias"])
    res = H.check_train(got, case, radius)
    assert max(res.values()) <= 1e-3, res


# ---- a float32 emulation passes, planted mistakes fail --------------------------------------------------------------------------
HOST_EVAL = [c for c in H.EVAL_CASES if c[0] * c[1] * c[2] <= 300000]
HOST_TRAIN = [c for c in H.TRAIN_CASES if c[0] * c[1] * c[2] <= 300000 or c[3] == "offset"]


@pytest.mark.parametrize("case_id", HOST_EVAL, ids=lambda c: "-".join(map(str, c)))
def test_float32_emulation_passes_every_eval_comparison(case_id):
    case = H.eval_case(*case_id)
    for radius in (False, True):
        out = H.emulate32(case, radius, "eval")
        for kind, dt in H.KINDS.items():
            r = H.check_eval(torch.from_numpy(out).to(dt), case, radius, kind)
            assert r <= 1.0, (radius, kind, r)


@pytest.mark.parametrize("case_id", HOST_TRAIN, ids=lambda c: "-".join(map(str, c)))
def test_float32_emulation_passes_every_train_comparison(case_id):
    p, t, c, variant, bias = case_id
    case = H.train_case(p, t, c, variant, bias=bias)
    for radius in (False, True):
        res = H.check_train(H.emulate32(case, radius, "train"), case, radius)
        print(case_id, radius, {k: f"{v:.2e}" for k, v in res.items()}, case[("consts", radius)])
        assert set(res) == set(H.FWD_KEYS + H.BWD_KEYS + ("argmax", "gate"))
        assert max(res.values()) <= 1.0, (radius, res)


def _planted_case():
    case = H.train_case(65, 9, 64, "plain", seed=5, bias=(0.5, 1.5))
    case.update(H.eval_case(65, 9, 64, "axis", "plain", seed=5) | dict(wt9=case["wt9"], vox=case["vox"], num=case["num"], coords=case["coords"]))
    return case


EVAL_BUGS = ("pad_out_of_max", "mean_div_T", "centre_col", "radius_x")
TRAIN_BUGS = {"pad_out_of_max": ("out", "argmax"), "n_live": ("mean", "invstd"), "mean_div_T": ("out",), "centre_col": ("out",),
              "unbiased_norm": ("invstd",), "gate_from_grad": ("d_norm_bias",), "no_s1": ("d_linear_weight",),
              "m_transposed": ("d_linear_weight",), "radius_x": ("out",), "rv_biased": ("running_var",)}


@pytest.mark.parametrize("bug", EVAL_BUGS)
def test_planted_mistakes_fail_the_eval_comparison(bug):
    case = _planted_case()
    for radius in ((True,) if bug == "radius_x" else (False, True)):
        assert H.check_eval(H.emulate32(case, radius, "eval"), case, radius, "fp32") <= 1.0
        for kind, dt in H.KINDS.items():
            r = H.check_eval(torch.from_numpy(H.emulate32(case, radius, "eval", bug)).to(dt), case, radius, kind)
            assert r > 1.0, (bug, radius, kind, r)


@pytest.mark.parametrize("bug", sorted(TRAIN_BUGS))
def test_planted_mistakes_fail_the_train_comparison(bug):
    case = _planted_case()
    for radius in ((True,) if bug == "radius_x" else (False, True)):
        res = H.check_train(H.emulate32(case, radius, "train", bug), case, radius)
        for k in TRAIN_BUGS[bug]:
            assert res.get(k, float("inf")) > 1.0, (bug, radius, k, res)


def test_ignored_live_count_fails_the_sentinel_check():
    case = _planted_case()
    case.update(num_dev=30, sentinel=np.float32(-7.5))
    good, bad = H.emulate32(case, False, "eval"), H.emulate32(case, False, "eval", "num_dev_ignored")
    assert bool((good[30:] == -7.5).all()) and not bool((bad[30:] == -7.5).all())
    assert H.check_eval(good[:30], {k: (v[:30] if k in ("vox", "num", "coords") else v) for k, v in case.items() if not isinstance(k, tuple)}, False, "fp32") <= 1.0


def test_scatter_restatement_and_its_clamp():
    feat, coords, batch, ny, nx = H.scatter_case(40, 5)
    full, half, over = (H.scatter64(feat, coords, batch, ny, nx, live) for live in (None, 20, 99))
    assert np.array_equal(full, over) and int((half != 0).sum()) == 20 * 5 and int((full != 0).sum()) == 40 * 5
    assert np.array_equal(H.gather64(full, coords), feat) and H.gather64(full, coords, 20).shape == (20, 5)
    assert not np.array_equal(half, full)                    # a scatter that ignores the live count fails a bit-equal comparison


# ---- the generators deliver what they claim -------------------------------------------------------------------------------------
def test_case_tables_cover_every_boundary():
    assert {c[1] for c in H.EVAL_CASES} >= set(H.EVAL_T) and {c[2] for c in H.EVAL_CASES} == set(H.EVAL_C)
    assert {c[0] for c in H.EVAL_CASES} == set(H.EVAL_P)
    assert {c[3] for c in H.EVAL_CASES} == set(H.POINT_SETS) and {c[4] for c in H.EVAL_CASES} == set(H.PARAM_SETS)
    shapes = {c[:3] for c in H.TRAIN_CASES}
    assert {(1, 2, 64), (33, 5, 64), (3, 127, 64), (700, 60, 64), (5000, 20, 64), (700, 60, 16), (33, 5, 16), (4100, 20, 64), (700, 60, 33)} <= shapes
    assert {c[3] for c in H.TRAIN_CASES} == {"plain", "full", "zero_weight", "gamma0", "pad_wins", "zero_grad_rows", "offset"}
    assert 4100 > 1024 * 4 >= 4096


def test_point_sets_have_their_properties():
    t = 9
    for kind in H.POINT_SETS:
        vox, num, coords = H.pillars(40, t, kind, seed=1)
        live = np.arange(t)[None, :] < num[:, None]
        assert not vox[~live].any() and num.min() >= 1 and num.max() <= t
        cen = -49.875 + coords[:, [3, 2]] * 0.25
        assert np.abs(vox[..., :2] - cen[:, None, :])[live & ~((vox[..., 0] == 0) & (vox[..., 1] == 0))].max() <= 0.125 + 1e-5 or kind == "duplicated"
        if kind == "centred":
            assert np.abs(vox[..., :2]).max() <= 3.0
        if kind in ("far", "intensity255", "full"):
            assert np.abs(vox[..., 0]).max() > 45 and np.abs(vox[..., 1]).max() > 45
        if kind == "far":
            assert abs(vox[-1, 0, 0]) > 49.7 and abs(vox[-1, 0, 1]) > 49.7
        if kind == "axis":
            assert vox[0, 0, 0] == 0 and vox[0, 0, 1] == 0 and num[0] == t
        if kind == "single":
            assert (num == 1).all()
            dec = H.decorate64(vox, num, coords, H.GEOM, False)[0]
            assert not dec[:, 0, 4:7].any()                                 # x - mean exactly 0
        if kind == "duplicated":
            assert all((vox[i, :num[i]] == vox[i, 0]).all() for i in range(40)) and num.max() > 1
        if kind == "intensity255":
            assert vox[..., 3].max() > 200
        if kind == "full":
            assert (num == t).all()
        else:
            assert kind == "single" or ((num == t).any() and (num < t).any() and num[1] == 1)


def test_parameter_sets_have_their_properties():
    for radius in (False, True):
        case = H.eval_case(33, 9, 64, "far", "negative_scale")
        assert (case["scale"][::3] < 0).all() and (case["scale"][1::3] > 0).all()
        case = H.eval_case(33, 9, 64, "far", "pad_wins")
        ref, _ = H.eval64(case, radius)
        live_only, _ = H.eval64(case, radius, pad_in_max=False)
        ragged = case["num"] < 9
        assert ragged.sum() > 3 and (ref[ragged, 0] == np.maximum(np.float64(case["shift"][0]), 0)).all() and (live_only[ragged, 0] < ref[ragged, 0]).all()
        case = H.eval_case(33, 9, 64, "far", "dead_channel")
        ref, _ = H.eval64(case, radius)
        assert (ref[:, 63] == 0).all() and (ref[:, :63] > 0).any()


def test_training_variants_have_their_properties():
    for radius in (False, True):
        case = H.train_case(33, 5, 64, "zero_weight")
        ref = H.train64(case, radius)
        assert ref["var"][0] == 0 and ref["invstd"][0] == 1 / np.sqrt(H.EPS) and (ref["var"][1:] > 0).all()
        case = H.train_case(33, 5, 64, "gamma0")
        ref = H.train64(case, radius)
        assert (ref["out"][:, 1] == max(float(case["beta"][1]), 0.0)).all()
        case = H.train_case(65, 9, 64, "pad_wins")
        ref = H.train64(case, radius)
        ragged = case["num"] < 9
        assert ragged.sum() > 10 and (ref["argmax"][ragged, 2] == -1).all() and (ref["out"][ragged, 2] > 0).all() and (ref["argmax"][~ragged] >= 0).all()
        case = H.train_case(33, 5, 64, "zero_grad_rows")
        assert not case["grad_out"][::3].any() and case["grad_out"][1::3].all()
        case = H.train_case(33, 8, 64, "full")
        assert (case["num"] == 8).all() and (H.train64(case, radius)["argmax"] >= 0).all()
        case = H.train_case(33, 5, 64, "plain", bias=(2.0, 4.0))
        ref = H.train64(case, radius)
        assert (ref["argmax"] == -1).any() and (ref["argmax"] >= 0).any()
    case = H.train_case(700, 32, 64, "offset")
    ref = H.train64(case, False)
    assert case["vox"][..., 0].min() >= 60 and case["vox"][..., 0].max() <= 70 and case["vox"][..., 3].min() >= 200 and (case["num"] == 32).all()
    assert np.count_nonzero(case["wt9"][:, 0]) == 1 and case["wt9"][0, 0] != 0 and np.count_nonzero(case["wt9"][:, 1]) == 1 and case["wt9"][3, 1] != 0
    ratio = ref["mean"] ** 2 / ref["var"]
    print("offset case mean^2 / var of channels 0, 1:", ratio[:2])
    assert ratio[0] > 300 and ratio[1] > 100                      # |mean| >> std: sum x^2 / N - mean^2 cancels
    case = H.train_case(3, 127, 64, "plain")
    assert (H.train64(case, False)["argmax"] == 126).any()        # the int8 argmax at its last slot


def test_one_pass_float32_variance_misses_the_invstd_bar_of_the_offset_case():
    """Suspicion 1 on the CPU: sum x and sum x^2 run in float32 (per 'wave' of rows, as k_pfn_stats accumulated them before its sums
    went to fp64) lose invstd far beyond four times what torch's float32 BatchNorm shows; fp64 sums of the same float32 rows keep it."""
    case = H.train_case(700, 32, 64, "offset")
    ref = H.train64(case, False)
    k4 = ref["consts"]
    dec = H.decorate64(case["vox"], case["num"], case["coords"], case["geom"], False)[0].astype(np.float32)
    x = (dec @ case["wt9"]).astype(np.float32).reshape(-1, 64)
    rows = x.shape[0]
    s, q = np.zeros(64, np.float32), np.zeros(64, np.float32)
    waves = x.reshape(700, 32, 64)
    parts = []
    for w in range(0, 700, 175):                                  # four 'waves' of 175 pillars, sequential float32 sums
        s[:], q[:] = 0, 0
        for pillar in waves[w:w + 175]:
            for row in pillar:
                s += row
                q += row * row
        parts.append((s.astype(np.float64), q.astype(np.float64)))
    mean = sum(p[0] for p in parts) / rows
    one_pass = 1 / np.sqrt(np.maximum(sum(p[1] for p in parts) / rows - mean ** 2, 0) + H.EPS)
    x64 = x.astype(np.float64)
    fixed = 1 / np.sqrt((x64 ** 2).sum(0) / rows - (x64.sum(0) / rows) ** 2 + H.EPS)
    e_old, e_new = np.abs(one_pass - ref["invstd"]) / ref["invstd"], np.abs(fixed - ref["invstd"]) / ref["invstd"]
    print("torch f32", k4["invstd"], "bar", 4 * k4["invstd"], "float32 one-pass", e_old[:2], e_old.max(), "fp64 sums", e_new[:2], e_new.max())
    assert e_old[:2].min() > 4 * k4["invstd"] and e_new.max() <= 4 * k4["invstd"]


def test_trimmed_slots_and_the_undecided_comparison():
    """What audit_pfn (train_step_audit_helpers.py) uses: the statistics of slot-trimmed pillars count the cut zero rows, and the
    comparison without the kernel's argmax passes the emulation and fails a planted mistake."""
    case = H.train_case(65, 30, 16, "plain", seed=2)
    case["num"] = np.minimum(case["num"], 7).astype(np.int32)
    case["vox"] = case["vox"] * (np.arange(30)[None, :] < case["num"][:, None])[..., None]
    small = H.trim_slots(case)
    assert small["vox"].shape[1] == 8 and small["slots"] == 30
    for radius in (False, True):
        a, b = H.train64(case, radius), H.train64(small, radius)
        for k in ("mean", "invstd", "out", "running_mean", "running_var", "argmax"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=1e-14, err_msg=k)
        got = H.emulate32(case, radius, "train")
        keep = {k: got[k] for k in ("out", "running_mean", "running_var") + H.BWD_KEYS}
        res = H.check_train_undecided(keep, small, radius)
        assert set(res) == {"out", "running_mean", "running_var", "gate"} | set(H.BWD_KEYS) and max(res.values()) <= 1.0, res
        bad = H.emulate32(case, radius, "train", "no_s1")
        assert H.check_train_undecided({k: bad[k] for k in keep}, H.trim_slots(case), radius)["d_linear_weight"] > 1.0


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def test_exact_eval_case_is_exact():
    case = H.exact_eval_case()
    assert set(np.unique(case["num"])) <= {1, 2, 4, 8} and (case["num"] == 8).any() and (case["num"] < 12).all()
    for radius in (False, True):
        ref, _ = H.eval64(case, radius)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and (ref > 0).any()
        assert np.array_equal(H.emulate32(case, radius, "eval").astype(np.float64), ref)
        dec = H.decorate64(case["vox"], case["num"], case["coords"], case["geom"], radius)[0]
        assert np.array_equal(dec.astype(np.float32).astype(np.float64), dec)
    r = np.sqrt(case["vox"][..., 0].astype(np.float64) ** 2 + case["vox"][..., 1].astype(np.float64) ** 2) * 8
    assert np.array_equal(r, np.round(r)) and (r == 0).any() and (r > 20).any()


@pytest.mark.parametrize("radius", [False, True])
def test_exact_train_cases_are_exact(radius):
    case = H.exact_train_fwd_case(radius)
    ref = H.train64(case, radius)
    assert (ref["var"] == 1).all() and (ref["invstd"] == 0.5).all()
    for k in ("mean", "out", "running_mean"):                     # running_var carries N / (N - 1), which no power-of-two N makes dyadic
        assert np.array_equal(ref[k].astype(np.float32).astype(np.float64), ref[k]), k
    assert len(np.unique(ref["mean"])) > 3 and (ref["out"] > 0).any() and (ref["out"] == 0).any() and len(np.unique(ref["argmax"])) > 2
    got = H.emulate32(case, radius, "train")
    for k in ("mean", "invstd", "out", "running_mean", "argmax"):
        assert np.array_equal(np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)), k
    assert np.array_equal(got["running_var"], ref["running_var"].astype(np.float32))          # one rounding of the float64 value
    b = H.exact_train_bwd_case(radius)
    k = 8 if radius else 9
    assert b["stats"].shape == (64 * (2 + k) + k,) and (b["argmax"] == -1).any() and (b["argmax"] > 0).any() and (b["out"] == 0).any()
    assert all(np.abs(v).max() > 0 for v in b["want"].values())
    m = b["stats"][128:128 + 64 * k].reshape(64, k)
    assert len(np.unique(m)) == m.size                             # distinct: a [K][C] read gives another dW


# ---- the measured constants -----------------------------------------------------------------------------------------------------
def test_measured_constants_are_printed_and_small():
    """Four times these (float32 torch formulation against float64, CPU) bound the accumulation of the statistics; DESIGN.md section 4
    records them.  A float32 BatchNorm that keeps a relative 1e-5 at these sizes is the order this holds torch to: beyond it the bound
    would be measuring a broken yardstick."""
    for cid in H.TRAIN_CASES:
        if cid[0] * cid[1] * cid[2] > 300000 and cid[3] != "offset":
            continue
        case = H.train_case(cid[0], cid[1], cid[2], cid[3], bias=cid[4])
        for radius in (False, True):
            k4 = H.torch_f32_constants(case, radius)
            print(cid, "radius" if radius else "nine", {k: f"{v:.2e}" for k, v in k4.items()})
            rows = cid[0] * cid[1]            # the variance of two rows is a difference of two nearly equal x: large relative to itself
            assert all(0 <= v < 1e-5 for k, v in k4.items() if k != "var" or rows >= 64), (cid, k4)
