"""CPU-only: the training-metrics fixture (tests/golden/train_metrics.npz, recorded from the reference's VoxelNet.update_metrics)
against the two restatements the GPU tests lean on, the hook's routing (second_amd.train_metrics.install) and the argument checks
sec_train_metrics_f32 makes before any launch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import train_metrics_helpers as H


@pytest.fixture(scope="module")
def fixture():
    return H.load_fixture()


def _args(u, device="cpu"):
    cared = (u["labels"] >= 0) if u["cared"] is None else u["cared"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return (torch.tensor(u["cls_loss"]).to(device), torch.tensor(u["loc_loss"]).to(device), t(u["logits"]), t(u["labels"]), t(cared))


def test_fixture_covers_what_it_has_to(fixture):
    meta, cases = fixture
    assert meta["replaced"] / meta["logits"] < 0.01 and meta["margin"] == 2.0 ** -20 and meta["state_order"] == list(H.STATE)
    assert {c["C"] for c in cases.values()} == {1, 2, 10} and {c["N"] for c in cases.values()} == {1, 255, 256, 257, 4099}
    assert {c["label_dtype"] for c in cases.values()} == {"int32", "int64"} and all(c["B"] == 2 and len(c["updates"]) >= 3 for c in cases.values())
    ups = [u for c in cases.values() for u in c["updates"]]
    assert any((u["labels"] == -1).all() for u in ups) and any(not (u["labels"] > 0).any() and (u["labels"] == 0).any() for u in ups)
    assert any(H.sigmoid64(u["logits"]).max() < 0.1 for u in ups)
    assert any(np.isnan(u["logits"]).any() for u in ups) and any((u["logits"].max(-1) == 0).any() for u in ups)
    first, later = [c["updates"][0] for c in cases.values()], [u for c in cases.values() for u in c["updates"][1:]]
    assert any(u["cls_loss"] == 0 and np.isnan(u["ret"][1]) for u in first) and any(u["cls_loss"] == 0 or u["loc_loss"] == 0 for u in later)
    # admission, re-derived from the stored logits: no float64 sigmoid within the margin of a threshold in use, bar the logits at 0
    for c in cases.values():
        thr = np.array([np.float64(np.float32(t)) for t in c["thresholds"]] + [0.5])
        for u in c["updates"]:
            x = u["logits"][~np.isnan(u["logits"]) & (u["logits"] != 0)]
            assert (np.abs(H.sigmoid64(x)[:, None] - thr) >= H.MARGIN).all()


def test_numpy_restatement_reproduces_the_fixture_exactly(fixture):
    _, cases = fixture
    for name, c in cases.items():
        thr = c["thresholds"]
        state = H.zero_state(len(thr))
        for k, u in enumerate(c["updates"]):
            ret = H.restate(state, u["cls_loss"], u["loc_loss"], u["logits"], u["labels"], u["cared"], thr)
            assert H.same(H.state_vector(state), u["state"]), (name, k)
            assert H.same(H.ret_vector(ret, thr), u["ret"]), (name, k)


def test_torch_standin_reproduces_the_fixture_exactly(fixture):
    """What the GPU tests and the probe call "the reference's own method" where no reference checkout exists."""
    _, cases = fixture
    for name, c in cases.items():
        net = H.holder(c["C"], c["thresholds"])
        for k, u in enumerate(c["updates"]):
            ret = net.update_metrics(*_args(u))
            got = H.state_vector({kk: v.numpy() for kk, v in H.net_state(net).items()})
            assert H.same(got, u["state"]) and H.same(H.ret_vector(ret, c["thresholds"]), u["ret"]), (name, k)
        net.clear_metrics()
        assert not H.state_vector({kk: v.numpy() for kk, v in H.net_state(net).items()}).any()


def test_hook_on_a_cpu_network_is_the_reference_and_counts_a_fallback(fixture):
    from second_amd import train_metrics as TM
    _, cases = fixture
    c = cases["D"]
    plain, hooked = H.holder(c["C"], c["thresholds"]), H.holder(c["C"], c["thresholds"])
    stats = {}
    dev = TM.install(hooked, stats)
    assert TM.install(hooked, stats) is dev and "update_metrics" in hooked.__dict__
    for k, u in enumerate(c["updates"]):
        a, b = plain.update_metrics(*_args(u)), hooked.update_metrics(*_args(u))
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
        assert H.same(H.ret_vector(b, c["thresholds"]), u["ret"])
        for kk, v in H.net_state(hooked).items():
            assert H.same(v.numpy(), H.net_state(plain)[kk].numpy()), kk
    assert stats["train_metrics_fallbacks"] == 3 and stats["train_metrics_calls"] == 0 and stats["train_metrics_fallback_reason"] == "CPU tensors"
    assert hooked.standin_calls == 3


def test_hook_sends_what_the_kernel_does_not_cover_to_the_original_method(fixture):
    from second_amd import train_metrics as TM
    _, cases = fixture
    c = cases["B"]
    u = c["updates"][2]

    def routed(edit, args=None):
        net = H.holder(c["C"], c["thresholds"])
        calls = []
        type(net).update_metrics = lambda self, *a: calls.append(a) or "original"      # the class's method: what the hook falls back to
        stats = {}
        TM.install(net, stats)
        edit(net)
        assert net.update_metrics(*(args or _args(u))) == "original" and len(calls) == 1
        assert stats["train_metrics_fallbacks"] == 1 and stats["train_metrics_calls"] == 0
        return stats["train_metrics_fallback_reason"]

    assert "background column" in routed(lambda n: setattr(n, "_encode_background_as_zeros", False))
    assert routed(lambda n: setattr(n.rpn_metrics, "_use_sigmoid_score", False)) == "softmax scores"
    a = _args(u)
    assert "sampled in torch.float32" in routed(lambda n: None, a[:4] + (a[4].float(),))
    assert "labels in torch.float32" in routed(lambda n: None, a[:3] + (a[3].float(), a[4]))


def test_argument_checks_come_before_any_launch():
    """Status codes of include/second_hip.h, decided on the host: no device is touched (the pointers are never dereferenced)."""
    from second_amd import ops, runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)
    state = (ctypes.c_void_p * 10)(*[4096] * 10)
    thr = rt.f_arr([0.5] * 17)
    ws = l.sec_train_metrics_workspace_bytes(7)
    assert ws >= (2 + 3 * 16) * 4 and l.sec_train_metrics_workspace_bytes(16) == ws and l.sec_train_metrics_workspace_bytes(17) == 0
    call = lambda n=1000, c=1, t=7, st=state, out=one, w=one, wb=ws: l.sec_train_metrics_f32(one, one, 0, None, n, c, thr, t, 0.5, one, one, st, out, w, wb, None)
    assert call(n=(1 << 24) + 1) == -3 and call(t=17) == -3                       # SEC_E_UNSUPPORTED
    assert call(c=0) == -1 and call(n=-1) == -1 and call(st=None) == -1 and call(out=None) == -1
    holed = (ctypes.c_void_p * 10)(*([4096] * 9 + [None]))
    assert call(st=holed) == -1                                                   # a NULL state pointer
    assert call(w=None) == -2 and call(wb=16) == -2                               # SEC_E_WORKSPACE
    assert ops.TRAIN_METRICS_MAX_ANCHORS == 1 << 24 and ops.TRAIN_METRICS_MAX_THRESHOLDS == 16
    from second_amd import train_metrics as TM
    with pytest.raises(ValueError):
        TM.DeviceTrainMetrics(thresholds=[0.5] * 17, device="cpu")


def test_unset_accelerate_model_leaves_update_metrics_alone(monkeypatch):
    from reference_standin import build_voxelnet
    from second_amd import compat
    from second_amd.models import CAR_FHD
    from second_amd import train_metrics as TM
    monkeypatch.delenv("SEC_TRAIN_METRICS", raising=False)
    net = H.attach_metrics(build_voxelnet(CAR_FHD))
    with monkeypatch.context() as m:                                  # unset: the new module is not even entered
        m.setattr(TM, "install", lambda *a, **k: pytest.fail("train_metrics.install called with SEC_TRAIN_METRICS unset"))
        assert compat.accelerate_model(net) is net and net._second_amd_engine is not None
    assert "update_metrics" not in net.__dict__ and net.update_metrics.__func__ is type(net).update_metrics
    assert not any(k.startswith("train_metrics") for k in net._second_amd_engine.stats)
    # asked for: shadowed on the instance, its counters in the engine's stats; the environment switch does the same
    compat.accelerate_model(net, train_metrics=True)
    assert "update_metrics" in net.__dict__ and net._second_amd_engine.stats["train_metrics_fallbacks"] == 0
    other = H.attach_metrics(build_voxelnet(CAR_FHD))
    monkeypatch.setenv("SEC_TRAIN_METRICS", "1")
    compat.accelerate_model(other)
    assert "update_metrics" in other.__dict__ and other._second_amd_original_update_metrics.__func__ is type(other).update_metrics
    bare = build_voxelnet(CAR_FHD)                                    # no metric modules: the environment route leaves it alone, the argument raises
    compat.accelerate_model(bare)
    assert "update_metrics" not in bare.__dict__
    with pytest.raises(AttributeError):
        compat.accelerate_model(bare, train_metrics=True)
