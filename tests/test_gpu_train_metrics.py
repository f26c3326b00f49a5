"""sec_train_metrics_f32 / second_amd.train_metrics on the MI355X against tests/golden/train_metrics.npz (recorded from the
reference's VoxelNet.update_metrics) -- BIT-equal: the decisions are integer counts (the fixture keeps every sigmoid 2^-20 from a
threshold, fp32 sigmoids differ from the exact value by ~2^-23), and the state arithmetic is the reference's fp32 operations in
its order on those integers, so there is no error to bound.  Where no fixture exists (a tied maximum, the grid-stride size, an odd
class count) the yardstick is the numpy restatement that tests/test_train_metrics_host.py holds to the fixture exactly."""
import ctypes

import numpy as np
import pytest
import torch

import train_metrics_helpers as H

pytestmark = pytest.mark.gpu
CASES = ("A", "B", "C", "D", "E", "F", "G")


@pytest.fixture(scope="module")
def fixture():
    return H.load_fixture()[1]


def dev_args(u, explicit_cared=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cared = u["cared"] if u["cared"] is not None else (u["labels"] >= 0 if explicit_cared else None)
    return (torch.tensor(u["cls_loss"]).cuda(), torch.tensor(u["loc_loss"]).cuda(), t(u["logits"]), t(u["labels"]),
            None if cared is None else t(cared))


def state_of(m):
    return np.concatenate([s.cpu().numpy().reshape(-1) for s in m.state()])


@pytest.mark.parametrize("name", CASES)
def test_fixture_sequences_are_bit_equal(fixture, name):
    """All ten state buffers and every returned float after every update; ``cared`` given and, where it is labels >= 0, left out."""
    from second_amd.train_metrics import DeviceTrainMetrics
    c = fixture[name]
    forms = (True,) if c["updates"][0]["cared"] is not None else (True, False)
    for explicit in forms:
        m = DeviceTrainMetrics(thresholds=c["thresholds"])
        for k, u in enumerate(c["updates"]):
            ret = m.update(*dev_args(u, explicit))
            got, want = state_of(m), u["state"]
            print(name, "cared given" if explicit else "cared = labels >= 0", "update", k, "state", got, "want", want)
            assert H.same(got, want), (name, k, explicit)
            assert H.same(H.ret_vector(ret, c["thresholds"]), u["ret"]), (name, k, explicit, ret)


def test_tied_maximum_takes_the_lowest_index():
    """Hand-built: the rule is torch.max's on the CPU (lowest index of the maximum), checked against counts written out by hand."""
    from second_amd.train_metrics import DeviceTrainMetrics
    rows = np.float32([[1, 3, 3, 0],        # tie of classes 2, 3 -> 2
                       [1, 3, 3, 0],
                       [2, 2, 2, 2],        # all four -> 1
                       [2, 2, 2, 2],
                       [-1, 0.5, -1, 0.5],  # 2, 4 -> 2
                       [-1, 0.5, -1, 0.5],
                       [-4, -4, -4, -4],    # tied below the threshold: nothing predicted
                       [-np.inf, -np.inf, -np.inf, -np.inf]])
    labels = np.int32([2, 3, 1, 4, 2, 4, 0, 0])
    want_matches = 1 + 0 + 1 + 0 + 1 + 0 + 1 + 1
    logits = np.tile(rows, (2, 40, 1)).reshape(2, 320, 4)          # [B, N, C]: more than one workgroup
    lab = np.tile(labels, 80).reshape(2, 320)
    m = DeviceTrainMetrics(thresholds=[0.5])
    ret = m.update(torch.tensor(0.5).cuda(), torch.tensor(0.25).cuda(), torch.from_numpy(logits).cuda(), torch.from_numpy(lab).cuda())
    s = dict(zip(H.STATE, m.state()))
    assert s["acc_total"].item() == want_matches * 80 and s["acc_count"].item() == 640
    assert ret["rpn_acc"] == float(np.float32(want_matches * 80) / np.float32(640))
    # six of the eight rows are positives above 0.5, two are negatives below it
    assert s["rec_total"].item() == s["rec_count"].item() == s["prec_total"].item() == s["prec_count"].item() == 6 * 80
    mine = H.zero_state(1)
    H.restate(mine, 0.5, 0.25, logits, lab, None, [0.5])
    assert H.same(state_of(m), H.state_vector(mine))


@pytest.mark.parametrize("total, c", [(2048 * 256 + 300, 1), (70001, 3)])
def test_grid_stride_and_odd_class_count_against_the_restatement(total, c):
    """More anchors than 2048 workgroups hold (the kernel strides), and a class count that is neither 1 nor even."""
    from second_amd.train_metrics import DeviceTrainMetrics
    rng = np.random.default_rng(total)
    x = rng.normal(0, 2, (1, total, c)).astype(np.float32)
    thr = H.DEFAULT_THRESHOLDS
    near = (np.abs(H.sigmoid64(x)[..., None] - np.array([np.float64(np.float32(t)) for t in thr])) < H.MARGIN).any(-1)
    x[near] += np.float32(0.01)                                    # admission as for the fixture
    if c > 1:
        srt = np.sort(x, -1)
        assert (srt[..., -1] > srt[..., -2]).all()                 # no tied maximum
    lab = rng.choice(np.arange(-1, c + 1), size=(1, total), p=[0.1, 0.85] + [0.05 / c] * c).astype(np.int64)
    m = DeviceTrainMetrics()
    mine = H.zero_state(len(thr))
    for k in range(2):
        ret = m.update(torch.tensor(0.5).cuda(), torch.tensor(0.0).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda())
        want = H.restate(mine, 0.5, 0.0, x, lab, None, thr)
        assert H.same(state_of(m), H.state_vector(mine)), k
        assert H.same(H.ret_vector(ret, thr), H.ret_vector(want, thr)), k


def test_from_net_shares_the_networks_buffers_with_its_own_method(fixture):
    """Three device updates on the stand-in VoxelNet's buffers, then ONE call of the network's own method (the torch formulation the
    host test pins to the reference) continues the same totals, and clear_metrics() zeroes what the device form sees."""
    from reference_standin import build_voxelnet
    from second_amd.models import CAR_FHD
    from second_amd.train_metrics import DeviceTrainMetrics
    c = fixture["A"]
    net = H.attach_metrics(build_voxelnet(CAR_FHD)).cuda()
    m = DeviceTrainMetrics.from_net(net)
    assert m.thresholds == c["thresholds"] and all(a is b for a, b in zip(m.state(), H.net_state(net).values()))
    for u in c["updates"]:
        ret = m.update(*dev_args(u))
    assert H.same(state_of(m), c["updates"][2]["state"]) and H.same(H.ret_vector(ret, c["thresholds"]), c["updates"][2]["ret"])
    assert H.same(H.state_vector({k: v.cpu().numpy() for k, v in H.net_state(net).items()}), c["updates"][2]["state"])
    assert "rpn_acc.total" in net.state_dict() and net.state_dict()["rpn_acc.total"].item() == c["updates"][2]["state"][0]
    # the fourth update by the network's own method == four updates of the restatement
    mine = H.split_state(c["updates"][2]["state"].copy(), len(c["thresholds"]))
    u = c["updates"][0]
    want = H.restate(mine, u["cls_loss"], u["loc_loss"], u["logits"], u["labels"], None, c["thresholds"])
    ret = net.update_metrics(*dev_args(u))
    assert H.same(state_of(m), H.state_vector(mine)) and H.same(H.ret_vector(ret, c["thresholds"]), H.ret_vector(want, c["thresholds"]))
    net.clear_metrics()
    assert not state_of(m).any()
    ret = m.update(*dev_args(u))                                   # and starts over
    assert H.same(state_of(m), u["state"]) and H.same(H.ret_vector(ret, c["thresholds"]), u["ret"])


def test_hook_serves_gpu_calls_and_counts_what_it_hands_back(fixture):
    from second_amd import train_metrics as TM
    c = fixture["D"]
    net = H.holder(c["C"], c["thresholds"]).cuda()
    stats = {}
    TM.install(net, stats)
    for u in c["updates"]:
        ret = net.update_metrics(*dev_args(u))
        assert H.same(H.ret_vector(ret, c["thresholds"]), u["ret"])
    assert stats["train_metrics_calls"] == 3 and stats["train_metrics_fallbacks"] == 0 and getattr(net, "standin_calls", 0) == 0
    assert H.same(H.state_vector({k: v.cpu().numpy() for k, v in H.net_state(net).items()}), c["updates"][2]["state"])
    a = dev_args(c["updates"][0])
    net.update_metrics(a[0], a[1], a[2].half(), a[3], a[4])        # the reference takes this sigmoid in fp16: its own method serves it
    assert stats["train_metrics_fallbacks"] == 1 and "torch.float16" in stats["train_metrics_fallback_reason"] and net.standin_calls == 1


def test_accumulate_captures_into_two_kernel_nodes_and_replays(fixture):
    """accumulate under runtime.capture_guard(): two nodes (no memset, no copy), three replays over changing static inputs == three
    eager updates."""
    from second_amd import runtime as rt
    from second_amd.train_metrics import DeviceTrainMetrics
    c = fixture["C"]
    static = list(dev_args(c["updates"][0]))
    m = DeviceTrainMetrics(thresholds=c["thresholds"])
    m.accumulate(*static)                                          # warm-up: library load, buffers
    m.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with rt.capture_guard(), torch.cuda.graph(graph):
        m.accumulate(*static)
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0 and n.value == 2, n.value
    graph.instantiate()
    assert not state_of(m).any()                                   # capturing ran nothing
    for k, u in enumerate(c["updates"]):
        for dst, src in zip(static, dev_args(u)):
            dst.copy_(src)
        graph.replay()
        assert H.same(state_of(m), u["state"]), k
        assert H.same(H.ret_vector(m.read(), c["thresholds"]), u["ret"]), k


def test_two_calls_without_a_read_leave_the_counters_clean(fixture):
    from second_amd.train_metrics import DeviceTrainMetrics
    c = fixture["A"]
    m = DeviceTrainMetrics(thresholds=c["thresholds"])
    m.accumulate(*dev_args(c["updates"][0]))
    m.accumulate(*dev_args(c["updates"][1]))
    assert H.same(state_of(m), c["updates"][1]["state"]) and H.same(H.ret_vector(m.read(), c["thresholds"]), c["updates"][1]["ret"])
    assert not m._ws.cpu().numpy().any()
