"""The routing of the refine calls (csrc/call_plan.h + csrc/call_host.h) tied to the drivers on the GPU, at the smallest shape that
still has a ragged tile (17 x 33, max_pairs = 8): a fixed script of queued calls of several kinds, and graph replay with fewer slots
than calls.  Every output is compared bit for bit with the same call run unqueued / plainly on a fresh engine, and the counters with
figures worked out by hand from the rules of include/tcsfm.h ("coalesced calls", "graph replay of repeated calls")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, MAX_PAIRS = 17, 33, 8


def _alone(kind, c, o):
    """the call on its own, unqueued, on a fresh engine -> its outputs"""
    from tightly_coupled_sfm_amd.engine import Engine
    e = Engine(H, W, MAX_PAIRS)
    if kind == "dense":
        pose, depth, _ = e.refine_dense_window(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], o)
        out = (pose.clone(), depth.clone())
    elif kind == "scale":
        pose, ls, _ = e.refine_window(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], o, log_scale=c["ls"])
        out = (pose.clone(), ls.clone())
    else:
        out = (e.refine_window(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], o)[0].clone(),)
    e.synchronize()
    e.close()
    return out


def test_queued_script_bits_and_counts():
    """coal_max = 3 on a handle of 8 pairs.  The script, and what the rules make of it (sequences / calls so far):
         1-3   pose 1 x 1 (A)             the third fills the queue: ONE sequence of three                                  1 / 3
         4     A                          waits
         5     A, w_dc changed (A')       other options: the waiting A runs alone, A' waits                                 2 / 4
         6-7   pose + scale 1 x 1         other options (refine): A' runs alone; the two wait                               3 / 5
         8-9   per-pair dense 1 x 1       never merged with pose calls: the two scale calls run as one sequence; two wait   4 / 7
         10    pose 1 x 2 (4 pairs)       the two dense calls run as one sequence; the call waits: a second one still fits  5 / 9
         11    pose 1 x 2                 a third would not fit max_pairs (2 S B x 3 = 12 > 8): the two run now             6 / 11
         12    pose 1 x 1, REFERENCE rule never merged: runs at once, a sequence of its own                                 7 / 12
         flush                            nothing waits: nothing runs                                                       7 / 12"""
    import test_gpu_coalesce as TC
    from tightly_coupled_sfm_amd import _lib
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    one = TC._calls(9, H, W, seed=210)
    two = TC._calls(2, H, W, S=2, seed=230)
    for c in two:
        c["K"] = one[0]["K"]
    o_a = default_opts(n_iters=2)
    o_b = default_opts(n_iters=2, w_dc=0.15)
    o_s = default_opts(n_iters=2, refine=_lib.REFINE_POSE_SCALE)
    o_d = default_opts(n_iters=2, min_depth=0.06, max_depth=2.67)
    o_r = default_opts(n_iters=2, window_rule=_lib.WINDOW_REFERENCE)
    for c in one[5:7]:
        c["ls"] = torch.full((2,), 0.02, device="cuda")
    script = [("pose", one[0], o_a), ("pose", one[1], o_a), ("pose", one[2], o_a), ("pose", one[3], o_a), ("pose", one[4], o_b),
              ("scale", one[5], o_s), ("scale", one[6], o_s), ("dense", one[7], o_d), ("dense", one[8], o_d),
              ("pose", two[0], o_a), ("pose", two[1], o_a), ("pose", one[0], o_r)]
    counts = [(0, 0), (0, 0), (1, 3), (1, 3), (2, 4), (3, 5), (3, 5), (4, 7), (4, 7), (5, 9), (6, 11), (7, 12)]
    want = [_alone(kind, c, o) for kind, c, o in script]
    torch.cuda.synchronize()

    e = Engine(H, W, MAX_PAIRS)
    e.set_coalesce(3)
    got = []
    for (kind, c, o), n in zip(script, counts):
        pose_out = torch.zeros_like(c["pose"])
        if kind == "dense":
            depth_out = torch.zeros(c["pose"].shape[0], 1, H, W, device="cuda")
            e.refine_dense_window_queued(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], pose_out, depth_out, o)
            got.append((pose_out, depth_out))
        elif kind == "scale":
            ls_out = torch.zeros_like(c["ls"])
            e.refine_window_scale_queued(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], c["ls"], pose_out, ls_out, o)
            got.append((pose_out, ls_out))
        else:
            e.refine_window_queued(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], pose_out, o)
            got.append((pose_out,))
        assert e.coalesce_counts() == n, (len(got), e.coalesce_counts(), n)
    e.flush()
    assert e.coalesce_counts() == (7, 12)
    e.synchronize()
    for i, (g, w_) in enumerate(zip(got, want)):
        for a, b in zip(g, w_):
            assert torch.equal(a, b), (i, script[i][0])
    e.close()


def test_graph_replay_two_slots_three_calls():
    """Two slots, three distinct calls X Y Z on the handle's own stream.  Cycled three times, every sighting finds its call evicted: the
    least recently used of two entries is always the call that comes next but one, so nothing is ever seen twice -- no capture, no replay.
    Then Z Z Z: Z was the last to be seen, so it is captured (its second sighting), replayed, replayed; X evicts Y (Z was used later), Z is
    replayed; Y evicts X, Z is replayed: one capture, four replays.  Every output is the plain run's, bit for bit."""
    import test_gpu_coalesce as TC
    from tightly_coupled_sfm_amd.engine import Engine, default_opts
    calls = TC._calls(3, H, W, seed=250)
    o = default_opts(n_iters=2)
    plain = Engine(H, W, MAX_PAIRS)
    want = [plain.refine_window(c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], o)[0].clone() for c in calls]
    plain.synchronize()
    plain.close()

    e = Engine(H, W, MAX_PAIRS)
    e.use_own_stream()            # (a capture needs a stream of its own, not the default stream)
    e.set_graph_replay(2)
    outs = [torch.zeros_like(c["pose"]) for c in calls]
    torch.cuda.synchronize()
    order = [0, 1, 2] * 3 + [2, 2, 2, 0, 2, 1, 2]
    figures = [(0, 0)] * 10 + [(1, 0), (1, 1), (1, 2), (1, 2), (1, 3), (1, 3), (1, 4)]
    assert e.graph_replay_counts() == figures[0]
    for i, n in zip(order, figures[1:]):
        c = calls[i]
        outs[i].zero_()
        torch.cuda.synchronize()
        e.refine_window_async(0, c["tgt"], c["srcs"], c["dt"], c["ds"], c["K"], c["pose"], outs[i], o)
        e.synchronize()
        assert e.graph_replay_counts() == n, (i, e.graph_replay_counts(), n)
        assert torch.equal(outs[i], want[i]), i
    e.set_graph_replay(0)
    e.close()
