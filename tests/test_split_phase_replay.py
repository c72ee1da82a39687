"""The graph replay of the split-phase path (generic.py): its controller with fakes, and its segment boundaries on the device.

CPU part: generic.replay_segments decides by integers and callables only, so a dict plays the device -- a log of executed
iterations and a violation counter -- and the test states which iterations must have run, once each and in order.
GPU part: runs whose length ends inside, at and just past a 64-iteration segment equal the eager loop bit for bit, and a
rolled-back segment leaves the moment sums as the eager loop leaves them.
"""
import copy

import numpy as np
import pytest
import torch

from helpers import bits, make_dist
from glabcmcmc_amd import generic
from test_generic_path import BoxedModel, FixedDescriptor, ProtocolModel
from test_stream_independence import abs_gauss_model, proposals

LENGTHS = [9, 68, 69, 133]            # one partial segment; exactly one; one and an iteration; two and a tail


class FakeDevice:
    """state = {'log': [(iteration, rounds)], 'violations': count}; `need` says how many redraw rounds an iteration needs,
    `capture_fails_on` the capture calls (counted from 0) that return None"""

    def __init__(self, need=None, capture_fails_on=()):
        self.state = {"log": [], "violations": 0}
        self.saved = None
        self.need = need or {}
        self.capture_fails_on = set(capture_fails_on)
        self.captures, self.restores = [], 0

    def iteration(self, i, rounds):
        self.state["log"].append((i, rounds))
        if rounds < self.need.get(i, 0):
            self.state["violations"] += 1

    def capture(self, i, rounds):
        self.captures.append((i, rounds))
        self.state["violations"] = 0
        if len(self.captures) - 1 in self.capture_fails_on:
            self.state["log"].append(("half an iteration", i))      # a failed capture may have run part of an iteration
            return None
        self.iteration(i, rounds)
        dev = self

        class Graph:
            def replay(self):
                dev.iteration(dev.state["log"][-1][0] + 1, rounds)
        return Graph()

    def snapshot(self):
        self.saved = copy.deepcopy(self.state)

    def restore(self):
        self.restores += 1
        self.state = copy.deepcopy(self.saved)

    def run(self, num_ite, speculative=True, max_graph_rounds=32):
        """the controller from iteration 4 and the eager tail (every redraw round the iteration needs); returns the
        controller's (rounds, rolled_back_at, stayed_graph) and where the eager tail began"""
        nxt, rounds, rolled_back_at, stayed = generic.replay_segments(
            4, num_ite, self.capture, self.snapshot, self.restore, lambda: self.state["violations"], speculative,
            max_graph_rounds)
        for i in range(nxt, num_ite):
            self.iteration(i, 1 << 20)
        return rounds, rolled_back_at, stayed, nxt

    def iterations(self):
        return [i for i, _ in self.state["log"]]


@pytest.mark.parametrize("num_ite", LENGTHS)
def test_replay_controller_without_violations(num_ite):
    for speculative in (True, False):
        dev = FakeDevice()
        assert dev.run(num_ite, speculative) == (0, None, True, num_ite)
        assert dev.state["log"] == [(i, 0) for i in range(4, num_ite)]
        assert dev.captures == [(4, 0)] and dev.restores == 0


@pytest.mark.parametrize("num_ite", LENGTHS)
@pytest.mark.parametrize("at", [4, 67, 68])
def test_replay_controller_rolls_back_to_the_segment_start(num_ite, at):
    """an iteration that needs 3 redraw rounds: its segment is rolled back twice (0 -> 2 -> 4 rounds) and the run stays a
    graph; segments before it keep the rounds they ran with, segments after it run with 4"""
    dev = FakeDevice(need={at: 3})
    got = dev.run(num_ite)
    if at >= num_ite:                                                # the run ends before the iteration that needs them
        assert got == (0, None, True, num_ite) and dev.restores == 0
        return
    seg = 4 if at < 68 else 68
    assert got == (4, seg, True, num_ite)
    assert dev.state["log"] == [(i, 0 if i < seg else 4) for i in range(4, num_ite)]
    assert dev.captures == [(4, 0), (seg, 2), (seg, 4)] and dev.restores == 2
    # a non-speculative replay (no sentinel check in the graph) never reads the counter
    plain = FakeDevice(need={at: 3})
    assert plain.run(num_ite, speculative=False) == (0, None, True, num_ite) and plain.restores == 0


@pytest.mark.parametrize("num_ite", LENGTHS)
@pytest.mark.parametrize("at", [4, 67, 68])
def test_replay_controller_gives_up_above_max_graph_rounds(num_ite, at):
    """a need above max_graph_rounds: not a graph, the eager tail starts at the rolled-back iteration"""
    dev = FakeDevice(need={at: 40})
    got = dev.run(num_ite)
    if at >= num_ite:
        assert got == (0, None, True, num_ite)
        return
    seg = 4 if at < 68 else 68
    assert got[1:] == (seg, False, seg)
    assert dev.iterations() == list(range(4, num_ite))
    assert [r for _, r in dev.captures if r] == [2, 4, 8, 16, 32] and dev.restores == 6
    tight = FakeDevice(need={at: 40})
    assert tight.run(num_ite, max_graph_rounds=1)[1:] == (seg, False, seg) and tight.restores == 1
    assert tight.iterations() == list(range(4, num_ite))


@pytest.mark.parametrize("num_ite", LENGTHS)
def test_replay_controller_capture_that_fails(num_ite):
    """a capture that returns None -- on the first call, and after a roll-back: the state is restored, the rest is eager"""
    dev = FakeDevice(capture_fails_on=[0])
    assert dev.run(num_ite) == (0, None, False, 4)
    assert dev.iterations() == list(range(4, num_ite)) and dev.restores == 1
    dev = FakeDevice(need={5: 1}, capture_fails_on=[1])
    assert dev.run(num_ite) == (2, 4, False, 4)
    assert dev.iterations() == list(range(4, num_ite)) and dev.captures == [(4, 0), (4, 2)]
    assert dev.restores == 2                                         # the roll-back, and again behind the failed capture


# ----------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("num_ite", LENGTHS)
@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc"])
def test_hip_graph_segment_boundaries_equal_the_eager_loop(hip, algo, num_ite):
    """130 chains (no multiple of 64), d = 2, N = 3, a protocol-only Model: the replayed graph -- GLMCMC with the sentinel
    check on, GlobalMCMC -- and the eager loop give the same history and move counts, bit for bit"""
    import glabcmcmc_amd as g_
    n, d = 130, 2
    model = abs_gauss_model(d, 0.5)
    lp, ip = (FixedDescriptor(p) for p in proposals(d, "gauss"))
    rng = np.random.default_rng(11)
    theta0 = rng.uniform(1.0, 1.9, (n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236 * rng.standard_normal((n, d))).astype(np.float32)
    outs = {}
    for mode in ("auto", False):
        st = {}
        kw = dict(seed=9, verbose=False, graph=mode, state_out=st)
        if algo == "glmcmc":
            out = g_.GLMCMC(ProtocolModel(model), num_ite, torch.from_numpy(theta0), torch.from_numpy(y0), lp, None, 0.4, ip, 3,
                            **kw)
        else:
            out = g_.GlobalMCMC(ProtocolModel(model), num_ite, torch.from_numpy(theta0), torch.from_numpy(y0), ip, None, 0.4, lp,
                                **kw)
        assert st.get("graph", False) is (mode == "auto") and "graph_rolled_back_at" not in st
        outs[mode] = (out.numpy(), st["chains"].n_moves.cpu().numpy())
    assert outs["auto"][0].shape == (num_ite, n, d)
    assert np.array_equal(bits(outs["auto"][0]), bits(outs[False][0]))
    assert np.array_equal(outs["auto"][1], outs[False][1]) and outs[False][1].sum() > 0


@pytest.mark.gpu
def test_hip_graph_roll_back_restores_the_moment_sums(hip):
    """case (b) of test_hip_speculative_graph_replay_with_the_sentinel_check with stats: the segment that is rolled back has
    added to the moment sums, so they belong to the restored state -- the sums equal the eager loop's, bit for bit"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    rng = np.random.default_rng(3)
    n, T, d = 256, 150, 2
    bm = abs_gauss_model(d, 0.5)
    lp, _ = proposals(d, "uniform")
    ip = make_dist(("uniform", [0.9, 0.9], [2.0, 2.0])).descriptor()
    theta0 = rng.uniform(1.0, 1.9, (n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236 * rng.standard_normal((n, d))).astype(np.float32)
    got = {}
    for mode in ("auto", False):
        st = {}
        mom = engine.Moments(n, d, torch.device("cuda", 0))
        g_.GLMCMC(BoxedModel(bm), T + 1, torch.from_numpy(theta0), torch.from_numpy(y0), FixedDescriptor(lp), None, 0.3,
                  FixedDescriptor(ip), 3, seed=5, verbose=False, stats=mom, graph=mode, state_out=st)
        assert st.get("graph_rolled_back_at") == (4 if mode == "auto" else None)
        got[mode] = (mom.steps, [t.cpu().numpy() for t in (mom.sum_theta, mom.sum_outer, mom.sum_jump)])
    assert got["auto"][0] == got[False][0] == T
    for a, b in zip(got["auto"][1], got[False][1]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.abs(b).sum() > 0
