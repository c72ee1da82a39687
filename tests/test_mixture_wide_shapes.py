"""glabc_glmcmc_mix_wide_steps -- the GaussianMixture variant of the lane-group kernel (csrc/glabc_wide.h, batch sizes 17..4096)
-- against the split-phase reference chain of tests/test_mixture_shapes.py, bit for bit: per iteration
    oracle_propose -> the numpy restatement (tests/mixture_ref.py) fills theta' / log q' of the global candidates ->
    oracle_model_* -> q_cur from the restatement -> oracle_select
Compared: the history, the final theta / y / flags / n_moves, log_w on chains whose `local` flag is clear, the three moment sums.
The chain id offset is 2^32 + 7 (the high counter word is live).  65 chains leave a tail group at every L: three workgroups
with one live group in the last at L = 8, seventeen workgroups of four groups at L = 64.

Shapes are the smallest at which each mechanism can go wrong: every instantiation (theta_dim 1..4 and g-and-k x L), the edges of
torch.sum's tree (n = N + 1 = 18, 24, 32, 34), one and several candidates per lane (the winner by shuffle or re-evaluated), the
default lanes at the batch sizes where they change, batch sizes whose LDS rows need the 48 KiB grant lifted, K = 1 / 8 modes, a
Uniform local increment and prior.  Each comparison first asks of the reference chain alone that it is worth comparing against:
every mode drawn within the first four steps, a chain moved, and, from 6 steps on, chains ending on either branch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import bits
from test_arg_checks import ARG
from test_mixture_shapes import CHAIN0, GF, K_LAUNCH, SEED, assert_equals_reference, case, reference
from glabcmcmc_amd import _capi as A

N65 = 65


def wide_run(kind, d, N, K, local="gauss", prior="gauss", n=N65, steps=8, debug_flags=0, lanes=0, cut=None):
    from glabcmcmc_amd import engine
    model_o, lp_o, mix_o, theta0, y0 = case(kind, d, K, local, prior, n)
    model, lp, mix = model_o.descriptor(), lp_o.descriptor(), mix_o.descriptor()
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
    engine.init_weights(model, mix, chains)
    hist = torch.empty(steps, chains.d, chains.n, dtype=torch.float32, device=dev)
    mom = engine.Moments(chains.n, chains.d, dev)
    engine.run_steps("glabc_glmcmc_mix_wide_steps", model, lp, mix, chains, steps, 1, SEED, GF, N, history=hist, moments=mom,
                     steps_per_launch=cut, debug_flags=debug_flags, lanes_per_chain=lanes)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), chains, mom


def wide_reference(oracle, kind, d, N, K, local="gauss", prior="gauss", n=N65, steps=8):
    """the shared reference chain, and what keeps a comparison against it from passing vacuously"""
    want = reference(oracle, "glmcmc", kind, d, N, K, local, prior, n, steps)
    hh, hc, hm, modes = want
    what = (kind, d, N, K, local, prior, n, steps)
    assert np.isfinite(hh).all(), what
    assert modes == K, "%s: %d of %d modes drawn in the first four steps" % (what, modes, K)
    assert int((hc.n_moves > 0).sum()) >= 1, what
    if steps >= 6:
        local_set = (hc.flags & A.FLAG_LOCAL) != 0
        assert local_set.any() and not local_set.all(), what
    return want


def check(oracle, kind, d, N, K, lanes=0, **kw):
    run_kw = {k: kw.pop(k) for k in ("debug_flags", "cut") if k in kw}
    want = wide_reference(oracle, kind, d, N, K, **kw)
    got = wide_run(kind, d, N, K, lanes=lanes, **run_kw, **kw)
    assert_equals_reference(got, want, (kind, d, N, K, lanes, kw), True)
    return got


# ---- every instantiation ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [8, 16, 32, 64])
@pytest.mark.parametrize("kind,d", [("abs", 1), ("abs", 2), ("abs", 3), ("abs", 4), ("gk", 4)])
def test_hip_mixture_wide_every_instantiation(hip, oracle, kind, d, L):
    """wide_kernel<D, YD, L, false, true>: N = 17 is one candidate per lane at L = 32 / 64 and up to three at L = 8"""
    check(oracle, kind, d, 17, 3, lanes=L)


# ---- the total ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 23, 31, 33])
def test_hip_mixture_wide_row_sum_tree_edges(hip, oracle, N):
    """n = N + 1 = 18 (two vectors, no full group of four), 24, 32 (the first full group), 34"""
    check(oracle, "abs", 2, N, 3, lanes=8)


# ---- the winner ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,N", [(32, 17), (64, 64), (64, 65), (8, 17)])
def test_hip_mixture_wide_winner_by_shuffle_and_by_re_evaluation(hip, oracle, L, N):
    """N <= L: the winner comes from its owner's registers; otherwise every lane draws and evaluates it again"""
    check(oracle, "abs", 2, N, 3, lanes=L)


# ---- the library's own lanes ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,d,N,K,steps", [("abs", 2, 64, 3, 8), ("abs", 3, 65, 8, 8), ("abs", 1, 128, 2, 8), ("abs", 4, 129, 4, 6),
                                              ("abs", 2, 256, 3, 4), ("gk", 4, 257, 3, 4)])
def test_hip_mixture_wide_default_lanes(hip, oracle, kind, d, N, K, steps):
    """lanes_per_chain = 0: wide_default_lanes picks 8, 16, 16, 32, 32, 64"""
    check(oracle, kind, d, N, K, steps=steps)


@pytest.mark.gpu
@pytest.mark.parametrize("N,n,steps", [(1200, 33, 3), (4096, 9, 2)])
def test_hip_mixture_wide_large_batches_and_the_lds_grant(hip, oracle, N, n, steps):
    """default L = 64: 19.7 KB of group rows at N = 1200; 66 KB at N = 4096, more than a kernel gets without the grant"""
    check(oracle, "abs", 2, N, 3, n=n, steps=steps)


# ---- mode counts and branches ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,d,N,K", [("abs", 3, 65, 1), ("abs", 3, 65, 8), ("gk", 4, 17, 8)])
def test_hip_mixture_wide_mode_counts(hip, oracle, kind, d, N, K):
    check(oracle, kind, d, N, K)


@pytest.mark.gpu
def test_hip_mixture_wide_uniform_local_and_prior(hip, oracle):
    """a Uniform local increment turns its words into uniforms; the mixture reads the same words as normals"""
    check(oracle, "abs", 1, 33, 2, local="uniform", prior="uniform")
    check(oracle, "abs", 1, 33, 2)


# ---- geometry is only geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_mixture_wide_geometry_does_not_change_a_bit(hip, oracle):
    """one fixture at every L, and with the reference's sequential index search forced: 96 chains, 60 steps, launches cut every 13"""
    kw = dict(n=96, steps=60)
    runs = [check(oracle, "abs", 2, 65, 3, lanes=L, cut=K_LAUNCH, **kw) for L in (8, 16, 32, 64)]
    runs.append(check(oracle, "abs", 2, 65, 3, debug_flags=A.DEBUG_EXACT_INDEX, cut=K_LAUNCH, **kw))
    first = runs[0]
    for other in runs[1:]:
        assert np.array_equal(bits(first[0]), bits(other[0]))
        assert np.array_equal(bits(first[1].log_w.cpu().numpy()), bits(other[1].log_w.cpu().numpy()))      # every chain, stale ones too
        assert np.array_equal(first[2].sum_outer.cpu().numpy().view(np.uint64), other[2].sum_outer.cpu().numpy().view(np.uint64))


# ---- package level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_mixture_wide_through_the_package(hip, oracle, tmp_path):
    """MCMCRunner.run_glmcmc with a GaussianMixture at batch_size 32: path='auto' runs the lane-group kernel -- the bits of the
    direct C call with the same seed; path='generic' still runs; one chain in, one chain out"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    n, steps, N = 96, 26, 32
    model, lp, mix, theta0, y0 = case("abs", 2, 3, n=n)
    direct = check(oracle, "abs", 2, N, 3, n=n, steps=steps, cut=K_LAUNCH)
    runner = g_.MCMCRunner(model, str(tmp_path))
    t0, yy0 = torch.from_numpy(theta0), torch.from_numpy(y0)
    mom, state = engine.Moments(n, 2, torch.device("cuda", 0)), {}
    h = runner.run_glmcmc(steps + 1, t0, yy0, GF, lp, mix, N, seed=SEED, chain0=CHAIN0, stats=mom, return_device=True, verbose=False,
                          state_out=state, steps_per_launch=K_LAUNCH, output_file=None).cpu().numpy()
    assert h.shape == (steps + 1, n, 2) and np.array_equal(bits(h[0]), bits(theta0))
    assert np.array_equal(bits(h[1:].transpose(0, 2, 1)), bits(direct[0]))
    assert np.array_equal(bits(state["chains"].y.cpu().numpy()), bits(direct[1].y.cpu().numpy()))
    assert np.array_equal(bits(state["chains"].log_w.cpu().numpy()), bits(direct[1].log_w.cpu().numpy()))
    assert np.array_equal(mom.sum_jump.cpu().numpy().view(np.uint64), direct[2].sum_jump.cpu().numpy().view(np.uint64))
    with pytest.raises(TypeError):                                           # a fused call takes no generic-path extras
        runner.run_glmcmc(5, t0, yy0, GF, lp, mix, N, seed=SEED, verbose=False, output_file=None, sentinel_redraw=False)
    g = runner.run_glmcmc(12, t0, yy0, GF, lp, mix, N, seed=SEED, return_device=True, verbose=False, output_file=None, path="generic")
    assert g.shape == (12, n, 2) and torch.isfinite(g).all() and (g[-1] != g[0]).any()
    one = runner.run_glmcmc(20, t0[0], yy0[0], GF, lp, mix, N, seed=SEED, verbose=False, output_file=None)
    assert one.shape == (20, 2) and one.dtype == torch.float32 and not one.is_cuda and torch.isfinite(one).all()
    with pytest.raises(ValueError):
        runner.run_glmcmc(5, t0, yy0, GF, lp, mix, N, seed=SEED, verbose=False, output_file=None, fast_math=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_mixture_wide_refusals_on_the_device_library(hip):
    """each entry point keeps to its own batch sizes, and a refused call leaves the chains as they were"""
    from glabcmcmc_amd import engine
    model_o, lp_o, mix_o, theta0, y0 = case("abs", 2, 3, n=N65)
    model, lp, mix = model_o.descriptor(), lp_o.descriptor(), mix_o.descriptor()
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
    engine.init_weights(model, mix, chains)
    cs = chains.struct()

    def call(entry, **fields):
        run = A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency = SEED, 1, 2, GF
        for k, v in fields.items():
            setattr(run, k, v)
        return getattr(hip, entry)(C.byref(model), C.byref(lp), C.byref(mix), C.byref(cs), C.byref(run), None)

    assert call("glabc_glmcmc_mix_wide_steps", batch_size=16) == ARG
    assert call("glabc_glmcmc_mix_steps", batch_size=17) == ARG
    assert call("glabc_glmcmc_mix_wide_steps", batch_size=4097) == ARG
    assert call("glabc_glmcmc_mix_wide_steps", batch_size=17, lanes_per_chain=4) == ARG
    torch.cuda.synchronize()
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(np.ascontiguousarray(theta0.T)))
