"""glabc_glmala_mix_steps (GLMALA with a GaussianMixture importance proposal, include/glabc.h) on the GPU, bit for bit against the
reference chain of tests/mala_mix_ref.py: the checker's MALA move and a numpy restatement of the iSIR move with the mixture of
tests/mixture_ref.py, itself held to the checker by tests/test_glmala_mix_host.py, which also asserts what the cases below reach.

Compared: history, theta / y / log_w, theta64 / y64 / log_w64, the cached gradient, flags, n_moves and the three moment sums.  Device
buffers start as canaries with padded strides (tests/test_glmala_shapes.py DeviceRun): after GLABC_OK no owned element holds one,
every padding element does, and after a refusal every buffer is what it was.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import glmala_mix_cases as cases
import mala_mix_ref as ref
from glabcmcmc_amd import _capi as A
from helpers import AbsGaussModel, bits, dev, make_dist
from test_glmala_shapes import DeviceRun, assert_equal_runs
from test_mixture_host import make_mixture

OK, ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = 0, -1, -2, -3, -4          # glabc_status, include/glabc.h


class MixRun(DeviceRun):
    """DeviceRun whose launches go to glabc_glmala_mix_steps"""

    def steps(self, hip, model, mix, mala, seed, gf, N, spl=None, lanes=0, edit=None, call=None):
        cs = self.chains()
        ms = A.Moments(*(self.g[k].data_ptr() for k in ("sum_theta", "sum_outer", "sum_jump"))) if "sum_theta" in self.g else None
        done = 0
        while done < self.T:
            k = min(spl or self.T, self.T - done)
            run = A.Run()
            run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = seed, 1 + done, k, gf, N
            run.lanes_per_chain = lanes
            if "history" in self.g:
                run.history, run.hist_stride = self.g["history"][done].data_ptr(), self.HS
            if ms is not None:
                run.moments = C.pointer(ms)
            if edit is not None:
                edit(run, cs)
            ptr = lambda x: None if x is None else C.byref(x)          # noqa: E731
            args = call(model, mix, mala, cs, run) if call else (model, mix, mala, cs, run)
            rc = hip.glabc_glmala_mix_steps(*[ptr(x) for x in args], None)
            if rc != 0:
                return rc
            done += k
        return 0


def device_case(hip, c):
    model, mix, mala, _ = cases.descriptors(c)
    theta0, y0 = cases.inputs(c)
    r = MixRun(theta0, y0, c["T"], chain0=c["chain0"], pad=c["pad"], hist_pad=c["hist_pad"])
    assert r.init(hip, model) == 0
    assert r.steps(hip, model, mix, mala, c["seed"], c["gf"], c["N"], spl=c["spl"], lanes=c["lanes"]) == 0
    return r.result()


# ------------------------------------------------------------------------------------------------------ every instantiation
@pytest.mark.gpu
@pytest.mark.parametrize("c", cases.SWEEP, ids=cases.case_id)
def test_hip_glmala_mix_every_compiled_shape(hip, oracle, c):
    """glmala_kernel<D, N, LEAN, MX> for D = 1..4, N = 1..16, both LEAN, and the theta_dim 2 team of two: 65 chains, 8-12 iterations
    in launches that do not divide them, 1 / 3 / 4 / 5 / 8 modes, chain ids above 2^32."""
    want, _, _ = cases.reference(oracle, c)
    got = device_case(hip, c)
    assert set(got) == set(want)
    assert_equal_runs(got, want, cases.case_id(c))


# ------------------------------------------------------------------------------------------------------ deep cases
@pytest.mark.gpu
@pytest.mark.parametrize("c", cases.DEEP, ids=cases.case_id)
def test_hip_glmala_mix_deep(hip, oracle, c):
    """130 chains x 60 iterations, N = 5, gf = 0.5: both branches in one wavefront in one iteration, every precision combination of
    the state slot, every mode, stays, and (Uniform prior) candidates of weight 0 -- test_deep_cases_reach_every_branch_of_the_move"""
    want, _, _ = cases.reference(oracle, c)
    got = device_case(hip, c)
    assert_equal_runs(got, want, cases.case_id(c))


@pytest.mark.gpu
def test_hip_glmala_mix_team_equals_one_wavefront(hip, oracle):
    """theta_dim 2 at lanes_per_chain 1 and 2, and the default (a team below 2048 wavefronts): the same bits"""
    one, two = (c for c in cases.DEEP if c["d"] == 2 and c["lanes"] in (1, 2))
    a, b, z = device_case(hip, one), device_case(hip, dict(two, pad=one["pad"], hist_pad=one["hist_pad"])), device_case(hip, dict(one, lanes=0))
    assert_equal_runs(a, b, "lanes 1 against 2")
    assert_equal_runs(z, b, "lanes 0 against 2")
    assert_equal_runs(a, cases.reference(oracle, one)[0], "lanes 1 against the reference")


# ------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_hip_glmala_mix_refusals_touch_nothing(hip):
    """every refusal of check_mala_mix_run once on the device, buffers unchanged; n_chains = 0 and n_steps = 0 are GLABC_OK and touch
    nothing"""
    from glabcmcmc_amd.examples.GK import GK_set
    c = cases.make_case(3, 5, 3, 70, 3, 0.5, 4, "away", 5, pad=2, hist_pad=1)
    model, mix, mala, _ = cases.descriptors(c)
    theta0, y0 = cases.inputs(c)
    spare = dev(np.zeros(4096, np.float32))
    tape = A.Tape(spare.data_ptr(), spare.data_ptr(), spare.data_ptr(), 4, 0)
    dd = A.DrawsOut(spare.data_ptr(), spare.data_ptr(), spare.data_ptr())

    def attempt(want, model=model, mix=mix, mala=mala, N=5, edit=None, call=None):
        r = MixRun(theta0, y0, c["T"], chain0=c["chain0"], pad=c["pad"], hist_pad=c["hist_pad"])
        assert r.steps(hip, model, mix, mala, c["seed"], c["gf"], N, edit=edit, call=call) == want
        r.assert_unchanged()

    def changed(obj, **kw):
        out = type(obj).from_buffer_copy(obj)
        for k, v in kw.items():
            setattr(out, k, v)
        return out

    def run_field(name, value):
        return lambda run, cs: setattr(run, name, value)

    def chain_field(name, value):
        return lambda run, cs: setattr(cs, name, value)

    attempt(ERR_NULL, call=lambda m, g, p, cs, r: (None, g, p, cs, r))
    attempt(ERR_KIND, model=GK_set(1.0).descriptor())
    gamma = AbsGaussModel(cases.EPS, cases.y_obs(c))
    gamma._prior = lambda: make_dist(("gamma", [2.0] * 3, [1.0] * 3))
    attempt(ERR_KIND, model=gamma.descriptor())
    m5 = AbsGaussModel(cases.EPS, [1.5, 0.8, 1.0, 0.5, 1.2]).descriptor()
    attempt(ERR_DIM, model=m5, mix=make_mixture(3, 5).descriptor())
    attempt(ERR_NULL, call=lambda m, g, p, cs, r: (m, None, p, cs, r))
    attempt(ERR_ARG, mix=changed(mix, n_modes=0))
    attempt(ERR_ARG, mix=changed(mix, n_modes=9))
    attempt(ERR_DIM, mix=make_mixture(3, 2).descriptor())
    bad = changed(mix)
    bad.scale[1][2] = 0.0
    attempt(ERR_ARG, mix=bad)
    bad = changed(mix)
    bad.cum_weight[1] = 0.01
    attempt(ERR_ARG, mix=bad)
    attempt(ERR_NULL, call=lambda m, g, p, cs, r: (m, g, None, cs, r))
    attempt(ERR_NULL, call=lambda m, g, p, cs, r: (m, g, p, cs, None))
    attempt(ERR_NULL, call=lambda m, g, p, cs, r: (m, g, p, None, r))
    attempt(ERR_NULL, edit=chain_field("theta64", None))
    attempt(ERR_NULL, edit=chain_field("grad", None))
    attempt(ERR_ARG, edit=chain_field("stride", 69))
    attempt(ERR_ARG, edit=chain_field("chain0", -1))
    attempt(ERR_ARG, edit=run_field("n_steps", -1))
    attempt(ERR_ARG, N=0)
    attempt(ERR_ARG, N=17)
    attempt(ERR_ARG, edit=run_field("global_frequency", float("nan")))
    attempt(ERR_ARG, edit=run_field("global_frequency_per_chain", spare.data_ptr()))
    attempt(ERR_ARG, mala=changed(mala, num_grad=1))
    attempt(ERR_ARG, mala=changed(mala, num_grad=65537))
    attempt(ERR_ARG, mala=changed(mala, tau=0.0))
    attempt(ERR_ARG, mala=changed(mala, eps_sq=-1.0))
    attempt(ERR_ARG, edit=run_field("hist_stride", 69))
    attempt(ERR_NULL, edit=lambda run, cs: setattr(run.moments.contents, "sum_jump", None))
    attempt(ERR_ARG, edit=run_field("tape", C.pointer(tape)))
    attempt(ERR_ARG, edit=run_field("math_mode", A.MATH_FAST))
    attempt(ERR_ARG, edit=run_field("dump_draws", C.pointer(dd)))
    attempt(ERR_ARG, edit=run_field("lanes_per_chain", 3))
    attempt(ERR_ARG, edit=run_field("step0", 0xFFFFFFFE))
    # nothing to do is not an error, and is nothing done
    attempt(OK, edit=chain_field("n_chains", 0))
    attempt(OK, edit=run_field("n_steps", 0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the package
def _package_case():
    d, n, T, N, num, gf, seed = 2, 70, 40, 5, 7, 0.5, 2031
    m = AbsGaussModel(cases.EPS, [1.5, 0.8])
    mix = make_mixture(4, d, spread=1.5)
    rng = np.random.default_rng(4)
    theta0 = (1.2 * rng.standard_normal((n, d))).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    return d, n, T, N, num, gf, seed, m, mix, theta0, y0


@pytest.mark.gpu
def test_glmala_function_with_a_mixture_is_fused_and_equals_the_c_calls(hip, oracle):
    """glabcmcmc_amd.GLMALA(|theta| + noise Model, ..., GaussianMixture, N) with path="auto" runs glabc_glmala_init +
    glabc_glmala_mix_steps through engine: the chains of the direct C calls and of the reference; state_out has `chains` and no
    `callback_device`; a single chain keeps the reference's shapes; path="generic" still takes the callback path."""
    import glabcmcmc_amd as g
    d, n, T, N, num, gf, seed, m, mix, theta0, y0 = _package_case()
    st = {}
    out = g.GLMALA(m, T + 1, torch.from_numpy(theta0), torch.from_numpy(y0), cases.TAU, num, None, gf, mix, N, seed=seed, verbose=False,
                   state_out=st, steps_per_launch=13)
    assert "callback_device" not in st and "chains" in st
    assert out.shape == (T + 1, n, d) and out.dtype == torch.float32
    model, md, mala = m.descriptor(), mix.descriptor(), A.Mala(cases.TAU, cases.TAU ** 2, cases.EPS ** 2, num, 0)
    r = MixRun(theta0, y0, T, pad=3, hist_pad=1)
    assert r.init(hip, model) == 0 and r.steps(hip, model, md, mala, seed, gf, N, spl=7) == 0
    direct = r.result()
    filler = make_dist(("gauss", [0.0] * d, [1.1] * d)).descriptor()
    want = ref.assemble(oracle, model, mala, ref.MixProvider(md), filler, theta0, y0, seed=seed, chain0=0, T=T, N=N, gf=gf)
    assert_equal_runs(direct, want, "direct C calls against the reference")
    got = out.numpy()
    assert np.array_equal(bits(got[0]), bits(theta0))
    same = bits(got[1:].transpose(0, 2, 1)) == bits(direct["history"])
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    ch = st["chains"]
    assert np.array_equal(ch.n_moves.cpu().numpy().astype(np.uint32), direct["n_moves"].astype(np.uint32)) and direct["n_moves"].sum() > 0
    assert np.array_equal(ch.flags.cpu().numpy().astype(np.uint32), direct["flags"].astype(np.uint32))
    assert np.array_equal(ch.theta64.cpu().numpy().view(np.uint64), direct["theta64"].view(np.uint64))
    assert np.array_equal(ch.log_w64.cpu().numpy().view(np.uint64), direct["log_w64"].view(np.uint64))
    # MCMCRunner passes the object through
    runner = g.MCMCRunner(m)
    again = runner.run_glmala(T + 1, torch.from_numpy(theta0), torch.from_numpy(y0), gf, mix, N, cases.TAU, num, None, seed=seed,
                              verbose=False)
    assert np.array_equal(bits(again.numpy()), bits(got))
    one = g.GLMALA(m, 30, torch.zeros(d) + 1.0, torch.tensor([[1.4, 0.9]]), cases.TAU, num, None, gf, mix, N, seed=3, verbose=False)
    assert one.shape == (30, d) and torch.isfinite(one).all()
    st2 = {}
    gen = g.GLMALA(m, 8, torch.from_numpy(theta0[:16]), torch.from_numpy(y0[:16]), cases.TAU, 3, None, gf, mix, N, seed=seed, verbose=False,
                   state_out=st2, path="generic")
    assert "callback_device" in st2 and gen.shape == (8, 16, d) and torch.isfinite(gen).all()


@pytest.mark.gpu
def test_glmala_function_with_a_mixture_outside_the_matrix_takes_the_callback_path(hip):
    """a 5-parameter Model and GK_set with a GaussianMixture stay on generic.run_glmala (state_out says so)"""
    import glabcmcmc_amd as g
    from glabcmcmc_amd.examples.GK import GK_set
    m5 = AbsGaussModel(0.5, [1.5, 1.0, 0.8, 1.2, 0.6])
    th5 = torch.zeros(12, 5) + 1.0
    st = {}
    out = g.GLMALA(m5, 8, th5, m5.generate_samples(th5), 0.2, 3, None, 0.5, make_mixture(3, 5, spread=1.5), 4, seed=11, verbose=False,
                   state_out=st)
    assert "callback_device" in st and out.shape == (8, 12, 5) and torch.isfinite(out).all()
    gk = GK_set(1.0)
    thg = torch.tensor([[3.0, 1.0, 2.0, 0.5]]).repeat(12, 1)
    st = {}
    out = g.GLMALA(gk, 8, thg, gk.generate_samples(thg), 0.05, 3, None, 0.5, make_mixture(3, 4, spread=1.0), 4, seed=12, verbose=False,
                   state_out=st)
    assert "callback_device" in st and out.shape == (8, 12, 4)
