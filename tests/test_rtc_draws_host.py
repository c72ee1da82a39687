"""glabc_rtc_compile_draws / glabc_rtc_abc_draws / glabc_rtc_smc_draws without a GPU: hiprtc cross-compiles the two draw kernels around a
user's source (a valid one then fails to LOAD here: GLABC_ERR_NO_DEVICE, GLABC_OK on a GPU, as tests/test_rtc_wide.py has it), the
refusals that need no program, and which path rejection / smc take for a CompiledModel."""
import ctypes as C

import pytest
import torch

from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, rejection, smc
from glabcmcmc_amd.compiled import CompiledModel
from test_rtc import ALL_USER, NONLINEAR, PRIOR_ONLY, mixture_source

OK, ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -6
MIXTURE = mixture_source([0.05 ** 0.5, 0.05 ** 0.5])
# the simulator of ALL_USER with its discrepancy and its kernel, and the descriptor's prior: theta[2], eps[3] -> y[3]
DIS_AND_KERNEL = ALL_USER[:ALL_USER.index("#define GLABC_USER_PRIOR")] + ALL_USER[ALL_USER.index("#define GLABC_USER_DISCREPANCY"):]
BROKEN = "GLABC_SIMULATOR void glabc_user_simulate(const float* t, const float* e, float* y) { y[0] = t[0] + ; }"


@pytest.fixture(scope="module")
def lib():
    try:
        return A.lib()
    except A.HipLibraryMissing:
        pytest.skip("libglabc_hip.so not built")


def compile_draws(lib, source, d, yd, nd):
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = lib.glabc_rtc_compile_draws(None if source is None else source.encode(), d, yd, nd, C.byref(handle), log, len(log))
    return rc, handle, log.value.decode(errors="replace")


@pytest.mark.parametrize("source,dims", [(NONLINEAR, (3, 2, 4)), (MIXTURE, (2, 2, 2)), (DIS_AND_KERNEL, (2, 3, 3))],
                         ids=["nonlinear", "mixture", "dis_and_kernel"])
def test_a_valid_source_compiles_and_needs_a_device(lib, source, dims):
    rc, handle, log = compile_draws(lib, source, *dims)
    if torch.cuda.is_available():
        assert rc == OK, log
        lib.glabc_rtc_release(handle)
    else:
        assert rc == ERR_NO_DEVICE, log
    assert "error" not in log


def test_compile_refusals(lib):
    rc, _, log = compile_draws(lib, BROKEN, 1, 1, 1)
    assert rc == ERR_ARG and "error" in log and "user_simulator" in log
    for dims in ((0, 2, 4), (9, 2, 4), (3, 0, 4), (3, 9, 4), (3, 2, 0), (3, 2, 9)):
        assert compile_draws(lib, NONLINEAR, *dims)[0] == ERR_DIM, dims
    assert compile_draws(lib, None, 3, 2, 4)[0] == ERR_NULL
    log = C.create_string_buffer(256)
    assert lib.glabc_rtc_compile_draws(NONLINEAR.encode(), 3, 2, 4, None, log, len(log)) == ERR_NULL
    assert compile_draws(lib, None, 9, 2, 4)[0] == ERR_NULL                      # the order: pointers before dimensions
    for source in (ALL_USER, PRIOR_ONLY):
        rc, _, log = compile_draws(lib, source, 2, 3, 3)
        assert rc == ERR_KIND and "GLABC_USER_PRIOR" in log
    assert compile_draws(lib, ALL_USER, 9, 3, 3)[0] == ERR_DIM                   # ... and dimensions before the user prior


def test_draws_without_a_program_are_refused(lib):
    m = A.Model()
    out = C.c_void_p(8)
    assert lib.glabc_rtc_abc_draws(None, C.byref(m), 0, 0, None, 1, 1, out, None, None, None, None) == ERR_NULL
    assert lib.glabc_rtc_smc_draws(None, C.byref(m), C.byref(A.Kde()), 0, 0, None, 1, 1, out, None, None, None, None, None) == ERR_NULL


def test_the_abi_declares_the_three_entry_points():
    assert {"glabc_rtc_compile_draws", "glabc_rtc_abc_draws", "glabc_rtc_smc_draws"} <= set(A.ENTRY_POINTS)
    assert len(A.ENTRY_POINTS["glabc_rtc_abc_draws"][1]) == 12 and len(A.ENTRY_POINTS["glabc_rtc_smc_draws"][1]) == 14
    assert A.VERSION == 301 and A.STREAM_LAYOUT == 2


# ---------------------------------------------------------------------------------- routing
def model(source, dims, prior):
    d, yd, nd = dims
    return CompiledModel(theta_dim=d, y_dim=yd, simulator_source=source, prior=prior, y_obs=[1.0] * yd, epsilon=0.1, noise_dim=nd)


def gauss(d):
    return distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))


def test_user_and_gamma_priors_stay_on_the_generic_path():
    user = model(ALL_USER, (2, 3, 3), gauss(2))
    gamma = model(NONLINEAR, (3, 2, 4), distribution.Gamma(torch.full((3,), 4.0), torch.full((3,), 2.0)))
    for m, word in ((user, "GLABC_USER_PRIOR"), (gamma, "neither DiagGaussian nor Uniform")):
        assert word in m.draws_refusal()
        assert rejection._path(m, "auto", 0.1) is None and rejection._path(m, "generic", 0.1) is None
        with pytest.raises(ValueError, match="fused"):
            rejection._path(m, "fused", 0.1)
        with pytest.raises(ValueError, match='path="fused"'):
            rejection.sample(m, 100, kernel="hard", n_accept=5, path="fused", seed=1)
        with pytest.raises(ValueError, match='path="fused"'):
            smc.sample(m, 16, kernel="hard", epsilon=1.0, path="fused", seed=1)
        with pytest.raises(ValueError, match="no draws program"):
            m.draws_program()
        # "auto" is the generic path, which asks for prior= before anything runs
        with pytest.raises(ValueError, match="prior="):
            rejection.sample(m, 100, kernel="hard", n_accept=5, seed=1)
        with pytest.raises(ValueError, match="prior="):
            smc.sample(m, 16, kernel="hard", epsilon=1.0, seed=1)
    for prior in (gauss(3), distribution.Uniform(3, torch.zeros(3), torch.ones(3))):
        assert model(NONLINEAR, (3, 2, 4), prior).draws_refusal() is None
    assert rejection.accepted(model(NONLINEAR, (3, 2, 4), gauss(3))) is None     # accepted() keeps its meaning: the built-in kernels


def test_auto_without_a_gpu_is_the_generic_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = model(NONLINEAR, (3, 2, 4), gauss(3))
    assert rejection._path(m, "auto", 0.1) is None
    with pytest.raises(ValueError, match="prior="):
        rejection.sample(m, 100, kernel="hard", n_accept=5, seed=1)


def test_callback_models_keep_asking_for_a_prior():
    class Callback:
        epsilon = 0.1

        def generate_samples(self, theta, n):
            return theta

        def discrepancy(self, y):
            return y.norm(dim=1)

    for path in ("auto", "generic"):
        with pytest.raises(ValueError, match="prior="):
            rejection.sample(Callback(), 100, kernel="hard", n_accept=5, seed=1, path=path)
        with pytest.raises(ValueError, match="prior="):
            smc.sample(Callback(), 16, kernel="hard", epsilon=1.0, seed=1, path=path)
    with pytest.raises(ValueError, match='path="fused"'):
        rejection.sample(Callback(), 100, kernel="hard", n_accept=5, seed=1, path="fused")
