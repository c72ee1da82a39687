"""glabc_rtc_compile_predictive / glabc_rtc_predictive_draws / glabc_rtc_predictive_counts without a GPU: hiprtc cross-compiles
predictive_kernel around a user's source (a valid one then fails to LOAD here: GLABC_ERR_NO_DEVICE, GLABC_OK on a GPU, as
tests/test_rtc_draws_host.py has it), the refusals that need no program, the ABI, and which path predictive takes for a CompiledModel.

The ABI: glabc_rtc_predictive_counts has the 17 parameters of glabc_predictive_counts behind the program, 18 in all, as
glabc_rtc_predictive_draws has glabc_predictive_draws' 14 behind it, 15 in all."""
import ctypes as C

import pytest
import torch

from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, predictive
from glabcmcmc_amd.compiled import CompiledModel, SimulatorCompileError
from test_rtc import ALL_USER, NONLINEAR, mixture_source
from test_rtc_draws_host import BROKEN, DIS_AND_KERNEL

OK, ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -6
MIXTURE = mixture_source([0.05 ** 0.5, 0.05 ** 0.5])


@pytest.fixture(scope="module")
def lib():
    try:
        return A.lib()
    except A.HipLibraryMissing:
        pytest.skip("libglabc_hip.so not built")


def compile_predictive(lib, source, d, yd, nd):
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = lib.glabc_rtc_compile_predictive(None if source is None else source.encode(), d, yd, nd, C.byref(handle), log, len(log))
    return rc, handle, log.value.decode(errors="replace")


@pytest.mark.parametrize("source,dims", [(NONLINEAR, (3, 2, 4)), (MIXTURE, (2, 2, 2)), (DIS_AND_KERNEL, (2, 3, 3)), (ALL_USER, (2, 3, 3))],
                         ids=["nonlinear", "mixture", "dis_and_kernel", "all_user"])
def test_a_valid_source_compiles_and_needs_a_device(lib, source, dims):
    """ALL_USER announces a prior of its own: accepted, unlike the draws program -- theta comes from the history"""
    rc, handle, log = compile_predictive(lib, source, *dims)
    if torch.cuda.is_available():
        assert rc == OK, log
        lib.glabc_rtc_release(handle)
    else:
        assert rc == ERR_NO_DEVICE, log
    assert "error" not in log


def test_compile_refusals_in_their_order(lib):
    rc, _, log = compile_predictive(lib, BROKEN, 1, 1, 1)
    assert rc == ERR_ARG and "error" in log and "user_simulator" in log
    for dims in ((0, 2, 4), (9, 2, 4), (3, 0, 4), (3, 9, 4), (3, 2, 0), (3, 2, 9)):
        assert compile_predictive(lib, NONLINEAR, *dims)[0] == ERR_DIM, dims
    assert compile_predictive(lib, None, 3, 2, 4)[0] == ERR_NULL
    log = C.create_string_buffer(256)
    assert lib.glabc_rtc_compile_predictive(NONLINEAR.encode(), 3, 2, 4, None, log, len(log)) == ERR_NULL
    assert compile_predictive(lib, None, 9, 2, 4)[0] == ERR_NULL                 # the order: pointers before dimensions
    assert lib.glabc_rtc_compile_predictive(NONLINEAR.encode(), 9, 2, 4, None, log, len(log)) == ERR_NULL
    assert compile_predictive(lib, BROKEN, 9, 1, 1)[0] == ERR_DIM                # ... and dimensions before the compiler
    assert compile_predictive(lib, ALL_USER, 9, 3, 3)[0] == ERR_DIM


def test_launches_without_a_program_are_refused(lib):
    m = A.Model()
    p = C.c_void_p(8)
    assert lib.glabc_rtc_predictive_draws(None, C.byref(m), p, 1, 1, 1, 1, 0, 0, 1, p, 1, p, 1, None) == ERR_NULL
    assert lib.glabc_rtc_predictive_counts(None, C.byref(m), p, 1, 1, 1, 1, 0, 0, 1, 1, p, p, p, p, p, p, None) == ERR_NULL
    assert lib.glabc_rtc_predictive_draws(None, None, None, 0, 0, -1, 0, 0, -1, 0, None, 0, None, 0, None) == ERR_NULL
    # the built-in entry points keep refusing a user simulator: no chains, nothing launched
    m.sim_kind, m.theta_dim, m.y_dim = A.SIM_USER, 2, 2
    assert lib.glabc_predictive_draws(C.byref(m), p, 1, 2, 0, 0, 0, 0, 0, p, 0, None, 0, None) == ERR_KIND


def test_the_abi_declares_the_three_entry_points():
    names = {"glabc_rtc_compile_predictive", "glabc_rtc_predictive_draws", "glabc_rtc_predictive_counts"}
    assert names <= set(A.ENTRY_POINTS)
    assert len(A.ENTRY_POINTS["glabc_rtc_compile_predictive"][1]) == 7
    assert len(A.ENTRY_POINTS["glabc_rtc_predictive_draws"][1]) == 15 == len(A.ENTRY_POINTS["glabc_predictive_draws"][1]) + 1
    assert len(A.ENTRY_POINTS["glabc_rtc_predictive_counts"][1]) == 18 == len(A.ENTRY_POINTS["glabc_predictive_counts"][1]) + 1
    assert A.VERSION == 301 and A.STREAM_LAYOUT == 2


def test_the_library_resolves_the_entry_points(lib):
    for name in ("glabc_rtc_compile_predictive", "glabc_rtc_predictive_draws", "glabc_rtc_predictive_counts"):
        assert getattr(lib, name).argtypes == A.ENTRY_POINTS[name][1]
    assert lib.glabc_version() == 301


# ---------------------------------------------------------------------------------- routing
def model(source, dims):
    d, yd, nd = dims
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    return CompiledModel(theta_dim=d, y_dim=yd, simulator_source=source, prior=prior, y_obs=[1.0] * yd, epsilon=0.1, noise_dim=nd)


def test_a_cpu_history_stays_on_the_generic_path():
    m = model(NONLINEAR, (3, 2, 4))
    assert callable(m.predictive_program)
    history = torch.zeros(4, 5, 3)
    assert predictive._path(m, history, "auto") is None and predictive._path(m, history, "generic") is None
    with pytest.raises(ValueError, match="GPU"):
        predictive._path(m, history, "fused")
    assert predictive.accepted(m) is None                          # accepted() keeps its meaning: the built-in kernels


def test_auto_without_a_gpu_is_the_generic_path(monkeypatch, recwarn):
    """... decided before any program is asked for: no compile, no warning"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def never(self):
        raise AssertionError("predictive_program() was asked for without a GPU")

    monkeypatch.setattr(CompiledModel, "predictive_program", never)
    m = model(NONLINEAR, (3, 2, 4))

    class OnGpu(torch.Tensor):                                     # a history that says it lives on a GPU, where there is none
        is_cuda = True

    assert predictive._path(m, torch.zeros(4, 5, 3).as_subclass(OnGpu), "auto") is None
    assert predictive._path(m, torch.zeros(4, 5, 3), "auto") is None
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning)]


def test_a_source_that_does_not_compile_is_compiled_once(lib, monkeypatch):
    m = model(BROKEN, (1, 1, 1))
    for _ in range(2):
        with pytest.raises(SimulatorCompileError, match="user_simulator"):
            m.predictive_program()
    calls = []
    real = lib.glabc_rtc_compile_predictive
    monkeypatch.setattr(lib, "glabc_rtc_compile_predictive", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(SimulatorCompileError, match="user_simulator"):
        m.predictive_program()
    assert not calls and (CompiledModel.PREDICTIVE,) not in m._programs


def test_a_bad_rows_knob_is_ignored_and_named_in_the_log(lib, monkeypatch):
    monkeypatch.setenv("GLABC_RTC_PRED_ROWS", "many")
    rc, handle, log = compile_predictive(lib, NONLINEAR, 3, 2, 4)
    assert rc in (OK, ERR_NO_DEVICE) and "GLABC_RTC_PRED_ROWS" in log and "ignored" in log
    if rc == OK:
        lib.glabc_rtc_release(handle)
    assert CompiledModel.predictive_rows() == 1
    for value, rows in (("17", 1), ("0", 1), ("8", 8), ("1", 1)):
        monkeypatch.setenv("GLABC_RTC_PRED_ROWS", value)
        assert CompiledModel.predictive_rows() == rows
        rc, handle, log = compile_predictive(lib, NONLINEAR, 3, 2, 4)
        assert rc in (OK, ERR_NO_DEVICE) and ("ignored" in log) == (value in ("17", "0")), (value, log)
        if rc == OK:
            lib.glabc_rtc_release(handle)


def test_fused_on_a_callback_model_still_raises():
    class Callback:
        epsilon, theta_dim, y_obs = 0.1, 3, torch.zeros(1, 3)

        def generate_samples(self, theta, n):
            return theta

        def discrepancy(self, y):
            return y.norm(dim=1)

    history = torch.zeros(4, 5, 3)
    with pytest.raises(ValueError, match='path="fused"'):
        predictive._path(Callback(), history, "fused")
    with pytest.raises(ValueError, match='path="fused"'):
        predictive.check(Callback(), history, seed=1, path="fused")
    assert predictive._path(Callback(), history, "auto") is None
    assert predictive.check(Callback(), history, bins=3, seed=1).n == 20     # callback Models stay generic
