"""GLMCMC's path="auto" dispatch: fast_math names a variant of the fused kernel, so "auto" takes the fused path for it whatever
else the call asks (the opt-in GLABC_MATH_FAST variant is never dropped for the split-phase path, exact arithmetic).
"""
import importlib

import numpy as np
import pytest
import torch

from helpers import bits, make_dist


class Route(Exception):
    pass


def _to(name):
    def go(*a, **k):
        raise Route(name)
    return go


def test_auto_takes_the_fused_path_with_and_without_fast_math(monkeypatch):
    """the route GLMCMC(..., path="auto") picks for a built-in Model, with the split-phase loop and the fused path's chain set-up
    replaced by markers (no device needed)"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import _host, generic
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    monkeypatch.setattr(generic, "run", _to("split-phase"))
    monkeypatch.setattr(_host, "prepare", _to("fused"))
    lp, ip = make_dist(("gauss", [0.0, 0.0], [0.35, 0.35])), make_dist(("gauss", [0.0, 0.0], [1.0, 1.0]))
    for fast_math in (False, True):
        with pytest.raises(Route, match="^fused$"):
            g_.GLMCMC(Mixture_set(0.05), 5, torch.zeros(8, 2), torch.ones(8, 2), lp, None, 0.5, ip, 5, seed=1, verbose=False,
                      fast_math=fast_math)
    with pytest.raises(Route, match="^split-phase$"):
        g_.GLMCMC(Mixture_set(0.05), 5, torch.zeros(8, 2), torch.ones(8, 2), lp, None, 0.5, ip, 5, seed=1, verbose=False, path="generic")


@pytest.mark.gpu
def test_hip_auto_fast_math_launches_the_fast_variant(hip, monkeypatch):
    """GLMCMC(..., fast_math=True) under "auto" reaches engine.run_steps with math_mode = GLABC_MATH_FAST, and gives the chains
    of path="fused", fast_math=True"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    engine = importlib.import_module("glabcmcmc_amd.engine")
    modes = []
    real = engine.run_steps

    def spy(*a, **k):
        modes.append(k.get("math_mode"))
        return real(*a, **k)

    monkeypatch.setattr(engine, "run_steps", spy)
    lp, ip = make_dist(("gauss", [0.0, 0.0], [0.35, 0.35])), make_dist(("gauss", [0.0, 0.0], [1.0, 1.0]))
    g = torch.Generator().manual_seed(2)
    th0 = torch.randn(512, 2, generator=g)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(512, 2, generator=g)
    auto = g_.GLMCMC(Mixture_set(0.05), 30, th0, y0, lp, None, 0.9, ip, 5, seed=11, verbose=False, fast_math=True)
    assert modes == [A.MATH_FAST]
    fused = g_.GLMCMC(Mixture_set(0.05), 30, th0, y0, lp, None, 0.9, ip, 5, seed=11, verbose=False, fast_math=True, path="fused")
    assert modes == [A.MATH_FAST, A.MATH_FAST]
    assert np.array_equal(bits(auto.numpy()), bits(fused.numpy())) and (auto[1:] != auto[:-1]).any()
