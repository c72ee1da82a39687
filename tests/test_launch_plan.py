"""Which kernel a fused sampler call launches (csrc/glabc_plan.h plan_launch), on the CPU: the header is a pure function of
plain integers, so a small g++ driver evaluates it and the rows below -- written out by hand from DESIGN.md 4.0, never produced
by the function -- say what it must answer.  No GPU test can see the choice: every kernel gives the same chains."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GLMCMC, GLOBAL = 0, 1
NO_TEAM, TEAM, DEFAULT_SCHEDULE = 2, 4, 8
ERR_DIM, ERR_ARG = -2, -4

FIELDS = ["algo", "D", "YD", "gk", "gamma", "fast", "tape", "debug", "lanes", "N", "C", "waves", "prio",
          "rtc", "team2", "team3", "gteam", "rtc_lanes"]
# every row: GLMCMC, |theta| + noise, D = YD = 2, exact arithmetic, no tape, no flags, geometry left to the library, no overrides
DEFAULTS = dict(algo=GLMCMC, D=2, YD=2, gk=0, gamma=0, fast=0, tape=0, debug=0, lanes=0, N=5, C=65536, waves=None, prio=None,
                rtc=0, team2=0, team3=0, gteam=0, rtc_lanes=0)

DRIVER = r"""
#include <cstdio>
#include "glabc_plan.h"
int main()
{
    using namespace glabc;
    static_assert(plan_launch(PlanIn{}).kind == PLAN_REFUSED, "constexpr, and theta_dim 0 is refused");
    const char* kind[] = {"refused", "lanes", "team", "gteam", "wide"};
    PlanIn in;
    long long c;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %d", &in.algo, &in.theta_dim, &in.y_dim, &in.gk,
                      &in.gamma, &in.fast, &in.tape, &in.debug_flags, &in.lanes_per_chain, &in.batch_size, &c, &in.team_waves.set,
                      &in.team_waves.value, &in.team_prio.set, &in.team_prio.value, &in.rtc, &in.rtc_team2, &in.rtc_team3,
                      &in.rtc_gteam, &in.rtc_lanes) == 20) {
        in.n_chains = c;
        const LaunchPlan p = plan_launch(in);
        std::printf("%s %d %d %d %d %d\n", kind[p.kind], p.status, p.waves, p.lanes, p.ilp, p.prio);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(**overrides of DEFAULTS) -> ("lanes", L, "ilp" | "def") | ("team" | "gteam", waves, prio) | ("wide", L) |
    ("refused", status); GK=True stands for the g-and-k shape (D 4, YD 8)."""
    d = tmp_path_factory.mktemp("plan")
    (d / "plan.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc"), str(d / "plan.cpp"), "-o", str(d / "plan")])

    def run(GK=False, **kw):
        assert set(kw) <= set(DEFAULTS), kw
        row = dict(DEFAULTS, **kw)
        if GK:
            row.update(D=4, YD=8, gk=1)
        elif "YD" not in kw:
            row["YD"] = row["D"]
        words = []
        for f in FIELDS:
            words += [int(row[f] is not None), row[f] or 0] if f in ("waves", "prio") else [row[f]]
        out = subprocess.run([str(d / "plan")], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, check=True)
        kind, status, waves, lanes, ilp, prio = out.stdout.split()
        if kind == "lanes":
            return kind, int(lanes), "ilp" if int(ilp) else "def"
        if kind in ("team", "gteam"):
            return kind, int(waves), int(prio)
        return (kind, int(lanes)) if kind == "wide" else (kind, int(status))
    return run


def L(lanes, sched):
    return "lanes", lanes, sched


def team(waves, prio=1):
    return "team", waves, prio


def gteam(waves, prio=1):
    return "gteam", waves, prio


def test_window_edges(plan):
    want = {16383: L(4, "def"), 16384: team(3), 65536: team(3), 65537: team(2), 131072: team(2), 131073: L(1, "def")}
    assert {c: plan(C=c) for c in want} == want


def test_pick_lanes(plan):
    assert plan(debug=NO_TEAM, C=65536) == L(1, "ilp")
    assert plan(debug=NO_TEAM, C=32768) == L(2, "def")
    assert plan(debug=NO_TEAM, C=16384) == L(4, "def")
    assert plan(debug=NO_TEAM, C=512, N=2) == L(2, "def")
    assert plan(debug=NO_TEAM, C=512, N=1) == L(1, "ilp")
    assert plan(debug=NO_TEAM, C=40000, lanes=1) == L(1, "ilp")
    assert plan(lanes=2, C=65536) == L(2, "def")            # explicit lanes close the window


def test_team_size_from_split_and_lds(plan):
    want = {(2, 1): L(1, "ilp"), (2, 2): team(2), (2, 3): team(3), (2, 12): team(3), (2, 13): team(3), (2, 15): team(2),
            (2, 16): team(2),                               # three wavefronts would need 45 056 bytes
            (3, 11): team(3), (3, 12): team(2), (3, 16): L(1, "ilp"),
            (4, 7): team(3), (4, 8): team(3), (4, 9): team(2), (4, 11): team(2), (4, 12): L(1, "ilp"), (4, 16): L(1, "ilp")}
    assert {k: plan(D=k[0], N=k[1]) for k in want} == want
    assert plan(D=4, N=12, debug=TEAM, C=100) == L(4, "def")        # no team fits: lanes from pick_lanes


def test_g_and_k(plan):
    want = {5: team(3), 7: team(3), 8: team(2), 9: team(2), 10: L(1, "def")}
    assert {n: plan(GK=True, N=n) for n in want} == want
    assert plan(GK=True, C=512, debug=NO_TEAM, lanes=1) == L(1, "def")      # never the max-ilp objects


def test_team_waves_and_prio_overrides(plan):
    assert plan(debug=TEAM, C=512, waves=4) == team(4)
    assert plan(debug=TEAM, C=512, waves=4, N=3) == team(3)
    assert plan(debug=TEAM, C=512, waves=4, N=13) == team(3)
    assert plan(debug=TEAM, C=512, waves=4, N=2) == team(2)
    assert plan(debug=TEAM, C=512, waves=7) == team(4)
    assert plan(debug=TEAM, C=512, waves=1) == team(2)
    assert plan(debug=TEAM, C=512, waves=0) == team(2)
    assert plan(debug=TEAM, C=512, waves=2) == team(2)
    assert [plan(debug=TEAM, C=512, prio=p) for p in (0, 3, 9, -1)] == [team(3, 0), team(3, 3), team(3, 3), team(3, 0)]


def test_debug_bits(plan):
    assert plan(debug=TEAM | NO_TEAM) == L(1, "ilp")        # NO_TEAM wins
    assert plan(debug=NO_TEAM | DEFAULT_SCHEDULE, C=512, lanes=1) == L(1, "def")


def test_fast_math(plan):
    assert plan(fast=1, C=512) == team(3)
    assert plan(fast=1, C=512, debug=NO_TEAM) == team(3)
    assert plan(fast=1, C=512, waves=4) == team(3)
    assert plan(fast=1, C=200000) == team(2)
    assert plan(fast=1, D=4, N=12) == ("refused", ERR_ARG)


def test_gamma(plan):
    assert plan(gamma=1) == team(3)
    assert plan(gamma=1, waves=4) == team(3)
    assert plan(gamma=1, C=512) == L(1, "def")
    assert plan(gamma=1, C=512, lanes=4) == L(1, "def")


def test_tape(plan):
    assert plan(tape=1) == L(1, "def")
    assert plan(tape=1, debug=TEAM) == L(1, "def")


def test_theta_dim_6(plan):
    assert plan(D=6) == L(4, "def")
    assert plan(D=6, N=2) == L(2, "def")
    assert plan(D=6, N=1) == L(1, "def")
    assert plan(D=6, lanes=1) == L(1, "def")
    assert plan(D=6, tape=1) == L(1, "def")
    assert plan(D=6, algo=GLOBAL) == L(1, "def")
    assert plan(D=6, N=17) == ("refused", ERR_DIM)
    assert plan(D=9) == ("refused", ERR_DIM)


def test_wide(plan):
    want = {17: 8, 64: 8, 65: 16, 128: 16, 129: 32, 256: 32, 257: 64, 4096: 64}
    assert {n: plan(N=n) for n in want} == {n: ("wide", l) for n, l in want.items()}
    assert plan(N=17, lanes=32) == ("wide", 32)
    assert plan(GK=True, N=100, debug=TEAM) == ("wide", 16)


def test_globalmcmc(plan):
    assert plan(algo=GLOBAL) == gteam(2)
    assert plan(algo=GLOBAL, waves=3) == gteam(3)
    assert plan(algo=GLOBAL, waves=4) == gteam(3)
    assert plan(algo=GLOBAL, waves=1) == gteam(2)
    assert plan(algo=GLOBAL, prio=3) == gteam(2)            # GLABC_TEAM_PRIO is the GLMCMC team's
    assert plan(algo=GLOBAL, C=512) == L(1, "ilp")
    assert plan(algo=GLOBAL, C=512, debug=TEAM) == gteam(2)
    assert plan(algo=GLOBAL, gamma=1) == L(1, "def")
    assert plan(algo=GLOBAL, C=131073) == L(1, "def")
    assert plan(algo=GLOBAL, GK=True) == gteam(2)
    assert plan(algo=GLOBAL, GK=True, C=512) == L(1, "def")
    assert plan(algo=GLOBAL, N=4096) == gteam(2)            # GlobalMCMC ignores batch_size


def test_run_time_compiled_program(plan):
    both = dict(rtc=1, team2=1, team3=1, rtc_lanes=1)
    assert plan(**both) == team(3)
    assert plan(rtc=1, team2=1, rtc_lanes=1) == team(2)
    assert plan(C=100000, **both) == team(2)
    assert plan(C=100000, rtc=1, team3=1, rtc_lanes=1) == team(3)
    assert plan(rtc=1, rtc_lanes=2) == L(2, "def")          # the compiled entry at its compiled lane count
    assert plan(debug=NO_TEAM, **dict(both, rtc_lanes=4)) == L(4, "def")
    assert plan(C=512, debug=TEAM, **both) == team(3)
    assert plan(waves=2, prio=3, **both) == team(3)         # the overrides do not reach a program
    assert plan(D=7, YD=3, N=16, **both) == team(3)         # what the program holds counts, not the built-in shapes
    assert plan(algo=GLOBAL, rtc=1, gteam=1, rtc_lanes=1) == gteam(2)
    assert plan(algo=GLOBAL, rtc=1, gteam=1, rtc_lanes=1, waves=3) == gteam(2)
    assert plan(algo=GLOBAL, rtc=1, rtc_lanes=1) == L(1, "def")
    assert plan(algo=GLOBAL, rtc=1, gteam=1, rtc_lanes=1, C=512) == L(1, "def")
    want = {17: 8, 64: 8, 65: 16, 256: 32, 257: 64, 4096: 64}                   # a wide program: the built-in lane rule
    assert {n: plan(rtc=1, D=6, YD=3, N=n) for n in want} == {n: ("wide", l) for n, l in want.items()}
    assert plan(rtc=1, N=17, lanes=32) == ("wide", 32)


# test_hip_parity.py::test_team_geometry_is_only_geometry forces GLABC_DEBUG_TEAM and sets GLABC_TEAM_WAVES = 2, 3, 4: the kernel
# each (theta_dim, batch size) of its TEAM_CASES then reaches, so that a row which exercises no team kernel is visible here
TEAM_CASE_PLANS = {
    (2, 5): (team(2), team(3), team(4)),
    (2, 2): (team(2), team(2), team(2)),
    (2, 3): (team(2), team(3), team(3)),
    (2, 4): (team(2), team(3), team(4)),
    (2, 6): (team(2), team(3), team(4)),
    (2, 8): (team(2), team(3), team(4)),
    (2, 13): (team(2), team(3), team(3)),
    (2, 16): (team(2), team(2), team(2)),
    (1, 5): (team(2), team(3), team(4)),
    (3, 5): (team(2), team(3), team(4)),
    (3, 7): (team(2), team(3), team(4)),
    (4, 5): (team(2), team(3), team(4)),
    (4, 8): (team(2), team(3), team(3)),
    (4, 11): (team(2), team(2), team(2)),
    (4, 12): (L(4, "def"),) * 3,                            # no team fits 40 KiB: pins the fall-through to sampler_kernel
}


def test_team_cases_of_the_parity_test(plan):
    from test_hip_parity import TEAM_CASES
    assert {(c[0], c[1]) for c in TEAM_CASES} == set(TEAM_CASE_PLANS)
    for d, N, _gf, _eps, _local, _global, chains, _T in TEAM_CASES:
        got = tuple(plan(D=d, N=N, C=chains, debug=TEAM, waves=w) for w in (2, 3, 4))
        assert got == TEAM_CASE_PLANS[(d, N)], (d, N)
        if N == 12:     # ... where the second half of the test (GLABC_DEBUG_NO_TEAM) runs the very same kernel
            assert plan(D=d, N=N, C=chains, debug=NO_TEAM, waves=2) == got[0]
