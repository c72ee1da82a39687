"""Which kernels a run-time compiled program holds (csrc/glabc_rtc_kernels.h), on the CPU: rtc_kernels, rtc_defines and
rtc_slot_for are pure functions of plain integers, so a small g++ driver evaluates them.  The rows below were written out by hand
from what glabc_rtc.hip asked hiprtc for and what the #if ladder of glabc_rtc_kernel.h instantiates, before the header existed;
they are never printed from it.  No GPU test sees a missing unit or team slot: every kernel gives the same chains."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc")]
GLMCMC, GLOBAL = 0, 1

SLOT_NAMES = ["entry", "entry_unit", "entry_gamma", "team2_gamma", "team3_gamma", "team2", "team2_unit", "team3", "team3_unit",
              "gteam", "gteam_unit", "wide8", "wide16", "wide32", "wide64", "wide8_gamma", "wide16_gamma", "wide32_gamma",
              "wide64_gamma", "simulate_rows", "model_rows"]

COMMON = r"""
#include <cstdio>
#include <cstring>
#include "glabc_rtc_kernels.h"
using namespace glabc;
static const char* SLOT[] = {%s};
static_assert(sizeof SLOT / sizeof SLOT[0] == RTC_SLOTS, "a name per slot");
static_assert(RTC_ENTRY == 0 && RTC_TEAM2_GAMMA == 3 && RTC_TEAM2 == 5 && RTC_TEAM3 == 7 && RTC_GTEAM == 9 && RTC_WIDE == 11 &&
              RTC_WIDE_GAMMA == 15 && RTC_SIMULATE_ROWS == 19 && RTC_MODEL_ROWS == 20, "the names above are in the enumeration's order");
""" % ", ".join('"%s"' % s for s in SLOT_NAMES)

DRIVER = COMMON + r"""
int main()
{
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "shape")) {
            RtcShape s;
            if (std::scanf("%d %d %d %d %d %d %d %d %d", &s.algo, &s.theta_dim, &s.y_dim, &s.noise_dim, &s.batch_size, &s.lanes, &s.wide,
                           &s.gamma, &s.hooks) != 9) return 1;
            const RtcKernels t = rtc_kernels(s);
            for (int i = 0; i < RTC_SLOTS; ++i)
                if (t.k[i].present)
                    std::printf("slot|%s|%s|%s|%s|%s\n", SLOT[i], t.k[i].fatal ? "fatal" : "empty", t.k[i].lowered ? "expr" : "symbol",
                                t.k[i].define ? t.k[i].define : "-", t.k[i].name.c_str());
            std::printf("defines\n%send\n", rtc_defines(s, t).c_str());
        } else {                                                   // plan kind, waves, lanes; Gamma launch; unit launch; held slots as a bit mask
            LaunchPlan p = {};
            int gamma, unit;
            unsigned mask;
            if (std::scanf("%d %d %d %d %d %u", &p.kind, &p.waves, &p.lanes, &gamma, &unit, &mask) != 6) return 1;
            bool held[RTC_SLOTS];
            for (int i = 0; i < RTC_SLOTS; ++i) held[i] = (mask >> i) & 1u;
            const int slot = rtc_slot_for(p, gamma != 0, unit != 0, held);
            std::printf("%s\n", slot < 0 ? "none" : SLOT[slot]);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("rtc_kernels")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + INCLUDES + [str(d / "driver.cpp"), "-o", str(d / "driver")])

    def run(text):
        return subprocess.run([str(d / "driver")], input=text, capture_output=True, text=True, check=True).stdout
    return run


@pytest.fixture(scope="module")
def kernels(driver):
    """kernels(algo, D, YD, ND, N, lanes=1, wide=0, gamma=0, hooks=0) -> ({slot: (fatal | empty, name)}, {slot: define}, #define block)"""
    def run(algo, d, yd, nd, n, lanes=1, wide=0, gamma=0, hooks=0):
        out = driver("shape %d %d %d %d %d %d %d %d %d\n" % (algo, d, yd, nd, n, lanes, wide, gamma, hooks))
        head, defines = out.split("defines\n")
        assert defines.endswith("end\n")
        slots, macros = {}, {}
        for line in head.splitlines():
            _, slot, fatal, kind, define, name = line.split("|")
            assert kind == ("symbol" if slot in ("simulate_rows", "model_rows") else "expr")
            slots[slot] = (fatal, name)
            if define != "-":
                macros[slot] = define
        return slots, macros, defines[:-len("end\n")]
    return run


ROWS = {"simulate_rows": ("fatal", "glabc_rtc_simulate_rows"), "model_rows": ("fatal", "glabc_rtc_model_rows_kernel")}


def entry(algo, d, yd, n, lanes, var, fatal="fatal"):
    return fatal, "glabc::sampler_kernel<%d, %d, %d, %d, %d, glabc::VAR_%s, 0>" % (algo, d, yd, n, lanes, var)


def team(d, yd, n, var, nw):
    return "empty", "glabc::team_sampler_kernel<%d, %d, %d, glabc::VAR_%s, %d, false>" % (d, yd, n, var, nw)


def head(lanes, algo, d, yd, n, nd):
    return ("#define GLABC_RTC_L %d\n#define GLABC_RTC_ALGO %d\n#define GLABC_RTC_D %d\n#define GLABC_RTC_YD %d\n#define GLABC_RTC_N %d\n"
            "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM %d\n#define GLABC_THETA_DIM %d\n#define GLABC_Y_DIM %d\n"
            "#define GLABC_NOISE_DIM %d\n#define GLABC_SIMULATOR static __device__ __forceinline__\n" % (lanes, algo, d, yd, n, nd, d, yd, nd))


def test_glmcmc_plain(kernels):
    slots, macros, defines = kernels(GLMCMC, 2, 2, 2, 5)
    assert slots == dict(ROWS, entry=entry(0, 2, 2, 5, 1, "GENERIC"), entry_unit=entry(0, 2, 2, 5, 1, "GAUSS_UNIT", "empty"),
                         team2=team(2, 2, 5, "GENERIC", 2), team2_unit=team(2, 2, 5, "GAUSS_UNIT", 2),
                         team3=team(2, 2, 5, "GENERIC", 3), team3_unit=team(2, 2, 5, "GAUSS_UNIT", 3))
    assert macros == {"team2": "GLABC_RTC_TEAM2", "team3": "GLABC_RTC_TEAM3"}       # the unit variants: the kernel header's own #if
    # the whole block, as a literal
    assert defines == ("#define GLABC_RTC_L 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 2\n#define GLABC_RTC_YD 2\n#define GLABC_RTC_N 5\n"
                       "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 2\n#define GLABC_THETA_DIM 2\n#define GLABC_Y_DIM 2\n"
                       "#define GLABC_NOISE_DIM 2\n#define GLABC_SIMULATOR static __device__ __forceinline__\n"
                       "#define GLABC_RTC_TEAM3 1\n#define GLABC_RTC_TEAM2 1\n")


def test_hooks_leave_no_unit_slot(kernels):
    slots, macros, defines = kernels(GLMCMC, 2, 2, 2, 5, hooks=1)
    assert slots == dict(ROWS, entry=entry(0, 2, 2, 5, 1, "GENERIC"), team2=team(2, 2, 5, "GENERIC", 2), team3=team(2, 2, 5, "GENERIC", 3))
    assert defines == head(1, 0, 2, 2, 5, 2) + "#define GLABC_RTC_TEAM3 1\n#define GLABC_RTC_TEAM2 1\n"
    slots, _, _ = kernels(GLOBAL, 2, 2, 2, 1, hooks=1)
    assert set(slots) == set(ROWS) | {"entry", "gteam"}


def test_unit_slots_need_equal_dimensions(kernels):
    slots, _, _ = kernels(GLMCMC, 2, 3, 3, 5)
    assert slots == dict(ROWS, entry=entry(0, 2, 3, 5, 1, "GENERIC"), team2=team(2, 3, 5, "GENERIC", 2), team3=team(2, 3, 5, "GENERIC", 3))


def test_more_lanes_leave_no_team(kernels):
    for lanes in (2, 4):
        slots, macros, defines = kernels(GLMCMC, 2, 2, 2, 5, lanes=lanes)
        assert slots == dict(ROWS, entry=entry(0, 2, 2, 5, lanes, "GENERIC"), entry_unit=entry(0, 2, 2, 5, lanes, "GAUSS_UNIT", "empty"))
        assert macros == {} and defines == head(lanes, 0, 2, 2, 5, 2)
    slots, _, defines = kernels(GLOBAL, 2, 2, 2, 1, lanes=2)
    assert set(slots) == set(ROWS) | {"entry", "entry_unit"} and defines == head(2, 1, 2, 2, 1, 2)


def test_team_sizes_follow_the_lds_budget(kernels):
    # team_config_ok (glabc_geometry.h): D = YD = 2 holds three wavefronts up to N 14 (10 helper candidates: 40 960 bytes) and two
    # up to 16; a single candidate has no team, two have no team of three
    want = {1: set(), 2: {"team2"}, 3: {"team2", "team3"}, 14: {"team2", "team3"}, 15: {"team2"}, 16: {"team2"}}
    for n, teams in want.items():
        slots, _, _ = kernels(GLMCMC, 2, 2, 2, n)
        assert {s for s in slots if s in ("team2", "team3")} == teams, n
        assert {s for s in slots if s in ("team2_unit", "team3_unit")} == {t + "_unit" for t in teams}, n


@pytest.mark.parametrize("n,teams", [(5, (3, 2)), (12, (2,)), (16, ())])
def test_gamma_program(kernels, n, teams):
    """(2, 3, 3): nine floats per candidate -- three wavefronts fit up to N 11, two up to 15; the Gamma teams by the same rule as
    the generic ones, the order of the #defines as the parent's format string had it"""
    slots, macros, defines = kernels(GLMCMC, 2, 3, 3, n, gamma=1)
    want = dict(ROWS, entry=entry(0, 2, 3, n, 1, "GENERIC"), entry_gamma=entry(0, 2, 3, n, 1, "GAMMA"))
    for nw in teams:
        want["team%d" % nw] = team(2, 3, n, "GENERIC", nw)
        want["team%d_gamma" % nw] = team(2, 3, n, "GAMMA", nw)
    assert slots == want
    assert macros == dict({"entry_gamma": "GLABC_RTC_WITH_GAMMA"}, **{"team%d" % nw: "GLABC_RTC_TEAM%d" % nw for nw in teams},
                          **{"team%d_gamma" % nw: "GLABC_RTC_GAMMA_TEAM%d" % nw for nw in teams})
    assert defines == (head(1, 0, 2, 3, n, 3) + "".join("#define GLABC_RTC_TEAM%d 1\n" % nw for nw in teams) + "#define GLABC_RTC_WITH_GAMMA 1\n" +
                       "".join("#define GLABC_RTC_GAMMA_TEAM%d 1\n" % nw for nw in teams))


def test_gamma_program_block_as_a_literal(kernels):
    assert kernels(GLMCMC, 2, 3, 3, 5, gamma=1)[2] == (
        "#define GLABC_RTC_L 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 2\n#define GLABC_RTC_YD 3\n#define GLABC_RTC_N 5\n"
        "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 3\n#define GLABC_THETA_DIM 2\n#define GLABC_Y_DIM 3\n"
        "#define GLABC_NOISE_DIM 3\n#define GLABC_SIMULATOR static __device__ __forceinline__\n"
        "#define GLABC_RTC_TEAM3 1\n#define GLABC_RTC_TEAM2 1\n#define GLABC_RTC_WITH_GAMMA 1\n#define GLABC_RTC_GAMMA_TEAM3 1\n"
        "#define GLABC_RTC_GAMMA_TEAM2 1\n")


def test_gamma_program_has_no_unit_slot(kernels):
    slots, _, _ = kernels(GLMCMC, 2, 2, 2, 5, gamma=1)
    assert set(slots) == set(ROWS) | {"entry", "entry_gamma", "team2", "team3", "team2_gamma", "team3_gamma"}


def test_gamma_kernels_keep_one_lane(kernels):
    slots, macros, defines = kernels(GLMCMC, 2, 3, 3, 5, lanes=4, gamma=1)
    assert slots == dict(ROWS, entry=entry(0, 2, 3, 5, 4, "GENERIC"), entry_gamma=entry(0, 2, 3, 5, 1, "GAMMA"),
                         team2_gamma=team(2, 3, 5, "GAMMA", 2), team3_gamma=team(2, 3, 5, "GAMMA", 3))
    assert defines == head(4, 0, 2, 3, 5, 3) + "#define GLABC_RTC_WITH_GAMMA 1\n#define GLABC_RTC_GAMMA_TEAM3 1\n#define GLABC_RTC_GAMMA_TEAM2 1\n"


def test_globalmcmc(kernels):
    slots, macros, defines = kernels(GLOBAL, 2, 2, 2, 1)
    assert slots == dict(ROWS, entry=entry(1, 2, 2, 1, 1, "GENERIC"), entry_unit=entry(1, 2, 2, 1, 1, "GAUSS_UNIT", "empty"),
                         gteam=("empty", "glabc::global_team_kernel<2, 2, glabc::VAR_GENERIC, 2>"),
                         gteam_unit=("empty", "glabc::global_team_kernel<2, 2, glabc::VAR_GAUSS_UNIT, 2>"))
    assert macros == {"gteam": "GLABC_RTC_GTEAM"}
    assert defines == head(1, 1, 2, 2, 1, 2) + "#define GLABC_RTC_GTEAM 1\n"
    assert "#define GLABC_RTC_N 1\n" in defines


def test_globalmcmc_team_needs_48_kib(kernels):
    # global_team_lds_bytes = 2 * 8 * (2 + D + 2 ceil(ND / 2)) * 64 * 4: (4, 6) takes 49 152 bytes, exactly 48 KiB; (4, 7) and
    # (5, 5) take 57 344 and 53 248
    assert "gteam" in kernels(GLOBAL, 4, 4, 6, 1)[0] and "gteam_unit" in kernels(GLOBAL, 4, 4, 6, 1)[0]
    for d, nd in ((4, 7), (5, 5), (8, 8)):
        slots, macros, defines = kernels(GLOBAL, d, d, nd, 1)
        assert set(slots) == set(ROWS) | {"entry", "entry_unit"} and macros == {} and defines == head(1, 1, d, d, 1, nd)


def test_globalmcmc_gamma_program(kernels):
    slots, macros, defines = kernels(GLOBAL, 2, 2, 2, 1, gamma=1)
    assert slots == dict(ROWS, entry=entry(1, 2, 2, 1, 1, "GENERIC"), entry_gamma=entry(1, 2, 2, 1, 1, "GAMMA"),
                         gteam=("empty", "glabc::global_team_kernel<2, 2, glabc::VAR_GENERIC, 2>"))
    assert defines == head(1, 1, 2, 2, 1, 2) + "#define GLABC_RTC_GTEAM 1\n#define GLABC_RTC_WITH_GAMMA 1\n"


def test_wide_programs(kernels):
    wide_head = ("#define GLABC_RTC_WIDE 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 3\n#define GLABC_RTC_YD 2\n"
                 "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 3\n#define GLABC_Y_DIM 2\n"
                 "#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    plain = dict(ROWS, **{"wide%d" % l: ("fatal", "glabc::wide_kernel<3, 2, %d, false>" % l) for l in (8, 16, 32, 64)})
    for hooks in (0, 1):
        slots, macros, defines = kernels(GLMCMC, 3, 2, 4, 0, lanes=0, wide=1, hooks=hooks)
        assert slots == plain and macros == {} and defines == wide_head
        slots, macros, defines = kernels(GLMCMC, 3, 2, 4, 0, lanes=0, wide=1, gamma=1, hooks=hooks)
        assert slots == dict(plain, **{"wide%d_gamma" % l: ("fatal", "glabc::wide_kernel<3, 2, %d, true>" % l) for l in (8, 16, 32, 64)})
        assert macros == {"wide%d_gamma" % l: "GLABC_RTC_WITH_GAMMA" for l in (8, 16, 32, 64)}
        assert defines == wide_head + "#define GLABC_RTC_WITH_GAMMA 1\n"


# ---- the slot a launch plan runs -------------------------------------------------------------------------------------------------
LANES, TEAM, GTEAM, WIDE = 1, 2, 3, 4               # PlanKind


@pytest.fixture(scope="module")
def slot_for(driver):
    def run(kind, waves=0, lanes=0, gamma=False, unit=False, held=SLOT_NAMES):
        mask = sum(1 << SLOT_NAMES.index(s) for s in held)
        return driver("plan %d %d %d %d %d %d\n" % (kind, waves, lanes, gamma, unit, mask)).strip()
    return run


def test_slot_of_a_plan(slot_for):
    families = {(LANES, 0, 1): "entry", (LANES, 0, 4): "entry", (TEAM, 2, 0): "team2", (TEAM, 3, 0): "team3", (GTEAM, 2, 0): "gteam"}
    for (kind, waves, lanes), generic in families.items():
        assert slot_for(kind, waves, lanes) == generic
        assert slot_for(kind, waves, lanes, unit=True) == generic + "_unit"
        # a unit launch of a program without that unit slot (hooks, theta_dim != y_dim, no lowered name): the generic kernel
        assert slot_for(kind, waves, lanes, unit=True, held=[s for s in SLOT_NAMES if s != generic + "_unit"]) == generic
        assert slot_for(kind, waves, lanes, unit=True, held=[]) == generic
        # a Gamma launch never takes a unit slot; the GlobalMCMC team has no Gamma kernel (the plan never names it for one)
        for unit in (False, True):
            assert slot_for(kind, waves, lanes, gamma=True, unit=unit) == ("none" if kind == GTEAM else generic + "_gamma")
    for l in (8, 16, 32, 64):
        for unit in (False, True):
            assert slot_for(WIDE, lanes=l, unit=unit) == "wide%d" % l
            assert slot_for(WIDE, lanes=l, unit=unit, gamma=True) == "wide%d_gamma" % l
    # what no program holds
    assert slot_for(WIDE, lanes=4) == "none" and slot_for(WIDE, lanes=0, gamma=True) == "none"
    assert slot_for(TEAM, 4) == "none" and slot_for(TEAM, 1, unit=True) == "none"
    assert slot_for(0) == "none" and slot_for(0, gamma=True, unit=True) == "none"


# ---- the header and the argument checks under the sanitizers ---------------------------------------------------------------------
WALK = COMMON + r"""
#include "glabc_check.h"
int main()
{
    long present = 0, picked = 0;
    for (int algo = 0; algo < 2; ++algo)
        for (int d = 1; d <= 8; ++d)
            for (int yd = 1; yd <= 8; ++yd)
                for (int n = 1; n <= 16; ++n)
                    for (int lanes = 1; lanes <= 4; lanes *= 2)
                        for (int flags = 0; flags < 8; ++flags) {
                            // noise_dim runs with y_dim; wide programs carry neither a batch size nor a lane count
                            const bool wide = flags & 4;
                            const RtcShape s = {algo, d, yd, 1 + (yd + n) % 8, wide ? 0 : n, wide ? 0 : lanes, wide, flags & 1, (flags >> 1) & 1};
                            const RtcKernels t = rtc_kernels(s);
                            bool held[RTC_SLOTS];
                            for (int i = 0; i < RTC_SLOTS; ++i) {
                                held[i] = t.k[i].present;
                                present += held[i];
                                if (held[i] && (t.k[i].name.empty() || t.k[i].name.size() >= 159)) return 2;
                            }
                            if (rtc_defines(s, t).size() >= 599) return 3;
                            for (int kind = 0; kind <= 5; ++kind)
                                for (int waves = 0; waves <= 5; ++waves)
                                    for (int l : {0, 1, 2, 4, 8, 16, 32, 64, 65})
                                        for (int gu = 0; gu < 4; ++gu) {
                                            const LaunchPlan p = {kind, 0, waves, l, 0, 1};
                                            const int slot = rtc_slot_for(p, gu & 1, gu & 2, held);
                                            if (slot < -1 || slot >= RTC_SLOTS) return 4;
                                            picked += slot >= 0 && held[slot];
                                        }
                        }
    std::printf("%ld %ld\n", present, picked);
    return 0;
}
"""


def test_walk_every_shape_under_the_sanitizers(tmp_path):
    """every shape of 1..8 x 1..8 x N 1..16 x lanes 1, 2, 4 x (Gamma, hooks, wide) through rtc_kernels, rtc_defines and every plan
    through rtc_slot_for, in a stand-alone program built with -fsanitize=address,undefined: no report, names and blocks within
    the buffers they are written through"""
    (tmp_path / "walk.cpp").write_text(WALK)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + INCLUDES +
                          [str(tmp_path / "walk.cpp"), "-o", str(tmp_path / "walk")])
    out = subprocess.run([str(tmp_path / "walk")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    present, picked = map(int, out.stdout.split())
    assert present > 0 and picked > 0
