"""Which kernels a run-time compiled MIXTURE program holds (rtc_mix_kernels of csrc/glabc_rtc_tables.h), on the CPU: the slots and
the #define block are pure functions of plain integers, so a small g++ driver evaluates them -- once as built, once under
-fsanitize=address,undefined (a stand-alone program).  The expected rows are literals written from what glabc_rtc_kernel.h
instantiates under GLABC_RTC_WITH_MIX; they are never printed from the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc")]
GLMCMC, GLOBAL = 0, 1

DRIVER = r"""
#include <cstdio>
#include "glabc_rtc_tables.h"
using namespace glabc;
static const char* SLOT[] = {"entry", "wide8", "wide16", "wide32", "wide64", "simulate_rows", "model_rows"};
static_assert(sizeof SLOT / sizeof SLOT[0] == RTC_MIX_SLOTS, "a name per slot");
static_assert(RTC_MIX_ENTRY == 0 && RTC_MIX_WIDE == 1 && RTC_MIX_SIMULATE_ROWS == 5 && RTC_MIX_MODEL_ROWS == 6 && RTC_MIX_SLOTS == 7,
              "entry, wide x 4, the two row kernels");
static_assert(RTC_SLOTS == 21 && RTC_SIMULATE_ROWS == 19, "the other table is untouched");
int main()
{
    RtcShape s;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &s.algo, &s.theta_dim, &s.y_dim, &s.noise_dim, &s.batch_size, &s.lanes, &s.wide, &s.gamma,
                      &s.hooks) == 9) {
        const RtcKernels t = rtc_mix_kernels(s);
        for (int i = 0; i < RTC_MIX_SLOTS; ++i)
            if (t.k[i].present)
                std::printf("slot|%s|%s|%s|%s|%s\n", SLOT[i], t.k[i].fatal ? "fatal" : "empty", t.k[i].lowered ? "expr" : "symbol",
                            t.k[i].define ? t.k[i].define : "-", t.k[i].name.c_str());
        std::printf("defines\n%send\n", t.defines.c_str());
    }
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def kernels(request, tmp_path_factory):
    """kernels(algo, D, YD, ND, N, wide=0, hooks=0) -> ({slot: (fatal | empty, expr | symbol, define, name)}, #define block)"""
    d = tmp_path_factory.mktemp("rtc_mix_kernels")
    (d / "driver.cpp").write_text(DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + INCLUDES + [str(d / "driver.cpp"), "-o", str(d / "driver")])

    def run(algo, th, yd, nd, n, wide=0, hooks=0, lanes=1):
        r = subprocess.run([str(d / "driver")], input="%d %d %d %d %d %d %d 0 %d\n" % (algo, th, yd, nd, n, lanes, wide, hooks),
                           capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        head, defines = r.stdout.split("defines\n")
        assert defines.endswith("end\n")
        slots = {}
        for line in head.splitlines():
            _, slot, fatal, kind, define, name = line.split("|")
            slots[slot] = (fatal, kind, define, name)
        return slots, defines[:-len("end\n")]
    return run


ROWS = {"simulate_rows": ("fatal", "symbol", "-", "glabc_rtc_simulate_rows"),
        "model_rows": ("fatal", "symbol", "-", "glabc_rtc_model_rows_kernel")}


def mix(name):
    return "fatal", "expr", "GLABC_RTC_WITH_MIX", name


def test_glmcmc_register_program(kernels):
    slots, defines = kernels(GLMCMC, 2, 2, 2, 5)
    assert slots == dict(ROWS, entry=mix("glabc::sampler_kernel<0, 2, 2, 5, 1, glabc::VAR_MIX, 0>"))
    assert defines == ("#define GLABC_RTC_L 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 2\n#define GLABC_RTC_YD 2\n#define GLABC_RTC_N 5\n"
                       "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 2\n#define GLABC_THETA_DIM 2\n#define GLABC_Y_DIM 2\n"
                       "#define GLABC_NOISE_DIM 2\n#define GLABC_SIMULATOR static __device__ __forceinline__\n"
                       "#define GLABC_RTC_WITH_MIX 1\n")


def test_hooks_change_nothing_and_lanes_are_not_read(kernels):
    for lanes in (1, 4):
        slots, defines = kernels(GLMCMC, 3, 2, 4, 12, hooks=1, lanes=lanes)
        assert slots == dict(ROWS, entry=mix("glabc::sampler_kernel<0, 3, 2, 12, 1, glabc::VAR_MIX, 0>"))
        assert defines == ("#define GLABC_RTC_L 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 3\n#define GLABC_RTC_YD 2\n#define GLABC_RTC_N 12\n"
                           "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 3\n#define GLABC_Y_DIM 2\n"
                           "#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n"
                           "#define GLABC_RTC_WITH_MIX 1\n")


def test_globalmcmc(kernels):
    slots, defines = kernels(GLOBAL, 8, 1, 3, 1)
    assert slots == dict(ROWS, entry=mix("glabc::sampler_kernel<1, 8, 1, 1, 1, glabc::VAR_MIX, 0>"))
    assert defines.startswith("#define GLABC_RTC_L 1\n#define GLABC_RTC_ALGO 1\n#define GLABC_RTC_D 8\n#define GLABC_RTC_YD 1\n#define GLABC_RTC_N 1\n")
    assert defines.endswith("#define GLABC_RTC_WITH_MIX 1\n") and defines.count("#define") == 12


def test_wide_program(kernels):
    slots, defines = kernels(GLMCMC, 3, 2, 4, 0, wide=1, lanes=0)
    assert slots == dict(ROWS, **{"wide%d" % L: mix("glabc::wide_kernel<3, 2, %d, false, true>" % L) for L in (8, 16, 32, 64)})
    assert defines == ("#define GLABC_RTC_WIDE 1\n#define GLABC_RTC_ALGO 0\n#define GLABC_RTC_D 3\n#define GLABC_RTC_YD 2\n"
                       "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 3\n#define GLABC_Y_DIM 2\n"
                       "#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n"
                       "#define GLABC_RTC_WITH_MIX 1\n")
