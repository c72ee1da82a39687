"""The kernel tables of the run-time compiled DRAWS, PREDICTIVE and WEIGHTED PREDICTIVE programs (rtc_draws_kernels,
rtc_predictive_kernels, rtc_weighted_predictive_kernels of csrc/glabc_rtc_tables.h), on the CPU, and the row-kernel slots every
kind's table announces: pure functions of plain integers, so a small g++ driver evaluates them -- once as built, once under
-fsanitize=address,undefined (a stand-alone program).  The expected rows and #define blocks are literals written out by hand from
the three per-kind headers these tables had before they were merged into one (profiles/rtc_one_table.txt says which); they are
never printed from the header.  A one-character drift in a name expression or a #define line would otherwise show only on a GPU.
tests/test_rtc_kernels.py and tests/test_rtc_mix_kernels.py pin the sampler and the mixture tables."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc")]

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "glabc_rtc_tables.h"
using namespace glabc;
static_assert(RTC_DRAWS_ABC == 0 && RTC_DRAWS_SMC == 1 && RTC_DRAWS_SIMULATE_ROWS == 2 && RTC_DRAWS_MODEL_ROWS == 3 && RTC_DRAWS_SMC_FULL == 4 &&
              RTC_DRAWS_SLOTS == 5, "the two draw kernels, the two row kernels, the full-covariance twin");
static_assert(RTC_PRED_KERNEL == 0 && RTC_PRED_SIMULATE_ROWS == 1 && RTC_PRED_MODEL_ROWS == 2 && RTC_PRED_SLOTS == 3, "the kernel, the two row kernels");
static_assert(RTC_WPRED_KERNEL == 0 && RTC_WPRED_SIMULATE_ROWS == 1 && RTC_WPRED_MODEL_ROWS == 2 && RTC_WPRED_SLOTS == 3, "the kernel, the two row kernels");
static_assert(RTC_SLOTS == 21 && RTC_MIX_SLOTS == 7, "the other tables are untouched");
static_assert(RTC_PRED_ROWS == 1 && RTC_WEIGHTED_PRED_SEGMENTS == 1, "one row, one segment per item");

static void print(const RtcKernels& t)
{
    std::printf("geometry|%d|%d|%d|%d|%d\n", t.n_slots, t.wide0, t.n_wide, t.simulate_rows, t.model_rows);
    for (int i = 0; i < RTC_SLOTS; ++i)                           // past n_slots nothing may be present
        if (t.k[i].present)
            std::printf("slot|%d|%s|%s|%s|%s\n", i, t.k[i].fatal ? "fatal" : "empty", t.k[i].lowered ? "expr" : "symbol",
                        t.k[i].define ? t.k[i].define : "-", t.k[i].name.c_str());
    std::printf("defines\n%send\n", t.defines.c_str());
}

int main()
{
    char kind[32];
    while (std::scanf("%31s", kind) == 1) {
        if (!std::strcmp(kind, "rows")) {                           // rtc_predictive_rows of the knob's text ("-": not set)
            char asked[32];
            if (std::scanf("%31s", asked) != 1) return 1;
            std::printf("%d\n", rtc_predictive_rows(std::strcmp(asked, "-") ? asked : nullptr));
            continue;
        }
        RtcShape s = {};
        int rows = 0;
        if (std::scanf("%d %d %d %d %d %d %d", &s.theta_dim, &s.y_dim, &s.noise_dim, &s.hooks, &s.wide, &s.batch_size, &rows) != 7) return 1;
        s.algo = GLABC_ALGO_GLMCMC;
        s.lanes = s.wide ? 0 : 1;
        if (!std::strcmp(kind, "sampler")) print(rtc_kernels(s));
        else if (!std::strcmp(kind, "mixture")) print(rtc_mix_kernels(s));
        else if (!std::strcmp(kind, "draws")) print(rtc_draws_kernels(s));
        else if (!std::strcmp(kind, "predictive")) print(rows ? rtc_predictive_kernels(s, rows) : rtc_predictive_kernels(s));
        else if (!std::strcmp(kind, "weighted")) print(rtc_weighted_predictive_kernels(s));
        else return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def table(request, tmp_path_factory):
    """table(kind, D, YD, ND, hooks=0, wide=0, n=0, rows=0) -> ((n_slots, wide0, n_wide, simulate_rows, model_rows),
    {slot index: (fatal | empty, expr | symbol, define, name)}, #define block)"""
    d = tmp_path_factory.mktemp("rtc_tables")
    (d / "driver.cpp").write_text(DRIVER)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + INCLUDES + [str(d / "driver.cpp"), "-o", str(d / "driver")])

    def drive(text):
        r = subprocess.run([str(d / "driver")], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        return r.stdout

    def run(kind, th, yd, nd, hooks=0, wide=0, n=0, rows=0):
        head, defines = drive("%s %d %d %d %d %d %d %d\n" % (kind, th, yd, nd, hooks, wide, n, rows)).split("defines\n")
        assert defines.endswith("end\n")
        lines = head.splitlines()
        geometry = tuple(int(v) for v in lines[0].split("|")[1:])
        slots = {}
        for line in lines[1:]:
            _, slot, fatal, how, define, name = line.split("|")
            slots[int(slot)] = (fatal, how, define, name)
        return geometry, slots, defines[:-len("end\n")]
    run.drive = drive
    return run


SIMULATE_ROWS = ("fatal", "symbol", "-", "glabc_rtc_simulate_rows")
MODEL_ROWS = ("fatal", "symbol", "-", "glabc_rtc_model_rows_kernel")


def test_draws_table(table):
    for hooks in (0, 1):                                           # a user discrepancy or kernel changes nothing
        geometry, slots, defines = table("draws", 2, 3, 4, hooks=hooks)
        assert geometry == (5, 0, 0, 2, 3)                         # no lane-group kernels
        assert slots == {0: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::abc_draws_kernel<2, 3>"),
                         1: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::smc_draws_kernel<2, 3>"),
                         2: SIMULATE_ROWS, 3: MODEL_ROWS,
                         4: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::smc_draws_kernel<2, 3, true>")}
        assert defines == ("#define GLABC_RTC_DRAWS 1\n#define GLABC_RTC_D 2\n#define GLABC_RTC_YD 3\n"
                           "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 2\n#define GLABC_Y_DIM 3\n"
                           "#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    geometry, slots, defines = table("draws", 8, 8, 8)
    assert geometry == (5, 0, 0, 2, 3)
    assert slots == {0: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::abc_draws_kernel<8, 8>"),
                     1: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::smc_draws_kernel<8, 8>"),
                     2: SIMULATE_ROWS, 3: MODEL_ROWS,
                     4: ("fatal", "expr", "GLABC_RTC_DRAWS", "glabc::smc_draws_kernel<8, 8, true>")}
    assert defines == ("#define GLABC_RTC_DRAWS 1\n#define GLABC_RTC_D 8\n#define GLABC_RTC_YD 8\n"
                       "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 8\n#define GLABC_THETA_DIM 8\n#define GLABC_Y_DIM 8\n"
                       "#define GLABC_NOISE_DIM 8\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")


def test_predictive_table(table):
    for rows in (0, 1):                                            # 0: the default argument, RTC_PRED_ROWS
        geometry, slots, defines = table("predictive", 2, 3, 4, rows=rows)
        assert geometry == (3, 0, 0, 1, 2)
        assert slots == {0: ("fatal", "expr", "GLABC_RTC_PREDICTIVE", "glabc::predictive_kernel<2, 3, 1>"), 1: SIMULATE_ROWS, 2: MODEL_ROWS}
        assert defines == ("#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS 1\n#define GLABC_RTC_D 2\n"
                           "#define GLABC_RTC_YD 3\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 2\n"
                           "#define GLABC_Y_DIM 3\n#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    geometry, slots, defines = table("predictive", 2, 3, 4, hooks=1, rows=16)
    assert geometry == (3, 0, 0, 1, 2)
    assert slots == {0: ("fatal", "expr", "GLABC_RTC_PREDICTIVE", "glabc::predictive_kernel<2, 3, 16>"), 1: SIMULATE_ROWS, 2: MODEL_ROWS}
    assert defines == ("#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS 16\n#define GLABC_RTC_D 2\n"
                       "#define GLABC_RTC_YD 3\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 2\n"
                       "#define GLABC_Y_DIM 3\n#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    _, slots, defines = table("predictive", 8, 8, 8, rows=1)
    assert slots == {0: ("fatal", "expr", "GLABC_RTC_PREDICTIVE", "glabc::predictive_kernel<8, 8, 1>"), 1: SIMULATE_ROWS, 2: MODEL_ROWS}
    assert defines == ("#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS 1\n#define GLABC_RTC_D 8\n"
                       "#define GLABC_RTC_YD 8\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 8\n#define GLABC_THETA_DIM 8\n"
                       "#define GLABC_Y_DIM 8\n#define GLABC_NOISE_DIM 8\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    _, slots, defines = table("predictive", 8, 8, 8, rows=16)       # the longest text of the three kinds
    assert slots == {0: ("fatal", "expr", "GLABC_RTC_PREDICTIVE", "glabc::predictive_kernel<8, 8, 16>"), 1: SIMULATE_ROWS, 2: MODEL_ROWS}
    assert defines == ("#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS 16\n#define GLABC_RTC_D 8\n"
                       "#define GLABC_RTC_YD 8\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 8\n#define GLABC_THETA_DIM 8\n"
                       "#define GLABC_Y_DIM 8\n#define GLABC_NOISE_DIM 8\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")


def test_predictive_rows_knob(table):
    """rtc_predictive_rows, which moved with the table: GLABC_RTC_PRED_ROWS=1..16 is taken, anything else is RTC_PRED_ROWS"""
    want = {"-": 1, "1": 1, "4": 4, "16": 16, "0": 1, "17": 1, "-3": 1, "many": 1, "8x": 8}            # atoi: "8x" reads 8
    got = table.drive("".join("rows %s\n" % text for text in want)).split()
    assert [int(v) for v in got] == list(want.values())


def test_weighted_predictive_table(table):
    for hooks in (0, 1):
        geometry, slots, defines = table("weighted", 2, 3, 4, hooks=hooks)
        assert geometry == (3, 0, 0, 1, 2)
        assert slots == {0: ("fatal", "expr", "GLABC_RTC_WEIGHTED_PREDICTIVE", "glabc::weighted_predictive_kernel<2, 3, 1>"),
                         1: SIMULATE_ROWS, 2: MODEL_ROWS}
        assert defines == ("#define GLABC_RTC_WEIGHTED_PREDICTIVE 1\n#define GLABC_RTC_WPRED_SEGMENTS 1\n#define GLABC_RTC_D 2\n"
                           "#define GLABC_RTC_YD 3\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 4\n#define GLABC_THETA_DIM 2\n"
                           "#define GLABC_Y_DIM 3\n#define GLABC_NOISE_DIM 4\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")
    geometry, slots, defines = table("weighted", 8, 8, 8)
    assert geometry == (3, 0, 0, 1, 2)
    assert slots == {0: ("fatal", "expr", "GLABC_RTC_WEIGHTED_PREDICTIVE", "glabc::weighted_predictive_kernel<8, 8, 1>"),
                     1: SIMULATE_ROWS, 2: MODEL_ROWS}
    assert defines == ("#define GLABC_RTC_WEIGHTED_PREDICTIVE 1\n#define GLABC_RTC_WPRED_SEGMENTS 1\n#define GLABC_RTC_D 8\n"
                       "#define GLABC_RTC_YD 8\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM 8\n#define GLABC_THETA_DIM 8\n"
                       "#define GLABC_Y_DIM 8\n#define GLABC_NOISE_DIM 8\n#define GLABC_SIMULATOR static __device__ __forceinline__\n")


@pytest.mark.parametrize("kind,kw,geometry", [
    ("sampler", dict(n=5), (21, 11, 8, 19, 20)), ("sampler", dict(wide=1), (21, 11, 8, 19, 20)),
    ("mixture", dict(n=5), (7, 1, 4, 5, 6)), ("mixture", dict(wide=1), (7, 1, 4, 5, 6)),
    ("draws", {}, (5, 0, 0, 2, 3)), ("predictive", dict(rows=16), (3, 0, 0, 1, 2)), ("weighted", {}, (3, 0, 0, 1, 2))])
def test_every_kind_announces_its_row_kernels(table, kind, kw, geometry):
    """the two slots a table names for the row kernels hold the extern "C" symbols (glabc_rtc_simulate and glabc_rtc_model_rows launch
    them by these fields alone), every slot stands below n_slots, and the lane-group range holds lane-group kernels or nothing"""
    for shape in ((2, 3, 4), (8, 8, 8)):
        got, slots, _ = table(kind, *shape, **kw)
        assert got == geometry
        n_slots, wide0, n_wide, simulate_rows, model_rows = got
        assert slots[simulate_rows] == SIMULATE_ROWS and slots[model_rows] == MODEL_ROWS
        assert [s for s, row in slots.items() if row[1] == "symbol"] == [simulate_rows, model_rows]
        assert max(slots) < n_slots and wide0 + n_wide <= n_slots
        assert all("wide_kernel<" in slots[s][3] for s in range(wide0, wide0 + n_wide) if s in slots)
        assert not any("wide_kernel<" in row[3] for s, row in slots.items() if not wide0 <= s < wide0 + n_wide)
