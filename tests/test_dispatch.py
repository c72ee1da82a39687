"""Run-time integer -> template parameter (csrc/glabc_dispatch.h), on the CPU: a small g++ driver runs dispatch_range and
dispatch_values over every integer around their sets and reports what reached the callable.  Every launcher of the library
picks its kernel instantiation through these two functions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_FOUND = -77          # the caller's status: no library status, so nothing else can produce it

# name -> the members of the set; the driver below holds the same sets as template arguments
SETS = {"r1_8": list(range(1, 9)), "r2_16": list(range(2, 17)), "r2_3": [2, 3], "r5_5": [5], "wide": [8, 16, 32, 64],
        "unordered": [4, 1, 2]}

DRIVER = r"""
#include <cstdio>
#include "glabc_dispatch.h"
using namespace glabc;

static int n_calls, seen;

// what the callable returns for V: distinct per V, negative and positive, never NOT_FOUND
static int answer(int v) { return 1000 - 37 * v; }

template <class Dispatch>
static void sweep(const char* name, Dispatch dispatch)
{
    for (int v = -3; v <= 70; ++v) {
        n_calls = 0;
        seen = -1000;
        const int rc = dispatch(v, [](auto c) {
            constexpr int V = decltype(c)::value;                    // a constant expression: usable as a template argument
            static_assert(V >= 1 && V <= 64, "only members are instantiated");
            ++n_calls;
            seen = V;
            return answer(V);
        });
        std::printf("%s %d %d %d %d\n", name, v, rc, n_calls, seen);
    }
}

int main()
{
    const int nf = -77;
    sweep("r1_8", [=](int v, auto f) { return dispatch_range<1, 8>(v, nf, f); });
    sweep("r2_16", [=](int v, auto f) { return dispatch_range<2, 16>(v, nf, f); });
    sweep("r2_3", [=](int v, auto f) { return dispatch_range<2, 3>(v, nf, f); });
    sweep("r5_5", [=](int v, auto f) { return dispatch_range<5, 5>(v, nf, f); });
    sweep("wide", [=](int v, auto f) { return dispatch_values<8, 16, 32, 64>(v, nf, f); });
    sweep("unordered", [=](int v, auto f) { return dispatch_values<4, 1, 2>(v, nf, f); });
    // a callable with state, passed as an lvalue, and one that answers the not-found status itself
    int hits = 0;
    auto count = [&](auto c) { hits += decltype(c)::value; return 0; };
    dispatch_range<1, 4>(3, nf, count);
    dispatch_range<1, 4>(4, nf, count);
    dispatch_range<1, 4>(5, nf, count);
    std::printf("state 0 %d 0 0\n", hits);
    std::printf("same 0 %d 0 0\n", dispatch_range<1, 4>(2, nf, [=](auto) { return nf; }));
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """{set name: {v: (returned, number of calls, the V the callable saw)}}"""
    d = tmp_path_factory.mktemp("dispatch")
    (d / "dispatch.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc"),
                           str(d / "dispatch.cpp"), "-o", str(d / "dispatch")])
    out = subprocess.run([str(d / "dispatch")], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        name, v, rc, calls, seen = line.split()
        table.setdefault(name, {})[int(v)] = (int(rc), int(calls), int(seen))
    return table


def answer(v):
    return 1000 - 37 * v


@pytest.mark.parametrize("name", sorted(SETS))
def test_every_member_reaches_the_callable_once_with_its_own_value(rows, name):
    for v in SETS[name]:
        assert rows[name][v] == (answer(v), 1, v), (name, v)


@pytest.mark.parametrize("name", sorted(SETS))
def test_every_other_value_returns_the_callers_status_and_calls_nothing(rows, name):
    members = SETS[name]
    outside = [v for v in range(-3, 71) if v not in members]
    # Lo - 1, Hi + 1, 0, a negative value; for the lists a value between two members
    assert {min(members) - 1, max(members) + 1, 0, -1} <= set(outside)
    if name == "wide":
        assert {9, 24, 33, 63} <= set(outside)
    if name == "unordered":
        assert 3 in outside
    for v in outside:
        assert rows[name][v] == (NOT_FOUND, 0, -1000), (name, v)


def test_the_callable_keeps_its_state_and_its_return_value(rows):
    assert rows["state"][0][0] == 3 + 4              # 5 is outside 1..4: not called
    assert rows["same"][0][0] == NOT_FOUND           # the callable's own value, whatever it is
