"""The argument checks the C ABI's entry points share (csrc/glabc_check.h), on the CPU.  The header is a set of pure functions
of the descriptors of include/glabc.h, so a g++ driver evaluates them; the rows below say what each must answer.  They were
written by hand from the checks the entry points carried before the header existed (check_dist / check_model / check_run /
check_mala_chains of glabc_hip.hip, the checks glabc_rtc_steps of glabc_rtc.hip carried inline, pack_gen_dist / pack_common of
glabc_generic.hip) and are never printed from the header: a status code is behaviour, a caller tells the defects apart by it.

A row is (C++ statements that spoil the valid baseline `b`, expected status).  Every table starts from the untouched baseline,
which must return GLABC_OK."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4

PRELUDE = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include "glabc_check.h"
using namespace glabc;

static const float NaN = NAN, Inf = INFINITY;

static glabc_dist dist3(int kind)
{
    glabc_dist g;
    std::memset(&g, 0, sizeof g);
    g.kind = kind;
    g.dim = 3;
    for (int j = 0; j < 3; ++j) {
        if (kind == GLABC_DIST_GAMMA) { g.p0[j] = 2.0f + j; g.p1[j] = 0.5f; g.p2[j] = 2.0f; g.p3[j] = 0.25f * j; }      // shape, rate, scale, gammaln
        else if (kind == GLABC_DIST_UNIFORM) { g.p0[j] = -1.0f; g.p1[j] = 3.0f; g.p2[j] = 4.0f; }                    // low, high, high - low
        else { g.p0[j] = 0.5f - j; g.p1[j] = -0.6931472f; g.p2[j] = 0.5f; }                                          // loc, log_scale, scale
    }
    g.c0 = -2.7568155f;
    return g;
}

struct Base {
    glabc_dist g;
    glabc_model m;
    glabc_chains c;
    glabc_moments mo;
    glabc_run r;
    float f[4];
    double d[4];
    uint32_t u[4];
    Base()
    {
        g = dist3(GLABC_DIST_DIAG_GAUSS);
        std::memset(&m, 0, sizeof m);
        m.sim_kind = GLABC_SIM_ABS_GAUSS;
        m.theta_dim = m.y_dim = 3;
        m.gk_c = 0.8f;
        m.prior = dist3(GLABC_DIST_UNIFORM);
        m.noise = dist3(GLABC_DIST_DIAG_GAUSS);
        for (int j = 0; j < 3; ++j) m.y_obs[j] = 1.5f;
        m.kern_log_scale = -2.3025851f;
        m.kern_scale = 0.1f;
        m.kern_c0 = -0.9189385f;
        m.epsilon = 0.1f;
        std::memset(&c, 0, sizeof c);
        c.n_chains = 65;
        c.chain0 = 0;
        c.stride = 65;
        c.theta = f; c.y = f; c.log_w = f; c.flags = u; c.n_moves = nullptr;
        c.theta64 = d; c.y64 = d; c.log_w64 = d; c.grad = d;
        mo.sum_theta = d; mo.sum_outer = d; mo.sum_jump = d;
        std::memset(&r, 0, sizeof r);
        r.step0 = 1;
        r.n_steps = 3;
        r.global_frequency = 0.25f;
        r.batch_size = 5;
    }
};

// the g-and-k shape: theta_dim 4, y_dim 8, a prior of dimension 4
static void make_gk(Base& b)
{
    b.m.sim_kind = GLABC_SIM_GK;
    b.m.theta_dim = 4;
    b.m.y_dim = 8;
    b.m.prior.dim = 4;
    b.m.prior.p0[3] = -1.0f; b.m.prior.p1[3] = 3.0f; b.m.prior.p2[3] = 4.0f;
    for (int j = 0; j < 8; ++j) b.m.y_obs[j] = 0.5f * j;
}

int main()
{
"""


def run_rows(tmp_path_factory, name, calls, flags=()):
    """calls: [(spoiling statements, expression)] -> the expressions' values, each evaluated on a fresh baseline"""
    d = tmp_path_factory.mktemp(name)
    # a function per row: a compiler, and a sanitizer's instrumentation above all, takes long over one function of hundreds of scopes
    rows = "".join("static void row_%d() { Base b; %s std::printf(\"%%d\\n\", (int)(%s)); }\n" % (i, spoil, expr)
                   for i, (spoil, expr) in enumerate(calls))
    head, main = PRELUDE.split("int main()")
    body = "".join("    row_%d();\n" % i for i in range(len(calls)))
    (d / "checks.cpp").write_text(head + rows + "int main()" + main + body + "    return 0;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc"), str(d / "checks.cpp"), "-o", str(d / "checks")])
    run = subprocess.run([str(d / "checks")], capture_output=True, text=True, check=True)
    assert run.stderr == "", run.stderr                                    # a sanitizer's report
    out = run.stdout.split()
    assert len(out) == len(calls)
    return [int(x) for x in out]


def check_table(tmp_path_factory, name, rows, flags=()):
    """rows: [(spoil, expression, expected)]"""
    got = run_rows(tmp_path_factory, name, [(s, e) for s, e, _ in rows], flags)
    wrong = [(s, e, want, g) for (s, e, want), g in zip(rows, got) if g != want]
    assert not wrong, "(spoil, call, expected, returned): %r" % wrong


def test_header_needs_no_hip(tmp_path_factory):
    """glabc_check.h includes include/glabc.h, <cmath> and the shape of a run-time compiled program, glabc_rtc_kernels.h; that
    one the standard library and the two headers of integer rules, which include nothing but include/glabc.h"""
    def includes(name):
        src = open(os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc", name)).read()
        return [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes("glabc_check.h") == ["<cmath>", '"../../include/glabc.h"', '"glabc_rtc_kernels.h"']
    assert includes("glabc_rtc_kernels.h") == ["<cstdio>", "<string>", '"glabc_geometry.h"', '"glabc_plan.h"']
    assert includes("glabc_plan.h") == ['"../../include/glabc.h"', '"glabc_geometry.h"']
    assert includes("glabc_geometry.h") == ['"../../include/glabc.h"']


# ---- glabc_dist ------------------------------------------------------------------------------------------------------------
GAUSS, UNIFORM, GAMMA = "GLABC_DIST_DIAG_GAUSS", "GLABC_DIST_UNIFORM", "GLABC_DIST_GAMMA"


def dist_rows():
    rows = []

    def row(spoil, want, dim=3, allow=None):
        for a in ((False, True) if allow is None else (allow,)):
            rows.append((spoil, "check_dist(&b.g, %d, %s)" % (dim, "true" if a else "false"), want))

    row("", OK)                                                            # the baseline
    rows.append(("", "check_dist(&b.g, 3)", OK))                           # allow_gamma defaults to false
    rows.append(("b.g = dist3(%s);" % GAMMA, "check_dist(&b.g, 3)", KIND))
    rows.append(("", "check_dist(nullptr, 3, true)", NULL))
    rows.append(("", "check_dist(nullptr, 0, false)", NULL))
    # each kind, allowed and not
    row("b.g = dist3(%s);" % UNIFORM, OK)
    row("b.g = dist3(%s);" % GAMMA, OK, allow=True)
    row("b.g = dist3(%s);" % GAMMA, KIND, allow=False)
    row("b.g.kind = 3;", KIND)
    row("b.g.kind = -1;", KIND)
    # dimension: 0, 9, a mismatch with the expected one; expected 0 = any of 1..8
    for kind in (GAUSS, UNIFORM, GAMMA):
        k = "b.g = dist3(%s); " % kind
        row(k + "b.g.dim = 0;", DIM, allow=True)
        row(k + "b.g.dim = 9;", DIM, allow=True)
        row(k + "b.g.dim = 0;", DIM, dim=0, allow=True)
        row(k + "b.g.dim = 9;", DIM, dim=0, allow=True)
        row(k + "b.g.dim = -1;", DIM, dim=0, allow=True)
        row(k, DIM, dim=2, allow=True)
        row(k, DIM, dim=4, allow=True)
        row(k, OK, dim=0, allow=True)
        row(k + "b.g.dim = 1;", OK, dim=1, allow=True)
        row(k + "b.g.dim = 1;", OK, dim=0, allow=True)
    row("b.g = dist3(%s); b.g.dim = 8; for (int j = 3; j < 8; ++j) { b.g.p0[j] = -1.0f; b.g.p1[j] = 3.0f; b.g.p2[j] = 4.0f; }" % UNIFORM,
        OK, dim=8)
    # the dimension is looked at before the kind, the kind before the parameters
    row("b.g.kind = 3; b.g.dim = 9;", DIM)
    row("b.g = dist3(%s); b.g.dim = 2;" % GAMMA, DIM, allow=False)
    row("b.g.kind = 3; b.g.p0[0] = NaN;", KIND)
    row("b.g = dist3(%s); b.g.p0[0] = NaN;" % GAMMA, KIND, allow=False)
    # a NaN or an infinity in each parameter array: at the first and the last used coordinate, and one past it (ignored)
    for kind in (GAUSS, UNIFORM):
        k = "b.g = dist3(%s); " % kind
        for arr in ("p0", "p1", "p2"):
            for bad in ("NaN", "Inf", "-Inf"):
                row(k + "b.g.%s[0] = %s;" % (arr, bad), ARG)
                row(k + "b.g.%s[2] = %s;" % (arr, bad), ARG)
                row(k + "b.g.%s[3] = %s;" % (arr, bad), OK)
                row(k + "b.g.%s[7] = %s;" % (arr, bad), OK)
        for j in (0, 2, 3):
            row(k + "b.g.p3[%d] = NaN;" % j, OK)                           # gammaln(shape): a Gamma's only
        row(k + "b.g.c0 = NaN;", ARG)
        row(k + "b.g.c0 = Inf;", ARG)
        row(k + "b.g.c0 = -Inf;", ARG)
    # DiagGaussian: scale > 0; a Uniform's p2 = high - low is only finite
    for j, want in ((0, ARG), (2, ARG), (3, OK)):
        row("b.g.p2[%d] = 0.0f;" % j, want)
        row("b.g.p2[%d] = -0.5f;" % j, want)
        row("b.g = dist3(%s); b.g.p2[%d] = 0.0f;" % (UNIFORM, j), OK)
        row("b.g = dist3(%s); b.g.p2[%d] = -4.0f;" % (UNIFORM, j), OK)
    row("b.g.p0[0] = -3.0f; b.g.p1[2] = 0.0f;", OK)                        # loc, log_scale: any finite number
    # Gamma: shape, rate, scale > 0 and finite, gammaln(shape) finite; c0 is not read
    k = "b.g = dist3(%s); " % GAMMA
    for arr in ("p0", "p1", "p2"):
        for bad in ("0.0f", "-1.0f", "NaN", "Inf", "-Inf"):
            row(k + "b.g.%s[0] = %s;" % (arr, bad), ARG, allow=True)
            row(k + "b.g.%s[2] = %s;" % (arr, bad), ARG, allow=True)
            row(k + "b.g.%s[3] = %s;" % (arr, bad), OK, allow=True)
    for bad in ("NaN", "Inf", "-Inf"):
        row(k + "b.g.p3[0] = %s;" % bad, ARG, allow=True)
        row(k + "b.g.p3[2] = %s;" % bad, ARG, allow=True)
        row(k + "b.g.p3[3] = %s;" % bad, OK, allow=True)
    row(k + "b.g.p3[1] = -7.5f; b.g.p3[2] = 0.0f;", OK, allow=True)        # gammaln(shape): any finite number
    for bad in ("NaN", "Inf"):
        row(k + "b.g.c0 = %s;" % bad, OK, allow=True)
        row(k + "b.g.c0 = %s;" % bad, KIND, allow=False)
    return rows


def test_check_dist(tmp_path_factory):
    check_table(tmp_path_factory, "dist", dist_rows())


# ---- glabc_model -----------------------------------------------------------------------------------------------------------
def model_rows():
    """(spoil, expected) or (spoil, function of (allow_user_sim, allow_gamma_prior)), under each combination of the two flags"""
    user = "b.m.sim_kind = GLABC_SIM_USER; "
    gk = "make_gk(b); "
    gamma_prior = "b.m.prior = dist3(%s); " % GAMMA
    table = [
        ("", OK),
        (gk, OK),
        (user, lambda u, g: OK if u else KIND),
        ("b.m.sim_kind = 3;", KIND),
        ("b.m.sim_kind = -1;", KIND),
        ("b.m.sim_kind = 3; b.m.theta_dim = 0;", KIND),                     # the simulator's kind is looked at first ...
        (user + "b.m.theta_dim = 0;", lambda u, g: DIM if u else KIND),
        ("b.m.theta_dim = 0; b.m.prior.kind = 3;", DIM),                    # ... then the dimensions, then the prior
        (gamma_prior, lambda u, g: OK if g else KIND),
        (gk + "b.m.prior = dist3(%s); b.m.prior.dim = 4; b.m.prior.p0[3] = 1.0f; b.m.prior.p1[3] = 1.0f; b.m.prior.p2[3] = 1.0f;" % GAMMA,
         lambda u, g: OK if g else KIND),
        (user + gamma_prior, lambda u, g: KIND if not u else (OK if g else KIND)),
        (gamma_prior + "b.m.prior.p0[1] = 0.0f;", lambda u, g: ARG if g else KIND),
        ("b.m.prior.kind = 3;", KIND),
        ("b.m.prior.dim = 2;", DIM),
        ("b.m.prior.p0[2] = NaN;", ARG),
        ("b.m.prior.p0[3] = NaN;", OK),
        ("b.m.prior.c0 = Inf;", ARG),
        ("b.m.prior = dist3(%s); b.m.prior.p2[0] = 0.0f;" % GAUSS, ARG),
        # |theta| + noise: y_dim = theta_dim, a DiagGaussian noise of that dimension
        ("b.m.y_dim = 2;", lambda u, g: DIM),
        ("b.m.noise.dim = 2;", DIM),
        ("b.m.noise.dim = 0;", DIM),
        ("b.m.noise = dist3(%s);" % UNIFORM, KIND),
        ("b.m.noise = dist3(%s);" % GAMMA, KIND),
        ("b.m.noise.kind = 3;", KIND),
        ("b.m.noise.p2[2] = 0.0f;", ARG),
        ("b.m.noise.p0[0] = NaN;", ARG),
        ("b.m.noise.p0[3] = NaN;", OK),
        ("b.m.noise.c0 = NaN;", ARG),
        ("b.m.gk_c = NaN;", OK),                                            # the g-and-k constant is not read
        ("b.m.noise.kind = 3; b.m.kern_scale = 0.0f;", KIND),               # the noise before the kernel
        ("b.m.y_dim = 2; b.m.prior.p0[0] = NaN;", ARG),                     # the prior before the simulator's shape
        # g-and-k: the compiled shape (4, 8); the noise descriptor is not read
        (gk + "b.m.gk_c = NaN;", ARG),
        (gk + "b.m.gk_c = Inf;", ARG),
        (gk + "b.m.y_dim = 4;", DIM),
        (gk + "b.m.y_dim = 7;", DIM),
        (gk + "b.m.theta_dim = 3; b.m.prior.dim = 3;", DIM),
        (gk + "b.m.noise.kind = 3; b.m.noise.dim = 77; b.m.noise.p2[0] = NaN;", OK),
        (gk + "b.m.y_obs[7] = NaN;", ARG),
        # the caller's simulator (row-wise callbacks): neither the shape nor gk_c nor the noise is read
        (user + "b.m.y_dim = 5; for (int j = 0; j < 5; ++j) b.m.y_obs[j] = 0.0f;", lambda u, g: OK if u else KIND),
        (user + "b.m.noise.kind = 3; b.m.noise.dim = 77; b.m.noise.p2[0] = NaN; b.m.gk_c = NaN;", lambda u, g: OK if u else KIND),
        (user + "b.m.y_dim = 9;", lambda u, g: DIM if u else KIND),
        (user + "b.m.prior.dim = 2;", lambda u, g: DIM if u else KIND),
        (user + "b.m.kern_scale = 0.0f;", lambda u, g: ARG if u else KIND),
        (user + "b.m.kern_scale = Inf;", lambda u, g: ARG if u else KIND),
        (user + "b.m.y_obs[2] = NaN;", lambda u, g: ARG if u else KIND),
        (user + "b.m.y_obs[3] = NaN;", lambda u, g: OK if u else KIND),
        # dimensions
        ("b.m.theta_dim = 0;", DIM),
        ("b.m.theta_dim = 9;", DIM),
        ("b.m.theta_dim = -1;", DIM),
        ("b.m.y_dim = 0;", DIM),
        ("b.m.y_dim = 9;", DIM),
        ("b.m.theta_dim = 2;", DIM),                                        # the prior's dimension is 3
        # the ABC kernel and the observation
        ("b.m.kern_log_scale = NaN;", ARG),
        ("b.m.kern_log_scale = -Inf;", ARG),
        ("b.m.kern_scale = 0.0f;", ARG),
        ("b.m.kern_scale = -0.1f;", ARG),
        ("b.m.kern_scale = Inf;", ARG),
        ("b.m.kern_scale = NaN;", ARG),
        ("b.m.kern_c0 = Inf;", ARG),
        ("b.m.kern_c0 = NaN;", ARG),
        ("b.m.epsilon = NaN;", OK),                                         # GLMALA's own
        ("b.m.y_obs[0] = NaN;", ARG),
        ("b.m.y_obs[2] = Inf;", ARG),
        ("b.m.y_obs[3] = NaN;", OK),
    ]
    rows = []
    for spoil, want in table:
        for u in (False, True):
            for g in (False, True):
                rows.append((spoil, "check_model(&b.m, %s, %s)" % (str(u).lower(), str(g).lower()),
                             want(u, g) if callable(want) else want))
    rows += [("", "check_model(nullptr)", NULL), ("", "check_model(nullptr, true, true)", NULL),
             ("", "check_model(&b.m)", OK),                                 # both flags default to false
             ("b.m.sim_kind = GLABC_SIM_USER;", "check_model(&b.m)", KIND),
             ("b.m.prior = dist3(%s);" % GAMMA, "check_model(&b.m)", KIND),
             ("b.m.prior = dist3(%s);" % GAMMA, "check_model(&b.m, true)", KIND)]
    return rows


def test_check_model(tmp_path_factory):
    check_table(tmp_path_factory, "model", model_rows())


# ---- glabc_chains ----------------------------------------------------------------------------------------------------------
FORMS = {"CHAINS_PLAIN": ["theta", "y"], "CHAINS_ISIR": ["theta", "y", "log_w", "flags"],
         "CHAINS_MALA": ["theta", "y", "flags", "theta64", "y64", "log_w64", "grad"]}
POINTERS = ["theta", "y", "log_w", "flags", "n_moves", "theta64", "y64", "log_w64", "grad"]
RANGE = [("b.c.n_chains = -1;", ARG), ("b.c.stride = 64;", ARG), ("b.c.chain0 = -1;", ARG),
         ("b.c.n_chains = 0;", OK), ("b.c.n_chains = 0; b.c.stride = 0;", OK), ("b.c.stride = 66;", OK),
         ("b.c.chain0 = (int64_t)1 << 40;", OK), ("b.c.n_chains = 0; b.c.stride = -1;", ARG)]


def chain_rows():
    rows = []
    for form, required in FORMS.items():
        both, ptrs = "check_chains(&b.c, %s)" % form, "check_chain_pointers(&b.c, %s)" % form
        rows += [("", both, OK), ("", ptrs, OK),
                 ("", "check_chains(nullptr, %s)" % form, NULL), ("", "check_chain_pointers(nullptr, %s)" % form, NULL)]
        for p in POINTERS:
            want = NULL if p in required else OK
            rows += [("b.c.%s = nullptr;" % p, both, want), ("b.c.%s = nullptr;" % p, ptrs, want)]
        for spoil, want in RANGE:
            rows += [(spoil, both, want), (spoil, "check_chain_range(&b.c)", want), (spoil, ptrs, OK)]
        # a missing array is reported before a bad range
        rows.append(("b.c.%s = nullptr; b.c.n_chains = -1;" % required[-1], both, NULL))
    return rows


def test_check_chains(tmp_path_factory):
    check_table(tmp_path_factory, "chains", chain_rows())


# ---- glabc_run -------------------------------------------------------------------------------------------------------------
def run_rows_table():
    with_moments = "b.r.moments = &b.mo; "
    rows = [
        ("", "check_frequency(&b.r)", OK),
        ("b.r.global_frequency = NaN;", "check_frequency(&b.r)", ARG),
        ("b.r.global_frequency = -NaN;", "check_frequency(&b.r)", ARG),
        # any number is a frequency: below 0 never global, above 1 always
        ("b.r.global_frequency = 0.0f;", "check_frequency(&b.r)", OK),
        ("b.r.global_frequency = -1.0f;", "check_frequency(&b.r)", OK),
        ("b.r.global_frequency = 2.0f;", "check_frequency(&b.r)", OK),
        ("b.r.global_frequency = Inf;", "check_frequency(&b.r)", OK),
        ("b.r.global_frequency = -Inf;", "check_frequency(&b.r)", OK),
        # the history's stride, only where there is a history
        ("", "check_history(&b.r, 65)", OK),
        ("b.r.hist_stride = 64;", "check_history(&b.r, 65)", OK),
        ("b.r.history = b.f; b.r.hist_stride = 64;", "check_history(&b.r, 65)", ARG),
        ("b.r.history = b.f; b.r.hist_stride = 65;", "check_history(&b.r, 65)", OK),
        ("b.r.history = b.f; b.r.hist_stride = 66;", "check_history(&b.r, 65)", OK),
        ("b.r.history = b.f; b.r.hist_stride = 0;", "check_history(&b.r, 0)", OK),
        ("b.r.history = b.f; b.r.hist_stride = -1;", "check_history(&b.r, 0)", ARG),
        # the three moment arrays
        ("", "check_moments(&b.r)", OK),
        (with_moments, "check_moments(&b.r)", OK),
        (with_moments + "b.mo.sum_theta = nullptr;", "check_moments(&b.r)", NULL),
        (with_moments + "b.mo.sum_outer = nullptr;", "check_moments(&b.r)", NULL),
        (with_moments + "b.mo.sum_jump = nullptr;", "check_moments(&b.r)", NULL),
        ("b.mo.sum_jump = nullptr;", "check_moments(&b.r)", OK),            # not attached to the run
        # the 32-bit step counter: step0 + n_steps = 2^32 is refused, 2^32 - 1 accepted
        ("", "check_step_counter(&b.r)", OK),
        ("b.r.step0 = 0xFFFFFFFFu; b.r.n_steps = 1;", "check_step_counter(&b.r)", ARG),
        ("b.r.step0 = 0xFFFFFFFFu; b.r.n_steps = 0;", "check_step_counter(&b.r)", OK),
        ("b.r.step0 = 0xFFFFFFFEu; b.r.n_steps = 1;", "check_step_counter(&b.r)", OK),
        ("b.r.step0 = 0xFFFFFFFEu; b.r.n_steps = 2;", "check_step_counter(&b.r)", ARG),
        ("b.r.step0 = 0x80000001u; b.r.n_steps = 0x7FFFFFFF;", "check_step_counter(&b.r)", ARG),
        ("b.r.step0 = 0x80000000u; b.r.n_steps = 0x7FFFFFFF;", "check_step_counter(&b.r)", OK),
        ("b.r.step0 = 0; b.r.n_steps = 0x7FFFFFFF;", "check_step_counter(&b.r)", OK),
        ("b.r.step0 = 0; b.r.n_steps = 0;", "check_step_counter(&b.r)", OK),
    ]
    # lanes_per_chain: every value from 0 to 65 (and a negative one) against both sets
    for lanes in [-1] + list(range(0, 66)):
        rows.append(("", "check_lanes(%d)" % lanes, OK if lanes in (0, 1, 2, 4) else ARG))
        rows.append(("", "check_lanes_wide(%d)" % lanes, OK if lanes in (0, 8, 16, 32, 64) else ARG))
    return rows


def test_check_run(tmp_path_factory):
    check_table(tmp_path_factory, "run", run_rows_table())


# ---- glabc_rtc_steps -------------------------------------------------------------------------------------------------------
# the baseline as a launch of a run-time compiled program: the caller's simulator, a local and a global proposal, and the shape
# the program was compiled for -- {algo, theta_dim, y_dim, noise_dim, batch_size, lanes, wide, gamma, hooks}
RTC_BASE = ("b.m.sim_kind = GLABC_SIM_USER; glabc_dist lo = dist3(%s), gl = dist3(%s); " % (GAUSS, GAUSS) +
            "RtcShape p = {GLABC_ALGO_GLMCMC, 3, 3, 3, 5, 1, 0, 0, 0}; ")
RTC_CALL = "check_rtc_run(p, &b.m, &lo, &gl, &b.c, &b.r)"
RTC_GLOBAL = "p.algo = GLABC_ALGO_GLOBALMCMC; p.batch_size = 1; "
RTC_WIDE = "p.batch_size = 0; p.lanes = 0; p.wide = 1; b.r.batch_size = 17; "
RTC_GAMMA = "p.gamma = 1; "


def rtc_rows():
    rows = []

    def row(spoil, want, call=RTC_CALL):
        rows.append((RTC_BASE + spoil, call, want))

    def every_program(spoil, want):
        for program in ("", RTC_GLOBAL, RTC_WIDE, RTC_GAMMA, RTC_WIDE + RTC_GAMMA, RTC_GLOBAL + RTC_GAMMA):
            row(program + spoil, want)

    every_program("", OK)
    every_program("p.lanes = p.wide ? 0 : 4; p.hooks = 1;", OK)                 # neither is a matter of the launch
    # null pointers first; a missing proposal is a defect of a descriptor
    for call in ("check_rtc_run(p, nullptr, &lo, &gl, &b.c, &b.r)", "check_rtc_run(p, &b.m, &lo, &gl, nullptr, &b.r)",
                 "check_rtc_run(p, &b.m, &lo, &gl, &b.c, nullptr)", "check_rtc_run(p, nullptr, nullptr, nullptr, nullptr, nullptr)"):
        row("", NULL, call)
        row("b.m.sim_kind = GLABC_SIM_GK; b.m.theta_dim = 2;", NULL, call)
    row("", ARG, "check_rtc_run(p, &b.m, nullptr, &gl, &b.c, &b.r)")
    row("", ARG, "check_rtc_run(p, &b.m, &lo, nullptr, &b.c, &b.r)")
    row("b.m.theta_dim = 2;", DIM, "check_rtc_run(p, &b.m, nullptr, nullptr, &b.c, &b.r)")
    # the caller's simulator, then the program's dimensions; the noise descriptor gives the normals per simulation and no more
    every_program("b.m.sim_kind = GLABC_SIM_ABS_GAUSS;", KIND)
    row("b.m.sim_kind = GLABC_SIM_GK;", KIND)
    row("b.m.sim_kind = GLABC_SIM_ABS_GAUSS; b.m.theta_dim = 2;", KIND)
    every_program("b.m.theta_dim = 2;", DIM)
    row("b.m.y_dim = 2;", DIM)
    row("b.m.noise.dim = 2;", DIM)
    row("p.theta_dim = 4;", DIM)
    row("p.y_dim = 4;", DIM)
    row("p.noise_dim = 4;", DIM)
    row("p.noise_dim = 2; b.m.noise.dim = 2;", OK)
    row("b.m.noise.kind = 3; b.m.noise.p2[0] = NaN; b.m.noise.c0 = NaN; b.m.gk_c = NaN;", OK)
    row("b.m.y_dim = 2; b.m.prior.p0[0] = NaN;", DIM)
    # the prior, `local`, `global`: GLABC_ERR_ARG whatever check_dist finds
    for d in ("b.m.prior", "lo", "gl"):
        every_program(d + ".dim = 2;", ARG)                                     # check_dist: GLABC_ERR_DIM
        every_program(d + ".kind = 3;", ARG)                                    # check_dist: GLABC_ERR_KIND
        row(d + ".p0[0] = NaN;", ARG)
        row(d + ".p0[3] = NaN;", OK)
        row(d + ".c0 = Inf;", ARG)
    row("b.m.prior.c0 = NaN;", ARG)                                             # a Uniform prior's constant
    row("lo.p2[2] = 0.0f;", ARG)
    row("b.m.prior.p2[2] = 0.0f;", OK)                                          # high - low of a Uniform: only finite
    # a Gamma: the prior and the global proposal of a program that holds the Gamma kernels; `local` never
    for program in ("", RTC_GLOBAL, RTC_WIDE):
        for d in ("b.m.prior", "gl"):
            row(program + d + " = dist3(%s);" % GAMMA, ARG)
            row(program + RTC_GAMMA + d + " = dist3(%s);" % GAMMA, OK)
            row(program + RTC_GAMMA + d + " = dist3(%s); %s.p1[1] = 0.0f;" % (GAMMA, d), ARG)
        row(program + RTC_GAMMA + "b.m.prior = dist3(%s); gl = dist3(%s);" % (GAMMA, GAMMA), OK)
        row(program + "lo = dist3(%s);" % GAMMA, ARG)
        row(program + RTC_GAMMA + "lo = dist3(%s);" % GAMMA, ARG)
    row("b.m.sim_kind = GLABC_SIM_GK; gl = dist3(%s);" % GAMMA, KIND)
    # the ABC kernel: a finite log scale and constant, a scale above zero (an infinite one passes here); y_obs is not read
    for spoil, want in (("b.m.kern_log_scale = NaN;", ARG), ("b.m.kern_log_scale = -Inf;", ARG), ("b.m.kern_scale = 0.0f;", ARG),
                        ("b.m.kern_scale = -0.1f;", ARG), ("b.m.kern_scale = NaN;", ARG), ("b.m.kern_scale = Inf;", OK),
                        ("b.m.kern_c0 = NaN;", ARG), ("b.m.kern_c0 = Inf;", ARG), ("b.m.y_obs[0] = NaN;", OK), ("b.m.epsilon = NaN;", OK)):
        row(spoil, want)
    row("gl.kind = 3; b.m.kern_scale = 0.0f; b.c.theta = nullptr;", ARG)
    row("b.m.kern_scale = 0.0f; b.c.theta = nullptr;", ARG)                     # the kernel before the chains
    # the chains: iSIR arrays for GLMCMC (register and wide), theta and y for GlobalMCMC
    for program, required in (("", FORMS["CHAINS_ISIR"]), (RTC_WIDE, FORMS["CHAINS_ISIR"]), (RTC_GLOBAL, FORMS["CHAINS_PLAIN"])):
        for ptr in POINTERS:
            row(program + "b.c.%s = nullptr;" % ptr, NULL if ptr in required else OK)
        for spoil, want in RANGE:
            row(program + spoil, want)
        row(program + "b.c.theta = nullptr; b.c.n_chains = -1;", NULL)
        row(program + "b.c.y = nullptr; b.r.n_steps = -1;", NULL)               # the chains before n_steps
        row(program + "b.r.n_steps = -1;", ARG)
        row(program + "b.r.n_steps = 0;", OK)
        row(program + "b.r.n_steps = -1; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)
    # a wide program: batch sizes 17..4096, lane groups of 8 / 16 / 32 / 64, neither a tape nor a device step counter
    for n, want in ((0, ARG), (5, ARG), (16, ARG), (17, OK), (64, OK), (4096, OK), (4097, ARG), (-1, ARG)):
        row(RTC_WIDE + "b.r.batch_size = %d;" % n, want)
        row(RTC_WIDE + RTC_GAMMA + "b.r.batch_size = %d;" % n, want)
    for lanes in (-1, 0, 1, 2, 4, 7, 8, 9, 16, 32, 64, 65, 128):
        row(RTC_WIDE + "b.r.lanes_per_chain = %d;" % lanes, OK if lanes in (0, 8, 16, 32, 64) else ARG)
    # a register program: GLMCMC at the compiled batch size, GlobalMCMC at any; one lane per chain or the library's choice
    for n, want in ((4, ARG), (5, OK), (6, ARG), (1, ARG), (16, ARG), (17, ARG), (0, ARG)):
        row("b.r.batch_size = %d;" % n, want)
    row("p.batch_size = 16; b.r.batch_size = 16;", OK)
    row("p.batch_size = 16;", ARG)
    for n in (0, 1, 5, 16, 17, 4097, -3):
        row(RTC_GLOBAL + "b.r.batch_size = %d;" % n, OK)
    for program in ("", RTC_GLOBAL, RTC_GAMMA):
        for lanes in (-1, 0, 1, 2, 4, 8, 64):
            row(program + "b.r.lanes_per_chain = %d;" % lanes, OK if lanes in (0, 1) else ARG)
        row(program + "p.lanes = 2; b.r.lanes_per_chain = 2;", ARG)             # whatever the entry was compiled for
    for program in ("", RTC_GLOBAL, RTC_WIDE):
        row(program + "glabc_tape t = {}; b.r.tape = &t;", ARG)
        row(program + "b.r.step0_device = b.u;", ARG)
        # exact arithmetic only, and nowhere to write draws
        row(program + "b.r.math_mode = GLABC_MATH_FAST;", ARG)
        row(program + "b.r.math_mode = 2;", ARG)
        row(program + "glabc_draws_out o = {}; b.r.dump_draws = &o;", ARG)
        # what every stepping entry point asks, in its order: frequency, history, moments, step counter
        row(program + "b.r.global_frequency = NaN;", ARG)
        row(program + "b.r.global_frequency = Inf;", OK)
        row(program + "b.r.history = b.f; b.r.hist_stride = 64;", ARG)
        row(program + "b.r.history = b.f; b.r.hist_stride = 65;", OK)
        row(program + "b.r.hist_stride = 64;", OK)
        row(program + "b.r.moments = &b.mo;", OK)
        for arr in ("sum_theta", "sum_outer", "sum_jump"):
            row(program + "b.r.moments = &b.mo; b.mo.%s = nullptr;" % arr, NULL)
        row(program + "b.r.step0 = 0xFFFFFFFEu; b.r.n_steps = 1;", OK)
        row(program + "b.r.step0 = 0xFFFFFFFEu; b.r.n_steps = 2;", ARG)
        row(program + "b.r.math_mode = GLABC_MATH_FAST; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)
        row(program + "b.r.history = b.f; b.r.hist_stride = 64; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)
        row(program + "b.r.moments = &b.mo; b.mo.sum_jump = nullptr; b.r.step0 = 0xFFFFFFFFu; b.r.n_steps = 1;", NULL)
        row(program + "b.r.lanes_per_chain = 3; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)
    return rows


def test_check_rtc_run(tmp_path_factory):
    """the statuses of glabc_rtc_steps; the table's driver is built with the address and undefined-behaviour sanitizers"""
    check_table(tmp_path_factory, "rtc", rtc_rows(), flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
