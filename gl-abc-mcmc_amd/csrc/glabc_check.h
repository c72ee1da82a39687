// glabc_check.h -- the argument checks the entry points of include/glabc.h share, as pure functions of the descriptors
// (no HIP: tests/test_arg_checks.py compiles this header with g++; glabc_rtc_kernels.h is host only too).  Each returns GLABC_OK or the status the entry point
// returns; an entry point calls them in the order its own contract lists the checks and keeps inline what only it asks.
#pragma once

#include <cmath>

#include "../../include/glabc.h"
#include "glabc_rtc_kernels.h"

namespace glabc {

// allow_gamma: GLABC_DIST_GAMMA is known where include/glabc.h says so (importance / global proposal and prior of
// glabc_glmcmc_steps / glabc_globalmcmc_steps / glabc_init_weights, glabc_dist_log_prob, the row-wise Model callbacks, the
// global proposal of the split-phase entry points).  dim: the dimension the caller expects, or 0 for any of 1..GLABC_MAX_DIM
inline int check_dist(const glabc_dist* g, int dim, bool allow_gamma = false)
{
    if (!g) return GLABC_ERR_NULL;
    if (g->dim < 1 || g->dim > GLABC_MAX_DIM || (dim > 0 && g->dim != dim)) return GLABC_ERR_DIM;
    if (g->kind == GLABC_DIST_GAMMA) {
        if (!allow_gamma) return GLABC_ERR_KIND;
        for (int j = 0; j < g->dim; ++j)            // shape, rate, scale = 1/rate > 0 and finite; gammaln(shape) finite
            if (!(g->p0[j] > 0.0f) || !std::isfinite(g->p0[j]) || !(g->p1[j] > 0.0f) || !std::isfinite(g->p1[j]) ||
                !(g->p2[j] > 0.0f) || !std::isfinite(g->p2[j]) || !std::isfinite(g->p3[j]))
                return GLABC_ERR_ARG;
        return GLABC_OK;
    }
    if (g->kind != GLABC_DIST_DIAG_GAUSS && g->kind != GLABC_DIST_UNIFORM) return GLABC_ERR_KIND;
    for (int j = 0; j < g->dim; ++j) {
        if (!std::isfinite(g->p0[j]) || !std::isfinite(g->p1[j]) || !std::isfinite(g->p2[j])) return GLABC_ERR_ARG;
        if (g->kind == GLABC_DIST_DIAG_GAUSS && !(g->p2[j] > 0.0f)) return GLABC_ERR_ARG;
    }
    return std::isfinite(g->c0) ? GLABC_OK : GLABC_ERR_ARG;
}

// allow_user_sim: the row-wise callbacks, where the simulator is not involved
inline int check_model(const glabc_model* m, bool allow_user_sim = false, bool allow_gamma_prior = false)
{
    if (!m) return GLABC_ERR_NULL;
    const bool user = allow_user_sim && m->sim_kind == GLABC_SIM_USER;
    if (!user && m->sim_kind != GLABC_SIM_ABS_GAUSS && m->sim_kind != GLABC_SIM_GK) return GLABC_ERR_KIND;
    if (m->theta_dim < 1 || m->theta_dim > GLABC_MAX_DIM || m->y_dim < 1 || m->y_dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    int rc = check_dist(&m->prior, m->theta_dim, allow_gamma_prior);
    if (rc) return rc;
    if (user) {
        // neither gk_c nor the noise descriptor is read
    } else if (m->sim_kind == GLABC_SIM_GK) {
        if (m->theta_dim != 4 || m->y_dim != 8) return GLABC_ERR_DIM;          // the compiled g-and-k shape
        if (!std::isfinite(m->gk_c)) return GLABC_ERR_ARG;
    } else {
        if (m->y_dim != m->theta_dim) return GLABC_ERR_DIM;
        rc = check_dist(&m->noise, m->y_dim);
        if (rc) return rc;
        if (m->noise.kind != GLABC_DIST_DIAG_GAUSS) return GLABC_ERR_KIND;
    }
    if (!std::isfinite(m->kern_log_scale) || !(m->kern_scale > 0.0f) || !std::isfinite(m->kern_scale) ||
        !std::isfinite(m->kern_c0))
        return GLABC_ERR_ARG;
    for (int j = 0; j < m->y_dim; ++j)
        if (!std::isfinite(m->y_obs[j])) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_chains ------------------------------------------------------------------------------------------------------
// the arrays an algorithm reads: theta and y always, log_w and flags for iSIR, the float64 state and flags for GLMALA
enum ChainForm { CHAINS_PLAIN = 0, CHAINS_ISIR = 1, CHAINS_MALA = 2 };

inline int check_chain_pointers(const glabc_chains* c, ChainForm form)
{
    if (!c || !c->theta || !c->y) return GLABC_ERR_NULL;
    if (form == CHAINS_ISIR && (!c->log_w || !c->flags)) return GLABC_ERR_NULL;
    if (form == CHAINS_MALA && (!c->flags || !c->theta64 || !c->y64 || !c->log_w64 || !c->grad)) return GLABC_ERR_NULL;
    return GLABC_OK;
}

inline int check_chain_range(const glabc_chains* c)
{
    return (c->n_chains < 0 || c->stride < c->n_chains || c->chain0 < 0) ? GLABC_ERR_ARG : GLABC_OK;
}

inline int check_chains(const glabc_chains* c, ChainForm form)
{
    const int rc = check_chain_pointers(c, form);
    return rc ? rc : check_chain_range(c);
}

// ---- glabc_run: what every stepping entry point asks ---------------------------------------------------------------------
inline int check_frequency(const glabc_run* r)
{
    return (!(r->global_frequency >= 0.0f) && !(r->global_frequency < 0.0f)) ? GLABC_ERR_ARG : GLABC_OK;      // NaN
}

inline int check_history(const glabc_run* r, int64_t n_chains)
{
    return (r->history && r->hist_stride < n_chains) ? GLABC_ERR_ARG : GLABC_OK;
}

inline int check_moments(const glabc_run* r)
{
    return (r->moments && (!r->moments->sum_theta || !r->moments->sum_outer || !r->moments->sum_jump)) ? GLABC_ERR_NULL : GLABC_OK;
}

// the Philox step counter is 32 bits wide
inline int check_step_counter(const glabc_run* r)
{
    return ((uint64_t)r->step0 + (uint64_t)r->n_steps > 0xFFFFFFFFull) ? GLABC_ERR_ARG : GLABC_OK;
}

// lanes_per_chain, 0 = the library chooses: the lane-group kernel (batch sizes > GLABC_MAX_BATCH) and the register kernels
inline int check_lanes_wide(int lanes)
{
    return (lanes == 0 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64) ? GLABC_OK : GLABC_ERR_ARG;
}

inline int check_lanes(int lanes) { return (lanes == 0 || lanes == 1 || lanes == 2 || lanes == 4) ? GLABC_OK : GLABC_ERR_ARG; }

// ---- glabc_mixture (include/glabc.h) ---------------------------------------------------------------------------------------------
// dim: the dimension the caller expects, or 0 for any of 1..GLABC_MAX_DIM
inline int check_mixture(const glabc_mixture* g, int dim)
{
    if (!g) return GLABC_ERR_NULL;
    if (g->n_modes < 1 || g->n_modes > GLABC_MAX_MODES) return GLABC_ERR_ARG;
    if (g->dim < 1 || g->dim > GLABC_MAX_DIM || (dim > 0 && g->dim != dim)) return GLABC_ERR_DIM;
    for (int k = 0; k < g->n_modes; ++k) {
        for (int q = 0; q < g->dim; ++q)
            if (!std::isfinite(g->loc[k][q]) || !(g->scale[k][q] > 0.0) || !std::isfinite(g->scale[k][q]) ||
                !(g->inv_scale[k][q] > 0.0) || !std::isfinite(g->inv_scale[k][q]))
                return GLABC_ERR_ARG;
        // log_weight may be -inf (a mode of weight 0), never NaN or +inf
        if (!(g->log_weight[k] < INFINITY) || !std::isfinite(g->sum_log_scale[k])) return GLABC_ERR_ARG;
        if (!(g->cum_weight[k] >= (k ? g->cum_weight[k - 1] : 0.0))) return GLABC_ERR_ARG;           // monotone, no NaN
    }
    const double last = g->cum_weight[g->n_modes - 1];
    if (!(last > 0.0) || !(last <= 1.0 + 1e-9)) return GLABC_ERR_ARG;
    return std::isfinite(g->c0) ? GLABC_OK : GLABC_ERR_ARG;
}

// glabc_glmcmc_mix_steps / glabc_globalmcmc_mix_steps: the support matrix of the mixture variant (include/glabc.h)
inline int check_mix_model(const glabc_model* m, const glabc_mixture* g)
{
    if (int e = check_model(m, false, true)) return e;
    if (m->prior.kind == GLABC_DIST_GAMMA) return GLABC_ERR_KIND;
    if (m->sim_kind == GLABC_SIM_ABS_GAUSS && m->theta_dim > 4) return GLABC_ERR_KIND;               // instantiated up to 4, and g-and-k
    return check_mixture(g, m->theta_dim);
}

// what the stepping entry points of the mixture variant share, in one order; wide: the batch sizes and lanes per chain of the
// lane-group kernel instead of the register kernels'
inline int check_mix_steps(const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c,
                           const glabc_run* r, bool isir, bool wide)
{
    if (int e = check_mix_model(m, g)) return e;
    if (int e = check_dist(local, m->theta_dim)) return e;
    if (!c || !r) return GLABC_ERR_NULL;
    if (r->tape) return GLABC_ERR_ARG;                          // a tape has no mode draws
    if (int e = check_chains(c, isir ? CHAINS_ISIR : CHAINS_PLAIN)) return e;
    if (r->n_steps < 0) return GLABC_ERR_ARG;
    if (int e = check_frequency(r)) return e;
    const int n_lo = wide ? GLABC_MAX_BATCH + 1 : 1, n_hi = wide ? GLABC_MAX_BATCH_WIDE : GLABC_MAX_BATCH;
    if (isir && (r->batch_size < n_lo || r->batch_size > n_hi)) return GLABC_ERR_ARG;
    if (wide ? check_lanes_wide(r->lanes_per_chain) != GLABC_OK : (r->lanes_per_chain != 0 && r->lanes_per_chain != 1)) return GLABC_ERR_ARG;
    if (int e = check_history(r, c->n_chains)) return e;
    if (int e = check_moments(r)) return e;
    if (int e = check_step_counter(r)) return e;
    if (r->step0_device) return GLABC_ERR_ARG;                  // the split-phase entry points only
    if (r->math_mode != GLABC_MATH_EXACT || r->dump_draws) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// glabc_glmcmc_mix_steps (isir: batch sizes 1..GLABC_MAX_BATCH) / glabc_globalmcmc_mix_steps: one lane per chain
inline int check_mix_run(const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c,
                         const glabc_run* r, bool isir)
{
    return check_mix_steps(m, local, g, c, r, isir, false);
}

// glabc_glmcmc_mix_wide_steps: batch sizes GLABC_MAX_BATCH + 1..GLABC_MAX_BATCH_WIDE in lane groups of 8 / 16 / 32 / 64 (0: the
// library chooses); the rest of the matrix is check_mix_run's
inline int check_mix_wide_run(const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c,
                              const glabc_run* r)
{
    return check_mix_steps(m, local, g, c, r, true, true);
}

// ---- glabc_glmala_mix_steps: glabc_glmala_steps' checks in glabc_glmala_steps' order, with the mixture's own where that entry point
// checks its importance proposal.  The order is the contract (include/glabc.h): the model (a Gamma prior is GLABC_ERR_KIND there),
// the simulator kind, theta_dim 5..8 (GLABC_ERR_DIM: no kernel is instantiated; glabc_glmala_steps finds that out last), the mixture,
// null mala / run, the chains, n_steps and the batch size, global_frequency, global_frequency_per_chain, the MALA parameters,
// history, moments, tape / math mode / dump_draws, lanes_per_chain, the step counter.
inline int check_mala_params(const glabc_mala* p)
{
    return (p->num_grad < 2 || p->num_grad > (1 << 16) || !(p->tau > 0.0) || !std::isfinite(p->tau) || !std::isfinite(p->tau_sq) ||
            !std::isfinite(p->eps_sq) || !(p->eps_sq >= 0.0))
               ? GLABC_ERR_ARG
               : GLABC_OK;
}

inline int check_mala_mix_run(const glabc_model* m, const glabc_mixture* g, const glabc_mala* p, const glabc_chains* c, const glabc_run* r)
{
    if (int e = check_model(m)) return e;
    if (m->sim_kind != GLABC_SIM_ABS_GAUSS) return GLABC_ERR_KIND;
    if (m->theta_dim > 4) return GLABC_ERR_DIM;
    if (int e = check_mixture(g, m->theta_dim)) return e;
    if (!p || !r) return GLABC_ERR_NULL;
    if (int e = check_chains(c, CHAINS_MALA)) return e;
    if (r->n_steps < 0 || r->batch_size < 1 || r->batch_size > GLABC_MAX_BATCH) return GLABC_ERR_ARG;
    if (int e = check_frequency(r)) return e;
    if (r->global_frequency_per_chain) return GLABC_ERR_ARG;        // GLMCMC / GlobalMCMC only
    if (int e = check_mala_params(p)) return e;
    if (int e = check_history(r, c->n_chains)) return e;
    if (int e = check_moments(r)) return e;
    if (r->tape || r->math_mode != GLABC_MATH_EXACT || r->dump_draws) return GLABC_ERR_ARG;
    if (r->lanes_per_chain < 0 || r->lanes_per_chain > 2) return GLABC_ERR_ARG;      // wavefronts per 64 chains (theta_dim 2)
    return check_step_counter(r);
}

// ---- glabc_propose_mix: the mixture's checks in the order glabc_glmcmc_mix_steps makes them (the mixture, the local increment, the
// pointers, a tape), ahead of glabc_propose's own, which the entry point makes next.  io gives the dimension the mixture must have;
// local may be null as for glabc_propose (the caller then fills the local move's row); io->q_cur is written, so it must be there
inline int check_propose_mix(int algo, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c, const glabc_run* r,
                             const glabc_step_io* io)
{
    if (!io) return GLABC_ERR_NULL;
    if (algo != GLABC_ALGO_GLMCMC && algo != GLABC_ALGO_GLOBALMCMC) return GLABC_ERR_KIND;
    if (io->theta_dim < 1 || io->theta_dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    if (int e = check_mixture(g, io->theta_dim)) return e;
    if (local)
        if (int e = check_dist(local, io->theta_dim)) return e;
    if (!c || !r) return GLABC_ERR_NULL;
    if (r->tape) return GLABC_ERR_ARG;                          // a tape has no mode draws
    if (!io->q_cur) return GLABC_ERR_NULL;
    return GLABC_OK;
}

// ---- glabc_autocov: a chain-major history and its two dense outputs, in the order include/glabc.h lists the refusals ----------------
inline int check_autocov(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t max_lag,
                         const double* mean_out, const double* acov_out)
{
    if (!history || !mean_out || !acov_out) return GLABC_ERR_NULL;
    if (theta_dim < 1 || theta_dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    if (n_rows < 1 || n_chains < 0 || stride < n_chains) return GLABC_ERR_ARG;
    if (max_lag < 0 || max_lag > n_rows - 1 || max_lag > GLABC_MAX_LAG) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_key_counts / glabc_histogram: the history of glabc_autocov and a table of counts, in the order include/glabc.h lists
// the refusals.  The levels of the radix selection: (prefix bits, digit bits) = (0, 11), (11, 11), (22, 10)
constexpr int key_prefix_bits(int level) { return 11 * level; }
constexpr int key_digit_bits(int level) { return level == 2 ? 10 : 11; }
constexpr uint32_t KEY_UNUSED_SLOT = 0xFFFFFFFFu;

inline int check_counts_history(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride,
                                const void* host_table, const void* host_table2, const uint64_t* counts)
{
    if (!history || !host_table || !host_table2 || !counts) return GLABC_ERR_NULL;
    if (theta_dim < 1 || theta_dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    if (n_rows < 1 || n_chains < 0 || stride < n_chains) return GLABC_ERR_ARG;
    return GLABC_OK;
}

inline int check_key_counts(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t level,
                            int32_t n_prefixes, const uint32_t* prefixes, const uint64_t* counts)
{
    if (int e = check_counts_history(history, n_rows, theta_dim, n_chains, stride, prefixes, prefixes, counts)) return e;
    if (level < 0 || level > 2) return GLABC_ERR_ARG;
    if (n_prefixes < 1 || n_prefixes > GLABC_MAX_PREFIXES || (level == 0 && n_prefixes != 1)) return GLABC_ERR_ARG;
    if (level == 0) return GLABC_OK;                              // the prefix word is ignored
    for (int j = 0; j < theta_dim; ++j)
        for (int s = 0; s < n_prefixes; ++s) {
            const uint32_t p = prefixes[j * n_prefixes + s];
            if (p == KEY_UNUSED_SLOT) continue;
            if ((p >> key_prefix_bits(level)) != 0) return GLABC_ERR_ARG;
            for (int q = 0; q < s; ++q)
                if (prefixes[j * n_prefixes + q] == p) return GLABC_ERR_ARG;
        }
    return GLABC_OK;
}

inline int check_histogram(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_bins,
                           const double* lo, const double* hi, const uint64_t* counts)
{
    if (int e = check_counts_history(history, n_rows, theta_dim, n_chains, stride, lo, hi, counts)) return e;
    if (n_bins < 1 || n_bins > GLABC_MAX_BINS) return GLABC_ERR_ARG;
    for (int j = 0; j < theta_dim; ++j)
        if (!std::isfinite(lo[j]) || !std::isfinite(hi[j]) || !(lo[j] < hi[j])) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_histogram2d / glabc_cross_moments: the same history, in the order include/glabc.h lists the refusals.  lo and hi are
// looked at for the coordinates a pair uses only
inline int check_histogram2d(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_pairs,
                             const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, const uint64_t* counts)
{
    if (!pairs) return GLABC_ERR_NULL;
    if (int e = check_counts_history(history, n_rows, theta_dim, n_chains, stride, lo, hi, counts)) return e;
    if (n_pairs < 1 || n_pairs > GLABC_MAX_PAIRS) return GLABC_ERR_ARG;
    for (int p = 0; p < n_pairs; ++p) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= theta_dim || b < 0 || b >= theta_dim || a == b) return GLABC_ERR_ARG;
    }
    if (n_bins < 1 || n_bins > GLABC_MAX_JOINT_BINS) return GLABC_ERR_ARG;
    for (int q = 0; q < 2 * n_pairs; ++q) {
        const int32_t j = pairs[q];
        if (!std::isfinite(lo[j]) || !std::isfinite(hi[j]) || !(lo[j] < hi[j])) return GLABC_ERR_ARG;
    }
    return GLABC_OK;
}

inline int check_cross_moments(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride,
                               const double* mean_out, const double* cov_out)
{
    return check_autocov(history, n_rows, theta_dim, n_chains, stride, 0, mean_out, cov_out);
}

// ---- glabc_weighted_key_counts / glabc_weighted_histogram / glabc_weighted_histogram2d: the twins' refusals in the twins' order on
// the one-row history [1][dim][stride] of n draws (a null weight array is a null pointer like the others), then what the weights
// add: more than GLABC_MAX_WEIGHTED_DRAWS draws (n < 0 and stride < n are the twins' own), a scale that is not finite or not > 0
inline int check_weight_scale(int64_t n, double scale)
{
    return (n > GLABC_MAX_WEIGHTED_DRAWS || !std::isfinite(scale) || !(scale > 0.0)) ? GLABC_ERR_ARG : GLABC_OK;
}

inline int check_weighted_key_counts(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t level,
                                     int32_t n_prefixes, const uint32_t* prefixes, const uint64_t* counts)
{
    if (!w) return GLABC_ERR_NULL;
    if (int e = check_key_counts(x, 1, dim, n, stride, level, n_prefixes, prefixes, counts)) return e;
    return check_weight_scale(n, scale);
}

inline int check_weighted_histogram(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t n_bins,
                                    const double* lo, const double* hi, const uint64_t* counts)
{
    if (!w) return GLABC_ERR_NULL;
    if (int e = check_histogram(x, 1, dim, n, stride, n_bins, lo, hi, counts)) return e;
    return check_weight_scale(n, scale);
}

inline int check_weighted_histogram2d(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t n_pairs,
                                      const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, const uint64_t* counts)
{
    if (!w) return GLABC_ERR_NULL;
    if (int e = check_histogram2d(x, 1, dim, n, stride, n_pairs, pairs, n_bins, lo, hi, counts)) return e;
    return check_weight_scale(n, scale);
}

// ---- glabc_weighted_gram / glabc_regression_apply: the dimension-major rows of glabc_abc_draws, in the order include/glabc.h lists
// the refusals.  Both dimensions are free in 1 .. GLABC_MAX_DIM; a NaN delta fails `delta > 0`, +inf passes
inline int check_regress_dims(int32_t theta_dim, int32_t y_dim)
{
    return (theta_dim < 1 || theta_dim > GLABC_MAX_DIM || y_dim < 1 || y_dim > GLABC_MAX_DIM) ? GLABC_ERR_DIM : GLABC_OK;
}

inline int check_weighted_gram(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y, int64_t stride_y, int32_t y_dim,
                               int64_t n, const double* y_obs, double delta, int32_t kind, const double* gram, const double* workspace)
{
    if (!theta || !y || !y_obs || !gram || (!workspace && n > 0)) return GLABC_ERR_NULL;
    if (int e = check_regress_dims(theta_dim, y_dim)) return e;
    if (kind != GLABC_GRAM_EPANECHNIKOV && kind != GLABC_GRAM_UNIFORM) return GLABC_ERR_KIND;
    if (n < 0 || stride_t < n || stride_y < n || !(delta > 0.0)) return GLABC_ERR_ARG;
    return GLABC_OK;
}

inline int check_regression_apply(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y, int64_t stride_y, int32_t y_dim,
                                  int64_t n, const double* y_obs, const double* beta, const float* out, int64_t stride_o)
{
    if (!theta || !y || !y_obs || !beta || !out) return GLABC_ERR_NULL;
    if (int e = check_regress_dims(theta_dim, y_dim)) return e;
    if (n < 0 || stride_t < n || stride_y < n || stride_o < n) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_abc_draws: the Model a fused rejection draw is compiled for and the range of draws, in the order include/glabc.h lists
// the refusals.  The parameters' values are not looked at: a draw from a prior of scale 0 or NaN is what the arithmetic says it is
// the shapes the built-in simulators are compiled for, then the simulator's kind; theta_dim: what the caller's data has (a history's;
// the Model's own where there is none), asked between the two
inline int check_draw_sim(const glabc_model* m, int32_t theta_dim)
{
    if (m->theta_dim < 1 || m->theta_dim > GLABC_MAX_DIM || m->y_dim < 1 || m->y_dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    if (m->sim_kind == GLABC_SIM_GK && (m->theta_dim != 4 || m->y_dim != 8)) return GLABC_ERR_DIM;
    if (m->sim_kind == GLABC_SIM_ABS_GAUSS && m->y_dim != m->theta_dim) return GLABC_ERR_DIM;
    if (theta_dim != m->theta_dim) return GLABC_ERR_DIM;
    if (m->sim_kind != GLABC_SIM_ABS_GAUSS && m->sim_kind != GLABC_SIM_GK) return GLABC_ERR_KIND;
    return GLABC_OK;
}

// the priors a draw kernel draws theta from
inline int check_draw_prior(const glabc_model* m)
{
    if (m->prior.kind != GLABC_DIST_DIAG_GAUSS && m->prior.kind != GLABC_DIST_UNIFORM) return GLABC_ERR_KIND;
    if (m->prior.dim != m->theta_dim) return GLABC_ERR_KIND;
    return GLABC_OK;
}

inline int check_abc_model(const glabc_model* m)
{
    if (int e = check_draw_sim(m, m->theta_dim)) return e;
    return check_draw_prior(m);
}

inline int check_abc_range(int64_t row0, const int64_t* ids, int64_t n, int64_t stride)
{
    return (n < 0 || stride < n || row0 < 0 || (ids && row0 != 0)) ? GLABC_ERR_ARG : GLABC_OK;
}

inline int check_abc_draws(const glabc_model* m, int64_t row0, const int64_t* ids, int64_t n, int64_t stride, const float* theta_out,
                           const float* y_out, const float* dis_out, const uint8_t* accept_out)
{
    if (!m || (!theta_out && !y_out && !dis_out && !accept_out)) return GLABC_ERR_NULL;
    if (int e = check_abc_model(m)) return e;
    return check_abc_range(row0, ids, n, stride);
}

// ---- glabc_coverage_counts: check_abc_draws' order -- the pointers, the Model as glabc_abc_draws examines it, then the numbers.  The
// widths' and the test rows' values are not looked at (they are on the device): a pair is what the arithmetic says it is
inline int check_coverage_counts(const glabc_model* m, int64_t row0, int64_t n, const float* theta_star, const float* y_star,
                                 const float* width, int64_t n_tests, int64_t test_stride, int32_t kernel, const unsigned long long* mass)
{
    if (!m || !mass || !theta_star || !y_star || !width) return GLABC_ERR_NULL;
    if (int e = check_abc_model(m)) return e;
    if (n < 0 || row0 < 0 || n_tests < 0 || test_stride < n_tests || (kernel != 0 && kernel != 1)) return GLABC_ERR_ARG;
    if (n > GLABC_MAX_COVERAGE_DRAWS || n_tests > GLABC_MAX_COVERAGE_TESTS) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_predictive_draws / glabc_predictive_counts: the Model a predictive draw is compiled for (check_abc_model's rules without
// the prior, which is neither used nor examined), the history and the ids, in the order include/glabc.h lists the refusals; each
// entry point adds what its own outputs ask
inline int check_predictive_model(const glabc_model* m, int32_t theta_dim) { return check_draw_sim(m, theta_dim); }

// the last id of a call, id0 + (n_rows - 1) * id_step + n_chains - 1, must be an int64
inline int check_predictive_range(int64_t n_rows, int64_t n_chains, int64_t stride, int64_t id0, int64_t id_step)
{
    if (n_rows < 1 || n_chains < 0 || stride < n_chains) return GLABC_ERR_ARG;
    if (id0 < 0 || id_step < n_chains) return GLABC_ERR_ARG;
    int64_t last;
    if (__builtin_mul_overflow(n_rows - 1, id_step, &last) || __builtin_add_overflow(last, id0, &last) ||
        __builtin_add_overflow(last, n_chains > 0 ? n_chains - 1 : 0, &last))
        return GLABC_ERR_ARG;
    return GLABC_OK;
}

// The Model of a predictive call, asked between the pointers and the numbers.  The built-in entry points: check_predictive_model.  The
// launch of a run-time compiled predictive program has examined the Model against its program before (check_rtc_predictive_program):
// what is left is the history's theta_dim.  The prior is neither used nor examined by either.
struct PredModelCheck {
    bool rtc = false;
    int operator()(const glabc_model* m, int32_t theta_dim) const
    {
        if (!rtc) return check_predictive_model(m, theta_dim);
        return theta_dim != m->theta_dim ? GLABC_ERR_DIM : GLABC_OK;
    }
};

inline int check_predictive_draws(const glabc_model* m, const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                  int64_t stride, int64_t id0, int64_t id_step, const float* y_out, int64_t y_stride, const float* dis_out,
                                  int64_t dis_stride, const PredModelCheck& model_check = PredModelCheck())
{
    if (!m || !history || (!y_out && !dis_out)) return GLABC_ERR_NULL;
    if (int e = model_check(m, theta_dim)) return e;
    if (n_rows < 1 || n_chains < 0 || stride < n_chains) return GLABC_ERR_ARG;
    if ((y_out && y_stride < n_chains) || (dis_out && dis_stride < n_chains)) return GLABC_ERR_ARG;
    return check_predictive_range(n_rows, n_chains, stride, id0, id_step);
}

inline int check_predictive_counts(const glabc_model* m, const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                   int64_t stride, int64_t id0, int64_t id_step, int32_t n_bins, const double* lo, const double* hi,
                                   const float* threshold, const uint64_t* counts, const uint64_t* tails, const uint32_t* extremes,
                                   const PredModelCheck& model_check = PredModelCheck())
{
    if (!m || !history || (!counts && !tails && !extremes)) return GLABC_ERR_NULL;
    if ((counts && (!lo || !hi)) || (tails && !threshold)) return GLABC_ERR_NULL;
    if (int e = model_check(m, theta_dim)) return e;
    if (int e = check_predictive_range(n_rows, n_chains, stride, id0, id_step)) return e;
    const int n_stats = m->y_dim + 1;
    if (counts) {
        if (n_bins < 1 || n_bins > GLABC_MAX_PREDICTIVE_BINS) return GLABC_ERR_ARG;
        for (int k = 0; k < n_stats; ++k)
            if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(lo[k] < hi[k])) return GLABC_ERR_ARG;
    }
    if (tails)
        for (int k = 0; k < n_stats; ++k)
            if (threshold[k] != threshold[k]) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_weighted_predictive_counts (and, with PredModelCheck{true}, its run-time compiled twin): check_predictive_counts on the
// one-row history [1][theta_dim][stride] of n draws with id_step = n -- so n < 0, stride < n, id0 < 0 and a last id id0 + n - 1 past
// int64 are its own -- with a null weight array a null pointer like the others; then what the weights add (check_weight_scale) and
// the smaller limit on the bins, looked at where the twin looks at its own
inline int check_weighted_predictive_counts(const glabc_model* m, const float* x, int64_t stride, int32_t theta_dim, const float* w, int64_t n,
                                            double scale, int64_t id0, int32_t n_bins, const double* lo, const double* hi,
                                            const float* threshold, const uint64_t* counts, const uint64_t* tails, const uint32_t* extremes,
                                            const PredModelCheck& model_check = PredModelCheck())
{
    if (!w) return GLABC_ERR_NULL;
    if (int e = check_predictive_counts(m, x, 1, theta_dim, n, stride, id0, n, n_bins, lo, hi, threshold, counts, tails, extremes, model_check))
        return e;
    if (counts && n_bins > GLABC_MAX_WEIGHTED_PREDICTIVE_BINS) return GLABC_ERR_ARG;
    return check_weight_scale(n, scale);
}

// ---- glabc_kde: what every entry point that reads a fitted KernelDensity asks of its descriptor (cum_q is glabc_kde_sample's and
// glabc_smc_draws' alone and they ask for it themselves)
inline int kde_check(const glabc_kde* k)
{
    if (!k) return GLABC_ERR_NULL;
    if (k->dim < 1 || k->dim > GLABC_MAX_DIM) return GLABC_ERR_DIM;
    if (k->n_samples < 1) return GLABC_ERR_ARG;
    if (!k->x || !k->log_w) return GLABC_ERR_NULL;
    for (int d = 0; d < k->dim; ++d)
        if (!(k->bandwidth[d] > 0.0f) || k->bandwidth[d] == INFINITY) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_smc_draws: check_abc_draws with a fifth output and the population between the Model and the range of draws, in the order
// include/glabc.h lists the refusals.  The population's values are looked at (kde_check): a bandwidth of 0 has no mixture density
// (the population's own rules, for glabc_rtc_smc_draws too)
inline int check_draw_population(const glabc_kde* pop, int32_t theta_dim)
{
    if (int e = kde_check(pop)) return e;
    if (!pop->cum_q) return GLABC_ERR_NULL;
    return pop->dim != theta_dim ? GLABC_ERR_DIM : GLABC_OK;
}

inline int check_smc_draws(const glabc_model* m, const glabc_kde* pop, int64_t row0, const int64_t* ids, int64_t n, int64_t stride,
                           const float* theta_out, const float* y_out, const float* dis_out, const float* log_prior_out,
                           const uint8_t* accept_out)
{
    if (!m || !pop || (!theta_out && !y_out && !dis_out && !log_prior_out && !accept_out)) return GLABC_ERR_NULL;
    if (int e = check_abc_model(m)) return e;
    if (int e = check_draw_population(pop, m->theta_dim)) return e;
    return check_abc_range(row0, ids, n, stride);
}

// ---- the lower Cholesky factor of a full-covariance perturbation (glabc_kde_sample_full, glabc_smc_draws_full and its run-time
// compiled twin): a HOST array of dim (dim + 1) / 2 floats packed row-major, every entry finite, the diagonal positive.  `dim` has
// passed the population's checks
inline int check_chol(const float* chol, int32_t dim)
{
    if (!chol) return GLABC_ERR_NULL;
    for (int d = 0, i = 0; d < dim; ++d)
        for (int e = 0; e <= d; ++e, ++i)
            if (!std::isfinite(chol[i]) || (e == d && !(chol[i] > 0.0f))) return GLABC_ERR_ARG;
    return GLABC_OK;
}

// ---- glabc_smc_draws_full: check_smc_draws with the factor between the population and the range of draws
inline int check_smc_draws_full(const glabc_model* m, const glabc_kde* pop, const float* chol, int64_t row0, const int64_t* ids, int64_t n,
                                int64_t stride, const float* theta_out, const float* y_out, const float* dis_out,
                                const float* log_prior_out, const uint8_t* accept_out)
{
    if (!m || !pop || (!theta_out && !y_out && !dis_out && !log_prior_out && !accept_out)) return GLABC_ERR_NULL;
    if (int e = check_abc_model(m)) return e;
    if (int e = check_draw_population(pop, m->theta_dim)) return e;
    if (int e = check_chol(chol, m->theta_dim)) return e;
    return check_abc_range(row0, ids, n, stride);
}

// ---- glabc_rtc_steps: a launch of the run-time compiled program of shape `p` -------------------------------------------------
inline int check_rtc_run(const RtcShape& p, const glabc_model* m, const glabc_dist* local, const glabc_dist* global, const glabc_chains* c,
                         const glabc_run* r)
{
    if (!m || !c || !r) return GLABC_ERR_NULL;
    if (m->sim_kind != GLABC_SIM_USER) return GLABC_ERR_KIND;
    if (m->theta_dim != p.theta_dim || m->y_dim != p.y_dim || m->noise.dim != p.noise_dim) return GLABC_ERR_DIM;
    // a Gamma prior / global proposal: where the program holds the Gamma kernels (GLABC_RTC_GAMMA); `local` never
    const bool allow_gamma = p.gamma != 0;
    if (check_dist(&m->prior, p.theta_dim, allow_gamma) || check_dist(local, p.theta_dim) || check_dist(global, p.theta_dim, allow_gamma))
        return GLABC_ERR_ARG;                                     // whatever the defect of a descriptor
    if (!std::isfinite(m->kern_log_scale) || !(m->kern_scale > 0.0f) || !std::isfinite(m->kern_c0)) return GLABC_ERR_ARG;
    if (int e = check_chains(c, p.algo == GLABC_ALGO_GLMCMC ? CHAINS_ISIR : CHAINS_PLAIN)) return e;
    if (r->n_steps < 0) return GLABC_ERR_ARG;
    if (p.wide) {                                                 // lane groups: batch sizes the register kernels do not hold
        if (r->batch_size <= GLABC_MAX_BATCH || r->batch_size > GLABC_MAX_BATCH_WIDE) return GLABC_ERR_ARG;
        if (check_lanes_wide(r->lanes_per_chain) || r->tape || r->step0_device) return GLABC_ERR_ARG;
    } else {
        if (p.algo == GLABC_ALGO_GLMCMC && r->batch_size != p.batch_size) return GLABC_ERR_ARG;      // compiled for one batch size
        if (r->tape || r->step0_device || (r->lanes_per_chain != 0 && r->lanes_per_chain != 1)) return GLABC_ERR_ARG;
    }
    if (r->math_mode != GLABC_MATH_EXACT || r->dump_draws) return GLABC_ERR_ARG;
    if (int e = check_frequency(r)) return e;
    if (int e = check_history(r, c->n_chains)) return e;
    if (int e = check_moments(r)) return e;
    return check_step_counter(r);
}

// ---- glabc_rtc_mix_steps: a launch of the run-time compiled MIXTURE program of shape `p` ----------------------------------------
// mix_program: the program was built from the mixture table (glabc_rtc_compile_mix / _wide_mix, rtc_mix_kernels of glabc_rtc_tables.h); a program of
// the other table holds no kernel that takes a MixStepArgs.  The order is the contract (include/glabc.h).
inline int check_rtc_mix_run(const RtcShape& p, bool mix_program, const glabc_model* m, const glabc_dist* local, const glabc_mixture* g,
                             const glabc_chains* c, const glabc_run* r)
{
    if (!m || !local || !g || !c || !r) return GLABC_ERR_NULL;
    if (m->sim_kind != GLABC_SIM_USER) return GLABC_ERR_KIND;
    if (m->theta_dim != p.theta_dim || m->y_dim != p.y_dim || m->noise.dim != p.noise_dim) return GLABC_ERR_DIM;
    if (!mix_program) return GLABC_ERR_KIND;
    if (m->prior.kind == GLABC_DIST_GAMMA) return GLABC_ERR_KIND;               // the mixture variant knows no Gamma
    if (check_dist(&m->prior, p.theta_dim) || check_dist(local, p.theta_dim)) return GLABC_ERR_ARG;      // whatever the defect of a descriptor
    if (!std::isfinite(m->kern_log_scale) || !(m->kern_scale > 0.0f) || !std::isfinite(m->kern_c0)) return GLABC_ERR_ARG;
    if (r->tape || r->math_mode != GLABC_MATH_EXACT || r->dump_draws) return GLABC_ERR_ARG;      // a tape has no mode draws
    if (int e = check_mixture(g, p.theta_dim)) return e;
    if (int e = check_chains(c, p.algo == GLABC_ALGO_GLMCMC ? CHAINS_ISIR : CHAINS_PLAIN)) return e;
    if (r->n_steps < 0 || r->step0_device) return GLABC_ERR_ARG;
    if (p.wide) {                                                 // lane groups: batch sizes the register kernels do not hold
        if (r->batch_size <= GLABC_MAX_BATCH || r->batch_size > GLABC_MAX_BATCH_WIDE) return GLABC_ERR_ARG;
        if (check_lanes_wide(r->lanes_per_chain)) return GLABC_ERR_ARG;
    } else {
        if (p.algo == GLABC_ALGO_GLMCMC && r->batch_size != p.batch_size) return GLABC_ERR_ARG;      // compiled for one batch size
        if (r->lanes_per_chain != 0 && r->lanes_per_chain != 1) return GLABC_ERR_ARG;
    }
    if (int e = check_frequency(r)) return e;
    if (int e = check_history(r, c->n_chains)) return e;
    if (int e = check_moments(r)) return e;
    return check_step_counter(r);
}

// ---- glabc_rtc_abc_draws / glabc_rtc_smc_draws: a launch of the run-time compiled DRAWS program of shape `p` -------------------------
// draws_program: the program was built from the draws table (glabc_rtc_compile_draws, rtc_draws_kernels of glabc_rtc_tables.h); no other program
// holds a draw kernel.  any_output: one of the entry point's outputs is not NULL.  smc: glabc_rtc_smc_draws, which reads `pop` --
// refused as glabc_smc_draws refuses it (check_draw_population), between the Model and the range of draws; the prior is
// check_draw_prior's, the range check_abc_range's.  The order is the contract (include/glabc.h); the entry point has refused a NULL program before.
inline int check_rtc_draws(const RtcShape& p, bool draws_program, const glabc_model* m, bool smc, const glabc_kde* pop, bool any_output,
                           int64_t row0, const int64_t* ids, int64_t n, int64_t stride, bool full = false, const float* chol = nullptr)
{
    if (!m || !any_output) return GLABC_ERR_NULL;
    if (m->sim_kind != GLABC_SIM_USER) return GLABC_ERR_KIND;
    if (!draws_program) return GLABC_ERR_KIND;
    if (m->theta_dim != p.theta_dim || m->y_dim != p.y_dim || m->noise.dim != p.noise_dim) return GLABC_ERR_DIM;
    if (int e = check_draw_prior(m)) return e;
    if (smc)
        if (int e = check_draw_population(pop, m->theta_dim)) return e;
    if (full)                                                     // glabc_rtc_smc_draws_full: the factor, as glabc_smc_draws_full refuses it
        if (int e = check_chol(chol, m->theta_dim)) return e;
    return check_abc_range(row0, ids, n, stride);
}

// ---- glabc_rtc_predictive_draws / glabc_rtc_predictive_counts: a launch of the run-time compiled PREDICTIVE program of shape `p` -------
// pred_program: the program was built from the predictive table (glabc_rtc_compile_predictive, rtc_predictive_kernels of glabc_rtc_tables.h); no
// other program holds predictive_kernel.  The entry point has refused a NULL program before; after this, check_predictive_draws /
// check_predictive_counts with PredModelCheck{true} refuse what the built-in entry points refuse, in their order.  The prior is not
// looked at: theta comes from the history.  The order is the contract (include/glabc.h).
inline int check_rtc_predictive_program(const RtcShape& p, bool pred_program, const glabc_model* m)
{
    if (!m) return GLABC_ERR_NULL;
    if (m->sim_kind != GLABC_SIM_USER) return GLABC_ERR_KIND;
    if (!pred_program) return GLABC_ERR_KIND;
    if (m->theta_dim != p.theta_dim || m->y_dim != p.y_dim || m->noise.dim != p.noise_dim) return GLABC_ERR_DIM;
    return GLABC_OK;
}

}  // namespace glabc
