/*
 * glabc.h -- C ABI of the MI355X-native GL-ABC-MCMC hot path.
 *
 * The reference (caofff/GL-ABC-MCMC, /root/reference) has no FFI of its own:
 * its hot path is the body of three Python loops,
 *     GlobalMCMC  glabcmcmc/GlobalMCMC.py:37-68
 *     GLMCMC      glabcmcmc/GLMCMC.py:58-104
 *     GLMALA      glabcmcmc/GLMALA.py:150-200
 * calling distribution.{DiagGaussian,Uniform,Gamma} (glabcmcmc/distribution.py)
 * and the user's Model callbacks (glabcmcmc/examples/Mixture.py:13-45).  Each
 * entry point below replaces one of those loop bodies (or one distribution /
 * ESJD.py call) for a whole batch of independent chains; the Python package
 * glabcmcmc_amd binds them with ctypes (INTEGRATION.md shows the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types.
 *   - every pointer inside glabc_chains / glabc_run is a DEVICE pointer
 *     (hipMalloc'd or a torch CUDA tensor's data_ptr); descriptor structs
 *     themselves are read on the host at call time and may live on the stack.
 *   - calls are stream-ordered on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream), allocate nothing, keep no global state, and
 *     are safe to call concurrently on different streams / chain sets.
 *   - return 0 on success or a negative glabc_status; never throw.
 *   - chain state is structure-of-arrays, chain index innermost
 *     ("chain-major"): component j of chain c is at  base[j*stride + c], so a
 *     64-lane wavefront reads 256 contiguous bytes per component.
 *   - random numbers: Philox4x32-10 keyed by the 64-bit seed with counter
 *     (global chain id, step, slot) -- include/glabc_numerics.h -- so results
 *     do not depend on launch geometry, on n_steps per call, or on how chains
 *     are sharded over GPUs (chain0 carries the shard offset).
 */
#ifndef GLABC_H
#define GLABC_H

#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define GLABC_VERSION 301          /* 0.3.1: bumped whenever a struct of this header changes (the Python binding refuses a library
                                      of another version: a stale .so would misread the argument blocks) */
/* Layout of the random stream (include/glabc_numerics.h): which Philox (counter, slot, word) a draw of (chain, iteration) reads.
 * A checkpoint stores it; resuming on another layout would continue on a different stream.  2 = simulator normals start at an
 * even word (round 2), NF pool rows keyed (refresh << 44) + chain0 * P + r. */
#define GLABC_STREAM_LAYOUT 2
#define GLABC_MAX_DIM 8            /* theta_dim, y_dim, distribution dim */
#define GLABC_MAX_BATCH 16         /* iSIR proposals per step held in registers (one to four lanes per chain) */
#define GLABC_MAX_BATCH_WIDE 4096  /* glabc_glmcmc_steps beyond that: 8 to 64 lanes of a wavefront share a chain's proposals */

typedef enum glabc_status {
    GLABC_OK = 0,
    GLABC_ERR_NULL = -1,           /* a required pointer is NULL */
    GLABC_ERR_DIM = -2,            /* dimension out of range / not compiled in */
    GLABC_ERR_KIND = -3,           /* distribution / simulator kind not supported by this entry point */
    GLABC_ERR_ARG = -4,            /* bad scalar argument (n_steps < 0, batch_size out of range, ...) */
    GLABC_ERR_LAUNCH = -5,         /* hipLaunchKernel failed; see glabc_last_hip_error() */
    GLABC_ERR_NO_DEVICE = -6       /* no HIP device / wrong architecture */
} glabc_status;

/* ---- distributions: glabcmcmc/distribution.py ---------------------------- */
typedef enum glabc_dist_kind {
    GLABC_DIST_DIAG_GAUSS = 0,     /* distribution.py:143-181 */
    GLABC_DIST_UNIFORM = 1,        /* distribution.py:50-86   */
    GLABC_DIST_GAMMA = 2           /* distribution.py:90-137  */
} glabc_dist_kind;

typedef struct glabc_dist {
    int32_t kind;                  /* glabc_dist_kind */
    int32_t dim;
    float p0[GLABC_MAX_DIM];       /* DiagGaussian loc        | Uniform low        | Gamma shape */
    float p1[GLABC_MAX_DIM];       /* DiagGaussian log_scale  | Uniform high       | Gamma rate  */
    float p2[GLABC_MAX_DIM];       /* DiagGaussian exp(log_scale) exactly as the caller's exp returned it
                                      (distribution.py:170,178 recompute it per call; the round trip
                                      exp(log(s)) != s matters for bit parity) | Uniform high-low
                                      | Gamma scale = 1/rate as the reference forms it (float32 division, distribution.py:118,133) */
    float p3[GLABC_MAX_DIM];       /* Gamma scipy.special.gammaln(shape) (a float32 number: the reference keeps Shape as a float32
                                      array, distribution.py:103) | unused otherwise */
    float c0;                      /* DiagGaussian f32(-0.5*dim*log(2*pi)) (distribution.py:171,177)
                                      | Uniform log_prob_val (distribution.py:71) | unused */
} glabc_dist;

/* GLABC_DIST_GAMMA inside the samplers (glabc_glmcmc_steps incl. batch sizes beyond GLABC_MAX_BATCH, glabc_globalmcmc_steps,
 * glabc_propose / glabc_select, glabc_init_weights, glabc_dist_log_prob, the row-wise Model callbacks): accepted as the
 * importance / global proposal and as the Model's prior (not as the local increment, not as simulator noise).  The reference's
 * Gamma is float64 (distribution.py:106-137); the chains' state is float32 here, so
 *   forward:  z_q = glabc_gamma_draw_candidate(shape_q; chain, iteration, candidate j, coordinate q) * scale_q in double
 *             (include/glabc_numerics.h: Marsaglia-Tsang on the chain's Philox stream), theta'_q = (float) z_q,
 *             log q' = (float) sum_q log(pdf(z_q))  -- the density of the double variate, summed in torch.sum's float64 order
 *   log_prob: (float) sum_q log(pdf((double) theta_q)), -inf outside the support or where the pdf underflows (distribution.py:136)
 * which is what the split-phase path does with a Gamma object's callbacks (results rounded to float32 for glabc_select).
 * Where the fused samplers take it: glabc_glmcmc_steps (every batch size) and glabc_globalmcmc_steps on GLABC_SIM_ABS_GAUSS with
 * theta_dim <= 4 and on GLABC_SIM_GK; glabc_rtc_steps on a program compiled with GLABC_RTC_GAMMA (glabc_rtc_compile_ex /
 * glabc_rtc_compile_wide_ex).  Still refused: theta_dim 5..8 (GLABC_ERR_KIND), a tape and GLABC_MATH_FAST (GLABC_ERR_ARG),
 * glabc_glmala_steps and the pool entry points (GLABC_ERR_KIND), a program compiled without the flag (GLABC_ERR_ARG). */

/* ---- the Model callbacks: glabcmcmc/examples/Mixture.py:5-53 ------------- */
typedef enum glabc_sim_kind {
    GLABC_SIM_ABS_GAUSS = 0,       /* y = |theta| + noise, noise ~ DiagGaussian   Mixture.py:13-26 */
    GLABC_SIM_GK = 1,              /* g-and-k order statistics (BASELINE config 4; no counterpart in the reference tree --
                                      the Model is the build's own, glabcmcmc_amd/examples/GK.py): theta = (A, B, g, k),
                                      y = sort_j( A + B (1 + c tanh(g z_j/2)) (1 + z_j^2)^k z_j ), z_j ~ N(0,1), j < y_dim = 8 */
    GLABC_SIM_USER = 2             /* the caller's simulator, C source compiled into the fused kernel at run time (glabc_rtc_compile):
                                      y[y_dim] = glabc_user_simulate(theta[theta_dim], eps[noise.dim] standard normals); only
                                      glabc_rtc_steps and the row-wise Model callbacks accept it */
} glabc_sim_kind;

typedef struct glabc_model {
    int32_t sim_kind;              /* glabc_sim_kind */
    int32_t theta_dim;             /* Mixture.py:8  */
    int32_t y_dim;                 /* Mixture.py:10 */
    float gk_c;                    /* GLABC_SIM_GK: the constant c (0.8) */
    glabc_dist prior;              /* prior_log_prob      Mixture.py:28-31 */
    glabc_dist noise;              /* generate_samples    Mixture.py:19    */
    float y_obs[GLABC_MAX_DIM];    /* discrepancy = ||y - y_obs||_2         Mixture.py:9,33-36 */
    float kern_log_scale;          /* log(f32 epsilon)      calculate_log_kernel, Mixture.py:42-43 */
    float kern_scale;              /* exp(log(f32 epsilon)) */
    float kern_c0;                 /* f32(-0.5*log(2*pi))   */
    float epsilon;                 /* epsilon itself (GLMALA.py:90 uses epsilon**2 in double) */
} glabc_model;

/* ---- chain state ----------------------------------------------------------- */
#define GLABC_FLAG_LOCAL 1u        /* the reference's `local` dirty flag, GLMCMC.py:50,65,100 */
/* GLMALA only.  The reference's tensors change dtype while a chain runs: the gradient estimate is
 * float64 (GLMALA.py:70-72), so the first ACCEPTED MALA move turns Theta_old / y_old into float64
 * tensors (GLMALA.py:43,197-198) and every later torch.cat keeps them float64; log_weight_old takes
 * the dtype the state has when it is first computed (GLMALA.py:152-156) and keeps it.  The two
 * sticky bits below record in which precision the reference would be computing. */
#define GLABC_FLAG_TH64 2u         /* Theta_old, y_old are float64 tensors */
#define GLABC_FLAG_LW64 4u         /* log_weight_old (and hence the iSIR weights) are float64 */
#define GLABC_FLAG_HAS_GRAD 8u     /* grad_logABC_Theta_old is not None, GLMALA.py:146,183-184 */

typedef struct glabc_chains {
    int64_t n_chains;              /* chains in this call (this GPU's shard) */
    int64_t chain0;                /* global id of chain 0 of the shard (Philox counter words 0,1) */
    int64_t stride;                /* elements between components, >= n_chains */
    float* theta;                  /* [theta_dim][stride]  Theta_old  GLMCMC.py:48 */
    float* y;                      /* [y_dim][stride]      y_old      GLMCMC.py:49 */
    float* log_w;                  /* [stride] log_weight_old GLMCMC.py:53-55 (iSIR samplers; else NULL) */
    uint32_t* flags;               /* [stride] GLABC_FLAG_* (iSIR samplers; else NULL) */
    uint32_t* n_moves;             /* [stride] accepted moves, num_acc GLMCMC.py:51,88,101; NULL = not counted */
    /* GLMALA state (NULL for the other samplers): the authoritative copy of the state in double
     * (float32-exact values while the corresponding GLABC_FLAG_*64 bit is clear); theta / y above
     * then receive the float32 casts that Theta_Re records (GLMALA.py:180,200) */
    double* theta64;               /* [theta_dim][stride] */
    double* y64;                   /* [y_dim][stride] */
    double* log_w64;               /* [stride] */
    double* grad;                  /* [theta_dim][stride] grad_logABC_Theta_old, GLMALA.py:146,199 */
} glabc_chains;

/* Per-chain streaming sums for ESJD.py:17-24 and posterior moments, updated
 * once per iteration inside the kernel (so a run needs no history to report
 * them).  tri(d) = d(d+1)/2 entries, row-major upper triangle. */
typedef struct glabc_moments {
    double* sum_theta;             /* [theta_dim][stride]        sum_t theta_t            */
    double* sum_outer;             /* [tri(theta_dim)][stride]   sum_t theta_t theta_t^T  */
    double* sum_jump;              /* [tri(theta_dim)][stride]   sum_t (theta_t - theta_{t-1})(..)^T */
} glabc_moments;

/* Replayed random numbers (tests, common-random-number studies): when
 * glabc_run.tape is non-NULL glabc_glmcmc_steps / glabc_globalmcmc_steps read their draws
 * from here (device arrays covering exactly the call's n_steps) instead of Philox.
 * Layout is chain-outermost, as recorded by tests/golden/make_golden.py.  (GLMALA and the
 * GLMCMC_NF entry points do not take a tape.) */
typedef struct glabc_tape {
    const float* u;                /* [n_chains][n_steps][2]  (branch, accept) f32 in [0,1) */
    const double* r;               /* [n_chains][n_steps]     resampling uniform f64 in [0,1) */
    const float* z;                /* [n_chains][n_steps][n_prop][theta_dim + y_dim] N(0,1) draws:
                                      proposal noise then simulator noise; the local move uses row 0 */
    int32_t n_prop;                /* rows per step on the tape */
    int32_t reserved;
} glabc_tape;

typedef struct glabc_run {
    uint64_t seed;                 /* Philox key */
    uint32_t step0;                /* iteration index of the first step of this call (the reference's
                                      loop variable i starts at 1: GLMCMC.py:58); Philox counter word 2 */
    int32_t n_steps;               /* iterations fused into this launch (K) */
    float global_frequency;        /* GLMCMC.py:59 */
    int32_t batch_size;            /* iSIR proposals N, GLMCMC.py:66: 1..GLABC_MAX_BATCH_WIDE for glabc_glmcmc_steps (no tape above
                                      GLABC_MAX_BATCH), 1..GLABC_MAX_BATCH for the other samplers; ignored by GlobalMCMC */
    float* history;                /* NULL or [n_steps][theta_dim][hist_stride]: Theta_Re rows i=step0.. GLMCMC.py:89,104 */
    int64_t hist_stride;           /* >= n_chains */
    const glabc_moments* moments;  /* NULL or accumulators (same stride as chains) */
    const glabc_tape* tape;        /* NULL = Philox */
    int32_t lanes_per_chain;       /* launch geometry only, never changes results: 0 = the library chooses the kernel and its lanes
                                      (DESIGN.md 4.0), or 1 / 2 / 4 lanes cooperating on one chain's batch_size proposals (8 / 16 /
                                      32 / 64 when batch_size > GLABC_MAX_BATCH).  A non-zero value also keeps a launch off the team
                                      kernels unless GLABC_DEBUG_TEAM asks for them; it is capped by what batch_size can feed (4
                                      lanes need 3 proposals) and is one lane for GlobalMCMC, a tape and the Gamma variant (every Model that
                                      takes a Gamma: |theta| + noise, g-and-k, a run-time compiled program's Gamma entry) */
    int32_t debug_flags;           /* 0, or GLABC_DEBUG_* bits: execution strategy only, never changes results */
    const uint32_t* step0_device;  /* glabc_propose / glabc_propose_redraw / glabc_select only: NULL, or a DEVICE word holding the
                                      iteration index of this call.  The kernels then read the index from it (Philox counter
                                      word 2) and write the Theta_Re row (index - step0) of `history`, so ONE captured hipGraph
                                      of an iteration can be replayed while the word is incremented between replays */
    const float* global_frequency_per_chain;   /* NULL, or device array [n_chains] that replaces global_frequency chain by
                                      chain -- a hyper-parameter grid (examples/Mixture_hyper.py:24) is then one launch.
                                      glabc_glmcmc_steps / glabc_globalmcmc_steps only */
    int32_t math_mode;             /* GLABC_MATH_EXACT (0, default) or GLABC_MATH_FAST, see below */
    int32_t reserved;
    const struct glabc_draws_out* dump_draws;  /* GLABC_MATH_FAST only: NULL, or where the kernel WRITES the draws it used */
} glabc_run;

/* glabc_run.math_mode -- an OPT-IN variant of glabc_glmcmc_steps (batch size 2..GLABC_MAX_BATCH, theta_dim <= 4, the
 * |theta| + noise simulator; anything else returns GLABC_ERR_ARG).
 *   GLABC_MATH_EXACT  every elementary function is the specified sequence of IEEE operations of include/glabc_numerics.h: the
 *                     CPU checker reproduces every bit.  The default, and what every parity statement in this repository is about.
 *   GLABC_MATH_FAST   Box-Muller with the hardware's v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32, the iSIR weights with
 *                     v_exp_f32, the accept uniform's logarithm with v_log_f32, the discrepancy's square root with v_sqrt_f32 and
 *                     the division by the kernel width with v_rcp_f32 (about 1 ulp each).  The normals are then NOT the checker's:
 *                     the run samples the same law from another stream.  Parity is shown the teacher-forced way (SURVEY.md
 *                     appendix A.4): with dump_draws set the kernel records every uniform and normal it used in the glabc_tape
 *                     layout; the CPU checker replays that tape through the EXACT arithmetic and must take the same accept /
 *                     resample decisions except where a decision lies within rounding of its threshold
 *                     (tests/test_hip_parity.py::test_fast_math_*).  Philox, the candidates' arithmetic (IEEE + - x), torch.sum's
 *                     order and the double-precision index are unchanged. */
#define GLABC_MATH_EXACT 0
#define GLABC_MATH_FAST 1
typedef struct glabc_draws_out {   /* device arrays covering exactly the call's n_steps, layout of glabc_tape */
    float* u;                      /* [n_chains][n_steps][2] */
    double* r;                     /* [n_chains][n_steps] */
    float* z;                      /* [n_chains][n_steps][batch_size][theta_dim + y_dim] */
} glabc_draws_out;

/* glabc_run.debug_flags: the iSIR index (GLMCMC.py:7-22) is normally found from float32 reciprocal-multiplied
 * weights and recomputed the reference's way (IEEE divisions, double partial sums) only when the resampling uniform
 * lies within 4e-6 of a partial sum (the two cannot disagree otherwise: the fast partial sums are within 1.3e-6 of
 * the reference's).  This bit takes the reference's path always -- tests use it to show both give the same chains. */
#define GLABC_DEBUG_EXACT_INDEX 1
/* glabc_glmcmc_steps, batch_size 2..GLABC_MAX_BATCH: launches of 16 384 to 131 072 chains (at most two wavefronts per SIMD) with
 * lanes_per_chain 0 run as TEAMS of three (above 65 536 chains: two) wavefronts per 64 chains (csrc/glabc_team.h: one holds the
 * chains and takes the decisions, the others evaluate candidates one iteration ahead), or of fewer where the batch does not
 * split that far or the candidates exceed the LDS budget.  These bits forbid / force that geometry for a launch of any size --
 * tests use them to show that both give the same chains.  NO_TEAM wins over TEAM; GLABC_MATH_FAST ignores both; a configuration
 * that no team fits (theta_dim 4, batch_size 12..16, say) runs one to four lanes per chain even under TEAM. */
#define GLABC_DEBUG_NO_TEAM 2
#define GLABC_DEBUG_TEAM 4
/* (Round 3: teams of two / three wavefronts also run the Gamma variant, the g-and-k Model, GlobalMCMC -- glabc_globalmcmc_steps: a
 * helper wavefront draws an iteration's random numbers a chunk of iterations ahead -- and the run-time compiled kernels of
 * glabc_rtc_steps; the same two bits force / forbid the geometry there.  The Gamma variant has teams on g-and-k -- three
 * wavefronts for batch_size 3..7, two for 2..9, one lane per chain above -- and in a GLABC_RTC_GAMMA program; GlobalMCMC with a
 * Gamma always runs one lane per chain.) */
/* One lane per chain, theta_dim 1..4 (not g-and-k), launches of at most two wavefronts per SIMD: the library picks the build of the kernels scheduled for
 * instruction-level parallelism; this bit picks the default-schedule build (the one larger launches get) -- so that a test
 * can walk EVERY instantiation with small launches (tests/test_slp_twin.py). */
#define GLABC_DEBUG_DEFAULT_SCHEDULE 8

/* ---- entry points ------------------------------------------------------------ */

/* GLMCMC.py:58-104 -- iSIR global move with probability global_frequency,
 * else random-walk MH local move.  `local` is the zero-mean increment
 * distribution (GLMCMC.py:91), `importance` the absolute proposal (GLMCMC.py:66). */
int glabc_glmcmc_steps(const glabc_model* model, const glabc_dist* local, const glabc_dist* importance,
                       const glabc_chains* chains, const glabc_run* run, void* stream);

/* GlobalMCMC.py:37-68 -- independence MH global move / random-walk MH local move. */
int glabc_globalmcmc_steps(const glabc_model* model, const glabc_dist* local, const glabc_dist* global,
                           const glabc_chains* chains, const glabc_run* run, void* stream);

/* GLMALA.py:150-200 -- iSIR global move (GLMALA.py:151-180) / MALA local move whose drift is the
 * common-random-number central-difference gradient of a synthetic-likelihood log-ABC
 * (numberical_gradient_logABC, GLMALA.py:46-95; Local_proposal_forward :25-44; log_proposal :97-116).
 * tau_sq = tau**2 and eps_sq = epsilon**2 are passed as the caller's double-precision values
 * (Python evaluates them in float, GLMALA.py:43,90).  chains->theta64 / y64 / log_w64 / grad are
 * required; initialise them with glabc_glmala_init. */
typedef struct glabc_mala {
    double tau;                    /* GLMALA.py:118 */
    double tau_sq;                 /* tau ** 2 */
    double eps_sq;                 /* ABCset.epsilon ** 2 */
    int32_t num_grad;              /* simulations per finite-difference side, GLMALA.py:46 `num` */
    int32_t reserved;
} glabc_mala;

int glabc_glmala_steps(const glabc_model* model, const glabc_dist* importance, const glabc_mala* mala,
                       const glabc_chains* chains, const glabc_run* run, void* stream);

/* GLMALA.py:143-149: theta64 / y64 <- theta / y, flags <- LOCAL, no gradient yet. */
int glabc_glmala_init(const glabc_model* model, const glabc_chains* chains, void* stream);

/* ---- RealNVP coupling stack of GLMCMC_NF (GLMCMC_NFs.py:51-61,70-72,96-98) -------------------------
 * theta_dim = 2, hidden width 128 (nf.nets.MLP([1, 128, 128, 2]), GLMCMC_NFs.py:56).  One coupling's
 * parameters are one block of GLABC_NF_COUPLING_FLOATS floats in DEVICE memory:
 *     W2^T [k][i] (128*128, input-major) | W1[128] | b1[128] | (b2[i], W3[0][i], W3[1][i], 0) x 128 | b3[2], 0, 0
 * (W1: Linear(1,128).weight[:,0]; W2: Linear(128,128).weight [out][in]; W3: Linear(128,2).weight; row 0 of the
 * last layer is the shift, row 1 the log-scale: normflows AffineCoupling, param[:, 0::2] / param[:, 1::2]).
 * Rows are chain-major: x[0*n + r], x[1*n + r]. */
#define GLABC_NF_HIDDEN 128
#define GLABC_NF_COUPLING_FLOATS (128 * 128 + 128 + 128 + 4 * 128 + 4)

typedef struct glabc_flow {
    int32_t n_couplings;           /* GLMCMC_NFs.py:51 num_layers (32 there) */
    int32_t hidden;                /* must be GLABC_NF_HIDDEN */
    const float* params;           /* device, [n_couplings][GLABC_NF_COUPLING_FLOATS] */
    float base_loc[2];             /* nf.distributions.base.DiagGaussian(2): loc, log_scale, exp(log_scale) */
    float base_log_scale[2];
    float base_scale[2];
    float base_c0;                 /* f32(-0.5*2*log(2 pi)) */
    int32_t reserved;
} glabc_flow;

/* NF_model.sample(n): z = base(eps) pushed FORWARD through every coupling + swap; log_q = base log-density minus
 * the accumulated log-determinants.  eps[2][n] = the base noise, or NULL to draw it from Philox
 * (key = seed, counter = (row0 + r, 0, 0)). */
int glabc_nf_sample(const glabc_flow* flow, const float* eps, uint64_t seed, int64_t row0, int64_t n_rows,
                    float* z_out, float* log_q, void* stream);

/* NF_model.log_prob(x): x pulled back through the couplings in reverse order (inverse pass) + base log_prob. */
int glabc_nf_log_prob(const glabc_flow* flow, const float* x, int64_t n_rows, float* log_q, void* stream);

/* NF_model.log_prob for the rows listed in idx[0 .. *n_dev - 1] only: x = (theta[idx], theta[stride + idx]) (the chain-major
 * state arrays), result to log_q[idx].  *n_dev is read on the device (no host synchronisation); max_rows bounds it (the grid).
 * Same arithmetic per row as glabc_nf_log_prob. */
int glabc_nf_log_prob_indexed(const glabc_flow* flow, const float* theta, int64_t stride, const int32_t* idx,
                              const int32_t* n_dev, int64_t max_rows, float* log_q, void* stream);

/* NF_model.log_prob(x) AND the base-space point it is evaluated at: z_out[2][n] = x pulled back through every coupling;
 * trace (may be NULL): [n_couplings][n] the conditioner input every coupling saw on the way (what the training step needs to
 * open exactly the ReLU gates the forward evaluation opened). */
int glabc_nf_inverse(const glabc_flow* flow, const float* x, int64_t n_rows, float* z_out, float* log_q, float* trace,
                     void* stream);

/* ---- the training step of GLMCMC_NFs.py:63,112-124 -----------------------------------------------------------------------
 * loss = NF_model.forward_kld(x) = -mean(NF_model.log_prob(x)) over x[2][n_rows] and its gradient with respect to every
 * parameter, differentiated by hand (the reference lets autograd do it, GLMCMC_NFs.py:120-122): grad_params has the layout
 * of flow->params ([n_couplings][GLABC_NF_COUPLING_FLOATS], padding entries 0), grad_base = d/d(loc0, loc1, log_scale0,
 * log_scale1) of the base distribution, *loss is a device scalar.  workspace: device memory of at least
 * glabc_nf_grad_workspace bytes, contents undefined afterwards.  The derivative is that of the float32 evaluation's active
 * set: every ReLU gate is opened exactly where glabc_nf_log_prob's arithmetic opened it (the conditioner inputs of the
 * downward pass are kept, 4 bytes per row and coupling).  Floating-point parity (sums over rows run on the matrix cores in
 * float32, reduced over workgroups in a fixed order): reproducible to the bit from run to run, within 2e-4 of each tensor's
 * largest entry of the checker's double-precision sums over the same active set (tests/test_nf_train.py). */
int glabc_nf_grad_workspace(int32_t n_couplings, int64_t n_rows, int64_t* bytes);
int glabc_nf_grad(const glabc_flow* flow, const float* x, int64_t n_rows, void* workspace, int64_t workspace_bytes,
                  float* grad_params, float* grad_base, float* loss, void* stream);

/* torch.optim.Adam.step() (GLMCMC_NFs.py:63,123: lr 5e-4, weight_decay 1e-5 added to the gradient, no amsgrad) on `count`
 * float32 values, step = 1, 2, ...: exp_avg <- lerp(exp_avg, g, 1 - beta1); exp_avg_sq <- beta2 exp_avg_sq + (1 - beta2) g g;
 * p <- p - lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps). */
int glabc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int32_t step, void* stream);

/* ---- GLMCMC_NF (GLMCMC_NFs.py:43-186): iSIR against a pool of flow proposals -----------------------------
 * A pool holds P = batch_size*step_size proposals per chain, row r = p*n_chains + c (slice kk of chain c =
 * rows p in [kk*batch_size, (kk+1)*batch_size)), arrays chain-major [dim][P*n_chains].
 *
 * glabc_pool_weights, GLMCMC_NFs.py:73-85 / 128-140: x = generate_samples(theta) with Philox noise keyed by
 * (row_id0 + r), w = exp(prior(theta) + K(x) - log_q), NaN -> 0. */
int glabc_pool_weights(const glabc_model* model, const float* theta, const float* log_q, int64_t n_rows,
                       uint64_t seed, int64_t row_id0, float* x_out, float* w_out, void* stream);

/* One iteration (GLMCMC_NFs.py:90-111,141-152) for every chain: with probability global_frequency the iSIR
 * move against the chain's next pool slice -- weights cat(exp(prior + K - log_q_old), pool_w[slice]) normalised
 * with torch.sum, index by the double running sum (GLMCMC_NFs.py:11-26), kk += 1 -- else the random-walk MH
 * local move (same draws as glabc_glmcmc_steps).  log_q_old[c] = NF_model.log_prob(Theta_old) (glabc_nf_log_prob
 * on chains->theta).  run->n_steps must be 1; run->history (if any) receives the row. */
typedef struct glabc_pool {
    const float* theta;            /* [theta_dim][P*n_chains] */
    const float* x;                /* [y_dim][P*n_chains] */
    const float* w;                /* [P*n_chains] */
    const float* log_q_old;        /* [n_chains] */
    int32_t* kk;                   /* [n_chains] slices already consumed, GLMCMC_NFs.py:86,111 */
    int32_t step_size;             /* slices per pool */
    int32_t reserved;
    /* optional (all three NULL or moved_idx + n_moved set): the chains that moved in this iteration, so that the caller
     * re-evaluates NF_model.log_prob(Theta_old) (GLMCMC_NFs.py:96-98, a pure function of the state and the flow) only for
     * them -- glabc_nf_log_prob_indexed.  The order of the list is unspecified. */
    int32_t* moved_idx;            /* [n_chains] local chain indices, entries 0 .. *n_moved - 1 */
    int32_t* n_moved;              /* device counter, incremented atomically; the caller or n_moved_reset zeroes it */
    int32_t* n_moved_reset;        /* NULL or a counter this call sets to 0 (the one the NEXT iteration will count into) */
} glabc_pool;

int glabc_glmcmc_nf_step(const glabc_model* model, const glabc_dist* local, const glabc_pool* pool,
                         const glabc_chains* chains, const glabc_run* run, void* stream);

/* GLMCMC.py:52-55 -- (re)initialise log_w = prior + log-kernel - q(theta) and set
 * GLABC_FLAG_LOCAL for every chain. */
int glabc_init_weights(const glabc_model* model, const glabc_dist* importance,
                       const glabc_chains* chains, void* stream);

/* ---- split-phase iteration for Models whose callbacks are arbitrary code -------------------------------------------
 * The reference's plug-in API is the duck-typed Model protocol (examples/Mixture.py:5-53): the sampler loops call
 * ABCset.generate_samples / prior_log_prob / calculate_log_kernel (GLMCMC.py:71-74,94-97; GlobalMCMC.py:41-46,57-61).
 * A Model that cannot describe itself as a glabc_model runs one iteration in three phases:
 *
 *   glabc_propose   every random draw of the iteration (same Philox slots as the fused kernels): the branch / accept /
 *                   resampling numbers of each chain and its n_prop candidates theta' with their proposal log-density
 *   the callbacks   generate_samples, prior_log_prob, calculate_log_kernel on the candidate rows -- PyTorch on the same
 *                   device, or anything else that fills y_prop / prior_prop / kern_prop
 *   glabc_select    iSIR weights, torch.sum normalisation, double-precision index (GLMCMC.py:74-88, 7-22) or the MH test
 *                   (GLMCMC.py:96-103; GlobalMCMC.py:44-52,60-67), state update, Theta_Re row, streaming sums
 *
 * Candidate j of chain c is row r = j*n_chains + c of every candidate array (the Model sees one (n_prop*n_chains, dim)
 * row-major batch).  A chain on the local branch uses row j = 0 only (theta' = Theta_old + increment, GLMCMC.py:91); its
 * other rows still hold global candidates and are ignored by glabc_select.  All pointers are device pointers.
 * theta_dim and y_dim are free in glabc_select (loops); a descriptor proposal limits theta_dim to GLABC_MAX_DIM. */
typedef enum glabc_algo {
    GLABC_ALGO_GLMCMC = 0,         /* GLMCMC.py:58-104 */
    GLABC_ALGO_GLOBALMCMC = 1,     /* GlobalMCMC.py:37-68 */
    GLABC_ALGO_GLMALA = 2          /* GLMALA.py:150-200: the iSIR move as GLMCMC; on the local branch the caller evaluates the
                                      MALA proposal (gradient, drift, GLMALA.py:182-193) and puts theta', y', prior', K' in
                                      row c and the proposal terms log_proposal(theta', grad', Theta_old) - log q_forward in
                                      log_q[c]; glabc_select takes the accept decision.  `local` stays clear after an accepted
                                      MALA move (GLMALA.py:195-199) */
} glabc_algo;

typedef struct glabc_step_io {
    int32_t n_prop;                /* candidate rows per chain: batch_size (GLMCMC.py:66) | 1 (GlobalMCMC) */
    int32_t theta_dim;
    int32_t y_dim;
    int32_t noise_dim;             /* standard normals per candidate handed to the simulator (0 = the Model draws its own) */
    /* written by glabc_propose */
    float* theta_prop;             /* [n_prop*n_chains][theta_dim] */
    float* log_q;                  /* [n_prop*n_chains] forward()'s log_p of a global candidate (GLMCMC.py:66, GlobalMCMC.py:40) */
    float* sim_noise;              /* NULL or [n_prop*n_chains][noise_dim]: words DP + i of the candidate's Philox blocks,
                                      DP = theta_dim rounded up to even (the fused kernels' simulator draws) */
    float* log_u;                  /* [n_chains] log(torch.rand(1)), GLMCMC.py:98 */
    double* u_res;                 /* [n_chains] np.random.uniform(0,1), GLMCMC.py:17 */
    int32_t* is_global;            /* [n_chains] bit 0: torch.rand(1) < global_frequency, GLMCMC.py:59; glabc_select sets
                                      bit 1 when the chain moved in this iteration */
    /* written by the Model callbacks, read by glabc_select */
    const float* y_prop;           /* [n_prop*n_chains][y_dim]  generate_samples(theta_prop, 1) */
    const float* prior_prop;       /* [n_prop*n_chains]         prior_log_prob(theta_prop) */
    const float* kern_prop;        /* [n_prop*n_chains]         calculate_log_kernel(y_prop) */
    /* callbacks of the CURRENT state, carried from the iteration in which it was proposed (the reference re-evaluates
     * them every iteration, GLMCMC.py:61-64,97; pure functions of the state) -- maintained by glabc_select */
    float* prior_cur;              /* [n_chains] prior_log_prob(Theta_old) */
    float* kern_cur;               /* [n_chains] calculate_log_kernel(y_old) */
    const float* q_cur;            /* NULL (glabc_select evaluates the descriptor `global` at Theta_old) or [n_chains]
                                      Importance_Proposal.log_prob(Theta_old) from the caller */
    const int32_t* n_valid;        /* NULL, or [n_chains]: GLMCMC.py:67-70 removes the proposals that have a NaN coordinate BEFORE
                                      the Model sees them -- the weight vector is then shorter (torch.sum adds fewer terms, the index
                                      counts the survivors).  Only a proposal given as a callback can produce such rows; the caller
                                      moves them behind the chain's valid candidates (keeping their order) and says how many are
                                      left: glabc_select uses rows 0 .. n_valid[c]-1 of chain c.  Ignored on the local branch. */
} glabc_step_io;

/* Philox slots of the local move's redraws (GLMCMC.py:92-93): round k of a chain reads blocks GLABC_SLOT_REDRAW + k*2 + b */
#define GLABC_SLOT_REDRAW 0x40000000u

/* Draws of iteration run->step0 for every chain (run->n_steps must be 1).  `local` / `global` may be NULL: the caller then
 * fills the corresponding rows of theta_prop / log_q itself (proposal objects without a descriptor). */
int glabc_propose(int algo, const glabc_dist* local, const glabc_dist* global, const glabc_chains* chains,
                  const glabc_run* run, const glabc_step_io* io, void* stream);

/* GLMCMC.py:92-93, `while prior_log_prob(Theta_prop) == 7*log(1e-10): redraw`: for every chain on the local branch whose
 * prior_prop[c] equals the sentinel, row c of theta_prop <- Theta_old + a fresh increment (redraw round `round` >= 1) and
 * n_redrawn (device counter, caller-zeroed) is incremented.  The caller re-evaluates prior_prop and repeats until 0. */
int glabc_propose_redraw(const glabc_dist* local, const glabc_chains* chains, const glabc_run* run, const glabc_step_io* io,
                         int32_t round, int32_t* n_redrawn, void* stream);

/* The decision and the state update of iteration run->step0 (run->n_steps must be 1; run->history, if any, receives the
 * Theta_Re row; run->moments the streaming sums).  chains->log_w / flags are required for GLABC_ALGO_GLMCMC. */
int glabc_select(int algo, const glabc_dist* global, const glabc_chains* chains, const glabc_run* run,
                 const glabc_step_io* io, void* stream);

/* ---- user simulators inside the fused kernel (run-time compilation, hiprtc) ----------------------------------------------
 * The reference's generate_samples is any Python method (examples/Mixture.py:13-26).  Its GPU counterpart is a few lines of C:
 *
 *     GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
 *     {   // theta[GLABC_THETA_DIM], eps[GLABC_NOISE_DIM] standard normals -> y[GLABC_Y_DIM]
 *         for (int j = 0; j < GLABC_Y_DIM; ++j) y[j] = fabsf(theta[j]) + 0.2236068f * eps[j];
 *     }
 *
 * glabc_rtc_compile builds the library's own sampler code (Philox slots, proposals, prior, discrepancy ||y - y_obs||, Gaussian
 * ABC kernel, iSIR / MH decisions, history, sums -- the source of the built-in kernels, embedded in the library) around that
 * function for one configuration (algorithm, dimensions, batch size) and returns a handle; glabc_rtc_steps is then
 * glabc_glmcmc_steps / glabc_globalmcmc_steps for a glabc_model with sim_kind = GLABC_SIM_USER (noise.dim = the normals the
 * simulator consumes).  Written with + - * / fma, sqrtf and the glabc_* functions of glabc_numerics.h the simulator gives
 * results a CPU build of the same source reproduces bit for bit.  log (may be NULL) receives the compiler's messages. */
typedef struct glabc_rtc_program glabc_rtc_program;
int glabc_rtc_compile(const char* simulator_source, int32_t algo, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                      int32_t batch_size, glabc_rtc_program** out, char* log, int64_t log_size);
/* GLMCMC only: one program serves every batch size 17..GLABC_MAX_BATCH_WIDE (N is a launch argument of wide_kernel).  The
 * lane-group kernel of glabc_glmcmc_steps above GLABC_MAX_BATCH (8 / 16 / 32 / 64 lanes of a wavefront share a chain's proposals)
 * compiled around the same user source, hooks included; glabc_rtc_steps then takes run->batch_size 17..GLABC_MAX_BATCH_WIDE and
 * run->lanes_per_chain 0 (the library's choice, as for the built-in Models), 8, 16, 32 or 64, and refuses with GLABC_ERR_ARG a
 * batch size of 16 or less and an (N, lanes) pair whose 4 (256 / lanes) (N + 33) bytes of group rows exceed what the device
 * gives a workgroup.  glabc_rtc_simulate / glabc_rtc_hooks / glabc_rtc_model_rows accept such a program unchanged. */
int glabc_rtc_compile_wide(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                           glabc_rtc_program** out, char* log, int64_t log_size);
/* The two entry points above with `flags`: 0 builds exactly what they build; any bit but GLABC_RTC_GAMMA is GLABC_ERR_ARG.
 * GLABC_RTC_GAMMA: the program also holds the kernels of a GLABC_DIST_GAMMA prior and / or importance / global proposal, and
 * glabc_rtc_steps accepts such descriptors on it (on any other program they are GLABC_ERR_ARG; `local` is never a Gamma).
 *   register program  the generic kernels as without the flag, less the unit-Gaussian variants (speed only), plus the Gamma entry at
 *                     one lane per chain (whatever lane count the generic entry was given) and, for GLMCMC, its teams of two and
 *                     three wavefronts where the batch's candidates fit the LDS budget; GlobalMCMC with a Gamma runs the one-lane entry
 *   wide program      wide_kernel with and without the Gamma at 8 / 16 / 32 / 64 lanes; spill notes of both go to `log`
 * A launch whose prior and global proposal are no Gamma runs the generic kernels of the same program.  With a user prior hook
 * (GLABC_USER_PRIOR) the hook stays the prior and only the proposal is the Gamma. */
#define GLABC_RTC_GAMMA 1u
int glabc_rtc_compile_ex(const char* simulator_source, int32_t algo, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                         int32_t batch_size, uint32_t flags, glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_compile_wide_ex(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim, uint32_t flags,
                              glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_steps(const glabc_rtc_program* program, const glabc_model* model, const glabc_dist* local, const glabc_dist* global,
                    const glabc_chains* chains, const glabc_run* run, void* stream);
/* generate_samples(theta, 1) of the compiled simulator on n row-major points: theta[n][theta_dim], eps[n][noise_dim] -> y[n][y_dim] */
int glabc_rtc_simulate(const glabc_rtc_program* program, const float* theta, const float* eps, int64_t n, float* y, void* stream);
void glabc_rtc_release(glabc_rtc_program* program);

/* The Model's OTHER callbacks as user source (examples/Mixture.py:28-45 are Python methods too).  The same source string may
 * define, each announced by a #define in that source, any of
 *     #define GLABC_USER_PRIOR 1
 *     GLABC_SIMULATOR float glabc_user_prior_log_prob(const float* theta)               // prior_log_prob, Mixture.py:28-31
 *     #define GLABC_USER_DISCREPANCY 1
 *     GLABC_SIMULATOR float glabc_user_discrepancy(const float* y, const float* y_obs)  // discrepancy, Mixture.py:33-36
 *     #define GLABC_USER_KERNEL 1
 *     GLABC_SIMULATOR float glabc_user_log_kernel(float dis, float scale)               // calculate_log_kernel of a discrepancy,
 *                                                                                      // Mixture.py:38-45; scale = model->kern_scale
 * and the fused kernel calls them where it would evaluate the descriptor's prior / Euclidean discrepancy / Gaussian kernel
 * (a callback that is not announced stays the descriptor's; model->prior must still be a valid placeholder).  glabc_rtc_hooks
 * reports what a program replaces; glabc_rtc_model_rows evaluates prior_log_prob (user priors only: descriptor priors have
 * glabc_model_prior_log_prob), discrepancy or calculate_log_kernel on n row-major points through the very functions the fused
 * kernel calls: in[n][theta_dim] or in[n][y_dim] -> out[n]. */
#define GLABC_RTC_PRIOR_LOG_PROB 0
#define GLABC_RTC_DISCREPANCY 1
#define GLABC_RTC_LOG_KERNEL 2
int glabc_rtc_hooks(const glabc_rtc_program* program, int32_t* user_prior, int32_t* user_discrepancy, int32_t* user_kernel);
int glabc_rtc_model_rows(const glabc_rtc_program* program, const glabc_model* model, int32_t what, const float* in, int64_t n,
                         float* out, void* stream);

/* generate_samples(theta, 1) of a descriptor Model on n row-major points (Mixture.py:13-26 regime n x 1):
 * theta[n][theta_dim], eps[n][y_dim] standard normals (NULL: drawn from Philox(seed; row0 + r, 0, b), pairs of words)
 * -> y[n][y_dim].  The standalone form of the simulator the fused kernels inline. */
int glabc_model_simulate(const glabc_model* model, const float* theta, const float* eps, int64_t n, uint64_t seed,
                         int64_t row0, float* y, void* stream);

/* distribution.py:176-181 / 81-86 / 123-137: log_prob of n row-major points z[n][dim] -> out[n]. */
int glabc_dist_log_prob(const glabc_dist* dist, const float* z, int64_t n, float* out, void* stream);

/* BaseDistribution.forward(n), distribution.py:165-173 / 73-78, drawn on the device: row r (global id row0 + r)
 * takes its dim variates from Philox(seed; id, 0, b), b = 0..ceil(dim/4)-1 -- DiagGaussian: Box-Muller pairs of
 * words (2i, 2i+1), z = loc + exp(log_scale)*eps; Uniform: one float32 uniform per word, z = low + (high-low)*u --
 * and returns forward()'s log_p.  z_out is dimension-major [dim][n]. */
int glabc_dist_forward(const glabc_dist* dist, int64_t n, uint64_t seed, int64_t row0, float* z_out, float* log_p_out,
                       void* stream);

/* Gamma.log_prob, distribution.py:123-137: float64, log(scipy.stats.gamma.pdf(z, shape, scale=1/rate)) with -inf where
 * the pdf is 0 (it underflows earlier than a logpdf would -- reproduced), summed over the dimensions.
 *   pdf_j = exp((shape_j - 1) log(x) - x - gammaln(shape_j)) / scale_j,  x = z_j / scale_j,  0 outside x > 0
 * gammaln[] is supplied by the caller (scipy.special.gammaln(shape) on the host; a constant of the distribution).
 * z[n][dim] row-major float64 -> out[n] float64. */
typedef struct glabc_gamma {
    int32_t dim;
    int32_t reserved;
    double shape[GLABC_MAX_DIM];
    double scale[GLABC_MAX_DIM];   /* 1/rate as the reference forms it (float32 reciprocal, distribution.py:133) */
    double gammaln[GLABC_MAX_DIM];
} glabc_gamma;

int glabc_gamma_log_prob(const glabc_gamma* dist, const double* z, int64_t n, double* out, void* stream);

/* Gamma.forward(n), distribution.py:106-121, drawn on the device: z[r][j] = glabc_gamma_draw(shape_j; Philox(seed; row0 + r,
 * j, attempt)) * scale_j (include/glabc_numerics.h: Marsaglia-Tsang in double; the reference draws scipy.stats.gamma.rvs from
 * NumPy's generator) and log_p[r] = Gamma.log_prob(z[r]).  z_out[n][dim] row-major float64, log_p_out[n] float64. */
int glabc_gamma_forward(const glabc_gamma* dist, int64_t n, uint64_t seed, int64_t row0, double* z_out, double* log_p_out,
                        void* stream);

/* ---- GaussianMixture, distribution.py:206-293: a mixture of diagonal Gaussians as the importance / global proposal ------------
 * The reference's mixture is float64 end to end (its parameters are float64 tensors); the chains' state is float32 here, so, as
 * for GLABC_DIST_GAMMA above, everything is computed in double and rounded once to the float32 state.  The constants are
 * formed on the HOST in float64 (the Python class, with torch / numpy) and cross the ABI as numbers:
 *   loc[k][q]; scale[k][q] = torch.exp(log_scale); inv_scale[k][q] = 1.0 / scale; log_weight[k] = torch.log(torch.softmax(
 *   weight_scores, 1)); cum_weight[k] = np.cumsum(softmax weights); sum_log_scale[k] = torch.sum(log_scale, 2);
 *   c0 = -0.5 * dim * np.log(2 * np.pi).
 * log_prob(z), z in double (distribution.py:284-291):
 *   S_k = sum_q ((z_q - loc[k][q]) * inv_scale[k][q])^2     each square one multiplication, the sum in torch.sum's float64 order
 *   t_k = ((c0 + log_weight[k]) - 0.5 * S_k) - sum_log_scale[k]
 *   m + glabc_log(sum_k glabc_exp(t_k - m)),  m = max_k t_k, 0 if that is infinite; the sum over k in the same row-sum order
 * with no contraction into fma anywhere.  ONE DEVIATION from the reference's arithmetic: (z - loc) is MULTIPLIED by the
 * host-formed reciprocal inv_scale instead of divided by scale -- a float64 division per mode, coordinate and evaluation would
 * be the most expensive operation of the loop.  The result is therefore not bit-identical to torch's; it stays within
 * 1e-12 * max(1, |value|) of it (tests/test_mixture_host.py), the bound the Gamma density is held to.
 * forward inside a sampler, candidate j of (chain, iteration):
 *   u = glabc_uniform_f64(w0, w1) of the Philox block at counter (chain lo, chain hi, iteration, GLABC_SLOT_MIX + j)
 *   mode k = the first k with u < cum_weight[k], else n_modes - 1
 *   eps_q = the candidate's ordinary proposal normals (words 0..dim-1 of its blocks, Box-Muller pairs) promoted to double
 *   z_q = eps_q * scale[k][q] + loc[k][q] (two roundings), theta'_q = (float) z_q, log q' = (float) log_prob(z) -- the density
 *   of the DOUBLE variate, as for Gamma.  log_prob of a float32 state is (float) log_prob((double) theta).
 * Existing draws are untouched (GLABC_STREAM_LAYOUT stays 2).
 * On a GLABC_SIM_USER Model the same kernels are compiled around the user's source at run time, for theta_dim 1..8 and any y_dim /
 * noise_dim (glabc_rtc_compile_mix / glabc_rtc_compile_wide_mix / glabc_rtc_mix_steps, below).
 * Where the fused samplers take it (glabc_glmcmc_mix_steps / glabc_globalmcmc_mix_steps / glabc_init_weights_mix): GLABC_SIM_ABS_GAUSS
 * with theta_dim 1..4 and GLABC_SIM_GK, batch size 1..GLABC_MAX_BATCH, prior and local increment DiagGaussian or Uniform, with
 * history, moments, global_frequency_per_chain and GLABC_DEBUG_EXACT_INDEX; one lane per chain in the default schedule
 * (lanes_per_chain 0 or 1).  Refused: theta_dim 5..8 and a Gamma prior (GLABC_ERR_KIND), a tape and GLABC_MATH_FAST
 * (GLABC_ERR_ARG), n_modes outside 1..GLABC_MAX_MODES (GLABC_ERR_ARG), dim != theta_dim (GLABC_ERR_DIM), a scale or inv_scale
 * that is not finite and > 0, a non-monotone cum_weight or a last cum_weight outside (0, 1 + 1e-9] (GLABC_ERR_ARG).
 * Batch sizes GLABC_MAX_BATCH + 1..GLABC_MAX_BATCH_WIDE of GLMCMC (glabc_glmcmc_mix_wide_steps): the same matrix, refusals and
 * order of checks, in the lane-group kernel -- lanes_per_chain 0 (wide_default_lanes: 8 / 16 / 32 / 64 for a batch size up to 64 /
 * 128 / 256 / above) or 8 / 16 / 32 / 64, anything else and a batch size outside that range, 1..GLABC_MAX_BATCH included, is
 * GLABC_ERR_ARG; a launch whose group rows (4 (256 / lanes) (batch_size + 33) bytes of LDS) the device cannot give a workgroup is
 * GLABC_ERR_LAUNCH and launches nothing.  Candidate j reads the same slots and words at every batch size (GLABC_SLOT_MIX + j,
 * j < 4096); glabc_init_weights_mix serves both entry points. */
#define GLABC_MAX_MODES 8
typedef struct glabc_mixture {
    int32_t n_modes;               /* 1..GLABC_MAX_MODES */
    int32_t dim;                   /* 1..GLABC_MAX_DIM */
    double loc[GLABC_MAX_MODES][GLABC_MAX_DIM];
    double scale[GLABC_MAX_MODES][GLABC_MAX_DIM];
    double inv_scale[GLABC_MAX_MODES][GLABC_MAX_DIM];
    double log_weight[GLABC_MAX_MODES];
    double cum_weight[GLABC_MAX_MODES];
    double sum_log_scale[GLABC_MAX_MODES];
    double c0;
} glabc_mixture;

/* GaussianMixture.log_prob: z[n][dim] row-major float64, dim 1..8 -> out[n] float64 (mirrors glabc_gamma_log_prob). */
int glabc_mixture_log_prob(const glabc_mixture* dist, const double* z, int64_t n, double* out, void* stream);

/* GaussianMixture.forward(n) drawn on the device, in the layout of glabc_kde_sample: row r (global id row0 + r) reads
 * Philox(seed; id lo, id hi, 0, b): the mode uniform from words 0-1 of block 0, the normals from words 2-3 of block 0, then
 * blocks 1 and up.  z_out[n][dim] row-major float64, log_p_out[n] = log_prob(z_out[r]). */
int glabc_mixture_forward(const glabc_mixture* dist, int64_t n, uint64_t seed, int64_t row0, double* z_out, double* log_p_out,
                          void* stream);

/* glabc_init_weights / glabc_glmcmc_steps / glabc_globalmcmc_steps with a mixture as the importance / global proposal. */
int glabc_init_weights_mix(const glabc_model* model, const glabc_mixture* importance, const glabc_chains* chains, void* stream);
int glabc_glmcmc_mix_steps(const glabc_model* model, const glabc_dist* local, const glabc_mixture* importance,
                           const glabc_chains* chains, const glabc_run* run, void* stream);
int glabc_globalmcmc_mix_steps(const glabc_model* model, const glabc_dist* local, const glabc_mixture* global,
                               const glabc_chains* chains, const glabc_run* run, void* stream);
int glabc_glmcmc_mix_wide_steps(const glabc_model* model, const glabc_dist* local, const glabc_mixture* importance,
                                const glabc_chains* chains, const glabc_run* run, void* stream);

/* glabc_glmala_steps with a mixture as the importance proposal of the iSIR global move (GLMALA.py:151-180); glabc_glmala_init serves
 * it unchanged (it does not look at the proposal).  The move's proposal is the mixture exactly as glabc_glmcmc_mix_steps has it:
 * candidate j of (chain, iteration) takes its mode uniform from the Philox block at slot GLABC_SLOT_MIX + j, eps are the candidate's
 * ordinary proposal NORMALS (the words glabc_glmala_steps reads for a DiagGaussian proposal), z = eps * scale + loc in double,
 * theta' = (float) z, log q' = (float) log_prob(z).  The current state's slot follows GLMALA's dtype bookkeeping (GLABC_FLAG_TH64 /
 * GLABC_FLAG_LW64, GLMALA.py:152-156): a float32 state uses q = (float) log_prob((double) theta) and float32 weights; a float64 state
 * uses log_prob(theta64) UNROUNDED in log_w and sets GLABC_FLAG_LW64.  The reference's GaussianMixture holds float64 parameters and
 * would promote more than this (a float32 state's weight, every candidate's weight): as for the GLMCMC mixture entry points the
 * density is float64, rounded once to the float32 state.  No existing draw, slot or struct changes: the MALA local move, the
 * gradient noise slots and log_w's lifetime are glabc_glmala_steps', and a chain on the local branch computes exactly what it
 * computes there.
 * Scope: GLABC_SIM_ABS_GAUSS with theta_dim 1..4, batch size 1..GLABC_MAX_BATCH, 1..GLABC_MAX_MODES modes, a DiagGaussian or Uniform
 * prior, lanes_per_chain 0 / 1 / 2 as for glabc_glmala_steps, with history and moments.
 * Checks, first defect wins (glabc_glmala_steps' order, the mixture's own checks where it checks its importance proposal):
 *   the model (a null pointer GLABC_ERR_NULL, then what glabc_glmala_steps refuses of a model: a Gamma prior is GLABC_ERR_KIND);
 *   sim_kind != GLABC_SIM_ABS_GAUSS (GLABC_ERR_KIND); theta_dim 5..8 (GLABC_ERR_DIM, the status glabc_glmala_steps gives it, but
 *   here ahead of everything that follows);
 *   the mixture: null (GLABC_ERR_NULL), n_modes outside 1..GLABC_MAX_MODES (GLABC_ERR_ARG), dim != theta_dim (GLABC_ERR_DIM), its
 *   tables as glabc_glmcmc_mix_steps checks them (GLABC_ERR_ARG);
 *   null mala / run (GLABC_ERR_NULL); the chains' pointers, theta64 / y64 / log_w64 / grad / flags included (GLABC_ERR_NULL), and range
 *   (GLABC_ERR_ARG); n_steps < 0 or a batch size outside 1..GLABC_MAX_BATCH (GLABC_ERR_ARG); a NaN global_frequency (GLABC_ERR_ARG);
 *   global_frequency_per_chain (GLABC_ERR_ARG); num_grad outside 2..65536, tau not finite and > 0, tau_sq not finite, eps_sq not
 *   finite and >= 0 (GLABC_ERR_ARG); hist_stride < n_chains (GLABC_ERR_ARG); incomplete moments (GLABC_ERR_NULL); a tape,
 *   GLABC_MATH_FAST or dump_draws (GLABC_ERR_ARG); lanes_per_chain outside 0..2 (GLABC_ERR_ARG); step0 + n_steps past 2^32
 *   (GLABC_ERR_ARG).  Then n_chains == 0 or n_steps == 0 returns GLABC_OK and touches nothing. */
int glabc_glmala_mix_steps(const glabc_model* model, const glabc_mixture* importance, const glabc_mala* mala,
                           const glabc_chains* chains, const glabc_run* run, void* stream);

/* The mixture variant around a USER simulator (GLABC_SIM_USER): glabc_rtc_compile / glabc_rtc_compile_wide with the kernels of the
 * three entry points above instead of the generic ones -- sampler_kernel<.., VAR_MIX> at one lane per chain for one (algorithm,
 * batch size 1..GLABC_MAX_BATCH), or the lane-group kernel's mixture variant at 8 / 16 / 32 / 64 lanes per chain for any batch size
 * GLABC_MAX_BATCH + 1..GLABC_MAX_BATCH_WIDE -- for theta_dim, y_dim and noise_dim 1..GLABC_MAX_DIM each, user hooks included.  New entry
 * points, not a `flags` bit of the _ex calls.  Register or scratch spills of a kernel are named in `log` (slower, never wrong).
 * glabc_rtc_simulate / glabc_rtc_hooks / glabc_rtc_model_rows / glabc_rtc_release take such a program unchanged; glabc_rtc_steps
 * refuses it (GLABC_ERR_KIND), as glabc_rtc_mix_steps refuses a program of the other kind.
 * glabc_rtc_mix_steps names its kernel itself (no launch plan): a register program takes its compiled batch size at lanes_per_chain
 * 0 or 1, a wide program 17..4096 at lanes_per_chain 0 (wide_default_lanes) or 8 / 16 / 32 / 64.  Checks, first defect wins: a null
 * pointer (GLABC_ERR_NULL); sim_kind != GLABC_SIM_USER (GLABC_ERR_KIND); theta_dim / y_dim / noise.dim other than the program's
 * (GLABC_ERR_DIM); a program not compiled by the two calls below (GLABC_ERR_KIND); a Gamma prior (GLABC_ERR_KIND); an invalid prior,
 * local increment or kernel scale (GLABC_ERR_ARG); a tape, GLABC_MATH_FAST or dump_draws (GLABC_ERR_ARG); the mixture's own checks as
 * glabc_glmcmc_mix_steps makes them; the chains; n_steps < 0, step0_device, batch size and lanes_per_chain (GLABC_ERR_ARG);
 * global_frequency, history, moments and the step counter as every stepping entry point.  Then, for a wide program, group rows
 * that with the kernel's static LDS exceed what the device gives a workgroup: GLABC_ERR_ARG, before anything runs.  The chains start
 * as for glabc_rtc_steps (GLABC_FLAG_LOCAL set: log_w is computed at the first global move), so there is no init-weights twin. */
/* glabc_propose(algo, local, NULL, ...) with the rows it leaves to the caller filled from a GaussianMixture, in the same launch: the
 * split-phase twin of the mixture kernels, drawing from the kernel's Philox stream.  Head draws, is_global, the local move's row and
 * every candidate's sim_noise are glabc_propose's.  On top: theta_prop and log_q of every row j > 0, and of row 0 for chains whose
 * is_global bit 0 is set, are what the fused kernels compute (above: mode uniform at GLABC_SLOT_MIX + j, the candidate's proposal
 * normals promoted to double, z = eps * scale + loc, theta' = (float) z, log q' = (float) log_prob(z)); and io->q_cur[c] =
 * (float) log_prob((double) Theta_old) is WRITTEN for every chain, for glabc_select(algo, NULL, ...) to read.  algo GLABC_ALGO_GLMCMC /
 * GLABC_ALGO_GLOBALMCMC (else GLABC_ERR_KIND), theta_dim 1..8 (GLABC_ERR_DIM), then the mixture's checks as glabc_glmcmc_mix_steps makes
 * them (the mixture against io->theta_dim, the local increment -- which may be NULL as for glabc_propose --, null chains / run, a
 * tape), a null io->q_cur (GLABC_ERR_NULL), then glabc_propose's own checks. */
int glabc_propose_mix(int algo, const glabc_dist* local, const glabc_mixture* global, const glabc_chains* chains,
                      const glabc_run* run, const glabc_step_io* io, void* stream);

int glabc_rtc_compile_mix(const char* simulator_source, int32_t algo, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                          int32_t batch_size, glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_compile_wide_mix(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                               glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_mix_steps(const glabc_rtc_program* program, const glabc_model* model, const glabc_dist* local,
                        const glabc_mixture* global, const glabc_chains* chains, const glabc_run* run, void* stream);

/* Model callbacks on n row-major points (Mixture.py:28-45): used by the host
 * mirror's Model class and by the parity tests. */
int glabc_model_prior_log_prob(const glabc_model* model, const float* theta, int64_t n, float* out, void* stream);
int glabc_model_discrepancy(const glabc_model* model, const float* y, int64_t n, float* out, void* stream);
int glabc_model_log_kernel(const glabc_model* model, const float* y, int64_t n, float* out, void* stream);

/* ESJD.py:2-25 for a batch of chains: history [n_rows][theta_dim][stride]
 * (chain-major, as written by the samplers) -> esjd[n_chains] =
 * det(D^T D / (n_rows-1))^(1/theta_dim), D = consecutive differences. */
int glabc_esjd(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride,
               float* esjd_out, void* stream);

/* The same quantity from the streamed jump sums (glabc_moments.sum_jump after n_steps
 * iterations): esjd[c] = det(sum_jump_c / n_steps)^(1/theta_dim).  No history needed. */
int glabc_moments_esjd(const glabc_moments* moments, int64_t n_steps, int32_t theta_dim, int64_t n_chains,
                       int64_t stride, float* esjd_out, void* stream);

/* ---- chain diagnostics: per-chain means and lagged autocovariances of a history, the sufficient statistics of split-R-hat and
 * of the effective sample size (glabcmcmc_amd/diagnostics.py forms both from them).
 *
 * history is [n_rows][theta_dim][stride] float32, chain-major: what the samplers write and glabc_esjd reads; columns
 * n_chains .. stride - 1 are never read.  The outputs are dense, with output stride n_chains:
 *     mean_out[j * n_chains + c]                          j < theta_dim
 *     acov_out[(k * theta_dim + j) * n_chains + c]        k = 0 .. max_lag
 *
 * Numerical specification.  For every chain c and coordinate j, with x_t = history[t][j][c]: all arithmetic is IEEE double, every
 * line is one rounded operation in the stated order, and there is no FMA (the object is built with -ffp-contract=off, as the
 * rest of the numerical contract is):
 *     S = 0.0;    for t = 0 .. n_rows - 1 ascending:  S = S + (double) x_t;            m = S / (double) n_rows
 *     u_t = (double) x_t - m
 *     A_k = 0.0;  for t = k .. n_rows - 1 ascending:  A_k = A_k + u_t * u_{t-k};        acov_k = A_k / (double) n_rows
 * (the biased 1/n normalisation of Geyer and of Stan).  The order is fixed per (chain, coordinate, lag), so the result does not
 * depend on the launch geometry, and a float64 loop on the host reproduces it bit for bit.  A NaN or an infinity in a chain makes
 * that chain's mean of that coordinate non-finite and acov_k NaN at every lag that pairs the row with another (all of them when
 * the row is the first or max_lag is at most its index), as the lines above say; no other chain or coordinate is touched.
 *
 * Refusals, in this order; a refused call launches nothing and writes nothing: a null pointer GLABC_ERR_NULL; theta_dim outside
 * 1 .. GLABC_MAX_DIM GLABC_ERR_DIM; n_rows < 1, n_chains < 0, stride < n_chains, max_lag < 0, max_lag > n_rows - 1 or
 * max_lag > GLABC_MAX_LAG GLABC_ERR_ARG.  n_chains == 0 returns GLABC_OK and writes nothing. */
#define GLABC_MAX_LAG 4096
int glabc_autocov(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride,
                  int32_t max_lag, double* mean_out, double* acov_out, void* stream);

/* ---- posterior quantiles and marginal histograms of a history: integer counts, exact and additive over shards of chains and
 * slices of rows (glabcmcmc_amd/diagnostics.py drives a three-pass radix selection with them).  The history is glabc_autocov's:
 * [n_rows][theta_dim][stride] float32, columns n_chains .. stride - 1 never read; its base needs 4-byte alignment only.
 *
 * Key.  The order-preserving uint32 of a float32 x with bit pattern u: x == 0 takes the bits of +0.0 (-0 and +0 are one value);
 * key = ~u when the sign bit is set and u | 0x80000000 otherwise; every NaN has key 0xFFFFFFFF (NaNs sort last, as in
 * numpy.sort).  unkey is the inverse: +0.0 for the zero's key, a NaN for 0xFFFFFFFF.
 *
 * Levels.  Level 0, 1, 2 is (prefix bits, digit bits) = (0, 11), (11, 11), (22, 10).  A value with key k belongs to prefix p at
 * a level when the level has no prefix bits or k >> (32 - prefix_bits) == p; its digit is
 * (k >> (32 - prefix_bits - digit_bits)) & (2^digit_bits - 1).
 *
 * glabc_key_counts: for every coordinate j and slot s < n_prefixes, ADDS to counts[(j * n_prefixes + s) << digit_bits | digit]
 * the number of values of coordinate j that belong to prefixes[j * n_prefixes + s] -- the caller zeroes `counts`, so slabs of
 * chains and slices of rows accumulate into one table.  `prefixes` is a HOST array (it travels as kernel arguments), `counts` a
 * device array of uint64.  A slot holding 0xFFFFFFFF is unused: its row of counts is not touched.  Level 0 needs n_prefixes == 1
 * and ignores the prefix word.  The counts are integers, so they are the same bits whatever the launch geometry and the order
 * of the atomic adds.
 *
 * Refusals, in this order; a refused call launches nothing and writes nothing: a null pointer GLABC_ERR_NULL; theta_dim outside
 * 1 .. GLABC_MAX_DIM GLABC_ERR_DIM; n_rows < 1, n_chains < 0, stride < n_chains, level outside 0 .. 2, n_prefixes outside
 * 1 .. GLABC_MAX_PREFIXES (or not 1 at level 0), a used prefix >= 2^prefix_bits, or two equal used prefixes of one coordinate
 * GLABC_ERR_ARG.  n_chains == 0 returns GLABC_OK and writes nothing. */
#define GLABC_MAX_PREFIXES 8
int glabc_key_counts(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t level,
                     int32_t n_prefixes, const uint32_t* prefixes, uint64_t* counts, void* stream);

/* glabc_histogram: per coordinate j, n_bins equal bins over [lo[j], hi[j]] and three more slots, counts[j * (n_bins + 3) + slot]
 * (device, uint64; the call ADDS, the caller zeroes).  lo and hi are HOST arrays.  Numerical specification, IEEE double, every
 * operation rounded once, no FMA:
 *     scale = (double) n_bins / (hi - lo)                                  on the host, per coordinate
 *     u = ((double) x - lo) * scale;   b = (int64) floor(u)                per value
 *     NaN -> slot n_bins + 2;  x < lo -> slot n_bins (below);  x > hi -> slot n_bins + 1 (above);
 *     x == hi -> bin n_bins - 1 (NumPy's closed last bin);  otherwise bin min(b, n_bins - 1)
 * Refusals as for glabc_key_counts, with GLABC_ERR_ARG for n_bins outside 1 .. GLABC_MAX_BINS and for a lo or hi that is not
 * finite or not lo < hi. */
#define GLABC_MAX_BINS 4096
int glabc_histogram(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_bins,
                    const double* lo, const double* hi, uint64_t* counts, void* stream);

/* ---- the joint posterior of a history: pair histograms (integer counts, additive over shards of chains and slices of rows) and
 * per-chain cross moments, the sufficient statistics of the posterior covariance (glabcmcmc_amd/diagnostics.py forms the covariance,
 * the correlation and the highest-density levels of a contour plot from them).  The history is glabc_autocov's in both:
 * [n_rows][theta_dim][stride] float32, columns n_chains .. stride - 1 never read; its base needs 4-byte alignment only.
 *
 * glabc_histogram2d: every pair p = (a, b) = (pairs[2p], pairs[2p + 1]) of coordinates has a table of n_bins^2 + 2 slots,
 * counts[p * (n_bins^2 + 2) + slot] (device, uint64; the call ADDS, the caller zeroes).  pairs, lo and hi are HOST arrays.  Each of
 * the two values of a draw (row t, chain c) is binned by glabc_histogram's rule on its own coordinate -- the same double
 * arithmetic, scale = (double) n_bins / (hi - lo) formed on the host, x == hi in the last bin, every operation rounded once, no
 * FMA -- and the draw adds one to
 *     slot n_bins^2 + 1                  if either value is a NaN
 *     slot n_bins^2                      otherwise, if either value is below its lo or above its hi
 *     slot bin_a * n_bins + bin_b        otherwise
 * (a, b) and (b, a) are both legal and each other's transposes; a pair may repeat, each occurrence has its own table.  The counts
 * are integers: the same bits whatever the launch geometry.
 *
 * Refusals, in this order; a refused call launches nothing and writes nothing: a null pointer GLABC_ERR_NULL; theta_dim outside
 * 1 .. GLABC_MAX_DIM GLABC_ERR_DIM; n_rows < 1, n_chains < 0, stride < n_chains, n_pairs outside 1 .. GLABC_MAX_PAIRS, a pair
 * member outside 0 .. theta_dim - 1 or a == b, n_bins outside 1 .. GLABC_MAX_JOINT_BINS, and -- for a coordinate that a pair
 * uses; the others' lo and hi are not looked at -- a lo or hi that is not finite or not lo < hi GLABC_ERR_ARG.  n_chains == 0
 * returns GLABC_OK and writes nothing. */
#define GLABC_MAX_PAIRS 28          /* GLABC_MAX_DIM (GLABC_MAX_DIM - 1) / 2 */
#define GLABC_MAX_JOINT_BINS 128
int glabc_histogram2d(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_pairs,
                      const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, uint64_t* counts, void* stream);

/* glabc_cross_moments: per chain, the means and the biased (1/n) covariance of every pair of coordinates.  The outputs are dense
 * device arrays with output stride n_chains, the covariance as the packed upper triangle:
 *     mean_out[j * n_chains + c]                          j < theta_dim, as glabc_autocov's
 *     cov_out[q * n_chains + c]                           q = i * theta_dim - i (i - 1) / 2 + (j - i),   i <= j < theta_dim
 * Numerical specification.  All arithmetic is IEEE double, every line one rounded operation in the stated order, no FMA.  With
 * m and u_t per coordinate as in glabc_autocov:
 *     A = 0.0;  for t = 0 .. n_rows - 1 ascending:  A = A + u_t,i * u_t,j;        cov = A / (double) n_rows
 * so the diagonal entries are glabc_autocov's acov_0 bit for bit, and the result does not depend on the launch geometry.  A NaN
 * or an infinity in a chain propagates as the lines say: into that chain's entries of the coordinates involved, nowhere else.
 *
 * Refusals, in this order; a refused call launches nothing and writes nothing: a null pointer GLABC_ERR_NULL; theta_dim outside
 * 1 .. GLABC_MAX_DIM GLABC_ERR_DIM; n_rows < 1, n_chains < 0 or stride < n_chains GLABC_ERR_ARG.  n_chains == 0 returns GLABC_OK
 * and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged by both: no struct changes. */
int glabc_cross_moments(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, double* mean_out,
                        double* cov_out, void* stream);

/* ---- plain rejection ABC: prior draw -> simulation -> distance -> the Model's own acceptance, one fused kernel (csrc/glabc_abc.hip).
 * What picks a tolerance (a quantile of the prior-predictive distances), starts chains (the nearest draws) and samples the
 * samplers' target independently of them (glabcmcmc_amd/rejection.py).
 *
 * Draw r < n has the 64-bit id  ids ? ids[r] : row0 + r.  `ids` is a DEVICE array; it may hold any order, repeats and values >= 2^32.
 * The outputs are device arrays.  theta_out / y_out are dimension-major with stride `stride` >= n, the layout of glabc_chains:
 *     theta_out[j * stride + r]   j < theta_dim          y_out[j * stride + r]   j < y_dim
 * and columns n .. stride - 1 are never written; dis_out[r] (float32) and accept_out[r] (one byte, 0 or 1) are dense.  Each output
 * may be NULL, but not all four; what only a NULL output needs is neither computed nor stored.
 *
 * Specification of a draw.  The result depends on (model, seed, id) only -- never on n, row0, the position in `ids` or the launch
 * geometry -- and restates three entry points above.  With id_lo / id_hi the two words of the id:
 *     theta  = row id of glabc_dist_forward(&model->prior, ., seed, .): the Philox blocks (seed; id_lo, id_hi, 0, b),
 *              b < ceil(theta_dim / 4), DiagGaussian: Box-Muller pairs of words (2i, 2i + 1), Uniform: one float32 uniform per word,
 *              theta_j = p0_j + p2_j * e_j (two rounded operations)
 *     y      = glabc_model_simulate(model, theta, eps = NULL, seed ^ GLABC_ABC_NOISE_KEY, id): the same counters under another key,
 *              so theta and the noise are independent
 *     dis    = glabc_model_discrepancy(model, y)
 *     u      = glabc_uniform_f32(word 0 of Philox(seed ^ GLABC_ABC_ACCEPT_KEY; id_lo, id_hi, 0, 0))
 *     e      = (dis - 0.0f) / kern_scale
 *     p      = glabc_expf(-(0.5f * (e * e)))                       K_eps(dis) / K_eps(0) of calculate_log_kernel, Mixture.py:38-45
 *     accept = u < p ? 1 : 0
 * every line one rounded float32 operation per operator (no FMA: -ffp-contract=off), so a NaN distance gives accept = 0.
 *
 * Models: GLABC_SIM_ABS_GAUSS with theta_dim == y_dim in 1 .. GLABC_MAX_DIM, and GLABC_SIM_GK (4, 8); the prior DiagGaussian or Uniform.
 * Refusals, in this order; a refused call launches nothing and writes nothing:
 *   a NULL model, or all four outputs NULL                                                        GLABC_ERR_NULL
 *   theta_dim or y_dim outside 1 .. GLABC_MAX_DIM, GLABC_SIM_GK not (4, 8), GLABC_SIM_ABS_GAUSS with y_dim != theta_dim    GLABC_ERR_DIM
 *   GLABC_SIM_USER (or an unknown kind), a prior that is not DiagGaussian / Uniform, a prior whose dim != theta_dim       GLABC_ERR_KIND
 *   n < 0, stride < n, row0 < 0, or row0 != 0 together with ids                                    GLABC_ERR_ARG
 * n == 0 returns GLABC_OK and writes nothing.  The parameters' values are not examined (a scale of 0 draws a constant).
 * GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes and no existing draw moves. */
#define GLABC_ABC_NOISE_KEY  0x9E3779B97F4A7C15ull
#define GLABC_ABC_ACCEPT_KEY 0xD1B54A32D192ED03ull
int glabc_abc_draws(const glabc_model* model, uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride,
                    float* theta_out, float* y_out, float* dis_out, uint8_t* accept_out, void* stream);

/* ---- coverage checks on pseudo-observed data: is epsilon small enough for the credible intervals to be trusted?  One fused kernel
 * (csrc/glabc_coverage.hip; glabcmcmc_amd/coverage.py forms ranks, rank histograms and interval coverage from its sums).  For R test
 * pairs (theta*, y*) with y* simulated from theta*, ABC is run against each y* as if it were the observation, on one table of n prior
 * draws that is never stored: a draw is a function of (model, seed, id), so the table is regenerated in registers and all that
 * reaches memory is 2 + theta_dim integers per test.
 *
 * Table draw i < n has the id row0 + i; its (theta_i, y_i) are exactly glabc_abc_draws' theta and y of that id under `seed`: the same
 * Philox keys (seed, seed ^ GLABC_ABC_NOISE_KEY), the same prior draw, the same simulator -- the same bits.
 * Test r < n_tests is row r of the DEVICE arrays theta_star[j * test_stride + r] (j < theta_dim), y_star[j * test_stride + r]
 * (j < y_dim) and width[r]: dimension-major with stride test_stride >= n_tests, the layout glabc_abc_draws writes, so its outputs pass
 * straight in; columns n_tests .. test_stride - 1 are never read.
 *
 * Specification of the pair (r, i), every operator one rounded float32 operation (no FMA: -ffp-contract=off):
 *     d = glabc_model_discrepancy of y_i for a Model whose y_obs is y*_r (the Model's own y_obs is not read)
 *     kernel 0 (hard):   m = d <= width_r ? 1 : 0                       a NaN on either side gives 0
 *     kernel 1 (model):  e = (d - 0.0f) / width_r;  p = glabc_expf(-(0.5f * (e * e)));  m = (uint32)rintf(p * 65536.0f), a NaN p: 0
 *                        glabc_abc_draws' K(d) / K(0) at the test's width used as an importance weight quantised to 2^-16 -- no
 *                        uniform is drawn, so it adds no Monte-Carlo noise and stays exact; m <= 65536
 * m is an integer, and the outputs are integer sums over the table, ADDED to what the arrays hold (the caller zeroes them):
 *     mass[r]                   += sum_i m
 *     mass2[r]                  += sum_i m * m                                                    mass2 may be NULL
 *     below[r * theta_dim + j]  += sum_i m * [theta_ij < theta*_rj]     a float32 <: a tie or a NaN is not below.  below may be NULL:
 *                                                                       a counting-only call that skips the theta comparisons
 * Limits: n <= GLABC_MAX_COVERAGE_DRAWS per call (the worst sum, 2^32 x 2^30, fits 64 bits; the sums of several calls are the
 * caller's to bound), n_tests <= GLABC_MAX_COVERAGE_TESTS.  Integer adds commute: the result depends on (model, seed, row0, n, the
 * test rows, kernel) only, never on the launch geometry, and calls over [row0, row0 + n1) and [row0 + n1, row0 + n) add up to the call
 * over [row0, row0 + n).
 *
 * Models: those of glabc_abc_draws.  Refusals, in its order; a refused call launches nothing and writes nothing:
 *   a NULL model, mass, theta_star, y_star or width                                               GLABC_ERR_NULL
 *   the Model's dimensions, then its kinds, as glabc_abc_draws refuses them                       GLABC_ERR_DIM, GLABC_ERR_KIND
 *   n < 0, row0 < 0, n_tests < 0, test_stride < n_tests, kernel not 0 or 1, n > GLABC_MAX_COVERAGE_DRAWS,
 *   n_tests > GLABC_MAX_COVERAGE_TESTS                                                            GLABC_ERR_ARG
 * n == 0 or n_tests == 0 returns GLABC_OK and writes nothing.  The widths' values are not examined (a width of 0 keeps the pairs at
 * distance 0 under the hard kernel; +inf keeps every pair with a distance).  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no
 * struct changes and no existing draw moves. */
#define GLABC_MAX_COVERAGE_DRAWS (1ll << 30)
#define GLABC_MAX_COVERAGE_TESTS (1ll << 20)
#define GLABC_COVERAGE_TEST_KEY 0xC2B2AE3D27D4EB4Full   /* glabcmcmc_amd/coverage.py: the default test pairs are draws under seed ^ this */
int glabc_coverage_counts(const glabc_model* model, uint64_t seed, int64_t row0, int64_t n, const float* theta_star,
                          const float* y_star, const float* width, int64_t n_tests, int64_t test_stride, int32_t kernel,
                          unsigned long long* mass, unsigned long long* mass2, unsigned long long* below, void* stream);

/* ---- posterior predictive checks: a fresh simulation y_rep ~ p(y | theta) for every draw theta of a history, and integer summaries
 * of y_rep and of its distance to y_obs, one fused kernel family (csrc/glabc_predictive.hip; glabcmcmc_amd/predictive.py forms the
 * predictive p-values and histograms from them).  The history is glabc_autocov's: [n_rows][theta_dim][stride] float32, chain-major,
 * columns n_chains .. stride - 1 never read; its base needs 4-byte alignment only; theta_dim must equal model->theta_dim.
 *
 * Specification of a predictive draw.  Draw (row t, chain c) has the 64-bit id  id = id0 + t * id_step + c  with id0 >= 0 and
 * id_step >= n_chains, so the ids of a call are distinct, and slabs of chains (id0 + chain0) or slices of rows (id0 + row0 * id_step)
 * address the very draws of the whole.  With id_lo / id_hi the two words of the id:
 *     theta = history[t][:][c]
 *     y     = glabc_model_simulate(model, theta, eps = NULL, seed ^ GLABC_PREDICTIVE_KEY, id): the Philox blocks
 *             (seed ^ GLABC_PREDICTIVE_KEY; id_lo, id_hi, 0, b), b < ceil(y_dim / 4), Box-Muller pairs of words (2i, 2i + 1), as in
 *             glabc_abc_draws; the key differs from both of that entry point's, so the predictive noise is no stream a sampler or the
 *             rejection kernel used under the same seed
 *     dis   = glabc_model_discrepancy(model, y)
 * every line one rounded float32 operation per operator (no FMA: -ffp-contract=off).  The result depends on (model, the history's
 * value, seed, id) only -- never on the launch geometry, nor on how rows and chains were cut into calls.  A NaN or an infinity in the
 * history propagates as the lines say.  Models: those of glabc_abc_draws, GLABC_SIM_ABS_GAUSS with theta_dim == y_dim in
 * 1 .. GLABC_MAX_DIM and GLABC_SIM_GK (4, 8); the prior is not used and not examined.
 *
 * glabc_predictive_draws materialises the draws (device arrays, float32):
 *     y_out[(t * y_dim + j) * y_stride + c]   j < y_dim: the history's layout with its own stride      dis_out[t * dis_stride + c]
 * Either may be NULL, not both; what only a NULL output needs is not computed.  Columns n_chains .. of either are never written.
 *
 * glabc_predictive_counts keeps the draws in registers and ADDS to integer tables (device arrays; the caller zeroes or initialises
 * them, so slabs of chains and slices of rows accumulate into one).  There are K = y_dim + 1 statistics: statistic k < y_dim is y_k,
 * statistic y_dim is dis.  Each of the three outputs may be NULL, not all of them.
 *     counts[k * (n_bins + 3) + slot]   uint64.  glabc_histogram's rule on statistic k over [lo[k], hi[k]], the same double arithmetic:
 *                                       scale = (double) n_bins / (hi[k] - lo[k]) on the host;  u = ((double) x - lo[k]) * scale,
 *                                       b = floor(u);  NaN -> slot n_bins + 2;  x < lo -> slot n_bins;  x > hi -> slot n_bins + 1;
 *                                       x == hi -> bin n_bins - 1;  otherwise bin min(b, n_bins - 1).  lo and hi are HOST arrays of K
 *                                       doubles, looked at only when counts is not NULL, as n_bins in 1 .. GLABC_MAX_PREDICTIVE_BINS
 *     tails[k * 4 + s]                  uint64.  x against threshold[k] (HOST array of K float32, looked at only when tails is not
 *                                       NULL), compared in float32:  s = 0 for x < thr, 1 for x == thr, 2 for x > thr, 3 for a NaN x
 *     extremes[k * 2 + {0, 1}]          uint32.  atomicMin / atomicMax of the order-preserving key of glabc_key_counts over the
 *                                       statistic's values that are not NaN; the caller initialises the pair to 0xFFFFFFFF / 0
 *                                       (what it still holds after a call: every value was a NaN)
 * All three are integers: the same bits for every launch geometry and every order of the atomics.
 *
 * Refusals of both, in this order; a refused call launches nothing and writes nothing:
 *   a NULL model or history, all outputs NULL, counts without lo or hi, tails without threshold   GLABC_ERR_NULL
 *   theta_dim or y_dim of the Model outside 1 .. GLABC_MAX_DIM, GLABC_SIM_GK not (4, 8), GLABC_SIM_ABS_GAUSS with y_dim != theta_dim,
 *   theta_dim != model->theta_dim                                                                GLABC_ERR_DIM
 *   GLABC_SIM_USER or an unknown simulator kind                                                  GLABC_ERR_KIND
 *   n_rows < 1, n_chains < 0, stride < n_chains; the stride of an output that is not NULL < n_chains; id0 < 0, id_step < n_chains,
 *   or id0 + (n_rows - 1) * id_step + n_chains - 1 past int64; with counts: n_bins outside 1 .. GLABC_MAX_PREDICTIVE_BINS, a lo or
 *   hi that is not finite or not lo < hi; with tails: a NaN threshold                            GLABC_ERR_ARG
 * n_chains == 0 returns GLABC_OK and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes and no
 * existing draw moves. */
#define GLABC_PREDICTIVE_KEY 0xA0761D6478BD642Full
#define GLABC_MAX_PREDICTIVE_BINS 1024
int glabc_predictive_draws(const glabc_model* model, const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                           int64_t stride, uint64_t seed, int64_t id0, int64_t id_step, float* y_out, int64_t y_stride, float* dis_out,
                           int64_t dis_stride, void* stream);
int glabc_predictive_counts(const glabc_model* model, const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                            int64_t stride, uint64_t seed, int64_t id0, int64_t id_step, int32_t n_bins, const double* lo,
                            const double* hi, const float* threshold, uint64_t* counts, uint64_t* tails, uint32_t* extremes,
                            void* stream);

/* ---- KernelDensity, the adaptive proposal of AGLMCMC (kernel_density.py:4-177) --------
 * A weighted Gaussian KDE over n_samples centres.  All arrays are device pointers; x is dimension-major.
 *
 * glabc_kde_fit (kernel_density.py:70-94, weighted_std :40-68): weights = w_raw / sum(w_raw) (w_raw NULL: 1/n);
 * bandwidth = h * weighted_std(x, weights, unbiased) with h the Silverman / Scott factor the host formed in Python
 * floats (:24-33), or bw_fixed[dim] (host array) when the caller passes an explicit bandwidth (then h is ignored).
 * Sums are float64 in a fixed order (256 strided partials, then a binary tree) instead of torch.sum's float32
 * cascade; everything else is the reference's float32 arithmetic.  Outputs: weights_out[n], log_w_out[n] =
 * log(weights + 1e-10) (:125), wq_out[n] = rint(weights * 2^40) (the integer weights glabc_kde_sample draws
 * from; the caller turns them into inclusive prefix sums -- integer, so any scan gives the same numbers) and
 * consts_out[dim + 2] = bandwidth[0..dim), sum(log(bandwidth)) (:122), 0.5*dim*log(2 pi) (:121). */
int glabc_kde_fit(const float* x, const float* w_raw, int64_t n_samples, int32_t dim, double h, const float* bw_fixed,
                  float* weights_out, float* log_w_out, int64_t* wq_out, float* consts_out, void* stream);

typedef struct glabc_kde {
    int32_t dim;                   /* 1..GLABC_MAX_DIM */
    int32_t reserved;
    int64_t n_samples;
    const float* x;                /* [dim][n_samples] kernel centres */
    const float* log_w;            /* [n_samples] log(weights + 1e-10) */
    const int64_t* cum_q;          /* [n_samples] inclusive prefix sums of wq (glabc_kde_sample only; else may be NULL) */
    float bandwidth[GLABC_MAX_DIM];
    float sum_log_bw;              /* consts_out[dim] */
    float c_2pi;                   /* consts_out[dim + 1] */
} glabc_kde;

/* KernelDensity.log_prob, kernel_density.py:96-128: out[p] = logsumexp_s( ((-0.5 * sum_d ((pt_pd - x_sd)*(1/bw_d))^2
 * - c_2pi) - sum_log_bw) + log_w_s ), the inner float32 operations in the reference's order; the logsumexp is
 * max + log(sum exp(. - max)) with the sum taken exactly in 2^-40 fixed point (order-independent, so the lanes of a
 * wavefront can share one point).  pts is dimension-major [dim][n_points]. */
int glabc_kde_log_prob(const glabc_kde* kde, const float* pts, int64_t n_points, float* out, void* stream);

/* The same for the points listed in idx[0 .. *n_dev - 1] only: point i = (pts[idx[i]], pts[stride + idx[i]], ...), result to
 * out[idx[i]].  *n_dev is read on the device (no host synchronisation); max_points bounds it (the grid).  AGLMCMC keeps the
 * proposal density of every chain's current state (AGLMCMC.py:137-140, a pure function of the state and the fitted KDE) and
 * refreshes it for the chains that moved. */
int glabc_kde_log_prob_indexed(const glabc_kde* kde, const float* pts, int64_t stride, const int32_t* idx, const int32_t* n_dev,
                               int64_t max_points, float* out, void* stream);

/* KernelDensity.sample, kernel_density.py:130-150: row r (global id row0 + r) picks centre j = first index with
 * cum_q[j] > floor(u * cum_q[n-1]), u the float64 uniform of Philox(seed; id, 0, 0) words 0-1 (torch.multinomial
 * with replacement is the same inverse-CDF draw on torch's generator), and adds bandwidth_d * normal_d (normals from
 * words 2-3 of block 0, then blocks 1..).  out is dimension-major [dim][n]. */
int glabc_kde_sample(const glabc_kde* kde, int64_t n, uint64_t seed, int64_t row0, float* out, void* stream);

/* ---- ABC-SMC proposals: ancestor -> perturbation -> prior density -> simulation -> distance -> acceptance, one fused kernel
 * (csrc/glabc_smc.hip).  glabc_abc_draws with theta drawn from a fitted population -- the weighted particles of the previous
 * generation as a glabc_kde -- instead of the prior; the generations, tolerances and weights are glabcmcmc_amd/smc.py's.
 *
 * Ids, layouts and NULL outputs are glabc_abc_draws': draw r < n has the 64-bit id  ids ? ids[r] : row0 + r  (`ids` a DEVICE array, any
 * order, repeats, values >= 2^32); theta_out / y_out are dimension-major with stride `stride` >= n and columns n .. stride - 1 are never
 * written; dis_out[r], log_prior_out[r] (float32) and accept_out[r] (one byte, 0 or 1) are dense.  Each output may be NULL, but not all
 * five; what only a NULL output needs is neither computed nor stored.  More than 2^30 draws go in several launches; every index is
 * 64 bits wide.
 *
 * Specification of a draw.  The result depends on (model, population, seed, id) only, and restates entry points of this header:
 *     theta     = row id of glabc_kde_sample(population, ., seed, .): the Philox blocks (seed; id_lo, id_hi, 0, b), b < ceil((dim + 2) / 4);
 *                 words 0-1 of block 0 give the float64 uniform u, the ancestor is the first j with
 *                 cum_q[j] > (int64)(u * cum_q[n_samples - 1]), the normals come from words 2-3 of block 0 and then from blocks 1
 *                 onwards, theta_d = x[d * n_samples + j] + nrm_d * bandwidth_d (two rounded operations)
 *     log_prior = glabc_model_prior_log_prob(model, theta)
 *     y         = glabc_model_simulate(model, theta, eps = NULL, seed ^ GLABC_ABC_NOISE_KEY, id)
 *     dis       = glabc_model_discrepancy(model, y), replaced by +inf where log_prior == -inf (a select: y_out still holds the simulated
 *                 row).  A proposal outside a Uniform prior's support is then kept by neither acceptance rule
 *     accept    = as in glabc_abc_draws on that dis, under seed ^ GLABC_ABC_ACCEPT_KEY (dis = +inf: p = 0, accept = 0)
 *
 * Models: those of glabc_abc_draws.  Refusals, in this order; a refused call launches nothing and writes nothing:
 *   a NULL model or population, or all five outputs NULL                                          GLABC_ERR_NULL
 *   the Model's dimensions, then its kinds, as glabc_abc_draws refuses them                       GLABC_ERR_DIM, GLABC_ERR_KIND
 *   the population as glabc_kde_sample refuses it: dim outside 1 .. GLABC_MAX_DIM (GLABC_ERR_DIM), n_samples < 1 (GLABC_ERR_ARG),
 *     a NULL x or log_w (GLABC_ERR_NULL), a bandwidth that is not positive and finite (GLABC_ERR_ARG); then
 *     a NULL cum_q                                                                                GLABC_ERR_NULL
 *     population->dim != theta_dim                                                                GLABC_ERR_DIM
 *   n < 0, stride < n, row0 < 0, or row0 != 0 together with ids                                    GLABC_ERR_ARG
 * n == 0 returns GLABC_OK and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes and no existing
 * draw moves. */
int glabc_smc_draws(const glabc_model* model, const glabc_kde* population, uint64_t seed, int64_t row0, const int64_t* ids,
                    int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out, float* log_prior_out,
                    uint8_t* accept_out, void* stream);

/* ---- The same proposals under a full-covariance perturbation kernel (Filippi et al. 2013; Beaumont et al. 2009 in its multivariate
 * form): theta = x_j + L nrm, L the lower Cholesky factor of the kernel's covariance (glabcmcmc_amd/smc.py: a multiple of the weighted
 * population covariance).  `chol` is a HOST array of dim (dim + 1) / 2 float32 packed row-major: chol[d (d + 1) / 2 + e] = L[d][e],
 * e <= d; it travels in the kernel's argument block.
 *
 * Specification of theta for draw `id` -- it departs from glabc_kde_sample's row (above) in its last line only:
 *     the Philox blocks, the float64 uniform u, the ancestor j and the normals nrm[0 .. dim) are glabc_kde_sample's: no new random
 *     number is used and no existing draw moves;
 *     acc = nrm_0 * L[d][0], then acc = acc + nrm_e * L[d][e] for e = 1 .. d ascending, every product and every sum a rounded float32
 *     operation (no fused multiply-add: -ffp-contract=off is part of the specification, as elsewhere);
 *     theta_d = x[d * n_samples + j] + acc
 * so IEEE float32 arithmetic restates it bit for bit, and a diagonal L gives glabc_kde_sample's / glabc_smc_draws' draws with
 * bandwidth = diag(L) bit for bit (0 * nrm_e = +-0 and +-0 + v = v), but for a coordinate x = -0 of the ancestor whose acc is +0.
 * The population's bandwidth, sum_log_bw and c_2pi are not read for drawing (they still pass the population's checks: the Python
 * layer fills bandwidth with the marginal scales sqrt(diag(L L^T))).
 *
 * glabc_kde_sample_full is glabc_kde_sample with that row: out dimension-major [dim][n].  Refusals, in this order: those of
 * glabc_kde_sample on kde; a NULL chol GLABC_ERR_NULL; an entry of chol that is not finite or a diagonal entry <= 0 GLABC_ERR_ARG;
 * then n < 0 or row0 < 0 GLABC_ERR_ARG; n == 0 returns GLABC_OK; a NULL out or cum_q GLABC_ERR_NULL.
 *
 * glabc_smc_draws_full is glabc_smc_draws with theta = row id of glabc_kde_sample_full(population, chol, ., seed, .); log_prior, y,
 * dis and accept, the ids, layouts and NULL outputs are glabc_smc_draws'.  Its refusals are glabc_smc_draws', in that order, with the
 * two of chol (NULL: GLABC_ERR_NULL; not finite, or a diagonal entry <= 0: GLABC_ERR_ARG) after population->dim != theta_dim and before
 * the range of draws.  A refused call launches nothing and writes nothing.  glabc_rtc_smc_draws_full is glabc_rtc_smc_draws in the
 * same way: the same kernel (csrc/glabc_smc.h smc_draws_kernel<D, YD, true>) in the draws program of glabc_rtc_compile_draws, chol refused at
 * the same place.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes and no existing draw moves. */
int glabc_kde_sample_full(const glabc_kde* kde, const float* chol, int64_t n, uint64_t seed, int64_t row0, float* out, void* stream);
int glabc_smc_draws_full(const glabc_model* model, const glabc_kde* population, const float* chol, uint64_t seed, int64_t row0,
                         const int64_t* ids, int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out,
                         float* log_prior_out, uint8_t* accept_out, void* stream);

/* ---- The two draw kernels around a USER simulator (csrc/glabc_rtc.hip): glabc_abc_draws and glabc_smc_draws for GLABC_SIM_USER Models.
 * glabc_rtc_compile_draws compiles (hiprtc, gfx950) the templates those two entry points are instantiated from -- abc_draws_kernel
 * (csrc/glabc_abc.h) and smc_draws_kernel (csrc/glabc_smc.h) -- around `simulator_source` (the source of glabc_rtc_compile, with its
 * optional GLABC_USER_DISCREPANCY / GLABC_USER_KERNEL), plus the two row kernels every program holds: glabc_rtc_simulate,
 * glabc_rtc_hooks, glabc_rtc_model_rows and glabc_rtc_release take a draws program as any other.  It holds no sampler kernel:
 * glabc_rtc_steps and glabc_rtc_mix_steps refuse it with GLABC_ERR_KIND (a third kind of program beside the sampler and the mixture
 * programs).  Compile options, the log and GLABC_ERR_ARG / GLABC_ERR_NO_DEVICE are glabc_rtc_compile's; a kernel that spills
 * registers is named in the log and handed out.  Refusals of glabc_rtc_compile_draws, in this order:
 *   a NULL source or out                                                                          GLABC_ERR_NULL
 *   theta_dim, y_dim or noise_dim outside 1 .. GLABC_MAX_DIM                                      GLABC_ERR_DIM
 *   a source that announces GLABC_USER_PRIOR (a line in the log says so): theta is drawn from the descriptor's prior, and
 *     generation 0 of ABC-SMC takes that for the prior                                            GLABC_ERR_KIND
 *
 * Ids, layouts, NULL outputs, the 2^30-draw launches and the 64-bit indices of glabc_rtc_abc_draws / glabc_rtc_smc_draws are
 * glabc_abc_draws' / glabc_smc_draws'.  Specification of draw `id`, a composition of entry points of this header (nd = noise_dim):
 *     theta     = row id of glabc_dist_forward(&model->prior, ., seed, .)                 (glabc_rtc_abc_draws)
 *                 row id of glabc_kde_sample(population, ., seed, .)                      (glabc_rtc_smc_draws)
 *     eps       = row id of glabc_dist_forward(a DiagGaussian of dimension nd, location 0 and scale 1, ., seed ^ GLABC_ABC_NOISE_KEY, .):
 *                 the Philox blocks (key; id_lo, id_hi, 0, b), b < ceil(nd / 4), Box-Muller pairs of words (2i, 2i + 1) -- the blocks
 *                 and pairs of the built-in kernels' noise; 0 + 1 * e is e
 *     y         = glabc_rtc_simulate(program, theta, eps)
 *     dis       = glabc_rtc_model_rows(program, model, GLABC_RTC_DISCREPANCY, y) where the source announces GLABC_USER_DISCREPANCY,
 *                 else glabc_model_discrepancy(model, y); glabc_rtc_smc_draws: +inf where log_prior == -inf, as in glabc_smc_draws
 *     log_prior = glabc_model_prior_log_prob(model, theta)                                 (glabc_rtc_smc_draws)
 *     u         = glabc_uniform_f32(word 0 of Philox(seed ^ GLABC_ABC_ACCEPT_KEY; id_lo, id_hi, 0, 0))
 *     p         = without GLABC_USER_KERNEL: e = (dis - 0.0f) / kern_scale, p = glabc_expf(-(0.5f * (e * e))), as in glabc_abc_draws;
 *                 with it: p = glabc_expf(lk(dis) - lk(0.0f)), lk(d) = glabc_user_log_kernel(d, kern_scale) -- the ratio
 *                 K(dis) / K(0) from its two logarithms
 *     accept    = u < p ? 1 : 0                    (a NaN p: 0)
 * Refusals of the two, in this order; a refused call launches nothing and writes nothing:
 *   a NULL program or model, or every output NULL                                                 GLABC_ERR_NULL
 *   model->sim_kind != GLABC_SIM_USER                                                             GLABC_ERR_KIND
 *   a program that glabc_rtc_compile_draws did not make                                           GLABC_ERR_KIND
 *   model->theta_dim, y_dim or noise.dim differ from the program's                                GLABC_ERR_DIM
 *   a prior that is not DiagGaussian / Uniform, or whose dim != theta_dim                         GLABC_ERR_KIND
 *   glabc_rtc_smc_draws: the population as glabc_smc_draws refuses it (a NULL population: GLABC_ERR_NULL; dim, n_samples, x / log_w,
 *     bandwidth; a NULL cum_q: GLABC_ERR_NULL; population->dim != theta_dim: GLABC_ERR_DIM)
 *   n < 0, stride < n, row0 < 0, or row0 != 0 together with ids                                    GLABC_ERR_ARG
 * n == 0 returns GLABC_OK and writes nothing.  glabc_abc_draws and glabc_smc_draws keep refusing GLABC_SIM_USER.  GLABC_VERSION and
 * GLABC_STREAM_LAYOUT are unchanged. */
int glabc_rtc_compile_draws(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                            glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_abc_draws(const glabc_rtc_program* program, const glabc_model* model, uint64_t seed, int64_t row0, const int64_t* ids,
                        int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out, uint8_t* accept_out, void* stream);
int glabc_rtc_smc_draws(const glabc_rtc_program* program, const glabc_model* model, const glabc_kde* population, uint64_t seed,
                        int64_t row0, const int64_t* ids, int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out,
                        float* log_prior_out, uint8_t* accept_out, void* stream);
/* glabc_rtc_smc_draws under a full-covariance perturbation kernel: see glabc_smc_draws_full */
int glabc_rtc_smc_draws_full(const glabc_rtc_program* program, const glabc_model* model, const glabc_kde* population, const float* chol,
                             uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride, float* theta_out, float* y_out,
                             float* dis_out, float* log_prior_out, uint8_t* accept_out, void* stream);

/* ---- The posterior predictive kernel around a USER simulator (csrc/glabc_rtc.hip): glabc_predictive_draws and glabc_predictive_counts
 * for GLABC_SIM_USER Models.  glabc_rtc_compile_predictive compiles (hiprtc, gfx950) the template those two entry points are
 * instantiated from -- predictive_kernel (csrc/glabc_predictive.h) -- around `simulator_source` (the source of glabc_rtc_compile, with
 * its optional GLABC_USER_DISCREPANCY), plus the two row kernels every program holds: glabc_rtc_simulate, glabc_rtc_hooks,
 * glabc_rtc_model_rows and glabc_rtc_release take a predictive program as any other.  It is a fourth kind of program beside the
 * sampler, the mixture and the draws programs: glabc_rtc_steps, glabc_rtc_mix_steps, glabc_rtc_abc_draws and glabc_rtc_smc_draws
 * refuse it with GLABC_ERR_KIND, and the two launch entry points below refuse those three kinds the same way.  The kernel walks
 * the history one row per item whatever the source (csrc/glabc_rtc_predictive_kernels.h); a draw does not depend on that.  Compile
 * options, the log and GLABC_ERR_ARG / GLABC_ERR_NO_DEVICE are glabc_rtc_compile's; a kernel that spills registers or keeps a private
 * segment is named in the log and handed out.  Refusals of glabc_rtc_compile_predictive, in this order:
 *   a NULL source or out                                                                          GLABC_ERR_NULL
 *   theta_dim, y_dim or noise_dim outside 1 .. GLABC_MAX_DIM                                      GLABC_ERR_DIM
 *   a source that does not compile (see the log)                                                  GLABC_ERR_ARG
 * A source that announces GLABC_USER_PRIOR is accepted: theta comes from the history, the prior is never evaluated -- and for the
 * same reason a Gamma or a user prior in the descriptor is no ground for refusal at launch.
 *
 * Ids, layouts, NULL outputs, the tables, thresholds, extremes, bins and the LDS table of at most 36 972 bytes of
 * glabc_rtc_predictive_draws / glabc_rtc_predictive_counts are glabc_predictive_draws' / glabc_predictive_counts'.  Specification of
 * draw (row t, chain c), id = id0 + t * id_step + c, a composition of entry points of this header (nd = noise_dim):
 *     theta = history[t][.][c]
 *     eps   = row id of glabc_dist_forward(a DiagGaussian of dimension nd, location 0 and scale 1, ., seed ^ GLABC_PREDICTIVE_KEY, .):
 *             per history row t one call with row0 = id0 + t * id_step, n = n_chains
 *     y     = glabc_rtc_simulate(program, theta, eps)
 *     dis   = glabc_rtc_model_rows(program, model, GLABC_RTC_DISCREPANCY, y) where the source announces GLABC_USER_DISCREPANCY,
 *             else glabc_model_discrepancy(model, y)
 * Refusals of the two, in this order; a refused call launches nothing and writes nothing:
 *   a NULL program or model                                                                       GLABC_ERR_NULL
 *   model->sim_kind != GLABC_SIM_USER                                                             GLABC_ERR_KIND
 *   a program that glabc_rtc_compile_predictive did not make                                      GLABC_ERR_KIND
 *   model->theta_dim, y_dim or noise.dim differ from the program's                                GLABC_ERR_DIM
 *   everything glabc_predictive_draws / glabc_predictive_counts refuse, in their order (of the Model, what is left is
 *     theta_dim != model->theta_dim: GLABC_ERR_DIM)
 * n_chains == 0 returns GLABC_OK and writes nothing.  glabc_predictive_draws and glabc_predictive_counts keep refusing
 * GLABC_SIM_USER.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes. */
int glabc_rtc_compile_predictive(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                                 glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_predictive_draws(const glabc_rtc_program* program, const glabc_model* model, const float* history, int64_t n_rows,
                               int32_t theta_dim, int64_t n_chains, int64_t stride, uint64_t seed, int64_t id0, int64_t id_step,
                               float* y_out, int64_t y_stride, float* dis_out, int64_t dis_stride, void* stream);
int glabc_rtc_predictive_counts(const glabc_rtc_program* program, const glabc_model* model, const float* history, int64_t n_rows,
                                int32_t theta_dim, int64_t n_chains, int64_t stride, uint64_t seed, int64_t id0, int64_t id_step,
                                int32_t n_bins, const double* lo, const double* hi, const float* threshold, uint64_t* counts,
                                uint64_t* tails, uint32_t* extremes, void* stream);

/* ---- ABC regression adjustment (Beaumont, Zhang and Balding 2002; csrc/glabc_regress.hip, glabcmcmc_amd/regression.py): the weighted
 * second moments of n kept draws, from which the host fits theta = alpha + B^T (y - y_obs) + e, and the row-wise correction
 * theta - B^T (y - y_obs).  The rows are what glabc_abc_draws writes, float32 and dimension-major, read in place:
 *     theta[j * stride_t + r]   j < theta_dim          y[k * stride_y + r]   k < y_dim          dis[r]          weight[r]
 * Columns n .. stride - 1 are never read.  theta_dim and y_dim are each 1 .. GLABC_MAX_DIM and independent of one another.  dis and
 * weight are device arrays, each of which may be NULL; y_obs (and beta below) are HOST arrays.  The entry points allocate nothing.
 *
 * glabc_weighted_gram.  With P = 1 + y_dim + theta_dim, row r has the design vector
 *     z_r = (1.0, (double) y_r,0 - y_obs_0, .., (double) y_r,y_dim-1 - y_obs_y_dim-1, (double) theta_r,0, .., (double) theta_r,theta_dim-1)
 * and gram[Q], Q = P (P + 1) / 2 + 1 doubles on the device, holds the packed upper triangle of sum_r w_r z_r z_r^T,
 *     gram[q],   q = a * P - a (a - 1) / 2 + (b - a),   a <= b < P           (the packing of glabc_cross_moments)
 * and, last, gram[Q - 1] = sum_r w_r^2 (for Kish's effective sample size).  workspace: ceil(n / GLABC_GRAM_SEGMENT) * Q doubles on
 * the device, the caller's (it may be NULL when n == 0); its contents afterwards are the segments' partial sums.
 *
 * Numerical specification.  All arithmetic is IEEE double, every line one rounded operation in the stated order, no FMA.
 *     d = (double) dis_r;    u = d / delta
 *     GLABC_GRAM_EPANECHNIKOV:  k = d <= delta ? 1.0 - u * u : 0.0          GLABC_GRAM_UNIFORM:  k = d <= delta ? 1.0 : 0.0
 *     dis == NULL:  k = 1.0                                                 w_r = weight ? k * (double) weight_r : k
 * A NaN distance fails the comparison: k = 0.  delta = +inf is legal and keeps every finite distance with k = 1 (u = 0).
 *     term_r of statistic (a, b):  (w_r * z_r,a) * z_r,b                    term_r of the last statistic:  w_r * w_r
 * A row with w_r == 0.0 contributes NOTHING: it is skipped, not multiplied, so a NaN theta or y in a row outside the tolerance
 * poisons nothing.  A NaN w_r is not 0: it propagates into every statistic, and a NaN or an infinity in z of a weighted row into the
 * statistics that involve the coordinate, as the lines say.  The order of the sums does not depend on the launch geometry:
 *     segment s covers rows 1024 s .. 1024 s + 1023 (GLABC_GRAM_SEGMENT); column l < 64 of a segment is
 *         c_l = 0.0;  for t = 0 .. 15:  r = 1024 s + 64 t + l;  if r < n and w_r != 0.0:  c_l = c_l + term_r
 *     then for h = 1, 2, 4, 8, 16, 32, all columns at once:  c_l = c_l + c_(l xor h)      (every column ends with the same bits)
 *     partial_s = c_0;        G = 0.0;  for s ascending:  G = G + partial_s
 * so a NumPy loop reproduces gram bit for bit (tests/regress_ref.py).  Two launches on the caller's stream: the segments, then one
 * workgroup that adds the partial sums.  n == 0 returns GLABC_OK and writes Q zeros.
 * Refusals, in this order; a refused call launches nothing and writes nothing:
 *   a NULL theta, y, y_obs or gram; a NULL workspace with n > 0                                   GLABC_ERR_NULL
 *   theta_dim or y_dim outside 1 .. GLABC_MAX_DIM                                                 GLABC_ERR_DIM
 *   a kind that is neither GLABC_GRAM_EPANECHNIKOV nor GLABC_GRAM_UNIFORM                         GLABC_ERR_KIND
 *   n < 0, stride_t < n, stride_y < n, a delta that is NaN or <= 0                                GLABC_ERR_ARG
 *
 * glabc_regression_apply.  For every row r < n and every j < theta_dim, with beta[k * theta_dim + j] the HOST array B of the fit:
 *     a = (double) theta_r,j;   for k = 0 .. y_dim - 1 ascending:  a = a - beta[k * theta_dim + j] * ((double) y_r,k - y_obs_k)
 *     out[j * stride_o + r] = (float) a
 * (each subtraction and each product rounded once, no FMA).  Every row is corrected, whatever its weight.  `out` may be `theta`
 * itself with stride_o == stride_t (in place) and nothing else that overlaps an input; columns n .. stride_o - 1 are not written.
 * Refusals, in this order: a NULL pointer GLABC_ERR_NULL; theta_dim or y_dim outside 1 .. GLABC_MAX_DIM GLABC_ERR_DIM; n < 0 or a
 * stride < n GLABC_ERR_ARG.  n == 0 returns GLABC_OK and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged by
 * both: no struct changes. */
#define GLABC_GRAM_EPANECHNIKOV 0
#define GLABC_GRAM_UNIFORM 1
#define GLABC_GRAM_SEGMENT 1024
int glabc_weighted_gram(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y, int64_t stride_y, int32_t y_dim,
                        const float* dis, const float* weight, int64_t n, const double* y_obs, double delta, int32_t kind, double* gram,
                        double* workspace, void* stream);
int glabc_regression_apply(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y, int64_t stride_y, int32_t y_dim,
                           int64_t n, const double* y_obs, const double* beta, float* out, int64_t stride_o, void* stream);

/* ---- summaries of weighted draws (csrc/glabc_weighted.hip, glabcmcmc_amd/weighted.py): the digit counts of a radix selection,
 * marginal histograms and pair histograms of n draws with one float32 weight each -- an ABC-SMC population, regression-adjusted
 * draws.  The draws are dimension-major float32 as glabc_weighted_gram reads them, x[j * stride + i], j < dim, i < n, stride >= n;
 * columns n .. stride - 1 are never read and the base needs 4-byte alignment only.  w[i] is a device array of n float32 weights,
 * `scale` a positive finite double of the host's.
 *
 * The quantised weight.  A draw counts with the integer multiplicity m of its weight w; IEEE double, no FMA:
 *     v = (double) w * scale                                       one rounded product
 *     m = 0                   if !(w > 0)                           zero, negative and NaN weights count nothing
 *     m = 2^32 - 1            if v >= 4294967295.0
 *     m = (uint64) rint(v)    otherwise                             ties to even
 * A draw with m == 0 is skipped whatever its coordinates hold, a NaN included (glabc_weighted_gram skips a row of weight 0 in the
 * same way).  A weighted quantile is then an ordinary order statistic of the multiset in which draw i occurs m_i times.  The counts
 * are sums of integers: the same bits whatever the launch geometry and the order of the atomic adds, additive over slices of draws,
 * and -- n <= GLABC_MAX_WEIGHTED_DRAWS = 2^31 draws of at most 2^32 - 1 each -- below 2^63, so no uint64 wraps.
 *
 * Each entry point is exactly glabc_key_counts / glabc_histogram / glabc_histogram2d on the history [1][dim][stride] with
 * n_chains = n, but that a draw ADDS m where the twin adds 1: the same key, levels, prefix rules, bin arithmetic and slot layouts
 * (counts[(j * n_prefixes + s) << digit_bits | digit]; counts[j * (n_bins + 3) + slot]; counts[p * (n_bins^2 + 2) + slot]), the same
 * host arrays (prefixes, lo, hi, pairs) and device arrays (x, w, counts), the same limits, and "the call ADDS, the caller zeroes".
 * With every weight 1.0 and scale 1.0 they return the twins' counts.
 *
 * Refusals: the twin's, in the twin's order (w is one of its pointers: NULL is GLABC_ERR_NULL), with GLABC_ERR_ARG also for n < 0
 * or n > GLABC_MAX_WEIGHTED_DRAWS, stride < n, and a scale that is not finite or not > 0.  A refused call launches nothing and
 * writes nothing.  n == 0 returns GLABC_OK and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct
 * changes. */
#define GLABC_MAX_WEIGHTED_DRAWS 2147483648ll
int glabc_weighted_key_counts(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t level,
                              int32_t n_prefixes, const uint32_t* prefixes, uint64_t* counts, void* stream);
int glabc_weighted_histogram(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t n_bins,
                             const double* lo, const double* hi, uint64_t* counts, void* stream);
int glabc_weighted_histogram2d(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t n_pairs,
                               const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, uint64_t* counts, void* stream);

/* ---- posterior predictive checks of weighted draws (csrc/glabc_weighted_predictive.hip, glabcmcmc_amd/predictive.py check_weighted):
 * glabc_predictive_counts for n draws with one float32 weight each -- an ABC-SMC population, regression-adjusted draws -- one fused
 * kernel.  x is dimension-major as the weighted entry points above read it, x[j * stride + i], j < theta_dim, i < n, stride >= n;
 * columns n .. stride - 1 are never read, nor is anything behind w[n - 1]; both bases need 4-byte alignment only.  w[i] is a device
 * array of n float32 weights, `scale` a positive finite double of the host's.
 *
 * Specification.  Draw i has the id id0 + i and is exactly the draw (row 0, chain i) that glabc_predictive_draws makes on the history
 * [1][theta_dim][stride] with n_chains = n and the same model, seed and id0: the same key (seed ^ GLABC_PREDICTIVE_KEY), the same
 * noise, the same simulator, the same distance -- the same bits as the unweighted twin's draw, whatever the launch geometry and
 * however the draws were cut into calls (a slice that starts at draw a passes id0 + a).  Draw i counts with the quantised weight
 * m_i = weight_multiplicity(w_i, scale) of the weighted entry points above.  A draw with m_i == 0 is skipped whatever theta holds: it
 * adds nothing to any count, to any tail (the NaN tail included) or to the extremes.
 *
 * The three tables are laid out as glabc_predictive_counts lays them out, with K = y_dim + 1 statistics (y, then the distance):
 *     counts[k * (n_bins + 3) + slot]   uint64.  The same slot rule; a draw adds m_i where the twin adds 1
 *     tails[k * 4 + s]                  uint64.  The same four classes against threshold[k]; a draw adds m_i where the twin adds 1
 *     extremes[k * 2 + {0, 1}]          uint32.  atomicMin / atomicMax of the key over the draws with m_i > 0 whose statistic is no NaN
 * The call ADDS: the caller zeroes counts and tails and pre-sets the extremes to 0xFFFFFFFF / 0.  Each of the three may be NULL, not
 * all of them.  lo, hi and threshold are HOST arrays as in the twin.  With every weight 1.0 and scale 1.0 the three tables equal
 * glabc_predictive_counts' on that one-row history.  n <= GLABC_MAX_WEIGHTED_DRAWS draws of at most 2^32 - 1 each stay below 2^63:
 * no uint64 wraps, by the argument of the weighted summaries above.
 *
 * GLABC_MAX_WEIGHTED_PREDICTIVE_BINS is 512 where the twin has 1024.  The counters in LDS are 64-bit (two draws of multiplicity 2^31
 * wrap a uint32), and the tails take four more per statistic: 1024 bins at K = 9 would need 9 x 1031 x 8 = 74 232 bytes, past the 48 KiB
 * a launch gets without a grant (csrc/glabc_lds_grant.h).  512 bins keep the largest table at 9 x (512 + 3 + 4) x 8 = 37 368 bytes,
 * which holds for the built-in launch and for the hipModuleLaunchKernel of a run-time compiled program alike; nothing here shows that
 * a grant takes effect on a module function, so the limit is one that needs none.
 *
 * Refusals, in the twins' order; a refused call launches nothing and writes nothing:
 *   a NULL model, x or w, all outputs NULL, counts without lo or hi, tails without threshold      GLABC_ERR_NULL
 *   the Model and dimension refusals of glabc_predictive_counts                                   GLABC_ERR_DIM, GLABC_ERR_KIND
 *   n < 0, n > GLABC_MAX_WEIGHTED_DRAWS, stride < n, a scale that is not finite or not > 0; id0 < 0 or id0 + n - 1 past int64; with
 *   counts: n_bins outside 1 .. GLABC_MAX_WEIGHTED_PREDICTIVE_BINS, a lo or hi that is not finite or not lo < hi; with tails: a NaN
 *   threshold                                                                                     GLABC_ERR_ARG
 * n == 0 returns GLABC_OK and writes nothing.  GLABC_VERSION and GLABC_STREAM_LAYOUT are unchanged: no struct changes.
 *
 * The run-time compiled twin.  glabc_rtc_compile_weighted_predictive compiles the same kernel template around a USER simulator: a
 * program kind of its own (it holds the weighted kernel and the two row kernels every program holds, and no other entry point
 * launches it), compiled, logged and released as glabc_rtc_compile_predictive's.  glabc_rtc_weighted_predictive_counts is
 * glabc_weighted_predictive_counts on such a program: draw i is the draw of glabc_rtc_predictive_draws of the predictive program of
 * the same source, the distance the user's where the source announces GLABC_USER_DISCREPANCY.  Its refusals are a NULL program
 * (GLABC_ERR_NULL), glabc_rtc_predictive_counts' of a program of another kind or shape, then the list above. */
#define GLABC_MAX_WEIGHTED_PREDICTIVE_BINS 512
int glabc_weighted_predictive_counts(const glabc_model* model, const float* x, int64_t stride, int32_t theta_dim, const float* w,
                                     int64_t n, double scale, uint64_t seed, int64_t id0, int32_t n_bins, const double* lo,
                                     const double* hi, const float* threshold, uint64_t* counts, uint64_t* tails, uint32_t* extremes,
                                     void* stream);
int glabc_rtc_compile_weighted_predictive(const char* simulator_source, int32_t theta_dim, int32_t y_dim, int32_t noise_dim,
                                          glabc_rtc_program** out, char* log, int64_t log_size);
int glabc_rtc_weighted_predictive_counts(const glabc_rtc_program* program, const glabc_model* model, const float* x, int64_t stride,
                                         int32_t theta_dim, const float* w, int64_t n, double scale, uint64_t seed, int64_t id0,
                                         int32_t n_bins, const double* lo, const double* hi, const float* threshold, uint64_t* counts,
                                         uint64_t* tails, uint32_t* extremes, void* stream);

/* AGLMCMC.py:199-204 (and :104-109): weights of a proposal pool from its stored discrepancies,
 * w[r] = exp((prior(theta_r) + calculate_log_kernel_dis(dis_r)) - log_q[r]), NaN -> 0.  The threshold is the one in
 * model->kern_* (the caller passes a copy of its descriptor with the annealed eps_hat, Mixture.py:47-53).
 * theta is dimension-major [theta_dim][n]. */
int glabc_kde_train_weights(const glabc_model* model, const float* theta, const float* dis, const float* log_q, int64_t n,
                            float* w_out, void* stream);

/* Test hooks (not part of the sampling API): evaluate include/glabc_numerics.h on the device.
 * op 0 expf, 1 logf, 2 sin(2 pi u), 3 cos(2 pi u) on float bit patterns in[n] -> out[n];
 * op 4 / 5: the two normals of glabc_normal_pair(in[2i], in[2i+1]);
 * op 6: glabc_philox4x32_10(in[6i .. 6i+3], key in[6i+4], in[6i+5]) -> out[4i .. 4i+3] (n counters);
 * op 7 / 8: the fast index pass's approximate iSIR weight / the specified one (exp, NaN -> 0) of the
 * float bit patterns in[n].  glabc_selftest_sqrt counts the
 * floats with bit pattern in [first_bits, last_bits] whose glabc_sqrtf_normal differs from the
 * exactly rounded square root (*mismatches is a device counter the caller zeroed). */
int glabc_selftest_numerics(int op, const uint32_t* in, uint32_t* out, int64_t n, void* stream);
int glabc_selftest_sqrt(uint32_t first_bits, uint32_t last_bits, uint64_t* mismatches, void* stream);
/* torch.sum's float32 association for rows of any length as glabc_select evaluates it: x[n_rows][n] -> out[n_rows] */
int glabc_selftest_rowsum(const float* x, int32_t n_rows, int32_t n, float* out, void* stream);

int glabc_version(void);
int glabc_stream_layout(void);
const char* glabc_status_string(int status);
int glabc_last_hip_error(void);    /* hipError_t of the most recent failed launch on this thread */

#ifdef __cplusplus
}
#endif
#endif /* GLABC_H */
