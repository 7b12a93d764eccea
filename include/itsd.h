/*
 * itsd.h — C ABI of libitsd_hip.so, the MI355X (gfx950) search-over-noise sampler.
 *
 * The reference exposes this path as Python duck-typed objects;
 * each entry point below replaces one of them:
 *
 *   itsd_unet_create / _destroy  <- UNet(T, ch, ch_mult, attn, num_res_blocks, dropout)
 *                                   + load_state_dict   (Diffusion/Model.py:213,
 *                                   DiffusionFreeGuidence/ModelCondition.py:165,
 *                                   Diffusion/Train.py:814-818)
 *   itsd_unet_forward            <- UNet.forward(x, t[, labels])   (Model.py:265,
 *                                   ModelCondition.py:206)
 *   itsd_unet_representation     <- UNet.forward(..., return_representation=True)'s second
 *                                   output, the pre-tail h (ModelCondition.py:206,225-235)
 *   itsd_set_schedule            <- GaussianDiffusionSampler.__init__ tables
 *                                   (Diffusion/Diffusion.py:51-65, DiffusionCondition.py:57-73)
 *   itsd_sampler_run             <- GaussianDiffusionSampler.forward loop
 *                                   (Diffusion.py:84-102, DiffusionCondition.py:89-105)
 *   itsd_set_schedule_x0         <- (no reference counterpart: it has no few-step sampler) a schedule of K rows, row k
 *                                   run at timestep tau[k], stepped by DDIM(eta) written through the x_0 estimate
 *                                   (optionally clipped, Ho et al.'s clip_denoised). Opt-in: itsd_set_schedule's
 *                                   ancestral form stays the default and the parity contract
 *   itsd_set_schedule_x0_2m      <- (no reference counterpart) the same K rows stepped second order: DPM-Solver++(2M)
 *                                   in data prediction, with the previous row's x_0 estimate kept by the library
 *   itsd_set_guidance            <- the guided eps of DiffusionCondition.py:79-87 with w a function of (row, candidate
 *                                   image): guidance schedules (intervals, ramps) and a per-candidate scale a search
 *                                   can sweep, under one captured step graph; rows with w = 0 skip the uncond half
 *   itsd_sampler_predict_x0      <- (no reference counterpart) the x_0 estimate of a half-denoised state, what a
 *                                   verifier can score mid-trajectory: the branching PathSearch its docstring
 *                                   describes (search/search_algorithm.py:238-250; its code, :307-312, is a placeholder)
 *   itsd_sampler_set_trace       <- (no reference counterpart) a score trace: every step of an x0-form run leaves each
 *                                   image's x_0 moments (sum, sum of squares, min, max), what the image-statistics
 *                                   verifiers need, at no extra UNet evaluation
 *   itsd_branch                  <- (no reference counterpart) gather the surviving paths and re-noise them
 *   itsd_es_candidates / _es_step / _es_workspace_bytes
 *                                <- GradientBasedSearch (search/search_algorithm.py:343-438) without autograd: the
 *                                   antithetic candidates pivot +- sigma z of an evolution-strategies estimate of the
 *                                   score's gradient, and the reference's Adam step on that estimate, summed in slices
 *                                   of kEsSlice = 16 pairs
 *   itsd_verify                  <- OracleVerifier / SelfSupervisedVerifier /
 *                                   AestheticPredictor .score (search/verifier.py:45-66,
 *                                   223-248, 262-287), batched per candidate
 *   itsd_verify_paired           <- SelfSupervisedVerifier.score(images, reference_features)
 *                                   (search/verifier.py:235-240)
 *   itsd_verify_denoise          <- (no reference counterpart) the diffusion model as its own verifier: the squared
 *                                   denoising error of a candidate image, under its label and under the null label.
 *                                   Every verifier of the reference that sees content (SupervisedVerifier, CLIPScore,
 *                                   IntegratedVerifier, search/verifier.py:69-188, 290-388) needs downloaded CLIP /
 *                                   DINO weights; this one needs only the checkpoint already on the device
 *   itsd_attention               <- AttnBlock core softmax(q k^T C^-0.5) v
 *                                   (Diffusion/Model.py:152-161, ModelCondition.py:105-115)
 *   itsd_profile_forward / _ops / _op, itsd_unet_query, itsd_set_option
 *                                <- (no reference counterpart) per-kernel census used by
 *                                   bench.py for the roofline line, introspection, A/B switches
 *   itsd_unet_op_info / _act_info / _read / _poison
 *                                <- (no reference counterpart) introspection: a read-only probe of the op program
 *                                   for the per-op parity tests (what each launch is, what it read and wrote)
 *
 * Conventions
 *  - Every tensor argument is a DEVICE pointer owned by the caller; the library
 *    borrows it for the stream-ordered duration of the call. Weights passed to
 *    itsd_unet_create are HOST fp32 pointers (a state_dict on CPU); they are
 *    repacked and copied, and may be freed after the call returns.
 *  - Layouts at the boundary are the reference's: images NCHW fp32, timesteps and
 *    labels int32 per sample. Internally activations are NHWC (bf16 or fp32).
 *  - Every function returns ITSD_OK (0) or an error code; no exception or abort
 *    crosses the ABI. itsd_last_error() returns a thread-local message.
 *  - Calls are asynchronous on the given stream (a hipStream_t passed as void*;
 *    NULL = the default stream) unless documented otherwise. One handle per
 *    device/process; a handle is not thread-safe.
 */
#ifndef ITSD_H
#define ITSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITSD_OK 0
#define ITSD_ERR_INVALID 1   /* bad argument / shape / unsupported configuration */
#define ITSD_ERR_HIP 2       /* a HIP runtime call failed */
#define ITSD_ERR_WEIGHTS 3   /* state_dict key or shape mismatch (load_state_dict strict) */
#define ITSD_ERR_NAN 4       /* the sampler produced a NaN (Diffusion.py:100 assert) */
#define ITSD_ERR_OOM 5
#define ITSD_ERR_HANDOFF 6   /* an in-kernel cross-block hand-off wait exhausted its poll bound (the grid was not
                                co-resident); its outputs are NaN. Reported by itsd_sampler_run with ITSD_RUN_SYNC
                                and by itsd_unet_query(u, "status", ...) after itsd_unet_forward */

enum { ITSD_ARCH_DDPM = 0, ITSD_ARCH_CFG = 1 };
enum { ITSD_PREC_FP32 = 0, ITSD_PREC_BF16 = 1 };
enum { ITSD_VERIFY_ORACLE = 0, ITSD_VERIFY_SELFSUP = 1, ITSD_VERIFY_AESTHETIC = 2, ITSD_VERIFY_MEAN = 3 };

/* itsd_sampler_run flags */
#define ITSD_RUN_GRAPH 1u   /* capture one denoising step in a hipGraph and replay it */
#define ITSD_RUN_CLIP 2u    /* clip(x, -1, 1) after the last step (Diffusion.py:102) */
#define ITSD_RUN_SYNC 4u    /* synchronise at the end and report ITSD_ERR_NAN */
#define ITSD_RUN_CONTINUE 8u /* 2M schedule only: the step at t_begin reads the x_0 the previous run left (below) */

typedef struct itsd_unet itsd_unet;

/* Constructor arguments of the reference UNets plus sizing. */
typedef struct {
  int32_t arch;            /* ITSD_ARCH_DDPM (Model.py) or ITSD_ARCH_CFG (ModelCondition.py) */
  int32_t T;               /* model T (CFG: rows of the time-embedding table) */
  int32_t ch;              /* 'channel' */
  int32_t n_mult;
  int32_t ch_mult[8];      /* 'channel_mult' */
  int32_t n_attn;
  int32_t attn[8];         /* 'attn' level indices (DDPM only) */
  int32_t num_res_blocks;
  int32_t img_size;        /* H = W: divisible by 2^(n_mult - 1); every level's H*W divides or is a multiple of 128
                              (else create answers ITSD_ERR_INVALID: 8, 16, 32, 64, 128, 256 px hold) */
  int32_t num_labels;      /* CFG only */
  int32_t max_batch;       /* largest n passed to forward/sampler (CFG: per-branch n) */
  int32_t precision;       /* ITSD_PREC_FP32 (parity) or ITSD_PREC_BF16 (throughput) */
} itsd_unet_desc;

/* One state_dict entry (host fp32, contiguous, reference key name). */
typedef struct {
  const char* name;
  const float* data;
  int64_t numel;
} itsd_tensor_view;

int itsd_unet_create(const itsd_unet_desc* desc, const itsd_tensor_view* weights, int n_weights,
                     int device, itsd_unet** out);
int itsd_unet_destroy(itsd_unet* u);

/* eps[n,3,H,W] = UNet(x[n,3,H,W], t[n]) (DDPM) or UNet(x, t, labels[n]) (CFG). */
int itsd_unet_forward(itsd_unet* u, const float* x, const int32_t* t, const int32_t* labels,
                      float* eps, int n, void* stream);

/* repr[n,C,H,W] (NCHW fp32) = the pre-tail activation h of the LAST itsd_unet_forward on this handle
 * (ModelCondition.py:225-235: last_representation = h before self.tail), C = ch * ch_mult[0];
 * stream-ordered after that forward (same stream, or synchronised); n <= that forward's n. */
int itsd_unet_representation(itsd_unet* u, float* repr, int n, void* stream);

/* Host fp32 tables of length T: coeff1, coeff2 and sqrt(var) (the fp32 casts the
 * reference's extract() produces, Diffusion.py:9-16), plus the CFG weight w. */
int itsd_set_schedule(itsd_unet* u, int T, const float* coeff1, const float* coeff2,
                      const float* sqrt_var, float w);

/* The x0-form schedule. Row k of K evaluates the model at timestep tau[k] (strictly increasing, >= 0) and steps
 *     x0 = a0[k] x - b0[k] eps,  clipped to [-1, 1] iff clip_x0;   x' = (c0[k] x0 + cx[k] x) + sg[k] z
 * in fp32 without contraction; where sg[k] == 0, z is neither drawn nor read. All tables are HOST arrays of length K
 * (the fp32 casts of fp64 values: a = abar[tau[k]], p = abar[tau[k-1]] (1 at k = 0), a0 = 1/sqrt(a),
 * b0 = sqrt(1/a - 1), sg = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p), d = sqrt(1 - p - sg^2), c0 = sqrt(p) - d sqrt(a/(1-a)),
 * cx = d/sqrt(1-a); row 0 is (c0, cx, sg) = (1, 0, 0)). w: the CFG weight. */
typedef struct {
  int32_t K;
  const int32_t* tau;
  const float* a0;
  const float* b0;
  const float* c0;
  const float* cx;
  const float* sg;
  int32_t clip_x0;         /* 0 | 1 */
  float w;
} itsd_x0_schedule;

/* Install an x0-form schedule: clears the step graphs, uploads the five tables, builds the time-embedding table as
 * [K][sum Cout] rows for the timesteps tau, and sets T_sched = K ("sched_form" = 1). itsd_set_schedule puts the handle
 * back into the ancestral form: the two calls replace each other. Under this schedule itsd_sampler_run's t_begin / t_end
 * are ROWS, the step counter counts rows, the Philox stream id and the index into an injected noise [K][n][3][H][W] are
 * the row, and itsd_sampler_predict_x0's t is a row (its time embedding is tau[row]'s; the caller passes tau[row]'s
 * a0, b0). ITSD_ERR_INVALID with a message before any HIP call: a null struct or table, K < 1, tau negative or not
 * strictly increasing, clip_x0 outside {0, 1}, a null handle, CFG with tau[K-1] >= the embedding table's rows. */
int itsd_set_schedule_x0(itsd_unet* u, const itsd_x0_schedule* schedule);

/* The 2M schedule: DPM-Solver++(2M) in data prediction on the rows of an x0-form schedule. Everything
 * itsd_set_schedule_x0 does, plus a sixth HOST table cp[K] and a library-owned history hist[max_batch][3][H][W] fp32
 * (allocated at the first such call on the handle, filled by itsd_unet_poison like every buffer); "sched_form" = 2. The
 * three schedule calls replace one another. Row k steps, in fp32 without contraction,
 *     x0 = a0[k] x - b0[k] eps,  clipped to [-1, 1] iff clip_x0
 *     cp[k] != 0:  x0p = (k == restart row) ? x0 : hist ;   m = ((c0[k] x0) + (cp[k] x0p)) + (cx[k] x)
 *     cp[k] == 0:  m = (c0[k] x0) + (cx[k] x)               (hist is not read)
 *     hist = x0 ;  x' = sg[k] != 0 ? m + sg[k] z : m
 * With lambda_k = ln(abar_k / (1 - abar_k)) / 2, h = lambda_{k-1} - lambda_k, r = (lambda_k - lambda_{k+1}) / h and
 * c0d the eta = 0 value of itsd_set_schedule_x0's c0, the caller passes c0[k] = c0d[k] (1 + 1/(2r)) and
 * cp[k] = -c0d[k] / (2r) for 1 <= k <= K - 2; rows K - 1 (no predecessor) and 0 (an infinite last lambda gap) keep c0d
 * and cp = 0: they are first order, and row 0 stays (1, 0, 0). Under CFG hist holds the guided x0 of the n candidates.
 * The restart row: itsd_sampler_run without ITSD_RUN_CONTINUE treats its first step as having no history (the step
 * uses its own x0 for x0p); with the flag the step at t_begin reads what the previous run on this handle left. The
 * handle remembers the row whose x0 hist holds and for how many images (a run sets them to its t_end and n; installing
 * any schedule forgets them), and the flag is refused unless they are t_begin + 1 and n. The restart row is a device
 * run parameter: one captured step graph serves restarted and continued runs.
 * itsd_sampler_predict_x0, itsd_verify_denoise and itsd_unet_forward neither read nor write hist.
 * ITSD_ERR_INVALID with a message naming this function, before any HIP call: everything itsd_set_schedule_x0 refuses,
 * a null cp, a cp[k] that is not finite, cp[K-1] != 0. */
int itsd_set_schedule_x0_2m(itsd_unet* u, const itsd_x0_schedule* schedule, const float* cp);

/* DiffusionCondition.py:79-87 with w a function of (row, image). Host pointers; the library copies them.
 * w_rows [rows] fp32, or NULL = every row the schedule's scalar w; w_img [n_img] fp32 multipliers, or NULL = 1.
 * Both NULL detaches.
 * While attached, the x0-form step of itsd_sampler_run at row k guides candidate image i (never i + n) with
 *   w = w_rows[k] ; if (w_img) w = w * w_img[i] ; w1 = 1.0f + w ; eps = w1 * eps_c - w * eps_u
 * in fp32 without contraction, read on the device from library-owned buffers whose addresses never change: installing
 * new values needs no new graph capture. With w_img NULL and w_rows[k] the schedule's scalar these are the scalar
 * path's bits. The upload is ordered on the handle's stream behind every run already queued (which keeps the values it
 * was queued under) and the call returns when it is done.
 * Cond-only rows: a row with w_rows[k] == 0.0f (the host's copy decides; w_img cannot turn a guided row into one) has
 * eps = eps_c, and its step runs a second program on the n conditional images alone -- half the UNet batch -- through
 * the same step mode's unguided form. Graph mode keeps one graph for each program (the cache key holds "table
 * attached" and "cond-only"). The score trace and the 2M history work on both kinds of row; on a cond-only row the
 * history receives the unguided x0. itsd_set_option("cfg_skip", 0) runs such rows on the doubled batch through the
 * table instead. The two programs pick kernels by batch, so a cond-only row equals its doubled-batch form to rounding,
 * not to the bit.
 * itsd_unet_query: "guidance" = 0 none, 1 rows, 2 rows and per-image multipliers; "cond_only_steps" = steps of the
 * last itsd_sampler_run that ran the cond-only program.
 * itsd_sampler_predict_x0 at row t guides with w_rows[t] as its scalar, and answers ITSD_ERR_INVALID while per-image
 * multipliers are installed; itsd_verify_denoise ignores the table (the probe is unguided). Installing a schedule
 * (any of the three calls) detaches.
 * ITSD_ERR_INVALID with a message naming this function, before any HIP call: a null handle; a non-CFG handle; no
 * x0-form schedule installed (the ancestral form keeps its scalar; ddim with steps = T, eta = 1 is its x0-form
 * equivalent); rows != T_sched; n_img outside [1, max_batch]; a non-finite entry; a tail geometry whose blocks would
 * straddle two images. At run time itsd_sampler_run answers ITSD_ERR_INVALID for n > n_img while multipliers are
 * installed, before any launch. */
int itsd_set_guidance(itsd_unet* u, const float* w_rows, int rows, const float* w_img, int n_img);

/* Run steps t_begin..t_end (inclusive, descending) of the ancestral sampler in
 * place on x[n,3,H,W]. With ITSD_RUN_GRAPH one denoising step is captured per
 * (n, x, labels, noise, option state) and replayed: seed, noise_offset and the clip
 * step are device-side run parameters, so rounds that differ only in them reuse it. noise == NULL: z ~ N(0,1) from counter-based Philox keyed
 * (seed, step, noise_offset + element); otherwise noise is [T][n][3][H][W] fp32 and
 * step t uses noise[t] (t >= 1; the reference draws no noise at t = 0). labels: CFG only.
 * Under an x0-form schedule (itsd_set_schedule_x0) the same call walks rows with that schedule's step; a graph
 * captured under one form is never replayed under another (the form is part of the cache key).
 * ITSD_RUN_CONTINUE (itsd_set_schedule_x0_2m) is refused with ITSD_ERR_INVALID before any launch under the other two
 * forms, at t_begin == K - 1, and when the history does not hold row t_begin + 1 of n images. */
int itsd_sampler_run(itsd_unet* u, float* x, const int32_t* labels, int n, int t_begin, int t_end,
                     uint64_t seed, int64_t noise_offset, const float* noise, uint32_t flags, void* stream);

/* Attach (trace != NULL) or detach a score trace. trace: device fp64 [rows][stride][4], caller-owned,
 * 32-byte aligned; rows must equal T_sched of the installed x0-form schedule (either form: under the 2M schedule the
 * moments are those of the row's own x0, not of the multistep combination), stride >= the n of every run.
 * While attached, step k of itsd_sampler_run on images i < n writes
 * trace[k][i] = (sum x0, sum x0^2, min x0, max x0) over the image's 3 H W elements,
 * x0 the estimate that step used (clipped iff clip_x0); rows not run and images >= n are not written.
 * x after the run is bit-identical to the untraced run.
 * CFG: the x0 of the guided step, for the n candidates. Summation: fp32 without contraction inside a tail block (the
 * thread's items in order, a 6-level lane butterfly, the wave partials in wave order; min / max through the same
 * tree), one plain store of four floats a block, then each image's blocks in block order in fp64 by a second small
 * launch that reads the row from the device step counter -- it is part of the step program, so one captured step
 * graph serves every row. No atomics: a row entry is a function of the candidate alone.
 * The trace pointer and stride are part of the step graph's cache key: a graph captured untraced is never replayed
 * traced, or the reverse, and detaching brings the earlier graph back without a new capture. Installing a schedule
 * (either call) detaches. itsd_sampler_predict_x0 and itsd_verify_denoise ignore the trace.
 * itsd_unet_query(u, "trace", ..) answers 0 | 1.
 * ITSD_ERR_INVALID with a message naming this function, before any HIP call: a null handle; attaching with no
 * x0-form schedule installed (the ancestral form has no a0 / b0 rows; ddim with steps = T, eta = 1 is its x0-form
 * equivalent), rows != T_sched, stride < 1, a pointer that is not 32-byte aligned. At run time itsd_sampler_run
 * answers ITSD_ERR_INVALID for n > stride and for a tail geometry whose blocks would straddle two images (the generic
 * tail kernel with H W % 256 != 0), before any launch. */
int itsd_sampler_set_trace(itsd_unet* u, double* trace, int rows, int stride);

/* x0[n,3,H,W] = clip(a0*x - b0*eps(x, t[, labels]), -1, 1): the sampler's own forward at step t
 * (guided for CFG) with the x0 epilogue; x is not modified. Needs itsd_set_schedule (t < T_sched) or
 * itsd_set_schedule_x0 (t is then a row: the forward runs at timestep tau[t]).
 * x is the state x_t, the INPUT of step t (what itsd_sampler_run(.., t_end = t + 1) leaves); the caller passes
 * a0 = 1/sqrt(abar_t), b0 = sqrt(1/abar_t - 1) (fp64 on the host, cast). Runs eagerly: no step graph is captured or
 * evicted, and the NaN flag of the last itsd_sampler_run is left alone. ITSD_ERR_INVALID before any HIP call: null
 * u / x / x0, t outside [0, T_sched), CFG without labels, n outside [1, max_batch]. */
int itsd_sampler_predict_x0(itsd_unet* u, const float* x, const int32_t* labels, int n, int t,
                            float a0, float b0, float* x0, void* stream);

/* dst[j][e] = a * src[parents[j]][e] + b * z,  z ~ N(0,1) from Philox keyed
 * (seed, stream_id, (cand_offset + j) * per_cand + e) -- the same z itsd_noise draws for candidate
 * cand_offset + j. j < n_dst, e < per_cand. parents: HOST int32[n_dst], each in [0, n_src).
 * src [n_src][per_cand] and dst [n_dst][per_cand] are device fp32 and must not overlap. b == 0: no draw.
 * The table is read during the call (it travels in the kernel arguments) and may be freed after it. A parent out of
 * range, overlapping ranges, a null pointer, n_src < 1, n_dst < 0 or per_cand < 1: ITSD_ERR_INVALID before any HIP
 * call. n_dst == 0: a no-op. */
int itsd_branch(float* dst, const float* src, const int32_t* parents, int n_src, int n_dst, int64_t per_cand,
                float a, float b, uint64_t seed, uint32_t stream_id, int64_t cand_offset, void* stream);

/* out[c][e] = (pivot ? pivot[e] : 0) + scale * z, z ~ N(0,1) from Philox keyed
 * (seed, stream_id, (cand_offset + c) * per_cand + e), for c < n_cand, e < per_cand.
 * Candidate noises are thus a function of their GLOBAL index, so every rank can
 * regenerate any candidate (search_algorithm.py:67 randn, :225 pivot + randn*(1-lambda)). */
int itsd_noise(float* out, const float* pivot, int n_cand, int64_t per_cand, float scale, uint64_t seed,
               uint32_t stream_id, int64_t cand_offset, void* stream);

/* ---- The antithetic evolution-strategies gradient: GradientBasedSearch without autograd. Throughout,
 * z_p[e] = Philox (seed, stream_id, p * per_cand + e): itsd_noise's draw for candidate p. Every fp32 expression below is
 * evaluated without contraction in the order its parentheses state; no atomics: a call is bit-reproducible.
 *
 * out[j][e] = pivot[e] + (s * z_p[e]) for the global candidate c = cand_offset + j, j < n_cand: pair p = c >> 1,
 * s = +sigma for an even c, -sigma for an odd one (pairing is by global index: a shard may begin on a minus
 * candidate). out [n_cand][per_cand] and pivot [per_cand] are device fp32. ITSD_ERR_INVALID with a message before any
 * HIP call: a null out / pivot, n_cand < 0, per_cand < 1, cand_offset < 0, sigma not finite or <= 0. n_cand == 0: a
 * no-op. */
int itsd_es_candidates(float* out, const float* pivot, int n_cand, int64_t per_cand, float sigma, uint64_t seed,
                       uint32_t stream_id, int64_t cand_offset, void* stream);

/* Bytes of the workspace itsd_es_step needs for n_pairs pairs of per_cand elements (the slice sums of the gradient,
 * ceil(n_pairs / 16) * per_cand fp32, and one fp64 a block of the update); <= 0: invalid arguments. No device call. */
int64_t itsd_es_workspace_bytes(int n_pairs, int64_t per_cand);

/* The Adam constants of one step, computed in fp64 on the host and cast: omb1 = 1 - beta1, omb2 = 1 - beta2,
 * c1 = lr / (1 - beta1^k), c2 = 1 / sqrt(1 - beta2^k), k = 1 for the first step. */
typedef struct { float beta1, omb1, beta2, omb2, c1, c2, eps; } itsd_adam_step;

/* One ascent step on theta [per_cand] from the weights w [n_pairs] (device fp32; for the ES estimate of the gradient
 * of a score, w[p] = (score of candidate 2p - score of candidate 2p + 1) / (2 n_pairs sigma)):
 *   g[e]  = sum over the slices q of (sum over the pairs p of slice q of (w[p] * z_p[e]))
 *           slice q = pairs [kEsSlice q, min(n_pairs, kEsSlice (q + 1))), kEsSlice = 16 (csrc/common.h); both sums
 *           ascend and start from 0.0f; a pair with w[p] == 0 is not drawn
 *   gl = -g;  m' = (beta1 m) + (omb1 gl);  v' = (beta2 v) + (omb2 (gl gl));
 *   den = (sqrtf(v') c2) + eps;  theta' = theta - ((c1 m') / den)
 * theta, m, v are updated in place (torch.optim.Adam's step on grad = -g: it ascends g). grad_out (NULL ok) receives
 * g; gnorm2_out (device fp64 [1]) the sum of g^2 in fp64: every block of the update adds its elements in a fixed order
 * and a last launch adds the blocks in block order. ws: itsd_es_workspace_bytes(n_pairs, per_cand) bytes of device
 * memory, 16-byte aligned, overwritten. ITSD_ERR_INVALID with a message before any HIP call: a null theta / m / v / w /
 * adam / gnorm2_out / ws, n_pairs < 1, per_cand < 1, beta1 or beta2 outside [0, 1), eps <= 0, a non-finite field of
 * adam, a misaligned ws, or any two of theta / m / v / grad_out / ws overlapping. */
int itsd_es_step(float* theta, float* m, float* v, const float* w, int n_pairs, int64_t per_cand, uint64_t seed,
                 uint32_t stream_id, const itsd_adam_step* adam, float* grad_out, double* gnorm2_out, void* ws,
                 void* stream);

/* scores[c] = verifier(images[c*b:(c+1)*b]) for c < n_cand; images NCHW fp32.
 * ITSD_VERIFY_MEAN is OracleVerifier.score with dataset_stats (search/verifier.py:66: mean). */
int itsd_verify(int kind, const float* images, int n_cand, int b, int c, int h, int w,
                double* scores, void* stream);

/* SelfSupervisedVerifier.score(images, reference_features) (search/verifier.py:235-240):
 * scores[i] = cos(pool8x8(images[i]), ref_features[i]) for i < n_cand (one image per
 * candidate: the reference's .item() of the per-image vector needs a single image);
 * ref_features [n_cand][c*64] fp32. */
int itsd_verify_paired(const float* images, const float* ref_features, int n_cand, int c, int h, int w,
                       double* scores, void* stream);

/* One denoising-error probe of n images at row t of the installed schedule:
 *   x_t = (a x0) + (b z);  sse[i][0] = sum_e (z - eps_c(x_t, t, label_i))^2;
 *   sse[i][1] = sum_e (z - eps_u(x_t, t))^2  (CFG, eps_u under label 0; DDPM: 0).  x0 [n,3,H,W] is only read.
 * z is ONE field [3][H][W] shared by every image of the call: noise (device fp32) when non-NULL, else Philox keyed
 * (seed, stream_id, element within the image) -- itsd_noise's draw for one candidate. A sum is therefore a function of
 * (image, label, seed / field, t) alone: not of n, of the image's place in the batch, or of its neighbours. t means
 * what it means for itsd_sampler_predict_x0 (a timestep, or a row of an x0-form schedule: the time embedding is
 * tau[t]'s); the caller passes a = sqrt(abar), b = sqrt(1 - abar) of that row (fp64 on the host, cast). The forward is
 * the sampler step's own program (the doubled cond||uncond batch for CFG) and is NOT guided: the two errors come from
 * the two branches. All arithmetic on z is fp32 without contraction; every block of the tail sums its elements in a
 * fixed order and a second launch adds each image's block sums in block order in fp64 (no atomics: bit-reproducible).
 * sse: device fp64 [n][2]. xt_out (NULL ok) receives x_t [n,3,H,W]; eps_out (NULL ok) the unguided eps,
 * [1 (DDPM) or 2 (CFG: cond, then uncond)][n][3][H][W]: both for tests, NULL in production. Runs eagerly on the
 * handle's stream: no step graph is captured or evicted, the NaN flag and the run parameters of the last
 * itsd_sampler_run are left alone, and the hand-off status word ("status") is this forward's. The probe's x_t and
 * the tail's per-block sums live in two library-owned buffers allocated at the first call (itsd_unet_poison fills
 * them too). ITSD_ERR_INVALID with a message before any HIP call: null u / x0 / sse, no schedule installed, CFG
 * without labels, n outside [1, max_batch], t outside [0, T_sched). */
int itsd_verify_denoise(itsd_unet* u, const float* x0, const int32_t* labels, int n, int t, float a, float b,
                        uint64_t seed, uint32_t stream_id, const float* noise, double* sse, float* xt_out,
                        float* eps_out, void* stream);

/* AttnBlock core on n images of S tokens, width C (single head):
 *   out[i][s][:] = softmax_j(q_s . k_j * C^-0.5) v_j
 * qkv: [n][S][3C] (q | k | v per token, the fused projection the UNet produces);
 * precision ITSD_PREC_FP32: fp32 tensors; ITSD_PREC_BF16: bf16 tensors and vt, the
 * channel-major V [n][C][S] (the MFMA kernels read V^T; S <= 256: whole-row kernel,
 * S > 256: the flash kernel, S % 32 == 0 and C in {64,128,256}, or the channel-split kernel,
 * S % 64 == 0 and C in {256,384,512,1024}), out [n][S][C]. */
int itsd_attention(const void* qkv, const void* vt, void* out, int n, int S, int C, int precision, void* stream);

/* Census of one forward at batch n (synchronous): runs the op program eagerly with
 * HIP events around every launch. Outputs (any may be NULL):
 *   conv_ms / conv_flops / conv_launches : the implicit-GEMM conv kernel
 *   total_ms                              : the whole forward (sum of launches) */
int itsd_profile_forward(itsd_unet* u, const float* x, const int32_t* t, int n, double* conv_ms,
                         double* conv_flops, int* conv_launches, double* total_ms, void* stream);

/* Per-launch census of one forward (synchronous, eager, HIP events): for launch i
 * (head, program ops in order, tail GN, tail) kinds[i] = (kernel << 8) | (kind & 0xff) with
 * kind the op class (0 GN, 1 conv, 2 attention, 3 GN finalize, 4/5/6 fused GroupNorm conv
 * 128 px / 256 px / 8x8 level; -1 head, -2 tail, as a signed byte) and kernel the id of
 * the first kernel the launch ran (itsd_kernel_name), ms[i], flops[i] and shapes[8*i..] =
 * {M, Cout, K or Cin, Hout, ksize, 10*stride+upsample, op, flags} with op the program op index
 * (1-based, itsd_profile_op's numbering; 0 = head / tail). Ops whose launch is folded into the
 * next one (a GroupNorm finalize done by conv3x3_gn_p5_kernel) have no entry. kind 7 = the fused
 * AttnBlock. flags: bit 0 the op adds a residual, bit 1 it writes its output's GroupNorm statistics, bit 2
 * its input GroupNorm(+SiLU) is fused (statistics read). CFG UNets run with label 0.
 * At most max_ops entries; *n_ops = entries written. */
int itsd_profile_ops(itsd_unet* u, const float* x, const int32_t* t, int n, int max_ops, int* kinds,
                     double* ms, double* flops, int* shapes, int* n_ops, void* stream);

/* Steady-state duration of one program op (synchronous): runs one forward at batch n to set up
 * its inputs, then launches op `op_index` (census numbering of itsd_profile_ops: 1 = first
 * program op) `reps` times back to back between two HIP events on the UNet's stream;
 * *ms = elapsed / reps. The per-launch time a replayed step graph sees, without the eager
 * census's per-launch event overhead. */
int itsd_profile_op(itsd_unet* u, const float* x, const int32_t* t, int n, int op_index, int reps, double* ms,
                    void* stream);

/* Process-wide choices between the shipped paths (api.hip's kOptions table is the list: every key with its range
 * and meaning): kernel and tile choices ("conv_variant", "splitk" 0/1, "splitk_inl", "subpix_split", "conv1x1" 0/1,
 * "small_conv", "small_8x8", "small_wide", "small_gn", "gn_wide", "gn_fold", "p4_w", "p4_c96", "p4_sub", "p4_plain",
 * "p5", "p5_split", "p5_sc", "p5_pub", "p5_xl", "p5_dist", "convt_prune", "attn_split", "attn_wide",
 * "attn_wide_nq"), the in-kernel hand-off poll bound ("spin_bound"), the cond-only step of w = 0 guidance rows
 * ("cfg_skip" 0/1, itsd_set_guidance), and build-time choices read at create
 * ("fuse_gn", "io_mfma", "attn_fuse", "attn_s1", "tap_prune", "down_merge"). Defaults are the shipped choices; every
 * alternative is covered by a parity test. Measurement switches of measured-and-dropped variants ("conv_dbg",
 * "attn_cs", "attn_aq", "p4_xcd", "small_minks", "p5_c64", forced "splitk" slice counts, "conv1x1" 2) exist in
 * diagnostic builds only (tools/build_diag.sh): this library returns ITSD_ERR_INVALID for them. A refused call
 * leaves the previous value in place. */
int itsd_set_option(const char* key, int value);

/* Introspection of a handle (no device work): "graph_captures" (step graphs captured and
 * instantiated so far; a search replays one graph across all its rounds), "max_batch",
 * "T_sched" (timesteps, or the rows K of an x0-form schedule), "sched_form" (0 ancestral, 1 x0-form, 2 the 2M x0-form), "trace" (1 while a score trace is attached), "guidance" and "cond_only_steps" (itsd_set_guidance), "ws_bytes"
 * (activation arena), "ops" (program length); and, synchronising the
 * handle's stream, "status" = the in-kernel hand-off status word of the last forward / sampler run
 * (0 ok; bit 0: attn_block_split_kernel's wait exhausted its bound, bit 1: conv3x3_gn_p5_kernel's shared split-K
 * combine -- ITSD_ERR_HANDOFF). */
int itsd_unet_query(const itsd_unet* u, const char* key, int64_t* value);

/* ---- Introspection of the op program (read-only; eager host code, nothing on the sampler's path).
 * The per-op parity tests walk the program with these: describe an op, read what it read and wrote.
 *
 * Op indices are itsd_profile_ops' (1 = first program op .. "ops"); 0 is the head conv and "ops" + 1 the tail
 * (GroupNorm + conv). Act ids index the handle's activation buffers (every op output has its own buffer; the
 * channel-major V buffers are activations too, shaped H = C, W = S, C = 1); ITSD_ACT_PROJ is proj_buf, the
 * [n][sumC] fp32 temb_proj rows of the last itsd_unet_forward. -1 = none. */
enum { ITSD_OP_GN = 0, ITSD_OP_CONV = 1, ITSD_OP_ATTN = 2, ITSD_OP_GNCOEF = 3, ITSD_OP_ATTNBLOCK = 4,
       ITSD_OP_HEAD = 5, ITSD_OP_TAIL = 6 };
/* ops whose weights are not one state_dict tensor (itsd_op_info::tag) */
enum { ITSD_TAG_NONE = 0,
       ITSD_TAG_QKV = 1,         /* 1x1 conv over proj_q | proj_k | proj_v of the AttnBlock `name` */
       ITSD_TAG_DOWN_MERGE = 2,  /* CFG DownSample `name`: c1 (3x3) + c2 (5x5) as one 5x5 conv */
       ITSD_TAG_ATTN_S1 = 3,     /* one-token AttnBlock `name`: resid + proj(proj_v(src1)), src1 = its GroupNorm */
       ITSD_TAG_CONVT = 4,       /* ConvTranspose2d(5, 2, 2, 1) `name` */
       ITSD_TAG_ATTNBLOCK = 5 }; /* the fused AttnBlock `name` (GroupNorm, q|k|v, attention, proj, + x), run with
                                    proj_q^T proj_k and proj proj_v folded at create: bf16 roundings of the GroupNorm
                                    output, the two folded projections, the softmax weights and the output */
#define ITSD_ACT_PROJ (-2)
typedef struct {
  int32_t kind;                    /* ITSD_OP_* */
  int32_t launched;                /* 1: run_program launches it at this batch / option state; 0: folded away */
  int32_t folded_into;             /* launched == 0: the op (index) whose launch does this op's work */
  int32_t src1, src2, dst, resid, vt;  /* act ids */
  int32_t ksize, stride, pad, upsample, zins, subpix, Cout, K, temb_col, vt_from;  /* conv geometry as built */
  int32_t silu;                    /* GN: SiLU applied */
  int32_t S, C;                    /* attention kinds: tokens, width */
  int32_t kernel;                  /* conv: the plan's ConvKernel enumerator (common.h order), else -1 */
  int32_t ksplit, sc_split, kS;    /* conv: the plan's p5 K slices, folded-shortcut slices, conv_small / pipe slices */
  int32_t epilogue;                /* conv: kS slices combined by a second launch (splitk_epilogue_kernel) */
  int32_t gn_fold;                 /* conv: finalizes its input GroupNorm itself (its GNCOEF op is not launched) */
  int32_t gn_out_op;               /* conv: the GN op (index) whose dst its epilogue writes, 0 none */
  int32_t sc_op;                   /* conv with sc_split > 0: the shortcut op (index) it absorbs, else 0 */
  int32_t has_coef;                /* GNCOEF / tail: writes a coef buffer; conv: its input GroupNorm is fused */
  int32_t tag;                     /* ITSD_TAG_* */
  char name[96];                   /* the state_dict prefix the op was built from, e.g. "downblocks.3.block2.3" */
} itsd_op_info;
typedef struct {
  int32_t H, W, C;
  int32_t elem_size;               /* bytes: 2 (bf16) or 4 */
  int32_t has_stats;               /* a GroupNorm statistics slab [n * spi][2][C] fp32 belongs to it */
  int32_t spi;                     /* its slots per image (stat_spi: HW / min(HW, 128), or 4 phases) */
  int32_t capacity;                /* images the buffer holds */
} itsd_act_info;
/* What program op `op_index` is and how it would run at batch n under the current options: resolved exactly as
 * the pass resolves it -- ITSD_PASS_FORWARD: itsd_unet_forward; ITSD_PASS_STEP: the sampler step of
 * itsd_sampler_run / itsd_sampler_predict_x0, whose program runs 2n images for CFG (cond || uncond: image i >= n
 * reads x[i - n] and label 0, and the tail combines the halves). No launch, no device call. ITSD_ERR_INVALID: null
 * u / info, unknown pass, op_index outside [0, ops + 1], n outside [1, max_batch]. */
enum { ITSD_PASS_FORWARD = 0, ITSD_PASS_STEP = 1 };
int itsd_unet_op_info(itsd_unet* u, int pass, int n, int op_index, itsd_op_info* info);
/* ITSD_ERR_INVALID: null u / info, act neither ITSD_ACT_PROJ nor in [0, acts). No device call. */
int itsd_unet_act_info(const itsd_unet* u, int act, itsd_act_info* info);
/* Stream-ordered device-to-device copy of raw buffer contents (no conversion) into dst (device, `bytes` long):
 * ITSD_READ_ACT: the first n images of activation `id` (n H W C elements); ITSD_READ_STATS: its statistics slab
 * (n spi 2 C fp32); ITSD_READ_COEF: the coef buffer [n][Cin/8][a0..a7, b0..b7] fp32 of GNCOEF op `id` (or of the
 * tail, id = ops + 1); ITSD_READ_PROJ: proj_buf (n sumC fp32; id ignored). ITSD_ERR_INVALID before any HIP call:
 * null u / dst, unknown what, id out of range or without such a buffer, n outside [1, capacity], bytes != the
 * size above. */
enum { ITSD_READ_ACT = 0, ITSD_READ_STATS = 1, ITSD_READ_COEF = 2, ITSD_READ_PROJ = 3 };
int itsd_unet_read(itsd_unet* u, int what, int id, int n, void* dst, int64_t bytes, void* stream);
/* Fill every buffer a forward overwrites completely with NaN bits (bf16 0xFFFF, fp32 0xFFFFFFFF), stream-ordered:
 * the activation arena (activations, channel-major V, coef buffers and the statistics slabs -- every producer
 * stores its slots plainly, none accumulates), the split-K workspace and, once allocated, itsd_verify_denoise's two
 * scratch buffers. Left alone: what the program increments or
 * needs zero between launches (split-K tickets, the AttnBlock hand-off counters, the NaN / status words, the zero
 * page), the weights, proj_buf and the embedding tables. A forward afterwards must give the bits it gives on a fresh
 * handle: a NaN or a changed value means a launch read something no launch of that forward wrote. */
int itsd_unet_poison(itsd_unet* u, void* stream);

/* Name of census kernel id `id` (itsd_profile_ops): the launch site's kernel expression,
 * e.g. "conv3x3_gn_p4_kernel<32>"; "" for 0 / unknown ids. */
const char* itsd_kernel_name(int id);

/* On-box peak calibration (synchronous on stream; measurement only, no reference counterpart):
 * ITSD_CALIB_MFMA_BF16 -> *value = the achievable dense bf16 MFMA rate in TFLOP/s (v_mfma_f32_32x32x16_bf16
 * chains on random operands, every CU, 2 waves per SIMD); ITSD_CALIB_HBM_COPY -> *value = the achievable
 * HBM streaming rate in GB/s (a 1 GiB 16-B-per-lane copy, bytes read + written); ITSD_CALIB_MFMA_BF16_16X16
 * -> the ITSD_CALIB_MFMA_BF16 loop on v_mfma_f32_16x16x32_bf16 (the chip holds another clock under that shape).
 * bench.py reports its roofline fractions against these as well as against the datasheet peaks. */
enum { ITSD_CALIB_MFMA_BF16 = 0, ITSD_CALIB_HBM_COPY = 1, ITSD_CALIB_MFMA_BF16_16X16 = 2 };
int itsd_calibrate(int what, double* value, void* stream);

const char* itsd_last_error(void);
int itsd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ITSD_H */
