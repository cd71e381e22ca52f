/* pert_hip.h -- C ABI of the MI355X PERT hot path (libpert_hip.so, gfx950).
 *
 * The reference has no FFI: its replaceable unit is Pyro's
 *   svi.step(gammas, libs, data=..., etas=..., lamb=..., t_init=...) -> float
 * (scdna_replication_tools/pert_model.py:743 step 1, :801 step 2, :868 step 3)
 * plus the MAP decode infer_discrete(temperature=0) (:762-769, :820-827, :886-893).
 * One SVI step of this library is the launch sequence
 *   pert_enum_pass(PERT_MODE_STEP)   (steps 2/3)  or  pert_obs_pass()  (step 1)
 *   pert_finalize()                  per-cell / per-bin / global gradient reductions
 *   [all-reduce of the shared gradient block across ranks, from the host]
 *   pert_adam()                      Adam on the packed non-pi parameters
 * and the decode is pert_enum_pass(PERT_MODE_DECODE).  With the three-wave pass (variant 3)
 * a step of steps 2/3 is instead pert_enum_step() [+ all-reduce + pert_adam_shared()].
 *
 * Conventions: every buffer is device memory owned by the caller (allocated via
 * the torch caching allocator on the caller's side); nothing here allocates.  All
 * launches go on the caller's stream.  Entry points return 0 on success, a
 * positive PERT_E* code for an argument error and 1000 + hipError_t for a launch
 * failure.  A NaN loss is returned as data (pert_model.py:755-758), never raised.
 *
 * Layouts (bin-major like the reference's (loci x cells) tensors, pert_model.py:156-166);
 * ldn = N rounded up to a multiple of 256 (PERT_BLOCK); padded cells are never stored:
 *   reads      float  [L][ldn]     integer-valued counts
 *   gcf        float  [L][K1]      [gc^K .. gc^1, 1] (make_gc_features, pert_model.py:460-463)
 *   eta_code   uint16 [L][ldn]     row index into eta_table          (steps 2/3)
 *   eta_table  float  [n_codes][P+2]  eta_k - 1 for k < P, then S1 = sum_k (eta_k - 1), then
 *                                   A = fp32 lgamma(sum_k eta_k) as torch evaluates it: each
 *                                   element's Dirichlet value is rounded to A's grid as the
 *                                   reference's fp32 log_prob rounds it (0: not rounded)
 *   z_pi/m_pi/v_pi/g_pi float [ldn/64][L][P][64]  softmax logits of expose_pi and Adam
 *                                   moments in wave tiles: cell n, state k of bin l at
 *                                   (((n/64)*L + l)*P + k)*64 + n%64  (a wave streams one
 *                                   contiguous run over its bins)
 *   cn_obs/rep_obs, cn_out/rep_out uint8 [L][ldn]
 *   packed params (unconstrained, see pert_layout below), float
 *
 * Step 1 pair mode (rep_obs == NULL): the training set of pert_model.py:228-251 -- every
 * G1/2 cell twice, rep 0 then rep 1, same reads and CN -- stored once: N is even, cells
 * [0, N/2) are the rep-0 copies and [N/2, N) the rep-1 copies of the N/2 columns that reads
 * and cn_obs hold, whose row stride ldn (>= N/2, multiple of 256) is that of the stored
 * arrays.  Parameters, libs, mean_reads, ploidy and the workspace stay per cell (N).
 */
#ifndef PERT_HIP_H
#define PERT_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERT_KIND_STEP1 1   /* G1/2 cells, cn/rep observed (pert_model.py:718-774) */
#define PERT_KIND_STEP2 2   /* S cells, cn x rep enumerated (:776-830) */
#define PERT_KIND_STEP3 3   /* step 2 with rho, a frozen, on G1 cells (:834-896) */

#define PERT_MODE_STEP   0  /* ELBO + grads + fused Adam on pi + reduction partials */
#define PERT_MODE_GRAD   1  /* ELBO + grads; d(-ELBO)/dz_pi written to g_pi, no update */
#define PERT_MODE_DECODE 2  /* joint argmax over (rep, cn): cn_out, rep_out */

#define PERT_OK 0
#define PERT_E_ARG 1
#define PERT_E_UNSUPPORTED_P 2
#define PERT_E_UNSUPPORTED_K 3
#define PERT_E_COMM_UNAVAILABLE 5   /* RCCL not loaded (pert_comm_load) or lacks a symbol */
#define PERT_E_COMM_ABORTED 6       /* a rank of the fit failed and raised the abort word */
#define PERT_E_COMM_TIMEOUT 7       /* a peer did not arrive within the communicator's deadline */
#define PERT_E_COMM_FAULT 8         /* injected by pert_comm_inject_fault (tests) */
#define PERT_E_HIP_BASE 1000        /* + hipError_t */
#define PERT_E_COMM_BASE 2000       /* + ncclResult_t */

#define PERT_MAX_K1 8      /* K + 1 <= 8 */
#define PERT_MIN_P 2
#define PERT_MAX_P 16
#define PERT_BLOCK 256     /* cells per workgroup (4 waves x 64 lanes) */

/* Offsets into the packed parameter / gradient vectors.  The shared block
 * [0, n_shared) is replicated on every rank and its gradient is all-reduced;
 * the cell block [n_shared, n_params) is local to the rank's cell shard. */
typedef struct {
  int32_t off_rho;     /* L    z_rho (unit interval)                          */
  int32_t off_a;       /* 1    z_a   (positive)                               */
  int32_t off_lam;     /* 1    z_lambda (interval(0.001, 0.999)), step 1      */
  int32_t off_bstds;   /* n_libs*K1  z_beta_stds (positive)                   */
  int32_t off_bmeans;  /* n_libs*K1  beta_means (real), step 1                */
  int32_t n_shared;
  int32_t off_u;       /* N    u (real)                                        */
  int32_t off_beta;    /* K1*N betas, plane layout [k][n]                      */
  int32_t off_tau;     /* N    z_tau (unit interval)                           */
  int32_t n_params;
} pert_layout;

typedef struct {
  int32_t kind, L, N, P, K1, n_libs, n_codes;
  int32_t ldn;                     /* row stride (cells) of every [L][*] array: N rounded up to 256 */
  int32_t is_root;                 /* adds the global priors once across ranks */
  const float* reads;
  const float* gcf;
  const int32_t* libs;             /* [N] library index per cell */
  const uint16_t* eta_code;        /* steps 2/3 */
  const float* eta_table;
  const uint8_t* cn_obs;           /* step 1 */
  const uint8_t* rep_obs;
  const float* mean_reads;         /* [N] mean over bins of reads (u prior, :597) */
  const float* ploidy;             /* [N] mean argmax eta (steps 2/3) or 2 (step 1) */
  float lamb;                      /* steps 2/3: fixed lambda from step 1 */
  float log1m_lam;                 /* log(1 - lamb) */
  double sum_reads;                /* step 1: sum of reads of this shard (d/dlam of x log lam), fp64 */
  float a_fixed;                   /* step 3 */
  const float* beta_means;         /* steps 2/3 fixed [n_libs][K1] */
  const float* rho_fixed;          /* step 3 [L] constrained */
} pert_problem;

typedef struct {
  pert_layout lay;
  float* params;                   /* [n_params] unconstrained */
  float* adam_m;                   /* [n_params] */
  float* adam_v;                   /* [n_params] */
  double* grad_shared;             /* [n_shared + 1]: d loss / d shared params, then loss (local sum) */
  float* grad_cell;                /* [n_params - n_shared] */
  float* z_pi;                     /* [ldn/64][L][P][64] steps 2/3 */
  float* m_pi;
  float* v_pi;
  float* g_pi;                     /* [ldn/64][L][P][64] only for PERT_MODE_GRAD */
  uint8_t* cn_out;                 /* [L][ldn] PERT_MODE_DECODE */
  uint8_t* rep_out;
  /* workspace, sized by pert_workspace_sizes() */
  float* cell_part;
  float* bin_part;
  double* blk_part;
  double* cellblk_part;
  int32_t bins_per_tile;           /* LT; 0 = library default */
  int32_t variant;                 /* enumerated-pass kernel: 0 LDS-DMA streamed (two waves per SIMD),
                                      2 = variant 0 + wave timeline stamps into g_pi (diagnostic, STEP mode),
                                      3 = three waves per SIMD, online logsumexp (pert_enum_step);
                                      anything else (1 was retired in round 3) -> PERT_E_ARG */
  /* Device-side SVI loop control (the loop of pert_model.py:742-758, :800-816, :867-883).
   * loop_ctl == NULL disables it.  Otherwise pert_adam records the loss of iteration
   * `step` (after the cross-rank all-reduce) into loop_rec and evaluates the reference's
   * stopping rule on the device: rel-tol plateau once step >= min_iter (:749-753), then
   * NaN (:755-758); on a stop it sets loop_ctl[0] = step.  Every PERT_MODE_STEP /
   * obs / finalize / adam launch of a later step is then a no-op, so the host can queue
   * iterations ahead without a per-step synchronisation and the fit still stops after
   * exactly the iteration the reference stops after. */
  int32_t* loop_ctl;               /* [2]: stop_at (-1 while running), reason (1 rel_tol, 2 NaN) */
  double* loop_rec;                /* [max_iter][2]: loss of each step, stop_at after it */
  const double* loss_offset;       /* [max_iter] or NULL: per-step loss term kept on the host side
                                      of the ABI (step 1's canonical pi block) */
  double loss_const;               /* loss = grad_shared[n_shared] - loss_const - loss_offset[step] */
  double rel_tol;
  int32_t min_iter;
  int32_t step;                    /* 0-based iteration index of this launch sequence */
} pert_state;

typedef struct {
  float lr, beta1, beta2, eps;
  float step_size;                 /* lr / (1 - beta1^t)               (torch/optim/adam.py) */
  float inv_bc2_sqrt;              /* 1 / sqrt(1 - beta2^t)                               */
} pert_adam_hparams;

/* Packed layout for (kind, L, N, K1, n_libs). */
int pert_make_layout(int32_t L, int32_t N, int32_t K1, int32_t n_libs, pert_layout* out);

/* Workspace element counts for cell_part (float), bin_part (float), blk_part (double),
 * cellblk_part (double) at bins_per_tile (0 = default).  cellblk_part must be
 * zero-initialised once: its last element holds pert_finalize's arrival counter, which
 * every finalize launch leaves at zero again. */
int pert_workspace_sizes(int32_t kind, int32_t L, int32_t N, int32_t K1, int32_t n_libs,
                         int32_t bins_per_tile, int64_t* n_cell_part, int64_t* n_bin_part,
                         int64_t* n_blk_part, int64_t* n_cellblk_part);

/* Bins per workgroup tile for the enumerated pass of this shard on the current device:
 * the tile length in [8, 64] whose grid (ldn/64 cell tiles x ceil(L/LT) bin tiles) best
 * fills whole rounds of the device's resident wave slots (occupancy queried for the
 * kernel instance and its LDS at that length), so a small shard does not end on a
 * partly filled last round.  Written to *out; steps 2/3 only (step 1 uses the default). */
int pert_auto_bins_per_tile(const pert_problem* prob, int32_t variant, int32_t* out);

/* Enumerated (steps 2/3) pass over every (bin, cell) of the shard.
 * Replaces the JitTraceEnum_ELBO forward + autograd backward of pert_model.py:801 / :868,
 * and with PERT_MODE_STEP the pi part of the Adam update; with PERT_MODE_DECODE it is
 * infer_discrete(temperature=0) of :820-827 / :886-893. */
int pert_enum_pass(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                   int32_t mode, hipStream_t stream);

/* One whole SVI step of steps 2/3 as ONE launch (variant 3 only): the PERT_MODE_STEP pass
 * with pert_finalize's reductions folded in -- the last bin tile of each cell tile to finish
 * reduces that tile's per-cell partials and runs Adam on its cells' u / betas / tau, the last
 * cell tile of each bin tile reduces that tile's rho partials, and the last of those adds
 * the global sums into grad_shared (loss in slot n_shared).  update_shared != 0 (a single
 * rank): the same launch also records the loss for the device loop and runs Adam on the
 * shared block.  update_shared == 0 (several ranks): all-reduce grad_shared, then
 * pert_adam_shared().  Uses the arrival counters at the end of cellblk_part (sized by
 * pert_workspace_sizes, zero-initialised once, re-armed by every launch).
 * Replaces svi.step() of pert_model.py:801 / :868 with the same update. */
int pert_enum_step(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                   int32_t update_shared, hipStream_t stream);

/* Adam on the shared block [0, n_shared) only (after the all-reduce of a pert_enum_step with
 * update_shared == 0), plus the device loop's loss record / stopping rule. */
int pert_adam_shared(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                     hipStream_t stream);

/* Observed (step 1) pass: JitTrace_ELBO forward + backward of pert_model.py:743.  In pair
 * mode (rep_obs == NULL, see the layouts above) one lane evaluates both copies of a G1/2 cell
 * from one load of its reads and CN (bins_per_tile up to 128). */
int pert_obs_pass(const pert_problem* prob, pert_state* st, hipStream_t stream);

/* Reductions of the pass partials + priors of the non-enumerated sites (pert_model.py:553-603)
 * -> grad_cell (local) and grad_shared (local partial sums incl. the loss in slot n_shared).
 * One launch: its last workgroup to finish adds the global sums. */
int pert_finalize(const pert_problem* prob, pert_state* st, hipStream_t stream);
/* pert_finalize split in two for a sharded step, so the shared block's all-reduce overlaps the
 * per-cell work: _shared writes grad_shared (local sums and loss) from the bin partials, the
 * pass's ELBO / d/da partials and the priors' terms (parameters only); _cells writes grad_cell
 * from each cell's partial rows and the u / beta / tau priors.  Together they write exactly
 * what pert_finalize writes; pert_adam follows both. */
int pert_finalize_shared(const pert_problem* prob, pert_state* st, hipStream_t stream);
int pert_finalize_cells(const pert_problem* prob, pert_state* st, hipStream_t stream);

/* Adam (torch.optim.Adam semantics, betas (0.8, 0.99)) on the packed params with
 * grad_shared (already all-reduced) and grad_cell. */
int pert_adam(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
              hipStream_t stream);

/* n whole SVI steps of a single-rank fit queued in one call (no all-reduce between the
 * reductions and Adam, so one rank only): for i < n the step of loop iteration iter0 + i
 * (st->step, the device loop's record index) with Adam hyper-parameters hp and
 * hp->step_size = step_size[i], hp->inv_bc2_sqrt = inv_bc2_sqrt[i] (host arrays the caller
 * computes for Adam steps t as torch.optim.Adam does: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)).
 * Each step is pert_enum_step(update_shared = 1) when one_launch (steps 2/3, variant 3), else
 * pert_enum_pass(PERT_MODE_STEP) or pert_obs_pass, then pert_finalize and pert_adam.  With the
 * device loop armed (loop_ctl), the steps after the stopping one are no-ops.  pass_events
 * (NULL, or 2n caller-created events, NULL entries skipped): events[2i] / events[2i+1] are
 * recorded on the stream around step i's pass launch (the one launch of a one_launch step).  The call
 * only queues launches (a few microseconds each), so a binding may release its interpreter
 * lock around it.  Replaces n iterations of the svi.step loop of pert_model.py:742-758 /
 * :800-816 / :867-883 (the loss record and stopping rule stay on the device). */
int pert_svi_steps(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                   const float* step_size, const float* inv_bc2_sqrt, int32_t iter0, int32_t n,
                   int32_t one_launch, hipEvent_t* pass_events, hipStream_t stream);

/* A whole single-rank SVI fit with the device loop armed (st->loop_ctl / loop_rec set): up to
 * n_iter iterations queued in chunks of `chunk` (pert_svi_steps, step_size / inv_bc2_sqrt hold
 * all n_iter entries), each chunk followed by a copy of its loss records into host_rec (pinned
 * host memory, [n_iter][2] doubles) and an event; at most `depth` chunks are in flight, and
 * queueing ends once a copied record shows the stop.  pass_events: NULL, or 2 n_iter
 * caller-created events (NULL entries skipped) recorded around iteration i's pass as in
 * pert_svi_steps.  Returns after the stream has drained,
 * with *n_launched = the iterations queued (loop_ctl[0] holds the stopping iteration).  One
 * call per fit, so a binding that releases its interpreter lock around it leaves the host
 * thread free for the rest of the program for the whole fit.  Replaces the loop of
 * pert_model.py:742-758 / :800-816 / :867-883. */
int pert_svi_run(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                 const float* step_size, const float* inv_bc2_sqrt, int32_t n_iter, int32_t chunk,
                 int32_t depth, int32_t one_launch, hipEvent_t* pass_events, double* host_rec,
                 int32_t* n_launched, hipStream_t stream);

/* ---- Sharded fits: cells split over ranks, one process per GPU.
 * The shared block's gradient [0, n_shared) and the loss (slot n_shared) are summed across
 * the ranks once per SVI step, between the reductions and Adam.  A pert_comm is an RCCL
 * communicator over the fit's ranks (xGMI) -- or, for ranks sharing a GPU (which RCCL
 * refuses; tests), a host-staged sum through POSIX shared memory -- and the library queues
 * that all-reduce itself on the fit's stream, so a whole sharded fit is one C call like a
 * single-rank one.  Failure is bounded: a rank whose loop fails raises the node's abort word
 * (and aborts its RCCL communicator), and a rank waiting on its stream polls that word, RCCL's
 * async error and a deadline instead of blocking; the loop then returns PERT_E_COMM_ABORTED /
 * PERT_E_COMM_TIMEOUT / RCCL's error on every rank.  A comm is not usable after a failure. */
typedef struct pert_comm pert_comm;

/* dlopen RCCL from rccl_path (the copy the process already uses -- torch's) and resolve
 * ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy / ncclCommAbort /
 * ncclCommGetAsyncError.  Once per process. */
int pert_comm_load(const char* rccl_path);
/* ncclGetUniqueId into id (n = 128 bytes), on one rank; the caller broadcasts it. */
int pert_comm_unique_id(uint8_t* id, int32_t n);
/* ncclCommInitRank on the current device (collective: returns once every rank has called). */
int pert_comm_init(const uint8_t* id, int32_t n, int32_t world, int32_t rank, pert_comm** out);
/* The host-staged communicator: every rank of one node calls with the same POSIX shm name
 * ("/..."; the segment is unlinked once all ranks have mapped it) and max_n >= the longest
 * all-reduce; returns once every rank has attached or after timeout_s (PERT_E_COMM_TIMEOUT).
 * Each all-reduce is a copy to pinned memory, a host function summing the ranks' blocks in
 * rank order (identical bits on every rank) and a copy back, all queued on the stream. */
int pert_comm_init_host(const char* name, int32_t world, int32_t rank, int64_t max_n, double timeout_s,
                        pert_comm** out);
/* The deadline of every wait (seconds, default 600) and, for an RCCL communicator, a
 * node-local abort word: POSIX shm `abort_name` mapped collectively like pert_comm_init_host's
 * segment (NULL: the word is this process's own, peers then stop by the deadline). */
int pert_comm_set_watchdog(pert_comm* comm, const char* abort_name, double timeout_s);
/* Raise the abort word with `code` and, RCCL, abort the communicator (its queued collectives
 * return).  pert_svi_run_sharded calls it on any failure of its rank. */
int pert_comm_abort(pert_comm* comm, int32_t code);
/* PERT_OK, or the first failure seen by this rank (its own, or a peer's abort). */
int pert_comm_status(pert_comm* comm);
/* Wait for `ev` (recorded on the fit's stream) polling the abort word, RCCL's async error and
 * the deadline; on failure aborts the comm and returns the failure.  eager: poll without
 * sleeping (a wait whose end the caller's latency includes).  comm == NULL: hipEventSynchronize,
 * or with eager a poll. */
int pert_comm_wait_event(pert_comm* comm, hipEvent_t ev, int32_t eager);
/* Test hook: this rank's all-reduce call number `at_call` (0-based, -1 = never) fails at
 * queue time with PERT_E_COMM_FAULT, as a rank's launch failure would. */
int pert_comm_inject_fault(pert_comm* comm, int64_t at_call);
/* overlap (default 0, measured slower on ROCm 7.2: DESIGN.md section 6): pert_svi_run_sharded's
 * three-launch step runs split -- pert_finalize_shared,
 * the all-reduce on the comm's side stream (pert_comm_allreduce_async) while the fit's stream runs
 * pert_finalize_cells, then pert_comm_join + pert_adam; 0: pert_finalize, the all-reduce,
 * pert_adam on one stream.  delay_us > 0 (measurement only): every all-reduce also
 * runs a kernel spinning that long on its stream, a stand-in for an 8-rank ring's latency. */
int pert_comm_set_options(pert_comm* comm, int32_t overlap, double delay_us);
int pert_comm_overlap(const pert_comm* comm);
/* The all-reduce queued on the comm's side stream after the work already queued on `stream`
 * (overlap 0: on `stream` itself); pert_comm_join makes `stream` wait for it. */
int pert_comm_allreduce_async(pert_comm* comm, const double* send, double* recv, int64_t n, hipStream_t stream);
int pert_comm_join(pert_comm* comm, hipStream_t stream);
int pert_comm_destroy(pert_comm* comm);
/* recv = sum over ranks of send (fp64, n elements; send == recv allowed), queued on stream. */
int pert_comm_allreduce_sum_f64(pert_comm* comm, const double* send, double* recv, int64_t n,
                                hipStream_t stream);

/* pert_svi_steps / pert_svi_run of one rank of a sharded fit: each step's reductions write
 * this shard's shared-block sums to grad_local ([n_shared + 1] doubles), pert_comm_allreduce_sum_f64
 * sums them over the ranks into st->grad_shared, then Adam runs on the summed block
 * (pert_enum_step(update_shared = 0) + all-reduce + pert_adam_shared when one_launch; else
 * pass, pert_finalize, all-reduce, pert_adam).  Every rank stops after the same iteration
 * (the loss the rule tests is the all-reduced one) and queues the same number of
 * all-reduces.  Replaces the svi_s.step() loop of pert_model.py:800-816 on a cell shard. */
int pert_svi_steps_sharded(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                           const float* step_size, const float* inv_bc2_sqrt, int32_t iter0, int32_t n,
                           int32_t one_launch, pert_comm* comm, double* grad_local,
                           hipEvent_t* pass_events, hipStream_t stream);
int pert_svi_run_sharded(const pert_problem* prob, pert_state* st, const pert_adam_hparams* hp,
                         const float* step_size, const float* inv_bc2_sqrt, int32_t n_iter, int32_t chunk,
                         int32_t depth, int32_t one_launch, pert_comm* comm, double* grad_local,
                         hipEvent_t* pass_events, double* host_rec, int32_t* n_launched, hipStream_t stream);

/* Diagnostic (bench.py): the HBM streams of pert_enum_pass(PERT_MODE_STEP) -- x, eta code,
 * z/m/v read and written back unchanged, same grid and tile length -- with no arithmetic.
 * Its duration is the access pattern's HBM ceiling on the running device; the state is
 * left bit-identical.  Steps 2/3 shards only. */
int pert_stream_ceiling(const pert_problem* prob, pert_state* st, hipStream_t stream);

/* Posterior marginals of the enumerated latent states at the current parameters (steps 2/3;
 * one pass after a fit, post_kernels.hip).  For every (bin, cell) the posterior over the 2P
 * joint states is gamma(c, r) = softmax_{c,r} s(c, r), s the joint score the passes enumerate
 * (log pi~_c + log Bern(r | phi) + NB'(c (1 + r)); the Dirichlet prior does not enter given pi).
 * Read only: prob->reads [L][ldn], gcf, lamb / log1m_lam, rho_fixed / a_fixed (step 3);
 * st->params with st->lay, st->z_pi in its wave tiles [ldn/64][L][P][64]; st->bins_per_tile
 * (0 = default) sets the bins per wave.  Nothing in st is written.
 *   rep_prob  float [L][ldn]     P(rep = 1) = sum_c gamma(c, 1)                     (required)
 *   cn_state  uint8 [L][ldn]     a CN state per element, e.g. st->cn_out after a decode
 *   cn_prob   float [L][ldn]     the cn marginal gamma(k, 0) + gamma(k, 1) at k = cn_state: the
 *                                probability of the call the caller holds (0 for a state >= P);
 *                                cn_state and cn_prob are given together or both NULL
 *   cn_marg   float [P][L][ldn]  all P cn marginals                                 (or NULL)
 * Columns n >= N of the outputs are left untouched.  No atomics and no cross-lane sums: reruns
 * are bit-identical.  PERT_E_ARG for a null prob, st or rep_prob, a step-1 problem, cn_prob without
 * cn_state (or the reverse), L < 1, N < 1, ldn < N or ldn not a multiple of PERT_BLOCK; then
 * PERT_E_UNSUPPORTED_P / PERT_E_UNSUPPORTED_K for P outside [PERT_MIN_P, PERT_MAX_P] / K1 outside
 * [1, PERT_MAX_K1]; then PERT_E_ARG for a null reads, gcf, st->params or st->z_pi, a null rho_fixed
 * in step 3, or more than 65535 bin tiles (ceil(L / bins_per_tile)); all before any launch. */
int pert_enum_posterior(const pert_problem* prob, const pert_state* st, const uint8_t* cn_state,
                        float* rep_prob, float* cn_prob, float* cn_marg, hipStream_t stream);

/* Posterior draws of the enumerated latent states at the current parameters (steps 2/3,
 * post_kernels.hip): whole-matrix realisations from the posterior gamma(c, r) that
 * pert_enum_posterior gives the marginals of and the decode the argmax of
 * (infer_discrete(temperature=1)).  Reads what pert_enum_posterior reads; nothing in st is written.
 * Per element the weights e(c, r) = exp(s(c, r) - max s) and their inclusive running sums C_j over
 * the joint states in the order j = 2 c + r (cn-major, rep inner) are formed once; S = C_{2P-1}.
 * A draw with uniform u in (0, 1) is the FIRST j with u S < C_j (strict: a state whose weight
 * underflowed to 0 is never drawn); if rounding leaves no such j, the last state with e > 0.
 * Random numbers follow THE COUNTER RULE below with stream tag PERT_TAG_DRAWS: draw g (global
 * index first_draw + d) of (bin l, global cell cell0 + n) takes word g & 3 of
 *   philox(counter = {l, low word of the cell index, g >> 2, high word of the cell index})
 * so one Philox call serves four consecutive draws and a draw depends only on (seed, bin, global
 * cell, g): not on the grid, the tile size, how first_draw / n_draws chunk the draws or which cells
 * a launch holds.  The uniform is ((w >> 8) + 0.5) 2^-24 rounded to fp32 and kept below 1.
 *   rep_draw  uint8 [n_draws][L][ldn]  rep = j & 1 of draw first_draw + d in plane d   (required)
 *   cn_draw   uint8 [n_draws][L][ldn]  cn = j >> 1                                     (or NULL)
 * Each plane is a contiguous [L][ldn] matrix in the decode's encodings.  Columns n >= N are left
 * untouched.  No atomics, no cross-lane sums: reruns are bit-identical.  Argument checks, all
 * before any launch: pert_enum_posterior's, in its order (a null rep_draw for its null rep_prob);
 * then PERT_E_ARG for n_draws outside [1, PERT_MAX_DRAWS], first_draw < 0, first_draw + n_draws
 * above INT32_MAX or cell0 < 0; then for more than 65535 bin tiles. */
#define PERT_TAG_DRAWS 3u
#define PERT_MAX_DRAWS 4096
int pert_enum_draw(const pert_problem* prob, const pert_state* st, uint64_t seed, int64_t cell0,
                   int32_t first_draw, int32_t n_draws, uint8_t* rep_draw, uint8_t* cn_draw, hipStream_t stream);

/* Per-cell likelihood curves over S-phase time tau at the current parameters (steps 2/3,
 * curve_kernels.hip).  tau enters an element's 2P joint scores through the Bernoulli term alone, so
 * with everything but tau held fixed the log marginal of (bin l, cell n) at any tau is
 *   m_ln(tau) = log((1 - phi) exp(e_0) + phi exp(e_1)),
 *   phi = clamp(1 / (1 + exp(-a (tau - rho_l))), 0.001, 0.999),
 *   e_r = log sum_c exp(log pi~_c + NB'(x ; c (1 + r))),  r = 0, 1    (the branch evidences:
 *         pert_enum_posterior's scores without the Bernoulli term, the same omitted kappa(x)).
 *
 * pert_enum_evidence writes the branch evidences, fp32:
 *   ev  float [2][L][ldn]  plane 0 = e_0, plane 1 = e_1
 * It reads what pert_enum_posterior reads, in its launch shape (st->bins_per_tile bins per wave),
 * and writes nothing of st.  Columns n >= N of ev are left untouched.  No atomics, no cross-lane
 * sums: reruns are bit-identical.  Argument checks, all before any launch: pert_enum_posterior's,
 * in its order (a null ev for its null rep_prob; there is no cn_state / cn_prob pair).
 *
 * pert_tau_curve sums the element marginals over the bins, per cell and grid point:
 *   grid    float  [G]     values of tau strictly inside (0, 1), ascending (device memory: the
 *                          caller validates them)
 *   curve   double [G][N]  curve[g][n] = sum_l m_ln(grid[g])
 *   at_fit  double [N]     sum_l m_ln(tau_n) at the cell's own fitted tau (clipped sigmoid of its
 *                          parameter, as the passes form it)
 * rho and a are the fit's (rho_fixed / a_fixed in step 3).  m is fp32 (pert_math.h tau_mix); the sum
 * over bins is fp64 and taken in bin order l = 0 .. L-1 for every (g, n), so the result does not
 * depend on the launch geometry or on how a caller chunks the grid (any split of the grid into
 * calls gives the bits of one call).  No atomics, no workspace, nothing allocated; reruns are
 * bit-identical; nothing of st is written.  PERT_E_ARG, before any launch, for a null argument, a
 * step-1 problem, G outside [1, PERT_TAU_MAX_GRID], L < 1, N < 1, ldn < N or ldn not a multiple of
 * PERT_BLOCK, a null st->params, or a null rho_fixed in step 3. */
#define PERT_TAU_MAX_GRID 1024
int pert_enum_evidence(const pert_problem* prob, const pert_state* st, float* ev, hipStream_t stream);
int pert_tau_curve(const pert_problem* prob, const pert_state* st, const float* ev, const float* grid, int32_t G,
                   double* curve, double* at_fit, hipStream_t stream);

/* tau initialiser (guess_times, pert_model.py:426-457): the batched pass of
 * manhattan_binarization (:364-423) for every cell in ONE launch, in fp64 -- standardisation,
 * GaussianMixture(n_components=2, random_state=0) (k-means++ and Lloyd initialisation, then EM),
 * the levels (GMM means, or percentiles chosen by the skew), the 100-threshold Manhattan scan --
 * twice per cell: run 0 breaks exact ties on a k-means decision towards centre 1, run 1 towards
 * centre 0.  Decisions that fp32 rounding (the reference's arithmetic) could flip are reported
 * in flags, so the caller recomputes those cells exactly (tau_init.exact_fractions). */
typedef struct {
  int32_t first;                   /* k-means++ first centre index (RandomState(0) draw) */
  int32_t lloyd_max_iter;          /* 300 (KMeans default) */
  int32_t em_max_iter;             /* 100 (GaussianMixture default) */
  int32_t q_lo[5], q_hi[5];        /* np.percentile 'linear' at q = .05 .25 .5 .75 .95: floor(q (L-1)), +1 (<= L-1) */
  int32_t pad_;
  double q_t[5];                   /* q (L-1) - floor(q (L-1)) */
  double u[2];                     /* the two local-trial uniforms of k-means++ */
  double tie;                      /* relative width of an exact tie on a k-means decision */
  double pp_margin;                /* k-means++ draw / choice margin, relative to the potential */
  double fragile;                  /* Lloyd shift-vs-tol margin, relative to tol */
  double em_margin;                /* EM |lower-bound change| vs tol margin, absolute */
  double em_tol;                   /* 1e-3 */
  double reg_covar;                /* 1e-6 */
  double mean_gap;                 /* 0.7  (MEAN_GAP_THRESH) */
  double early_skew, late_skew;    /* 0.2, -0.2 */
  double fragile_abs;              /* margin of the mean-gap / skew thresholds, absolute */
  double level_margin;             /* relative rounding budget of the scan levels (1e-6 sqrt(L)) */
  double eps32;                    /* float32 eps: the reference's summation noise in the scan */
} pert_tau_params;

/* norm: float [N][L] CN-normalised reads, one contiguous row per cell (device).
 * Outputs (device), per run r (0: ties to centre 1, 1: ties to centre 0) and cell n:
 *   labels  int8 [2][N][L]  final k-means labels (1 = centre 1)
 *   scratch int8 [2][N][L]  workspace
 *   means   double [2][N][2] GMM means
 *   flags   int32 [2][N]    bit 0: a Lloyd / EM stopping decision or the mean-gap / skew test
 *                           within its margin; bit 1: a k-means++ draw within its margin whose
 *                           alternatives end in other labels; bit 2: the scan's minimum within
 *                           its rounding slack of another threshold's
 *   frac    double [2][N]   replicated fraction (the reference's t_init where no flag is set)
 *   minor   double [2][N]   points within the levels' rounding budget of the chosen threshold */
int pert_tau_binarize(int32_t L, int32_t N, const float* norm, const pert_tau_params* p,
                      int8_t* labels, int8_t* scratch, double* means, int32_t* flags, double* frac,
                      double* minor, hipStream_t stream);

/* Threshold binarisation of RT profiles (Dileep & Gilbert; binarize_rt_profiles.py:44-117) for
 * every cell of one length in ONE launch, one workgroup per cell, in fp64, on the raw
 * (unstandardised) profile: GaussianMixture(n_components=2, random_state=0) as sklearn runs it on
 * float64 data (KMeans tolerance, centring, k-means++, Lloyd, EM, fit_predict's final E step), the
 * levels (GMM means, or percentiles chosen by the biased skew), and the scan of the 100 fixed
 * thresholds for the first least Manhattan distance.  Every sum is a fixed-order block sum, so
 * reruns are bit-identical.  The margins are those of an fp64-vs-fp64 comparison (another
 * summation order); a decision within its margin sets a bit of flags and the caller recomputes
 * that cell on the host (binarize.py). */
#define PERT_BIN_THRESHOLDS 100
typedef struct {
  int32_t first;                   /* k-means++ first centre index (RandomState(0) draw at this L) */
  int32_t lloyd_max_iter;          /* 300 */
  int32_t em_max_iter;             /* 100 */
  int32_t q_lo[5], q_hi[5];        /* np.percentile 'linear' at q = .05 .25 .5 .75 .95 */
  int32_t pad_;
  double q_t[5];
  double u[2];                     /* the two local-trial uniforms of k-means++ */
  double em_tol;                   /* 1e-3 */
  double reg_covar;                /* 1e-6 */
  double mean_gap;                 /* MEAN_GAP_THRESH */
  double early_skew, late_skew;    /* EARLY_S_SKEW_THRESH, LATE_S_SKEW_THRESH */
  double thresh[PERT_BIN_THRESHOLDS];  /* np.linspace(-3, 3, 100), the caller's bits */
  /* margins */
  double pp_margin;                /* k-means++ draw / choice, relative to the potential */
  double tie_margin;               /* a Lloyd assignment on the decision boundary, relative */
  double lloyd_margin;             /* Lloyd centre shift vs tol, relative to tol */
  double em_margin;                /* EM |lower-bound change| vs em_tol, absolute */
  double gap_margin;               /* |mean gap - mean_gap|, relative to max(1, |mu0| + |mu1|) */
  double skew_margin;              /* skew vs its thresholds, absolute */
  double resp_margin;              /* final E step's two log responsibilities, relative to 1 + |l0| + |l1| */
  double thresh_margin;            /* |x - chosen threshold|, absolute */
  double dist_margin;              /* another threshold's distance vs the least, relative to least + L max|level| */
} pert_bin_params;

#define PERT_BIN_F_PP 1        /* k-means++ draw or choice */
#define PERT_BIN_F_LLOYD 2     /* Lloyd: shift-vs-tol test, or a point on the assignment boundary */
#define PERT_BIN_F_EM 4        /* EM stopping test */
#define PERT_BIN_F_LEVELS 8    /* mean-gap or skew test */
#define PERT_BIN_F_RESP 16     /* a gmm_state whose two responsibilities are within margin */
#define PERT_BIN_F_POINT 32    /* a point within margin of the chosen threshold */
#define PERT_BIN_F_SCAN 64     /* a threshold that binarises differently, its distance within margin of the least */

/* x: double [N][L], one contiguous row per cell (device).  Outputs (device, the caller's):
 *   means, covs double [N][2]   GMM means and variances (reg_covar included), sklearn's component
 *                               order (component 0 grew from the k-means++ first centre), unsorted
 *   gmm_state int8 [N][L]       argmax of the final E step (also the Lloyd label workspace)
 *   rt_state  uint8 [N][L]      x > chosen threshold (also Lloyd's previous-label workspace)
 *   dist double [N][100]        Manhattan distance per threshold
 *   best int32 [N]              index of the chosen threshold (first strict minimum)
 *   n_rep int32 [N]             replicated bins
 *   flags int32 [N]             PERT_BIN_F_* bits
 * PERT_E_ARG for L < 2, N < 1, a null buffer or percentile / first-centre indices outside [0, L).
 * Allocates nothing. */
int pert_rt_binarize(int32_t L, int32_t N, const double* x, const pert_bin_params* p, double* means,
                     double* covs, int8_t* gmm_state, uint8_t* rt_state, double* dist, int32_t* best,
                     int32_t* n_rep, int32_t* flags, hipStream_t stream);

/* The cell-cycle-classifier features of compute_ccc_features.py:18-56 for every cell of one length
 * in ONE launch, one workgroup per cell, in fp64 (ccc_features.py):
 *   score1  GaussianMixture(n_components=1).fit(x).score(x): mean = sum x / (L + 10 eps),
 *           var = sum (x - mean)^2 / (L + 10 eps) + reg_covar, the mean log density
 *   score2  GaussianMixture(n_components=2): KMeans tolerance, centring, k-means++ from this cell's
 *           own draws, Lloyd, EM, then the mean log probability under the FINAL parameters
 *   lrs     -2 (score1 - score2)
 *   madn    median |x[i+1] - x[i]| over the L - 1 adjacent pairs in row order (radix select: the
 *           order statistics themselves, (a + b) / 2 for an even count: np.median's bits)
 *   breakpoints  # i with state[i] != state[i-1] and chrom[i] == chrom[i-1]
 * Every sum is a fixed-order block sum, so reruns are bit-identical.
 *
 * The random stream: the reference fits with random_state=None, so each cell consumes 4 doubles
 * of numpy's global generator in sorted-cell order: d0 -> first1 (the 1-component k-means++
 * choice; unused by the arithmetic, carried so the ABI documents the stream), d1 -> first2 (the
 * 2-component choice: searchsorted(cdf of L equal weights, d1, 'right')), d2, d3 -> u (the two
 * local-trial uniforms).  The caller draws them and passes them per cell. */
typedef struct {
  int32_t lloyd_max_iter;          /* 300 */
  int32_t em_max_iter;             /* 100 */
  double em_tol;                   /* 1e-3 */
  double reg_covar;                /* 1e-6 */
  /* margins, with the meaning of pert_bin_params' */
  double pp_margin;
  double tie_margin;
  double lloyd_margin;
  double em_margin;
} pert_ccc_params;

/* x: double [N][L], one contiguous row per cell in that cell's own row order (device).
 * first1, first2: int32 [N]; u: double [N][2].  state, chrom: int32 [N][L], or both null (no
 * breakpoints: zeros are written).  scratch: int8 [2][N][L] (Lloyd's labels).  Outputs (device,
 * the caller's): score1, score2, lrs, madn double [N]; breakpoints int32 [N]; flags int32 [N]:
 * PERT_BIN_F_PP / PERT_BIN_F_LLOYD / PERT_BIN_F_EM (the caller recomputes a flagged cell's scores
 * on the host; madn and breakpoints are exact either way).
 * PERT_E_ARG for L < 2, N < 1, a null required buffer, exactly one of state / chrom null, or an
 * iteration count < 1.  Allocates nothing. */
int pert_ccc_features(int32_t L, int32_t N, const double* x, const int32_t* first1, const int32_t* first2,
                      const double* u, const int32_t* state, const int32_t* chrom, const pert_ccc_params* p,
                      int8_t* scratch, double* score1, double* score2, double* lrs, double* madn,
                      int32_t* breakpoints, int32_t* flags, hipStream_t stream);

/* ---- The bulk G1 GC correction's LOWESS curve (gc_correction.py; reference
 * bulk_gc_correction.py:60-72: statsmodels' lowess(rpm, gc, xvals=...) with delta = 0) over the
 * C * L points (x = ux[inv[l]], y[c][l]) of a matrix whose x is a property of the column.
 *   y    double [C][L], device: one contiguous row per cell.  A non-finite y is no point.
 *   inv  int32 [L], HOST: the distinct-x index of each bin, in [0, U)
 *   ux   double [U], HOST: the distinct x, finite and strictly increasing
 *   xv   double [M], HOST: the finite x the curve is evaluated at
 * The host arrays are checked, then uploaded into the workspace on `stream`; they must stay valid
 * until the stream has passed the call.  k = int(frac * n + 1e-10) is the caller's, n the number
 * of finite points: the bandwidth of a fit at x0 is the k-th smallest |x - x0| over the points,
 * the weights are tricube times the bisquare robustness weights of `it` earlier rounds (the
 * median of the absolute residuals is exact: np.median's), and the fit is the weighted local line
 * at x0 (the weighted mean when the window holds one distinct x).  A fit whose bandwidth is 0 or
 * whose window carries zero weights only is NaN; when that happens to a fit at a data x of a
 * robustness round, its points' residuals are NaN, so is their median (np.median's propagation) and
 * the whole curve is NaN.  k must not exceed the number of finite points (only the caller knows
 * it before the first pass): a larger k has no k-th neighbour and every fit is NaN.
 * out: double [M], device.
 * All of it is fp64 with fixed-order sums and integer atomics only: two runs agree bit for bit.
 * Every launch of the it + 1 rounds and of the final evaluation is queued on `stream`; nothing
 * is read back.  workspace: device, 16-byte aligned, at least pert_lowess_workspace() bytes,
 * contents arbitrary.  PERT_E_ARG, before any launch or copy, for a null argument, C, L, U or M
 * < 1 (M = 0 is allowed in the workspace query: pert_lowess_absmed's), U > L, C > 32 * 65,535
 * (the sums pass's chunks of 32 cells are one grid dimension), C * L >= 2^31, an
 * inv outside [0, U), ux not finite and increasing, xv not finite, k outside [1, C * L], it < 0,
 * a misaligned or short workspace. */
int pert_lowess_workspace(int32_t C, int32_t L, int32_t U, int32_t M, int64_t* bytes);
int pert_lowess_curve(int32_t C, int32_t L, int32_t U, int32_t M, const double* y, const int32_t* inv,
                      const double* ux, const double* xv, int64_t k, int32_t it, double* out, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream);
/* The curve's exact median on its own: med[0], med[1] (device) = the two middle order statistics
 * (ranks (n - 1) / 2 and n / 2, equal for odd n) of |y[c][l] - fit[inv[l]]| over the finite y, by a
 * radix select on the values' bit patterns; *n_out (device int64, or null) = n.  Without a finite
 * y, or with a NaN residual (a NaN fit under a finite y), both are NaN.  fit: double [U], device.  Arguments as
 * above. */
int pert_lowess_absmed(int32_t C, int32_t L, int32_t U, const double* y, const int32_t* inv, const double* fit,
                       double* med, int64_t* n_out, void* workspace, int64_t workspace_bytes,
                       hipStream_t stream);

/* ---- The cell level's change-point search (normalize_cell.py; reference normalize_by_cell.py:45-46
 * and :73-74: ruptures' KernelCPD(kernel='linear', min_size=2).predict(n_bkps = 2 or 1)), for N
 * profiles at once.  For a profile Y[0..n): S[0] = 0, S[i] = S[i-1] + Y[i-1] added in bin order,
 * rinv[k] = 1.0 / k correctly rounded, and
 *   mode 2:  G(a, b) = (S[a] S[a]) rinv[a] + ((S[b] - S[a]) (S[b] - S[a])) rinv[b - a]
 *                      + ((S[n] - S[b]) (S[n] - S[b])) rinv[n - b]   over 2 <= a, a + 2 <= b <= n - 2
 *   mode 1:  G(a) = (S[a] S[a]) rinv[a] + ((S[n] - S[a]) (S[n] - S[a])) rinv[n - a]   over 2 <= a <= n - 2
 * each operation one IEEE fp64 operation, the terms added left to right, nothing fused.  The
 * largest G wins; a tie goes to the smallest a, then the smallest b.
 *   y       double [N][ld], device: one row per cell, its first len[c] entries the profile (finite)
 *   len     int32 [N], HOST: 0 <= len[c] <= ld
 *   mode    int32 [N], HOST: 1 or 2 breakpoints
 *   active  int32 [N], HOST: 1 = searched, 0 = skipped (the cell's outputs are left as they are)
 *   a, b    int32 [N], device: the breakpoints ([a, b, n] of ruptures; b = len[c] in mode 1);
 *           a = b = -1 when the search is infeasible (len < 6 in mode 2, < 4 in mode 1)
 *   gain    double [N], device: the winning G (0 when infeasible)
 * The host arrays are checked, then uploaded into the workspace on `stream`; they must stay valid
 * until the stream has passed the call.  Three launches (prefix sums, the search over cells x tiles
 * of a with S and rinv in LDS, the per-cell reduction of the tiles' winners by (gain, -a, -b)); no
 * atomics, so the result does not depend on the tiling and two runs agree bit for bit.  ld is at
 * most PERT_CPD_MAX_N: the two tables of the longest cell, 16 (len + 1) bytes, and 256 bytes of
 * winners must fit gfx950's 160 KiB of LDS.  workspace: device, 16-byte aligned, at least
 * pert_cpd_workspace() bytes, contents arbitrary.  PERT_E_ARG, before any launch or copy, for a
 * null argument, N < 1 or > 65,535 (cells are one grid dimension), ld < 1 or > PERT_CPD_MAX_N, a
 * len outside [0, ld], a mode other than 1 or 2, an active other than 0 or 1, a misaligned y or
 * workspace, a short workspace.  Allocates nothing. */
#define PERT_CPD_MAX_N 10000
int pert_cpd_workspace(int32_t N, int32_t ld, int64_t* bytes);
int pert_cpd_search(int32_t N, int32_t ld, const double* y, const int32_t* len, const int32_t* mode,
                    const int32_t* active, int32_t* a, int32_t* b, double* gain, void* workspace,
                    int64_t workspace_bytes, hipStream_t stream);

/* ---- Downstream replication-timing analyses (rt_profiles.py) on the decode's rep_out.
 * rep is uint8 [L][ldn] (0 / 1 per (bin, cell); ldn >= N a multiple of 16, the base 16-byte
 * aligned; columns n >= N hold undefined bytes and are never counted).  group is int32 [N]: the
 * pseudobulk row (clone) of each cell in [0, G), anything else = excluded.  Outputs are ADDED
 * to (integer adds only: exact, identical from run to run); the caller zeroes them. */
#define PERT_RT_MAX_GROUPS 32   /* pert_rt_tfs_hist: a tile's hours rows of every group sit in LDS */
#define PERT_RT_MAX_EDGES 257

/* bin_count uint32 [G][L]: replicated cells per bin and group (the numerators of
 * compute_pseudobulk_rt_profiles.py:18-19 per clone; their sum over groups is the population's).
 * cell_count uint32 [N]: replicated bins per cell, excluded cells included (the numerator of
 * compute_cell_frac, predict_cycle_phase.py:33-38). */
int pert_rt_counts(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep, const int32_t* group,
                   uint32_t* bin_count, uint32_t* cell_count, hipStream_t stream);

/* calc_pct_replicated_per_time_bin (calculate_twidth.py:37-71) as counts.  hours [G][L], f10 [N]
 * and the ascending edges [n_edges <= PERT_RT_MAX_EDGES] are float, or double when is_f64.  For
 * every bin l and cell n < N with g = group[n] in [0, G): t = hours[g][l] - f10[n] (one
 * subtraction in that type); the interval i with edges[i] <= t < edges[i+1] is found by
 * comparisons against the edges alone; hist_n[i] += 1, hist_rep[i] += rep[l][n].  A t that is
 * NaN or outside the edges counts nowhere.  per_cell 0: hist_n / hist_rep are uint32
 * [n_edges - 1]; per_cell 1 or 2: uint32 [N][n_edges - 1] (1: a 64-cell tile of histograms in
 * LDS per workgroup, the product path; 2: adds straight to global memory, kept for
 * measurement; same results).  PERT_E_ARG when L * N >= 2^32 (a counter could wrap). */
int pert_rt_tfs_hist(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep, const int32_t* group,
                     const void* hours, const void* f10, const void* edges, int32_t n_edges, int32_t is_f64,
                     int32_t per_cell, uint32_t* hist_n, uint32_t* hist_rep, hipStream_t stream);

/* ---- Cell bootstrap (cell_bootstrap.py): the two passes above for many resampled sets of cells at
 * once.  A replicate is a weight per cell, w uint8 [rows][ldw] (how often the resampling picked the
 * cell; ldw >= N a multiple of 16, the base 16-byte aligned, columns n >= N undefined and never
 * counted).  rep follows the pert_rt_* conventions.  Integer adds only: results are exact, do not
 * depend on the launch shape and repeat bit for bit.  Outputs are ADDED to; the caller zeroes them.
 * PERT_E_ARG, before any launch, for a null or misaligned argument or a size outside the limits
 * named below; nothing is written then. */
#define PERT_TAG_BOOT 4u             /* the resampler's stream tag of THE COUNTER RULE (below) */
#define PERT_BOOT_MAX_LAUNCH 65535   /* replicates of one pert_boot_weights call */

/* The stratified resampler, replicates b0 .. b0 + Bc - 1.  Positions j = 0 .. N - 1 run over the
 * cells sorted stably by stratum: order int32 [N] is the cell at each position, pos_lo / pos_n int32
 * [N] the first position and the size of position j's stratum.  Draw (b, j) takes the 64-bit word
 * (word 1 << 32 | word 0) of
 *   philox(counter = {j, low half of b, PERT_TAG_BOOT, high half of b}, key of (seed, PERT_TAG_BOOT))
 * and picks cell order[pos_lo[j] + mulhi64(word, pos_n[j])]; w[b - b0][n] = the number of draws of b
 * that picked n, columns [N, ldw) zero.  No rejection loop; a draw depends only on seed, b, j and the
 * stratum layout.  scratch uint32 [Bc][N] holds the counts before they are narrowed: zeroed by the
 * caller, ADDED to.  *flag (uint32, zeroed by the caller) gets bit 0 when a count exceeds 255 (stored
 * as 255) and bit 1 when pos_lo / pos_n / order do not describe strata of [0, N) (that draw is
 * dropped).  Bc <= PERT_BOOT_MAX_LAUNCH. */
int pert_boot_weights(int32_t N, int32_t ldw, const int32_t* pos_lo, const int32_t* pos_n, const int32_t* order,
                      uint64_t seed, int64_t b0, int32_t Bc, uint32_t* scratch, uint8_t* w, uint32_t* flag,
                      hipStream_t stream);

/* count uint32 [C][L]: count[c][l] += sum_{n < N} wg[c][n] rep[l][n] for C weight rows, one per
 * (replicate, group) and already masked by group (v_dot4_u32_u8 into 32-bit sums; an 8 x 8 tile of
 * (weight row, bin) sums per lane, so a loaded rep fragment serves 8 weight rows and a weight
 * fragment 8 bins).  N < 2^32 / 255 and L <= 8 * 65535. */
int pert_boot_counts(int32_t L, int32_t N, int32_t ldn, const uint8_t* rep, int32_t C, int32_t ldw,
                     const uint8_t* wg, uint32_t* count, hipStream_t stream);

/* pert_rt_tfs_hist (per_cell 0) per group, for Bc replicates in one launch: hours is [Bc][G][L],
 * f10 [N] and the edges as there; w uint8 [Bc][ldw] the replicates' weights (not masked: group does
 * that).  For every replicate b, bin l and cell n < N with g = group[n] in [0, G) and w[b][n] > 0:
 * t = hours[b][g][l] - f10[n], its interval i found by the routine of pert_rt_tfs_hist;
 * hist_n[b][g][i] += w[b][n], and hist_rep[b][g][i] += w[b][n] where rep[l][n] is non-zero.
 * hist_n / hist_rep are uint32 [Bc][G][n_edges - 1].  A workgroup reads its tile of rep once and
 * walks the replicates over it.  G <= PERT_RT_MAX_GROUPS and n_edges <= PERT_RT_MAX_EDGES; the
 * caller keeps L * sum_n w[b][n] < 2^32 for every b (a counter could wrap). */
int pert_boot_tfs_hist(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep, const int32_t* group,
                       int32_t Bc, int32_t ldw, const uint8_t* w, const void* hours, const void* f10,
                       const void* edges, int32_t n_edges, int32_t is_f64, uint32_t* hist_n, uint32_t* hist_rep,
                       hipStream_t stream);

/* ---- Per-cell quality features of the phase calls (phase_matrix.py; reference
 * predict_cycle_phase.py:23-88) on the decode's state matrices and the shard's reads, in place.
 * The series of cell n is column n of the matrix in row order, t = 0 .. L - 1; the lags are
 * k = 1 .. max_lag <= PERT_PHASE_MAX_LAG (the reference: 50, averaging lags 9..50).  Matrices follow
 * the pert_rt_* conventions: rows ldn elements apart, ldn >= N a multiple of 16, the base 16-byte
 * aligned, columns n >= N undefined and never read.  Both entry points return PERT_E_ARG for a null
 * or misaligned argument, N < 1, max_lag outside [1, PERT_PHASE_MAX_LAG], L <= max_lag, or L >= 2^20
 * (the host's n^3 integer arithmetic stays inside int64).  They allocate nothing. */
#define PERT_PHASE_MAX_LAG 64

/* The integer counts.  rep (and cn, or null: then cn_bk / cn0 are not touched and may be null) are
 * uint8 [n_planes][L][ldn], the planes plane_stride bytes apart (a multiple of 16, >= L * ldn; not
 * read when n_planes = 1): the layout of draw_states.  rep counts as replicated where non-zero.
 * Outputs are uint32 with a leading plane axis and are ADDED to (register sums, then integer
 * atomics: exact, identical from run to run); the caller zeroes them.
 *   rep_sum [planes][N]            T = sum_t x_t
 *   rep_bk, cn_bk [planes][N]      # t with a change between t and t + 1
 *   cn0 [planes][N]                # t with cn = 0
 *   rep_lag [planes][max_lag][N]   S_k = #{t < L - k : x_t = x_{t+k} = 1}, row k - 1
 *   rep_head, rep_tail [planes][max_lag][N]   the sum of the first k and of the last k states
 * The bins are cut into chunks of whole 64-bin words (>= 2 words; about 1024 waves in all); a chunk
 * reads the word before its first as the halo. */
int pert_phase_counts(int32_t L, int32_t N, int32_t ldn, int32_t n_planes, int64_t plane_stride,
                      const uint8_t* rep, const uint8_t* cn, int32_t max_lag, uint32_t* rep_sum,
                      uint32_t* rep_bk, uint32_t* cn_bk, uint32_t* cn0, uint32_t* rep_lag, uint32_t* rep_head,
                      uint32_t* rep_tail, hipStream_t stream);

/* The float series (the reads): x is float [L][ldn], or double when is_f64.  Outputs fp64 (device):
 * mean [N], and c [max_lag + 1][N] with c_k = sum_{t < L - k} (x_t - m)(x_{t+k} - m).  Two passes
 * inside the call (the mean, then the centred products; no raw moments), fp64 throughout, no
 * floating-point atomics: per-chunk partials in the workspace are added in chunk order, so two runs
 * agree bit for bit.  A NaN or Inf in a cell's series makes that cell's outputs NaN and no other's.
 * workspace: device, 8-byte aligned, at least pert_phase_acf_workspace() bytes
 * (= 8 * n_chunks * (max_lag + 2) * N); its contents need not be initialised. */
int pert_phase_acf_workspace(int32_t L, int32_t N, int32_t max_lag, int64_t* bytes);
int pert_phase_acf(int32_t L, int32_t N, int32_t ldn, const void* x, int32_t is_f64, int32_t max_lag,
                   double* mean, double* c, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- Read-count simulator (pert_simulator.py; reference pert_simulator.py:38-282): the
 * generative model run forwards, one Bernoulli and one negative-binomial draw per (bin, cell).
 *
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 / 0xBB67AE85), counter based.  THE COUNTER RULE: the words of a draw are
 *   philox(counter = {bin index, low word of the global cell index, draw round,
 *                     high word of the global cell index},
 *          key     = {low word of seed, high word of seed ^ (stream tag * 0x9E3779B9)})
 * so a draw depends only on the seed and on the element it belongs to (global cell index =
 * cell0 + column), never on the grid, the tile size or which cells a launch holds: cells
 * simulated in several launches (cell0) get the numbers one launch over all of them gives.
 * A uniform is ((w >> 8) + 0.5) 2^-24 rounded to fp32 and kept below 1 (the one value that
 * rounds to 1.0 becomes 1 - 2^-24): strictly inside (0, 1).
 * (Tags 1 and 2 are the simulator's streams; 3 is PERT_TAG_DRAWS, pert_enum_draw; 4 is
 * PERT_TAG_BOOT, pert_boot_weights, whose counter also carries the tag in the draw-round word.)
 * Stream PERT_SIM_TAG_CELLS (bin index 0): draw round 0 word 0 -> tau; draw round 1 + k words
 * 0, 1 -> beta k = mean + std sqrt(-2 ln u1) cos(2 pi u2), with u = ((w >> 8) + 0.5) 2^-24 and
 * the arithmetic in fp64, rounded to fp32 once.
 * Stream PERT_SIM_TAG_READS: draw round 0 word 0 -> the Bernoulli uniform (rep = u < phi);
 * draw round j < 64 words 1, 2, 3 -> attempt j of the Gamma sampler (Box-Muller pair,
 * acceptance uniform); draw round 64 + j words 0, 1 -> attempt j of the Poisson sampler (word 0
 * of round 64 alone for inversion, rate < 10).  Rejection loops run at most 64 rounds; a lane
 * that uses them up takes the rounded mean and adds 1 to `exhausted` (expected: never). */
#define PERT_SIM_TAG_CELLS 1u
#define PERT_SIM_TAG_READS 2u

/* Test hook of the generator: out[i] (uint32 [n][4], 16-byte aligned, device) = the four words
 * of the counter (c0, c1, c2, c3) + i, taken as a 128-bit integer with c0 lowest, under key
 * (key0, key1).  1 <= n <= 2^31. */
int pert_sim_raw(uint32_t key0, uint32_t key1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int64_t n,
                 uint32_t* out, hipStream_t stream);

/* Per-cell draws of global cells [cell0, cell0 + N): tau float [N] ~ U(0, 1) (Beta(1, 1),
 * pert_simulator.py:77; NULL: not drawn, G1/2 cells) and betas float [K1][N] (the fit's plane
 * layout) ~ Normal(beta_means[libs[n]][k], beta_stds[libs[n]][k]) (:83); beta_means / beta_stds
 * float [n_libs][K1], libs int32 [N]. */
int pert_sim_cells(int32_t N, int32_t K1, int32_t n_libs, int64_t cell0, uint64_t seed, const int32_t* libs,
                   const float* beta_means, const float* beta_stds, float* tau, float* betas, hipStream_t stream);

/* The fused pass over [L][ldn] (ldn as in pert_problem) for global cells [cell0, cell0 + N)
 * (pert_simulator.py:98-124): omega = exp(sum_k betas[k][n] gc[l]^(K - k)),
 * phi = 1 / (1 + exp(-a (tau[n] - rho[l]))), rep ~ Bernoulli(phi), chi = cn (1 + rep),
 * delta = max(u chi omega (1 - lamb) / lamb, 1), reads ~ NegativeBinomial(delta, probs = lamb)
 * drawn as Poisson(Gamma(delta, scale = lamb / (1 - lamb))).  tau == NULL: the G1/2 model,
 * rep = 0 (model_g1, :151-172; rho unused).  cn float [L][ldn], gc / rho float [L], betas float
 * [K1][N].  Outputs: counts uint32 [L][ldn] (saturating), rep uint8 [L][ldn], p_rep float
 * [L][ldn] = phi (NULL: skipped), all with columns [N, ldn) written as zero; colsum uint64 [N]
 * and the word *exhausted are ADDED to by integer atomics (exact, order independent): the
 * caller zeroes them.  Arithmetic is fp32: rates above 2^24 lose integer resolution. */
int pert_sim_reads(int32_t L, int32_t N, int32_t ldn, int32_t K1, int64_t cell0, uint64_t seed, const float* cn,
                   const float* gc, const float* rho, const float* tau, const float* betas, float u, float a,
                   float lamb, uint32_t* counts, uint8_t* rep, float* p_rep, uint64_t* colsum, uint32_t* exhausted,
                   hipStream_t stream);

/* reads_norm float [L][ldn] = int64(counts / colsum * num_reads), the three operations in fp64
 * (pert_simulator.py:245-247 on float64 tensors) -- the layout and type pert_problem.reads
 * takes.  Columns [N, ldn), and a cell whose colsum is 0, are written as zero.  PERT_E_ARG for
 * num_reads >= 2^24: the fp32 copy would no longer be exact. */
int pert_sim_normalise(int32_t L, int32_t N, int32_t ldn, double num_reads, const uint32_t* counts,
                       const uint64_t* colsum, float* reads_norm, hipStream_t stream);

/* Test-only entry points: the per-(bin, cell) arithmetic of pert_math.h evaluated on
 * the host (no GPU needed) or on the device, for the parity suite.  Not used by any
 * product path. */
int pert_selftest_nb_lgdiff_host(int64_t n, const float* d, const float* x, float* lam, float* psi);
int pert_selftest_nb_lgdiff_device(int64_t n, const float* d, const float* x, float* lam, float* psi,
                                   hipStream_t stream);
int pert_selftest_enum_cellbin_host(int32_t P, int64_t n, const float* x, const float* em1,
                                    const float* S1, const float* z, float log1m_lam,
                                    const float* D, const float* phi, float* E, float* dirv,
                                    float* gD, float* gt, float* gz, int32_t* argmax);
/* The three-wave pass's per-element arithmetic (enum_online + the tail's logit gradient with
 * the argmax logit in jmax form) on the host: E and d(E + dirv)/dz. */
int pert_selftest_enum_online_host(int32_t P, int64_t n, const float* x, const float* em1,
                                   const float* S1, const float* z, float log1m_lam, const float* D,
                                   const float* phi, float* E, float* gz);
/* pert_enum_posterior's per-element arithmetic (pert_math.h enum_posterior) on the host:
 * x, D, phi float [n], z float [n][P] -> p_rep float [n], p_cn float [n][P]. */
int pert_selftest_enum_posterior_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                      const float* D, const float* phi, float* p_rep, float* p_cn /* [n][P] */);
/* pert_enum_draw's per-element arithmetic (pert_math.h enum_draw_cdf / enum_draw_pick) on the host:
 * x, D, phi float [n], z float [n][P], u float [n][n_draws] in (0, 1) -> cn, rep uint8 [n][n_draws]. */
int pert_selftest_enum_draw_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                 const float* D, const float* phi, int32_t n_draws, const float* u /* [n][n_draws] */,
                                 uint8_t* cn, uint8_t* rep);
/* The likelihood curve's per-element arithmetic on the host (pert_math.h enum_evidence / tau_mix):
 * x, D float [n], z float [n][P] -> ev0, ev1 float [n];  ev0, ev1, phi (unclamped) float [n] -> m float [n]. */
int pert_selftest_enum_evidence_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                     const float* D, float* ev0, float* ev1);
int pert_selftest_tau_mix_host(int64_t n, const float* ev0, const float* ev1, const float* phi, float* m);

const char* pert_version(void);

#ifdef __cplusplus
}
#endif

#endif /* PERT_HIP_H */
