// engine.hpp — device-side engine interface shared by kernels.hip (HIP kernels + launchers) and
// hbegp.cpp (host runtime, C ABI).  Everything here is plain C++; no torch, no oracle.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>

namespace hbegp {

constexpr int NB = 128;     // leaf (diagonal block) size; all matrices are padded to a multiple of NB
constexpr int MAXD = 64;    // max number of features
constexpr int MAXP = MAXD + 2;

// Per-evaluation hyper-parameters, linear space, already clamped (fit.rs:94-96).  Lives in device memory;
// the host refreshes it with one hipMemcpyAsync before each evaluation so captured graphs stay valid.
struct EvalParams {
  double noise;      // sigma^2
  double amp;        // c
  double ell[MAXD];  // length scales
  unsigned long long seq;  // serial number of the evaluation (host); the last kernel echoes it into EvalOut::seq of the pinned result block
};

// Per-evaluation scalar results (device -> pinned host).
struct EvalOut {
  double lml;
  double yalpha;   // y^T alpha
  double logdet;   // sum_i log L_ii
  double grad[MAXP];
  int info;        // 0 ok, else 1 + index of the failing pivot (not positive definite)
  int n_warn;      // predict: variances below -sqrt(1e-5)
  int done;        // bit 0: lml written by this evaluation, bit 1: gradient written (a kernel that never ran leaves them clear)
  int pad_;
  unsigned long long seq;  // pinned copy only: EvalParams::seq of the evaluation these results belong to, stored LAST (system scope)
};

// What the first kernel of an evaluation (the kernel-matrix assembly) does besides its tiles when the evaluation is driven
// through pinned host memory (hbegp.cpp, HBEGP_HOSTIO): its workgroup 0 copies the parameters it reads from the host block to
// device memory for the later kernels, poisons the result block and clears the task queue's control words -- one graph node in
// front of the long kernel instead of four (parameter copy, reset kernel, assembly, memset), each of which the GPU spent
// ~30-50 us waiting for while three host threads were enqueuing their graphs.
struct EvalPrologue {
  EvalParams* dP = nullptr;   // device copy of the parameters (null: not the first kernel -- `info` is honoured as usual)
  EvalOut* out = nullptr;     // device result block to poison
  int* ctrl = nullptr;        // task-queue control words to clear (may be null)
  int ctrl_words = 0;
};

// One tile-GEMM operation on row-major matrices, in units of TILE x TILE tiles (global tile coordinates).
//   C(ti,tj) = beta*C(ti,tj) + alpha * sum_{tk in range(ti,tj)} opA(ti,tk) * opB(tk,tj)
// a_kmajor = 0: A tile (ti,tk) is read from A[ti*T.., tk*T..] (rows = output rows, contraction along columns)
// a_kmajor = 1: A tile is read from A[tk*T.., ti*T..] (rows = contraction index)        (same for B with tj)
struct GemmOp {
  const void* A;
  const void* B;
  void* C;
  int lda, ldb, ldc;
  int a_kmajor, b_kmajor;
  int ci0, cj0;   // first output tile (row, col)
  int mi, nj;     // output tiles (rows, cols)
  int c_lower;    // only tiles with global ti >= tj
  int k0, k1;     // contraction tile range [k0, k1)
  int klim;       // 0 none | 1: k <= tj | 2: k >= tj | 3: k <= ti | 4: k >= ti   (global tile coordinates)
  int maskA, maskB;  // operand is lower triangular (its strict upper part is zero IN MEMORY; only used for flop accounting)
  int ntiles;     // output tiles of this op (set by the launcher)
  int reverse;    // walk the tile list backwards (set by the launcher)
  int alpha_neg;  // alpha = -1 instead of +1
  int beta_one;   // beta = 1 instead of 0
};

constexpr int MAXOPS = 4;  // independent tile-GEMM operations per launch

struct GemmLaunch {
  GemmOp op[MAXOPS];
  int nops;
  const int* info;  // device flag: kernels return immediately when *info != 0
  // optional static schedule (device memory): workgroup b runs items [sched_off[b], sched_off[b+1]);
  // item = op << 30 | local tile row << 16 | local tile col, in units of the launch tile size
  const int* sched_off;
  const unsigned* sched_items;
  int sched_nwg;
};

// ---- device-scheduled factorisation: one persistent launch pulls leaf / tile tasks from an ordered queue ----------
// (dag_kernel.inc.hpp; plan built on the host by dag_plan.hpp).  A task waits until its counters have reached their
// values, runs, publishes its results write-through and bumps its own counter.  The queue order is a topological
// order of the dependency graph, so any number of resident workgroups >= 1 makes progress (no co-residency needed).
enum : uint16_t {
  DAG_GEMM_128x64 = 0, DAG_GEMM_64x64 = 1, DAG_LEAF = 2,
  // (3..7 were the kernel-matrix tiles and the alpha / lml reductions as tasks of the same queue, rounds 2-4: measured slower
  // than the launches around the queue, removed in round 5)
  // round 4: a 32x64 output tile whose operands (at most 128 contraction elements at a time, both stored [outer][k]) are
  // fetched in ONE shot -- the two products between consecutive diagonal blocks of the right-looking plan (L(k+1,k) =
  // A(k+1,k) X_kk^T and A(k+1,k+1) -= L(k+1,k) L(k+1,k)^T), where a tile's latency counts and its throughput does not.
  // Same accumulation order per element as the other tiles (k ascending in MFMA steps of four): same bits.
  DAG_GEMM_32x64 = 8,
  // 128x128 output tile for deep products without beta = 1 (no room in the LDS for the old values beside the stage buffers): half
  // the tasks, 8 MFMAs per 6 fragment reads instead of 4 per 4.  Same accumulation order per element: same bits.
  DAG_GEMM_128x128 = 9,
};
enum : uint16_t {
  DAGF_ABUF = 1,   // operand A lives in W2 (else W1)
  DAGF_BBUF = 2,
  DAGF_CBUF = 4,
  DAGF_AKM = 8,    // A tile is read with the contraction index along rows
  DAGF_BKM = 16,
  DAGF_NEG = 32,   // alpha = -1
  DAGF_ACC = 64,   // beta = 1
  DAGF_CKINV = 128,  // the result goes to the launch's K^-1 buffer (tiles of K^-1 = X^T X behind the recursion); skipped when
                     // the launch asks for the factorisation only
  // right-looking plan: the Cholesky factor L itself lives in a third work matrix (W3) until the inverse is complete
  DAGF_A3 = 256,   // operand A lives in W3 (overrides DAGF_ABUF)
  DAGF_B3 = 512,
  DAGF_C3 = 1024,  // the result goes to W3 (overrides DAGF_CBUF)
  // with DAGF_ACC (f64 only, no DAGF_NEG): the old values of the output tile START the accumulation instead of being added at the
  // end -- the second part of a contraction split in two then continues the first part's MFMA chain bit for bit
  DAGF_CINIT = 2048,
};
constexpr int DAG_MAXWAIT = 4;
constexpr int DAG_MAXSIG = 3;
constexpr uint16_t DAG_NOSIG = 0xffff;
struct DagTask {
  uint16_t kind, flags;
  int32_t row0, col0;  // origin of the output tile (elements); leaf: row0 = index of the 128-block
  int32_t kbeg, kend;  // contraction range (elements, whole stages)
  uint16_t nwait;
  uint16_t sig[DAG_MAXSIG];    // counters bumped once the task's results are visible (DAG_NOSIG: unused)
  uint16_t wcnt[DAG_MAXWAIT];  // counters waited for ...
  uint16_t wval[DAG_MAXWAIT];  // ... to reach these values (always the counter's full count)
  uint16_t cost;               // host-side estimate (tenths of a microsecond) used to order the queue
  uint16_t pad_[1];
};
static_assert(DAG_MAXSIG == 3, "DagTask::sig has three entries: dword 5 high half, dword 6 low half, dword 6 high half");
static_assert(sizeof(DagTask) == 48, "DagTask layout");  // dag_kernel decodes it dword by dword: keep the field order

// ---- structurally zero halves of a 128x128 task's operands (ONE rule for the host's accounting and the tile itself) ----------
// An operand that lives in W2 is read out of X = L^-1, whose strict upper triangle is zero in memory.  A 128x128 task's contraction
// range is the union of its two 64-wide halves' ranges, so at one end of the range one half of an operand can lie wholly above the
// diagonal: its products are exact zeros and the waves that own that half may skip them.  Per side (0: A, 1: B) and 64-wide half
// (rows / columns from origin + 64 h) the number of such stages of `bk` contraction elements:
//   operand read [outer][k] (no DAGF_AKM / DAGF_BKM): rows R .. R+63 are zero where k0 >= R + 64        -> TRAILING stages
//   operand read [k][outer] (DAGF_AKM / DAGF_BKM): columns R .. R+63 are zero where k0 + bk <= R          -> LEADING stages
// Operands in W1, W3 or the K^-1 buffer are never triangular to this rule.  No descriptor field carries any of it.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HBEGP_HD __host__ __device__
#else
#define HBEGP_HD
#endif
struct DagZeroHalf {
  int lead[2][2], trail[2][2];  // [side][half]: whole stages
};
HBEGP_HD inline DagZeroHalf dag_zero_halves(int flags, int row0, int col0, int kbeg, int kend, int bk) {
  DagZeroHalf z = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};
  const int nst = (kend - kbeg) / bk;
  if (nst <= 0) return z;
  for (int side = 0; side < 2; ++side) {
    const bool in_w2 = side == 0 ? ((flags & DAGF_ABUF) != 0 && (flags & DAGF_A3) == 0) : ((flags & DAGF_BBUF) != 0 && (flags & DAGF_B3) == 0);
    if (!in_w2) continue;
    const bool km = (flags & (side == 0 ? DAGF_AKM : DAGF_BKM)) != 0;
    for (int h = 0; h < 2; ++h) {
      const int r = (side == 0 ? row0 : col0) + 64 * h;
      if (km) {
        const int c = r > kbeg ? (r - kbeg) / bk : 0;  // stages that end at or above row r
        z.lead[side][h] = c < nst ? c : nst;
      } else {
        const int d = r + 64 - kbeg;
        const int first = d > 0 ? (d + bk - 1) / bk : 0;  // first stage that starts at or behind column r + 64
        z.trail[side][h] = first < nst ? nst - first : 0;
      }
    }
  }
  return z;
}

constexpr int DAG_CTRL_WORDS = 4;     // ctrl[0] queue head, [1] first task that gave up waiting (+1), [2..3] spare; counters follow
constexpr int DAG_INFO_TIMEOUT = -2;  // written to EvalOut::info when a wait exceeded its bound (a bug, never a data property)
struct DagLaunch {
  const DagTask* tasks;
  int ntasks;
  int* ctrl;
  void* W1;
  void* W2;
  void* W3;         // right-looking plan: the factor L (DAGF_A3 / B3 / C3)
  void* Kinv;       // target of the DAGF_CKINV tiles (null: skip them)
  int ld;
  void* ldiag;
  int* info;
  unsigned long long* trace;  // optional (diagnostics): per task [pulled, inputs ready, computed, published] on the 100 MHz clock, then the CU id
  unsigned long long wait_ticks;  // bound of one dependency wait in ticks of the 100 MHz clock (host: from the plan's simulated makespan)
  int leaf_dbg;                   // debug bits of the diagonal-block tasks (tests: 16 = the helper wave starts late, HBEGP_LEAF_DBG)
  int zero_skip;                  // 128x128 tiles: waves skip the MFMAs of structurally zero operand halves (dag_zero_halves; HBEGP_DAG_ZERO_SKIP)
};
template <typename T>
void launch_dag(const DagLaunch& g, int nwg, hipStream_t s);
int dag_stage_depth(bool is_f32);  // contraction elements per pipeline stage of the task-queue tiles (task ranges are whole stages)

// ---- launchers (kernels.hip), T in {double, float} ------------------------------------------------------------
template <typename T>
void launch_gemm(const GemmLaunch& g, int tile, hipStream_t s);  // tile in {32, 64, 128}

template <typename T>
// rv (may be null): known noise variances of the n rows, added to the diagonal entries of rows < n -- K = c Matern + diag(s2 + v)
void launch_kmat(const T* X, const T* rv, int n, int d, int np, int nu2, const EvalParams* P, T* W, const int* info, hipStream_t s,
                 const EvalPrologue* pro = nullptr);

// Factor the 128x128 diagonal block `blk` of W1 (lower) in place -> X_blk = L_blk^-1 into W2's block, diag(L) -> ldiag.
template <typename T>
void launch_leaf(T* W1, T* W2, int ld, int blk, T* ldiag, int* info, hipStream_t s, int dbg = 0);

// alpha = X^T (X y), lml pieces.  X lower-triangular np x np in W2.  part: [np/256][np] scratch.
template <typename T>
// ticket (device int, zero between launches): the last workgroup of the reduction forms the lml itself (no lml_final launch).
void launch_alpha_lml(const T* Xinv, int np, int n, const T* y, const T* ldiag, T* wbuf, double* part, T* alpha,
                      EvalOut* out, const int* info, hipStream_t s, int* ticket = nullptr);

// lml gradient: g_j = 1/2 sum_ik (alpha alpha^T - Kinv)_ik dK_ik/dtheta_j without materialising dK.
template <typename T>
// ticket (device int, zero between launches): the launch's last workgroup finalises the gradient itself and, with hout, copies
// the result block to the pinned one and publishes the evaluation's serial number -- no finalize / publish launches behind it
void launch_gradtrace(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Kinv, const T* alpha,
                      double* part, EvalOut* out, const int* info, hipStream_t s, int* ticket = nullptr, EvalOut* hout = nullptr);
size_t gradtrace_part_elems(int np, int d);

// Input warping (hbegp_problem_eval_xgrad / _eval_warped; kernels.hip: warp_kernel, xgrad_kernel, warp_chain_kernel)
//   warp:   U[n][d] (T) = the Kumaraswamy warp (warp.hpp) of X[n][d] with ab = [a_1..a_d, b_1..b_d] on the device, fp64 arithmetic
//           rounded once; dlna / dlnb [n][d] (fp64; each may be null) = dU/dln a, dU/dln b.  U may not alias X.
//   xgrad:  G[n][d] (fp64) = d lml / d X from the results of an evaluation at P: alpha and the LOWER triangle of Kinv (np x np).
//           part: xgrad_part_elems(n, d) doubles; ticket: a device int, zero between launches.  Fixed summation order.
//   chain:  out[2 d] (fp64) = sum_i G[i][k] dlna[i][k], then the same with dlnb.
size_t xgrad_part_elems(int n, int d);
template <typename T>
void launch_warp(const T* X, int n, int d, const double* ab, T* U, double* dlna, double* dlnb, hipStream_t s);
template <typename T>
void launch_xgrad(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Kinv, const T* alpha, double* part, double* G,
                  int* ticket, hipStream_t s);
void launch_warp_chain(const double* G, const double* dlna, const double* dlnb, int n, int d, double* out, hipStream_t s);

// Leave-one-out cross-validation (hbegp_model_loo / hbegp_problem_eval_loo; kernels.hip: loo_*_kernel), all on one stream:
//   diag:  m_j = column sums of squares of Xinv = L^-1 (rows < n), then mean / var / lpd [n] (T), avec = alpha / m and
//          sbvec = sqrt((1 + alpha^2 / m) / (2 m)) [np] (fp64, zero on the padding), out->lml = loo, out->done |= 1;
//          part: loo_diag_part_elems(np, n) doubles
//   uy:    Y = K^-1 diag(sbvec) (full np x np, zero padding) and u = K^-1 avec [np] (T) from the LOWER triangle of Kinv;
//          pu: loo_u_part_elems(np) doubles
//   trace: out->grad[j] = 1/2 sum_ik (u_i alpha_k + alpha_i u_k - 2 Cm_ik) dK_ik/dtheta_j over the lower triangle of Cm = Y Y^T,
//          out->done |= 2; part: gradtrace_part_elems(np, d) doubles; skipped when out->info != 0
size_t loo_diag_part_elems(int np, int n);
size_t loo_u_part_elems(int np);
template <typename T>
void launch_loo_diag(const T* Xinv, int np, int n, const T* y, const T* alpha, double* part, T* mean, T* var, T* lpd, double* avec,
                     double* sbvec, EvalOut* out, hipStream_t s);
template <typename T>
void launch_loo_uy(const T* Kinv, int np, int n, const double* avec, const double* sbvec, T* Y, double* pu, T* u, hipStream_t s);
template <typename T>
void launch_loo_trace(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Cm, const T* alpha, const T* u,
                      double* part, EvalOut* out, hipStream_t s);

// Leave-group-out cross-validation (hbegp_model_lgo / hbegp_problem_eval_lgo; kernels.hip: lgo_*_kernel).  The
// partition of the n rows into G groups of at most LGO_MAX_GROUP rows, as device arrays of ints (hbegp.cpp: LgoGroups):
//   member [n]      the rows, group by group in ascending dense id, ascending inside a group
//   gid    [n]      the dense id of the group that list position belongs to
//   goff   [G + 1]  where a group's members start in `member`
//   foff   [G + 1]  where its factor F_g (s x s, row-major, lower) starts in the packed array F: the sum of the earlier s^2
//   boff   [nb + 1] bundles of consecutive groups with at most 64 rows together: the first group of each
//   group: part: lgo_gram_chunks(n, smax) * f_elems doubles (f_elems = foff[G]: the chunks' shares of the Gram matrices M_II);
//          mean / var [n] and lpd [G] (T), avec [np] (fp64: r_g on the group's rows; the caller zeroes the padding), F, share [G],
//          out->lml = lgo, out->done |= 1; a pivot that is not > 0 sets out->info and makes the group's lpd NaN
//   uy:    Y (np x np; the caller zeroes the padding columns) and u [np] (T) from the LOWER triangle of Kinv; pu: nb * np doubles;
//          skipped when *info != 0
constexpr int LGO_MAX_GROUP = 64;
struct LgoLists {
  const int *member, *gid, *goff, *foff, *boff;
  int G, nb, smax;  // groups, bundles, the largest group
};
size_t lgo_group_lds_bytes(int smax);
int lgo_gram_chunks(int n, int smax);
size_t lgo_uy_lds_bytes(bool is_f32);
template <typename T>
void launch_lgo_group(const T* Xinv, int np, int n, const T* y, const T* alpha, const LgoLists& L, size_t f_elems, double* part, T* mean,
                      T* var, T* lpd, double* avec, double* F, double* share, EvalOut* out, hipStream_t s);
template <typename T>
void launch_lgo_uy(const T* Kinv, int np, int n, const LgoLists& L, const double* avec, const double* F, T* Y, double* pu, T* u,
                   const int* info, hipStream_t s);

template <typename T>
void launch_symmetrize(T* A, int np, hipStream_t s);  // mirror lower -> upper

// predict: Kstar [mp x np] (rows = candidates), mean, var
template <typename T>
void launch_kstar(const T* Xs, int m, int mp, const T* X, int n, int d, int np, int nu2, const EvalParams* P, T* Ks,
                  hipStream_t s);
template <typename T>
void launch_pred_mean(const T* Ks, int m, int np, const T* alpha, T* mean, hipStream_t s);
template <typename T>
void launch_pred_var(const T* Ks, const T* Q, int m, int np, const EvalParams* P, T* var, EvalOut* out, hipStream_t s);
// posterior gradient w.r.t. the candidates: dmean[m][d] (part: pred_grad_chunks(n) * m * d doubles); G[d][mp][np] = dKstar/dx*_k;
// dvar[m][d] = -2 rowsum(W_k o Q) with W = G X^T (tile GEMM), 0 where the clamped variance var[i] is 0
template <typename T>
void launch_pred_grad(const T* Xs, int m, const T* X, int n, int d, int nu2, const EvalParams* P, const T* alpha, double* part, T* dmean,
                      hipStream_t s);
template <typename T>
void launch_kstar_grad(const T* Xs, int m, int mp, const T* X, int n, int d, int np, int nu2, const EvalParams* P, T* G, hipStream_t s);
template <typename T>
void launch_pred_dvar(const T* W, const T* Q, int m, int mp, int np, int d, const T* var, T* dvar, hipStream_t s);
int pred_grad_chunks(int n);
// sensitivity of the posterior mean (hbegp_sobol_* / hbegp_main_effects_*; kernels.hip: sens_kernel).  Xb holds
// all base rows [.][d]; one call takes the slab of `rows` rows from r0 on.  Rows below nsub get every feature k substituted:
//   G = 0 (per row):  by sub[i][k] (sub [nsub][d], unscaled)                -> fsub[k][i] (T, leading dimension nsub)
//   G > 0 (per grid): by sg[k][0..G) (sub = sg [d][G] from launch_sens_scale_grid) -> chunk 0's slot of part, fp64, for
//                     launch_sens_effect: eff[k][g] (zero before the first slab) += the slab's rows in ascending order, / N at `last`
// The base value of every row of the slab -> fbase[r0 + row] (T).  part: sens_chunks(n) * rows * (1 + d * max(G, 1)) doubles.
// ev_mid (may be null) is recorded between the evaluation and the chunk sums.
// launch_sobol_reduce: fbase = [f_A | f_B] (N each), fsub = f_AB -> out = first[d], total[d], f0, V (fp64).
int sens_chunks(int n);
template <typename T>
void launch_sens_eval(const T* Xb, int r0, int rows, int nsub, const T* sub, int G, const T* X, int n, int d, int nu2, const EvalParams* P,
                      const T* alpha, double* part, T* fbase, T* fsub, hipStream_t s, hipEvent_t ev_mid = nullptr);
template <typename T>
void launch_sens_scale_grid(T* sg, int d, int G, const EvalParams* P, hipStream_t s);
void launch_sens_effect(const double* part, int rows, int d, int G, double* eff, int N, int last, hipStream_t s);
template <typename T>
void launch_sobol_reduce(const T* fbase, const T* fsub, int N, int d, double* out, hipStream_t s);
// joint posterior (hbegp_predict_cov / hbegp_sample_posterior): launch_leaf plus L_kk itself -> W3's block (lower, zeros above
// the diagonal); then, per draw s (row s of Y [S][ld] = (L z_s)^T): Y[s][i] += mean[i] when `store`, amin[s] = argmin_i, ties
// to the lowest index.  Both do nothing when *info != 0.
template <typename T>
void launch_leaf_keep(T* W1, T* W2, T* W3, int ld, int blk, T* ldiag, int* info, hipStream_t s);
template <typename T>
void launch_sample_epilogue(T* Y, int ld, const T* mean, int m, int S, int store, int* amin, const int* info, hipStream_t s);
// greedy batch selection by EI (hbegp_select_batch; batch_select_kernel: one workgroup, the whole k-step loop): Sig the symmetrised
// Sigma [ld][ld] at jitter 0, mean[m] the posterior mean, P->noise the fantasy observations' noise s2, use_lie ? lie : mu_j the
// fantasy.  Workspace (fp64): C [k][ld], v [ld], mu [ld]; picked [ld] ints.  Out: idx[k], ei[k], and mean_out / var_out [m] after
// the k conditionings (var clamped at 0).  1 <= k <= m.
template <typename T>
void launch_batch_select(const T* Sig, int ld, const T* mean, int m, int k, const EvalParams* P, double fmin, int use_lie, double lie,
                         double* C, double* v, double* mu, int* picked, int* idx, double* ei, T* mean_out, T* var_out, hipStream_t s);
// knowledge gradient over a candidate set (hbegp_knowledge_gradient; kg_kernel: one workgroup per candidate): Sig the symmetrised
// Sigma [ld][ld] at jitter 0, mean[m], P->noise the sample's noise s2.  Out: kg[mc] (fp64), res[2] = {the last index of the maximum
// of kg (-1 for mc = 0), the lowest index of the minimum of the mean}, var_out[m] = max(diag Sigma, 0).  0 <= mc <= m, m >= 1.
// The (b, a) lines of a candidate, padded to kg_padded_rows(m) (a power of two), live in the LDS up to KG_LDS_ROWS of them; beyond,
// in ws: kg_global_workgroups(m, mc) * kg_padded_rows(m) lines of 16 bytes (ws is unused, and may be null, where that is 0).
constexpr int KG_LDS_ROWS = 8192;
constexpr int KG_GLOBAL_WGS = 512;
constexpr size_t kg_lds_bytes(int rows) { return 16 * (size_t)rows + 8 * 256 + 16; }  // the lines, the sum's tree, the stack height
int kg_padded_rows(int m);
int kg_global_workgroups(int m, int mc);
template <typename T>
void launch_knowledge_gradient(const T* Sig, int ld, const T* mean, int m, int mc, const EvalParams* P, void* ws, double* kg, int* res,
                               T* var_out, hipStream_t s);
// noisy expected improvement over a candidate set (hbegp_noisy_ei).  The baseline takes rows 0 .. mb - 1 of every
// matrix, the candidates rows mbp .. mbp + mc - 1 (mbp = mb rounded up to NB).
//   pad:    rows and columns mb .. mbp - 1 of Sigma's lower tiles W [ld][ld] become identity padding (nothing to do for mb = mbp)
//   reduce: Sig = Sigma (its diagonal is read), LA = [L_b; A] (rows mbp .. of its first mb columns are read), Y [S][ld] the draw
//           product, mean [ld].  Out (fp64): fmin_draws[S]; with mc > 0 rho[mc], nei[mc] and *best = the last index of the maximum of
//           nei.  Nothing is written when *info != 0.
template <typename T>
void launch_nei_pad(T* W, int ld, int mb, int mbp, hipStream_t s);
template <typename T>
void launch_nei_reduce(const T* Sig, const T* LA, const T* Y, int ld, const T* mean, int mb, int mbp, int mc, int S, double* fmin_draws,
                       double* rho, double* nei, int* best, const int* info, hipStream_t s);
// expected hypervolume improvement of two independent objectives (hbegp_ehvi; ehvi_kernel: one wave per candidate).
// mean / var [m] and, with want_grad, dmean / dvar [m][d] of the two models; thr = [up | hb], ns = P + 1 strips each: up[i] the upper
// end of strip i along objective 0 (up[ns - 1] = r1), hb[i] its height threshold along objective 1 (hb[0] = r2).  Out: ehvi[m] (fp64),
// grad[m][d] (want_grad), *best = the last index of the maximum of ehvi (NaN never wins; m >= 1).  Up to EHVI_LDS_STRIPS strips are
// staged in the LDS.
constexpr int EHVI_LDS_STRIPS = 4096;
constexpr size_t ehvi_lds_bytes(int ns) { return 16 * (size_t)ns; }
template <typename T>
void launch_ehvi(const T* mean1, const T* var1, const T* dmean1, const T* dvar1, const T* mean2, const T* var2, const T* dmean2,
                 const T* dvar2, int m, int d, const double* thr, int ns, int want_grad, double* ehvi, T* grad, int* best, hipStream_t s);
// constrained expected improvement over K = 1 + C independent models (hbegp_constrained_ei; cei_kernel: one wave per candidate;
// DESIGN section 22).  Model 0 is the objective, models 1 .. C the constraints g_k <= thr[k]; thr[0] = fmin (+inf: no feasible
// incumbent, EI counts as 1).  mean / var [m] and, with want_grad, dmean / dvar [m][d] of every model (dmean / dvar are not read
// without a gradient).  Out: cei[m] (fp64), ei[m], pof[m] (fp64; each may be null), grad[m][d] (want_grad), *best = the last index
// of the maximum of cei (NaN never wins; m >= 1).
constexpr int CEI_MAX_MODELS = 9;  // 1 + HBEGP_CEI_MAX_CONSTRAINTS
template <typename T>
struct CeiArgs {
  const T* mean[CEI_MAX_MODELS];
  const T* var[CEI_MAX_MODELS];
  const T* dmean[CEI_MAX_MODELS];
  const T* dvar[CEI_MAX_MODELS];
  double thr[CEI_MAX_MODELS];
  int K;
};
template <typename T>
void launch_cei(const CeiArgs<T>& a, int m, int d, int want_grad, double* cei, double* ei, double* pof, T* grad, int* best, hipStream_t s);
// the same in log space (hbegp_log_constrained_ei; lcei_kernel): lcei = lei + lpof with lei = log ei (0 for fmin = +inf) and
// lpof = sum_k log F_k from stable forms, the gradient of lcei, *best = the last index of the maximum of lcei.
template <typename T>
void launch_lcei(const CeiArgs<T>& a, int m, int d, int want_grad, double* lcei, double* lei, double* lpof, T* grad, int* best, hipStream_t s);
// expected hypervolume improvement of 2 .. 4 independent objectives over a box decomposition of the free region (hbegp_ehvi_nd;
// ehvi_nd_kernel: one wave per candidate).  a.K = n_obj models: mean / var [m] and, with want_grad, dmean / dvar
// [m][d] (a.thr is not read).  thr [g.nt] on the device: objective k's thresholds at g.off[k] .. g.off[k] + g.T[k] - 1, entry 0 standing
// for -inf (never evaluated), the last one r_k.  boxes [g.n_boxes][2 n_obj] ints on the device: per objective (l, u), each g.off[k] +
// its index into objective k's thresholds.  Per candidate the kernel first fills a table of (G, Phi, phi) at every threshold -- 24
// bytes per entry, g.nt entries -- and then sums over the boxes by lookup.  Where the table lives is the call's regime, decided by
// g.nt alone:
//   nt <= EHVI_ND_LDS4_ENTRIES   in the LDS, EHVI_ND_WAVES candidates per workgroup (their tables fit the 64 KiB default)
//   nt <= EHVI_ND_LDS1_ENTRIES   in the LDS, one candidate per workgroup (one table in the workgroup's 160 KiB)
//   beyond                       in `scratch` [m][nt][3] doubles on the device (null in the two LDS regimes)
// A candidate's arithmetic is the same in all three.  Out: ehvi[m] (fp64), grad[m][d] (want_grad), *best = the last index of the
// maximum of ehvi (NaN never wins; m >= 1).
constexpr int EHVI_ND_MAX_OBJ = 4;
constexpr int EHVI_ND_WAVES = 4;
constexpr int EHVI_ND_LDS4_ENTRIES = 65536 / (24 * EHVI_ND_WAVES);  // 682
constexpr int EHVI_ND_LDS1_ENTRIES = 163840 / 24;                    // 6826
constexpr size_t ehvi_nd_lds_bytes(int nt, int waves) { return 24 * (size_t)nt * waves; }
struct EhviNdGeom {
  int n_obj;
  int T[EHVI_ND_MAX_OBJ];    // thresholds per objective, -inf and r_k included
  int off[EHVI_ND_MAX_OBJ];  // where they start in thr and in the table
  int nt;                    // their sum
  int n_boxes;
};
template <typename T>
void launch_ehvi_nd(const CeiArgs<T>& a, int m, int d, const double* thr, const int* boxes, const EhviNdGeom& g, double* scratch,
                    int want_grad, double* ehvi, T* grad, int* best, hipStream_t s);
// max-value entropy search (hbegp_mes; mes_kernel: one wave per candidate): mean, var [m] and, with want_grad, dmean, dvar [m][d] of
// ONE model; ystar [S] on the device, S >= 1.  Out: mes[m], grad[m][d] (want_grad), *best = the last index of the maximum of mes.
template <typename T>
void launch_mes(const T* mean, const T* var, const T* dmean, const T* dvar, int m, int d, const double* ystar, int S, int want_grad,
                double* mes, T* grad, int* best, hipStream_t s);
// the confidence bound mu + kappa sigma (hbegp_confidence_bound; cb_kernel: 2^ceil(log2 d) lanes per candidate):
// mean, var [m] and, with want_grad, dmean, dvar [m][d] of ONE model; kappa travels in the kernel's arguments.  Out: cb[m],
// grad[m][d] (want_grad), *best = the FIRST index of the minimum of cb (argmin_first_kernel; NaN never wins; m >= 1).
template <typename T>
void launch_cb(const T* mean, const T* var, const T* dmean, const T* dvar, int m, int d, double kappa, int want_grad, double* cb, T* grad,
               int* best, hipStream_t s);
// batch expected improvement by Monte Carlo (hbegp_qei; qei_batch_kernel: one workgroup per batch of q points).  Rows b q .. b q + q - 1
// of Xs [B q][d], Q [mp][np], mean, dmean [mp][d] and W [d][mp][np] (W and dmean are read only with want_grad); z [S][q] shared by
// the batches; noise = 1e-5 + jitter.  Out: qei[B], grad[B q][d] (want_grad), info[B] (0, or 1 + the column whose pivot failed).
constexpr int QEI_MAXQ = 64;
constexpr int QEI_CH = 256;  // draws per chunk
// dynamic LDS of qei_batch_kernel: fp64 points / ell [q d], Sigma -> L [q q], Lbar -> X [q q], mu, mubar [q], I_s [QEI_CH]; ints
// j_s [QEI_CH] and the failure flag (padded to 4)
constexpr size_t qei_lds_bytes(int q, int d) {
  return sizeof(double) * ((size_t)q * d + 2 * (size_t)q * q + 2 * (size_t)q + QEI_CH) + sizeof(int) * (QEI_CH + 4);
}
template <typename T>
void launch_qei_batch(const T* Xs, int B, int q, int d, const T* Q, const T* W, int mp, int np, const T* mean, const T* dmean,
                      const EvalParams* P, double noise, int nu2, const T* z, int S, double fmin, int want_grad, double* qei, T* grad,
                      int* info, hipStream_t s);

// posterior sample paths (hbegp_paths_*; kernels.hip: paths_project_kernel, paths_eval_kernel).  omT [d][F] = om0^T / ell, phase [F],
// Wf [S][F] are fp64 for both element types; Vt, Rt [Sp][np] hold one path per row (the tile GEMMs' operand layout).
//   scale_omega: omT from the caller's unit-length-scale om0 [F][d]
//   project:     Rt[s][i] = y_i - sqrt(2c/F) sum_j Wf[s][j] cos(om_j . x_i + b_j) - sqrt(sigma^2 + v_i) eps[s][i] (eps [S][n] or null;
//                v = rv [n] or null: the model's known row variances), zero padding; part: paths_project_chunks(F, n, S) * S * n doubles
//   eval:        f [S][m], df [S][m][d] (want_grad) at Xs [m][d] (per_path = 0) or [S][m][d] (per_path = 1);
//                part: paths_eval_chunks(n, F) * S * m * (d + 1) doubles
int paths_project_chunks(int F, int n, int S, int* fch_out = nullptr, int* cap_out = nullptr);  // cap_out: the most chunks the partial sums allow
int paths_eval_chunks(int n, int F, int* nchd_out = nullptr);
template <typename T>
void launch_paths_scale_omega(const T* om0, int F, int d, const EvalParams* P, double* omT, hipStream_t s);
template <typename T>
void launch_paths_project(const T* X, int n, int d, int np, const double* omT, const double* phase, int F, const double* Wf, int S, int Sp,
                          const T* y, const T* eps, const T* rv, const EvalParams* P, double* part, T* Rt, hipStream_t s);
template <typename T>
void launch_paths_eval(const T* Xs, int m, int per_path, int S, const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Vt,
                       const double* omT, const double* phase, const double* Wf, int F, int want_grad, double* part, T* f, T* df,
                       hipStream_t s);

// predict for m <= PRED_SMALL_MAX candidates without the 128-row padding: reads L^-1 once (row dots against the m
// cross-kernel vectors).  Ks: [PRED_SMALL_MAX][np] scratch, pmean: [(np+255)/256][PRED_SMALL_MAX], w: [n][PRED_SMALL_MAX].
constexpr int PRED_SMALL_MAX = 16;
template <typename T>
void launch_predict_small(const T* Xs, int m, const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* alpha, const T* Linv,
                          T* Ks, double* pmean, double* w, int want_var, T* mean, T* var, int* n_warn, hipStream_t s);

// One evaluation of a problem of at most 128 rows (np = NB, d <= SMALL_EVAL_MAXD) in ONE launch, everything in the LDS
// (kernels.hip: small_eval_kernel).  mode bit 0: alpha + lml, bit 1: K^-1, bit 2: gradient.
constexpr int SMALL_EVAL_MAXD = 32;
struct SmallEval {
  const void* X;
  const void* y;
  int n, d;
  const EvalParams* P;
  void* W2;
  void* ldiag;
  void* Kinv;
  void* alpha;
  EvalOut* out;    // device memory: the diagonal block's positive-definite flag (atomics)
  EvalOut* hout;   // where the results go: the slot's pinned host block (written by the kernel itself: no copy node) or `out`
  int mode;
};
// rv (may be null): known noise variances of the n rows, in the element type of X.  It travels beside SmallEval, not inside it: the
// descriptor a run of small_fit_kernel copies to its stack for every evaluation keeps its size.
template <typename T>
void launch_small_eval(const SmallEval& g, const void* rv, int nu2, hipStream_t s);

// One optimiser run of a fit of at most 128 rows in ONE launch (kernels.hip: small_fit_kernel): the evaluation above in a loop
// with the bounded L-BFGS step and the fit's objective wrapper (clamping, failed evaluations, capture of the best) on the device.
struct LbfgsState;
struct SmallFitResult {
  double best_lml;
  double best_theta[MAXP];   // as the optimiser passed it (log space, unclamped noise)
  double best_params[MAXP];  // the clamped linear-space parameters the captured evaluation ran with (the DEVICE's exp of best_theta: the
                             // model's L^-1 is refactored from exactly these, not from the host's exp of the same theta)
  int best_idx;              // ping-pong buffer (K^-1, alpha) that holds the captured evaluation; -1: every evaluation failed
  int best_eval;             // its index within the run
  int n_evals, n_not_pd;
};
struct SmallFit {
  SmallEval ev;              // X, y, n, d, P (device workspace, written by the kernel), W2, ldiag, out = hout (device workspace)
  void* Kinv[2];
  void* alpha[2];
  void* Xinv[2];             // L^-1 and diag(L) ping-pong with K^-1 and alpha (null: ev.W2 / ev.ldiag every time): the model is built
  void* ldiag[2];            // from the captured evaluation's own factor instead of factoring once more at the captured theta
  LbfgsState* st;            // device workspace
  const double* x0;          // start point (log space), p = d + 2 entries
  const double* lo;          // linear-space box
  const double* hi;
  int maxeval, memory, fixed_work;
  double pgtol, ftol;
  SmallFitResult* res;       // device
  SmallFitResult* hres;      // pinned host copy of *res, written at the end of the run (null: none) ...
  unsigned long long* hdone; // ... followed, behind a system-scope fence, by 1 in this pinned word: the host thread that owns the
                             // run polls it -- the launch may carry other fits' runs (hbegp.cpp: SmallBatcher) and need not be over
  double* trace_theta;       // [trace_cap][p] (device; may be null with trace_cap = 0)
  double* trace_lml;         // [trace_cap]
  double* trace_grad;        // [trace_cap][p]
  int trace_cap;
  const void* rv;            // known noise variances of the run's n rows (element type of X; null: none): every run of a shared launch
                             // carries its own
};
// fs_dev: device array of nruns descriptors; run r is workgroup r of one launch
template <typename T>
void launch_small_fit(const SmallFit* fs_dev, int nruns, int nu2, hipStream_t s);

void launch_set_info(int* info, int value, hipStream_t s);
// start of an evaluation: info = n_warn = done = 0, lml and gradient poisoned with NaN (a launch that was rejected or
// skipped can then never pass for a result)
void launch_reset_out(EvalOut* out, hipStream_t s);
// Last kernel of an evaluation driven through pinned host memory: copies the device result block to the pinned one and then,
// behind a system-scope fence, stores P->seq into hout->seq -- the host thread spins on that word instead of sleeping in
// hipStreamSynchronize (interrupt wake-up: ~50 us of every evaluation).
void launch_publish_out(const EvalOut* out, EvalOut* hout, const EvalParams* P, hipStream_t s);
// throws nothing: returns the first pending launch error of the calling thread's device (hipGetLastError)
void init_kernels();

// *flag |= 1 when the two device arrays differ anywhere in [0, count)
template <typename T>
void launch_prefix_differs(const T* a, const T* b, size_t count, int* flag, hipStream_t s);

}  // namespace hbegp
