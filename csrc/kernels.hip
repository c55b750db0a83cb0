// kernels.hip — hand-written gfx950 (CDNA4) kernels of the GP engine and their launchers.
//
//  gemm_kernel   : MFMA tile GEMM with triangular contraction ranges; carries Cholesky TRSM/SYRK, the
//                  triangular inverse (TRTRI as GEMMs), LAUUM (K^-1 = X^T X) and the predictive GEMM.
//  leaf_kernel   : 128x128 diagonal block: Cholesky + inverse of the factor, LDS resident, 16x16 diagonal
//                  sub-blocks factored in one wavefront with lane broadcasts, the rest on MFMA.
//  kmat_kernel   : K = c*Matern(X,X) + s2*I (lower tiles), matern_kernel.rs:37-81 + constant/product kernels + lml.rs:44.
//                  With known per-row noise variances v (rv, hbegp.h "row variances"): K = c*Matern + diag(s2 + v).
//  gradtrace     : 1/2 tr((aa^T - K^-1) dK/dtheta_j) for all j in one pass over K^-1 (lml.rs:62-70, matern_kernel.rs:83-135)
//                  without the n x n x (d+1) tensor the reference materialises.
//  trmv/finalize : alpha = X^T (X y), y^T alpha, sum log L_ii (lml.rs:54-59).
//  kstar/pred_*  : predict.rs:7-52.
//
// Element type T is double or float; MFMA = v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32
// (A frag: lane l holds A[l&15][l>>4]; B frag: B[l>>4][l&15]; C/D: col = l&15, row = (l>>4)+4r for f64,
//  4*(l>>4)+r for f32).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "engine.hpp"
#include "fastmath.hpp"
#include "lbfgs_step.hpp"
#include "warp.hpp"

namespace hbegp {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

template <typename T> struct Cfg;
template <> struct Cfg<double> {
  static constexpr int VEC = 2;   // elements per 16-byte chunk
  static constexpr int BK = 16;   // contraction depth per LDS stage (128 bytes)
  using vec_t = d2;
  using acc_t = d4;
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int lane, int r) { return (lane >> 4) + 4 * r; }
  static __device__ __forceinline__ void lds_store(double* dst, vec_t v) { *reinterpret_cast<vec_t*>(dst) = v; }
};
template <> struct Cfg<float> {
  static constexpr int VEC = 4;
  static constexpr int BK = 32;
  using vec_t = f4;
  using acc_t = f4;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int lane, int r) { return (lane >> 4) * 4 + r; }
  static __device__ __forceinline__ void lds_store(float* dst, vec_t v) {  // rows are only 8-byte aligned
    f2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
    *reinterpret_cast<f2*>(dst) = lo;
    *reinterpret_cast<f2*>(dst + 2) = hi;
  }
};

__device__ __forceinline__ double readlane(double v, int lane) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, lane);
  hi = __builtin_amdgcn_readlane(hi, lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// =================================================================================================================
// Tile GEMM
// =================================================================================================================
// contraction elements per f32 accumulation chunk (see gemm_kernel); boundaries at absolute multiples.  64 was measured (C5 f32
// fits 8.63 -> 9.70 /s, M f32 2.78 -> 2.79), but alpha at cond(K) = 7e4 then leaves the plain 1e-4 bar (8e-5 -> 1.03e-4,
// tests/test_gpu_fullsize.py)
constexpr int F32_CHUNK = 32;

template <typename T, int TILE, int KM = 0>
struct GemmGeom {
  using C = Cfg<T>;
  // contraction depth per LDS stage: 128 bytes of k for the big tiles, 256 bytes for the 32-tiles (small, latency-bound
  // launches: fewer, fatter stages; measured in the 3-stream bench, 32-tile depth x1 / x2 / x4: 1.104 / 1.127 / 1.054 fit+predict/s)
  static constexpr int BKE = (KM > 0 ? KM : (TILE == 32 ? 2 : 1)) * C::BK;
  static constexpr int SK = BKE + 2;          // LDS row stride, operand stored [outer][k]
  static constexpr int SM = TILE + 16;        // LDS row stride, operand stored [k][outer]
  static constexpr int LDSE = (TILE * SK > BKE * SM) ? TILE * SK : BKE * SM;  // elements per operand buffer
  static constexpr int NCH = TILE * BKE / C::VEC / 256;  // 16-byte chunks per thread per operand per stage
  static constexpr int TM = TILE / 32;        // 16x16 MFMA blocks per wave per dimension
};

__device__ __forceinline__ int tri_row(int idx) {
  // largest r with r(r+1)/2 <= idx
  int r = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  while (r * (r + 1) / 2 > idx) --r;
  return r;
}

template <typename T, int TILE, int KM = 0>
__global__ void __launch_bounds__(256, 2) gemm_kernel(GemmLaunch g) {
  using C = Cfg<T>;
  using G = GemmGeom<T, TILE, KM>;
  using vec_t = typename C::vec_t;
  using acc_t = typename C::acc_t;
  constexpr int VEC = C::VEC, BK = G::BKE, SK = G::SK, SM = G::SM, NCH = G::NCH, TM = G::TM;

  // The not-positive-definite flag is only needed before anything is written: load it now, test it in the epilogue, so
  // its latency overlaps the operand loads (work on garbage is harmless, stores are not).
  const int bad = *g.info;

  // Work list of this workgroup: either one tile decoded from blockIdx (plain launches) or a host-built static
  // schedule (longest-processing-time assignment of tiles to a fixed number of resident workgroups, see hbegp.cpp).
  int it = 0, it_end = 1;
  if (g.sched_off) {
    it = g.sched_off[blockIdx.x];
    it_end = g.sched_off[blockIdx.x + 1];
  }
  // Kernel-argument reads are scalar loads with a few hundred cycles of latency each.  Everything the decoding needs is
  // fetched in two batches -- the per-op tile counts at fixed offsets, then the whole descriptor of the chosen op by
  // value -- instead of one dependent load per field (measured: 3000 cycles from kernel entry to the first operand load).
  const int nops = g.nops;
  const int nt0 = g.op[0].ntiles, nt1 = g.op[1].ntiles, nt2 = g.op[2].ntiles;
  for (; it < it_end; ++it) {
  int oi = 0, li = 0, lj = 0, bid = blockIdx.x;
  if (g.sched_off) {
    const unsigned item = g.sched_items[it];
    oi = item >> 30;
    li = (item >> 16) & 0x3fff;
    lj = item & 0xffff;
  } else {
    if (nops > 1 && bid >= nt0) {
      bid -= nt0; oi = 1;
      if (nops > 2 && bid >= nt1) {
        bid -= nt1; oi = 2;
        if (nops > 3 && bid >= nt2) { bid -= nt2; oi = 3; }
      }
    }
  }
  const GemmOp op = g.op[oi];
  if (!g.sched_off) {
    if (op.reverse) bid = op.ntiles - 1 - bid;  // heaviest tiles first
    if (op.c_lower) {
      li = tri_row(bid);
      lj = bid - li * (li + 1) / 2;
    } else {
      li = bid / op.nj;
      lj = bid - li * op.nj;
    }
  }
  const int ti = op.ci0 + li, tj = op.cj0 + lj;

  int ka = op.k0, kb = op.k1;
  switch (op.klim) {
    case 1: kb = min(kb, tj + 1); break;
    case 2: ka = max(ka, tj); break;
    case 3: kb = min(kb, ti + 1); break;
    case 4: ka = max(ka, ti); break;
    default: break;
  }
  // contraction range in elements, rounded outward to whole stages.  The extension stays inside the same 128-block:
  // there a triangular operand is zero in memory (its strict upper triangle, see load_stage) and the other operand is finite.
  const int kbeg = (ka * TILE) / BK * BK, kend = (kb * TILE + BK - 1) / BK * BK;
  const int nstages = (kend - kbeg) / BK;

  extern __shared__ __align__(16) char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);  // [A buf0 | A buf1 | B buf0 | B buf1], LDSE elements each

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const int akm = op.a_kmajor, bkm = op.b_kmajor;
  const int lda = op.lda, ldb = op.ldb;

  // Per-thread chunk 0 of a stage slab: storage (row, col) relative to the slab origin; chunk q = chunk 0 + q row passes.
  constexpr int CPR = TILE / VEC;        // chunks per slab row, operand stored [k][outer]
  constexpr int CPK = BK / VEC;          // chunks per slab row, operand stored [outer][k]
  constexpr int RPP_K = 256 / CPK;       // slab rows covered per pass, operand stored [outer][k]
  constexpr int RPP_M = 256 / CPR;       // slab rows covered per pass, operand stored [k][outer]
  const int a_r0 = akm ? t / CPR : t / CPK, a_c0 = akm ? (t % CPR) * VEC : (t % CPK) * VEC;
  const int b_r0 = bkm ? t / CPR : t / CPK, b_c0 = bkm ? (t % CPR) * VEC : (t % CPK) * VEC;
  const int a_rpp = akm ? RPP_M : RPP_K, b_rpp = bkm ? RPP_M : RPP_K;
  const int a_lds0 = a_r0 * (akm ? SM : SK) + a_c0, a_ldsq = a_rpp * (akm ? SM : SK);
  const int b_lds0 = 2 * G::LDSE + b_r0 * (bkm ? SM : SK) + b_c0, b_ldsq = b_rpp * (bkm ? SM : SK);

  // global pointers of chunk 0 at stage 0; they advance by a uniform stride per stage
  const T* pA = static_cast<const T*>(op.A) +
                (akm ? (size_t)(kbeg + a_r0) * lda + ti * TILE + a_c0 : (size_t)(ti * TILE + a_r0) * lda + kbeg + a_c0);
  const T* pB = static_cast<const T*>(op.B) +
                (bkm ? (size_t)(kbeg + b_r0) * ldb + tj * TILE + b_c0 : (size_t)(tj * TILE + b_r0) * ldb + kbeg + b_c0);
  const size_t a_step = akm ? (size_t)BK * lda : (size_t)BK, b_step = bkm ? (size_t)BK * ldb : (size_t)BK;
  const size_t a_qs = (size_t)a_rpp * lda, b_qs = (size_t)b_rpp * ldb;

  // two register sets: the loads of stage s+2 are in flight while stage s is computed and stage s+1 sits in LDS
  vec_t ra0[NCH], rb0[NCH], ra1[NCH], rb1[NCH];

  // Triangular operands (X = L^-1 in W2 / the model's copy) need no masking: the strict upper triangle of those buffers
  // is zero in memory (cleared when the slot is created; the diagonal blocks write explicit zeros above the diagonal).
  auto load_stage = [&](vec_t (&ra)[NCH], vec_t (&rb)[NCH]) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) ra[q] = *reinterpret_cast<const vec_t*>(pA + q * a_qs);
#pragma unroll
    for (int q = 0; q < NCH; ++q) rb[q] = *reinterpret_cast<const vec_t*>(pB + q * b_qs);
    pA += a_step;
    pB += b_step;
  };
  auto store_stage = [&](int buf, vec_t (&ra)[NCH], vec_t (&rb)[NCH]) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      C::lds_store(lds + buf * G::LDSE + a_lds0 + q * a_ldsq, ra[q]);
      C::lds_store(lds + buf * G::LDSE + b_lds0 + q * b_ldsq, rb[q]);
    }
  };

  acc_t acc[TM][TM];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
  // f32 only: the MFMA accumulates in f32, and a long sum of products of one sign (the diagonals of T T^T and X^T X) loses
  // every term below half an ulp of the running sum -- a systematic loss, measured as a -2e-4 relative bias of K^-1 at
  // n=2048, cond 7e4 (LAPACK f32: -4e-5).  Every F32_CHUNK contraction elements the accumulators are added to fp64 totals
  // and cleared (chunk 32: bias -3e-6 in a host emulation).  Chunk boundaries are absolute multiples of F32_CHUNK, so every
  // tile size, and the task-queue kernel, produce the same bits.
  constexpr bool CHUNKED = sizeof(T) == 4;
  double tot[CHUNKED ? TM : 1][CHUNKED ? TM : 1][4];
  if constexpr (CHUNKED) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[a][b][r] = 0.0;
  }
  auto flush = [&]() {
    if constexpr (CHUNKED) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r) tot[a][b][r] += (double)acc[a][b][r];
          acc[a][b] = acc_t{0, 0, 0, 0};
        }
    }
  };
  int kabs = kbeg;  // f32: absolute contraction index of the stage being computed (chunk boundaries are absolute multiples of F32_CHUNK)

  // fragment addressing: element (outer index o, contraction k) at o*so + k*sk
  const int soA = akm ? 1 : SK, skA = akm ? SM : 1;
  const int soB = bkm ? 1 : SK, skB = bkm ? SM : 1;
  const int fa0 = (wm * (TILE / 2) + (lane & 15)) * soA + (lane >> 4) * skA;
  const int fb0 = 2 * G::LDSE + (wn * (TILE / 2) + (lane & 15)) * soB + (lane >> 4) * skB;

  // Fragments are double-buffered in registers: the LDS reads of k-step k4+1 are issued before the MFMAs of k-step k4,
  // otherwise every k-step exposes one LDS round trip (the MFMAs of a step are issued long before they finish, but the
  // next reads cannot start until the last of them has been issued).
  auto compute_stage = [&](int buf) {
    const int ia = buf * G::LDSE + fa0, ib = buf * G::LDSE + fb0;
    T af[2][TM], bf[2][TM];
#pragma unroll
    for (int a = 0; a < TM; ++a) af[0][a] = lds[ia + a * 16 * soA];
#pragma unroll
    for (int b = 0; b < TM; ++b) bf[0][b] = lds[ib + b * 16 * soB];
#pragma unroll
    for (int k4 = 0; k4 < BK / 4; ++k4) {
      const int cur = k4 & 1, nxt = cur ^ 1;
      if (k4 + 1 < BK / 4) {
#pragma unroll
        for (int a = 0; a < TM; ++a) af[nxt][a] = lds[ia + a * 16 * soA + (k4 + 1) * 4 * skA];
#pragma unroll
        for (int b = 0; b < TM; ++b) bf[nxt][b] = lds[ib + b * 16 * soB + (k4 + 1) * 4 * skB];
      }
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = C::mfma(af[cur][a], bf[cur][b], acc[a][b]);
      // pin the order: [LDS reads of step k4+1] then [MFMAs of step k4] (hipcc otherwise sinks half of the reads below
      // the MFMAs to save registers)
      if (k4 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 2 * TM, 0);
      if (k4 + 1 < BK / 4) __builtin_amdgcn_sched_group_barrier(0x100, 2 * TM, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, TM * TM, 0);
      if (CHUNKED && (kabs + (k4 + 1) * 4) % F32_CHUNK == 0) flush();
    }
    kabs += BK;
  };

  if constexpr (TILE == 128) {
    // one register set (the 128-tile already holds 128 accumulator registers; two spill: 52.9 vs 59.7 TFLOP/s): loads of
    // stage s+1 fly during stage s
    if (nstages > 0) {
      load_stage(ra0, rb0);
      store_stage(0, ra0, rb0);
    }
    __syncthreads();
    int s = 0;
    for (; s + 1 < nstages; ++s) {
      const int buf = s & 1;
      load_stage(ra0, rb0);
      compute_stage(buf);
      __builtin_amdgcn_sched_barrier(0);
      store_stage(buf ^ 1, ra0, rb0);
      __syncthreads();
    }
    if (s < nstages) {
      compute_stage(s & 1);
      __syncthreads();
    }
  } else if constexpr (TILE == 64) {
    // Software pipelining across the stage barrier: the fragments of a whole stage live in registers, the LDS stores of
    // the next stage are issued before the last-but-one k-step and the first fragments of the next stage are read
    // right after the barrier, under the MFMAs of the last k-step -- so neither the store latency nor the first read
    // latency sits between a barrier and an MFMA.  Measured: 64.7 -> 66.9 TFLOP/s at 3 workgroups per CU, 64.0 -> 66.5
    // at 2, 55.0 -> 61.5 at 1; the 32-tile loses with it (55.0 -> 52.9).
    constexpr int NK = BK / 4;
    T fa[NK][TM], fb[NK][TM];
    auto read_frags = [&](int buf, int k4) {
      const int ia = buf * G::LDSE + fa0 + k4 * 4 * skA, ib = buf * G::LDSE + fb0 + k4 * 4 * skB;
#pragma unroll
      for (int a = 0; a < TM; ++a) fa[k4][a] = lds[ia + a * 16 * soA];
#pragma unroll
      for (int b2 = 0; b2 < TM; ++b2) fb[k4][b2] = lds[ib + b2 * 16 * soB];
    };
    auto mfma_step = [&](int k4) {
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b2 = 0; b2 < TM; ++b2) acc[a][b2] = C::mfma(fa[k4][a], fb[k4][b2], acc[a][b2]);
    };
    // one stage; `cur` = LDS buffer of this stage.  On entry fa/fb[0] hold its first k-step.
    auto stage = [&](int cur, bool do_load, vec_t (&la)[NCH], vec_t (&lb)[NCH], bool do_store, vec_t (&sa)[NCH],
                     vec_t (&sb)[NCH], bool has_next) {
      if (do_load) load_stage(la, lb);
#pragma unroll
      for (int k4 = 1; k4 < NK; ++k4) read_frags(cur, k4);
#pragma unroll
      for (int k4 = 0; k4 + 2 < NK; ++k4) mfma_step(k4);
      __builtin_amdgcn_sched_barrier(0);
      if (do_store) store_stage(cur ^ 1, sa, sb);
      if (NK >= 2) mfma_step(NK - 2);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
      // fragments of k-step NK-1 are still needed: the next stage's first fragments go to slot 0
      if (has_next) read_frags(cur ^ 1, 0);
      mfma_step(NK - 1);
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * TM, 0);  // reads first: their latency hides under the MFMAs
      __builtin_amdgcn_sched_group_barrier(0x008, TM * TM, 0);
      __builtin_amdgcn_sched_barrier(0);
      static_assert(!CHUNKED || F32_CHUNK % BK == 0, "f32 64-tile: an accumulation chunk is a whole number of stages");
      kabs += BK;
      if (CHUNKED && kabs % F32_CHUNK == 0) flush();
    };
    if (nstages > 0) {
      load_stage(ra0, rb0);
      if (nstages > 1) load_stage(ra1, rb1);
      store_stage(0, ra0, rb0);
      __syncthreads();
      read_frags(0, 0);
      int s = 0;
      for (; s + 3 < nstages; s += 2) {
        stage(0, true, ra0, rb0, true, ra1, rb1, true);
        stage(1, true, ra1, rb1, true, ra0, rb0, true);
      }
      const int left = nstages - s;  // 1..3
      stage(0, left > 2, ra0, rb0, left > 1, ra1, rb1, left > 1);
      if (left > 1) stage(1, false, ra1, rb1, left > 2, ra0, rb0, left > 2);
      if (left > 2) stage(0, false, ra0, rb0, false, ra1, rb1, false);
      __syncthreads();  // the next tile of this workgroup overwrites LDS
    }
  } else {
    // prologue: stage 0 -> LDS buffer 0, stage 1 -> register set 1
    if (nstages > 0) {
      load_stage(ra0, rb0);
      if (nstages > 1) load_stage(ra1, rb1);
      store_stage(0, ra0, rb0);
    }
    __syncthreads();
    // steady state, unrolled by two so that the register sets are indexed statically:
    //   even s: loads(s+2) -> set 0 | compute LDS[0] | set 1 (stage s+1) -> LDS[1] | barrier
    //   odd  s: loads(s+2) -> set 1 | compute LDS[1] | set 0 (stage s+1) -> LDS[0] | barrier
    // Two things keep the loads two stages ahead of their use in the generated code:
    //  * the steady-state loop issues its loads unconditionally (the last stages are peeled off below): a load under an
    //    `if` makes hipcc's wait-count insertion assume the no-load path and emit vmcnt(0) before the LDS stores, i.e.
    //    wait for the loads issued a moment ago;
    //  * the scheduling fences keep it from hoisting the LDS stores (and their vmcnt wait) above the stage's MFMAs.
    // Left alone the exposed load latency costs 11 % (3 workgroups per CU) to 20 % (1 per CU) of the MFMA rate.
    int s = 0;
    for (; s + 3 < nstages; s += 2) {
      load_stage(ra0, rb0);
      compute_stage(0);
      __builtin_amdgcn_sched_barrier(0);
      store_stage(1, ra1, rb1);
      __syncthreads();
      load_stage(ra1, rb1);
      compute_stage(1);
      __builtin_amdgcn_sched_barrier(0);
      store_stage(0, ra0, rb0);
      __syncthreads();
    }
    // tail: 1..3 stages left (0 if the tile has none); LDS[0] holds stage s, register set 1 holds stage s+1
    if (s < nstages) {
      const int left = nstages - s;
      if (left > 2) load_stage(ra0, rb0);
      compute_stage(0);
      __builtin_amdgcn_sched_barrier(0);
      if (left > 1) store_stage(1, ra1, rb1);
      __syncthreads();
      if (left > 1) {
        compute_stage(1);
        __builtin_amdgcn_sched_barrier(0);
        if (left > 2) store_stage(0, ra0, rb0);
        __syncthreads();
        if (left > 2) {
          compute_stage(0);
          __syncthreads();
        }
      }
    }
  }

  // epilogue
  flush();  // f32: what the last (partial) chunk holds
  if (bad != 0) return;
  T* Cg = static_cast<T*>(op.C);
  const int row0 = ti * TILE + wm * (TILE / 2), col0 = tj * TILE + wn * (TILE / 2) + (lane & 15);
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + a * 16 + C::crow(lane, r);
        T* p = Cg + (size_t)row * op.ldc + col0 + b * 16;
        T v;
        if constexpr (CHUNKED) v = (T)tot[a][b][r];
        else v = acc[a][b][r];
        if (op.alpha_neg) v = -v;
        if (op.beta_one) v += *p;
        *p = v;
      }
  }  // work list
}

template <typename T, int TILE>
static void launch_gemm_t(const GemmLaunch& gl, hipStream_t s) {
  using G = GemmGeom<T, TILE>;
  GemmLaunch g = gl;
  int total = 0;
  for (int i = 0; i < g.nops; ++i) {
    GemmOp& op = g.op[i];
    op.ntiles = op.c_lower ? op.mi * (op.mi + 1) / 2 : op.mi * op.nj;
    // heaviest tiles first: contraction depth grows with tj (klim 1) or ti (klim 3) -> walk those tile lists backwards
    op.reverse = (op.klim == 1 || op.klim == 3) ? 1 : 0;
    total += op.ntiles;
  }
  if (g.sched_off) total = g.sched_nwg;
  if (total <= 0) return;
  size_t lds = (size_t)4 * G::LDSE * sizeof(T);
  // Static schedules assume exactly sched_nwg / 256 workgroups on every CU: pin that residency by asking for the matching
  // share of the 160 KiB LDS (otherwise the dispatcher may stack 3 workgroups on some CUs and 1 on others).
  if (g.sched_off && g.sched_nwg >= 256) {
    const size_t share = ((size_t)163840 / (size_t)(g.sched_nwg / 256)) / 4096 * 4096;  // LDS is allocated in coarse granules
    if (share > lds) lds = share;
  }
  hipLaunchKernelGGL((gemm_kernel<T, TILE>), dim3(total), dim3(256), lds, s, g);
}

// ops are specified in NB(=128)-tile units by the host; rescale to the launch tile size here.
template <typename T>
void launch_gemm(const GemmLaunch& gl, int tile, hipStream_t s) {
  GemmLaunch g = gl;
  const int f = NB / tile;
  for (int i = 0; i < g.nops; ++i) {
    GemmOp& op = g.op[i];
    op.ci0 *= f; op.cj0 *= f; op.mi *= f; op.nj *= f; op.k0 *= f; op.k1 *= f;
  }
  if (tile == 128) launch_gemm_t<T, 128>(g, s);
  else if (tile == 64) launch_gemm_t<T, 64>(g, s);
  else launch_gemm_t<T, 32>(g, s);
}
template void launch_gemm<double>(const GemmLaunch&, int, hipStream_t);
template void launch_gemm<float>(const GemmLaunch&, int, hipStream_t);

// =================================================================================================================
// Leaf: 128x128 diagonal block.  L = chol(A) (lower), X = L^-1.
// =================================================================================================================
template <typename T>
struct LeafGeom {
  static constexpr int S = 130;          // LDS row stride of the block image (and of the image of the 16x16 inverses)
  static constexpr int YS = 18;          // row stride of a 16x16 scratch image
  static constexpr int YB = 16 * YS;     // elements per 16x16 scratch image
  static constexpr size_t LDS_BYTES = (size_t)(128 * S + 16 * S + 4 * YB + 128) * sizeof(T);  // 160,000 B for f64
};

// ---- static item tables of the diagonal block's MFMA waves (see leaf_body) ---------------------------------------------------
// Every 16x16x16 product the block needs is known in advance.  Per phase p the products of panels k = p-1 and k2 = p-2 are
// listed class by class; an entry is four words {a, b, c, x}: byte offsets (LDS, from the block image) of the A operand, the B
// operand and the result block, and one more number.  A wave reads an entry with ONE broadcast LDS read and adds its lane
// pattern -- no scalar decoding, no class switch inside a loop: one wave issues one instruction per ~4.5 cycles whatever its kind,
// so an item must stay below ~50 instructions to keep up with its four MFMAs (256 cycles of the SIMD's matrix pipe).
//   F(j):      X[k,j] = -Y_k S[k,j], j < k         {j, S^T block (j,k), same, byte offset of column block j in a row of X}
//   U(i,j):    A[i,j] -= L[i,k] L[j,k]^T           {L block (i,k), L block (j,k), block (i,j), 0},   p+1 <= j <= i <= 7
//   G(i,j):    S[i,j] += L[i,k2] X[k2,j]           {L block (i,k2), X^T block (j,k2) or Yt_k2, S^T block (j,i), 0},  i >= p+1, j <= k2
//   GU1(j):    S[p,j] += L[p,k2] X[k2,j], j <= k2  (as G)
//   GU2(j):    S[p,j] += L[p,k] X[k,j],  j <= k    (as G; for j < k it waits for F(j)'s flag)
constexpr int LEAF_S = 130;
constexpr int LEAF_YT0 = 128 * LEAF_S;       // element offset of the image of the transposed 16x16 inverses: Y_q[r][c] at YT0 + c S + 16 q + r
constexpr int LEAF_MAXITEMS = 26;
struct LeafItemTab {
  unsigned e[8][LEAF_MAXITEMS][4];
  unsigned par[8][8][4];  // [phase][wave]: {first item of this wave in the F | U << 8 | G << 16 | GU << 24 list, number of MFMA waves, 0, 0}
};
constexpr int LEAF_TAB_WORDS = 8 * LEAF_MAXITEMS * 4 + 8 * 8 * 4;
constexpr unsigned leaf_blk_bytes(int i, int j) { return (unsigned)(((i * 16) * LEAF_S + j * 16) * 8); }
constexpr unsigned leaf_yt_bytes(int q) { return (unsigned)((LEAF_YT0 + 16 * q) * 8); }
// list sizes and offsets inside a phase's row (closed forms: leaf_body uses them instead of loading counts)
constexpr int leaf_nf(int p) { return p - 1; }
constexpr int leaf_nu(int p) { return (7 - p) * (8 - p) / 2; }
constexpr int leaf_ng(int p) { return p >= 2 ? (7 - p) * (p - 1) : 0; }
constexpr int leaf_ngu1(int p) { return p - 1; }
constexpr int leaf_ngu2(int p) { return p; }
constexpr LeafItemTab leaf_build_items(int xcol_bytes) {
  LeafItemTab t{};
  for (int p = 1; p < 8; ++p) {
    const int k = p - 1, k2 = p - 2;
    int n = 0;
    for (int j = 0; j < k; ++j, ++n) {
      t.e[p][n][0] = (unsigned)j; t.e[p][n][1] = leaf_blk_bytes(j, k); t.e[p][n][2] = leaf_blk_bytes(j, k); t.e[p][n][3] = (unsigned)(j * xcol_bytes);
    }
    for (int i = p + 1; i < 8; ++i)
      for (int j = p + 1; j <= i; ++j, ++n) {
        t.e[p][n][0] = leaf_blk_bytes(i, k); t.e[p][n][1] = leaf_blk_bytes(j, k); t.e[p][n][2] = leaf_blk_bytes(i, j);
      }
    if (k2 >= 0)
      for (int i = p + 1; i < 8; ++i)
        for (int j = 0; j <= k2; ++j, ++n) {
          t.e[p][n][0] = leaf_blk_bytes(i, k2); t.e[p][n][1] = j == k2 ? leaf_yt_bytes(k2) : leaf_blk_bytes(j, k2); t.e[p][n][2] = leaf_blk_bytes(j, i);
        }
    for (int j = 0; j <= k2; ++j, ++n) {
      t.e[p][n][0] = leaf_blk_bytes(p, k2); t.e[p][n][1] = j == k2 ? leaf_yt_bytes(k2) : leaf_blk_bytes(j, k2); t.e[p][n][2] = leaf_blk_bytes(j, p);
    }
    for (int j = 0; j <= k; ++j, ++n) {
      t.e[p][n][0] = leaf_blk_bytes(p, k); t.e[p][n][1] = j == k ? leaf_yt_bytes(k) : leaf_blk_bytes(j, k); t.e[p][n][2] = leaf_blk_bytes(j, p);
    }
    t.e[p][LEAF_MAXITEMS - 1][3] = (unsigned)n;  // for the consistency check below only
    // Round-robin dealing of the phase's items to its MFMA waves, continuing across the lists: waves 1, 2, 3, 5, 7 while wave 6
    // is the helper (p < 4), then 1, 2, 3, 5, 6, 7; wave 4 (it shares a SIMD with the eliminating wave 0) comes last.  The
    // first item of every wave in every list is tabulated: no division at run time (an integer modulo costs ~30
    // instructions -- more than half an item).  Wave 4 slows wave 0's elimination by a fifth (2370 -> 2870-3140 cycles), but
    // the MFMA items are what a phase waits for: 25.8 -> 24.7 us per block with it.
    const int nw = p < 4 ? 6 : 7;
    const int starts[4] = {0, leaf_nf(p), leaf_nf(p) + leaf_nu(p), leaf_nf(p) + leaf_nu(p) + leaf_ng(p)};  // GU: its own numbering (j)
    for (int w = 0; w < 8; ++w) {
      const int widx = w <= 3 ? w - 1 : (w == 4 ? nw - 1 : (w == 5 ? 3 : (p < 4 ? 4 : w - 2)));
      unsigned packed = 0;
      for (int l = 0; l < 4; ++l) {
        int f = widx - starts[l] % nw;
        if (f < 0) f += nw;
        packed |= (unsigned)(widx < 0 ? 255 : f) << (8 * l);
      }
      t.par[p][w][0] = packed;
      t.par[p][w][1] = (unsigned)nw;
    }
  }
  return t;
}
constexpr bool leaf_items_consistent() {
  const LeafItemTab t = leaf_build_items(128);
  for (int p = 1; p < 8; ++p) {
    const int n = leaf_nf(p) + leaf_nu(p) + leaf_ng(p) + leaf_ngu1(p) + leaf_ngu2(p);
    if ((int)t.e[p][LEAF_MAXITEMS - 1][3] != n || n > LEAF_MAXITEMS - 1) return false;
  }
  return true;
}
static_assert(leaf_items_consistent(), "item table sizes");
// copied into the LDS by every block (a scalar load from HBM per item would cost more than the item); one table per element type
// of X in HBM (the F items carry the byte offset of a column block)
__device__ const LeafItemTab g_leaf_items_f64 = leaf_build_items(16 * 8);
__device__ const LeafItemTab g_leaf_items_f32 = leaf_build_items(16 * 4);

// ---- lane broadcasts inside a 16-lane row, fused into the fp64 FMA (round 4) ------------------------------------------------
// gfx950 carries DPP for the double-precision ALU with one control: row_newbcast:n = "lane n of my 16-lane row".  With the 16
// pivot rows of a panel replicated in every 16-lane row of the wave, the multiplier l_jk every lane needs at pivot k is lane j of
// its own row: the trailing update a_ij -= l_ik l_jk is ONE v_fmac_f64_dpp (4.7 cycles issue, tools/leaf_ubench) where rounds 1-3
// spent two v_readlane_b32 + s_nop + v_fma_f64 (20 cycles) -- the elimination's instruction stream shrinks 2.5x.
// The compiler knows nothing about what is inside an asm statement, in particular not that a DPP operand read needs two wait
// states behind the VALU write of that register (CDNA3 ISA 4.5): every value that is read through DPP is therefore produced by
// mul_then_gap() / consumed by row_bcast_safe(), which carry the wait states inside their own asm text.
template <int J>
__device__ __forceinline__ void fmac_nbc(double& d, double s0, double s1) {  // d -= (lane J of my row: s0) * s1
  asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(s0), "v"(s1), "n"(J));
}
template <int K>
__device__ __forceinline__ double row_bcast_safe(double v) {  // lane K of my row's v; v may have been written by the previous instruction
  double r;
  asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(K));
  return r;
}
__device__ __forceinline__ double mul_then_gap(double a, double b) {  // a * b, safe to read through DPP right behind it
  double r;
  asm("v_mul_f64 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// One 16-column panel in registers.  a[]: the panel's 16 pivot rows, lane l holds row l & 15 (four replicas per wave);
// b[]: 64 more rows of the panel, one per lane (rows below the pivot block, or rows of the identity).  At pivot K every lane
// forms 1/sqrt(pivot) itself (the pivot is lane K of its row), scales its two columns K and applies the rank-1 update to the
// columns behind.  A row of b ends as b L_pp^-T: a row below the pivot block becomes its row of L, row r of the identity becomes
// column r of Y = L_pp^-1 (exact zeros above the diagonal) -- the inverse of the 16x16 factor costs no instruction of its own.
// Entries above the diagonal of the pivot block only ever feed themselves: no per-lane predicates.
// 1/sqrt(piv): hardware estimate (5e-8) + one third-order step r (1 + e/2 + 3e^2/8), e = 1 - piv r^2: 1.4e-16, the same as two
// Newton steps (tools/rsq_probe.hip) in 5 dependent operations instead of 8.  A pivot that is not positive (or NaN) gives NaN for
// its column and everything behind it: the caller tests the diagonal of L once, at the end.
template <int K, int J>
struct LeafCol {
  static __device__ __forceinline__ void run(double (&a)[16], double (&b)[16], double lka, double lkb) {
    fmac_nbc<J>(a[J], lka, lka);
    fmac_nbc<J>(b[J], lka, lkb);
    LeafCol<K, J + 1>::run(a, b, lka, lkb);
  }
};
template <int K>
struct LeafCol<K, 16> {
  static __device__ __forceinline__ void run(double (&)[16], double (&)[16], double, double) {}
};
template <int K>
struct LeafPivot {
  static __device__ __forceinline__ void run(double (&a)[16], double (&b)[16]) {
    const double piv = row_bcast_safe<K>(a[K]);
    double rinv = __builtin_amdgcn_rsq(piv);
    {
      const double gg = piv * rinv;
      const double ee = __builtin_fma(-gg, rinv, 1.0);
      const double pp = __builtin_fma(ee, 0.375, 0.5);
      rinv = __builtin_fma(rinv, ee * pp, rinv);
    }
    const double lka = mul_then_gap(a[K], rinv);  // l_{row,K} (pivot row: sqrt(piv))
    const double lkb = b[K] * rinv;
    a[K] = lka;
    b[K] = lkb;
    LeafCol<K, K + 1>::run(a, b, lka, lkb);
    LeafPivot<K + 1>::run(a, b);
  }
};
template <>
struct LeafPivot<16> {
  static __device__ __forceinline__ void run(double (&)[16], double (&)[16]) {}
};

// Structure (8 panels of 16 columns, two barrier-separated phases per panel p):
//   (A) wave 0 eliminates the panel in registers (LeafPivot): pivot rows 16p..16p+15 replicated four times, plus the next (up to)
//       64 rows.  While rows remain beyond that window (p < 4) one helper wave (wave 6) runs the SAME elimination -- redundantly,
//       bitwise the same -- with the remaining rows, so they are ready together with the window without any communication.  The
//       first 16 spare lanes of the helper (p < 4) or of wave 0 (p >= 4) carry the rows of the identity: Y_p = L_pp^-1.
//       Meanwhile the other waves pull 16x16x16 MFMA items of panel p-1 from a pool (an LDS counter; an item's arithmetic does not
//       depend on who runs it): the rest of the trailing update, and the inverse X = L^-1 in right-looking form --
//         F(j):   X[k,j] = -Y_k S[k,j]            (block row k = p-1 of X is final)
//         G(i,j): S[i,j] += L[i,k] X[k,j], i > k  (every later block row collects its sum as soon as a term exists)
//       so that behind the last panel only X[7,j] = -Y_7 S[7,j] is left (rounds 1-3 formed whole block rows of X at the end:
//       4,900 of the block's 53,000 cycles).  S[i,j] and later X[i,j] live TRANSPOSED in the strict upper blocks of the image,
//       which is exactly the layout of an MFMA B operand: nothing is staged through a scratch image.
//   (B) block column p+1 is updated for every remaining block row (one 16x16 block per wave).
// fp64 MFMA for every 16x16x16 product, two accumulator chains per product (a dependent v_mfma_f64_16x16x4 issues every 66
// cycles, tools/leaf_ubench).  Block indices are wave-uniform (scalar registers); a lane's part of every address is one of four
// constants.
// T = arithmetic type of the block (always double: the block is latency-bound, so f32 problems are factored in f64 too),
// TIO = element type in HBM.
__device__ long long g_leaf_stamps[256];
#define LEAF_STAMP(i) do { if ((dbg & 8) && t == 0) g_leaf_stamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
void read_leaf_stamps(long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_leaf_stamps), sizeof(long long) * 256); }

// Results another workgroup of the SAME launch will read (the task-queue kernel, dag_kernel.inc.hpp) are stored
// write-through (sc1) so that they need no release fence; between launches plain stores do.
template <bool SC1, typename TIO>
__device__ __forceinline__ void gstore(TIO* p, TIO v) {
  if constexpr (SC1) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// FROM_LDS: the block image is in the LDS already (lower 16x16 blocks valid, strict upper blocks zero; the caller has met at a
// barrier): small_eval_kernel assembles the kernel matrix there and never writes it to HBM.
template <typename T, typename TIO, bool SC1, bool FROM_LDS = false>
__device__ __forceinline__ void leaf_body(TIO* __restrict__ W1, TIO* __restrict__ W2, int ld, int blk,
                                          TIO* __restrict__ ldiag, int* info, int dbg, char* smem_raw) {
  static_assert(sizeof(T) == 8, "the diagonal block is factored in fp64");
  using C = Cfg<T>;
  using L = LeafGeom<T>;
  using acc_t = typename C::acc_t;
  using vec_t = typename Cfg<TIO>::vec_t;
  constexpr int S = L::S, YS = L::YS, YB = L::YB, VEC = Cfg<TIO>::VEC;

  T* As = reinterpret_cast<T*>(smem_raw);  // [128][S]: lower = A -> L ; strict upper blocks = S^T -> X^T
  T* Yt = As + 128 * S;                    // [16][S]: TRANSPOSED inverses of the diagonal 16x16 factors, Y_q[r][c] at Yt[c * S + 16 q + r]
  static_assert(S == LEAF_S, "the item tables are built for this row stride");
  T* Sc = Yt + 16 * S;                     // [16][YS]: copy of the next panel's pivot block for the helper wave
  T* Id = Sc + YB;                         // [17][YS]: the identity (rows 0-15) and a row of zeros (row 16)
  int* pool = reinterpret_cast<int*>(Id + 17 * YS + 2);  // [8]: flags of the F items (+ 8 spare)
  unsigned* tab = reinterpret_cast<unsigned*>(pool + 16);  // the item tables (g_leaf_items_*), 16-byte aligned
  static_assert(((128 * S + 16 * S + YB + 17 * YS + 2) * sizeof(T) + 64) % 16 == 0, "item table alignment");
  static_assert((YB + 17 * YS + 2) * sizeof(T) + 64 + LEAF_TAB_WORDS * 4 <= (4 * YB + 128) * sizeof(T), "the scratch region holds the item tables");

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);  // wave-uniform on purpose: block indices stay in scalar registers
  const int m16 = lane & 15, q4 = lane >> 4;
  const size_t g0 = (size_t)blk * NB * ld + (size_t)blk * NB;
  TIO* Ablk = W1 + g0;
  TIO* Xblk = W2 + g0;

  // Load the lower 16x16 blocks of the block; the strict upper blocks start as zeros (they will hold the sums S^T of the
  // inverse).  Wave w takes block row w (rows 16w .. 16w+15, four threads per row): the trip count is wave-uniform, and all
  // loads of a thread are issued before its first LDS store.
  if constexpr (!FROM_LDS) {
    const int r = t >> 2, sub = t & 3;           // row, position among the row's four threads
    constexpr int CPR = 16 / VEC;                // 16-byte chunks per 16 columns
    const int nch = (wave + 1) * CPR / 4;        // chunks of this thread: columns [0, 16 (wave + 1)) of its row, interleaved by 4
    const TIO* src = Ablk + (size_t)r * ld + sub * VEC;
    T* dst = As + r * S + sub * VEC;
    constexpr int MAXCH = 8 * CPR / 4;
    vec_t buf[MAXCH];
#pragma unroll
    for (int q = 0; q < MAXCH; ++q)
      if (q < nch) buf[q] = *reinterpret_cast<const vec_t*>(src + q * 4 * VEC);
#pragma unroll
    for (int q = 0; q < MAXCH; ++q) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) dst[q * 4 * VEC + e] = q < nch ? (T)buf[q][e] : T(0);
    }
  }
  // the first diagonal 16x16 block once more, into Sc: the helper wave takes the pivot rows from there (see the elimination)
  if (t < 256) {
    if constexpr (FROM_LDS) Sc[(t >> 4) * YS + (t & 15)] = As[(t >> 4) * S + (t & 15)];
    else Sc[(t >> 4) * YS + (t & 15)] = (T)Ablk[(size_t)(t >> 4) * ld + (t & 15)];
  } else {
    for (int e = t - 256; e < 17 * 16; e += 256) Id[(e >> 4) * YS + (e & 15)] = ((e >> 4) == (e & 15)) ? T(1) : T(0);
    if (t < 256 + 16) pool[t - 256] = 0;  // the F flags
  }
  {
    const unsigned* gt = reinterpret_cast<const unsigned*>(sizeof(TIO) == 8 ? &g_leaf_items_f64 : &g_leaf_items_f32);
    for (int e = t; e < LEAF_TAB_WORDS; e += 512) tab[e] = gt[e];
  }
  __syncthreads();

  LEAF_STAMP(0);
  // ---- 16x16x16 MFMA items on 16x16 blocks of the LDS image.  A lane adds one of two patterns to an entry's byte offsets:
  //   P0 = row m16 of the block, element q4 (+ 4 per step): operands stored [outer][k], and a TRANSPOSED result
  //   P1 = row q4 (+ 4 per step), column m16: a result in normal orientation (U), and Y_q read from the Yt image as an A operand (F)
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  const int P0 = (m16 * S + q4) * (int)sizeof(T), P1 = (q4 * S + m16) * (int)sizeof(T);
  constexpr int STEP0 = 4 * (int)sizeof(T), STEP1 = 4 * S * (int)sizeof(T);
  constexpr int CLS_U = 0, CLS_G = 1, CLS_F = 2;
  char* lds0 = reinterpret_cast<char*>(As);
  int* fflag = pool;  // [8]: fflag[j] = p once F(j) of phase p has written X[p-1, j]
  auto ldsT = [&](int byte_off) -> T& { return *reinterpret_cast<T*>(lds0 + byte_off); };
  // An item in two halves, so that two items can be in flight in one wave: issue = operand loads + the four MFMAs on two
  // accumulator chains (a dependent v_mfma_f64_16x16x4 issues every 66 cycles), finish = combine, store.
  struct Prod {
    T cf[4];
    acc_t a0, a1;
  };
  // ya: byte offset of Y_k in the Yt image (F items: their A operand)
  auto item_issue = [&](auto cls, const u4 d, int ya, Prod& pr) {
    constexpr int CLS = decltype(cls)::value;
    T af[4], bf[4];
    if constexpr (CLS == CLS_F) {
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) af[k4] = ldsT(ya + P1 + k4 * STEP1);
    } else {
      const int pa = (int)d[0] + P0;
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) af[k4] = ldsT(pa + k4 * STEP0);
    }
    const int pb = (int)d[1] + P0;
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) bf[k4] = ldsT(pb + k4 * STEP0);
    if constexpr (CLS == CLS_U) {
      const int pc = (int)d[2] + P1;
#pragma unroll
      for (int r = 0; r < 4; ++r) pr.cf[r] = ldsT(pc + r * STEP1);
    } else if constexpr (CLS == CLS_G) {
      const int pc = (int)d[2] + P0;
#pragma unroll
      for (int r = 0; r < 4; ++r) pr.cf[r] = ldsT(pc + r * STEP0);
    }
    pr.a0 = acc_t{0, 0, 0, 0};
    pr.a1 = acc_t{0, 0, 0, 0};
    pr.a0 = C::mfma(af[0], bf[0], pr.a0);
    pr.a1 = C::mfma(af[2], bf[2], pr.a1);
    pr.a0 = C::mfma(af[1], bf[1], pr.a0);
    pr.a1 = C::mfma(af[3], bf[3], pr.a1);
  };
  // xrow: F items, this lane's first element of block row k of X in HBM (row q4 of the block row, column m16); dcopy: the
  // result is the next panel's pivot block, the helper wave will eliminate it a second time: keep a copy in Sc
  auto item_finish = [&](auto cls, const u4 d, const Prod& pr, TIO* xrow, bool dcopy) {
    constexpr int CLS = decltype(cls)::value;
    if constexpr (CLS == CLS_U) {
      const int pc = (int)d[2] + P1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T v = pr.cf[r] - (pr.a0[r] + pr.a1[r]);
        ldsT(pc + r * STEP1) = v;
        if (dcopy) Sc[(q4 + 4 * r) * YS + m16] = v;
      }
    } else if constexpr (CLS == CLS_G) {
      const int pc = (int)d[2] + P0;
#pragma unroll
      for (int r = 0; r < 4; ++r) ldsT(pc + r * STEP0) = pr.cf[r] + (pr.a0[r] + pr.a1[r]);
    } else {
      const int pc = (int)d[2] + P0;
      TIO* xp = reinterpret_cast<TIO*>(reinterpret_cast<char*>(xrow) + d[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T v = -pr.a0[r] - pr.a1[r];
        ldsT(pc + r * STEP0) = v;  // in place of S^T: every lane's operand reads are complete, the products have consumed them
        gstore<SC1>(xp + (size_t)(4 * r) * ld, (TIO)v);
      }
    }
  };
  using cU = std::integral_constant<int, CLS_U>;
  using cG = std::integral_constant<int, CLS_G>;
  using cF = std::integral_constant<int, CLS_F>;
  auto xrow_of = [&](int k) { return Xblk + (size_t)(k * 16 + q4) * ld + m16; };
  // Phase A(p) of the MFMA waves: the products of panels k = p-1 and k2 = p-2, class by class --
  //   F(j,k), j < k                       block row k of X is final (sets fflag[j] = p)
  //   U(i,j,k), p+1 <= j <= i <= 7        the rest of the trailing update of panel k
  //   G(i,j,k2), i >= p+1, j <= k2        the sums of the later block rows collect the terms of block row k2 of X (final since
  //                                       the previous phase; one phase late, so that they wait for nothing)
  //   GU(j), j <= k                       S[p,j] += L[p,k2] X[k2,j] and += L[p,k] X[k,j]: block row p is finalised in the NEXT
  //                                       phase, so its last term cannot be late -- it waits for F(j,k)'s flag instead
  // Items are dealt round-robin to the MFMA waves, continuing across the lists (an LDS atomic per claim cost ~300 cycles with
  // six waves asking at once -- more than an item; the dealing is tabulated, LeafItemTab::par).  F, U and G items are independent of one another: a wave keeps two of them in flight.  Every wave runs its F items
  // before its GU items, so a wait for an F flag always ends.
  auto pool_phase = [&](int p) {
    const int k = p - 1;
    // this wave's first item in each list and the number of MFMA waves: one broadcast read of the phase's parameter record
    const u4 par = *reinterpret_cast<const u4*>(tab + 8 * LEAF_MAXITEMS * 4 + (p * 8 + wave) * 4);
    const unsigned firsts = (unsigned)__builtin_amdgcn_readfirstlane((int)par[0]);
    const int nworkers = __builtin_amdgcn_readfirstlane((int)par[1]);
    const u4* tabp = reinterpret_cast<const u4*>(tab) + p * LEAF_MAXITEMS;
    const int ya = (int)leaf_yt_bytes(0) + k * 16 * (int)sizeof(T);
    TIO* xrow = xrow_of(k);
    auto first_of = [&](int list) { return (int)((firsts >> (8 * list)) & 255u); };
    auto run_list = [&](auto cls, int list, int o, int n) {
      const int first = first_of(list);
      for (int i = first; i < n; i += 2 * nworkers) {
        const bool two = i + nworkers < n;
        const u4 d0 = tabp[o + i];
        const u4 d1 = tabp[o + (two ? i + nworkers : i)];
        Prod p0, p1;
        item_issue(cls, d0, ya, p0);
        if (two) item_issue(cls, d1, ya, p1);
        item_finish(cls, d0, p0, xrow, false);
        if (two) item_finish(cls, d1, p1, xrow, false);
        if constexpr (decltype(cls)::value == CLS_F) {  // publish the columns: the last term of S[p, j] waits for them
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (lane == 0) {
            __hip_atomic_store(&fflag[d0[0]], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (two) __hip_atomic_store(&fflag[d1[0]], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
    };
    const bool inv = !(dbg & 2);  // timing switches of tools/leaf_bench: dbg 2 = no inverse, dbg 4 = no trailing update
    if ((dbg & 8) && lane == 0) g_leaf_stamps[64 + (p * 8 + wave) * 2] = (long long)__builtin_readcyclecounter();
    int o = 0;
    if (inv) run_list(cF{}, 0, o, leaf_nf(p));
    o += leaf_nf(p);
    if (!(dbg & 4)) run_list(cU{}, 1, o, leaf_nu(p));
    o += leaf_nu(p);
    if (inv) run_list(cG{}, 2, o, leaf_ng(p));
    o += leaf_ng(p);
    if (inv) {
      const int o1 = o, o2 = o + leaf_ngu1(p);
      for (int j = first_of(3); j < p; j += nworkers) {
        Prod pr;
        if (j <= p - 2) {  // the term of k2
          const u4 d = tabp[o1 + j];
          item_issue(cG{}, d, ya, pr);
          item_finish(cG{}, d, pr, xrow, false);
        }
        if (j < k) {
          while (__hip_atomic_load(&fflag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != p) __builtin_amdgcn_s_sleep(1);
          asm volatile("" ::: "memory");
        }
        const u4 d = tabp[o2 + j];  // the term of k: same result block (LDS accesses of one wave stay in order)
        item_issue(cG{}, d, ya, pr);
        item_finish(cG{}, d, pr, xrow, false);
      }
    }
    if ((dbg & 8) && lane == 0) g_leaf_stamps[65 + (p * 8 + wave) * 2] = (long long)__builtin_readcyclecounter();
  };
  auto blk_bytes = [&](int i, int j) { return (unsigned)(((i * 16) * S + j * 16) * (int)sizeof(T)); };

  typedef T v2 __attribute__((ext_vector_type(2)));
  for (int p = 0; p < 8; ++p) {
    // Elimination of panel p.  Wave 0: the pivot rows and the (up to) 64 rows behind them.  While p < 4 there are 48 - 16p rows
    // beyond that window: the helper (wave 6) runs the SAME elimination on the pivot rows -- bitwise the same values -- with
    // those far rows in its b lanes, so they are ready together with the window.  The 16 lanes behind a wave's last row carry
    // the identity (helper for p < 4, wave 0 from p = 4 on) and end as the columns of Y_p.
    const bool helper = p < 4 && wave == 6;
    if (wave == 0 || helper) {
      if (!(dbg & 1)) {
        const int nrows = helper ? 48 - 16 * p : min(64, 112 - 16 * p);  // rows of the block in this wave's b lanes
        const int brow = 16 * p + 16 + (helper ? 64 : 0) + lane;        // the row of lane < nrows
        const bool has_y = helper || p >= 4;
        const int yr = lane - nrows;                                   // has_y: identity row of lanes nrows .. nrows + 15
        // dbg bit 4 (tests): the helper wave starts ~3 us late -- longer than wave 0's whole elimination.  Results must not
        // change: nothing a helper reads is written by another wave in this phase (tests/test_gpu_dag.py).
        if ((dbg & 16) && helper) {
          __builtin_amdgcn_s_sleep(127);
          asm volatile("" ::: "memory");
        }
        T a[16], b[16];
        {
          // Wave 0 overwrites the pivot rows with L at the end of this phase, and no barrier orders the helper's reads of them
          // before that: the helper takes them from the copy in Sc (written a phase earlier, behind a barrier) -- same values.
          const T* srca = helper ? Sc + m16 * YS : As + (16 * p + m16) * S + p * 16;
          // lanes without a row of the block: a row of the identity, or zeros
          const T* srcb = lane < nrows ? As + brow * S + p * 16 : Id + ((has_y && yr < 16) ? yr : 16) * YS;
#pragma unroll
          for (int j = 0; j < 16; j += 2) {
            const v2 va = *reinterpret_cast<const v2*>(srca + j);
            a[j] = va[0];
            a[j + 1] = va[1];
          }
#pragma unroll
          for (int j = 0; j < 16; j += 2) {
            const v2 vb = *reinterpret_cast<const v2*>(srcb + j);
            b[j] = vb[0];
            b[j + 1] = vb[1];
          }
        }
        LEAF_STAMP(40 + 3 * p);
        LeafPivot<0>::run(a, b);
        LEAF_STAMP(41 + 3 * p);
        if (lane < nrows || (has_y && yr < 16)) {
          // a row of the block -> its row of L; row yr of the identity -> column yr of Y_p = row yr of Yt[p]
          T* dst = lane < nrows ? As + brow * S + p * 16 : Yt + yr * S + p * 16;
#pragma unroll
          for (int j = 0; j < 16; j += 2) *reinterpret_cast<v2*>(dst + j) = v2{b[j], b[j + 1]};
        }
        if (!helper && lane < 16) {
          // the pivot block: L_pp (what lies above its diagonal is never read again)
          T* dst = As + (16 * p + lane) * S + p * 16;
#pragma unroll
          for (int j = 0; j < 16; j += 2) *reinterpret_cast<v2*>(dst + j) = v2{a[j], a[j + 1]};
        }
        LEAF_STAMP(42 + 3 * p);
      }
    } else if (p > 0) {
      // the other waves meanwhile
      pool_phase(p);
    }
    __syncthreads();
    LEAF_STAMP(1 + 2 * p);
    if (p == 7) break;
    if (dbg & 4) continue;

    // block column p+1 for every remaining block row (window rows from wave 0, far rows from the helper)
    if (p + 1 + wave < 8) {
      const u4 d = {blk_bytes(p + 1 + wave, p), blk_bytes(p + 1, p), blk_bytes(p + 1 + wave, p + 1), 0u};
      Prod pr;
      item_issue(cU{}, d, 0, pr);
      item_finish(cU{}, d, pr, nullptr, wave == 0 && p + 1 < 4);
    }
    __syncthreads();
    LEAF_STAMP(2 + 2 * p);
  }

  // ---------------- tail of the inverse: block row 7 of X ----------------
  if (!(dbg & 2)) {
    if (wave >= 1) {  // X[7,j] = -Y_7 S[7,j]: seven blocks, waves 1-7
      const int j = wave - 1;
      const u4 d = {(unsigned)j, blk_bytes(j, 7), blk_bytes(j, 7), (unsigned)(j * 16 * (int)sizeof(TIO))};
      Prod pr;
      item_issue(cF{}, d, (int)leaf_yt_bytes(7), pr);
      item_finish(cF{}, d, pr, xrow_of(7), false);
    }
    __syncthreads();
  }
  LEAF_STAMP(20);
  // diagonal sub-blocks of X
  for (int c = t; c < 8 * 256; c += 512) {
    const int pblk = c >> 8, r = (c >> 4) & 15, j = c & 15;
    gstore<SC1>(&Xblk[(size_t)(pblk * 16 + r) * ld + pblk * 16 + j], (TIO)Yt[j * S + 16 * pblk + r]);
  }
  // diag(L) (read by the alpha tasks of the same launch) and the positive-definite test: a pivot that was not positive has left
  // NaN on the diagonal from its column on
  if (t < 64) {
    const T dv0 = As[t * S + t], dv1 = As[(t + 64) * S + t + 64];
    gstore<SC1>(&ldiag[blk * NB + t], (TIO)dv0);
    gstore<SC1>(&ldiag[blk * NB + 64 + t], (TIO)dv1);
    const unsigned long long bad0 = __ballot(!(dv0 > T(0))), bad1 = __ballot(!(dv1 > T(0)));
    if (t == 0) pool[15] = (bad0 | bad1) != 0ull ? 1 : 0;  // small_eval_kernel reads it behind its next barrier
    if ((bad0 | bad1) != 0ull && t == 0) {
      const int first = bad0 != 0ull ? (int)__builtin_ctzll(bad0) : 64 + (int)__builtin_ctzll(bad1);
      atomicCAS(info, 0, 1 + blk * NB + (first & ~15));  // reported per 16-column panel, as rounds 1-3 did
    }
  }
}

template <typename T, typename TIO>
__global__ void __launch_bounds__(512, 2) leaf_kernel(TIO* __restrict__ W1, TIO* __restrict__ W2, int ld, int blk,
                                                   TIO* __restrict__ ldiag, int* info, int dbg) {
  if (*info != 0) return;
  extern __shared__ __align__(16) char smem_raw[];
  leaf_body<T, TIO, false>(W1, W2, ld, blk, ldiag, info, dbg, smem_raw);
}

template <typename T>
void launch_leaf(T* W1, T* W2, int ld, int blk, T* ldiag, int* info, hipStream_t s, int dbg) {
  hipLaunchKernelGGL((leaf_kernel<double, T>), dim3(1), dim3(512), LeafGeom<double>::LDS_BYTES, s, W1, W2, ld, blk, ldiag, info, dbg);
}
template void launch_leaf<double>(double*, double*, int, int, double*, int*, hipStream_t, int);
template void launch_leaf<float>(float*, float*, int, int, float*, int*, hipStream_t, int);

// =================================================================================================================
// Kernel-matrix assembly
// =================================================================================================================
// Matern map of matern_kernel.rs:65-80; nu2 = 2*nu in {1,3,5}; r = euclidean distance of length-scaled points.
// nu2 = 0 stands for nu = infinity, the squared-exponential kernel exp(-r^2/2): an extension the reference does not have
// (matern_kernel.rs:79 is unimplemented! for other nu); its oracle is sklearn's RBF (tests/golden/*_rbf.npz).
template <typename T>
__device__ __forceinline__ T matern_map(T r, int nu2) {
#pragma clang fp contract(off)
  if (nu2 == 0) return exp_nonpos(T(-0.5) * r * r);
  if (nu2 == 1) return exp_nonpos(-r);
  if (nu2 == 3) {
    const T k = r * T(1.7320508075688772);
    return (k + T(1)) * exp_nonpos(-k);
  }
  const T k = r * T(2.23606797749979);
  return __builtin_fma(k * k, T(1.0 / 3.0), T(1) + k) * exp_nonpos(-k);
}
// one entry of K from the squared scaled distance (matern_kernel.rs:37-81 x constant_kernel.rs x + noise on the diagonal, lml.rs:44)
template <typename T>
__device__ __forceinline__ T kmat_entry(T dist2, int nu2, T amp, T noise, bool diag) {
#pragma clang fp contract(off)
  const T v = amp * matern_map<T>(sqrt_nonneg(dist2), nu2);  // product_kernel.rs:37 (k1 * k2)
  return diag ? v + noise : v;
}
// a diagonal entry of K with the row's known noise variance: (c k(0) + s2) + v_i, one more rounding.  rvi = 0 (no variances)
// leaves the entry's bits as they are: it is positive.
template <typename T>
__device__ __forceinline__ T kmat_add_rv(T entry, T rvi) {
#pragma clang fp contract(off)
  return entry + rvi;
}

// the poison pattern run_eval looks for in outputs that were never written (a payload no arithmetic produces)
__device__ __forceinline__ void poison_out(EvalOut* out, int t) {
  const double nan = __longlong_as_double(0x7ff8000000005eedLL);
  if (t == 0) {
    out->lml = nan; out->yalpha = nan; out->logdet = nan;
    out->info = 0; out->n_warn = 0; out->done = 0;
  }
  if (t < MAXP) out->grad[t] = nan;
}
// One workgroup of 256 threads: parameters host -> device, poisoned result block, cleared task-queue control words.
__device__ __forceinline__ void eval_prologue(const EvalParams* __restrict__ P, const EvalPrologue& pro) {
  const int t = threadIdx.x;
  constexpr int PW = (int)(sizeof(EvalParams) / 8);
  static_assert(sizeof(EvalParams) % 8 == 0 && PW <= 256, "EvalParams is copied as 8-byte words by one workgroup");
  if (t < PW) reinterpret_cast<unsigned long long*>(pro.dP)[t] = reinterpret_cast<const unsigned long long*>(P)[t];
  poison_out(pro.out, t);
  int4* c4 = reinterpret_cast<int4*>(pro.ctrl);  // hipMalloc'd, a whole number of 16-byte words (hbegp.cpp: dag_ctrl_bytes)
  for (int i = t; i < pro.ctrl_words / 4; i += 256) c4[i] = int4{0, 0, 0, 0};
}

// ---- what kmat_kernel and gradtrace_kernel share (round 5) --------------------------------------------------------------
// Tiles of 64x64 entries; thread (tx = t&15, ty = t>>4) owns rows ty+16*r, cols 4*tx..4*tx+3.
//  * One workgroup per tile, dealt by the hardware dispatcher (which refills a CU the moment a workgroup leaves it).  Round 5
//    tried persistent workgroups fed through a software queue (one returning atomic on one queue word per tile):
//    2,080 grabs on one word cost more than the tiles (kmat 30 -> 45 us, gradtrace 48 -> 86 us alone, worse with more workgroups
//    per CU; profiles/r05_tail_kernels_queue.txt) -- removed.  Capping the occupancy through a larger LDS request (3 / 4 / 5 / 8
//    workgroups per CU, so that the dispatcher has tiles left to balance the end of the launch with) changed nothing either
//    (kmat 35.0 / 30.5 / 30.5 / 30.6 us, gradtrace 50.6 / 43.7 / 44.3 / 43.8 us): both kernels sit at ~64 % of the fp64 VALU issue
//    rate (kmat: ~75 fp64 instructions per entry, 8.4 M entries = 19 us at 100 %), bound by their sqrt / exp sequences.
//  * The j tile's features sit in the LDS so that a thread's four columns are ONE conflict-free 16-byte read (f32) or two
//    (f64: [k][half][tx][2] -- a 16-lane group then reads 256 contiguous bytes); the plain [k][64] layout made the f64 reads
//    2-way conflicted (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 45 % in kmat, 20 % in gradtrace, profiles/r04_pmc_sq.json).
template <typename T>
__device__ __forceinline__ int xj_index(int k, int col) {  // LDS element index of feature k of column `col` (0..63) of the j tile
  if constexpr (sizeof(T) == 8) return k * 64 + ((col >> 1) & 1) * 32 + (col >> 2) * 2 + (col & 1);
  else return k * 64 + col;
}
template <typename T>
__device__ __forceinline__ void read_xj4(const T* xj, int k, int tx, T (&b)[4]) {  // features k of columns 4 tx .. 4 tx + 3
  if constexpr (sizeof(T) == 8) {
    const d2 lo = *reinterpret_cast<const d2*>(xj + k * 64 + tx * 2), hi = *reinterpret_cast<const d2*>(xj + k * 64 + 32 + tx * 2);
    b[0] = lo[0]; b[1] = lo[1]; b[2] = hi[0]; b[3] = hi[1];
  } else {
    const f4 v = *reinterpret_cast<const f4*>(xj + k * 64 + tx * 4);
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
  }
}
// NU2: the Matern order at compile time (no branch per entry); tiles that lie wholly inside the n x n matrix skip the
// per-entry bounds tests.
template <typename T, int NU2>
__global__ void __launch_bounds__(256) kmat_kernel(const T* __restrict__ X, const T* __restrict__ rv, int n, int d, int np,
                                                   const EvalParams* __restrict__ P, T* __restrict__ W,
                                                   const int* info, EvalPrologue pro) {
  if (pro.dP) {
    // first kernel of an evaluation (engine.hpp, EvalPrologue): nothing has failed yet, `info` still holds the previous
    // evaluation's value and is not read; workgroup 0 prepares the device-side blocks for the kernels behind this one
    if (blockIdx.x == 0) eval_prologue(P, pro);
  } else if (*info != 0) {
    return;
  }
  extern __shared__ __align__(16) char smem_raw[];
  T* xi = reinterpret_cast<T*>(smem_raw);  // [d][64] scaled rows of the i tile (feature-major)
  T* xj = xi + (size_t)d * 64;             // [d] x 64 columns of the j tile, xj_index layout
  const int t = threadIdx.x;
  // the parameters once per workgroup: in an evaluation driven through pinned memory P is a host block, and every read of it is
  // an uncached round trip over the host link (per-thread reads made the launch 10 us longer at n=4096)
  __shared__ double sp[MAXP];
  if (t < d + 2) sp[t] = reinterpret_cast<const double*>(P)[t];
  static_assert(offsetof(EvalParams, noise) == 0 && offsetof(EvalParams, amp) == 8 && offsetof(EvalParams, ell) == 16, "EvalParams: noise, amp, ell[]");
  const int tx = t & 15, ty = t >> 4;
  typedef T vec4 __attribute__((ext_vector_type(4)));
  __syncthreads();
  {
    const int tile = blockIdx.x;
    const int li = tri_row(tile), lj = tile - li * (li + 1) / 2;
    const int i0 = li * 64, j0 = lj * 64;
    for (int e = t; e < 64 * d; e += 256) {
      const int row = e / d, k = e - row * d;
      const T ell = (T)sp[2 + k];  // A::from_f (matern_kernel.rs:50)
      const int gi = i0 + row, gj = j0 + row;
      xi[k * 64 + row] = (gi < n) ? X[(size_t)gi * d + k] / ell : T(0);  // matern_kernel.rs:51-60
      xj[xj_index<T>(k, row)] = (gj < n) ? X[(size_t)gj * d + k] / ell : T(0);
    }
    __syncthreads();
    T acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = T(0);
    for (int k = 0; k < d; ++k) {  // cdist accumulation order (matern_kernel.rs:274-278)
      T a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
      read_xj4<T>(xj, k, tx, b);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T df = a[r] - b[c];
          acc[r][c] += df * df;
        }
    }
    const T amp = (T)sp[1], noise = (T)sp[0];
    // rv (may be null): the rows' known noise variances.  In a diagonal tile the thread whose four columns hold row gi's diagonal
    // entry (column ty + 16 r of the tile: tx = that >> 2, c = ty & 3) loads rv[gi] and adds it there; nobody else reads rv.
    const bool dtile = li == lj;
    const bool rv_tile = rv != nullptr && dtile;
    if (i0 + 64 <= n && j0 + 64 <= n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + ty + 16 * r;
        vec4 out;
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = kmat_entry<T>(acc[r][c], NU2, amp, noise, dtile && gi == j0 + tx * 4 + c);
        if (rv_tile && ((ty + 16 * r) >> 2) == tx) {
          const T rvi = rv[gi];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c == (ty & 3)) out[c] = kmat_add_rv<T>(out[c], rvi);
        }
        *reinterpret_cast<vec4*>(W + (size_t)gi * np + j0 + tx * 4) = out;
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = i0 + ty + 16 * r;
      vec4 out;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int gj = j0 + tx * 4 + c;
        const T v = kmat_entry<T>(acc[r][c], NU2, amp, noise, gi == gj);
        out[c] = (gi < n && gj < n) ? v : ((gi == gj) ? T(1) : T(0));  // identity padding
      }
      if (rv_tile && ((ty + 16 * r) >> 2) == tx && gi < n) {  // never the padding's ones, never rv at an index >= n
        const T rvi = rv[gi];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c == (ty & 3)) out[c] = kmat_add_rv<T>(out[c], rvi);
      }
      *reinterpret_cast<vec4*>(W + (size_t)gi * np + j0 + tx * 4) = out;
    }
  }
}

template <typename T>
void launch_kmat(const T* X, const T* rv, int n, int d, int np, int nu2, const EvalParams* P, T* W, const int* info, hipStream_t s,
                 const EvalPrologue* pro) {
  const int nt = np / 64, ntiles = nt * (nt + 1) / 2;
  const size_t lds = (size_t)2 * d * 64 * sizeof(T);
  const dim3 grid(ntiles), block(256);
  const EvalPrologue pr = pro ? *pro : EvalPrologue{};
  switch (nu2) {
    case 0: hipLaunchKernelGGL((kmat_kernel<T, 0>), grid, block, lds, s, X, rv, n, d, np, P, W, info, pr); break;
    case 1: hipLaunchKernelGGL((kmat_kernel<T, 1>), grid, block, lds, s, X, rv, n, d, np, P, W, info, pr); break;
    case 3: hipLaunchKernelGGL((kmat_kernel<T, 3>), grid, block, lds, s, X, rv, n, d, np, P, W, info, pr); break;
    default: hipLaunchKernelGGL((kmat_kernel<T, 5>), grid, block, lds, s, X, rv, n, d, np, P, W, info, pr); break;
  }
}
template void launch_kmat<double>(const double*, const double*, int, int, int, int, const EvalParams*, double*, const int*, hipStream_t, const EvalPrologue*);
template void launch_kmat<float>(const float*, const float*, int, int, int, int, const EvalParams*, float*, const int*, hipStream_t, const EvalPrologue*);

// =================================================================================================================
// alpha = K^-1 y through the explicit inverse factor: w = X y, alpha = X^T w;  lml pieces (lml.rs:54-59)
// =================================================================================================================
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// block sum for 256 threads; result valid in thread 0. red: >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// What the LAST workgroup of a launch to finish does for the whole launch (the ticket pattern).  The L2s of the eight XCDs
// are not coherent with each other, and an agent-scope release fence writes back the whole L2 of the XCD (measured on config M:
// one per workgroup of the gradient launch doubled that launch, 138 -> 290 us, and slowed the other slots' task-queue
// launches by 10 %: it evicts their working set too).  So, as in the task-queue kernel: the few words a workgroup hands over
// (thread 0 writes them) are stored write-through (publish_f64), thread 0 drains them (s_waitcnt vmcnt(0)) and takes a ticket
// with a relaxed agent-scope atomic; the workgroup that draws the last ticket runs ONE agent-scope acquire (drops its CU's L1
// and the stale lines of its L2) and then sees everybody's words.  The ticket word is left at zero for the next launch.
// Returns true (uniformly) in the last workgroup.
__device__ __forceinline__ void publish_f64(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool last_workgroup(int* ticket) {
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = tk == (int)gridDim.x * (int)gridDim.y - 1;
    if (s_last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const bool last = s_last != 0;
  if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return last;
}

// w = X y (X lower triangular, row-major): w_i = sum_{k<=i} X[i][k] y[k]   (first half of alpha = X^T (X y), lml.rs:54)
// Round 5: one wave takes TWO rows, i and np-1-i (together np+1 entries: every wave the same work -- with one wave per row the
// launch ended with its longest rows), reads them with 16-byte loads, four independent loads in flight per lane (round 1-4:
// one 8-byte load per lane per round trip, 92 % of the wave cycles in SQ_WAIT_ANY).  Fixed summation order: lane l adds the
// entries k with (k / VEC) % 64 == l in ascending k into accumulator (k / (64 VEC)) % 4, then ((a0 + a1) + (a2 + a3)), then
// the wave sum.  Entries above the diagonal are skipped by the k <= i test, not read as zeros.
template <typename T>
__global__ void __launch_bounds__(256) trmv_n_kernel(const T* __restrict__ Xinv, int np, int n, const T* __restrict__ y,
                                                     T* __restrict__ w, const int* info) {
  if (*info != 0) return;
  using C = Cfg<T>;
  using vec_t = typename C::vec_t;
  constexpr int VEC = C::VEC, SPAN = 64 * VEC;
  const int lane = threadIdx.x & 63, gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (2 * gw >= np) return;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const int row = half == 0 ? gw : np - 1 - gw;
    if (half == 1 && row == gw) break;  // odd np: the middle row once
    const T* xr = Xinv + (size_t)row * np;
    const int len = min(row + 1, n);    // k <= row && k < n
    double acc[4] = {0, 0, 0, 0};
    for (int k0 = lane * VEC; k0 < len; k0 += 4 * SPAN) {
      vec_t xv[4], yv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * SPAN;
        const bool in = k < len;  // a whole vector lies inside the row's padded storage: np is a multiple of 128 >= VEC
        xv[u] = in ? *reinterpret_cast<const vec_t*>(xr + k) : vec_t{};
        yv[u] = in ? *reinterpret_cast<const vec_t*>(y + k) : vec_t{};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (k0 + u * SPAN + e < len) acc[u] = __builtin_fma((double)xv[u][e], (double)yv[u][e], acc[u]);
    }
    double a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    a = wave_sum(a);
    if (lane == 0) w[row] = (T)a;
  }
}

// partial[chunk][j] = sum_{i in chunk, i>=j} X[i][j] w[i]; chunk = 256 rows.  Round 5: a thread owns VEC adjacent columns
// (16-byte loads: 64 lanes cover 128 columns in f64, 256 in f32), wave q of the four takes the rows i = q (mod 4); eight loads in
// flight per lane.  Fixed order: per column the rows of a wave in ascending order, then the four waves' sums in order.
template <typename T>
__global__ void __launch_bounds__(256) trmv_t_kernel(const T* __restrict__ Xinv, int np, const T* __restrict__ w,
                                                     double* __restrict__ part, const int* info) {
  if (*info != 0) return;
  using C = Cfg<T>;
  using vec_t = typename C::vec_t;
  constexpr int VEC = C::VEC, COLS = 64 * VEC;
  __shared__ double red[4][COLS];
  const int lane = threadIdx.x & 63, sgrp = threadIdx.x >> 6;
  const int col0 = blockIdx.x * COLS, j0 = col0 + lane * VEC, chunk = blockIdx.y;
  const int i_begin = chunk * 256, i_end = min(i_begin + 256, np);
  if (i_end <= col0) return;  // the whole chunk lies above these columns' diagonal entries (uniform)
  double acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0;
  if (j0 < np) {
    int i = i_begin + sgrp;
    for (; i + 28 < i_end; i += 32) {
      vec_t xv[8];
      T wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int iu = i + 4 * u;
        xv[u] = (iu >= j0) ? *reinterpret_cast<const vec_t*>(Xinv + (size_t)iu * np + j0) : vec_t{};
        wv[u] = w[iu];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (i + 4 * u >= j0 + e) acc[e] = __builtin_fma((double)xv[u][e], (double)wv[u], acc[e]);
    }
    for (; i < i_end; i += 4) {
      if (i < j0) continue;
      const vec_t xv = *reinterpret_cast<const vec_t*>(Xinv + (size_t)i * np + j0);
      const double wi = (double)w[i];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (i >= j0 + e) acc[e] = __builtin_fma((double)xv[e], wi, acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[sgrp][lane * VEC + e] = acc[e];
  __syncthreads();
  for (int c = threadIdx.x; c < COLS; c += 256)
    if (col0 + c < np) part[(size_t)chunk * np + col0 + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// lml = -1/2 y^T alpha - sum log L_ii - n/2 log(2 pi)   (lml.rs:57-59); fixed summation order; one thread
__device__ __forceinline__ void lml_final(const double* __restrict__ sums, int nblocks, int n, EvalOut* out) {
  double s1 = 0, s2 = 0;
  for (int b = 0; b < nblocks; ++b) {
    s1 += sums[2 * b];
    s2 += sums[2 * b + 1];
  }
  out->yalpha = s1;
  out->logdet = s2;
  out->lml = __builtin_fma(-0.5, s1, -s2) - (double)n / 2.0 * log(2.0 * 3.14159265358979323846);
  atomicOr(&out->done, 1);
}

// alpha_j = sum_chunks part[c][j]; per-workgroup partial sums of y^T alpha and sum log L_jj  (256 columns per workgroup)
template <typename T>
__global__ void __launch_bounds__(256) alpha_reduce_kernel(const double* __restrict__ part, int nchunks, int np, int n,
                                                           const T* __restrict__ y, const T* __restrict__ ldiag,
                                                           T* __restrict__ alpha, double* __restrict__ sums, const int* info,
                                                           EvalOut* out_final, int* ticket) {
  if (*info != 0) return;
  __shared__ double red[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  double ya = 0, ld = 0;
  if (j < np) {
    double a = 0;
    // same sum, chunk by chunk in ascending order; the loads of eight chunks are issued together (as a plain loop each one was
    // waited for before the next: 16 dependent round trips at n = 4096)
    int c = j / 256;
    for (; c + 8 <= nchunks; c += 8) {
      double pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) pv[u] = part[(size_t)(c + u) * np + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += pv[u];
    }
    for (; c < nchunks; ++c) a += part[(size_t)c * np + j];
    const T at = (T)a;
    alpha[j] = (j < n) ? at : T(0);
    if (j < n) {
      ya = (double)y[j] * (double)at;
      ld = log((double)ldiag[j]);
    }
  }
  const double s1 = block_sum(ya, red);
  const double s2 = block_sum(ld, red);
  if (threadIdx.x == 0) {
    publish_f64(&sums[2 * blockIdx.x], s1);
    publish_f64(&sums[2 * blockIdx.x + 1], s2);
  }
  // out_final: the last workgroup to finish forms the lml itself (one launch less on every evaluation's serial tail)
  if (out_final && last_workgroup(ticket) && threadIdx.x == 0) lml_final(sums, (int)gridDim.x, n, out_final);
}

// lml = -1/2 y^T alpha - sum log L_ii - n/2 log(2 pi)   (lml.rs:57-59); fixed summation order
__global__ void lml_final_kernel(const double* __restrict__ sums, int nblocks, int n, EvalOut* out, const int* info) {
  if (*info != 0) return;
  if (threadIdx.x == 0) lml_final(sums, nblocks, n, out);
}

template <typename T>
void launch_alpha_lml(const T* Xinv, int np, int n, const T* y, const T* ldiag, T* wbuf, double* part, T* alpha,
                      EvalOut* out, const int* info, hipStream_t s, int* ticket) {
  hipLaunchKernelGGL((trmv_n_kernel<T>), dim3((np / 2 + 3) / 4), dim3(256), 0, s, Xinv, np, n, y, wbuf, info);
  const int nchunks = np / 256 > 0 ? (np + 255) / 256 : 1;
  constexpr int TCOLS = 64 * Cfg<T>::VEC;
  hipLaunchKernelGGL((trmv_t_kernel<T>), dim3((np + TCOLS - 1) / TCOLS, nchunks), dim3(256), 0, s, Xinv, np, wbuf, part, info);
  // the per-workgroup sums live behind the chunk partials (part has room for nchunks*np + 2*np/256 doubles)
  double* sums = part + (size_t)nchunks * np;
  const int nblocks = (np + 255) / 256;
  hipLaunchKernelGGL((alpha_reduce_kernel<T>), dim3(nblocks), dim3(256), 0, s, part, nchunks, np, n, y, ldiag, alpha, sums, info,
                     ticket ? out : nullptr, ticket);
  if (!ticket) hipLaunchKernelGGL(lml_final_kernel, dim3(1), dim3(64), 0, s, sums, nblocks, n, out, info);
}
template void launch_alpha_lml<double>(const double*, int, int, const double*, const double*, double*, double*, double*,
                                       EvalOut*, const int*, hipStream_t, int*);
template void launch_alpha_lml<float>(const float*, int, int, const float*, const float*, float*, double*, float*,
                                      EvalOut*, const int*, hipStream_t, int*);

// =================================================================================================================
// Gradient of the lml: g_j = 1/2 sum_ik (alpha_i alpha_k - Kinv_ik) dK_ik/dtheta_j   (lml.rs:62-70)
// theta order [noise, amplitude, ell_1..ell_d]; dK formulas: constant_kernel.rs:31-38, product_kernel.rs:56-67,
// matern_kernel.rs:88-131.  One pass over the lower triangle of Kinv (off-diagonal entries weighted twice).
// =================================================================================================================
constexpr int GT_CHUNK = 8;  // length-scale parameters accumulated per register pass

// Sums of NV per-thread values over the 256 threads of a workgroup, all at once: every thread parks its values in the LDS
// ([v][256]), wave q adds up the values v = q, q + 4, ... (lane l: threads l, l + 64, l + 128, l + 192 in that order, then the
// wave sum) and its lane 0 stores the result write-through.  Two barriers for up to GT_CHUNK + 2 values (round 1-4: a block sum
// with two barriers per value -- 20 barriers per tile at d = 8, as much time as the tile's arithmetic).  Fixed order.
template <int NV>
__device__ __forceinline__ void block_sums_publish(const double (&v)[NV], int nv, double* red, double* dst) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __syncthreads();  // the previous use of red has been read
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (q < nv) red[q * 256 + t] = v[q];
  __syncthreads();
  for (int q = wave; q < nv; q += 4) {
    const double* r = red + q * 256;
    double a = ((r[lane] + r[lane + 64]) + r[lane + 128]) + r[lane + 192];
    a = wave_sum(a);
    if (lane == 0) publish_f64(&dst[q], a);
  }
}

// LOO (loo_trace_kernel, the gradient of the leave-one-out pseudo-likelihood): the same pass with the weight
// u_i alpha_k + alpha_i u_k - 2 C_ik, C = K^-1 diag(b) K^-1 read through `Kinv`; nothing else differs, and the lml instantiations
// compile to the instructions they had before the parameter existed.
template <typename T, int NU2, bool LOO = false>
__device__ __forceinline__ void gradtrace_tile(int tile, const T* __restrict__ X, int n, int d, int np, T amp, T noise,
                                               const double* inv_l2, const T* __restrict__ Kinv, const T* __restrict__ alpha,
                                               double* __restrict__ part, T* xi, T* xj, double* red,
                                               const T* __restrict__ uvec = nullptr) {
  const int li = tri_row(tile), lj = tile - li * (li + 1) / 2;
  const int i0 = li * 64, j0 = lj * 64;
  const int t = threadIdx.x;
  for (int e = t; e < 64 * d; e += 256) {
    const int row = e / d, k = e - row * d;
    const int gi = i0 + row, gj = j0 + row;
    xi[k * 64 + row] = (gi < n) ? X[(size_t)gi * d + k] : T(0);
    xj[xj_index<T>(k, row)] = (gj < n) ? X[(size_t)gj * d + k] : T(0);
  }
  __syncthreads();
  const int tx = t & 15, ty = t >> 4;

  // pass A: per-element coefficient coef = wgt * W * c * g(r) and the noise / amplitude sums
  T coef[4][4];
  double g_noise = 0, g_amp = 0;
  {
    T dsum[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) dsum[r][c] = T(0);
    for (int k = 0; k < d; ++k) {
      const T il2 = (T)inv_l2[k];
      T a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
      read_xj4<T>(xj, k, tx, b);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T df = a[r] - b[c];
          dsum[r][c] += df * df * il2;
        }
    }
    // Matern value km and gradient factor gr of one entry: dK/dlog(ell_k) = c * gr * d_k (matern_kernel.rs:102-131)
    auto km_gr = [&](T ds, T* km, T* gr) {
#pragma clang fp contract(off)
      if (NU2 == 5) {
        const T tt = sqrt_nonneg(ds * T(5));
        const T e = exp_nonpos(-tt);
        *km = __builtin_fma(tt * tt, T(1.0 / 3.0), T(1) + tt) * e;
        *gr = T(5.0 / 3.0) * (tt + T(1)) * e;  // matern_kernel.rs:119-131
      } else if (NU2 == 3) {
        const T tt = sqrt_nonneg(ds * T(3));
        const T e = exp_nonpos(-tt);
        *km = (tt + T(1)) * e;
        *gr = T(3) * e;  // matern_kernel.rs:112-118
      } else if (NU2 == 0) {
        *km = exp_nonpos(T(-0.5) * ds);  // squared exponential: dK/dlog(ell_k) = K * d_k
        *gr = *km;
      } else {
        const T rr = sqrt_nonneg(ds);
        *km = exp_nonpos(-rr);
        *gr = (rr > T(0)) ? *km / rr : T(0);  // matern_kernel.rs:102-111 (non-finite -> 0)
      }
    };
    typedef T vec4 __attribute__((ext_vector_type(4)));
    if (li > lj && i0 + 64 <= n) {
      // a tile strictly below the diagonal and wholly inside the matrix: every entry counts twice, no bounds tests
      const vec4 aj = *reinterpret_cast<const vec4*>(alpha + j0 + tx * 4);
      vec4 uj{};
      if constexpr (LOO) uj = *reinterpret_cast<const vec4*>(uvec + j0 + tx * 4);
      vec4 kv[4];
      T ai[4], ui[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // the four rows' loads together
        const int gi = i0 + ty + 16 * r;
        ai[r] = alpha[gi];
        if constexpr (LOO) ui[r] = uvec[gi];
        kv[r] = *reinterpret_cast<const vec4*>(Kinv + (size_t)gi * np + j0 + tx * 4);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          T w;
          if constexpr (LOO) w = (ui[r] * aj[c] + ai[r] * uj[c]) - T(2) * kv[r][c];
          else w = ai[r] * aj[c] - kv[r][c];  // lml.rs:62 (tmp)
          T km, gr;
          km_gr(dsum[r][c], &km, &gr);
          g_amp += (double)(T(2) * w * (amp * km));  // constant_kernel.rs:31-38 x K_matern
          coef[r][c] = T(2) * w * amp * gr;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + ty + 16 * r;
        const T ai = (gi < n) ? alpha[gi] : T(0);
        T ui = T(0);
        if constexpr (LOO) ui = (gi < n) ? uvec[gi] : T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int gj = j0 + tx * 4 + c;
          T cf = T(0);
          if (gi < n && gj <= gi) {
            T w;
            if constexpr (LOO) w = (ui * alpha[gj] + ai * uvec[gj]) - T(2) * Kinv[(size_t)gi * np + gj];
            else w = ai * alpha[gj] - Kinv[(size_t)gi * np + gj];  // lml.rs:62 (tmp)
            const T wgt = (gi == gj) ? T(1) : T(2);
            T km, gr;
            km_gr(dsum[r][c], &km, &gr);
            if (gi == gj) g_noise += (double)(w * noise);      // noise gradient = eye * noise (lml.rs:41)
            g_amp += (double)(wgt * w * (amp * km));            // constant_kernel.rs:31-38 x K_matern
            cf = wgt * w * amp * gr;
          }
          coef[r][c] = cf;
        }
      }
    }
  }
  const int p = d + 2;
  double* my = part + (size_t)tile * p;
  // pass B: length-scale gradients, GT_CHUNK parameters at a time; the first chunk carries the noise / amplitude sums along
  for (int kc = 0; kc < d; kc += GT_CHUNK) {
    double vals[GT_CHUNK + 2];
#pragma unroll
    for (int u = 0; u < GT_CHUNK + 2; ++u) vals[u] = 0;
    const int lead = kc == 0 ? 2 : 0;
    if (kc == 0) { vals[0] = g_noise; vals[1] = g_amp; }
#pragma unroll
    for (int u = 0; u < GT_CHUNK; ++u) {
      const int k = kc + u;
      if (k < d) {
        const T il2 = (T)inv_l2[k];
        T a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
        read_xj4<T>(xj, k, tx, b);
        T sacc = T(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const T df = a[r] - b[c];
            sacc += coef[r][c] * (df * df * il2);
          }
        if (kc == 0) vals[2 + u] = (double)sacc;
        else vals[u] = (double)sacc;
      }
    }
    const int nv = lead + min(GT_CHUNK, d - kc);
    block_sums_publish<GT_CHUNK + 2>(vals, nv, red, my + (kc == 0 ? 0 : 2 + kc));
  }
}

// grad[j] = 0.5 * sum_blocks part[b][j] as finalize_grad_kernel forms it (thread t of 256 adds blocks t, t+256, ...; wave sums;
// the four wave sums in order), computed by ONE wave per parameter: lane l carries the four threads l, l+64, l+128, l+192.
__device__ __forceinline__ void finalize_grad_in_block(const double* __restrict__ part, int nblocks, int p, EvalOut* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < p; j += 4) {
    double acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      for (int b = q * 64 + lane; b < nblocks; b += 256) acc[q] += part[(size_t)b * p + j];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = wave_sum(acc[q]);
    if (lane == 0) publish_f64(&out->grad[j], 0.5 * (acc[0] + acc[1] + acc[2] + acc[3]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have reached the L2 before the caller's barrier opens
}

// device result block -> pinned host block, then the evaluation's serial number behind a system-scope fence (engine.hpp).
// Called by one whole workgroup (>= 128 threads) whose own writes to `out` are complete behind a barrier.
__device__ __forceinline__ void publish_out_in_block(const EvalOut* out, EvalOut* hout, const EvalParams* __restrict__ P) {
  const int t = threadIdx.x;
  constexpr int OW = (int)(offsetof(EvalOut, seq) / 8);
  static_assert(offsetof(EvalOut, seq) % 8 == 0 && OW <= 128, "EvalOut is copied as 8-byte words by one workgroup");
  if (t < OW) {
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(out) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    reinterpret_cast<unsigned long long*>(hout)[t] = v;
  }
  __threadfence_system();
  __syncthreads();
  if (t == 0) __hip_atomic_store(&hout->seq, P->seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// fin.out != null: the launch also finalises the gradient and publishes the evaluation (its last workgroup does), also when
// the factorisation failed (info != 0: the tiles are skipped, the host still gets its answer).
struct GradFinish {
  EvalOut* out = nullptr;
  EvalOut* hout = nullptr;   // pinned result block (null: finalise only)
  int* ticket = nullptr;
};
template <typename T, int NU2>
__global__ void __launch_bounds__(256) gradtrace_kernel(const T* __restrict__ X, int n, int d, int np,
                                                        const EvalParams* __restrict__ P, const T* __restrict__ Kinv,
                                                        const T* __restrict__ alpha, double* __restrict__ part,
                                                        const int* info, GradFinish fin) {
  extern __shared__ __align__(16) char smem_raw[];
  T* xi = reinterpret_cast<T*>(smem_raw);  // [d][64] raw features of the i tile
  T* xj = xi + (size_t)d * 64;             // j tile, xj_index layout
  __shared__ double red[(GT_CHUNK + 2) * 256];
  __shared__ double inv_l2[MAXD];
  const bool failed = *info != 0;
  const int t = threadIdx.x;
  if (!failed) {
    if (t < d) {
      const T ell = (T)P->ell[t];
      inv_l2[t] = (double)(T(1) / (ell * ell));  // 1/scales_k_square (matern_kernel.rs:94-98)
    }
    const T amp = (T)P->amp, noise = (T)P->noise;
    gradtrace_tile<T, NU2>((int)blockIdx.x, X, n, d, np, amp, noise, inv_l2, Kinv, alpha, part, xi, xj, red);
  }
  if (!fin.out) return;
  // every publishing lane (lane 0 of each wave) has its stores in the L2 before thread 0 takes the launch's ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (!last_workgroup(fin.ticket)) return;
  if (!failed) {
    finalize_grad_in_block(part, (int)gridDim.x, d + 2, fin.out);
    if (threadIdx.x == 0) atomicOr(&fin.out->done, 2);
  }
  __syncthreads();
  if (fin.hout) publish_out_in_block(fin.out, fin.hout, P);
}

// grad[j] = 0.5 * sum_blocks part[b][j]  (fixed summation order -> bitwise reproducible)
__global__ void __launch_bounds__(256) finalize_grad_kernel(const double* __restrict__ part, int nblocks, int p,
                                                            EvalOut* out, const int* info) {
  if (*info != 0) return;
  __shared__ double red[4];
  const int j = blockIdx.x;
  double acc = 0;
  for (int b = threadIdx.x; b < nblocks; b += 256) acc += part[(size_t)b * p + j];
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) {
    out->grad[j] = 0.5 * s;
    if (j == p - 1) atomicOr(&out->done, 2);  // the last block alone cannot vouch for the others; the host checks every entry for NaN
  }
}

size_t gradtrace_part_elems(int np, int d) {
  const int nt = np / 64;
  return (size_t)(nt * (nt + 1) / 2) * (d + 2);
}

template <typename T>
void launch_gradtrace(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Kinv, const T* alpha,
                      double* part, EvalOut* out, const int* info, hipStream_t s, int* ticket, EvalOut* hout) {
  const int nt = np / 64;
  const int ntiles = nt * (nt + 1) / 2;
  const size_t lds = (size_t)2 * d * 64 * sizeof(T);
  const dim3 grid(ntiles), block(256);
  GradFinish fin;
  if (ticket) { fin.out = out; fin.hout = hout; fin.ticket = ticket; }
  switch (nu2) {
    case 0: hipLaunchKernelGGL((gradtrace_kernel<T, 0>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, info, fin); break;
    case 1: hipLaunchKernelGGL((gradtrace_kernel<T, 1>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, info, fin); break;
    case 3: hipLaunchKernelGGL((gradtrace_kernel<T, 3>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, info, fin); break;
    default: hipLaunchKernelGGL((gradtrace_kernel<T, 5>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, info, fin); break;
  }
  if (!ticket) hipLaunchKernelGGL(finalize_grad_kernel, dim3(d + 2), dim3(256), 0, s, part, ntiles, d + 2, out, info);
}
template void launch_gradtrace<double>(const double*, int, int, int, int, const EvalParams*, const double*, const double*,
                                       double*, EvalOut*, const int*, hipStream_t, int*, EvalOut*);
template void launch_gradtrace<float>(const float*, int, int, int, int, const EvalParams*, const float*, const float*,
                                      double*, EvalOut*, const int*, hipStream_t, int*, EvalOut*);

// =================================================================================================================
// Input warping (hbegp_problem_eval_xgrad / _eval_warped).
//   warp_kernel        U = w(X; a, b) elementwise (warp.hpp, fp64, rounded once to T) and, on request, dU/dln a, dU/dln b (fp64)
//   xgrad_kernel       G_ik = d lml / d x_ik = sum_j (alpha_i alpha_j - Kinv_ij) c psi(r_ij) (x_ik - x_jk) / ell_k^2, psi = phi'(r) / r
//   warp_chain_kernel  out[k] = sum_i G_ik dU_ik/dln a_k, out[d + k] the same for b
// xgrad_kernel is gradtrace's sibling: the same 64-row tiles of X in the LDS (xj_index layout), the same thread -> 4 x 4 entries
// map, the same distance sum, the same gradient factor gr of the four orders (psi = -gr: dK/dln ell_k = c gr d_k with
// d_k = -r dr/dln ell_k), GT_CHUNK features per register pass.  What differs is the sum: a row's entries are added over j ONLY,
// with (x_ik - x_jk) / ell_k^2 in place of its square, so W is needed on both sides of the diagonal while the slot's K^-1 is valid
// on and below it only: element (max(i, j), min(i, j)) is read.  Entries with r = 0 (the diagonal, duplicate rows) contribute 0:
// their difference is 0 and gr is finite (0 for nu = 1/2).  Rows and columns >= n contribute nothing and receive nothing.
// Grid: x = (row tile, feature chunk), y = XG_SPLIT-th shares of the j tiles (row tiles alone are 64 workgroups at n = 4096).
// Workgroup (li, kc, s) adds its j tiles lj = s, s + S, ... in ascending order into fp64 registers (per entry row: the four
// columns of a thread in T, as gradtrace adds them), then the 16 threads of a row by an xor butterfly, and stores
// part[s][row][k] write-through; the launch's last workgroup (the ticket pattern) adds the S shares of every (row, k) in ascending
// s.  S depends on n alone: the same inputs give the same bits whatever the timing.
// =================================================================================================================
constexpr int XG_SPLIT = 8;

template <typename T, int NU2>
__device__ __forceinline__ T matern_gr(T ds) {  // gradtrace_tile's gr
#pragma clang fp contract(off)
  if (NU2 == 5) {
    const T tt = sqrt_nonneg(ds * T(5));
    return T(5.0 / 3.0) * (tt + T(1)) * exp_nonpos(-tt);
  } else if (NU2 == 3) {
    const T tt = sqrt_nonneg(ds * T(3));
    return T(3) * exp_nonpos(-tt);
  } else if (NU2 == 0) {
    return exp_nonpos(T(-0.5) * ds);
  } else {
    const T rr = sqrt_nonneg(ds);
    return (rr > T(0)) ? exp_nonpos(-rr) / rr : T(0);
  }
}

static int xgrad_splits(int n) { return std::min((n + 63) / 64, XG_SPLIT); }
size_t xgrad_part_elems(int n, int d) { return (size_t)xgrad_splits(n) * ((n + 63) / 64 * 64) * d; }

template <typename T, int NU2>
__global__ void __launch_bounds__(256) xgrad_kernel(const T* __restrict__ X, int n, int d, int np, const EvalParams* __restrict__ P,
                                                    const T* __restrict__ Kinv, const T* __restrict__ alpha,
                                                    double* __restrict__ part, double* __restrict__ G, int* ticket) {
  extern __shared__ __align__(16) char smem_raw[];
  T* xi = reinterpret_cast<T*>(smem_raw);  // [d][64] raw features of the i tile
  T* xj = xi + (size_t)d * 64;             // j tile, xj_index layout
  __shared__ double inv_l2[MAXD];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int nt = (n + 63) / 64;            // tiles that hold a live row
  const int li = (int)blockIdx.x % nt, kc = ((int)blockIdx.x / nt) * GT_CHUNK;
  const int split = (int)blockIdx.y, nsplit = (int)gridDim.y;
  const int i0 = li * 64;
  if (t < d) {
    const T ell = (T)P->ell[t];
    inv_l2[t] = (double)(T(1) / (ell * ell));
  }
  const T amp = (T)P->amp;
  for (int e = t; e < 64 * d; e += 256) {
    const int row = e / d, k = e - row * d;
    const int gi = i0 + row;
    xi[k * 64 + row] = (gi < n) ? X[(size_t)gi * d + k] : T(0);
  }
  double acc[4][GT_CHUNK];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int u = 0; u < GT_CHUNK; ++u) acc[r][u] = 0;
  typedef T vec4 __attribute__((ext_vector_type(4)));
  for (int lj = split; lj < nt; lj += nsplit) {
    const int j0 = lj * 64;
    __syncthreads();  // the previous j tile has been read
    for (int e = t; e < 64 * d; e += 256) {
      const int row = e / d, k = e - row * d;
      const int gj = j0 + row;
      xj[xj_index<T>(k, row)] = (gj < n) ? X[(size_t)gj * d + k] : T(0);
    }
    __syncthreads();
    T dsum[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) dsum[r][c] = T(0);
    for (int k = 0; k < d; ++k) {
      const T il2 = (T)inv_l2[k];
      T a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
      read_xj4<T>(xj, k, tx, b);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const T df = a[r] - b[c];
          dsum[r][c] += df * df * il2;
        }
    }
    // coef = W_ij c psi(r_ij)
    T coef[4][4];
    if (li > lj && i0 + 64 <= n) {
      // wholly inside the matrix and below the diagonal: K^-1 as stored, one 16-byte load per row
      const vec4 aj = *reinterpret_cast<const vec4*>(alpha + j0 + tx * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + ty + 16 * r;
        const T ai = alpha[gi];
        const vec4 kv = *reinterpret_cast<const vec4*>(Kinv + (size_t)gi * np + j0 + tx * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) coef[r][c] = -((ai * aj[c] - kv[c]) * amp * matern_gr<T, NU2>(dsum[r][c]));
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + ty + 16 * r;
        const T ai = (gi < n) ? alpha[gi] : T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int gj = j0 + tx * 4 + c;
          T cf = T(0);
          if (gi < n && gj < n) {
            const int hi = max(gi, gj), lo = min(gi, gj);  // the lower triangle is the valid one
            const T w = ai * alpha[gj] - Kinv[(size_t)hi * np + lo];
            cf = -(w * amp * matern_gr<T, NU2>(dsum[r][c]));
          }
          coef[r][c] = cf;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GT_CHUNK; ++u) {
      const int k = kc + u;
      if (k < d) {
        const T il2 = (T)inv_l2[k];
        T a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
        read_xj4<T>(xj, k, tx, b);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T sacc = T(0);
#pragma unroll
          for (int c = 0; c < 4; ++c) sacc += coef[r][c] * ((a[r] - b[c]) * il2);
          acc[r][u] += (double)sacc;
        }
      }
    }
  }
  // the 16 threads of a row (tx = 0..15 are neighbouring lanes); every lane ends with the sum
  const size_t n64 = (size_t)nt * 64;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int u = 0; u < GT_CHUNK; ++u) {
      double v = acc[r][u];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      const int k = kc + u;
      if (tx == 0 && k < d) publish_f64(&part[((size_t)split * n64 + i0 + ty + 16 * r) * d + k], v);
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (!last_workgroup(ticket)) return;
  const size_t nd = (size_t)n * d, stride = n64 * d;
  for (size_t e = t; e < nd; e += 256) {
    double s = 0;
    for (int q = 0; q < nsplit; ++q) s += part[(size_t)q * stride + e];
    G[e] = s;
  }
}

template <typename T>
void launch_xgrad(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Kinv, const T* alpha, double* part, double* G,
                  int* ticket, hipStream_t s) {
  const int nt = (n + 63) / 64, nch = (d + GT_CHUNK - 1) / GT_CHUNK;
  const size_t lds = (size_t)2 * d * 64 * sizeof(T);
  const dim3 grid(nt * nch, xgrad_splits(n)), block(256);
  switch (nu2) {
    case 0: hipLaunchKernelGGL((xgrad_kernel<T, 0>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, G, ticket); break;
    case 1: hipLaunchKernelGGL((xgrad_kernel<T, 1>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, G, ticket); break;
    case 3: hipLaunchKernelGGL((xgrad_kernel<T, 3>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, G, ticket); break;
    default: hipLaunchKernelGGL((xgrad_kernel<T, 5>), grid, block, lds, s, X, n, d, np, P, Kinv, alpha, part, G, ticket); break;
  }
}
template void launch_xgrad<double>(const double*, int, int, int, int, const EvalParams*, const double*, const double*, double*, double*,
                                   int*, hipStream_t);
template void launch_xgrad<float>(const float*, int, int, int, int, const EvalParams*, const float*, const float*, double*, double*, int*,
                                  hipStream_t);

template <typename T>
__global__ void __launch_bounds__(256) warp_kernel(const T* __restrict__ X, size_t count, int d, const double* __restrict__ ab,
                                                   T* __restrict__ U, double* __restrict__ dlna, double* __restrict__ dlnb) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const int k = (int)(e % (size_t)d);
  double u, da, db;
  warp::apply(ab[k], ab[d + k], (double)X[e], &u, &da, &db, nullptr);  // (always all three: a conditional pointer keeps them on the stack)
  U[e] = (T)u;
  if (dlna) dlna[e] = da;
  if (dlnb) dlnb[e] = db;
}
template <typename T>
void launch_warp(const T* X, int n, int d, const double* ab, T* U, double* dlna, double* dlnb, hipStream_t s) {
  const size_t count = (size_t)n * d;
  hipLaunchKernelGGL((warp_kernel<T>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, X, count, d, ab, U, dlna, dlnb);
}
template void launch_warp<double>(const double*, int, int, const double*, double*, double*, double*, hipStream_t);
template void launch_warp<float>(const float*, int, int, const double*, float*, double*, double*, hipStream_t);

// One workgroup; wave w takes the 2 d dot products q = w, w + 4, ...: lane l adds rows l, l + 64, ... in ascending order, then the
// wave sum.  Fixed order.
__global__ void __launch_bounds__(256) warp_chain_kernel(const double* __restrict__ G, const double* __restrict__ dlna,
                                                         const double* __restrict__ dlnb, int n, int d, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < 2 * d; q += 4) {
    const int k = q < d ? q : q - d;
    const double* __restrict__ D = q < d ? dlna : dlnb;
    double a = 0;
    for (int i = lane; i < n; i += 64) a += G[(size_t)i * d + k] * D[(size_t)i * d + k];
    a = wave_sum(a);
    if (lane == 0) out[q] = a;
  }
}
void launch_warp_chain(const double* G, const double* dlna, const double* dlnb, int n, int d, double* out, hipStream_t s) {
  hipLaunchKernelGGL(warp_chain_kernel, dim3(1), dim3(256), 0, s, G, dlna, dlnb, n, d, out);
}

// =================================================================================================================
// Leave-one-out cross-validation in closed form (Rasmussen & Williams 5.4.2).  With M = K^-1, m_i = M_ii:
//   mu_i = y_i - alpha_i / m_i,  var_i = 1 / m_i,  lpd_i = 1/2 ln m_i - alpha_i^2 / (2 m_i) - 1/2 ln 2 pi,  loo = sum_i lpd_i
//   dloo/dtheta_j = 1/2 sum_ik (u_i alpha_k + alpha_i u_k - 2 C_ik) dK_ik/dtheta_j,
//   a_i = alpha_i / m_i,  b_i = (1 + alpha_i^2 / m_i) / (2 m_i),  u = M a,  C = Y Y^T,  Y = M diag(sqrt b)
// Every sum is fp64 in a fixed order for both element types; no atomics on results.
// =================================================================================================================
// part[chunk][j] = sum_{i in chunk, j <= i < n} X[i][j]^2 of the lower-triangular X = L^-1: the column sums of squares that
// make m_j = (X^T X)_jj from positive terms alone (the diagonal of the stored K^-1 loses digits with cond(K)).  The access pattern of
// trmv_t_kernel (a thread owns VEC adjacent columns, wave q takes the rows i = q mod 4, eight 16-byte loads in flight per lane);
// per column the rows of a wave in ascending order, then the four waves' sums in order.  Rows of the identity padding are left out.
template <typename T>
__global__ void __launch_bounds__(256) loo_colsq_kernel(const T* __restrict__ Xinv, int np, int n, double* __restrict__ part) {
  using C = Cfg<T>;
  using vec_t = typename C::vec_t;
  constexpr int VEC = C::VEC, COLS = 64 * VEC;
  __shared__ double red[4][COLS];
  const int lane = threadIdx.x & 63, sgrp = threadIdx.x >> 6;
  const int col0 = blockIdx.x * COLS, j0 = col0 + lane * VEC, chunk = blockIdx.y;
  const int i_begin = chunk * 256, i_end = min(i_begin + 256, n);
  if (i_end <= col0) return;  // the whole chunk lies above these columns' diagonal entries (uniform); never read by the finish
  double acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0;
  if (j0 < np) {
    int i = i_begin + sgrp;
    for (; i + 28 < i_end; i += 32) {
      vec_t xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int iu = i + 4 * u;
        xv[u] = (iu >= j0) ? *reinterpret_cast<const vec_t*>(Xinv + (size_t)iu * np + j0) : vec_t{};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (i + 4 * u >= j0 + e) acc[e] = __builtin_fma((double)xv[u][e], (double)xv[u][e], acc[e]);
    }
    for (; i < i_end; i += 4) {
      if (i < j0) continue;
      const vec_t xv = *reinterpret_cast<const vec_t*>(Xinv + (size_t)i * np + j0);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (i >= j0 + e) acc[e] = __builtin_fma((double)xv[e], (double)xv[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[sgrp][lane * VEC + e] = acc[e];
  __syncthreads();
  for (int c = threadIdx.x; c < COLS; c += 256)
    if (col0 + c < np) part[(size_t)chunk * np + col0 + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// m_j = sum over the chunks from the column's own one on, ascending; then the row's diagnostics and the gradient's vectors
// a, sqrt b (fp64; zero on the padding); sums[block] = the block's share of loo (256 columns per workgroup)
template <typename T>
__global__ void __launch_bounds__(256) loo_diag_finish_kernel(const double* __restrict__ part, int nchunks, int np, int n,
                                                              const T* __restrict__ y, const T* __restrict__ alpha,
                                                              T* __restrict__ mean, T* __restrict__ var, T* __restrict__ lpd,
                                                              double* __restrict__ avec, double* __restrict__ sbvec,
                                                              double* __restrict__ sums) {
  __shared__ double red[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  double l = 0;
  if (j < np) {
    double a = 0, sb = 0;
    if (j < n) {
      double m = 0;
      for (int c = j / 256; c < nchunks; ++c) m += part[(size_t)c * np + j];
      const double al = (double)alpha[j];
      a = al / m;
      const double q = al * a;  // alpha_j^2 / m_j
      l = 0.5 * log(m) - 0.5 * q - 0.5 * log(2.0 * 3.14159265358979323846);
      sb = sqrt(0.5 * (1.0 + q) / m);
      mean[j] = (T)((double)y[j] - a);
      var[j] = (T)(1.0 / m);
      lpd[j] = (T)l;
    }
    avec[j] = a;
    sbvec[j] = sb;
  }
  const double s = block_sum(l, red);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// loo = the blocks' shares in ascending order (one thread)
__global__ void loo_sum_kernel(const double* __restrict__ sums, int nblocks, EvalOut* out) {
  if (threadIdx.x != 0) return;
  double s = 0;
  for (int b = 0; b < nblocks; ++b) s += sums[b];
  out->lml = s;
  atomicOr(&out->done, 1);
}

// One pass over the lower triangle of K^-1 (64 x 64 tiles; only entries on or below the diagonal are read, so the slot's
// unmirrored buffer and the model's full matrix give the same bits): the full matrix Y = K^-1 diag(sqrt b) -- the tile and its
// mirror image, zeros on the padding -- and the tile's share of u = K^-1 a: pu[q][i], q the 64-block of the contraction index.
// Wave 0 / 1 add the two halves of a row's 64 terms in ascending order, wave 2 / 3 those of a column (the mirror image's rows).
template <typename T>
__global__ void __launch_bounds__(256) loo_uy_kernel(const T* __restrict__ Kinv, int np, int n, const double* __restrict__ avec,
                                                     const double* __restrict__ sbvec, T* __restrict__ Y, double* __restrict__ pu) {
  __shared__ T tile[64][65];
  __shared__ double a_i[64], a_j[64], sb_i[64], sb_j[64];
  __shared__ double red[4][64];
  const int li = tri_row(blockIdx.x), lj = blockIdx.x - li * (li + 1) / 2;
  const int i0 = li * 64, j0 = lj * 64;
  const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int gi = i0 + r, gj = j0 + tx;
    tile[r][tx] = (gi < n && gj <= gi) ? Kinv[(size_t)gi * np + gj] : T(0);
  }
  if (ty == 0) { a_i[tx] = avec[i0 + tx]; sb_i[tx] = sbvec[i0 + tx]; }
  if (ty == 1) { a_j[tx] = avec[j0 + tx]; sb_j[tx] = sbvec[j0 + tx]; }
  __syncthreads();
  if (li == lj) {  // the diagonal tile: fill in its upper half (reads entries below the diagonal, writes entries above it)
    for (int r = ty; r < 64; r += 4)
      if (tx > r) tile[r][tx] = tile[tx][r];
    __syncthreads();
  }
  for (int r = ty; r < 64; r += 4) Y[(size_t)(i0 + r) * np + j0 + tx] = (T)((double)tile[r][tx] * sb_j[tx]);
  if (li != lj)
    for (int r = ty; r < 64; r += 4) Y[(size_t)(j0 + r) * np + i0 + tx] = (T)((double)tile[tx][r] * sb_i[tx]);
  const int h0 = (ty & 1) * 32;
  double s = 0;
  if (ty < 2) {
    for (int c = h0; c < h0 + 32; ++c) s = __builtin_fma((double)tile[tx][c], a_j[c], s);
  } else if (li != lj) {
    for (int r = h0; r < h0 + 32; ++r) s = __builtin_fma((double)tile[r][tx], a_i[r], s);
  }
  red[ty][tx] = s;
  __syncthreads();
  if (t < 64) pu[(size_t)lj * np + i0 + t] = red[0][t] + red[1][t];
  else if (t < 128 && li != lj) pu[(size_t)li * np + j0 + (t - 64)] = red[2][t - 64] + red[3][t - 64];
}

// u_i = sum_q pu[q][i], q ascending
template <typename T>
__global__ void __launch_bounds__(256) loo_u_finish_kernel(const double* __restrict__ pu, int nt, int np, T* __restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  double s = 0;
  int q = 0;
  for (; q + 8 <= nt; q += 8) {
    double pv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pv[e] = pu[(size_t)(q + e) * np + i];
#pragma unroll
    for (int e = 0; e < 8; ++e) s += pv[e];
  }
  for (; q < nt; ++q) s += pu[(size_t)q * np + i];
  u[i] = (T)s;
}

// the weighted trace: gradtrace_kernel's tiles with the leave-one-out weight (gradtrace_tile<.., LOO = true>); finalize_grad_kernel
// behind it forms the gradient
template <typename T, int NU2>
__global__ void __launch_bounds__(256) loo_trace_kernel(const T* __restrict__ X, int n, int d, int np,
                                                        const EvalParams* __restrict__ P, const T* __restrict__ Cm,
                                                        const T* __restrict__ alpha, const T* __restrict__ u,
                                                        double* __restrict__ part, const int* info) {
  extern __shared__ __align__(16) char smem_raw[];
  T* xi = reinterpret_cast<T*>(smem_raw);
  T* xj = xi + (size_t)d * 64;
  __shared__ double red[(GT_CHUNK + 2) * 256];
  __shared__ double inv_l2[MAXD];
  if (*info != 0) return;
  const int t = threadIdx.x;
  if (t < d) {
    const T ell = (T)P->ell[t];
    inv_l2[t] = (double)(T(1) / (ell * ell));
  }
  const T amp = (T)P->amp, noise = (T)P->noise;
  gradtrace_tile<T, NU2, true>((int)blockIdx.x, X, n, d, np, amp, noise, inv_l2, Cm, alpha, part, xi, xj, red, u);
}

size_t loo_diag_part_elems(int np, int n) { return (size_t)((n + 255) / 256) * np + (size_t)((np + 255) / 256); }
size_t loo_u_part_elems(int np) { return (size_t)(np / 64) * np; }

template <typename T>
void launch_loo_diag(const T* Xinv, int np, int n, const T* y, const T* alpha, double* part, T* mean, T* var, T* lpd, double* avec,
                     double* sbvec, EvalOut* out, hipStream_t s) {
  const int nchunks = (n + 255) / 256;
  constexpr int TCOLS = 64 * Cfg<T>::VEC;
  hipLaunchKernelGGL((loo_colsq_kernel<T>), dim3((np + TCOLS - 1) / TCOLS, nchunks), dim3(256), 0, s, Xinv, np, n, part);
  double* sums = part + (size_t)nchunks * np;
  const int nblocks = (np + 255) / 256;
  hipLaunchKernelGGL((loo_diag_finish_kernel<T>), dim3(nblocks), dim3(256), 0, s, part, nchunks, np, n, y, alpha, mean, var, lpd, avec,
                     sbvec, sums);
  hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(64), 0, s, sums, nblocks, out);
}
template <typename T>
void launch_loo_uy(const T* Kinv, int np, int n, const double* avec, const double* sbvec, T* Y, double* pu, T* u, hipStream_t s) {
  const int nt = np / 64;
  hipLaunchKernelGGL((loo_uy_kernel<T>), dim3(nt * (nt + 1) / 2), dim3(256), 0, s, Kinv, np, n, avec, sbvec, Y, pu);
  hipLaunchKernelGGL((loo_u_finish_kernel<T>), dim3((np + 255) / 256), dim3(256), 0, s, pu, nt, np, u);
}
template <typename T>
void launch_loo_trace(const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Cm, const T* alpha, const T* u,
                      double* part, EvalOut* out, hipStream_t s) {
  const int nt = np / 64;
  const int ntiles = nt * (nt + 1) / 2;
  const size_t lds = (size_t)2 * d * 64 * sizeof(T);
  const dim3 grid(ntiles), block(256);
  const int* info = &out->info;
  switch (nu2) {
    case 0: hipLaunchKernelGGL((loo_trace_kernel<T, 0>), grid, block, lds, s, X, n, d, np, P, Cm, alpha, u, part, info); break;
    case 1: hipLaunchKernelGGL((loo_trace_kernel<T, 1>), grid, block, lds, s, X, n, d, np, P, Cm, alpha, u, part, info); break;
    case 3: hipLaunchKernelGGL((loo_trace_kernel<T, 3>), grid, block, lds, s, X, n, d, np, P, Cm, alpha, u, part, info); break;
    default: hipLaunchKernelGGL((loo_trace_kernel<T, 5>), grid, block, lds, s, X, n, d, np, P, Cm, alpha, u, part, info); break;
  }
  hipLaunchKernelGGL(finalize_grad_kernel, dim3(d + 2), dim3(256), 0, s, part, ntiles, d + 2, out, info);
}
#define LOO_INST(T)                                                                                                               \
  template void launch_loo_diag<T>(const T*, int, int, const T*, const T*, double*, T*, T*, T*, double*, double*, EvalOut*,       \
                                   hipStream_t);                                                                                  \
  template void launch_loo_uy<T>(const T*, int, int, const double*, const double*, T*, double*, T*, hipStream_t);                 \
  template void launch_loo_trace<T>(const T*, int, int, int, int, const EvalParams*, const T*, const T*, const T*, double*,       \
                                    EvalOut*, hipStream_t);
LOO_INST(double)
LOO_INST(float)
#undef LOO_INST

// =================================================================================================================
// Leave-group-out cross-validation in closed form.  For a group with the row set I, |I| = s <= LGO_MAX_GROUP:
//   Sigma_g = (M_II)^-1,  r_g = Sigma_g alpha_I,  mu_g = y_I - r_g,  lpd_g = -1/2 alpha_I^T r_g + 1/2 ln|M_II| - s/2 ln 2 pi
//   dlgo/dtheta_j = 1/2 sum_ab (u_a alpha_b + alpha_a u_b - 2 C_ab) dK_ab/dtheta_j,
//   a_I = r_g,  u = M a,  B_g = 1/2 (r_g r_g^T + Sigma_g) = F_g F_g^T,  Y[:, I] = M[:, I] F_g,  C = Y Y^T
// (the column of Y that belongs to the k-th member of a group is the column of that member's row index).  With s = 1 these are the
// leave-one-out formulas above.  Every sum is fp64 in a fixed order for both element types; no atomics on results.
// =================================================================================================================
// In-place Cholesky factor (lower) of the s x s matrix A (leading dimension ld) in the LDS, right-looking, one column per step, by
// the whole workgroup.  Returns false -- in every thread -- where a pivot is not > 0 (NaN included); the factor is then garbage.
__device__ __forceinline__ bool lgo_chol(double* A, int s, int ld) {
  const int t = threadIdx.x;
  bool ok = true;
  for (int k = 0; k < s; ++k) {
    __syncthreads();
    const double piv = A[k * ld + k];
    ok = ok && (piv > 0.0);
    const double dk = sqrt(piv);
    __syncthreads();  // everyone has read the pivot
    for (int i = k + t; i < s; i += 256) A[i * ld + k] = (i == k) ? dk : A[i * ld + k] / dk;
    __syncthreads();
    const int m = s - k - 1;
    for (int e = t; e < m * m; e += 256) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) A[i * ld + j] = __builtin_fma(-A[i * ld + k], A[j * ld + k], A[i * ld + j]);
    }
  }
  __syncthreads();
  return ok;
}

constexpr int LGO_STAGE = 2048;  // doubles of the Gram pass's row stage
size_t lgo_gram_lds_bytes(int smax) { return sizeof(double) * ((size_t)smax * (smax | 1) + LGO_STAGE); }
size_t lgo_group_lds_bytes(int smax) { return sizeof(double) * ((size_t)2 * smax * (smax | 1)); }
// Rows per chunk of a group's Gram sums: a function of the group's size alone, so that a group's sums never depend on the other
// groups.  Small groups take all rows in one workgroup (a workgroup per group fills the chip by their number); a group of 64 rows
// has 2080 sums over up to n rows each, 16 workgroups at n = 4096.
__host__ __device__ inline int lgo_chunk_rows(int s) { return s <= 4 ? (1 << 30) : s <= 16 ? 1024 : 256; }
int lgo_gram_chunks(int n, int smax) { return (n + lgo_chunk_rows(smax) - 1) / lgo_chunk_rows(smax); }

// Workgroup (g, c): the share of chunk c -- the rows c CH .. (c + 1) CH - 1 below n, CH = lgo_chunk_rows(s) -- in M_II, the Gram
// matrix of the group's columns of X = L^-1 (entries above the diagonal of X are never read; chunks that end above the group's
// first row have no share and are never read): 4 x 4 register tiles of the lower triangle, the rows of a stage dealt round-robin to
// `nsplit` thread sets whose sums are added in ascending order.  part[c][foff[g] + p s + q], q <= p.
template <typename T>
__global__ void __launch_bounds__(256) lgo_gram_kernel(const T* __restrict__ Xinv, int np, int n, LgoLists L, size_t f_elems,
                                                       double* __restrict__ part) {
  extern __shared__ __align__(16) char smem_raw[];
  __shared__ int idx[LGO_MAX_GROUP];
  const int g = blockIdx.x, t = threadIdx.x;
  const int p0 = L.goff[g], s = L.goff[g + 1] - p0;
  const int ld = L.smax | 1;
  double* A = reinterpret_cast<double*>(smem_raw);
  double* stage = A + (size_t)L.smax * ld;
  if (t < s) idx[t] = L.member[p0 + t];
  __syncthreads();
  const int CH = lgo_chunk_rows(s);
  const long long c_lo = (long long)blockIdx.y * CH;
  if (c_lo >= n || c_lo + CH <= idx[0]) return;  // (uniform) no such chunk for this group's size, or all of it above the first row
  const int row_begin = max((int)c_lo, idx[0]), row_end = (int)min((long long)n, c_lo + CH);
  {
    const int s4 = (s + 3) & ~3, t4 = s4 / 4, ntl = t4 * (t4 + 1) / 2;
    const int nsplit = min(64, 256 / ntl);
    const int R = min(256, LGO_STAGE / s4);
    const int tile = t % ntl, rs = t / ntl;
    const bool active = rs < nsplit;
    const int tp = tri_row(tile), tq = tile - tp * (tp + 1) / 2;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    for (int a0 = row_begin; a0 < row_end; a0 += R) {
      __syncthreads();
      for (int e = t; e < R * s4; e += 256) {
        const int r = e / s4, p = e - r * s4, a = a0 + r;
        double v = 0;
        if (p < s && a < row_end && a >= idx[p]) v = (double)Xinv[(size_t)a * np + idx[p]];
        stage[e] = v;
      }
      __syncthreads();
      if (active)
        for (int r = rs; r < R; r += nsplit) {
          double xp[4], xq[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { xp[i] = stage[r * s4 + 4 * tp + i]; xq[i] = stage[r * s4 + 4 * tq + i]; }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fma(xp[i], xq[j], acc[i][j]);
        }
    }
    for (int q = 0; q < nsplit; ++q) {
      __syncthreads();
      if (active && rs == q)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int pi = 4 * tp + i, pj = 4 * tq + j;
            if (pi < s && pj <= pi) A[pi * ld + pj] = (q == 0 ? 0.0 : A[pi * ld + pj]) + acc[i][j];
          }
    }
  }
  __syncthreads();
  double* out = part + (size_t)blockIdx.y * f_elems + L.foff[g];
  for (int e = t; e < s * s; e += 256) {
    const int p = e / s, q = e - p * s;
    if (q <= p) out[e] = A[p * ld + q];
  }
}

// One workgroup per group.  M_II = its chunks' shares from the first one that has any, in ascending order; then in the LDS:
// M_II = Lm Lm^T, W = Lm^-1, z = W alpha_I, r = W^T z (the two triangular solves, through the inverse factor), Sigma = W^T W, lpd from
// z^T z and diag Lm, B = F F^T.  Nothing depends on the group's label or on the other groups: the rows' results are a function of
// (X, alpha, I) alone.
template <typename T>
__global__ void __launch_bounds__(256) lgo_group_kernel(const double* __restrict__ part, size_t f_elems, int n, const T* __restrict__ y,
                                                        const T* __restrict__ alpha, LgoLists L, T* __restrict__ mean,
                                                        T* __restrict__ var, T* __restrict__ lpd, double* __restrict__ avec,
                                                        double* __restrict__ F, double* __restrict__ share, int* info) {
  extern __shared__ __align__(16) char smem_raw[];
  __shared__ int idx[LGO_MAX_GROUP];
  __shared__ double al[LGO_MAX_GROUP], z[LGO_MAX_GROUP], rr[LGO_MAX_GROUP];
  const int g = blockIdx.x, t = threadIdx.x;
  const int p0 = L.goff[g], s = L.goff[g + 1] - p0;
  const int ld = L.smax | 1;
  double* A = reinterpret_cast<double*>(smem_raw);
  double* W = A + (size_t)L.smax * ld;
  if (t < s) {
    idx[t] = L.member[p0 + t];
    al[t] = (double)alpha[idx[t]];
  }
  __syncthreads();
  {
    const int CH = lgo_chunk_rows(s);
    const int c0 = idx[0] / CH, c1 = (n + CH - 1) / CH;
    const double* in = part + L.foff[g];
    for (int e = t; e < s * s; e += 256) {
      const int p = e / s, q = e - p * s;
      if (q > p) continue;
      double v = 0;
      for (int c = c0; c < c1; ++c) v += in[(size_t)c * f_elems + e];
      A[p * ld + q] = v;
    }
  }
  bool ok = lgo_chol(A, s, ld);  // A = Lm
  if (t < s) {  // column t of W = Lm^-1
    for (int i = t; i < s; ++i) {
      double v = (i == t) ? 1.0 : 0.0;
      for (int k = t; k < i; ++k) v = __builtin_fma(-A[i * ld + k], W[k * ld + t], v);
      W[i * ld + t] = v / A[i * ld + i];
    }
  }
  __syncthreads();
  if (t < s) {
    double v = 0;
    for (int k = 0; k <= t; ++k) v = __builtin_fma(W[t * ld + k], al[k], v);
    z[t] = v;
  }
  double l = 0;
  if (t == 0) {  // before A is overwritten
    double ldet = 0;
    for (int k = 0; k < s; ++k) ldet += log(A[k * ld + k]);
    l = ldet;
  }
  __syncthreads();
  if (t < s) {
    double v = 0;
    for (int k = t; k < s; ++k) v = __builtin_fma(W[k * ld + t], z[k], v);
    rr[t] = v;
  }
  __syncthreads();
  for (int e = t; e < s * s; e += 256) {
    const int p = e / s, q = e - p * s;
    if (q > p) continue;
    double v = 0;
    for (int k = p; k < s; ++k) v = __builtin_fma(W[k * ld + p], W[k * ld + q], v);  // Sigma_pq
    if (p == q) {
      const int ip = idx[p];
      var[ip] = (T)v;
      mean[ip] = (T)((double)y[ip] - rr[p]);
      avec[ip] = rr[p];
    }
    A[p * ld + q] = 0.5 * (rr[p] * rr[q] + v);
  }
  ok = lgo_chol(A, s, ld) && ok;  // A = F
  double* Fg = F + L.foff[g];
  for (int e = t; e < s * s; e += 256) {
    const int q = e / s, k = e - q * s;
    Fg[e] = (k <= q) ? A[q * ld + k] : 0.0;
  }
  if (t == 0) {
    double zz = 0;
    for (int k = 0; k < s; ++k) zz = __builtin_fma(z[k], z[k], zz);
    l = l - 0.5 * zz - 0.5 * (double)s * log(2.0 * 3.14159265358979323846);
    if (!ok) {
      l = __builtin_nan("");
      atomicCAS(info, 0, 1 + idx[0]);
    }
    lpd[g] = (T)l;
    share[g] = l;
  }
}

// lgo = the groups' shares: thread t adds its run of consecutive dense ids in ascending order, thread 0 the 256 runs in order
__global__ void __launch_bounds__(256) lgo_sum_kernel(const double* __restrict__ share, int G, EvalOut* out) {
  __shared__ double runs[256];
  const int per = (G + 255) / 256, b = threadIdx.x * per;
  double s = 0;
  for (int g = b; g < min(b + per, G); ++g) s += share[g];
  runs[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = 0;
  for (int i = 0; i < 256; ++i) s += runs[i];
  out->lml = s;
  atomicOr(&out->done, 1);
}

// One workgroup per (bundle of consecutive groups with at most 64 rows together, 64-row block of K^-1): the 64 x 64 panel
// M[block, rows of the bundle] -- an entry above the diagonal is read at its mirror position, so the slot's unmirrored buffer and
// the model's full matrix give the same bits -- then Y[block, member] = sum_q M[., q] F_g[q, k] over the member's own group and the
// bundle's share of u = M a: pu[bundle][row], the bundle's rows in ascending list order.
template <typename T>
__global__ void __launch_bounds__(256) lgo_uy_kernel(const T* __restrict__ Kinv, int np, int n, LgoLists L,
                                                     const double* __restrict__ avec, const double* __restrict__ F,
                                                     T* __restrict__ Y, double* __restrict__ pu, const int* info) {
  extern __shared__ __align__(16) char smem_raw[];
  __shared__ int col[64], gs[64], ge[64], fo[64];
  __shared__ double av[64];
  if (*info != 0) return;
  double* Fl = reinterpret_cast<double*>(smem_raw);  // [64][64], block diagonal
  T* tile = reinterpret_cast<T*>(Fl + 64 * 64);      // [64][65]
  const int b = blockIdx.x, a0 = blockIdx.y * 64;
  const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
  const int pb0 = L.goff[L.boff[b]], cnt = L.goff[L.boff[b + 1]] - pb0;
  if (t < 64) {
    int c = 0, s0 = 0, s1 = 0, f = 0;
    double a = 0;
    if (t < cnt) {
      const int g = L.gid[pb0 + t];
      c = L.member[pb0 + t];
      s0 = L.goff[g] - pb0;
      s1 = L.goff[g + 1] - pb0;
      f = L.foff[g];
      a = avec[c];
    }
    col[t] = c; gs[t] = s0; ge[t] = s1; fo[t] = f; av[t] = a;
  }
  __syncthreads();
  for (int e = t; e < 64 * 64; e += 256) {
    const int q = e >> 6, k = e & 63;
    double v = 0;
    if (q < cnt && k < cnt && gs[q] == gs[k]) v = F[(size_t)fo[k] + (size_t)(q - gs[k]) * (ge[k] - gs[k]) + (k - gs[k])];
    Fl[e] = v;
  }
  // the panel: lanes along the bundle's rows where the entry lies on or below the diagonal, along the block's rows where above
  for (int r = ty; r < 64; r += 4) {
    const int ga = a0 + r;
    if (tx < cnt && ga < n && ga >= col[tx]) tile[r * 65 + tx] = Kinv[(size_t)ga * np + col[tx]];
  }
  for (int q = ty; q < 64; q += 4) {
    const int ga = a0 + tx;
    T v = T(0);
    const bool upper = q < cnt && ga < col[q];
    if (upper) v = Kinv[(size_t)col[q] * np + ga];
    if (upper || q >= cnt || ga >= n) tile[tx * 65 + q] = v;
  }
  __syncthreads();
  if (tx < cnt) {
    const int ke = ge[tx], c = col[tx];
    for (int r = ty; r < 64; r += 4) {
      double sum = 0;
      for (int q = tx; q < ke; ++q) sum = __builtin_fma((double)tile[r * 65 + q], Fl[q * 64 + tx], sum);
      Y[(size_t)(a0 + r) * np + c] = (T)sum;
    }
  }
  if (t < 64) {
    double sum = 0;
    for (int q = 0; q < cnt; ++q) sum = __builtin_fma((double)tile[t * 65 + q], av[q], sum);
    pu[(size_t)b * np + a0 + t] = sum;
  }
}

size_t lgo_uy_lds_bytes(bool is_f32) { return sizeof(double) * 64 * 64 + (is_f32 ? sizeof(float) : sizeof(double)) * 64 * 65; }

template <typename T>
void launch_lgo_group(const T* Xinv, int np, int n, const T* y, const T* alpha, const LgoLists& L, size_t f_elems, double* part, T* mean,
                      T* var, T* lpd, double* avec, double* F, double* share, EvalOut* out, hipStream_t s) {
  hipLaunchKernelGGL((lgo_gram_kernel<T>), dim3(L.G, lgo_gram_chunks(n, L.smax)), dim3(256), lgo_gram_lds_bytes(L.smax), s, Xinv, np, n, L,
                     f_elems, part);
  hipLaunchKernelGGL((lgo_group_kernel<T>), dim3(L.G), dim3(256), lgo_group_lds_bytes(L.smax), s, part, f_elems, n, y, alpha, L, mean, var,
                     lpd, avec, F, share, &out->info);
  hipLaunchKernelGGL(lgo_sum_kernel, dim3(1), dim3(256), 0, s, share, L.G, out);
}
template <typename T>
void launch_lgo_uy(const T* Kinv, int np, int n, const LgoLists& L, const double* avec, const double* F, T* Y, double* pu, T* u,
                   const int* info, hipStream_t s) {
  hipLaunchKernelGGL((lgo_uy_kernel<T>), dim3(L.nb, np / 64), dim3(256), lgo_uy_lds_bytes(sizeof(T) == 4), s, Kinv, np, n, L, avec, F, Y,
                     pu, info);
  hipLaunchKernelGGL((loo_u_finish_kernel<T>), dim3((np + 255) / 256), dim3(256), 0, s, pu, L.nb, np, u);
}
#define LGO_INST(T)                                                                                                                  \
  template void launch_lgo_group<T>(const T*, int, int, const T*, const T*, const LgoLists&, size_t, double*, T*, T*, T*, double*, \
                                    double*, double*, EvalOut*, hipStream_t);                                                        \
  template void launch_lgo_uy<T>(const T*, int, int, const LgoLists&, const double*, const double*, T*, double*, T*, const int*,    \
                                 hipStream_t);
LGO_INST(double)
LGO_INST(float)
#undef LGO_INST

// =================================================================================================================
// symmetrize: mirror the lower triangle into the upper one (what invc() hands back, lml.rs:62)
// =================================================================================================================
template <typename T>
__global__ void __launch_bounds__(256) symmetrize_kernel(T* __restrict__ A, int np) {
  __shared__ T tile[64][65];
  const int li = tri_row(blockIdx.x), lj = blockIdx.x - li * (li + 1) / 2;
  const int i0 = li * 64, j0 = lj * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) tile[r][tx] = A[(size_t)(i0 + r) * np + j0 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    // element (j0+r, i0+tx) = A[i0+tx][j0+r]
    if (li != lj || tx > r) A[(size_t)(j0 + r) * np + i0 + tx] = tile[tx][r];
  }
}
template <typename T>
void launch_symmetrize(T* A, int np, hipStream_t s) {
  const int nt = np / 64;
  hipLaunchKernelGGL((symmetrize_kernel<T>), dim3(nt * (nt + 1) / 2), dim3(256), 0, s, A, np);
}
template void launch_symmetrize<double>(double*, int, hipStream_t);
template void launch_symmetrize<float>(float*, int, hipStream_t);

// flag |= 1 when a[0..count) and b[0..count) differ anywhere (bitwise comparison of the stored values)
template <typename T>
__global__ void __launch_bounds__(256) prefix_differs_kernel(const T* __restrict__ a, const T* __restrict__ b, size_t count,
                                                             int* __restrict__ flag) {
  bool diff = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) diff |= !(a[i] == b[i]);
  if (diff) atomicOr(flag, 1);
}
template <typename T>
void launch_prefix_differs(const T* a, const T* b, size_t count, int* flag, hipStream_t s) {
  if (count == 0) return;
  const int blocks = (int)std::min<size_t>(1024, (count + 255) / 256);
  hipLaunchKernelGGL((prefix_differs_kernel<T>), dim3(blocks), dim3(256), 0, s, a, b, count, flag);
}
template void launch_prefix_differs<double>(const double*, const double*, size_t, int*, hipStream_t);
template void launch_prefix_differs<float>(const float*, const float*, size_t, int*, hipStream_t);

// =================================================================================================================
// predict (predict.rs:7-52)
// =================================================================================================================
// Kstar[mp][np]: row = candidate.  64x64 tiles as in kmat, no noise, zero padding.
template <typename T>
__global__ void __launch_bounds__(256) kstar_kernel(const T* __restrict__ Xs, int m, const T* __restrict__ X, int n, int d,
                                                    int np, int nu2, const EvalParams* __restrict__ P, T* __restrict__ Ks) {
  extern __shared__ __align__(16) char smem_raw[];
  T* xi = reinterpret_cast<T*>(smem_raw);
  T* xj = xi + (size_t)d * 64;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int t = threadIdx.x;
  for (int e = t; e < 64 * d; e += 256) {
    const int row = e / d, k = e - row * d;
    const T ell = (T)P->ell[k];
    const int gi = i0 + row, gj = j0 + row;
    xi[k * 64 + row] = (gi < m) ? Xs[(size_t)gi * d + k] / ell : T(0);
    xj[k * 64 + row] = (gj < n) ? X[(size_t)gj * d + k] / ell : T(0);
  }
  __syncthreads();
  const int tx = t & 15, ty = t >> 4;
  T acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = T(0);
  for (int k = 0; k < d; ++k) {
    T a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = xi[k * 64 + ty + 16 * r];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = xj[k * 64 + tx * 4 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const T df = a[r] - b[c];
        acc[r][c] += df * df;
      }
  }
  const T amp = (T)P->amp;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = i0 + ty + 16 * r;
    T* p = Ks + (size_t)gi * np + j0 + tx * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gj = j0 + tx * 4 + c;
      p[c] = (gi < m && gj < n) ? kmat_entry<T>(acc[r][c], nu2, amp, T(0), false) : T(0);
    }
  }
}
template <typename T>
void launch_kstar(const T* Xs, int m, int mp, const T* X, int n, int d, int np, int nu2, const EvalParams* P, T* Ks,
                  hipStream_t s) {
  const size_t lds = (size_t)2 * d * 64 * sizeof(T);
  hipLaunchKernelGGL((kstar_kernel<T>), dim3(np / 64, mp / 64), dim3(256), lds, s, Xs, m, X, n, d, np, nu2, P, Ks);
}
template void launch_kstar<double>(const double*, int, int, const double*, int, int, int, int, const EvalParams*, double*,
                                   hipStream_t);
template void launch_kstar<float>(const float*, int, int, const float*, int, int, int, int, const EvalParams*, float*,
                                  hipStream_t);

// mean_k = sum_j Kstar[k][j] alpha[j]  (predict.rs:19); one wave per candidate
template <typename T>
__global__ void __launch_bounds__(256) pred_mean_kernel(const T* __restrict__ Ks, int m, int np, const T* __restrict__ alpha,
                                                        T* __restrict__ mean) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  double acc = 0;
  const T* kr = Ks + (size_t)row * np;
  for (int j = lane; j < np; j += 64) acc += (double)kr[j] * (double)alpha[j];
  acc = wave_sum(acc);
  if (lane == 0) mean[row] = (T)acc;
}
template <typename T>
void launch_pred_mean(const T* Ks, int m, int np, const T* alpha, T* mean, hipStream_t s) {
  hipLaunchKernelGGL((pred_mean_kernel<T>), dim3((m + 3) / 4), dim3(256), 0, s, Ks, m, np, alpha, mean);
}
template void launch_pred_mean<double>(const double*, int, int, const double*, double*, hipStream_t);
template void launch_pred_mean<float>(const float*, int, int, const float*, float*, hipStream_t);

// var_k = c + 1e-5 - sum_j Q[k][j] Kstar[k][j], clamp negatives, count those below -sqrt(1e-5)  (predict.rs:25-48)
template <typename T>
__global__ void __launch_bounds__(256) pred_var_kernel(const T* __restrict__ Ks, const T* __restrict__ Q, int m, int np,
                                                       const EvalParams* __restrict__ P, T* __restrict__ var, EvalOut* out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  double acc = 0;
  const T* kr = Ks + (size_t)row * np;
  const T* qr = Q + (size_t)row * np;
  for (int j = lane; j < np; j += 64) acc += (double)kr[j] * (double)qr[j];
  acc = wave_sum(acc);
  if (lane == 0) {
    const T min_noise = (T)1e-5;
    T v = (T)P->amp + min_noise - (T)acc;
    if (v < -sqrt(min_noise)) atomicAdd(&out->n_warn, 1);
    if (v < T(0)) v = T(0);
    var[row] = v;
  }
}
template <typename T>
void launch_pred_var(const T* Ks, const T* Q, int m, int np, const EvalParams* P, T* var, EvalOut* out, hipStream_t s) {
  hipLaunchKernelGGL((pred_var_kernel<T>), dim3((m + 3) / 4), dim3(256), 0, s, Ks, Q, m, np, P, var, out);
}
template void launch_pred_var<double>(const double*, const double*, int, int, const EvalParams*, double*, EvalOut*, hipStream_t);
template void launch_pred_var<float>(const float*, const float*, int, int, const EvalParams*, float*, EvalOut*, hipStream_t);

// =================================================================================================================
// posterior gradient at the candidates: the derivative of predict (predict.rs:7-52) w.r.t. the query point x*
//   dk_j/dx*_k = c psi(r_j) (x*_k - x_jk) / ell_k^2 = c psi(r_j) (s*_k - s_jk) / ell_k,   s = x / ell,  psi = phi'(r) / r
//   dmean_k = sum_j dk_j/dx*_k alpha_j
//   dvar_k  = -2 (dk/dx*_k)^T K^-1 k* = -2 (L^-1 dk/dx*_k) . (L^-1 k*) = -2 rowsum(W_k o Q),   W_k = G_k X^T (tile GEMM)
// The variance gradient goes through L^-1 like the variance itself (|L^-1 k*|^2): both factors are bounded (|L^-1 k*|^2 <= c),
// whereas V = K^-1 k* itself grows with cond(K) and the sum over V cancels -- measured on the fitted config-M model
// (cond(K) = 6.7e11) the V forms were off by 100 % of the gradient's scale.
// A training point at r = 0 contributes 0 for every order (the limit for nu >= 3/2; a choice for nu = 1/2, where k has a kink).
//
// pred_grad_kernel (dmean): grid (ceil(m/4), ceil(n/PG_CHUNK)); wave w of a workgroup is candidate row 4 blockIdx.x + w, lane
// l takes the training points j0 + l of the chunk, 64 at a time through the LDS (features scaled as in kstar_kernel, r^2
// accumulated in the same order and type).  psi and the sums are fp64 for both element types; per-lane sums over PG_KB
// features per pass over the chunk, then one wave_sum each: part[chunk][row][k].  pred_grad_finish_kernel adds the chunks in
// ascending order.
// kstar_grad_kernel writes G[k][i][j] = dk_j/dx*_i,k (zero padding, like Kstar); pred_dvar_kernel: one wave per (k, row).
// No atomics anywhere: the same rows give the same bits.
// =================================================================================================================
constexpr int PG_CHUNK = 512;  // training points per workgroup
constexpr int PG_KB = 16;      // features per pass (16 fp64 accumulators per lane)

// psi(r) = phi'(r) / r of matern_map, from r^2 (> 0)
__device__ __forceinline__ double matern_psi(double r2, int nu2) {
#pragma clang fp contract(off)
  if (nu2 == 0) return -exp_nonpos(-0.5 * r2);
  const double r = sqrt_nonneg(r2);
  if (nu2 == 1) return -exp_nonpos(-r) / r;
  if (nu2 == 3) return -3.0 * exp_nonpos(-1.7320508075688772 * r);
  const double k = 2.23606797749979 * r;
  return -(5.0 / 3.0) * (1.0 + k) * exp_nonpos(-k);
}

template <typename T>
__global__ void __launch_bounds__(256) pred_grad_kernel(const T* __restrict__ Xs, int m, const T* __restrict__ X, int n, int d, int nu2,
                                                        const EvalParams* __restrict__ P, const T* __restrict__ alpha,
                                                        double* __restrict__ part) {
  extern __shared__ __align__(16) char smem_raw[];
  T* sx = reinterpret_cast<T*>(smem_raw);  // [d][64] scaled features of 64 training points
  T* sq = sx + (size_t)d * 64;             // [4][d] scaled features of this workgroup's candidates
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int row = blockIdx.x * 4 + w;
  const bool live = row < m;
  const int jc0 = blockIdx.y * PG_CHUNK, jc1 = min(n, jc0 + PG_CHUNK);
  const double amp = P->amp;
  for (int e = t; e < 4 * d; e += 256) {
    const int q = e / d, k = e - q * d, gi = blockIdx.x * 4 + q;
    sq[e] = (gi < m) ? Xs[(size_t)gi * d + k] / (T)P->ell[k] : T(0);
  }
  const T* xq = sq + w * d;
  for (int kb = 0; kb < d; kb += PG_KB) {
    double am[PG_KB];
#pragma unroll
    for (int kk = 0; kk < PG_KB; ++kk) am[kk] = 0.0;
    for (int j0 = jc0; j0 < jc1; j0 += 64) {
      __syncthreads();  // the previous 64 points are consumed (first time: sq is written)
      for (int e = t; e < 64 * d; e += 256) {
        const int jj = e / d, k = e - jj * d, gj = j0 + jj;
        sx[k * 64 + jj] = (gj < n) ? X[(size_t)gj * d + k] / (T)P->ell[k] : T(0);
      }
      __syncthreads();
      const int j = j0 + lane;
      if (live && j < jc1) {
        T r2 = T(0);
        for (int k = 0; k < d; ++k) {  // kstar_kernel's accumulation (cdist order, matern_kernel.rs:274-278)
          const T df = xq[k] - sx[k * 64 + lane];
          r2 += df * df;
        }
        const double a = (r2 == T(0)) ? 0.0 : amp * matern_psi((double)r2, nu2) * (double)alpha[j];
#pragma unroll
        for (int kk = 0; kk < PG_KB; ++kk)
          if (kb + kk < d) am[kk] += a * (double)(xq[kb + kk] - sx[(kb + kk) * 64 + lane]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < PG_KB; ++kk) {
      if (kb + kk < d) {
        const double sm = wave_sum(am[kk]);
        if (live && lane == 0) part[((size_t)blockIdx.y * m + row) * d + kb + kk] = sm;
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) pred_grad_finish_kernel(const double* __restrict__ part, int nch, int m, int d,
                                                               const EvalParams* __restrict__ P, T* __restrict__ dmean) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m * d) return;
  const int k = e % d;
  double sm = 0.0;
  for (int c = 0; c < nch; ++c) sm += part[(size_t)c * m * d + e];
  dmean[e] = (T)(sm / P->ell[k]);
}

// G[k][i][j] (k < d, i < mp, j < np) = dk(x*_i, x_j) / dx*_i,k; 0 for i >= m or j >= n.  One thread per (i, j), all d features.
template <typename T>
__global__ void __launch_bounds__(256) kstar_grad_kernel(const T* __restrict__ Xs, int m, int mp, const T* __restrict__ X, int n, int d,
                                                         int np, int nu2, const EvalParams* __restrict__ P, T* __restrict__ G) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= np) return;
  const size_t plane = (size_t)mp * np, at = (size_t)i * np + j;
  if (i >= m || j >= n) {
    for (int k = 0; k < d; ++k) G[k * plane + at] = T(0);
    return;
  }
  T r2 = T(0);
  for (int k = 0; k < d; ++k) {
    const T ell = (T)P->ell[k];
    const T df = Xs[(size_t)i * d + k] / ell - X[(size_t)j * d + k] / ell;
    r2 += df * df;
  }
  const double g = (r2 == T(0)) ? 0.0 : P->amp * matern_psi((double)r2, nu2);
  for (int k = 0; k < d; ++k) {
    const T ell = (T)P->ell[k];
    const T df = Xs[(size_t)i * d + k] / ell - X[(size_t)j * d + k] / ell;
    G[k * plane + at] = (T)(g * (double)df / P->ell[k]);
  }
}

// dvar[i][k] = -2 sum_j W[k][i][j] Q[i][j]; 0 where the variance was clamped to 0 (a NaN variance keeps its NaN).  One wave per (k, i).
template <typename T>
__global__ void __launch_bounds__(256) pred_dvar_kernel(const T* __restrict__ W, const T* __restrict__ Q, int m, int mp, int np, int d,
                                                        const T* __restrict__ var, T* __restrict__ dvar) {
  const int lane = threadIdx.x & 63, item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= m * d) return;
  const int k = item / m, i = item - k * m;
  const T* wr = W + ((size_t)k * mp + i) * np;
  const T* qr = Q + (size_t)i * np;
  double acc = 0.0;
  for (int j = lane; j < np; j += 64) acc += (double)wr[j] * (double)qr[j];
  acc = wave_sum(acc);
  if (lane == 0) dvar[(size_t)i * d + k] = (var[i] == T(0)) ? T(0) : (T)(-2.0 * acc);
}

template <typename T>
void launch_pred_grad(const T* Xs, int m, const T* X, int n, int d, int nu2, const EvalParams* P, const T* alpha, double* part, T* dmean,
                      hipStream_t s) {
  const int nch = (n + PG_CHUNK - 1) / PG_CHUNK;
  const size_t lds = (size_t)(64 + 4) * d * sizeof(T);
  hipLaunchKernelGGL((pred_grad_kernel<T>), dim3((m + 3) / 4, nch), dim3(256), lds, s, Xs, m, X, n, d, nu2, P, alpha, part);
  hipLaunchKernelGGL((pred_grad_finish_kernel<T>), dim3((m * d + 255) / 256), dim3(256), 0, s, part, nch, m, d, P, dmean);
}
template <typename T>
void launch_kstar_grad(const T* Xs, int m, int mp, const T* X, int n, int d, int np, int nu2, const EvalParams* P, T* G, hipStream_t s) {
  hipLaunchKernelGGL((kstar_grad_kernel<T>), dim3((np + 255) / 256, mp), dim3(256), 0, s, Xs, m, mp, X, n, d, np, nu2, P, G);
}
template <typename T>
void launch_pred_dvar(const T* W, const T* Q, int m, int mp, int np, int d, const T* var, T* dvar, hipStream_t s) {
  hipLaunchKernelGGL((pred_dvar_kernel<T>), dim3((m * d + 3) / 4), dim3(256), 0, s, W, Q, m, mp, np, d, var, dvar);
}
template void launch_pred_grad<double>(const double*, int, const double*, int, int, int, const EvalParams*, const double*, double*, double*,
                                       hipStream_t);
template void launch_pred_grad<float>(const float*, int, const float*, int, int, int, const EvalParams*, const float*, double*, float*,
                                      hipStream_t);
template void launch_kstar_grad<double>(const double*, int, int, const double*, int, int, int, int, const EvalParams*, double*, hipStream_t);
template void launch_kstar_grad<float>(const float*, int, int, const float*, int, int, int, int, const EvalParams*, float*, hipStream_t);
template void launch_pred_dvar<double>(const double*, const double*, int, int, int, int, const double*, double*, hipStream_t);
template void launch_pred_dvar<float>(const float*, const float*, int, int, int, int, const float*, float*, hipStream_t);
int pred_grad_chunks(int n) { return (n + PG_CHUNK - 1) / PG_CHUNK; }

// =================================================================================================================
// sensitivity of the posterior mean: the mean at base rows with ONE coordinate substituted (hbegp_sobol_* /
// hbegp_main_effects_*)
//   mu(a | k <- s) = sum_j c phi(r_j) alpha_j,   r_j^2 = sum_{l != k} ((a_l - x_jl) / ell_l)^2 + ((s - x_jk) / ell_k)^2
// No query matrix and no Kstar exist: for a pair (base row, training point) the squared differences of the features are formed
// once per pass, a substituted point replaces one term of the sum, and only the Matern map and one FMA scale with the number of
// substituted points.
//
// sens_kernel: pred_grad_kernel's shape -- grid (ceil(rows/4), ceil(n/SENS_CHUNK)); wave w of a workgroup is base row
// 4 blockIdx.x + w of the slab, lane l takes the training points j0 + l of the chunk, 64 at a time through the LDS (features
// scaled as in kstar_kernel, terms accumulated in T).  One pass over the chunk takes KB features x VB values: KB x VB fp64
// sums per lane (the map and the sums are fp64 for both element types), then one wave_sum each: part[chunk][row][1 + k GV + g].
//   per row (GRID = false, GV = 1): the value of feature k of row i is sub[i][k]             -- pick-freeze, KB = 8, VB = 1
//   per grid (GRID = true, GV = G): the values of feature k are sg[k][0..G), already / ell_k -- main effects, KB = 2, VB = 8
// r^2 of a substituted point is a sum of NON-NEGATIVE terms only, never r^2_base - t_k + u_k (at nu = 1/2 the square root turns
// a cancellation residue of 1e-17 into 3e-9 of the amplitude per training point): with t_l the terms of the pass,
//   r^2 = ((sum_{l < kb} t_l + t_kb + .. + t_{k-1}) + (t_{k+1} + (.. + (t_{kb+KB-1} + sum_{l >= kb+KB} t_l)))) + u_k
// so a substituted point that coincides with a training point has r^2 == 0 exactly.  The two outer sums are re-read from the LDS
// per pass (d - KB terms; the maps of the pass cost KB x VB x ~40 fp64 instructions).
// The base value mu(a) (part[chunk][row][0]) comes from the first pass, r^2 in kstar_kernel's order.  Rows from nsub on (the
// second sample matrix of the pick-freeze scheme) get the base value only: their workgroups make one pass.
// No atomics; every value depends on its own row (and k, and the value) only: the same bits alone, in a batch or in any slab.
// sens_finish_kernel adds the chunks in ascending order; the reductions below are fixed-order fp64.
// =================================================================================================================
constexpr int SENS_CHUNK = 512;  // training points per workgroup

template <typename T, int NU2, int KB, int VB, bool GRID>
__global__ void __launch_bounds__(256) sens_kernel(const T* __restrict__ Xb, int r0, int rows, int nsub, const T* __restrict__ sub, int G,
                                                   const T* __restrict__ X, int n, int d, const EvalParams* __restrict__ P,
                                                   const T* __restrict__ alpha, double* __restrict__ part) {
  extern __shared__ __align__(16) char smem_raw[];
  T* sx = reinterpret_cast<T*>(smem_raw);  // [d][64] scaled features of 64 training points
  T* sq = sx + (size_t)d * 64;             // [4][d] scaled features of this workgroup's base rows
  T* sb = sq + 4 * d;                      // [4][d] their scaled substitution values (per row)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r = blockIdx.x * 4 + w;  // row of the slab
  const bool live = r < rows;
  const bool wsub = live && r0 + r < nsub;
  const bool any_sub = r0 + blockIdx.x * 4 < nsub;  // rows ascend: the workgroup's first row decides
  const int GV = GRID ? G : 1;
  const int nv = 1 + d * GV;
  const int jc0 = blockIdx.y * SENS_CHUNK, jc1 = min(n, jc0 + SENS_CHUNK);
  const double amp = P->amp;
  for (int e = t; e < 4 * d; e += 256) {
    const int q = e / d, k = e - q * d, rq = blockIdx.x * 4 + q;
    const size_t gi = (size_t)r0 + rq;
    sq[e] = (rq < rows) ? Xb[gi * d + k] / (T)P->ell[k] : T(0);
    if (!GRID) sb[e] = (rq < rows && gi < (size_t)nsub) ? sub[gi * d + k] / (T)P->ell[k] : T(0);
  }
  const T* xq = sq + w * d;
  const T* xb = sb + w * d;
  double* prow = part + ((size_t)blockIdx.y * rows + (live ? r : 0)) * nv;
  const int kend = any_sub ? d : 1, gend = any_sub ? GV : 1;  // base rows only: one pass, for the base value
  for (int kb = 0; kb < kend; kb += KB) {
    for (int gb = 0; gb < gend; gb += VB) {
      const bool first = kb == 0 && gb == 0;
      double acc[KB][VB];
#pragma unroll
      for (int kk = 0; kk < KB; ++kk)
#pragma unroll
        for (int v = 0; v < VB; ++v) acc[kk][v] = 0.0;
      double accb = 0.0;
      for (int j0 = jc0; j0 < jc1; j0 += 64) {
        __syncthreads();  // the previous 64 points are consumed (first time: sq / sb are written)
        for (int e = t; e < 64 * d; e += 256) {
          const int jj = e / d, k = e - jj * d, gj = j0 + jj;
          sx[k * 64 + jj] = (gj < n) ? X[(size_t)gj * d + k] / (T)P->ell[k] : T(0);
        }
        __syncthreads();
        const int j = j0 + lane;
        if (live && j < jc1) {
          const double aj = amp * (double)alpha[j];
          if (first) {
            T r2 = T(0);
            for (int k = 0; k < d; ++k) {  // kstar_kernel's accumulation (cdist order, matern_kernel.rs:274-278)
              const T df = xq[k] - sx[k * 64 + lane];
              r2 += df * df;
            }
            accb += aj * matern_map<double>(sqrt_nonneg((double)r2), NU2);
          }
          if (wsub) {
            T pfx = T(0), post = T(0);
            for (int l = 0; l < kb; ++l) {
              const T df = xq[l] - sx[l * 64 + lane];
              pfx += df * df;
            }
            for (int l = kb + KB; l < d; ++l) {
              const T df = xq[l] - sx[l * 64 + lane];
              post += df * df;
            }
            T tt[KB], xj[KB], sfx[KB];
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
              const bool in = kb + kk < d;
              xj[kk] = in ? sx[(kb + kk) * 64 + lane] : T(0);
              const T df = in ? xq[kb + kk] - xj[kk] : T(0);
              tt[kk] = df * df;
            }
            sfx[KB - 1] = post;
#pragma unroll
            for (int kk = KB - 2; kk >= 0; --kk) sfx[kk] = tt[kk + 1] + sfx[kk + 1];
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
              if (kb + kk < d) {
                const T others = pfx + sfx[kk];
#pragma unroll
                for (int v = 0; v < VB; ++v) {
                  if (gb + v < GV) {
                    const T sv = GRID ? sub[(size_t)(kb + kk) * G + gb + v] : xb[kb + kk];
                    const T df = sv - xj[kk];
                    const T r2 = others + df * df;
                    acc[kk][v] += aj * matern_map<double>(sqrt_nonneg((double)r2), NU2);
                  }
                }
                pfx += tt[kk];
              }
            }
          }
        }
      }
      if (first) {
        const double sm = wave_sum(accb);
        if (live && lane == 0) prow[0] = sm;
      }
      if (any_sub) {
#pragma unroll
        for (int kk = 0; kk < KB; ++kk)
#pragma unroll
          for (int v = 0; v < VB; ++v)
            if (kb + kk < d && gb + v < GV) {
              const double sm = wave_sum(acc[kk][v]);
              if (wsub && lane == 0) prow[1 + (size_t)(kb + kk) * GV + gb + v] = sm;
            }
      }
    }
  }
}

// sg[k][g] = grid[k][g] / ell_k (in place), the scaling of every feature in T
template <typename T>
__global__ void __launch_bounds__(256) sens_scale_grid_kernel(T* __restrict__ sg, int d, int G, const EvalParams* __restrict__ P) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)d * G) return;
  sg[e] = sg[e] / (T)P->ell[e / G];
}

// One thread per (row of the slab, value): the chunks in ascending order.  Value 0 -> fbase[r0 + row] (T); value 1 + k of row
// i < nsub -> fsub[k][i] (T, leading dimension nsub) per row, or, per grid, back into chunk 0's slot as fp64 for sens_effect_kernel.
template <typename T, bool GRID>
__global__ void __launch_bounds__(256) sens_finish_kernel(double* __restrict__ part, int nch, int r0, int rows, int nsub, int nv,
                                                          T* __restrict__ fbase, T* __restrict__ fsub) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)rows * nv;
  if (e >= per) return;
  const size_t r = e / nv, gi = (size_t)r0 + r;
  const int v = (int)(e - r * nv);
  if (v > 0 && gi >= (size_t)nsub) return;  // never written: a base row of the second sample matrix
  double sm = 0.0;
  for (int c = 0; c < nch; ++c) sm += part[(size_t)c * per + e];
  if (v == 0) fbase[gi] = (T)sm;
  else if (GRID) part[e] = sm;
  else fsub[(size_t)(v - 1) * nsub + gi] = (T)sm;
}

// eff[k][g] += the slab's rows in ascending order (one thread per (k, g)): whatever the slabs, the sum over the rows runs
// 0, 1, 2, ...; the last slab divides by N.
__global__ void __launch_bounds__(256) sens_effect_kernel(const double* __restrict__ part, int rows, int nv, double* __restrict__ eff, int N,
                                                          int last) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nv - 1) return;
  double acc = eff[e];
  for (int r = 0; r < rows; ++r) acc += part[(size_t)r * nv + 1 + e];
  eff[e] = last ? acc / (double)N : acc;
}

// The pick-freeze estimators (Saltelli et al. 2010 for the first-order index, Jansen 1999 for the total index) from the T values
// the caller gets: fbase = [f_A | f_B] (N each), fsub[k][i] = f_AB.  One workgroup; thread t adds i = t, t + 256, ... in ascending
// order, then block_sum.  out: first[d], total[d], f0, V.
template <typename T>
__global__ void __launch_bounds__(256) sobol_reduce_kernel(const T* __restrict__ fbase, const T* __restrict__ fsub, int N, int d,
                                                           double* __restrict__ out) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < 2 * N; i += 256) s += (double)fbase[i];
  const double f0 = block_sum(s, red) / (2.0 * N);
  s = 0.0;
  for (int i = t; i < 2 * N; i += 256) {
    const double dv = (double)fbase[i] - f0;
    s += dv * dv;
  }
  const double V = block_sum(s, red) / (2.0 * N);
  for (int k = 0; k < d; ++k) {
    double s1 = 0.0, st = 0.0;
    for (int i = t; i < N; i += 256) {
      const double fa = (double)fbase[i], fb = (double)fbase[N + i], fab = (double)fsub[(size_t)k * N + i];
      s1 += (fb - f0) * (fab - fa);
      st += (fa - fab) * (fa - fab);
    }
    s1 = block_sum(s1, red);
    st = block_sum(st, red);
    if (t == 0) {
      out[k] = (V == 0.0) ? 0.0 : s1 / N / V;
      out[d + k] = (V == 0.0) ? 0.0 : st / (2.0 * N) / V;
    }
  }
  if (t == 0) {
    out[2 * d] = f0;
    out[2 * d + 1] = V;
  }
}

int sens_chunks(int n) { return (n + SENS_CHUNK - 1) / SENS_CHUNK; }

template <typename T, int NU2>
static void launch_sens_eval_nu(const T* Xb, int r0, int rows, int nsub, const T* sub, int G, const T* X, int n, int d, const EvalParams* P,
                                const T* alpha, double* part, hipStream_t s) {
  const dim3 grid((rows + 3) / 4, sens_chunks(n));
  const size_t lds = (size_t)(64 + 8) * d * sizeof(T);
  if (G > 0)
    hipLaunchKernelGGL((sens_kernel<T, NU2, 2, 8, true>), grid, dim3(256), lds, s, Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part);
  else
    hipLaunchKernelGGL((sens_kernel<T, NU2, 8, 1, false>), grid, dim3(256), lds, s, Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part);
}
template <typename T>
void launch_sens_eval(const T* Xb, int r0, int rows, int nsub, const T* sub, int G, const T* X, int n, int d, int nu2, const EvalParams* P,
                      const T* alpha, double* part, T* fbase, T* fsub, hipStream_t s, hipEvent_t ev_mid) {
  if (nu2 == 0) launch_sens_eval_nu<T, 0>(Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part, s);
  else if (nu2 == 1) launch_sens_eval_nu<T, 1>(Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part, s);
  else if (nu2 == 3) launch_sens_eval_nu<T, 3>(Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part, s);
  else launch_sens_eval_nu<T, 5>(Xb, r0, rows, nsub, sub, G, X, n, d, P, alpha, part, s);
  if (ev_mid) (void)hipEventRecord(ev_mid, s);
  const int nv = 1 + d * (G > 0 ? G : 1);
  const unsigned nb = (unsigned)(((size_t)rows * nv + 255) / 256);
  if (G > 0)
    hipLaunchKernelGGL((sens_finish_kernel<T, true>), dim3(nb), dim3(256), 0, s, part, sens_chunks(n), r0, rows, nsub, nv, fbase, fsub);
  else
    hipLaunchKernelGGL((sens_finish_kernel<T, false>), dim3(nb), dim3(256), 0, s, part, sens_chunks(n), r0, rows, nsub, nv, fbase, fsub);
}
template <typename T>
void launch_sens_scale_grid(T* sg, int d, int G, const EvalParams* P, hipStream_t s) {
  hipLaunchKernelGGL((sens_scale_grid_kernel<T>), dim3((unsigned)(((size_t)d * G + 255) / 256)), dim3(256), 0, s, sg, d, G, P);
}
void launch_sens_effect(const double* part, int rows, int d, int G, double* eff, int N, int last, hipStream_t s) {
  hipLaunchKernelGGL(sens_effect_kernel, dim3((unsigned)(((size_t)d * G + 255) / 256)), dim3(256), 0, s, part, rows, 1 + d * G, eff, N, last);
}
template <typename T>
void launch_sobol_reduce(const T* fbase, const T* fsub, int N, int d, double* out, hipStream_t s) {
  hipLaunchKernelGGL((sobol_reduce_kernel<T>), dim3(1), dim3(256), 0, s, fbase, fsub, N, d, out);
}
#define SENS_INST(T)                                                                                                                       \
  template void launch_sens_eval<T>(const T*, int, int, int, const T*, int, const T*, int, int, int, const EvalParams*, const T*, double*, \
                                    T*, T*, hipStream_t, hipEvent_t);                                                                      \
  template void launch_sens_scale_grid<T>(T*, int, int, const EvalParams*, hipStream_t);                                                   \
  template void launch_sobol_reduce<T>(const T*, const T*, int, int, double*, hipStream_t);
SENS_INST(double)
SENS_INST(float)
#undef SENS_INST

// =================================================================================================================
// joint posterior at the candidates (hbegp.cpp: model_posterior).  Sigma = K** + (1e-5 + jitter) I - Q Q^T comes from kmat_kernel
// and one tile GEMM; its factor from the recursion of the fit with the diagonal blocks below, which keep L; the draws
// Y = Z L^T from one more tile GEMM.  Two kernels of their own:
//   leaf_keep_kernel:       leaf_kernel's diagonal block, plus L_kk itself -> W3 (lower, explicit zeros above the diagonal:
//                           the tile GEMM reads W3 as a triangular operand).  leaf_kernel's own code is unchanged.
//   sample_epilogue_kernel: one workgroup per draw s: v_i = Y[s][i] + mean_i (stored in place when asked), and the index of
//                           the smallest v, ties to the lowest index -- every thread scans its entries in ascending i, then a
//                           fixed tree over the threads.  No atomics: the same inputs give the same bits.
// Both return at once when `info` is set (a failed pivot upstream): nothing spins, nothing reads a factor that failed.
// =================================================================================================================
template <typename T, typename TIO>
__global__ void __launch_bounds__(512, 2) leaf_keep_kernel(TIO* __restrict__ W1, TIO* __restrict__ W2, TIO* __restrict__ W3, int ld,
                                                        int blk, TIO* __restrict__ ldiag, int* info) {
  if (*info != 0) return;
  extern __shared__ __align__(16) char smem_raw[];
  leaf_body<T, TIO, false>(W1, W2, ld, blk, ldiag, info, 0, smem_raw);
  __syncthreads();
  // the lower triangle of the image holds L since the last panel's barrier (what follows it writes X^T above the diagonal)
  const T* As = reinterpret_cast<const T*>(smem_raw);
  TIO* Lblk = W3 + (size_t)blk * NB * ld + (size_t)blk * NB;
  for (int c = threadIdx.x; c < NB * NB; c += 512) {
    const int r = c >> 7, j = c & (NB - 1);
    Lblk[(size_t)r * ld + j] = j <= r ? (TIO)As[r * LeafGeom<T>::S + j] : TIO(0);
  }
}
template <typename T>
void launch_leaf_keep(T* W1, T* W2, T* W3, int ld, int blk, T* ldiag, int* info, hipStream_t s) {
  hipLaunchKernelGGL((leaf_keep_kernel<double, T>), dim3(1), dim3(512), LeafGeom<double>::LDS_BYTES, s, W1, W2, W3, ld, blk, ldiag, info);
}
template void launch_leaf_keep<double>(double*, double*, double*, int, int, double*, int*, hipStream_t);
template void launch_leaf_keep<float>(float*, float*, float*, int, int, float*, int*, hipStream_t);

template <typename T>
__global__ void __launch_bounds__(256) sample_epilogue_kernel(T* __restrict__ Y, int ld, const T* __restrict__ mean, int m, int store,
                                                              int* __restrict__ amin, const int* info) {
  if (*info != 0) return;
  __shared__ T sv[256];
  __shared__ int si[256];
  const int t = threadIdx.x;
  T* y = Y + (size_t)blockIdx.x * ld;
  T best = T(0);
  int bi = -1;
  for (int i = t; i < m; i += 256) {
    const T v = y[i] + mean[i];
    if (store) y[i] = v;
    if (bi < 0 || v < best) { best = v; bi = i; }  // ascending i: an equal value keeps the earlier index
  }
  sv[t] = best;
  si[t] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const T v = sv[t + w];
      const int i = si[t + w];
      if (i >= 0 && (si[t] < 0 || v < sv[t] || (v == sv[t] && i < si[t]))) { sv[t] = v; si[t] = i; }
    }
    __syncthreads();
  }
  if (t == 0) amin[blockIdx.x] = si[0];
}
template <typename T>
void launch_sample_epilogue(T* Y, int ld, const T* mean, int m, int S, int store, int* amin, const int* info, hipStream_t s) {
  hipLaunchKernelGGL((sample_epilogue_kernel<T>), dim3(S), dim3(256), 0, s, Y, ld, mean, m, store, amin, info);
}
template void launch_sample_epilogue<double>(double*, int, const double*, int, int, int, int*, const int*, hipStream_t);
template void launch_sample_epilogue<float>(float*, int, const float*, int, int, int, int*, const int*, hipStream_t);

// =================================================================================================================
// greedy batch selection by expected improvement (hbegp.cpp: model_select_batch).  The whole k-step loop in ONE
// workgroup: each pick depends on the last, and a grid would need a device-wide seam per pick.  Thread tid owns the rows
// i = tid (mod BSEL_THREADS).  Per step t:
//   EI of every row not yet picked (fp64, acquisition.rs:141-171), the LAST index of the maximum (Rust's max_by) through a
//   fixed LDS tree; then the fantasy f = mu_j (kriging believer) or the lie, and the conditioning on a noisy observation f at
//   row j: r_i = Sigma[j][i] - sum_{s<t} C[s][i] C[s][j] (ascending s), r_j = v_j - 1e-5 (the latent variance),
//   c = r / sqrt(max(r_j, 0) + s2) -> C[t], v -= c^2, mu += c (f - mu_j) / sqrt(max(r_j, 0) + s2).
// Sigma (symmetrised, ld x ld) is read in T, row j contiguously; C [k][ld], v, mu are fp64 global workspace, so every
// read of C is coalesced across the threads; C[s][j] of the first BSEL_CJ steps is staged in the LDS once per step.  Global
// values another thread wrote are read only behind a __syncthreads (workgroup-scope fence: one CU, one L1).  No atomics: the
// same inputs give the same bits, and the first t picks do not depend on k.
// =================================================================================================================
constexpr int BSEL_THREADS = 1024;
constexpr int BSEL_CJ = 4096;

// not inlined: erfc's fp64 coefficients, hoisted out of the row loop, would take more SGPRs than the kernel has (26 spilled)
__device__ __noinline__ double bsel_ei(double mu, double var, double fmin) {
  const double sd = sqrt(fmax(var, 0.0));
  if (sd <= 2.220446049250313e-16) return mu < fmin ? -(mu - fmin) : 0.0;  // ulps_eq!(std, 0.0): |std| <= f64::EPSILON
  const double z = -(mu - fmin) / sd;
  const double cdf = 0.5 * erfc(-z / 1.4142135623730951);
  const double pdf = exp(-0.5 * z * z) / 2.5066282746310002;
  return fmax(-(mu - fmin) * cdf + sd * pdf, 0.0);
}

template <typename T>
__global__ void __launch_bounds__(BSEL_THREADS) batch_select_kernel(const T* __restrict__ Sig, int ld, const T* __restrict__ mean, int m,
                                                                    int k, const EvalParams* __restrict__ P, double fmin0, int use_lie,
                                                                    double lie, double* __restrict__ C, double* __restrict__ v,
                                                                    double* __restrict__ mu, int* __restrict__ picked, int* __restrict__ idx,
                                                                    double* __restrict__ ei, T* __restrict__ mean_out, T* __restrict__ var_out) {
  __shared__ double sv[BSEL_THREADS];
  __shared__ int si[BSEL_THREADS];
  __shared__ double cj[BSEL_CJ];
  __shared__ double sh_vj, sh_muj;
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += BSEL_THREADS) {
    v[i] = (double)Sig[(size_t)i * ld + i];
    mu[i] = (double)mean[i];
    picked[i] = 0;
  }
  const double s2 = P->noise;
  double fm = fmin0;
  for (int t = 0; t < k; ++t) {
    // every row not yet picked is a candidate whatever its EI: with k <= m the index found is a valid row
    double best = 0.0;
    int bi = -1;
    for (int i = tid; i < m; i += BSEL_THREADS) {
      if (picked[i]) continue;
      const double e = bsel_ei(mu[i], v[i], fm);
      if (bi < 0 || e >= best) { best = e; bi = i; }  // ascending i: an equal value moves to the later index
    }
    sv[tid] = best;
    si[tid] = bi;
    __syncthreads();
#pragma unroll 1
    for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) {
        const double o = sv[tid + w];
        const int oi = si[tid + w];
        if (oi >= 0 && (si[tid] < 0 || o > sv[tid] || (o == sv[tid] && oi > si[tid]))) { sv[tid] = o; si[tid] = oi; }
      }
      __syncthreads();
    }
    const int j = si[0];
    if (tid == 0) {
      idx[t] = j;
      ei[t] = sv[0];
      sh_vj = v[j];
      sh_muj = mu[j];
    }
    const int tc = t < BSEL_CJ ? t : BSEL_CJ;
    for (int s = tid; s < tc; s += BSEL_THREADS) cj[s] = C[(size_t)s * ld + j];
    __syncthreads();
    const double vj = sh_vj, muj = sh_muj;
    const double f = use_lie ? lie : muj;
    const double rj = vj - 1e-5;
    const double sd = sqrt(fmax(rj, 0.0) + s2);
    for (int i = tid; i < m; i += BSEL_THREADS) {
      double r = rj;
      if (i != j) {
        r = (double)Sig[(size_t)j * ld + i];
        for (int s = 0; s < tc; ++s) r -= C[(size_t)s * ld + i] * cj[s];
        for (int s = tc; s < t; ++s) r -= C[(size_t)s * ld + i] * C[(size_t)s * ld + j];
      } else {
        picked[i] = 1;
      }
      const double c = r / sd;
      C[(size_t)t * ld + i] = c;
      v[i] -= c * c;
      mu[i] += c * (f - muj) / sd;
    }
    fm = fmin(fm, f);
    // the next step's EI reads only this thread's own rows; its tree writes sv / si, which nobody reads before the barrier
    // behind them, and cj, which every thread has finished reading when it reaches that step's first barrier
  }
  for (int i = tid; i < m; i += BSEL_THREADS) {
    mean_out[i] = (T)mu[i];
    var_out[i] = (T)fmax(v[i], 0.0);
  }
}
template <typename T>
void launch_batch_select(const T* Sig, int ld, const T* mean, int m, int k, const EvalParams* P, double fmin, int use_lie, double lie,
                         double* C, double* v, double* mu, int* picked, int* idx, double* ei, T* mean_out, T* var_out, hipStream_t s) {
  hipLaunchKernelGGL((batch_select_kernel<T>), dim3(1), dim3(BSEL_THREADS), 0, s, Sig, ld, mean, m, k, P, fmin, use_lie, lie, C, v, mu,
                     picked, idx, ei, mean_out, var_out);
}
template void launch_batch_select<double>(const double*, int, const double*, int, int, const EvalParams*, double, int, double, double*,
                                          double*, double*, int*, int*, double*, double*, double*, hipStream_t);
template void launch_batch_select<float>(const float*, int, const float*, int, int, const EvalParams*, double, int, double, double*,
                                         double*, double*, int*, int*, double*, float*, float*, hipStream_t);

// =================================================================================================================
// knowledge gradient over a candidate set (hbegp.cpp: model_knowledge_gradient).  One workgroup per candidate
// j < mc, all arithmetic in fp64 for both element types:
//   lines   row j of the symmetrised Sigma (read contiguously in T) and the mean: r_i = Sigma_ji, r_j = Sigma_jj - 1e-5,
//           sd = sqrt(max(r_j, 0) + s2); line i = (b_i, a_i) = (-(r_i / sd), -mu_i), padded with (+inf, +inf) to P, the power of two
//           at or above m
//   sort    bitonic network over the P lines by (b, a) ascending: KG_THREADS threads, one barrier per stage
//   scan    ONE lane walks the sorted lines (Frazier, Powell, Dayanik 2009, Algorithm 1): of a run of equal slopes only the last
//           (the largest a) is kept; a kept line pops the top of the stack while its breakpoint with the top,
//           c = (a_top - a) / (b - b_top), is <= the breakpoint at which the top begins.  The stack is written over the head of the
//           sorted array (its height never exceeds the lines consumed), and the breakpoints are not stored but recomputed from
//           adjacent stack lines -- the same quotient of the same operands, so the same bits -- which keeps a line at 16 bytes
//   sum     KG_j = sum_k (b_{k+1} - b_k) f(-|c_k|) over adjacent stack lines, f(z) = phi(z) + z Phi(z): thread t adds the terms
//           k = t (mod KG_THREADS) in ascending k, then a fixed LDS tree.  A single surviving line gives exactly 0.
// kg_kernel keeps the lines in dynamic LDS (16 P + 2064 bytes: 130 KiB at P = KG_LDS_ROWS = 8192); kg_global_kernel, for larger
// m, keeps them in a global workspace of P lines per workgroup and strides its workgroups over the candidates.  A line another
// thread wrote is read only behind a __syncthreads (workgroup-scope fence: one CU, one L1).  No atomics; KG_j depends on nothing
// but row j, the mean and s2, so it is the same for any mc and any grid.
// =================================================================================================================
constexpr int KG_THREADS = 256;
static_assert(kg_lds_bytes(0) == 8 * KG_THREADS + 16, "kg_lds_bytes counts KG_THREADS doubles for the sum's tree");

// not inlined: erfc's fp64 coefficients (as bsel_ei).  ac = |c| >= 0; beyond 38 both terms are below 1e-314 (and an infinite
// breakpoint would give inf * 0)
__device__ __noinline__ double kg_tail(double ac) {
  if (!(ac < 38.0)) return 0.0;
  const double cdf = 0.5 * erfc(ac / 1.4142135623730951);
  const double pdf = exp(-0.5 * ac * ac) / 2.5066282746310002;
  return fmax(pdf - ac * cdf, 0.0);
}

__device__ __forceinline__ bool kg_less(const double2 x, const double2 y) { return x.x < y.x || (x.x == y.x && x.y < y.y); }

// KG of candidate j by the whole workgroup (every thread returns it).  ln: P lines (LDS or global), red: KG_THREADS doubles and
// cnt: one int in the LDS.  The caller puts a barrier between two calls.
template <typename T>
__device__ __forceinline__ double kg_candidate(const T* __restrict__ Sig, int ld, const T* __restrict__ mean, int m, int P, double s2,
                                               int j, double2* ln, double* red, int* cnt) {
  const int tid = threadIdx.x;
  const T* __restrict__ row = Sig + (size_t)j * ld;
  const double rj = (double)row[j] - 1e-5;  // the latent variance: the sample's own noise is s2
  const double sd = sqrt(fmax(rj, 0.0) + s2);
  for (int i = tid; i < P; i += KG_THREADS) {
    double2 e = make_double2(INFINITY, INFINITY);
    if (i < m) {
      const double r = i == j ? rj : (double)row[i];
      e.x = -(r / sd);
      e.y = -(double)mean[i];
    }
    ln[i] = e;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll 1
    for (int w = k >> 1; w > 0; w >>= 1) {
      for (int p = tid; p < (P >> 1); p += KG_THREADS) {
        const int lo = ((p & ~(w - 1)) << 1) | (p & (w - 1));
        const int hi = lo | w;
        const double2 x = ln[lo], y = ln[hi];
        if ((lo & k) == 0 ? kg_less(y, x) : kg_less(x, y)) { ln[lo] = y; ln[hi] = x; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
#ifdef KG_NO_SCAN  // diagnostics (make variant DEFS=-DKG_NO_SCAN): the time of everything but the scan; kg comes out 0
    *cnt = 0;
  }
  if (tid == 0 && m < 0) {
#endif
    int t = 0;                // the stack is ln[0 .. t)
    double2 top = ln[0];      // its top, and the breakpoint at which the top begins
    double ctop = -INFINITY;
    double2 nx = top;
    for (int i = 0; i < m; ++i) {
      const double2 e = nx;
      if (i + 1 < m) {
        nx = ln[i + 1];
        if (nx.x == e.x) continue;  // equal slopes: sorted by a within the run, the last one dominates
      }
      double c = -INFINITY;
      while (t > 0) {
        c = (top.y - e.y) / (e.x - top.x);
        if (t == 1 || c > ctop) break;
        --t;
        top = ln[t - 1];
        if (t >= 2) {
          const double2 u = ln[t - 2];
          ctop = (u.y - top.y) / (top.x - u.x);
        }
      }
      ln[t++] = e;
      top = e;
      ctop = c;
    }
    *cnt = t;
  }
  __syncthreads();
  const int t = *cnt;
  double acc = 0.0;
  for (int k = tid; k + 1 < t; k += KG_THREADS) {
    const double2 x = ln[k], y = ln[k + 1];
    const double c = (x.y - y.y) / (y.x - x.x);
    acc += (y.x - x.x) * kg_tail(fabs(c));
  }
  red[tid] = acc;
  __syncthreads();
#pragma unroll 1
  for (int w = KG_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

template <typename T>
__global__ void __launch_bounds__(KG_THREADS) kg_kernel(const T* __restrict__ Sig, int ld, const T* __restrict__ mean, int m, int P,
                                                        const EvalParams* __restrict__ Pm, double* __restrict__ kg) {
  extern __shared__ __align__(16) char smem_raw[];
  double2* ln = reinterpret_cast<double2*>(smem_raw);
  double* red = reinterpret_cast<double*>(ln + P);
  int* cnt = reinterpret_cast<int*>(red + KG_THREADS);
  const double v = kg_candidate<T>(Sig, ld, mean, m, P, Pm->noise, blockIdx.x, ln, red, cnt);
  if (threadIdx.x == 0) kg[blockIdx.x] = v;
}

template <typename T>
__global__ void __launch_bounds__(KG_THREADS) kg_global_kernel(const T* __restrict__ Sig, int ld, const T* __restrict__ mean, int m,
                                                               int P, int mc, const EvalParams* __restrict__ Pm, double2* ws,
                                                               double* __restrict__ kg) {
  __shared__ double red[KG_THREADS];
  __shared__ int cnt;
  double2* ln = ws + (size_t)blockIdx.x * P;
  const double s2 = Pm->noise;
  for (int j = blockIdx.x; j < mc; j += gridDim.x) {
    const double v = kg_candidate<T>(Sig, ld, mean, m, P, s2, j, ln, red, &cnt);
    if (threadIdx.x == 0) kg[j] = v;
    __syncthreads();  // red and the lines are rewritten by the next candidate
  }
}

// best = the LAST index of the maximum of kg[0 .. mc) (Rust's max_by; -1 for mc = 0), imin = the lowest index of the minimum of
// the mean over all m rows, both through a fixed LDS tree; var_out = max(diag Sigma, 0)
template <typename T>
__global__ void __launch_bounds__(BSEL_THREADS) kg_epilogue_kernel(const T* __restrict__ Sig, int ld, const T* __restrict__ mean, int m,
                                                                   const double* __restrict__ kg, int mc, int* __restrict__ res,
                                                                   T* __restrict__ var_out) {
  __shared__ double sv[BSEL_THREADS];
  __shared__ int si[BSEL_THREADS];
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += BSEL_THREADS) var_out[i] = (T)fmax((double)Sig[(size_t)i * ld + i], 0.0);
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < mc; i += BSEL_THREADS) {
    const double e = kg[i];
    if (bi < 0 || e >= best) { best = e; bi = i; }  // ascending i: an equal value moves to the later index
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
#pragma unroll 1
  for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = sv[tid + w];
      const int oi = si[tid + w];
      if (oi >= 0 && (si[tid] < 0 || o > sv[tid] || (o == sv[tid] && oi > si[tid]))) { sv[tid] = o; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) res[0] = si[0];
  __syncthreads();
  best = 0.0;
  bi = -1;
  for (int i = tid; i < m; i += BSEL_THREADS) {
    const double e = (double)mean[i];
    if (bi < 0 || e < best) { best = e; bi = i; }  // ascending i: an equal value stays at the earlier index
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
#pragma unroll 1
  for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = sv[tid + w];
      const int oi = si[tid + w];
      if (oi >= 0 && (si[tid] < 0 || o < sv[tid] || (o == sv[tid] && oi < si[tid]))) { sv[tid] = o; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) res[1] = si[0];
}

int kg_padded_rows(int m) {
  int P = 1;
  while (P < m) P <<= 1;
  return P;
}
int kg_global_workgroups(int m, int mc) { return kg_padded_rows(m) <= KG_LDS_ROWS ? 0 : (mc < KG_GLOBAL_WGS ? mc : KG_GLOBAL_WGS); }

template <typename T>
void launch_knowledge_gradient(const T* Sig, int ld, const T* mean, int m, int mc, const EvalParams* P, void* ws, double* kg, int* res,
                               T* var_out, hipStream_t s) {
  const int Pr = kg_padded_rows(m);
  if (mc > 0) {
    if (Pr <= KG_LDS_ROWS)
      hipLaunchKernelGGL((kg_kernel<T>), dim3(mc), dim3(KG_THREADS), kg_lds_bytes(Pr), s, Sig, ld, mean, m, Pr, P, kg);
    else
      hipLaunchKernelGGL((kg_global_kernel<T>), dim3(kg_global_workgroups(m, mc)), dim3(KG_THREADS), 0, s, Sig, ld, mean, m, Pr, mc, P,
                         static_cast<double2*>(ws), kg);
  }
  hipLaunchKernelGGL((kg_epilogue_kernel<T>), dim3(1), dim3(BSEL_THREADS), 0, s, Sig, ld, mean, m, kg, mc, res, var_out);
}
template void launch_knowledge_gradient<double>(const double*, int, const double*, int, int, const EvalParams*, void*, double*, int*, double*,
                                                hipStream_t);
template void launch_knowledge_gradient<float>(const float*, int, const float*, int, int, const EvalParams*, void*, double*, int*, float*,
                                               hipStream_t);

// =================================================================================================================
// noisy expected improvement over a candidate set (hbegp.cpp: model_noisy_ei).  The tile products around these
// kernels leave Sigma's lower tiles in W1, L_b (the factor of the baseline block alone) with A = Sigma_cb L_b^-T below it in W3, and
// Y = Z [L_b; A]^T [S][ld].  The baseline takes rows 0 .. mb - 1, the candidates rows mbp .. mbp + mc - 1 (mbp = mb rounded up to NB).
//   nei_pad_kernel:      rows and columns mb .. mbp - 1 of Sigma (a copy of row 0 stands there) become identity padding, so that the
//                        baseline's 128-blocks factor as a matrix of their own; one workgroup per gap index
//   nei_fmin_kernel:     one workgroup per draw s: fmin_s = min_{i < mb} (mean_i + Y[s][i]) in fp64; every thread scans its entries in
//                        ascending i, then a fixed tree (a NaN never replaces a number, as in sample_epilogue_kernel)
//   nei_rho_kernel:      one wave per candidate j: rho_j = max(Sigma_jj - sum_{k < mb} A_jk^2, 0), lanes along k, fp64, a fixed
//                        shuffle tree
//   nei_kernel:          NEI_JL lanes along j (the reads of Y coalesce) times NEI_SG groups along s: group g adds
//                        EI(mean_j + Y[s][j], rho_j, fmin_s) for s = g, g + NEI_SG, .. in ascending s, then the groups' sums are added
//                        in ascending g and divided by S
//   nei_best_kernel:     the LAST index of the maximum of nei (Rust's max_by), a fixed LDS tree
// No atomics anywhere: the same inputs give the same bits.  All but the padding return at once when `info` is set.
// =================================================================================================================
constexpr int NEI_THREADS = 256;
constexpr int NEI_JL = 32;
constexpr int NEI_SG = NEI_THREADS / NEI_JL;

template <typename T>
__global__ void __launch_bounds__(NEI_THREADS) nei_pad_kernel(T* __restrict__ W, int ld, int mb, int mbp) {
  const int g = mb + blockIdx.x;
  for (int t = threadIdx.x; t < ld; t += NEI_THREADS) {
    if (t < mbp) W[(size_t)g * ld + t] = t == g ? T(1) : T(0);
    // column g in the lower tiles: the diagonal block's rows above the gap, and every row below the baseline (the gap's own rows
    // are written by their workgroups' row loops)
    if ((t >= mbp - NB && t < mb) || t >= mbp) W[(size_t)t * ld + g] = T(0);
  }
}

template <typename T>
__global__ void __launch_bounds__(NEI_THREADS) nei_fmin_kernel(const T* __restrict__ Y, int ld, const T* __restrict__ mean, int mb,
                                                               double* __restrict__ fmin_out, const int* info) {
  if (*info != 0) return;
  __shared__ double sv[NEI_THREADS];
  __shared__ int sh[NEI_THREADS];
  const int t = threadIdx.x;
  const T* y = Y + (size_t)blockIdx.x * ld;
  double best = 0.0;
  int have = 0;
  for (int i = t; i < mb; i += NEI_THREADS) {
    const double v = (double)y[i] + (double)mean[i];
    if (!have || v < best) { best = v; have = 1; }
  }
  sv[t] = best;
  sh[t] = have;
  __syncthreads();
  for (int w = NEI_THREADS / 2; w > 0; w >>= 1) {
    if (t < w && sh[t + w] && (!sh[t] || sv[t + w] < sv[t])) { sv[t] = sv[t + w]; sh[t] = 1; }
    __syncthreads();
  }
  if (t == 0) fmin_out[blockIdx.x] = sv[0];
}

template <typename T>
__global__ void __launch_bounds__(NEI_THREADS) nei_rho_kernel(const T* __restrict__ Sig, const T* __restrict__ A, int ld, int mb, int mbp,
                                                              int mc, double* __restrict__ rho, const int* info) {
  if (*info != 0) return;
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (NEI_THREADS / 64) + (threadIdx.x >> 6);
  if (j >= mc) return;  // whole waves leave: the shuffles below see full waves
  const T* a = A + (size_t)(mbp + j) * ld;
  double acc = 0.0;
  for (int k = lane; k < mb; k += 64) {
    const double v = (double)a[k];
    acc += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) rho[j] = fmax((double)Sig[(size_t)(mbp + j) * ld + mbp + j] - acc, 0.0);
}

template <typename T>
__global__ void __launch_bounds__(NEI_THREADS) nei_kernel(const T* __restrict__ Y, int ld, int mbp, const T* __restrict__ mean,
                                                          const double* __restrict__ rho, const double* __restrict__ fmin_draws, int mc,
                                                          int S, double* __restrict__ nei, const int* info) {
  if (*info != 0) return;
  __shared__ double part[NEI_SG][NEI_JL];
  const int l = threadIdx.x % NEI_JL, g = threadIdx.x / NEI_JL;
  const int j = blockIdx.x * NEI_JL + l;
  double acc = 0.0;
  if (j < mc) {
    const double mu = (double)mean[mbp + j], r = rho[j];
    const T* y = Y + mbp + j;
#pragma unroll 1
    for (int s = g; s < S; s += NEI_SG) acc += bsel_ei(mu + (double)y[(size_t)s * ld], r, fmin_draws[s]);
  }
  part[g][l] = acc;
  __syncthreads();
  if (g == 0 && j < mc) {
    double sum = 0.0;
    for (int q = 0; q < NEI_SG; ++q) sum += part[q][l];
    nei[j] = sum / (double)S;
  }
}

__global__ void __launch_bounds__(BSEL_THREADS) nei_best_kernel(const double* __restrict__ nei, int mc, int* __restrict__ best_out,
                                                                const int* info) {
  if (*info != 0) return;
  __shared__ double sv[BSEL_THREADS];
  __shared__ int si[BSEL_THREADS];
  const int tid = threadIdx.x;
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < mc; i += BSEL_THREADS) {
    const double e = nei[i];
    if (bi < 0 || e >= best) { best = e; bi = i; }  // ascending i: an equal value moves to the later index
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
#pragma unroll 1
  for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = sv[tid + w];
      const int oi = si[tid + w];
      if (oi >= 0 && (si[tid] < 0 || o > sv[tid] || (o == sv[tid] && oi > si[tid]))) { sv[tid] = o; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) *best_out = si[0];
}

template <typename T>
void launch_nei_pad(T* W, int ld, int mb, int mbp, hipStream_t s) {
  if (mbp > mb) hipLaunchKernelGGL((nei_pad_kernel<T>), dim3(mbp - mb), dim3(NEI_THREADS), 0, s, W, ld, mb, mbp);
}
template <typename T>
void launch_nei_reduce(const T* Sig, const T* LA, const T* Y, int ld, const T* mean, int mb, int mbp, int mc, int S, double* fmin_draws,
                       double* rho, double* nei, int* best, const int* info, hipStream_t s) {
  hipLaunchKernelGGL((nei_fmin_kernel<T>), dim3(S), dim3(NEI_THREADS), 0, s, Y, ld, mean, mb, fmin_draws, info);
  if (mc <= 0) return;
  constexpr int per = NEI_THREADS / 64;
  hipLaunchKernelGGL((nei_rho_kernel<T>), dim3((mc + per - 1) / per), dim3(NEI_THREADS), 0, s, Sig, LA, ld, mb, mbp, mc, rho, info);
  hipLaunchKernelGGL((nei_kernel<T>), dim3((mc + NEI_JL - 1) / NEI_JL), dim3(NEI_THREADS), 0, s, Y, ld, mbp, mean, rho, fmin_draws, mc, S,
                     nei, info);
  hipLaunchKernelGGL(nei_best_kernel, dim3(1), dim3(BSEL_THREADS), 0, s, nei, mc, best, info);
}
template void launch_nei_pad<double>(double*, int, int, int, hipStream_t);
template void launch_nei_pad<float>(float*, int, int, int, hipStream_t);
template void launch_nei_reduce<double>(const double*, const double*, const double*, int, const double*, int, int, int, int, double*, double*,
                                        double*, int*, const int*, hipStream_t);
template void launch_nei_reduce<float>(const float*, const float*, const float*, int, const float*, int, int, int, int, double*, double*,
                                       double*, int*, const int*, hipStream_t);

// =================================================================================================================
// batch expected improvement by Monte Carlo (hbegp.cpp: model_qei).  One workgroup per batch b of q points
// (rows b q .. b q + q - 1 of the batched predict's Q [mp][np], mean, dmean [mp][d] and W [d][mp][np]):
//   Sigma = K** + noise I - Q_b Q_b^T   (fp64: K** from the points, q (q+1) / 2 wave dots over np, ascending lane stride)
//   L = chol(Sigma) in the LDS, right-looking, one column per step; a pivot that is not > 0 fails the batch (info = 1 + column)
//   per draw s (one wave, lane a = row a): f_a = sum_{c <= a} L_ac z_sc + mu_a; j_s = argmin (ties to the lowest index, a
//   fixed xor tree); I_s = max(0, fmin - f_j).  Draws go in chunks of QEI_CH: the waves store j_s (-1: I_s = 0) and I_s in the
//   LDS, then thread c adds z_sc to Lbar[j_s][c] and counts j_s = c, and thread 64 adds I_s, all in ascending s: no atomics.
//   reverse (want_grad): Lbar *= -1/S, mubar = -count/S; M = L^T Lbar (thread j owns column j, in place in ascending rows),
//   Phi(M) (lower, halved diagonal), P = L^-T Phi (column j, in place), X = P L^-1 (row i, in place), Sigmabar = (X + X^T) / 2;
//   grad[a][k] = mubar_a dmean[a][k] + 2 sum_c Sigmabar_ac (dk(x_a, x_c)/dx_a,k - w_ak . q_c), evaluated as
//   2 (sum_c Sigmabar_ac dk_ac,k - w_ak . v_a) with v_a = sum_c Sigmabar_ac q_c: one wave per (a, eight k), v_a formed per lane
//   element in ascending c and dotted with the eight W rows (Q is read d/8 times per point instead of q d times).  psi's
//   convention at r = 0 makes the c = a term -w_aa . q_a.
// Everything is fp64 for both element types; the same inputs give the same bits, and a batch reads nothing of another batch.
// LDS (doubles): scaled points q d, Sigma -> L q^2, Lbar -> X q^2, mu / mubar 2 q, I_s QEI_CH; ints: j_s QEI_CH, the failure flag.
// =================================================================================================================
constexpr int QEI_THREADS = 256;
static_assert(qei_lds_bytes(QEI_MAXQ, MAXD) <= 160 * 1024, "qei_batch_kernel: the largest batch must fit the LDS of one CU");

// not inlined (as bsel_ei): the Matern constants hoisted into the kernel body spilled SGPRs.  r^2 of the scaled points a and c;
// k(x_a, x_c) + noise [a == c] (kmat_entry in fp64), or c psi(r) (s_a,k - s_c,k) / ell_k (0 at r = 0).
__device__ __noinline__ double qei_r2(const double* sx, int a, int c, int d) {
  double r2 = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = sx[a * d + k] - sx[c * d + k];
    r2 += df * df;
  }
  return r2;
}
__device__ __noinline__ double qei_kss(double r2, int nu2, double amp, double noise, bool diag) {
  return kmat_entry<double>(r2, nu2, amp, noise, diag);
}
__device__ __noinline__ double qei_dk(double r2, int nu2, double amp, double df, double ell) {
  return r2 == 0.0 ? 0.0 : amp * matern_psi(r2, nu2) * df / ell;
}

template <typename T>
__global__ void __launch_bounds__(QEI_THREADS) qei_batch_kernel(const T* __restrict__ Xs, int q, int d, const T* __restrict__ Q,
                                                                const T* __restrict__ W, int mp, int np, const T* __restrict__ mean,
                                                                const T* __restrict__ dmean, const EvalParams* __restrict__ P,
                                                                double noise, int nu2, const T* __restrict__ z, int S, double fmin,
                                                                int want_grad, double* __restrict__ qei, T* __restrict__ grad,
                                                                int* __restrict__ info) {
  extern __shared__ __align__(16) char smem_raw[];
  double* sx = reinterpret_cast<double*>(smem_raw);  // [q][d] points / ell
  double* A = sx + (size_t)q * d;                    // [q][q] Sigma, then L (lower)
  double* Lb = A + (size_t)q * q;                    // [q][q] Lbar, then M, Phi, P, X
  double* mu = Lb + (size_t)q * q;                   // [q]
  double* mub = mu + q;                              // [q]
  double* Iv = mub + q;                              // [QEI_CH]
  int* jv = reinterpret_cast<int*>(Iv + QEI_CH);     // [QEI_CH]
  int* fail = jv + QEI_CH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, r0 = b * q;
  const double amp = P->amp;
  for (int e = tid; e < q * d; e += QEI_THREADS) sx[e] = (double)Xs[(size_t)r0 * d + e] / P->ell[e % d];
  for (int e = tid; e < q * q; e += QEI_THREADS) Lb[e] = 0.0;
  for (int a = tid; a < q; a += QEI_THREADS) mu[a] = (double)mean[r0 + a];
  if (tid == 0) *fail = 0;
  __syncthreads();
  // Sigma (lower): pair p = (a, c), c <= a, in row order, dealt to the waves round robin
  {
    int p = 0;
    for (int a = 0; a < q; ++a) {
      for (int c = 0; c <= a; ++c, ++p) {
        if ((p & 3) != wave) continue;
        const T* qa = Q + (size_t)(r0 + a) * np;
        const T* qc = Q + (size_t)(r0 + c) * np;
        double acc = 0.0;
        for (int j = lane; j < np; j += 64) acc += (double)qa[j] * (double)qc[j];
        acc = wave_sum(acc);
        if (lane == 0) A[a * q + c] = qei_kss(qei_r2(sx, a, c, d), nu2, amp, noise, a == c) - acc;
      }
    }
  }
  // Cholesky, right-looking
  for (int j = 0; j < q; ++j) {
    __syncthreads();
    if (tid == 0) {
      const double pv = A[j * q + j];
      if (pv > 0.0) A[j * q + j] = sqrt(pv);
      else *fail = j + 1;
    }
    __syncthreads();
    if (*fail) break;
    const double ljj = A[j * q + j];
    for (int i = j + 1 + tid; i < q; i += QEI_THREADS) A[i * q + j] /= ljj;
    __syncthreads();
    const int w = q - j - 1;
    for (int e = tid; e < w * w; e += QEI_THREADS) {
      const int i = j + 1 + e / w, k = j + 1 + e % w;
      if (k <= i) A[i * q + k] -= A[i * q + j] * A[k * q + j];
    }
  }
  if (*fail) {
    if (want_grad)
      for (int e = tid; e < q * d; e += QEI_THREADS) grad[(size_t)r0 * d + e] = T(0);
    if (tid == 0) {
      qei[b] = __longlong_as_double(0x7ff8000000000000LL);
      info[b] = *fail;
    }
    return;
  }
  // draws
  double isum = 0.0;
  int cnt = 0;
  for (int s0 = 0; s0 < S; s0 += QEI_CH) {
    const int s1 = min(S, s0 + QEI_CH);
    for (int s = s0 + wave; s < s1; s += QEI_THREADS / 64) {
      const double zl = lane < q ? (double)z[(size_t)s * q + lane] : 0.0;
      double f = 0.0;
      for (int c = 0; c < q; ++c) {
        const double zc = __shfl(zl, c, 64);
        if (c <= lane && lane < q) f += A[lane * q + c] * zc;
      }
      double v = lane < q ? f + mu[lane] : __longlong_as_double(0x7ff0000000000000LL);
      int ix = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(ix, off, 64);
        if (ov < v || (ov == v && oi < ix)) { v = ov; ix = oi; }
      }
      if (lane == 0) {
        const double imp = fmin - v;
        Iv[s - s0] = imp > 0.0 ? imp : 0.0;
        jv[s - s0] = imp > 0.0 ? ix : -1;
      }
    }
    __syncthreads();
    if (tid < q && want_grad) {
      for (int s = s0; s < s1; ++s) {
        const int j = jv[s - s0];
        if (j < 0) continue;
        if (tid <= j) Lb[j * q + tid] += (double)z[(size_t)s * q + tid];
        if (j == tid) ++cnt;
      }
    }
    if (tid == 64)
      for (int s = s0; s < s1; ++s) isum += Iv[s - s0];
    __syncthreads();
  }
  if (tid == 64) {
    qei[b] = isum / (double)S;
    info[b] = 0;
  }
  if (!want_grad) return;
  // reverse through the factor
  if (tid < q) {
    for (int a = tid; a < q; ++a) Lb[a * q + tid] = -Lb[a * q + tid] / (double)S;
    mub[tid] = -(double)cnt / (double)S;
  }
  __syncthreads();
  if (tid < q) {  // M = L^T Lbar, column j = tid, rows ascending (row i reads rows k >= i only); Phi: lower, halved diagonal
    const int j = tid;
    for (int i = 0; i < q; ++i) {
      if (i < j) { Lb[i * q + j] = 0.0; continue; }
      double m = 0.0;
      for (int k = i; k < q; ++k) m += A[k * q + i] * Lb[k * q + j];
      Lb[i * q + j] = i == j ? 0.5 * m : m;
    }
  }
  __syncthreads();
  if (tid < q) {  // P = L^-T Phi, column j = tid, rows descending
    const int j = tid;
    for (int i = q - 1; i >= 0; --i) {
      double p = Lb[i * q + j];
      for (int k = i + 1; k < q; ++k) p -= A[k * q + i] * Lb[k * q + j];
      Lb[i * q + j] = p / A[i * q + i];
    }
  }
  __syncthreads();
  if (tid < q) {  // X = P L^-1, row i = tid, columns descending
    const int i = tid;
    for (int j = q - 1; j >= 0; --j) {
      double x = Lb[i * q + j];
      for (int k = j + 1; k < q; ++k) x -= Lb[i * q + k] * A[k * q + j];
      Lb[i * q + j] = x / A[j * q + j];
    }
  }
  __syncthreads();
  if (tid < q) {  // Sigmabar = (X + X^T) / 2 in place, row i = tid against the rows below it
    const int i = tid;
    for (int j = i + 1; j < q; ++j) {
      const double v = 0.5 * (Lb[i * q + j] + Lb[j * q + i]);
      Lb[i * q + j] = v;
      Lb[j * q + i] = v;
    }
  }
  __syncthreads();
  // gradient: one wave per (a, eight features k0 .. k0 + 7)
  const int nkc = (d + 7) / 8;
  for (int item = wave; item < q * nkc; item += QEI_THREADS / 64) {
    const int a = item / nkc, k0 = (item - a * nkc) * 8;
    const double* sb = Lb + a * q;  // row a of Sigmabar
    double acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0;
    for (int j = lane; j < np; j += 64) {
      double v = 0.0;  // v_a[j] = sum_c Sigmabar_ac q_c[j]
      for (int c = 0; c < q; ++c) v += sb[c] * (double)Q[(size_t)(r0 + c) * np + j];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < d) acc[u] += (double)W[((size_t)(k0 + u) * mp + r0 + a) * np + j] * v;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = wave_sum(acc[u]);
    if (lane == 0) {
      for (int u = 0; u < 8 && k0 + u < d; ++u) {
        const int k = k0 + u;
        const double ell = P->ell[k];
        double dks = 0.0;
        for (int c = 0; c < q; ++c) dks += sb[c] * qei_dk(qei_r2(sx, a, c, d), nu2, amp, sx[a * d + k] - sx[c * d + k], ell);
        grad[(size_t)(r0 + a) * d + k] = (T)(mub[a] * (double)dmean[(size_t)(r0 + a) * d + k] + 2.0 * (dks - acc[u]));
      }
    }
  }
}
template <typename T>
void launch_qei_batch(const T* Xs, int B, int q, int d, const T* Q, const T* W, int mp, int np, const T* mean, const T* dmean,
                      const EvalParams* P, double noise, int nu2, const T* z, int S, double fmin, int want_grad, double* qei, T* grad,
                      int* info, hipStream_t s) {
  hipLaunchKernelGGL((qei_batch_kernel<T>), dim3(B), dim3(QEI_THREADS), qei_lds_bytes(q, d), s, Xs, q, d, Q, W, mp, np, mean, dmean, P,
                     noise, nu2, z, S, fmin, want_grad, qei, grad, info);
}
template void launch_qei_batch<double>(const double*, int, int, int, const double*, const double*, int, int, const double*, const double*,
                                       const EvalParams*, double, int, const double*, int, double, int, double*, double*, int*, hipStream_t);
template void launch_qei_batch<float>(const float*, int, int, int, const float*, const float*, int, int, const float*, const float*,
                                      const EvalParams*, double, int, const float*, int, double, int, double*, float*, int*, hipStream_t);

// =================================================================================================================
// predict for a handful of candidates (m <= PRED_SMALL_MAX): the caller's acquisition and selection loops issue
// thousands of single-point predicts per generation (acquisition.rs:46-64, minimize.rs:656-714).  The batched path pads
// to 128 candidate rows and runs a tile GEMM over all of L^-1 (0.2 ms at n=4096 whatever m is); here L^-1 is read once,
// row by row, against the m cross-kernel vectors:
//   kstar_small:  Ks[q][j] = c * Matern(x*_q, x_j)  (same arithmetic as kstar_kernel), partial sums of Ks[q][j] alpha_j
//   rowdot_small: w[i][q] = sum_{j<=i} Linv[i][j] Ks[q][j]          one wave per row, fp64 accumulation
//   finish_small: mean_q = sum partials; var_q = c + 1e-5 - sum_i w[i][q]^2, clamp, warning count   (predict.rs:18-48)
// All sums run in a fixed order: results are bitwise reproducible.
// =================================================================================================================
template <typename T>
__global__ void __launch_bounds__(256) kstar_small_kernel(const T* __restrict__ Xs, int m, const T* __restrict__ X, int n, int d, int np,
                                                          int nu2, const EvalParams* __restrict__ P, const T* __restrict__ alpha,
                                                          T* __restrict__ Ks, double* __restrict__ pmean) {
  __shared__ double red[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  const T amp = (T)P->amp;
  for (int q = 0; q < m; ++q) {
    T v = T(0);
    if (j < n) {
      T acc = T(0);
      for (int k = 0; k < d; ++k) {  // cdist accumulation order (matern_kernel.rs:274-278), operands scaled as matern_kernel.rs:50-60
        const T ell = (T)P->ell[k];
        const T df = Xs[(size_t)q * d + k] / ell - X[(size_t)j * d + k] / ell;
        acc += df * df;
      }
      v = kmat_entry<T>(acc, nu2, amp, T(0), false);
    }
    if (j < np) Ks[(size_t)q * np + j] = v;
    const double part = block_sum((j < n) ? (double)v * (double)alpha[j] : 0.0, red);
    if (threadIdx.x == 0) pmean[(size_t)blockIdx.x * PRED_SMALL_MAX + q] = part;
  }
}

template <typename T, int MQ>
__global__ void __launch_bounds__(256) rowdot_small_kernel(const T* __restrict__ Linv, int np, int n, const T* __restrict__ Ks,
                                                           double* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int row = n - 1 - (blockIdx.x * 4 + (threadIdx.x >> 6));  // longest rows first
  if (row < 0) return;
  double acc[MQ];
#pragma unroll
  for (int q = 0; q < MQ; ++q) acc[q] = 0.0;
  const T* xr = Linv + (size_t)row * np;
  for (int k = lane; k <= row; k += 64) {
    const double x = (double)xr[k];
#pragma unroll
    for (int q = 0; q < MQ; ++q) acc[q] += x * (double)Ks[(size_t)q * np + k];
  }
#pragma unroll
  for (int q = 0; q < MQ; ++q) {
    const double s = wave_sum(acc[q]);
    if (lane == 0) w[(size_t)row * PRED_SMALL_MAX + q] = s;
  }
}

// one workgroup finishes all candidates: every thread sums a strided share of the rows, fixed-order block reduction
template <typename T>
__global__ void __launch_bounds__(256) finish_small_kernel(const double* __restrict__ pmean, int nblk, const double* __restrict__ w, int n,
                                                           int m, const EvalParams* __restrict__ P, int want_var, T* __restrict__ mean,
                                                           T* __restrict__ var, int* __restrict__ n_warn) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int q = 0; q < m; ++q) {
    double mu = 0.0;
    for (int b = t; b < nblk; b += 256) mu += pmean[(size_t)b * PRED_SMALL_MAX + q];
    const double mu_all = block_sum(mu, red);
    double ss = 0.0;
    if (want_var)
      for (int i = t; i < n; i += 256) {
        const double v = w[(size_t)i * PRED_SMALL_MAX + q];
        ss += v * v;
      }
    const double ss_all = want_var ? block_sum(ss, red) : 0.0;
    if (t == 0) {
      mean[q] = (T)mu_all;
      if (want_var) {
        const T min_noise = (T)1e-5;
        T v = (T)P->amp + min_noise - (T)ss_all;  // predict.rs:25-37
        if (v < -sqrt(min_noise)) atomicAdd(n_warn, 1);
        if (v < T(0)) v = T(0);
        var[q] = v;
      }
    }
  }
}

template <typename T>
void launch_predict_small(const T* Xs, int m, const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* alpha, const T* Linv,
                          T* Ks, double* pmean, double* w, int want_var, T* mean, T* var, int* n_warn, hipStream_t s) {
  const int nblk = (np + 255) / 256;
  hipLaunchKernelGGL((kstar_small_kernel<T>), dim3(nblk), dim3(256), 0, s, Xs, m, X, n, d, np, nu2, P, alpha, Ks, pmean);
  if (want_var) {
    const dim3 grid((n + 3) / 4), block(256);
    if (m <= 1) hipLaunchKernelGGL((rowdot_small_kernel<T, 1>), grid, block, 0, s, Linv, np, n, Ks, w);
    else if (m <= 2) hipLaunchKernelGGL((rowdot_small_kernel<T, 2>), grid, block, 0, s, Linv, np, n, Ks, w);
    else if (m <= 4) hipLaunchKernelGGL((rowdot_small_kernel<T, 4>), grid, block, 0, s, Linv, np, n, Ks, w);
    else if (m <= 8) hipLaunchKernelGGL((rowdot_small_kernel<T, 8>), grid, block, 0, s, Linv, np, n, Ks, w);
    else hipLaunchKernelGGL((rowdot_small_kernel<T, 16>), grid, block, 0, s, Linv, np, n, Ks, w);
  }
  hipLaunchKernelGGL((finish_small_kernel<T>), dim3(1), dim3(256), 0, s, pmean, nblk, w, n, m, P, want_var, mean, var, n_warn);
}
template void launch_predict_small<double>(const double*, int, const double*, int, int, int, int, const EvalParams*, const double*, const double*,
                                           double*, double*, double*, int, double*, double*, int*, hipStream_t);
template void launch_predict_small<float>(const float*, int, const float*, int, int, int, int, const EvalParams*, const float*, const float*,
                                          float*, double*, double*, int, float*, float*, int*, hipStream_t);

// =================================================================================================================
// One evaluation in ONE launch for problems of at most 128 rows (np = 128, d <= 32): the reference's own regime
// (minimize.rs:118-120 keeps n at 100-200).  The five launches of the general path (kmat, diagonal block, trmv x2 + reductions,
// K^-1 = X^T X, gradient) cost ~2 us of launch gap and one HBM round trip each -- more than their arithmetic at this size.
// Here one workgroup keeps everything in the LDS:
//   K = c Matern + s2 I      into the block image (the arithmetic of kmat_kernel, entry for entry, the rows' rv on the diagonal
//                            included; K never goes to HBM)
//   L, X = L^-1              leaf_body on that image (X and diag(L) also go to HBM: the model keeps them)
//   alpha = X^T (X y), lml   fp64 dot products against the image (X lives transposed in its strict upper blocks)
//   K^-1 = X^T X             120 16x16x16 products on MFMA, into the lower blocks of the image (L is no longer needed) and to HBM
//   g_j = 1/2 sum (alpha alpha^T - K^-1) o dK_j    the arithmetic of gradtrace_kernel, K^-1 and alpha read from the LDS
// =================================================================================================================
// rv_raw (may be null): the rows' known noise variances.  They travel beside the descriptor, not inside it: a run of
// small_fit_kernel copies the descriptor to its stack for every evaluation, and eight more bytes there cost the fit without
// variances 0.5 % of its rate at n = 128 (profiles/rv_bench.txt).
template <typename TIO, int NU2>
__device__ __forceinline__ void small_eval_body(const SmallEval& g, const void* rv_raw, char* smem_raw) {
  using T = double;
  using C = Cfg<T>;
  using L = LeafGeom<T>;
  using acc_t = typename C::acc_t;
  constexpr int S = L::S, YS = L::YS, YB = L::YB;
  T* As = reinterpret_cast<T*>(smem_raw);
  T* Yt = As + 128 * S;
  T* Sc = Yt + 16 * S;       // the diagonal block's scratch region (pivot-block copy, identity, flags, item tables): 1280 doubles,
                             // and 480 more to the end of the CU's LDS.  Outside leaf_body it is this kernel's scratch:
  T* yv = Sc;                //   [128] y
  T* wv = Sc + 128;          //   [128] w = X y
  T* av = Sc + 256;          //   [128] alpha (rounded to the element type, as the general path stores it)
  T* red = Sc + 384;         //   [8 x 35] per-wave partial sums
  T* ellv = Sc + 664;        //   [32] length scales, then [32] their inverse squares (in the element type's arithmetic)
  T* feat = Sc + 728;        //   [8][128] a chunk of eight features of all rows, [feature][row]; 8 doubles to the end of the CU's LDS stay free
                             //   (small_fit_kernel keeps two flags there)
  static_assert(728 + 8 * 128 + 8 <= (163840 - (128 * S + 16 * S) * 8) / 8, "the scratch of small_eval_kernel fits behind the block image");
  int* pool = reinterpret_cast<int*>(Sc + YB + 17 * YS + 2);  // leaf_body's flags (pool[15]: not positive definite)
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int m16 = lane & 15, q4 = lane >> 4;
  const int n = g.n, d = g.d;
  const TIO* X = static_cast<const TIO*>(g.X);
  const EvalParams* P = g.P;
  // the parameters are read with agent-scope loads: inside small_fit_kernel they change between two evaluations of ONE launch,
  // and a scalar load (what a uniform address compiles to) goes through the scalar cache, which no vector store updates
  auto pld = [](const double* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const TIO amp = (TIO)pld(&P->amp), noise = (TIO)pld(&P->noise);
  if (t == 0) g_leaf_stamps[200] = (long long)__builtin_readcyclecounter();
  // start of an evaluation (what launch_reset_out does for the general path): the outputs are poisoned, the flags cleared
  EvalOut* out = g.hout;
  {
    const double poison = __longlong_as_double(0x7ff8000000005eedLL);
    if (t < MAXP) out->grad[t] = poison;
    if (t == 0) {
      out->lml = poison; out->yalpha = poison; out->logdet = poison;
      out->info = 0; out->n_warn = 0; out->done = 0;
      g.out->info = 0;
    }
  }
  // thread (tx, ty, half) owns, in each of the three lower 64x64 tiles (0,0), (1,0), (1,1): rows ty + 16 (2 half + r), r = 0, 1,
  // columns 4 tx .. 4 tx + 3 -- per entry the sums of kmat_kernel / gradtrace_kernel in their order
  const int tx = t & 15, ty = (t >> 4) & 15, half = t >> 8;
  auto tile_i0 = [](int tile) { return tile == 0 ? 0 : 64; };
  auto tile_j0 = [](int tile) { return tile == 2 ? 64 : 0; };
  // eight features of all 128 rows -> feat[u][row]; scaled: divided by the length scale (kmat), else raw (gradient)
  auto stage_features = [&](int kc, bool scaled) {
    for (int e = t; e < 8 * 128; e += 512) {
      const int row = e >> 3, u = e & 7, k = kc + u;
      TIO v = TIO(0);
      if (row < n && k < d) {
        v = X[(size_t)row * d + k];
        if (scaled) v = v / (TIO)ellv[k];  // matern_kernel.rs:51-60
      }
      feat[u * 128 + row] = (T)v;
    }
  };
  if (t < 32) {
    const TIO ell = t < d ? (TIO)pld(&P->ell[t]) : TIO(1);  // A::from_f (matern_kernel.rs:50)
    ellv[t] = (T)ell;
    ellv[32 + t] = (T)(TIO(1) / (ell * ell));          // 1/scales_k_square (matern_kernel.rs:94-98)
  }
  __syncthreads();

  // ---- K into the image (never to HBM): squared scaled distances accumulated feature by feature, eight features per staging
  {
    TIO acc[3][2][4];
#pragma unroll
    for (int tile = 0; tile < 3; ++tile)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[tile][r][c] = TIO(0);
    for (int kc = 0; kc < d; kc += 8) {
      stage_features(kc, true);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (kc + u < d) {  // uniform; cdist accumulation order (matern_kernel.rs:274-278)
#pragma unroll
          for (int tile = 0; tile < 3; ++tile) {
            TIO a[2], b[4];
#pragma unroll
            for (int r = 0; r < 2; ++r) a[r] = (TIO)feat[u * 128 + tile_i0(tile) + ty + 16 * (2 * half + r)];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = (TIO)feat[u * 128 + tile_j0(tile) + tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const TIO df = a[r] - b[c];
                acc[tile][r][c] += df * df;
              }
          }
        }
      }
      __syncthreads();
    }
    // zeros everywhere first (the strict upper 16x16 blocks must start as zeros), then the three tiles' entries
    for (int e = t; e < 128 * (S / 2); e += 512) reinterpret_cast<d2*>(As)[e] = d2{0, 0};
    __syncthreads();
#pragma unroll
    for (int tile = 0; tile < 3; ++tile)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int gi = tile_i0(tile) + ty + 16 * (2 * half + r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int gj = tile_j0(tile) + tx * 4 + c;
          if ((gj >> 4) <= (gi >> 4)) {  // lower 16x16 blocks only
            const TIO v = kmat_entry<TIO>(acc[tile][r][c], NU2, amp, noise, gi == gj);
            As[gi * S + gj] = (T)((gi < n && gj < n) ? v : ((gi == gj) ? TIO(1) : TIO(0)));  // identity padding
          }
        }
      }
    if (rv_raw != nullptr) {
      const TIO* rv = static_cast<const TIO*>(rv_raw);  // the rows' known noise variances: constant over a fit's evaluations
      // kmat_kernel's rule: (c k(0) + s2) + v_i, added by the thread that wrote the entry -- in the diagonal tiles (0 and 2) the one
      // whose four columns hold the row's own column (tx = (row within the tile) >> 2).  Rows >= n keep the padding's one.
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int li = ty + 16 * (2 * half + r);
        if ((li >> 2) == tx) {
#pragma unroll
          for (int tile = 0; tile < 3; tile += 2) {
            const int gi = tile_i0(tile) + li;
            if (gi < n) As[gi * S + gi] = (T)kmat_add_rv<TIO>((TIO)As[gi * S + gi], rv[gi]);
          }
        }
      }
    }
    __syncthreads();
  }
  if (t == 0) g_leaf_stamps[201] = (long long)__builtin_readcyclecounter();

  // ---- L and X = L^-1
  TIO* W2 = static_cast<TIO*>(g.W2);
  leaf_body<T, TIO, false, true>(nullptr, W2, 128, 0, static_cast<TIO*>(g.ldiag), &g.out->info, 0, smem_raw);
  __syncthreads();
  if (t == 0) g_leaf_stamps[202] = (long long)__builtin_readcyclecounter();
  if (pool[15] != 0) {  // not positive definite: the outputs stay poisoned (lml.rs:47-50)
    if (t == 0) out->info = g.out->info;
    return;
  }
  if (!(g.mode & 1)) return;
  __syncthreads();  // every thread has read the flag: the scratch may be reused

  // X[i][k] (i >= k) in the image: block (I, K), I > K, lives transposed in block (K, I); the diagonal blocks in Yt (transposed)
  auto xel = [&](int i, int k) -> T {
    const int I = i >> 4, K = k >> 4;
    return I > K ? As[(K * 16 + (k & 15)) * S + I * 16 + (i & 15)] : Yt[(k & 15) * S + 16 * I + (i & 15)];
  };
  if (t < 128) yv[t] = t < n ? (T)static_cast<const TIO*>(g.y)[t] : T(0);
  if (t >= 128 && t < 160) {  // the length scales again (leaf_body's scratch went over them)
    const int k = t - 128;
    const TIO ell = k < d ? (TIO)pld(&P->ell[k]) : TIO(1);
    ellv[k] = (T)ell;
    ellv[32 + k] = (T)(TIO(1) / (ell * ell));
  }
  __syncthreads();
  {
    // w_i = sum_{k <= i} X[i][k] y[k]: four threads per row, fp64, four independent partial sums per thread
    const int i = t >> 2, sub = t & 3;
    T acc[4] = {0, 0, 0, 0};
    int k = sub;
    for (; k + 12 <= i; k += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_fma(xel(i, k + 4 * u), yv[k + 4 * u], acc[u]);
    }
    for (; k <= i; k += 4) acc[0] = __builtin_fma(xel(i, k), yv[k], acc[0]);
    T a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (sub == 0) wv[i] = (T)(TIO)a;  // the general path keeps w in the element type
  }
  __syncthreads();
  {
    // alpha_j = sum_{i >= j} X[i][j] w_i
    const int j = t >> 2, sub = t & 3;
    T acc[4] = {0, 0, 0, 0};
    int i = j + sub;
    for (; i + 12 < 128; i += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_fma(xel(i + 4 * u, j), wv[i + 4 * u], acc[u]);
    }
    for (; i < 128; i += 4) acc[0] = __builtin_fma(xel(i, j), wv[i], acc[0]);
    T a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (sub == 0) {
      const TIO at = j < n ? (TIO)a : TIO(0);
      static_cast<TIO*>(g.alpha)[j] = at;
      av[j] = (T)at;
    }
  }
  __syncthreads();
  {
    // lml = -1/2 y^T alpha - sum log L_ii - n/2 log 2 pi (lml.rs:57-59)
    T ya = 0, ld = 0;
    if (t < n) {
      ya = yv[t] * av[t];
      ld = log((T)(TIO)As[t * S + t]);
    }
    ya = wave_sum(ya);
    ld = wave_sum(ld);
    if (lane == 0) { red[wave * 2] = ya; red[wave * 2 + 1] = ld; }
    __syncthreads();
    if (t == 0) {
      T s1 = 0, s2 = 0;
      for (int w = 0; w < 8; ++w) { s1 += red[2 * w]; s2 += red[2 * w + 1]; }
      out->yalpha = s1;
      out->logdet = s2;
      out->lml = __builtin_fma(-0.5, s1, -s2) - (double)n / 2.0 * log(2.0 * 3.14159265358979323846);
      out->done = 1;  // one writer
    }
  }
  if (t == 0) g_leaf_stamps[203] = (long long)__builtin_readcyclecounter();
  if (!(g.mode & 2)) return;

  // ---- K^-1 = X^T X, lower blocks (I, J): sum_{K >= I} X[K,I]^T X[K,J].  Both operands are rows of the image in the layout an
  // MFMA fragment wants (X[K,I]^T = block (I,K) of the image, or Yt_I for K = I).  36 blocks, 120 products, dealt to the 8 waves.
  {
    const int P0 = (m16 * S + q4) * (int)sizeof(T), P1 = (q4 * S + m16) * (int)sizeof(T);
    char* lds0 = reinterpret_cast<char*>(As);
    auto ldsT = [&](int byte_off) -> T& { return *reinterpret_cast<T*>(lds0 + byte_off); };
    TIO* Kinv = static_cast<TIO*>(g.Kinv);
    int q = 0;
    for (int I = 0; I < 8; ++I)
      for (int J = 0; J <= I; ++J, ++q) {
        if ((q & 7) != wave) continue;
        acc_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
        for (int K = I; K < 8; ++K) {
          const int pa = (K == I ? (int)leaf_yt_bytes(I) : (int)leaf_blk_bytes(I, K)) + P0;
          const int pb = (K == J ? (int)leaf_yt_bytes(J) : (int)leaf_blk_bytes(J, K)) + P0;
          T af[4], bf[4];
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) {
            af[k4] = ldsT(pa + k4 * 32);
            bf[k4] = ldsT(pb + k4 * 32);
          }
          a0 = C::mfma(af[0], bf[0], a0);
          a1 = C::mfma(af[2], bf[2], a1);
          a0 = C::mfma(af[1], bf[1], a0);
          a1 = C::mfma(af[3], bf[3], a1);
        }
        const int pc = (int)leaf_blk_bytes(I, J) + P1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const T v = a0[r] + a1[r];
          ldsT(pc + r * 4 * S * (int)sizeof(T)) = v;  // over L: nobody reads the factor any more
          Kinv[(size_t)(I * 16 + q4 + 4 * r) * 128 + J * 16 + m16] = (TIO)v;
        }
      }
  }
  if (!(g.mode & 4)) return;
  __syncthreads();
  if (t == 0) g_leaf_stamps[204] = (long long)__builtin_readcyclecounter();

  // ---- gradient (lml.rs:62-70): the arithmetic of gradtrace_kernel on the three lower 64x64 tiles; K^-1 and alpha come from the
  // LDS, the raw features are staged eight at a time
  {
    const int p = d + 2;
    double gsum[2] = {0, 0};          // noise, amplitude
    TIO coef[3][2][4], dsum[3][2][4];
#pragma unroll
    for (int tile = 0; tile < 3; ++tile)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) dsum[tile][r][c] = TIO(0);
    // pass A: scaled squared distances (matern_kernel.rs:94-98 form), then per entry the coefficient wgt * W * c * g(r)
    for (int kc = 0; kc < d; kc += 8) {
      stage_features(kc, false);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (kc + u < d) {
          const TIO il2 = (TIO)ellv[32 + kc + u];
#pragma unroll
          for (int tile = 0; tile < 3; ++tile) {
            TIO a[2], b[4];
#pragma unroll
            for (int r = 0; r < 2; ++r) a[r] = (TIO)feat[u * 128 + tile_i0(tile) + ty + 16 * (2 * half + r)];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = (TIO)feat[u * 128 + tile_j0(tile) + tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const TIO df = a[r] - b[c];
                dsum[tile][r][c] += df * df * il2;
              }
          }
        }
      }
      if (kc + 8 < d) __syncthreads();  // the last chunk stays staged: pass B starts with it when d <= 8
    }
#pragma unroll
    for (int tile = 0; tile < 3; ++tile)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int gi = tile_i0(tile) + ty + 16 * (2 * half + r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int gj = tile_j0(tile) + tx * 4 + c;
          TIO cf = TIO(0);
          if (gi < n && gj <= gi) {
#pragma clang fp contract(off)
            const TIO w = (TIO)av[gi] * (TIO)av[gj] - (TIO)As[gi * S + gj];  // lml.rs:62 (tmp)
            const TIO wgt = (gi == gj) ? TIO(1) : TIO(2);
            TIO km, gr;
            const TIO ds = dsum[tile][r][c];
            if (NU2 == 5) {
              const TIO tt = sqrt_nonneg(ds * TIO(5));
              const TIO e = exp_nonpos(-tt);
              km = __builtin_fma(tt * tt, TIO(1.0 / 3.0), TIO(1) + tt) * e;
              gr = TIO(5.0 / 3.0) * (tt + TIO(1)) * e;  // matern_kernel.rs:119-131
            } else if (NU2 == 3) {
              const TIO tt = sqrt_nonneg(ds * TIO(3));
              const TIO e = exp_nonpos(-tt);
              km = (tt + TIO(1)) * e;
              gr = TIO(3) * e;  // matern_kernel.rs:112-118
            } else if (NU2 == 0) {
              km = exp_nonpos(TIO(-0.5) * ds);
              gr = km;
            } else {
              const TIO rr = sqrt_nonneg(ds);
              km = exp_nonpos(-rr);
              gr = (rr > TIO(0)) ? km / rr : TIO(0);  // matern_kernel.rs:102-111
            }
            if (gi == gj) gsum[0] += (double)(w * noise);
            gsum[1] += (double)(wgt * w * (amp * km));
            cf = wgt * w * amp * gr;
          }
          coef[tile][r][c] = cf;
        }
      }
    {
      const double s0 = wave_sum(gsum[0]), s1 = wave_sum(gsum[1]);
      if (lane == 0) { red[wave * 35] = s0; red[wave * 35 + 1] = s1; }  // (the lml's sums in red were read before the K^-1 stage's barrier)
    }
    // pass B: the length-scale sums, eight parameters per staging
    const int last_kc = ((d - 1) >> 3) << 3;  // the chunk pass A left staged
    for (int kc = last_kc; kc >= 0; kc -= 8) {
      if (kc != last_kc) {
        __syncthreads();
        stage_features(kc, false);
        __syncthreads();
      }
      double acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (kc + u < d) {
          const TIO il2 = (TIO)ellv[32 + kc + u];
          TIO sacc = TIO(0);
#pragma unroll
          for (int tile = 0; tile < 3; ++tile) {
            TIO a[2], b[4];
#pragma unroll
            for (int r = 0; r < 2; ++r) a[r] = (TIO)feat[u * 128 + tile_i0(tile) + ty + 16 * (2 * half + r)];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = (TIO)feat[u * 128 + tile_j0(tile) + tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const TIO df = a[r] - b[c];
                sacc += coef[tile][r][c] * (df * df * il2);
              }
          }
          acc[u] = (double)sacc;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (kc + u < d) {
          const double sk = wave_sum(acc[u]);
          if (lane == 0) red[wave * 35 + 2 + kc + u] = sk;
        }
      }
    }
    __syncthreads();
    if (t < p) {
      double sacc = 0;
      for (int w = 0; w < 8; ++w) sacc += red[w * 35 + t];
      out->grad[t] = 0.5 * sacc;
    }
    __syncthreads();
    if (t == 0) {
      __threadfence_system();
      out->done = 3;
      g_leaf_stamps[205] = (long long)__builtin_readcyclecounter();
    }
  }
}

template <typename TIO, int NU2>
__global__ void __launch_bounds__(512, 2) small_eval_kernel(SmallEval g, const void* rv) {
  extern __shared__ __align__(16) char smem_raw[];
  small_eval_body<TIO, NU2>(g, rv, smem_raw);
}

// ---- the bounded L-BFGS step of lbfgs_step.hpp, one wavefront wide: lane i owns dimension i (the GP has at most 34 parameters
// here), a dot product is a reduction across the wave.  Same method, same constants, same decisions, same evaluation counting as
// lbfgs_begin / lbfgs_advance (which stay the host's implementation and this code's specification: a single thread walking
// the host form on the device took 70 us per evaluation -- longer than the evaluation -- because every load of the optimiser's
// state is a dependent round trip); sums run in another order, so iterates agree with the host form to rounding, not bit for
// bit (tests/test_gpu_fit.py compares the two on the same fits).  The vectors live in the run's LbfgsState in global memory
// (lane-indexed loads: never the scalar cache), the scalars in the wave's registers.
struct WaveLbfgs {
  int phase, nevals, iterations, converged, hcount;
  double f, step, gs;
  double rho[LBFGS_MAXM];
};

template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// sum / maximum over the 64 lanes, the result in every lane; fixed order: within quads, octets, rows of 16 (DPP), then the four rows
__device__ __forceinline__ double wave_allsum(double v) {
  v += dpp64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp64<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp64<0x141>(v);   // row_half_mirror
  v += dpp64<0x140>(v);   // row_mirror
  double r = readlane(v, 0);
  r += readlane(v, 16);
  r += readlane(v, 32);
  r += readlane(v, 48);
  return r;
}
__device__ __forceinline__ double wave_allmax(double v) {
  v = fmax(v, dpp64<0xB1>(v));
  v = fmax(v, dpp64<0x4E>(v));
  v = fmax(v, dpp64<0x141>(v));
  v = fmax(v, dpp64<0x140>(v));
  return fmax(fmax(readlane(v, 0), readlane(v, 16)), fmax(readlane(v, 32), readlane(v, 48)));
}

// proposes xn = clip(x + step d) (lane-wise); false: the step no longer changes x
__device__ __forceinline__ bool wl_propose(WaveLbfgs& w, LbfgsState* st, int i, bool act) {
  double dx = 0, gsl = 0;
  if (act) {
    double v = st->x[i] + w.step * st->d[i];
    v = fmin(fmax(v, st->lo[i]), st->hi[i]);
    st->xn[i] = v;
    dx = v - st->x[i];
    gsl = st->g[i] * dx;
  }
  w.gs = wave_allsum(gsl);
  return wave_allmax(fabs(dx)) != 0.0;
}

// start of an outer iteration at (x, f, g): convergence test, search direction, first trial point; returns the next phase
__device__ __forceinline__ int wl_begin_iteration(WaveLbfgs& w, LbfgsState* st, int i, bool act, int maxeval, double pgtol) {
  for (int guard = 0; guard < 3; ++guard) {
    if (w.nevals >= maxeval) return 2;
    const double xi = act ? st->x[i] : 0.0, gi = act ? st->g[i] : 0.0;
    const double loi = act ? st->lo[i] : 0.0, hii = act ? st->hi[i] : 0.0;
    const bool at_lo = xi <= loi && gi > 0, at_hi = xi >= hii && gi < 0;
    const double pg = (act && !(at_lo || at_hi)) ? gi : 0.0;
    if (wave_allmax(fabs(pg)) <= pgtol * fmax(1.0, fabs(w.f))) {
      w.converged = 1;
      return 2;
    }
    // two-loop recursion on the free variables; the history pairs of this lane's dimension are fetched up front (independent
    // loads: one round trip to the L2 instead of one per pair inside the dependent chain of reductions)
    double q = pg;
    double a[LBFGS_MAXM], sh[LBFGS_MAXM], yh[LBFGS_MAXM];
#pragma unroll
    for (int h = 0; h < LBFGS_MAXM; ++h) {
      const bool on = act && h < w.hcount;
      sh[h] = on ? st->S[h][i] : 0.0;
      yh[h] = on ? st->Y[h][i] : 0.0;
    }
#pragma unroll
    for (int h = LBFGS_MAXM - 1; h >= 0; --h) {
      a[h] = 0;
      if (h < w.hcount) {
        a[h] = w.rho[h] * wave_allsum(sh[h] * q);
        q -= a[h] * yh[h];
      }
    }
    double gamma = 1.0;
    if (w.hcount > 0) {
      double sl = 0, yl = 0;
#pragma unroll
      for (int h = 0; h < LBFGS_MAXM; ++h)
        if (h == w.hcount - 1) { sl = sh[h]; yl = yh[h]; }
      const double sy = wave_allsum(sl * yl), yy = wave_allsum(yl * yl);
      if (yy > 0) gamma = sy / yy;
    }
    q *= gamma;
#pragma unroll
    for (int h = 0; h < LBFGS_MAXM; ++h) {
      if (h < w.hcount) {
        const double bq = w.rho[h] * wave_allsum(yh[h] * q);
        q += sh[h] * (a[h] - bq);
      }
    }
    double dv = (pg == 0.0) ? 0.0 : -q;
    double dg = wave_allsum(dv * gi);
    if (!(dg < 0)) {  // not a descent direction: fall back to projected steepest descent
      w.hcount = 0;
      dv = -pg;
      dg = wave_allsum(dv * gi);
    }
    if (act) st->d[i] = dv;
    w.step = 1.0;
    if (w.hcount == 0) {
      const double dn = wave_allsum(dv * dv);
      w.step = fmin(1.0, 1.0 / sqrt(fmax(dn, 1e-300)));
    }
    if (wl_propose(w, st, i, act)) return 1;
    if (w.hcount > 0) {  // the first step does not move x: retry once from steepest descent with a clean history
      w.hcount = 0;
      continue;
    }
    return 2;
  }
  return 2;
}

// feeds the evaluation of the requested point (fe, the wave's gradient entry ge); true while another evaluation is wanted
__device__ __forceinline__ bool wl_advance(WaveLbfgs& w, LbfgsState* st, int i, bool act, double fe, double ge, int maxeval, int m,
                                           double pgtol, double ftol, bool fixed_work) {
  ++w.nevals;
  if (fe != fe) fe = INFINITY;
  int next = 2;
  if (w.phase == 0) {
    w.f = fe;
    if (act) st->g[i] = ge;
    next = (fe - fe == 0.0) ? wl_begin_iteration(w, st, i, act, maxeval, pgtol) : 2;
  } else if (w.phase == 1) {
    const double fn = fe;
    if ((fn - fn == 0.0) && fn <= w.f + 1e-4 * w.gs) {
      ++w.iterations;
      const double sv = act ? st->xn[i] - st->x[i] : 0.0, yv = act ? ge - st->g[i] : 0.0;
      const double sy = wave_allsum(sv * yv), ss = wave_allsum(sv * sv), yy = wave_allsum(yv * yv);
      if (sy > 1e-10 * sqrt(ss * yy) && sy > 0) {
        if (w.hcount == m) {  // drop the oldest pair
          for (int h = 1; h < w.hcount; ++h) {
            if (act) {
              st->S[h - 1][i] = st->S[h][i];
              st->Y[h - 1][i] = st->Y[h][i];
            }
          }
#pragma unroll
          for (int h = 1; h < LBFGS_MAXM; ++h) w.rho[h - 1] = w.rho[h];
          --w.hcount;
        }
        if (act) {
          st->S[w.hcount][i] = sv;
          st->Y[w.hcount][i] = yv;
        }
#pragma unroll
        for (int h = 0; h < LBFGS_MAXM; ++h)
          if (h == w.hcount) w.rho[h] = 1.0 / sy;
        ++w.hcount;
      }
      const double fold = w.f;
      if (act) {
        st->x[i] = st->xn[i];
        st->g[i] = ge;
      }
      w.f = fn;
      if (fold - w.f <= ftol * fmax(1.0, fabs(w.f))) {
        w.converged = 1;
        next = 2;
      } else {
        next = wl_begin_iteration(w, st, i, act, maxeval, pgtol);
      }
    } else {
      double nstep = 0.5 * w.step;
      if ((fn - fn == 0.0) && w.gs < 0) {
        const double denom = 2.0 * (fn - w.f - w.gs);
        if (denom > 0) nstep = fmin(fmax(-w.gs * w.step / denom, 0.1 * w.step), 0.5 * w.step);
      }
      w.step = nstep;
      const bool again = !(w.step < 1e-20) && w.nevals < maxeval && wl_propose(w, st, i, act);
      if (again) {
        next = 1;
      } else if (w.hcount > 0) {
        w.hcount = 0;
        next = w.nevals < maxeval ? wl_begin_iteration(w, st, i, act, maxeval, pgtol) : 2;
      } else {
        next = 2;
      }
    }
  }
  if (next == 1) {
    w.phase = 1;
    return true;
  }
  if (fixed_work && w.nevals < maxeval) {
    w.phase = 2;
    return true;
  }
  w.phase = 3;
  return false;
}

// out-of-line copy of the evaluation for small_fit_kernel: a register allocation of its own (inlined into the loop the kernel
// spilled 216 VGPRs)
template <typename TIO, int NU2>
__device__ __attribute__((noinline)) void small_eval_call(const SmallEval* g, const void* rv, char* smem_raw) {
  small_eval_body<TIO, NU2>(*g, rv, smem_raw);
}

// ---- a whole optimiser run in ONE launch (n <= 128): the evaluation above in a loop, with the bounded L-BFGS step and the fit's
// objective wrapper (fit.rs:94-133: clamped parameters, failed factorisation -> +inf, capture of the best evaluation) on the
// device, in wave 0.  The host launches one such kernel per optimiser run (gradmin.rs:19-31: the runs are independent), all
// side by side, and collects.  The ~40 us round trip through the host per evaluation (graph launch + completion wake-up +
// three host threads on the runtime's lock) becomes ~5 us of wave-wide vector arithmetic.
template <typename TIO, int NU2>
__global__ void __launch_bounds__(512, 2) small_fit_kernel(const SmallFit* __restrict__ fs) {
  // one workgroup = one optimiser run: the runs of a fit are the workgroups of ONE launch (round 4: one launch per run on a
  // stream of its own -- three streams per fit, and HIP maps streams onto a handful of hardware queues: fits side by side
  // then queued behind each other's persistent kernels)
  const SmallFit f = fs[blockIdx.x];
  extern __shared__ __align__(16) char smem_raw[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int p = f.ev.d + 2;
  LbfgsState* st = f.st;
  int* flags = reinterpret_cast<int*>(smem_raw + 163840 - 64);  // [0] another evaluation is wanted, [1] its ping-pong target
  SmallFitResult* res = f.res;
  EvalParams* P = const_cast<EvalParams*>(f.ev.P);
  const bool act = wave == 0 && lane < p;
  // wave 0's view of the run (registers: a scalar stored to global memory and re-read through a uniform address could come back
  // stale from the scalar cache)
  WaveLbfgs w{};
  int best_idx = -1, best_eval = 0, n_evals = 0, n_not_pd = 0;
  double best_lml = -INFINITY;
  double cur_param = 0.0;  // wave 0, lane = parameter: what the evaluation in flight runs with
  double best_th = 0.0, best_par = 0.0;  // wave 0, lane = parameter: the captured evaluation's (for the pinned copy of the result)
  // wave 0: the requested point -> clamped linear-space parameters (fit.rs:94-96; the noise is not clamped, :96)
  auto publish_request = [&]() {
    if (act) {
      const double th = w.phase == 1 ? st->xn[lane] : st->x[lane];
      double v = exp(th);
      if (lane >= 1) v = v < f.lo[lane] ? f.lo[lane] : (f.hi[lane] < v ? f.hi[lane] : v);  // bounded_value.rs:43-56
      cur_param = v;
      if (lane == 0) P->noise = v;
      else if (lane == 1) P->amp = v;
      else P->ell[lane - 2] = v;
    }
    if (lane == 0) flags[1] = best_idx < 0 ? 0 : 1 - best_idx;  // never overwrite the captured best (fit.rs:116-125)
    __threadfence();
  };
  if (wave == 0) {
    // log-space box (fit.rs:137-146) and the clipped start point
    if (act) {
      const double l = log(f.lo[lane]), h = log(f.hi[lane]);
      st->lo[lane] = l;
      st->hi[lane] = h;
      st->x[lane] = fmin(fmax(f.x0[lane], l), h);
    }
    w.phase = 0;
    w.f = INFINITY;
    w.step = 1.0;
    if (lane == 0) flags[0] = 1;
    publish_request();
  }
  __syncthreads();
  for (int eval_idx = 0; eval_idx < f.maxeval + 1; ++eval_idx) {  // bounded whatever the state machine does
    const int target = flags[1];
    __syncthreads();  // the flags sit behind the evaluation's scratch: read before it starts
    SmallEval g = f.ev;
    g.Kinv = f.Kinv[target];
    g.alpha = f.alpha[target];
    if (f.Xinv[target]) {
      g.W2 = f.Xinv[target];
      g.ldiag = f.ldiag[target];
    }
    g.mode = 7;
    small_eval_call<TIO, NU2>(&g, f.rv, smem_raw);
    __threadfence();
    __syncthreads();
    if (wave == 0) {
      const EvalOut* out = g.hout;
      double lml = __hip_atomic_load(&out->lml, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      double ge = act ? __hip_atomic_load(&out->grad[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      const int info = __hip_atomic_load(&out->info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool ok = info == 0 && (lml - lml == 0.0) && wave_allmax((ge - ge == 0.0) ? 0.0 : 1.0) == 0.0;
      if (!ok) {  // handled like a failed factorisation (lml.rs:47-50 -> fit.rs:105-112): objective +inf, zero gradient
        lml = -INFINITY;
        ge = 0.0;
        ++n_not_pd;
      }
      ++n_evals;
      const double th = act ? (w.phase == 1 ? st->xn[lane] : st->x[lane]) : 0.0;
      if (eval_idx < f.trace_cap) {
        if (act) {
          f.trace_theta[(size_t)eval_idx * p + lane] = th;
          f.trace_grad[(size_t)eval_idx * p + lane] = ge;
        }
        if (lane == 0) f.trace_lml[eval_idx] = lml;
      }
      if (ok && (best_idx < 0 || lml > best_lml)) {  // strictly greater wins; ties keep the earlier evaluation
        best_idx = target;
        best_lml = lml;
        best_eval = eval_idx;
        if (act) {
          res->best_theta[lane] = th;
          res->best_params[lane] = cur_param;
          best_th = th;
          best_par = cur_param;
        }
      }
      // fit.rs:128-133: the optimiser minimises -lml
      const bool more = wl_advance(w, st, lane, act, ok ? -lml : INFINITY, -ge, f.maxeval, f.memory < 1 ? 1 : (f.memory > LBFGS_MAXM ? LBFGS_MAXM : f.memory),
                                   f.pgtol, f.ftol, f.fixed_work != 0);
      if (lane == 0) flags[0] = more ? 1 : 0;
      if (more) publish_request();
    }
    __syncthreads();
    const int more = flags[0];
    __syncthreads();
    if (!more) break;
  }
  if (t == 0) {
    res->best_idx = best_idx;
    res->best_lml = best_lml;
    res->best_eval = best_eval;
    res->n_evals = n_evals;
    res->n_not_pd = n_not_pd;
  }
  // the run is over: its result to the pinned block and the word its host thread polls (every wave's device writes of the last
  // evaluation are behind an agent-scope fence and a barrier; a later kernel of any stream starts with an acquire of its own)
  if (wave == 0 && f.hres) {
    SmallFitResult* h = f.hres;
    if (act) {
      h->best_theta[lane] = best_th;
      h->best_params[lane] = best_par;
    }
    if (lane == 0) {
      h->best_idx = best_idx;
      h->best_lml = best_lml;
      h->best_eval = best_eval;
      h->n_evals = n_evals;
      h->n_not_pd = n_not_pd;
    }
    __threadfence_system();
    if (lane == 0) __hip_atomic_store(f.hdone, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <typename T>
void launch_small_fit(const SmallFit* fs_dev, int nruns, int nu2, hipStream_t s) {
  const dim3 grid(nruns), block(512);
  const size_t lds = 163840;  // the whole LDS of a CU
  switch (nu2) {
    case 0: hipLaunchKernelGGL((small_fit_kernel<T, 0>), grid, block, lds, s, fs_dev); break;
    case 1: hipLaunchKernelGGL((small_fit_kernel<T, 1>), grid, block, lds, s, fs_dev); break;
    case 3: hipLaunchKernelGGL((small_fit_kernel<T, 3>), grid, block, lds, s, fs_dev); break;
    default: hipLaunchKernelGGL((small_fit_kernel<T, 5>), grid, block, lds, s, fs_dev); break;
  }
}
template void launch_small_fit<double>(const SmallFit*, int, int, hipStream_t);
template void launch_small_fit<float>(const SmallFit*, int, int, hipStream_t);

template <typename T>
void launch_small_eval(const SmallEval& g, const void* rv, int nu2, hipStream_t s) {
  const dim3 grid(1), block(512);
  const size_t lds = 163840;  // the whole LDS of a CU: the block image + the kernel's scratch
  switch (nu2) {
    case 0: hipLaunchKernelGGL((small_eval_kernel<T, 0>), grid, block, lds, s, g, rv); break;
    case 1: hipLaunchKernelGGL((small_eval_kernel<T, 1>), grid, block, lds, s, g, rv); break;
    case 3: hipLaunchKernelGGL((small_eval_kernel<T, 3>), grid, block, lds, s, g, rv); break;
    default: hipLaunchKernelGGL((small_eval_kernel<T, 5>), grid, block, lds, s, g, rv); break;
  }
}
template void launch_small_eval<double>(const SmallEval&, const void*, int, hipStream_t);
template void launch_small_eval<float>(const SmallEval&, const void*, int, hipStream_t);

// =================================================================================================================
// posterior sample paths (hbegp_paths_*): pathwise conditioning on a random-Fourier-feature prior draw
//   f_s(x) = A sum_j w_sj cos(th_j(x)) + sum_i k(x, x_i) v_is,   th_j(x) = om_j . x + b_j,  A = sqrt(2 c / F),  om_jk = om0_jk / ell_k
//   df_s/dx_k = -A sum_j w_sj sin(th_j) om_jk + sum_i c psi(r_i) (x_k - x_ik) / ell_k^2 v_is
//   v_s = L^-T L^-1 r_s,  r_s = y - Phi(X) w_s - sqrt(sigma^2) eps_s    (two triangular tile GEMMs over an [S_p][n_p] operand)
// The phase, sin / cos, psi and every sum are fp64 for both element types: nu = 1/2 has a Cauchy spectral density, |th| reaches
// 1e4 .. 1e6, where an f32 argument has lost the 1e-4 bar before the cosine is taken.  r^2 is accumulated in the element type
// with kstar_kernel's scaling and order, so that k(x, x_i) agrees with the predict path.
//
// paths_project_kernel (preparation): grid (ceil(n/64), feature chunks (paths_project_chunks), ceil(S/64)).  A workgroup takes 64 training points (the
// lane) and walks its feature chunk 32 features at a time: the four waves fill phi[32][64] = cos(th) in the LDS (a feature is
// wave-uniform: its frequencies and the weights w_sj are scalar loads), then wave w adds the 32 features in ascending order
// into 16 accumulators, paths 64 z + 16 w .. + 15.  Phi(X) [n][F] is never stored.  part[chunk][s][i];
// paths_project_finish_kernel adds the chunks in ascending order and writes r into R^T [S_p][n_p] (zero padding).
//
// paths_eval_kernel<T, SB, DATA>: two launches, grid (ceil(items/4), data chunks) and (ceil(items/4), feature chunks), item = (point, block of SB paths): wave w of a
// workgroup is one item, the lane walks the chunk's terms -- PE_CHUNK training points (pred_grad_kernel's shape: 64 at a time
// through the LDS) or PE_CHUNK features -- 64 apart in ascending order.  A term's kernel value / slope or cosine / sine is
// computed once and used for the item's SB paths: SB (1 + PE_KB) fp64 accumulators per lane, PE_KB gradient components per pass.
// One wave_sum each -> part[chunk][row][1 + d], row = s m + point; paths_eval_finish_kernel adds the chunks in ascending
// order, data chunks first.  SB = 1 serves per-path points (every path its own x), SB = PE_SB shared points.  A path's sums do
// not depend on SB, on the other paths of its block or on the other points of the call: the same (path, point) gives the same
// bits alone, in a batch, shared or per path.  No atomics.
// =================================================================================================================
constexpr int PP_FT = 32;       // features per LDS tile of the projection
constexpr int PE_CHUNK = 512;   // terms per workgroup of the evaluation
constexpr int PE_KB = 8;        // gradient components per pass
constexpr int PE_SB = 2;        // paths per item at shared points (4: 151 VGPRs and a handful of SGPR spills)

template <typename T>
__global__ void __launch_bounds__(256) paths_project_kernel(const T* __restrict__ X, int n, int d, const double* __restrict__ omT,
                                                            const double* __restrict__ phase, int F, int fch,
                                                            const double* __restrict__ Wf, int S, double* __restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) char smem_raw[];
  double* phi = reinterpret_cast<double*>(smem_raw);  // [PP_FT][64]
  T* sx = reinterpret_cast<T*>(phi + PP_FT * 64);      // [d][64] features of the 64 training points (unscaled)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i0 = blockIdx.x * 64, gi = i0 + lane;
  const int f0 = blockIdx.y * fch, f1 = min(F, f0 + fch);
  const int s0 = blockIdx.z * 64 + w * 16;
  for (int e = t; e < 64 * d; e += 256) {
    const int row = e / d, k = e - row * d;
    sx[k * 64 + row] = (i0 + row < n) ? X[(size_t)(i0 + row) * d + k] : T(0);
  }
  double acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0;
  for (int j0 = f0; j0 < f1; j0 += PP_FT) {
    __syncthreads();  // the previous tile is consumed (first time: sx is written)
    for (int e = 0; e < PP_FT / 4; ++e) {
      const int jj = w + 4 * e, j = j0 + jj;  // wave-uniform
      double c = 0.0;
      if (j < f1) {
        double th = phase[j];
        for (int k = 0; k < d; ++k) th = __builtin_fma((double)sx[k * 64 + lane], omT[(size_t)k * F + j], th);
        c = cos(th);
      }
      phi[jj * 64 + lane] = c;
    }
    __syncthreads();
    const int jn = min(PP_FT, f1 - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const double p = phi[jj * 64 + lane];
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (s0 + q < S) acc[q] = __builtin_fma(Wf[(size_t)(s0 + q) * F + j0 + jj], p, acc[q]);
    }
  }
  if (gi < n) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (s0 + q < S) part[((size_t)blockIdx.y * S + s0 + q) * n + gi] = acc[q];
  }
}

// R^T[s][i] = y_i - A sum_chunks part[c][s][i] - sqrt(sigma^2 + v_i) eps[s][i] (eps may be null, v_i = 0 without rv); zero for s >= S or i >= n
template <typename T>
__global__ void __launch_bounds__(256) paths_project_finish_kernel(const double* __restrict__ part, int nch, int n, int np, int S, int F,
                                                                   const T* __restrict__ y, const T* __restrict__ eps,
                                                                   const T* __restrict__ rv, const EvalParams* __restrict__ P,
                                                                   T* __restrict__ Rt) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (i >= np) return;
  T r = T(0);
  if (s < S && i < n) {
    double sm = 0.0;
    for (int c = 0; c < nch; ++c) sm += part[((size_t)c * S + s) * n + i];
    double v = (double)y[i] - sqrt(2.0 * P->amp / (double)F) * sm;
    // the noise draw of row i: its learned noise plus, where the model has them, its known variance (rv: n entries or null)
    if (eps) v -= sqrt(rv ? P->noise + (double)rv[i] : P->noise) * (double)eps[(size_t)s * n + i];
    r = (T)v;
  }
  Rt[(size_t)s * np + i] = r;
}

// om^T[k][j] = om0[j][k] / ell_k (fp64 for both element types)
template <typename T>
__global__ void __launch_bounds__(256) paths_scale_omega_kernel(const T* __restrict__ om0, int F, int d, const EvalParams* __restrict__ P,
                                                                double* __restrict__ omT) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F * d) return;
  const int k = e / F, j = e - k * F;
  omT[e] = (double)om0[(size_t)j * d + k] / P->ell[k];
}

template <typename T, int SB, bool DATA>
__global__ void __launch_bounds__(256) paths_eval_kernel(const T* __restrict__ Xs, int m, int per_path, int S, const T* __restrict__ X, int n,
                                                         int d, int nu2, const EvalParams* __restrict__ P, const T* __restrict__ Vt, int np,
                                                         const double* __restrict__ omT, const double* __restrict__ phase,
                                                         const double* __restrict__ Wf, int F, int nchd, int want_grad,
                                                         double* __restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) char smem_raw[];
  T* sx = reinterpret_cast<T*>(smem_raw);  // [d][64] scaled features of 64 training points
  T* sq = sx + (size_t)d * 64;             // [4][d] this workgroup's query points: scaled (data chunks) or raw (feature chunks)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nsb = (S + SB - 1) / SB, items = m * nsb, d1 = d + 1;
  constexpr bool data = DATA;
  const int chunk = DATA ? (int)blockIdx.y : nchd + (int)blockIdx.y;  // data chunks first
  for (int e = t; e < 4 * d; e += 256) {
    const int q = e / d, k = e - q * d, it = blockIdx.x * 4 + q;
    T v = T(0);
    if (it < items) {
      const int pt = it / nsb, sb = it - pt * nsb;
      v = Xs[(per_path ? (size_t)sb * SB * m + pt : (size_t)pt) * d + k];  // per_path: SB = 1, the path's own point
      if (data) v = v / (T)P->ell[k];
    }
    sq[e] = v;
  }
  const int item = blockIdx.x * 4 + w;
  const bool live = item < items;
  const int pt = live ? item / nsb : 0, s0 = live ? (item - pt * nsb) * SB : 0;
  const T* xq = sq + w * d;
  const int npass = want_grad ? (d + PE_KB - 1) / PE_KB : 1;
  for (int ps = 0; ps < npass; ++ps) {
    const int kb = ps * PE_KB;
    double af[SB], ag[SB][PE_KB];
#pragma unroll
    for (int q = 0; q < SB; ++q) {
      af[q] = 0.0;
#pragma unroll
      for (int kk = 0; kk < PE_KB; ++kk) ag[q][kk] = 0.0;
    }
    if constexpr (data) {
      const int jc0 = blockIdx.y * PE_CHUNK, jc1 = min(n, jc0 + PE_CHUNK);
      const double amp = P->amp;
      for (int j0 = jc0; j0 < jc1; j0 += 64) {
        __syncthreads();  // the previous 64 points are consumed (first time: sq is written)
        for (int e = t; e < 64 * d; e += 256) {
          const int jj = e / d, k = e - jj * d, gj = j0 + jj;
          sx[k * 64 + jj] = (gj < n) ? X[(size_t)gj * d + k] / (T)P->ell[k] : T(0);
        }
        __syncthreads();
        const int j = j0 + lane;
        if (live && j < jc1) {
          T r2 = T(0);
          for (int k = 0; k < d; ++k) {  // kstar_kernel's accumulation
            const T df = xq[k] - sx[k * 64 + lane];
            r2 += df * df;
          }
          const double kv = (double)kmat_entry<T>(r2, nu2, (T)amp, T(0), false);
          const double sl = (!want_grad || r2 == T(0)) ? 0.0 : amp * matern_psi((double)r2, nu2);
          double dk[PE_KB];
#pragma unroll
          for (int kk = 0; kk < PE_KB; ++kk) {  // components past d repeat the last one (never written)
            const int kc = min(kb + kk, d - 1);
            dk[kk] = (double)(xq[kc] - sx[kc * 64 + lane]);
          }
#pragma unroll
          for (int q = 0; q < SB; ++q) {  // a block's tail repeats the last path (never written)
            const double v = (double)Vt[(size_t)min(s0 + q, S - 1) * np + j];
            af[q] = __builtin_fma(kv, v, af[q]);
            const double a = sl * v;
#pragma unroll
            for (int kk = 0; kk < PE_KB; ++kk) ag[q][kk] = __builtin_fma(a, dk[kk], ag[q][kk]);
          }
        }
      }
    } else {
      __syncthreads();  // sq is written
      const int jc0 = (int)blockIdx.y * PE_CHUNK, jc1 = min(F, jc0 + PE_CHUNK);
      for (int j = jc0 + lane; j < jc1 && live; j += 64) {
        double th = phase[j];
        for (int k = 0; k < d; ++k) th = __builtin_fma((double)xq[k], omT[(size_t)k * F + j], th);
        double sn, cs;
        sincos(th, &sn, &cs);  // one range reduction for both
        double om[PE_KB];
#pragma unroll
        for (int kk = 0; kk < PE_KB; ++kk) om[kk] = omT[(size_t)min(kb + kk, d - 1) * F + j];
#pragma unroll
        for (int q = 0; q < SB; ++q) {
          const double wv = Wf[(size_t)min(s0 + q, S - 1) * F + j];
          af[q] = __builtin_fma(wv, cs, af[q]);
          const double a = -(wv * sn);
#pragma unroll
          for (int kk = 0; kk < PE_KB; ++kk) ag[q][kk] = __builtin_fma(a, om[kk], ag[q][kk]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < SB; ++q) {
      const bool on = live && s0 + q < S;  // wave-uniform
      double* pr = part + (((size_t)chunk * S + (on ? s0 + q : 0)) * m + pt) * d1;
      if (ps == 0) {
        const double sm = wave_sum(af[q]);
        if (on && lane == 0) pr[0] = sm;
      }
      if (want_grad) {
#pragma unroll
        for (int kk = 0; kk < PE_KB; ++kk) {
          if (kb + kk < d) {
            const double sm = wave_sum(ag[q][kk]);
            if (on && lane == 0) pr[1 + kb + kk] = sm;
          }
        }
      }
    }
  }
}

// f[s][i] = sum of the data chunks + A * sum of the feature chunks; df[s][i][k] = (data sum) / ell_k + A * (feature sum)
template <typename T>
__global__ void __launch_bounds__(256) paths_eval_finish_kernel(const double* __restrict__ part, int nchd, int nch, int rows, int d, int F,
                                                                const EvalParams* __restrict__ P, int want_grad, T* __restrict__ f,
                                                                T* __restrict__ df) {
#pragma clang fp contract(off)
  const int d1 = d + 1;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)rows * d1) return;
  const int c0 = (int)(e % d1);
  const size_t row = e / d1;
  if (c0 > 0 && !want_grad) return;
  double sd = 0.0, sf = 0.0;
  for (int c = 0; c < nchd; ++c) sd += part[(size_t)c * rows * d1 + e];
  for (int c = nchd; c < nch; ++c) sf += part[(size_t)c * rows * d1 + e];
  const double A = sqrt(2.0 * P->amp / (double)F);
  if (c0 == 0) f[row] = (T)(sd + A * sf);
  else df[row * d + (c0 - 1)] = (T)(sd / P->ell[c0 - 1] + A * sf);
}

// Feature chunks of the projection.  A workgroup walks its chunk serially (one fp64 cosine per lane and feature), so the chunk
// length is the launch's latency: chunks of 64 features while the partial sums (chunks x S x n doubles) stay within 128 MiB and
// there are at most 64 of them, longer ones beyond.  The split depends only on (F, n, S): one handle, one summation order.
int paths_project_chunks(int F, int n, int S, int* fch_out, int* cap_out) {
  const size_t per_chunk = sizeof(double) * (size_t)S * (size_t)n;
  const int cap = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)128 << 20) / per_chunk));
  int nch = std::max(1, std::min(cap, (F + 63) / 64));
  int fch = ((F + nch - 1) / nch + PP_FT - 1) / PP_FT * PP_FT;
  nch = (F + fch - 1) / fch;
  if (fch_out) *fch_out = fch;
  if (cap_out) *cap_out = cap;
  return nch;
}
int paths_eval_chunks(int n, int F, int* nchd_out) {
  const int nchd = (n + PE_CHUNK - 1) / PE_CHUNK;
  if (nchd_out) *nchd_out = nchd;
  return nchd + (F + PE_CHUNK - 1) / PE_CHUNK;
}
template <typename T>
void launch_paths_scale_omega(const T* om0, int F, int d, const EvalParams* P, double* omT, hipStream_t s) {
  hipLaunchKernelGGL((paths_scale_omega_kernel<T>), dim3((F * d + 255) / 256), dim3(256), 0, s, om0, F, d, P, omT);
}
template <typename T>
void launch_paths_project(const T* X, int n, int d, int np, const double* omT, const double* phase, int F, const double* Wf, int S, int Sp,
                          const T* y, const T* eps, const T* rv, const EvalParams* P, double* part, T* Rt, hipStream_t s) {
  int fch = 0;
  const int nch = paths_project_chunks(F, n, S, &fch);
  const size_t lds = sizeof(double) * PP_FT * 64 + sizeof(T) * (size_t)d * 64;
  hipLaunchKernelGGL((paths_project_kernel<T>), dim3((n + 63) / 64, nch, (S + 63) / 64), dim3(256), lds, s, X, n, d, omT, phase, F, fch, Wf,
                     S, part);
  hipLaunchKernelGGL((paths_project_finish_kernel<T>), dim3((np + 255) / 256, Sp), dim3(256), 0, s, part, nch, n, np, S, F, y, eps, rv, P, Rt);
}
template <typename T>
void launch_paths_eval(const T* Xs, int m, int per_path, int S, const T* X, int n, int d, int np, int nu2, const EvalParams* P, const T* Vt,
                       const double* omT, const double* phase, const double* Wf, int F, int want_grad, double* part, T* f, T* df,
                       hipStream_t s) {
  int nchd = 0;
  const int nch = paths_eval_chunks(n, F, &nchd);
  const size_t lds = (size_t)(64 + 4) * d * sizeof(T);
  const int rows = S * m;
  if (per_path) {
    hipLaunchKernelGGL((paths_eval_kernel<T, 1, true>), dim3((rows + 3) / 4, nchd), dim3(256), lds, s, Xs, m, 1, S, X, n, d, nu2, P, Vt, np, omT,
                       phase, Wf, F, nchd, want_grad, part);
    hipLaunchKernelGGL((paths_eval_kernel<T, 1, false>), dim3((rows + 3) / 4, nch - nchd), dim3(256), lds, s, Xs, m, 1, S, X, n, d, nu2, P, Vt, np,
                       omT, phase, Wf, F, nchd, want_grad, part);
  } else {
    const int items = m * ((S + PE_SB - 1) / PE_SB);
    hipLaunchKernelGGL((paths_eval_kernel<T, PE_SB, true>), dim3((items + 3) / 4, nchd), dim3(256), lds, s, Xs, m, 0, S, X, n, d, nu2, P, Vt, np, omT,
                       phase, Wf, F, nchd, want_grad, part);
    hipLaunchKernelGGL((paths_eval_kernel<T, PE_SB, false>), dim3((items + 3) / 4, nch - nchd), dim3(256), lds, s, Xs, m, 0, S, X, n, d, nu2, P, Vt, np,
                       omT, phase, Wf, F, nchd, want_grad, part);
  }
  const size_t tot = (size_t)rows * (d + 1);
  hipLaunchKernelGGL((paths_eval_finish_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part, nchd, nch, rows, d, F, P,
                     want_grad, f, df);
}
#define PATHS_INST(T)                                                                                                                     \
  template void launch_paths_scale_omega<T>(const T*, int, int, const EvalParams*, double*, hipStream_t);                                  \
  template void launch_paths_project<T>(const T*, int, int, int, const double*, const double*, int, const double*, int, int, const T*,     \
                                        const T*, const T*, const EvalParams*, double*, T*, hipStream_t);                                  \
  template void launch_paths_eval<T>(const T*, int, int, int, const T*, int, int, int, int, const EvalParams*, const T*, const double*,    \
                                     const double*, const double*, int, int, double*, T*, T*, hipStream_t);
PATHS_INST(double)
PATHS_INST(float)
#undef PATHS_INST

// =================================================================================================================
// expected hypervolume improvement of two independent objectives over a candidate set (hbegp.cpp: model_ehvi).
// The host reduces the front to P non-dominated points inside the reference box, a ascending and b descending, and hands over
// ns = P + 1 strips: strip i spans objective 0 from a_i (a_0 = -inf) to up[i] = a_{i+1} (up[P] = r1) below the height
// hb[i] = b_i (hb[0] = r2).  thr = [up | hb].  With G_k(t) = E[(t - Y_k)^+] = sigma_k h((t - mu_k) / sigma_k), h(z) = z Phi(z) + phi(z),
//   EHVI = sum_i [G_1(up_i) - G_1(up_{i-1})] G_2(hb_i),   dG/dmu = -Phi(z),  dG/dsigma = phi(z).
// One WAVE per candidate, EHVI_WAVES candidates per workgroup; lane l takes the strips l, l + 64, ..: it evaluates (G_1, Phi, phi)
// at up_i and (G_2, Phi, phi) at hb_i once each and takes the values at up_{i-1} from lane l - 1 (lane 0: from lane 63's previous
// strip, nothing for strip 0) -- the same function of the same threshold, so the same bits as evaluating it twice.  Each lane adds
// its strips in ascending order into five sums (the value and the partials w.r.t. mu_1, sigma_1, mu_2, sigma_2), which then go
// through one xor butterfly (a fixed tree: every lane ends with the same bits).  Lane k < d forms grad[j][k] by the chain rule,
// dsigma = dvar / (2 sigma).  All of it in fp64 for both element types, the five sums with or without a gradient: a candidate's
// bits depend on nothing but its own posterior and the thresholds.  sigma = 0 (ei_with_gradient's test): G(t) = (t - mu)^+,
// Phi = [t > mu], phi = 0 and dsigma counts as 0.  A NaN in a candidate's posterior gives NaN in its value and its gradient row.
// The thresholds are staged in dynamic LDS up to EHVI_LDS_STRIPS strips (16 bytes each); beyond, they are read from global memory
// (every wave reads the same few KiB: they stay in the L2).
// =================================================================================================================
constexpr int EHVI_WAVES = 4;

struct EhviG {
  double g, cdf, pdf;  // G(t), Phi(z), phi(z)
};
// not inlined: erfc's fp64 coefficients (as kg_tail, whose evaluation of phi(a) - a Phi(-a) this is for z <= 0; h(z) = z + h(-z)
// above).  Beyond |z| = 38 the tail terms are below 1e-314.
__device__ __noinline__ EhviG ehvi_g(double t, double mu, double sd) {
  EhviG r;
  if (!(sd > 2.220446049250313e-16)) {  // sigma = 0
    r.g = fmax(t - mu, 0.0);
    r.cdf = t > mu ? 1.0 : 0.0;
    r.pdf = 0.0;
    return r;
  }
  const double z = (t - mu) / sd;
  const double az = fabs(z);
  double tail = 0.0, cl = 0.0, pdf = 0.0;  // h(-|z|), Phi(-|z|), phi(z)
  if (az < 38.0) {
    cl = 0.5 * erfc(az / 1.4142135623730951);
    pdf = exp(-0.5 * az * az) / 2.5066282746310002;
    tail = fmax(pdf - az * cl, 0.0);
  }
  r.g = sd * (z > 0.0 ? z + tail : tail);
  r.cdf = z > 0.0 ? 1.0 - cl : cl;
  r.pdf = pdf;
  return r;
}

// the sum over the 64 lanes through one xor butterfly, the result in every lane: a fixed tree, so every lane ends with the same bits
// (ehvi_kernel, mes_kernel)
__device__ __forceinline__ double wave_xor_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(64 * EHVI_WAVES) ehvi_kernel(const T* __restrict__ mean1, const T* __restrict__ var1,
                                                               const T* __restrict__ dmean1, const T* __restrict__ dvar1,
                                                               const T* __restrict__ mean2, const T* __restrict__ var2,
                                                               const T* __restrict__ dmean2, const T* __restrict__ dvar2, int m, int d,
                                                               const double* __restrict__ thr, int ns, int want_grad,
                                                               double* __restrict__ ehvi, T* __restrict__ grad) {
  extern __shared__ __align__(16) char smem_raw[];
  const double* up = thr;
  const double* hb = thr + ns;
  if (LDS) {
    double* st = reinterpret_cast<double*>(smem_raw);
    for (int i = threadIdx.x; i < 2 * ns; i += 64 * EHVI_WAVES) st[i] = thr[i];
    __syncthreads();
    up = st;
    hb = st + ns;
  }
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * EHVI_WAVES + (threadIdx.x >> 6);
  if (j >= m) return;  // whole waves leave, behind the only barrier
  const double mu1 = (double)mean1[j], v1 = (double)var1[j], mu2 = (double)mean2[j], v2 = (double)var2[j];
  const double sd1 = sqrt(v1), sd2 = sqrt(v2);
  const bool bad = (mu1 != mu1) || (v1 != v1) || (mu2 != mu2) || (v2 != v2);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  EhviG carry = {0.0, 0.0, 0.0};  // lane 63's upper threshold of the previous chunk (strip 0: G_1(-inf) = 0)
  for (int base = 0; base < ns; base += 64) {  // a uniform trip count: every lane takes part in the shuffles
    const int i = base + lane;
    const bool on = i < ns;
    EhviG u = {0.0, 0.0, 0.0}, h = {0.0, 0.0, 0.0};
    if (on) {
      u = ehvi_g(up[i], mu1, sd1);
      h = ehvi_g(hb[i], mu2, sd2);
    }
    EhviG lo;
    lo.g = __shfl_up(u.g, 1, 64);
    lo.cdf = __shfl_up(u.cdf, 1, 64);
    lo.pdf = __shfl_up(u.pdf, 1, 64);
    if (lane == 0) lo = carry;
    carry.g = __shfl(u.g, 63, 64);
    carry.cdf = __shfl(u.cdf, 63, 64);
    carry.pdf = __shfl(u.pdf, 63, 64);
    if (on) {
      const double dg = u.g - lo.g;
      s0 += fmax(dg, 0.0) * h.g;            // G_1 is monotone: a negative difference is rounding
      s1 += (lo.cdf - u.cdf) * h.g;         // d/dmu_1
      s2 += (u.pdf - lo.pdf) * h.g;         // d/dsigma_1
      s3 -= dg * h.cdf;                     // d/dmu_2
      s4 += dg * h.pdf;                     // d/dsigma_2
    }
  }
  s0 = wave_xor_sum(s0);
  s1 = wave_xor_sum(s1);
  s2 = wave_xor_sum(s2);
  s3 = wave_xor_sum(s3);
  s4 = wave_xor_sum(s4);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (lane == 0) ehvi[j] = bad ? nan : s0;
  if (want_grad && lane < d) {
    const size_t e = (size_t)j * d + lane;
    const double ds1 = sd1 > 2.220446049250313e-16 ? (double)dvar1[e] / (2.0 * sd1) : 0.0;
    const double ds2 = sd2 > 2.220446049250313e-16 ? (double)dvar2[e] / (2.0 * sd2) : 0.0;
    double g = s1 * (double)dmean1[e];
    g += s2 * ds1;
    g += s3 * (double)dmean2[e];
    g += s4 * ds2;
    grad[e] = bad ? (T)nan : (T)g;
  }
}

// The arg-max of the marginal acquisition functions (EHVI, cEI, log-cEI, MES): best = the LAST index of the maximum of v[0 .. m)
// through a fixed LDS tree (kg_epilogue_kernel's rule); a NaN never wins, -1 where no entry is a number
__global__ void __launch_bounds__(BSEL_THREADS) argmax_last_kernel(const double* __restrict__ v, int m, int* __restrict__ res) {
  __shared__ double sv[BSEL_THREADS];
  __shared__ int si[BSEL_THREADS];
  const int tid = threadIdx.x;
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < m; i += BSEL_THREADS) {
    const double e = v[i];
    if (e == e && (bi < 0 || e >= best)) { best = e; bi = i; }  // ascending i: an equal value moves to the later index
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
#pragma unroll 1
  for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = sv[tid + w];
      const int oi = si[tid + w];
      if (oi >= 0 && (si[tid] < 0 || o > sv[tid] || (o == sv[tid] && oi > si[tid]))) { sv[tid] = o; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) res[0] = si[0];
}
static void launch_argmax_last(const double* v, int m, int* best, hipStream_t s) {
  hipLaunchKernelGGL(argmax_last_kernel, dim3(1), dim3(BSEL_THREADS), 0, s, v, m, best);
}

template <typename T>
void launch_ehvi(const T* mean1, const T* var1, const T* dmean1, const T* dvar1, const T* mean2, const T* var2, const T* dmean2,
                 const T* dvar2, int m, int d, const double* thr, int ns, int want_grad, double* ehvi, T* grad, int* best,
                 hipStream_t s) {
  const dim3 grid((unsigned)((m + EHVI_WAVES - 1) / EHVI_WAVES)), block(64 * EHVI_WAVES);
  if (ns <= EHVI_LDS_STRIPS)
    hipLaunchKernelGGL((ehvi_kernel<T, true>), grid, block, ehvi_lds_bytes(ns), s, mean1, var1, dmean1, dvar1, mean2, var2, dmean2, dvar2,
                       m, d, thr, ns, want_grad, ehvi, grad);
  else
    hipLaunchKernelGGL((ehvi_kernel<T, false>), grid, block, 0, s, mean1, var1, dmean1, dvar1, mean2, var2, dmean2, dvar2, m, d, thr, ns,
                       want_grad, ehvi, grad);
  launch_argmax_last(ehvi, m, best, s);
}
template void launch_ehvi<double>(const double*, const double*, const double*, const double*, const double*, const double*, const double*,
                                  const double*, int, int, const double*, int, int, double*, double*, int*, hipStream_t);
template void launch_ehvi<float>(const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                                 const float*, int, int, const double*, int, int, double*, float*, int*, hipStream_t);

// =================================================================================================================
// expected hypervolume improvement of M = 2 .. 4 independent objectives (hbegp.cpp: model_ehvi_nd).  The host
// splits the part of (-inf, r) that no front point weakly dominates into disjoint boxes [l_j, u_j), every l_jk and u_jk one of
// objective k's thresholds (entry 0 = -inf, then the front's distinct coordinates, then r_k).  With ehvi_g's G, Phi, phi,
//   EHVI = sum_j prod_k dG_jk,   dG_jk = G_k(u_jk) - G_k(l_jk),   G_k(-inf) = 0,
//   d/dmu_k = -sum_j [Phi_k(u) - Phi_k(l)] prod_{i != k} dG_ji,   d/dsigma_k = sum_j [phi_k(u) - phi_k(l)] prod_{i != k} dG_ji.
// One WAVE per candidate.  Phase A: the lanes run over objective k's thresholds and store ehvi_g(thr, mu_k, sigma_k) -- all of the
// call's erfc and exp -- into the candidate's table (entry 0 of every objective is (0, 0, 0)).  Phase B: lane l takes the boxes
// l, l + 64, .. in ascending order, looks its 2 M entries up, and adds into 1 + 2 M sums: the value takes max(dG, 0) (G is monotone:
// a negative difference is rounding), the products of the partials the differences as they are, every product in ascending k.  The
// sums go through wave_xor_sum; lane k < d forms grad[j][k] by the chain rule as ehvi_kernel does.  fp64 for both element types, the
// 1 + 2 M sums with or without a gradient: a candidate's bits depend on its own posteriors, the thresholds and the boxes only.
// LDS = true: the table is this wave's slice of the dynamic LDS (blockDim.x / 64 candidates per workgroup: EHVI_ND_WAVES, or one
// with the whole LDS); false: its rows of `scratch`.  Every wave reaches the one barrier between the phases (a wave past m only
// waits there); the box indices are read by every wave and stay in the L2.
// =================================================================================================================
template <typename T, int M, bool LDS>
__global__ void __launch_bounds__(64 * EHVI_ND_WAVES) ehvi_nd_kernel(const CeiArgs<T> a, int m, int d, const double* __restrict__ thr,
                                                                     const int* __restrict__ boxes, const EhviNdGeom g, double* scratch,
                                                                     int want_grad, double* __restrict__ ehvi, T* __restrict__ grad) {
  extern __shared__ __align__(16) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = j < m;
  const int jj = live ? j : 0;
  double* tab = LDS ? reinterpret_cast<double*>(smem_raw) + 3 * (size_t)g.nt * wave : scratch + 3 * (size_t)g.nt * jj;
  double mu[M], sd[M];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < M; ++k) {
    mu[k] = (double)a.mean[k][jj];
    const double v = (double)a.var[k][jj];
    sd[k] = sqrt(v);
    bad = bad || (mu[k] != mu[k]) || (v != v);
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double* t = thr + g.off[k];
      double* e = tab + 3 * (size_t)g.off[k];
      for (int i = lane; i < g.T[k]; i += 64) {
        EhviG r = {0.0, 0.0, 0.0};
        if (i > 0) r = ehvi_g(t[i], mu[k], sd[k]);
        e[3 * i] = r.g;
        e[3 * i + 1] = r.cdf;
        e[3 * i + 2] = r.pdf;
      }
    }
  }
  __syncthreads();
  if (!live) return;  // whole waves leave, behind the only barrier
  double s[1 + 2 * M];
#pragma unroll
  for (int q = 0; q < 1 + 2 * M; ++q) s[q] = 0.0;
  for (int b = lane; b < g.n_boxes; b += 64) {
    const int* bx = boxes + (size_t)b * (2 * M);
    double dg[M], dc[M], dp[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double* lo = tab + 3 * (size_t)bx[2 * k];
      const double* up = tab + 3 * (size_t)bx[2 * k + 1];
      dg[k] = up[0] - lo[0];
      dc[k] = lo[1] - up[1];  // d dG / d mu
      dp[k] = up[2] - lo[2];  // d dG / d sigma
    }
    double v = fmax(dg[0], 0.0);
#pragma unroll
    for (int k = 1; k < M; ++k) v *= fmax(dg[k], 0.0);
    s[0] += v;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      double others = 1.0;
#pragma unroll
      for (int i = 0; i < M; ++i)
        if (i != k) others *= dg[i];
      s[1 + 2 * k] += dc[k] * others;
      s[2 + 2 * k] += dp[k] * others;
    }
  }
#pragma unroll
  for (int q = 0; q < 1 + 2 * M; ++q) s[q] = wave_xor_sum(s[q]);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (lane == 0) ehvi[j] = bad ? nan : s[0];
  if (want_grad && lane < d) {
    const size_t e = (size_t)j * d + lane;
    double gr = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double ds = sd[k] > 2.220446049250313e-16 ? (double)a.dvar[k][e] / (2.0 * sd[k]) : 0.0;
      gr += s[1 + 2 * k] * (double)a.dmean[k][e];
      gr += s[2 + 2 * k] * ds;
    }
    grad[e] = bad ? (T)nan : (T)gr;
  }
}

template <typename T, int M>
static void launch_ehvi_nd_m(const CeiArgs<T>& a, int m, int d, const double* thr, const int* boxes, const EhviNdGeom& g, double* scratch,
                             int want_grad, double* ehvi, T* grad, hipStream_t s) {
  if (g.nt <= EHVI_ND_LDS4_ENTRIES) {
    const dim3 grid((unsigned)((m + EHVI_ND_WAVES - 1) / EHVI_ND_WAVES)), block(64 * EHVI_ND_WAVES);
    hipLaunchKernelGGL((ehvi_nd_kernel<T, M, true>), grid, block, ehvi_nd_lds_bytes(g.nt, EHVI_ND_WAVES), s, a, m, d, thr, boxes, g, nullptr,
                       want_grad, ehvi, grad);
  } else if (g.nt <= EHVI_ND_LDS1_ENTRIES) {
    hipLaunchKernelGGL((ehvi_nd_kernel<T, M, true>), dim3((unsigned)m), dim3(64), ehvi_nd_lds_bytes(g.nt, 1), s, a, m, d, thr, boxes, g,
                       nullptr, want_grad, ehvi, grad);
  } else {
    const dim3 grid((unsigned)((m + EHVI_ND_WAVES - 1) / EHVI_ND_WAVES)), block(64 * EHVI_ND_WAVES);
    hipLaunchKernelGGL((ehvi_nd_kernel<T, M, false>), grid, block, 0, s, a, m, d, thr, boxes, g, scratch, want_grad, ehvi, grad);
  }
}
template <typename T>
void launch_ehvi_nd(const CeiArgs<T>& a, int m, int d, const double* thr, const int* boxes, const EhviNdGeom& g, double* scratch,
                    int want_grad, double* ehvi, T* grad, int* best, hipStream_t s) {
  if (g.n_obj == 2) launch_ehvi_nd_m<T, 2>(a, m, d, thr, boxes, g, scratch, want_grad, ehvi, grad, s);
  else if (g.n_obj == 3) launch_ehvi_nd_m<T, 3>(a, m, d, thr, boxes, g, scratch, want_grad, ehvi, grad, s);
  else launch_ehvi_nd_m<T, 4>(a, m, d, thr, boxes, g, scratch, want_grad, ehvi, grad, s);
  launch_argmax_last(ehvi, m, best, s);
}
template void launch_ehvi_nd<double>(const CeiArgs<double>&, int, int, const double*, const int*, const EhviNdGeom&, double*, int, double*,
                                     double*, int*, hipStream_t);
template void launch_ehvi_nd<float>(const CeiArgs<float>&, int, int, const double*, const int*, const EhviNdGeom&, double*, int, double*,
                                    float*, int*, hipStream_t);

// =================================================================================================================
// constrained expected improvement over K = 1 + C independent models (hbegp.cpp: model_constrained_ei):
//   cEI = EI_0 prod_{k=1..C} F_k,   EI_0 = G_0(fmin) (ehvi_g's G; 1 for fmin = +inf),   F_k = Phi((t_k - mu_k) / sigma_k).
// One WAVE per candidate, CEI_WAVES candidates per workgroup.  Lane k < K evaluates ehvi_g for model k once and keeps its factor
// f_k (EI_0 or F_k) with the factor's partials w.r.t. mu_k and sigma_k:
//   dEI/dmu = -Phi(z), dEI/dsigma = phi(z);   dF/dmu = -phi(z) / sigma, dF/dsigma = -z phi(z) / sigma   (all 0 for sigma = 0 but
//   dEI/dmu = -[fmin > mu]).
// Every lane then reads f_1 .. f_C from the lanes that hold them and forms, in the same fixed order, pof = f_1 f_2 .. f_C
// (ascending), the prefix product of the factors below its own index (ascending) and the suffix product of those above
// (descending): lane k's partials get the weight EI_0 (prefix suffix) -- never pof / f_k, so f_k = 0 gives a finite gradient -- and
// lane 0's get pof.  The lanes then stride over the features, adding the K models' chain-rule terms in ascending k
// (dsigma = dvar / (2 sigma), 0 for sigma = 0).  All of it in fp64 for both element types, with or without a gradient, no LDS and
// no atomics: a candidate's bits depend on nothing but its own posteriors and the thresholds.  A NaN in any model's posterior
// gives NaN in the candidate's cei, ei, pof and gradient row.
// =================================================================================================================
constexpr int CEI_WAVES = 4;

template <typename T>
__global__ void __launch_bounds__(64 * CEI_WAVES) cei_kernel(const CeiArgs<T> a, int m, int d, int want_grad, double* __restrict__ cei,
                                                             double* __restrict__ ei, double* __restrict__ pof, T* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * CEI_WAVES + (threadIdx.x >> 6);
  if (j >= m) return;  // whole waves leave: every lane of a wave that stays takes part in the shuffles
  const int K = a.K;
  double f = 1.0, pm = 0.0, ps = 0.0, sd = 0.0;  // model `lane`: its factor, the factor's partials w.r.t. mu and sigma, sigma
  bool bad = false;
  if (lane < K) {
    const double mu = (double)a.mean[lane][j], v = (double)a.var[lane][j], t = a.thr[lane];
    sd = sqrt(v);
    bad = (mu != mu) || (v != v);
    const EhviG g = ehvi_g(t, mu, sd);
    if (lane == 0) {
      if (t < __longlong_as_double(0x7ff0000000000000LL)) {  // fmin = +inf: EI counts as 1, its partials as 0
        f = g.g;
        pm = -g.cdf;
        ps = g.pdf;
      }
    } else {
      f = g.cdf;
      if (sd > 2.220446049250313e-16) {
        const double z = (t - mu) / sd;
        pm = -g.pdf / sd;
        ps = -z * g.pdf / sd;
      }
    }
  }
  const bool anybad = __any(bad) != 0;
  const double e = __shfl(f, 0, 64);
  double all = 1.0, pre = 1.0, suf = 1.0;
  for (int k = 1; k < K; ++k) {
    const double fk = __shfl(f, k, 64);
    all *= fk;
    if (k < lane) pre *= fk;
  }
  for (int k = K - 1; k >= 1; --k) {
    const double fk = __shfl(f, k, 64);
    if (k > lane) suf *= fk;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (lane == 0) {
    cei[j] = anybad ? nan : e * all;
    if (ei) ei[j] = anybad ? nan : e;
    if (pof) pof[j] = anybad ? nan : all;
  }
  if (!want_grad) return;
  const double w = lane == 0 ? all : e * (pre * suf);
  const double cm = w * pm, cs = w * ps;  // d cei / d mu_lane, d cei / d sigma_lane
  for (int base = 0; base < d; base += 64) {  // a uniform trip count: every lane takes part in the shuffles
    const int i = base + lane;
    const bool on = i < d;
    const size_t x = (size_t)j * d + (on ? i : 0);
    double g = 0.0;
    for (int k = 0; k < K; ++k) {
      const double cmk = __shfl(cm, k, 64), csk = __shfl(cs, k, 64), sdk = __shfl(sd, k, 64);
      if (on) {
        const double ds = sdk > 2.220446049250313e-16 ? (double)a.dvar[k][x] / (2.0 * sdk) : 0.0;
        g += cmk * (double)a.dmean[k][x] + csk * ds;
      }
    }
    if (on) grad[x] = anybad ? (T)nan : (T)g;
  }
}

template <typename T>
void launch_cei(const CeiArgs<T>& a, int m, int d, int want_grad, double* cei, double* ei, double* pof, T* grad, int* best,
                hipStream_t s) {
  const dim3 grid((unsigned)((m + CEI_WAVES - 1) / CEI_WAVES)), block(64 * CEI_WAVES);
  hipLaunchKernelGGL((cei_kernel<T>), grid, block, 0, s, a, m, d, want_grad, cei, ei, pof, grad);
  launch_argmax_last(cei, m, best, s);
}
template void launch_cei<double>(const CeiArgs<double>&, int, int, int, double*, double*, double*, double*, int*, hipStream_t);
template void launch_cei<float>(const CeiArgs<float>&, int, int, int, double*, double*, double*, float*, int*, hipStream_t);

// =================================================================================================================
// log-space constrained expected improvement (hbegp.cpp: model_constrained_ei with log_space):
//   lcei = lei + lpof,   lei = log sigma_0 + log h(z_0) (0 for fmin = +inf),   lpof = sum_{k=1..C} log Phi(z_k)   (ascending k).
// cei_kernel's shape: one WAVE per candidate, lane k < K evaluates lcei_term for model k once -- its log-term and the term's
// partials w.r.t. mu_k and sigma_k, which ARE lcei's (the log of a product is a sum: no prefix or suffix products) -- the K terms
// are read from the lanes that hold them and added in ascending k, then the lanes stride over the features as cei_kernel does.
// All of it in fp64 for both element types, with or without a gradient, no LDS and no atomics.
//
// lcei_term works through the Mills ratio for z = -a <= -1: u = Phi(-a) / phi(a) = sqrt(pi/2) erfcx(a / sqrt 2) and
// b = h(-a) / phi(a) = 1 - a u, so that
//   log h = -a^2/2 - log sqrt(2 pi) + log b,   log Phi = -a^2/2 - log sqrt(2 pi) + log u,   Phi/h = u/b,  phi/h = 1/b,  phi/Phi = 1/u
// and nothing that underflows is ever formed.  1 - a u cancels about a^2 eps; from a = LCEI_SERIES_A on both come from the
// asymptotic series in x = 1/a^2 (ten terms: the first omitted one is below 2e-18 at a = 25)
//   a u = 1 - x + 3 x^2 - 15 x^3 + ..,     b = x (1 - 3 x + 15 x^2 - 105 x^3 + ..).
// Above z = -1 the direct forms hold: h = phi(a) - a Phi(-a) for z = -a <= 0 and z + h(-z) above, log Phi = log(Phi(z)) up to
// z = 0 and log1p(-Phi(-z)) above.  z is clamped to +-1.7e308 (an overflowing quotient stays a number).
// =================================================================================================================
constexpr double LCEI_SERIES_A = 25.0;

struct LceiTerm {
  double v, pm, ps;  // the log-term and its partials w.r.t. mu and sigma
};
// The Mills-ratio pieces at a >= 1 for lcei_term and mes_term: au = a u and bx = b / x.  Below the switch point au comes from erfcx
// and b itself sits in bx with x = 1; from there on x = 1 / a^2 and both come from the series.
struct MillsPieces {
  double x, au, bx;
};
__device__ __forceinline__ MillsPieces mills_pieces(double a) {
  MillsPieces r;
  r.x = 1.0;
  if (a < LCEI_SERIES_A) {
    r.au = a * (1.2533141373155003 * erfcx(a / 1.4142135623730951));
    r.bx = 1.0 - r.au;
  } else {
    r.x = 1.0 / a / a;  // (a * a may overflow where 1 / a / a only underflows)
    const double x = r.x;
    r.au = 1.0 + x * (-1.0 + x * (3.0 + x * (-15.0 + x * (105.0 + x * (-945.0 + x * (10395.0 + x * (-135135.0 + x * (2027025.0 + x * -34459425.0))))))));
    r.bx = 1.0 + x * (-3.0 + x * (15.0 + x * (-105.0 + x * (945.0 + x * (-10395.0 + x * (135135.0 + x * (-2027025.0 + x * (34459425.0 + x * -654729075.0))))))));
  }
  return r;
}
// not inlined: erfcx's, log's and exp's fp64 coefficients, once per lane
__device__ __noinline__ LceiTerm lcei_term(double t, double mu, double sd, int objective) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  LceiTerm r = {0.0, 0.0, 0.0};
  if (objective && !(t < inf)) return r;  // fmin = +inf: the objective drops out
  if (!(sd > 2.220446049250313e-16)) {    // sigma = 0
    if (objective) {
      const double gap = t - mu;
      r.v = log(fmax(gap, 0.0));
      r.pm = gap > 0.0 ? -1.0 / gap : 0.0;
    } else {
      r.v = t > mu ? 0.0 : -inf;
    }
    return r;
  }
  const double z = fmin(fmax((t - mu) / sd, -1.7e308), 1.7e308);
  double lf, rr, qq;  // log h or log Phi;  Phi/h or phi/Phi;  phi/h or z phi/Phi
  if (z > -1.0) {
    const double az = fabs(z);
    const double cl = 0.5 * erfc(az / 1.4142135623730951);            // Phi(-|z|)
    const double pdf = exp(-0.5 * az * az) / 2.5066282746310002;      // phi(z)
    const double cdf = z > 0.0 ? 1.0 - cl : cl;
    if (objective) {
      const double tail = pdf - az * cl;                               // h(-|z|) > 0: |z| < 1 below 0, and z is added above
      const double h = z > 0.0 ? z + tail : tail;
      lf = log(h);
      rr = cdf / h;
      qq = pdf / h;
    } else {
      lf = z > 0.0 ? log1p(-cl) : log(cl);
      rr = pdf / cdf;
      qq = pdf > 0.0 ? z * rr : 0.0;                                   // (z = 1.7e308 times an underflowed phi is 0)
    }
  } else {
    const double a = -z;
    const MillsPieces q = mills_pieces(a);
    const double x = q.x, au = q.au, bx = q.bx;  // u = au / a, b = x bx
    const double base = -0.5 * a * a - 0.91893853320467274;
    if (objective) {
      lf = base + (log(bx) + log(x));
      rr = a < LCEI_SERIES_A ? au / a / bx : a * (au / bx);  // u / b
      qq = a < LCEI_SERIES_A ? 1.0 / bx : a * (a / bx);      // 1 / b
    } else {
      lf = base + (log(au) - log(a));
      rr = a / au;           // 1 / u
      qq = -a * rr;          // z / u
    }
  }
  if (objective) {
    r.v = log(sd) + lf;
    r.pm = -rr / sd;
    r.ps = qq / sd;
  } else {
    r.v = lf;
    r.pm = -rr / sd;
    r.ps = -qq / sd;
  }
  return r;
}

template <typename T>
__global__ void __launch_bounds__(64 * CEI_WAVES) lcei_kernel(const CeiArgs<T> a, int m, int d, int want_grad, double* __restrict__ lcei,
                                                              double* __restrict__ lei, double* __restrict__ lpof, T* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * CEI_WAVES + (threadIdx.x >> 6);
  if (j >= m) return;  // whole waves leave: every lane of a wave that stays takes part in the shuffles
  const int K = a.K;
  double v = 0.0, cm = 0.0, cs = 0.0, sd = 0.0;  // model `lane`: its log-term, d lcei / d mu_lane, d lcei / d sigma_lane, sigma
  bool bad = false;
  if (lane < K) {
    const double mu = (double)a.mean[lane][j], var = (double)a.var[lane][j];
    sd = sqrt(var);
    bad = (mu != mu) || (var != var);
    const LceiTerm g = lcei_term(a.thr[lane], mu, sd, lane == 0);
    v = g.v;
    cm = g.pm;
    cs = g.ps;
  }
  const bool anybad = __any(bad) != 0;
  const double e = __shfl(v, 0, 64);
  double all = 0.0;
  for (int k = 1; k < K; ++k) all += __shfl(v, k, 64);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (lane == 0) {
    lcei[j] = anybad ? nan : e + all;
    if (lei) lei[j] = anybad ? nan : e;
    if (lpof) lpof[j] = anybad ? nan : all;
  }
  if (!want_grad) return;
  for (int base = 0; base < d; base += 64) {  // a uniform trip count: every lane takes part in the shuffles
    const int i = base + lane;
    const bool on = i < d;
    const size_t x = (size_t)j * d + (on ? i : 0);
    double g = 0.0;
    for (int k = 0; k < K; ++k) {
      const double cmk = __shfl(cm, k, 64), csk = __shfl(cs, k, 64), sdk = __shfl(sd, k, 64);
      if (on) {
        const double ds = sdk > 2.220446049250313e-16 ? (double)a.dvar[k][x] / (2.0 * sdk) : 0.0;
        g += cmk * (double)a.dmean[k][x] + csk * ds;
      }
    }
    if (on) grad[x] = anybad ? (T)nan : (T)g;
  }
}

template <typename T>
void launch_lcei(const CeiArgs<T>& a, int m, int d, int want_grad, double* lcei, double* lei, double* lpof, T* grad, int* best,
                 hipStream_t s) {
  const dim3 grid((unsigned)((m + CEI_WAVES - 1) / CEI_WAVES)), block(64 * CEI_WAVES);
  hipLaunchKernelGGL((lcei_kernel<T>), grid, block, 0, s, a, m, d, want_grad, lcei, lei, lpof, grad);
  launch_argmax_last(lcei, m, best, s);
}
template void launch_lcei<double>(const CeiArgs<double>&, int, int, int, double*, double*, double*, double*, int*, hipStream_t);
template void launch_lcei<float>(const CeiArgs<float>&, int, int, int, double*, double*, double*, float*, int*, hipStream_t);

// =================================================================================================================
// max-value entropy search over ONE model and S sampled minimum values y*_s (hbegp.cpp: model_mes):
//   mes = (1/S) sum_s t(gamma_s),   gamma_s = (mu - y*_s) / sigma,   t(g) = g lambda(g) / 2 - log Phi(g),   lambda = phi / Phi,
//   t'(g) = -(lambda / 2) (1 + g^2 + g lambda),   d mes / d mu = (1/S) sum t' / sigma,   d mes / d sigma = -(1/S) sum g t' / sigma.
// One WAVE per candidate, CEI_WAVES candidates per workgroup; y* is staged once per workgroup in the LDS when S fits
// (S <= MES_LDS_SAMPLES: every call through the C ABI), else read from global memory.  Lane l evaluates mes_term for
// s = l, l + 64, .. in ascending s and keeps three partial sums (t, t', g t'), which go through wave_xor_sum's fixed butterfly and
// are then scaled by 1/S; every lane holds the same three totals, so the lanes stride over the features without another shuffle.
// All of it in fp64 for both element types, with or without a gradient, no atomics: a candidate's bits depend on nothing but its
// own posterior and the y* array in the order given.  sigma = 0: mes = 0 with a zero gradient.  A NaN in the posterior gives NaN
// in the candidate's mes and gradient row.
//
// mes_term has lcei_term's branch points.  For g > -1 the direct forms (g lambda and t' count as 0 where phi has underflowed).
// For g = -a <= -1 both terms of t grow like a^2 / 2 and cancel to O(log a); with au = a u (u the Mills ratio, as in lcei_term) and
// b = 1 - au:  w = a^2 b / au = -g (g + lambda),   t = -w / 2 + log sqrt(2 pi) + (log a - log au),   t' = -(a / au) (1 - w) / 2.
// From a = LCEI_SERIES_A on, au and bx = b / x (x = 1 / a^2) come from lcei_term's ten-term series and (au - bx) / x from the
// term-wise difference of the two coefficient lists (the constant terms cancel exactly):  w = bx / au,
// 1 - w = x ((au - bx) / x) / au; a * a is never formed.  g is clamped to +-1.7e308 by the caller.
// =================================================================================================================
constexpr int MES_LDS_SAMPLES = 1024;

struct MesTerm {
  double t, dt;  // t(g) and t'(g)
};
// not inlined: erfcx's, erfc's, log's and exp's fp64 coefficients, once per lane
__device__ __noinline__ MesTerm mes_term(double g) {
  MesTerm r = {0.0, 0.0};
  if (g > -1.0) {
    const double az = fabs(g);
    const double cl = 0.5 * erfc(az / 1.4142135623730951);        // Phi(-|g|)
    const double pdf = exp(-0.5 * az * az) / 2.5066282746310002;  // phi(g)
    const double cdf = g > 0.0 ? 1.0 - cl : cl;
    const double lam = pdf / cdf;
    const double lphi = g > 0.0 ? log1p(-cl) : log(cl);
    const double gl = pdf > 0.0 ? g * lam : 0.0;                  // (g = 1.7e308 times an underflowed phi is 0)
    r.t = 0.5 * gl - lphi;
    r.dt = pdf > 0.0 ? -0.5 * lam * (1.0 + g * g + gl) : 0.0;
  } else {
    const double a = -g;
    const MillsPieces q = mills_pieces(a);
    const double x = q.x, au = q.au, bx = q.bx;
    if (a < LCEI_SERIES_A) {
      const double w = a * a * bx / au;  // (bx = 1 - au here)
      r.t = -0.5 * w + 0.91893853320467274 + (log(a) - log(au));
      r.dt = -(a / au) * (1.0 - w) / 2.0;
    } else {
      const double dq = 2.0 + x * (-12.0 + x * (90.0 + x * (-840.0 + x * (9450.0 + x * (-124740.0 + x * (1891890.0 + x * (-32432400.0 + x * 620269650.0)))))));  // (au - bx) / x
      r.t = -bx / (2.0 * au) + 0.91893853320467274 + (log(a) - log(au));
      r.dt = -(a / au) * (x * dq / au) / 2.0;
    }
  }
  return r;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(64 * CEI_WAVES) mes_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                             const T* __restrict__ dmean, const T* __restrict__ dvar, int m, int d,
                                                             const double* __restrict__ ystar, int S, int want_grad,
                                                             double* __restrict__ mes, T* __restrict__ grad) {
  __shared__ double st[LDS ? MES_LDS_SAMPLES : 1];
  const double* ys = ystar;
  if (LDS) {
    for (int i = threadIdx.x; i < S; i += 64 * CEI_WAVES) st[i] = ystar[i];
    __syncthreads();
    ys = st;
  }
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * CEI_WAVES + (threadIdx.x >> 6);
  if (j >= m) return;  // whole waves leave, behind the only barrier
  const double mu = (double)mean[j], v = (double)var[j];
  const double sd = sqrt(v);
  const bool bad = (mu != mu) || (v != v);
  const bool live = sd > 2.220446049250313e-16;  // wave-uniform
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;           // this lane's sums of t, t' and g t'
  if (live)
    for (int base = 0; base < S; base += 64) {  // a uniform trip count, ascending s
      const int i = base + lane;
      if (i < S) {
        const double g = fmin(fmax((mu - ys[i]) / sd, -1.7e308), 1.7e308);
        const MesTerm r = mes_term(g);
        s0 += r.t;
        s1 += r.dt;
        s2 += g * r.dt;
      }
    }
  s0 = wave_xor_sum(s0);  // the whole wave is here: `live` is uniform and the loop has ended for every lane
  s1 = wave_xor_sum(s1);
  s2 = wave_xor_sum(s2);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (lane == 0) mes[j] = bad ? nan : s0 / (double)S;
  if (!want_grad) return;
  const double cm = live ? s1 / (double)S / sd : 0.0;   // d mes / d mu
  const double cs = live ? -s2 / (double)S / sd : 0.0;  // d mes / d sigma
  for (int i = lane; i < d; i += 64) {
    const size_t x = (size_t)j * d + i;
    const double ds = live ? (double)dvar[x] / (2.0 * sd) : 0.0;
    const double gx = cm * (double)dmean[x] + cs * ds;
    grad[x] = bad ? (T)nan : (T)gx;
  }
}

template <typename T>
void launch_mes(const T* mean, const T* var, const T* dmean, const T* dvar, int m, int d, const double* ystar, int S, int want_grad,
                double* mes, T* grad, int* best, hipStream_t s) {
  const dim3 grid((unsigned)((m + CEI_WAVES - 1) / CEI_WAVES)), block(64 * CEI_WAVES);
  if (S <= MES_LDS_SAMPLES)
    hipLaunchKernelGGL((mes_kernel<T, true>), grid, block, 0, s, mean, var, dmean, dvar, m, d, ystar, S, want_grad, mes, grad);
  else
    hipLaunchKernelGGL((mes_kernel<T, false>), grid, block, 0, s, mean, var, dmean, dvar, m, d, ystar, S, want_grad, mes, grad);
  launch_argmax_last(mes, m, best, s);
}
template void launch_mes<double>(const double*, const double*, const double*, const double*, int, int, const double*, int, int, double*,
                                 double*, int*, hipStream_t);
template void launch_mes<float>(const float*, const float*, const float*, const float*, int, int, const double*, int, int, double*,
                                float*, int*, hipStream_t);

// =================================================================================================================
// the confidence bound of ONE model (hbegp.cpp: model_cb):
//   cb = mu + kappa sigma,   grad[i] = dmean[i] + kappa (dvar[i] / (2 sigma)),   sigma = sqrt(var)
// The sigma term is dropped -- never divided -- where !(sigma > 2.220446049250313e-16) and where kappa = 0: cb = mu widened, grad =
// dmean's bits.  There is no sum over anything, so a wave per candidate (mes_kernel's mapping) would leave 64 - d lanes idle: a row
// gets L = 2^shift lanes, the smallest power of two >= d (1 without a gradient), and a workgroup of CB_THREADS lanes covers
// CB_THREADS / L consecutive rows -- lane (r, i) reads element r d + i of dmean and dvar, so a wave's loads cover one contiguous
// range, and at least half the lanes work.  Every lane of a row reads the row's mu and var (one cache line for the group) and forms
// sigma itself; lane i = 0 stores cb.  Every operation is a single rounded fp64 one (no contraction), the same with and without a
// gradient: a row's bits depend on its own (mu, var, dmean, dvar) and kappa alone.  A NaN in mu or var gives NaN in cb and the row.
// =================================================================================================================
constexpr int CB_THREADS = 256;

template <typename T>
__global__ void __launch_bounds__(CB_THREADS) cb_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                        const T* __restrict__ dmean, const T* __restrict__ dvar, int m, int d, int shift,
                                                        double kappa, int want_grad, double* __restrict__ cb, T* __restrict__ grad) {
#pragma clang fp contract(off)  // every product and sum below is rounded on its own (HIP's default would fuse them)
  const int L = 1 << shift;
  const long long j = (long long)blockIdx.x * (CB_THREADS >> shift) + (threadIdx.x >> shift);
  const int i0 = threadIdx.x & (L - 1);
  if (j >= m) return;
  const double mu = (double)mean[j], v = (double)var[j];
  const double sd = sqrt(v);
  const bool bad = (mu != mu) || (v != v);
  const bool live = sd > 2.220446049250313e-16 && kappa != 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (i0 == 0) cb[j] = bad ? nan : (live ? mu + kappa * sd : mu);
  if (!want_grad) return;
  const double two_sd = 2.0 * sd;
  for (int i = i0; i < d; i += L) {
    const size_t x = (size_t)j * d + i;
    const double dm = (double)dmean[x];
    const double g = live ? dm + kappa * ((double)dvar[x] / two_sd) : dm;
    grad[x] = bad ? (T)nan : (T)g;
  }
}

// The arg-min of the confidence bound: best = the FIRST index of the minimum of v[0 .. m) through argmax_last_kernel's fixed LDS
// tree with the order turned round; a NaN never wins, -1 where no entry is a number.  First, because the reference replaces its
// suggestion only on a strictly lower bound.
__global__ void __launch_bounds__(BSEL_THREADS) argmin_first_kernel(const double* __restrict__ v, int m, int* __restrict__ res) {
  __shared__ double sv[BSEL_THREADS];
  __shared__ int si[BSEL_THREADS];
  const int tid = threadIdx.x;
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < m; i += BSEL_THREADS) {
    const double e = v[i];
    if (e == e && (bi < 0 || e < best)) { best = e; bi = i; }  // ascending i: an equal value stays at the earlier index
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
#pragma unroll 1
  for (int w = BSEL_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = sv[tid + w];
      const int oi = si[tid + w];
      if (oi >= 0 && (si[tid] < 0 || o < sv[tid] || (o == sv[tid] && oi < si[tid]))) { sv[tid] = o; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) res[0] = si[0];
}

template <typename T>
void launch_cb(const T* mean, const T* var, const T* dmean, const T* dvar, int m, int d, double kappa, int want_grad, double* cb, T* grad,
               int* best, hipStream_t s) {
  int shift = 0;
  if (want_grad)
    while ((1 << shift) < d && (1 << shift) < 64) ++shift;
  const int rows = CB_THREADS >> shift;
  hipLaunchKernelGGL((cb_kernel<T>), dim3((unsigned)((m + rows - 1) / rows)), dim3(CB_THREADS), 0, s, mean, var, dmean, dvar, m, d, shift,
                     kappa, want_grad, cb, grad);
  hipLaunchKernelGGL(argmin_first_kernel, dim3(1), dim3(BSEL_THREADS), 0, s, cb, m, best);
}
template void launch_cb<double>(const double*, const double*, const double*, const double*, int, int, double, int, double*, double*, int*,
                                hipStream_t);
template void launch_cb<float>(const float*, const float*, const float*, const float*, int, int, double, int, double*, float*, int*,
                               hipStream_t);

// Per-device one-time setup: kernels that use more than 64 KiB of dynamic LDS need the attribute raised.  Called from
// hbegp_ctx_create() for every device, before any stream capture.
static void init_dag_kernels();  // dag_kernel.inc.hpp (end of this file)
static void set_lds_attr(const void* fn, int bytes, const char* what) {
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
template <typename T, int TILE>
static void init_gemm_attr() {
  set_lds_attr(reinterpret_cast<const void*>(&gemm_kernel<T, TILE>), 163840, "gemm_kernel: dynamic LDS limit");
}
// Throws std::runtime_error (caught in hbegp_ctx_create): a kernel that cannot get its LDS would be rejected at every launch.
void init_kernels() {
  init_gemm_attr<double, 128>(); init_gemm_attr<double, 64>(); init_gemm_attr<double, 32>();
  init_gemm_attr<float, 128>(); init_gemm_attr<float, 64>(); init_gemm_attr<float, 32>();
  set_lds_attr(reinterpret_cast<const void*>(&leaf_kernel<double, double>), (int)LeafGeom<double>::LDS_BYTES, "leaf_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&leaf_kernel<double, float>), (int)LeafGeom<double>::LDS_BYTES, "leaf_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&leaf_keep_kernel<double, double>), (int)LeafGeom<double>::LDS_BYTES, "leaf_keep_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&leaf_keep_kernel<double, float>), (int)LeafGeom<double>::LDS_BYTES, "leaf_keep_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&qei_batch_kernel<double>), (int)qei_lds_bytes(QEI_MAXQ, MAXD), "qei_batch_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&qei_batch_kernel<float>), (int)qei_lds_bytes(QEI_MAXQ, MAXD), "qei_batch_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_group_kernel<double>), (int)lgo_group_lds_bytes(LGO_MAX_GROUP), "lgo_group_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_group_kernel<float>), (int)lgo_group_lds_bytes(LGO_MAX_GROUP), "lgo_group_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_gram_kernel<double>), (int)lgo_gram_lds_bytes(LGO_MAX_GROUP), "lgo_gram_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_gram_kernel<float>), (int)lgo_gram_lds_bytes(LGO_MAX_GROUP), "lgo_gram_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_uy_kernel<double>), (int)lgo_uy_lds_bytes(false), "lgo_uy_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&lgo_uy_kernel<float>), (int)lgo_uy_lds_bytes(true), "lgo_uy_kernel<f32>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&kg_kernel<double>), (int)kg_lds_bytes(KG_LDS_ROWS), "kg_kernel<f64>: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&kg_kernel<float>), (int)kg_lds_bytes(KG_LDS_ROWS), "kg_kernel<f32>: dynamic LDS limit");
  {
    const int nd = (int)ehvi_nd_lds_bytes(EHVI_ND_LDS1_ENTRIES, 1);
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<double, 2, true>), nd, "ehvi_nd_kernel<f64, 2>: dynamic LDS limit");
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<double, 3, true>), nd, "ehvi_nd_kernel<f64, 3>: dynamic LDS limit");
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<double, 4, true>), nd, "ehvi_nd_kernel<f64, 4>: dynamic LDS limit");
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<float, 2, true>), nd, "ehvi_nd_kernel<f32, 2>: dynamic LDS limit");
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<float, 3, true>), nd, "ehvi_nd_kernel<f32, 3>: dynamic LDS limit");
    set_lds_attr(reinterpret_cast<const void*>(&ehvi_nd_kernel<float, 4, true>), nd, "ehvi_nd_kernel<f32, 4>: dynamic LDS limit");
  }
  init_dag_kernels();
  const int lb = 163840;
  // kmat / gradtrace: 2 d 64 elements of dynamic LDS (64 KiB at d = 64 in f64) beside ~21 KiB of static LDS
  {
    const void* fns[] = {
        (const void*)&kmat_kernel<double, 0>, (const void*)&kmat_kernel<double, 1>, (const void*)&kmat_kernel<double, 3>, (const void*)&kmat_kernel<double, 5>,
        (const void*)&kmat_kernel<float, 0>, (const void*)&kmat_kernel<float, 1>, (const void*)&kmat_kernel<float, 3>, (const void*)&kmat_kernel<float, 5>,
        (const void*)&gradtrace_kernel<double, 0>, (const void*)&gradtrace_kernel<double, 1>, (const void*)&gradtrace_kernel<double, 3>, (const void*)&gradtrace_kernel<double, 5>,
        (const void*)&gradtrace_kernel<float, 0>, (const void*)&gradtrace_kernel<float, 1>, (const void*)&gradtrace_kernel<float, 3>, (const void*)&gradtrace_kernel<float, 5>};
    for (const void* fn : fns) set_lds_attr(fn, 2 * MAXD * 64 * 8, "kmat / gradtrace kernel: dynamic LDS limit");
  }
  {
    const void* fns[] = {
        (const void*)&xgrad_kernel<double, 0>, (const void*)&xgrad_kernel<double, 1>, (const void*)&xgrad_kernel<double, 3>, (const void*)&xgrad_kernel<double, 5>,
        (const void*)&xgrad_kernel<float, 0>, (const void*)&xgrad_kernel<float, 1>, (const void*)&xgrad_kernel<float, 3>, (const void*)&xgrad_kernel<float, 5>};
    for (const void* fn : fns) set_lds_attr(fn, 2 * MAXD * 64 * 8, "xgrad kernel: dynamic LDS limit");
  }
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<double, 0>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<double, 1>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<double, 3>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<double, 5>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<float, 0>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<float, 1>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<float, 3>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_eval_kernel<float, 5>), lb, "small_eval_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<double, 0>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<double, 1>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<double, 3>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<double, 5>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<float, 0>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<float, 1>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<float, 3>), lb, "small_fit_kernel: dynamic LDS limit");
  set_lds_attr(reinterpret_cast<const void*>(&small_fit_kernel<float, 5>), lb, "small_fit_kernel: dynamic LDS limit");
}

__global__ void set_info_kernel(int* info, int value) { *info = value; }
void launch_set_info(int* info, int value, hipStream_t s) { hipLaunchKernelGGL(set_info_kernel, dim3(1), dim3(1), 0, s, info, value); }

__global__ void reset_out_kernel(EvalOut* out) { poison_out(out, threadIdx.x); }
void launch_reset_out(EvalOut* out, hipStream_t s) { hipLaunchKernelGGL(reset_out_kernel, dim3(1), dim3(128), 0, s, out); }

// device result block -> pinned host block, then the evaluation's serial number behind a system-scope fence (engine.hpp)
__global__ void __launch_bounds__(128) publish_out_kernel(const EvalOut* out, EvalOut* hout, const EvalParams* __restrict__ P) {
  publish_out_in_block(out, hout, P);
}
void launch_publish_out(const EvalOut* out, EvalOut* hout, const EvalParams* P, hipStream_t s) {
  hipLaunchKernelGGL(publish_out_kernel, dim3(1), dim3(128), 0, s, out, hout, P);
}

#include "dag_kernel.inc.hpp"

}  // namespace hbegp
