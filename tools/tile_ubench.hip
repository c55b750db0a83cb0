// The 128x128 task-queue tile function alone (csrc/dag_kernel.inc.hpp: dag_gemm_tile<T, 128, 128>), one workgroup per CU, 2048
// deep, with no / 4 leading / 4 trailing half-zero stages (2 in f32) on the A side and on the B side (engine.hpp: dag_zero_halves): the plain
// wave grid, the SIMD-paired grid, and either grid with the skip.  Says what a half-zero stage really costs (the planner's model
// assumes half a stage) and that the paired grid alone loses nothing on a full tile.  DESIGN.md section 7d,
// profiles/zero_half_tile_ubench.txt.
//
// Every workgroup runs the same task on the same operands (they come out of the L2, as most of a fit's do) and stores the same
// values to the same output tile.  Times are per tile, from the 100 MHz clock inside the kernel (median over the workgroups of
// the best of `rounds` launches), and as a share of the MFMA rate at 2.4 GHz: 128 flop per cycle and CU in f64, 256 in f32.
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I csrc -o tools/tile_ubench tools/tile_ubench.hip
// Run:   tools/tile_ubench [reps per launch = 8] [rounds = 5]
#include "../csrc/kernels.hip"

#include <vector>

using namespace hbegp;

template <typename T, bool PAIRED>
__global__ void __launch_bounds__(512, 2) tile_kernel(int flags, int row0, int col0, int kbeg, int kend, T* W1, T* W2, T* out, int ld,
                                                      int reps, int zero_skip, unsigned long long* ticks) {
  extern __shared__ __align__(16) char smem_raw[];
  auto nop = []() {};
  __syncthreads();
  const unsigned long long t0 = wall_clock64();
  for (int r = 0; r < reps; ++r) {
    dag_gemm_tile<T, 128, 128, PAIRED>(flags, row0, col0, kbeg, kend, W1, W2, W1, out, ld, smem_raw, nop, nop, nullptr, zero_skip != 0);
    __syncthreads();
  }
  if (threadIdx.x == 0) ticks[blockIdx.x] = wall_clock64() - t0;
}

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
      exit(1);                                                                                \
    }                                                                                         \
  } while (0)

struct Case {
  const char* name;
  int flags, row0, col0;
};

template <typename T, bool PAIRED>
static double run(const Case& c, int depth, int ld, T* W1, T* W2, T* out, int nwg, int reps, int rounds, int zero_skip, unsigned long long* dticks) {
  const void* fn = reinterpret_cast<const void*>(&tile_kernel<T, PAIRED>);
  CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, DAG_LDS_BYTES));
  std::vector<unsigned long long> h(nwg);
  double best = 1e30;
  for (int it = 0; it <= rounds; ++it) {  // the first launch warms up
    hipLaunchKernelGGL((tile_kernel<T, PAIRED>), dim3(nwg), dim3(512), DAG_LDS_BYTES, 0, c.flags | DAGF_CKINV, c.row0, c.col0, 0, depth, W1, W2,
                       out, ld, reps, zero_skip, dticks);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), dticks, nwg * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    const double us = h[nwg / 2] / 100.0 / reps;
    if (it > 0 && us < best) best = us;
  }
  return best;
}

template <typename T>
static void sweep(const char* tname, double flop_per_cycle, int nwg, int reps, int rounds) {
  const int depth = 2048, ld = 2048, bk = dag_stage_depth(sizeof(T) == 4);
  const size_t nn = (size_t)ld * ld;
  T *W1, *W2, *out;
  unsigned long long* dticks;
  CHECK(hipMalloc(&W1, nn * sizeof(T)));
  CHECK(hipMalloc(&W2, nn * sizeof(T)));
  CHECK(hipMalloc(&out, nn * sizeof(T)));
  CHECK(hipMalloc(&dticks, nwg * sizeof(unsigned long long)));
  {  // W1 dense, W2 lower triangular (strict upper triangle zero, as the inverse factor's matrix is)
    std::vector<T> h(nn);
    for (size_t i = 0; i < nn; ++i) h[i] = (T)(((i * 2654435761u) >> 8 & 1023) / 1024.0 - 0.5);
    CHECK(hipMemcpy(W1, h.data(), nn * sizeof(T), hipMemcpyHostToDevice));
    for (int i = 0; i < ld; ++i)
      for (int j = i + 1; j < ld; ++j) h[(size_t)i * ld + j] = 0;
    CHECK(hipMemcpy(W2, h.data(), nn * sizeof(T), hipMemcpyHostToDevice));
    CHECK(hipMemset(out, 0, nn * sizeof(T)));
  }
  // 64 rows = 64 / bk stages per half: the task's origin puts exactly one half of one side above the diagonal at one end
  const int hz = 4 * bk < 64 ? 4 * bk : 64;  // contraction elements of the half-zero stages: 4 in f64, 2 in f32 (a half is 64 deep)
  const Case cases[] = {
      {"full tile (no operand in the triangular matrix)", 0, 0, 128},
      {"A side, leading half-zero stages", DAGF_ABUF | DAGF_AKM, hz - 64, 1024},
      {"A side, trailing half-zero stages", DAGF_ABUF, depth - 64 - hz, 0},
      {"B side, leading half-zero stages", DAGF_BBUF | DAGF_BKM, 1024, hz - 64},
      {"B side, trailing half-zero stages", DAGF_BBUF, 1920, depth - 64 - hz},
  };
  const double ideal_us = 128.0 * 128.0 * depth * 2.0 / flop_per_cycle / 2400.0;
  printf("%s, stage depth %d, %d stages, %d workgroups, %d tiles per launch, best of %d launches; 100 %% of the MFMA rate = %.2f us per tile\n", tname,
         bk, depth / bk, nwg, reps, rounds, ideal_us);
  double full[4] = {0, 0, 0, 0};
  for (const Case& c : cases) {
    const DagZeroHalf z = dag_zero_halves(c.flags, c.row0, c.col0, 0, depth, bk);
    int nz = 0;
    for (int side = 0; side < 2; ++side)
      for (int h = 0; h < 2; ++h) nz += z.lead[side][h] + z.trail[side][h];
    double us[4];
    us[0] = run<T, false>(c, depth, ld, W1, W2, out, nwg, reps, rounds, 0, dticks);
    us[1] = run<T, true>(c, depth, ld, W1, W2, out, nwg, reps, rounds, 0, dticks);
    us[2] = run<T, false>(c, depth, ld, W1, W2, out, nwg, reps, rounds, 1, dticks);
    us[3] = run<T, true>(c, depth, ld, W1, W2, out, nwg, reps, rounds, 1, dticks);
    if (nz == 0)
      for (int v = 0; v < 4; ++v) full[v] = us[v];
    printf("  %-50s half-zero stages %d\n", c.name, nz);
    const char* vn[4] = {"plain grid", "paired grid", "plain grid + skip", "paired grid + skip"};
    for (int v = 0; v < 4; ++v) {
      printf("    %-20s %8.2f us per tile = %5.1f %% of the MFMA rate", vn[v], us[v], 100.0 * ideal_us / us[v]);
      if (nz > 0) printf("; against the same grid without skip: %+.3f us per half-zero stage (a whole stage: %.3f us)", (us[v] - us[v & 1]) / nz, us[v & 1] * bk / depth);
      printf("\n");
    }
  }
  (void)full;
  CHECK(hipFree(W1));
  CHECK(hipFree(W2));
  CHECK(hipFree(out));
  CHECK(hipFree(dticks));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 8, rounds = argc > 2 ? atoi(argv[2]) : 5;
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int nwg = prop.multiProcessorCount;
  printf("%s, %d CUs\n", prop.name, nwg);
  sweep<double>("f64", 128.0, nwg, reps, rounds);
  sweep<float>("f32", 256.0, nwg, reps, rounds);
  return 0;
}
