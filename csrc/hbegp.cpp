// hbegp.cpp — host runtime and C ABI of the MI355X GP engine (see include/hbegp.h).
//
// Layout in HBM (per evaluation slot, all row-major with leading dimension np = n rounded up to 128):
//   W1   np x np   kernel matrix K (lower) -> trailing Schur complements / scratch during the factorisation
//   W2   np x np   X = L^-1 (lower), built block by block while the Cholesky recursion runs
//   Kinv np x np   x2 (ping-pong): K^-1 = X^T X (lower); the copy holding the best lml so far is never overwritten
//   alpha np       x2 (ping-pong)
// The padding rows/cols carry an identity block, so every kernel works on whole 128-tiles.
//
// One evaluation (lml.rs:29-79) = kmat -> chol_inv recursion (leaf + tile GEMMs) -> alpha/lml -> lauum -> gradtrace,
// captured once per slot into a hipGraph and replayed for every theta the optimiser asks for.
#include "../include/hbegp.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <queue>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "dag_plan.hpp"
#include "engine.hpp"
#include "lbfgsb.hpp"
#include "lbfgs_step.hpp"
#include "lockstep.hpp"
#include "slot_share.hpp"
#include "warp.hpp"


using namespace hbegp;

// ---------------------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error = "";
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
struct HipError {
  hipError_t e;
  const char* what;
  int line;
};
#define HIPCHECK(x)                                \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) throw HipError{_e, #x, __LINE__}; \
  } while (0)

// A rejected launch (bad configuration, LDS request refused, ...) is only reported through hipGetLastError: checked after
// every group of launches, also while a stream is being captured.
#define CHECK_LAUNCHES()                                                        \
  do {                                                                          \
    hipError_t _e = hipGetLastError();                                          \
    if (_e != hipSuccess) throw HipError{_e, "kernel launch", __LINE__};        \
  } while (0)

static int hip_fail(const HipError& he) {
  return fail(he.e == hipErrorOutOfMemory ? HBEGP_ENOMEM : HBEGP_EHIP, "HIP error %d (%s) in %s at hbegp.cpp:%d", (int)he.e,
              hipGetErrorString(he.e), he.what, he.line);
}

static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

struct hbegp_ctx {
  std::vector<int> devs;
};
static std::atomic<int> g_live_ctx{0};  // the block pool is process-global: it is trimmed when the last context goes

// ---------------------------------------------------------------------------------------------------------------
// Device-memory pool for the large work matrices (np x np).  hipMalloc/hipFree of 128 MiB blocks costs tens of
// milliseconds per fit; the caller fits one model per generation with slowly growing n, so blocks are recycled by
// exact size.  What a block holds when it is handed out: zeros if it is fresh, otherwise whatever its last owner left --
// not necessarily finite numbers (an evaluation whose factorisation failed leaves NaN in L, L^-1 and K^-1, a NaN feature
// leaves NaN in K, a model at extreme parameters a K^-1 of 1e302).  So the engine requires NOTHING of a region its owner
// never writes: every such region is either never read, or only read into a place that is itself never read (W1's strict upper
// part: the upper tiles, and the upper right quadrant of the diagonal tiles, which SYRK's C += updates in place), or it is
// cleared by the owner (W2 / Xalt: triangular GEMM operands, whose diagonal tiles are loaded whole).  The table of every block
// is DESIGN section 23; tests/test_gpu_pool_hygiene.py holds every entry point to it under HBEGP_POOL_POISON.
#include <chrono>
#include <condition_variable>
#include <map>
#include <tuple>
struct DevPool {
  std::mutex mu;
  std::map<std::pair<int, size_t>, std::vector<void*>> free_list;
  // Fresh blocks are cleared on a NON-BLOCKING stream of the pool's own (one per device), never on the null stream: several
  // host threads may be fitting on one context (hbegp.h: "re-entrant per ctx"), and any null-stream operation issued while
  // another thread captures a graph fails with hipErrorStreamCaptureImplicit -- besides synchronising with nothing the engine
  // runs on (its streams are non-blocking), which is how round 4's late clear came about.
  std::map<int, hipStream_t> clear_stream;
  hipStream_t stream_of(int dev) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = clear_stream.find(dev);
    if (it != clear_stream.end()) return it->second;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) throw HipError{hipErrorOutOfMemory, "hipStreamCreateWithFlags (pool)", __LINE__};
    clear_stream[dev] = st;
    return st;
  }
  size_t cached = 0;
  static constexpr size_t MAX_CACHED = (size_t)24 << 30;
  void* get(int dev, size_t bytes, bool* fresh) {
    // Test switches (tests/test_gpu_parity.py::test_fresh_pool_blocks_are_cleared_before_their_first_writer):
    //   HBEGP_POOL_FRESH=1         never recycle: every block is a fresh hipMalloc, as in a fresh process
    //   HBEGP_POOL_NULL_DELAY_MB=N queue an N MiB fill on the null stream in front of every fresh block's clear (makes the
    //                              clear LATE on purpose: a first writer on a non-blocking stream then runs before it)
    //   HBEGP_POOL_OLD_CLEAR=1     round 1-4's clear: hipMemset with no synchronisation (the race the test must see fail)
    //   HBEGP_POOL_POISON=1|2      fill every block handed out, fresh (after its clear) or recycled, with finite garbage (1)
    //                              or with quiet NaNs (2): no result may depend on it (tests/test_gpu_pool_hygiene.py)
    const bool always_fresh = getenv("HBEGP_POOL_FRESH") != nullptr && atoi(getenv("HBEGP_POOL_FRESH")) != 0;
    void* recycled = nullptr;
    unsigned word = 0;
    if (!always_fresh) {
      std::lock_guard<std::mutex> lk(mu);
      auto it = free_list.find({dev, bytes});
      if (it != free_list.end() && !it->second.empty()) {
        void* p = it->second.back();
        it->second.pop_back();
        cached -= bytes;
        *fresh = false;
        recycled = p;
      }
    }
    if (recycled) {
      if (poison_word(&word)) {
        try {
          poison(dev, recycled, bytes, word);
        } catch (...) {
          put(dev, recycled, bytes);
          throw;
        }
      }
      return recycled;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      trim();  // give cached blocks back and retry once
      e = hipMalloc(&p, bytes);
      if (e != hipSuccess) throw HipError{e, "hipMalloc (pool)", __LINE__};
    }
    // a fresh block is cleared once, here (a recycled one is handed out as its last owner left it: see above)
    // hipMemset on device memory returns before the fill has run (it is queued on the null stream), and the engine's streams are
    // non-blocking ones that do not wait for the null stream: without the synchronisation below the fill runs CONCURRENTLY with,
    // or after, the block's first writer on such a stream (the model's copy of L^-1 in make_model, the kernel-matrix tiles of an
    // evaluation) and zeroes part or all of what was written -- seen once in round 4 as predictive variances that were off by
    // O(1) on a fresh process, where every block is a fresh one (profiles/r04_memset_race.txt).
    // (the work matrices only: with every small array delayed as well the backlog on the null stream outlasts the whole test)
    const int delay_mb = (bytes >= ((size_t)1 << 20) && getenv("HBEGP_POOL_NULL_DELAY_MB")) ? atoi(getenv("HBEGP_POOL_NULL_DELAY_MB")) : 0;
    if (delay_mb > 0) {
      static std::mutex dmu;
      static std::map<int, std::pair<void*, size_t>> scratch;  // per device, kept for the life of the process (a test switch)
      std::lock_guard<std::mutex> lk(dmu);
      auto& sc = scratch[dev];
      const size_t want = (size_t)delay_mb << 20;
      if (sc.second < want) {
        if (sc.first) (void)hipFree(sc.first);
        sc = {nullptr, 0};
        if (hipMalloc(&sc.first, want) == hipSuccess) sc.second = want;
      }
      if (sc.first) (void)hipMemsetAsync(sc.first, 0x5a, sc.second, nullptr);
    }
    if (bytes >= ((size_t)1 << 20) && getenv("HBEGP_POOL_OLD_CLEAR") != nullptr && atoi(getenv("HBEGP_POOL_OLD_CLEAR")) != 0) {
      e = hipMemset(p, 0, bytes);
    } else if (delay_mb > 0) {
      // the test's delayed form: the clear queues behind the long null-stream fill, and the synchronisation covers both
      e = hipMemsetAsync(p, 0, bytes, nullptr);
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    } else {
      hipStream_t st = stream_of(dev);
      e = hipMemsetAsync(p, 0, bytes, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
      (void)hipFree(p);
      throw HipError{e, "hipMemset (pool)", __LINE__};
    }
    if (poison_word(&word)) {
      try {
        poison(dev, p, bytes, word);
      } catch (...) {
        (void)hipFree(p);
        throw;
      }
    }
    *fresh = true;
    return p;
  }
  // HBEGP_POOL_POISON, read per call: 1 = 0x40490FDB (3.1415927f as a float, ~50.12 as the double 0x40490FDB40490FDB),
  // 2 = 0x7FF80000 (a quiet NaN in both element types).  Unset or 0: nothing.
  static bool poison_word(unsigned* word) {
    const char* v = getenv("HBEGP_POOL_POISON");
    const int mode = v ? atoi(v) : 0;
    if (mode == 1) *word = 0x40490FDBu;
    else if (mode == 2) *word = 0x7FF80000u;
    else return false;
    return true;
  }
  std::atomic<long long> poisoned_blocks{0}, poisoned_bytes{0};  // totals since process start (hbegp_debug_pool_poisoned)
  // The fill runs on the pool's own stream and is waited for, as the clear of a fresh block is; the trailing bytes % 4 bytes
  // get the word's low byte.
  void poison(int dev, void* p, size_t bytes, unsigned word) {
    hipStream_t st = stream_of(dev);
    hipError_t e = hipSuccess;
    const size_t words = bytes / 4, tail = bytes % 4;
    if (words) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)word, words, st);
    if (e == hipSuccess && tail) e = hipMemsetD8Async(reinterpret_cast<hipDeviceptr_t>(static_cast<char*>(p) + 4 * words), (unsigned char)(word & 0xff), tail, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) throw HipError{e, "poison fill (pool)", __LINE__};
    poisoned_blocks.fetch_add(1, std::memory_order_relaxed);
    poisoned_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
  }
  void put(int dev, void* p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    if (cached + bytes > MAX_CACHED) {
      (void)hipFree(p);
      return;
    }
    free_list[{dev, bytes}].push_back(p);
    cached += bytes;
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& kv : free_list)
      for (void* p : kv.second) (void)hipFree(p);
    free_list.clear();
    cached = 0;
  }
};
static DevPool g_pool;

// Pinned host blocks and streams are recycled as well: a fit of a small problem lasts ~10 ms, and creating + destroying its
// slots' streams, pinned parameter / result blocks and ~8 small device arrays per slot cost ~2 ms of it (every hipFree waits for
// the device).  Streams are handed back only after they have been synchronised.
struct HostPool {
  std::mutex mu;
  std::map<size_t, std::vector<void*>> free_list;
  void* get(size_t bytes) {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = free_list.find(bytes);
      if (it != free_list.end() && !it->second.empty()) {
        void* p = it->second.back();
        it->second.pop_back();
        return p;
      }
    }
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);  // fine-grained: a host thread spins on words the GPU writes (Problem::wait_eval)
    if (e != hipSuccess) throw HipError{e, "hipHostMalloc (pool)", __LINE__};
    return p;
  }
  void put(void* p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    auto& v = free_list[bytes];
    if (v.size() >= 64) { (void)hipHostFree(p); return; }
    v.push_back(p);
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& kv : free_list)
      for (void* p : kv.second) (void)hipHostFree(p);
    free_list.clear();
  }
};
static HostPool g_host_pool;
// HIP maps its streams onto a few hardware queues per device (4 by default) in the order the streams are
// created, and two streams that share a queue run one after the other.  So the pool is keyed by what a stream is FOR: the
// evaluation slots of a fit always get the same streams back (created first, on distinct queues), whatever a model's or the
// block pool's stream does in between -- with ONE free list a fit's three slots got, every other fit, two streams of one queue
// (measured: optimiser runs of config M 561 / 900 / 561 / 900 ms).
enum { STREAM_SLOT = 0, STREAM_MODEL = 1, STREAM_BATCH = 2 };
struct StreamPool {
  std::mutex mu;
  std::map<std::pair<int, int>, std::vector<hipStream_t>> free_list;
  hipStream_t get(int dev, int kind = STREAM_SLOT) {
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = free_list.find({dev, kind});
      if (it != free_list.end() && !it->second.empty()) {
        hipStream_t s = it->second.back();
        it->second.pop_back();
        return s;
      }
    }
    hipStream_t s = nullptr;
    hipError_t e;
    if (kind == STREAM_BATCH) {
      // the runtime keeps a pool of hardware queues PER PRIORITY: a stream of another priority never shares its queue with the
      // normal-priority streams of the fits -- whose copies and small kernels would otherwise wait for the ~10 ms persistent grid
      // of a small-fit batch whenever they land on its queue
      int least = 0, greatest = 0;
      e = hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (e != hipSuccess) throw HipError{e, "hipDeviceGetStreamPriorityRange", __LINE__};
      e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest);
    } else {
      e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    }
    if (e != hipSuccess) throw HipError{e, "hipStreamCreate (pool)", __LINE__};
    return s;
  }
  void put(int dev, hipStream_t s, int kind = STREAM_SLOT) {  // the caller has synchronised it
    if (!s) return;
    std::lock_guard<std::mutex> lk(mu);
    auto& v = free_list[{dev, kind}];
    if (v.size() >= 64) { (void)hipStreamDestroy(s); return; }
    v.push_back(s);
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& kv : free_list)
      for (hipStream_t s : kv.second) (void)hipStreamDestroy(s);
    free_list.clear();
  }
};
static StreamPool g_stream_pool;

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Fits of up to 128 rows from several host threads share their launches.  An optimiser run of such a fit is one workgroup of a
// persistent kernel (small_fit_kernel, ~10 ms); with a launch per fit the fits of different threads sit on different streams, HIP
// maps streams onto a handful of hardware queues, and a stream that shares its queue with another fit's persistent kernel waits
// for all of it (measured: 16 threads, 16 hardware queues: 560 fits/s where 16 / 10.5 ms = 1,500 would fit the chip; more
// queues made it worse).  So: a thread that arrives with its runs joins the batch that is open for its (device, kernel) or opens
// one; whoever opened it waits until no other thread is on its way (threads announce themselves when they enter the small-fit
// path: SmallBatcher::arriving) and none has just come back from a small fit (g_small_recent below), at most 3 ms of a ~10 ms fit (HBEGP_SMALL_BATCH_US; measured at 16 threads: 0.3 ms 724, 1 ms 959, 3 ms
// 1,113 fits/s -- under load a thread needs 2-3 ms to set its problem up), and launches all runs in ONE grid; every thread then polls the pinned words of its
// OWN runs (SmallFit::hdone) -- it neither waits for the other fits of the launch nor synchronises a stream.  One thread alone
// launches at once.  The workgroups of a launch do not depend on each other, so a run's bits do not depend on its company.
struct SmallBatch {
  std::vector<SmallFit> fits;
  bool closed = false, launched = false;
  int refs = 0;
  std::exception_ptr err;  // launch failure: every participant rethrows it
  void* fs_dev = nullptr;
  size_t fs_bytes = 0;
  hipStream_t stream = nullptr;
  int dev = 0;
};
struct SmallBatcher {
  std::mutex mu;
  std::condition_variable cv;
  std::map<std::tuple<int, int, bool>, std::shared_ptr<SmallBatch>> open;  // (device id, nu2, f32)
  std::atomic<int> arriving{0};  // threads inside the small-fit path that have not handed in their runs yet
};
static SmallBatcher g_small_batcher;
static std::mutex g_small_host_mu;      // turn-taking of the host-side phases of small fits (do_fit)
static std::atomic<int> g_small_active{0};  // threads inside a small fit
// Threads that have just come back from a small fit are the ones most likely to bring the next one: each thread keeps the time of
// its last return in a slot of this table (0 while it is inside a fit), and the thread that opens a batch also waits for those
// whose return is younger than SMALL_RECENT_NS (4 ms) -- without this, threads that finish together drift apart
// again (whoever is back first sees nobody on the way and launches alone: measured, 16 threads, 68 of 101 grids carried one fit).
constexpr int SMALL_RECENT_SLOTS = 64;
constexpr long long SMALL_RECENT_NS = 4000000;
static std::atomic<long long> g_small_recent[SMALL_RECENT_SLOTS];
static std::atomic<int> g_small_recent_next{0};
static int small_recent_slot() {
  static thread_local int slot = -1;
  if (slot < 0) slot = g_small_recent_next.fetch_add(1) % SMALL_RECENT_SLOTS;
  return slot;
}
static long long steady_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int small_recent_others(long long window_ns) {
  const long long now = steady_ns();
  const int mine = small_recent_slot();
  int c = 0;
  for (int i = 0; i < SMALL_RECENT_SLOTS; ++i) {
    const long long ts = g_small_recent[i].load(std::memory_order_relaxed);
    if (i != mine && ts != 0 && now - ts < window_ns) ++c;
  }
  return c;
}
struct SmallArrival {  // RAII: "I am on my way with runs"; on destruction: "I am back" (the time of the return is left in the table)
  bool counted = false, entered = false;
  void announce() {
    if (!counted) {
      g_small_batcher.arriving.fetch_add(1);
      counted = true;
      entered = true;
      g_small_recent[small_recent_slot()].store(0, std::memory_order_relaxed);
    }
  }
  void arrived() {
    if (counted) {
      g_small_batcher.arriving.fetch_sub(1);
      counted = false;
      g_small_batcher.cv.notify_all();
    }
  }
  ~SmallArrival() {
    arrived();
    if (entered) g_small_recent[small_recent_slot()].store(steady_ns(), std::memory_order_relaxed);
  }
};
static void small_batch_unref_locked(SmallBatch& b);
// Hands in `mine` (runs of one fit on device `dev`); returns the batch once its grid has been launched.  The caller polls its runs'
// SmallFit::hdone words and then calls small_batch_leave.  Throws if the launch failed.
template <typename T>
static std::shared_ptr<SmallBatch> small_batch_submit(int dev, int nu2, const std::vector<SmallFit>& mine, SmallArrival& arrival) {
  SmallBatcher& B = g_small_batcher;
  static const int window_us = env_int("HBEGP_SMALL_BATCH_US", 3000);
  std::unique_lock<std::mutex> lk(B.mu);
  const auto key = std::make_tuple(dev, nu2, sizeof(T) == 4);
  std::shared_ptr<SmallBatch> b = B.open[key];
  const bool leader = !b;
  if (leader) {
    b = std::make_shared<SmallBatch>();
    b->dev = dev;
    B.open[key] = b;
  }
  b->fits.insert(b->fits.end(), mine.begin(), mine.end());
  ++b->refs;
  arrival.arrived();  // (notifies: a leader waiting for the stragglers looks again)
  if (leader) {
    const auto t_open = std::chrono::steady_clock::now();
    if (window_us > 0) {
      // until nobody is on the way and nobody has just come back (their marks expire by themselves: look again every 200 us)
      const auto deadline = t_open + std::chrono::microseconds(window_us);
      while (std::chrono::steady_clock::now() < deadline && (B.arriving.load() != 0 || small_recent_others(SMALL_RECENT_NS) != 0))
        B.cv.wait_for(lk, std::chrono::microseconds(200));
    }
    b->closed = true;
    B.open.erase(key);
    lk.unlock();
    try {
      HIPCHECK(hipSetDevice(dev));
      b->fs_bytes = sizeof(SmallFit) * (size_t)round_up((int)b->fits.size(), 16);
      bool fresh = false;
      b->fs_dev = g_pool.get(dev, b->fs_bytes, &fresh);
      b->stream = g_stream_pool.get(dev, STREAM_BATCH);
      HIPCHECK(hipMemcpyAsync(b->fs_dev, b->fits.data(), sizeof(SmallFit) * b->fits.size(), hipMemcpyHostToDevice, b->stream));  // (the batch outlives the copy)
      launch_small_fit<T>(static_cast<const SmallFit*>(b->fs_dev), (int)b->fits.size(), nu2, b->stream);
      CHECK_LAUNCHES();
    } catch (...) {
      b->err = std::current_exception();
    }
    lk.lock();
    b->launched = true;
    B.cv.notify_all();
  } else {
    B.cv.wait(lk, [&] { return b->launched; });
  }
  if (b->err) {
    std::exception_ptr e = b->err;
    if (b->stream) (void)hipStreamSynchronize(b->stream);  // (a copy may have been queued before the launch failed)
    small_batch_unref_locked(*b);
    lk.unlock();
    std::rethrow_exception(e);
  }
  return b;
}
static void small_batch_unref_locked(SmallBatch& b) {
  if (--b.refs == 0) {  // every run of the grid is over (each participant saw its words, or waited for the stream)
    if (b.fs_dev) g_pool.put(b.dev, b.fs_dev, b.fs_bytes);
    if (b.stream) g_stream_pool.put(b.dev, b.stream, STREAM_BATCH);
    b.fs_dev = nullptr;
    b.stream = nullptr;
  }
}
// `finished`: the caller has seen every one of its runs' hdone words (false: it gave up -- the grid is waited for here, its
// workspaces are about to be released)
static void small_batch_leave(const std::shared_ptr<SmallBatch>& b, bool finished) {
  if (!b) return;
  if (!finished && b->stream) {
    (void)hipSetDevice(b->dev);
    (void)hipStreamSynchronize(b->stream);
  }
  std::lock_guard<std::mutex> lk(g_small_batcher.mu);
  small_batch_unref_locked(*b);
}
constexpr int DAG_PROG_MAX_BLOCKS = 20;  // right-looking plan: the inverse and K^-1 follow the chain row by row up to this many 128-blocks
constexpr int DAG_MIN_BLOCKS_FIT = 6;   // evaluations (a fit's, `extend`'s, single ones) use the task queue from this many 128-blocks on

// theta (log space) -> clamped linear-space parameters (fit.rs:94-96)
static void theta_to_params(const double* theta, const double* lo, const double* hi, int d, EvalParams* P) {
  auto clampv = [&](double v, int i) {
    if (!lo || !hi) return v;
    if (v < lo[i]) return lo[i];  // bounded_value.rs:43-56
    if (hi[i] < v) return hi[i];
    return v;
  };
  P->noise = std::exp(theta[0]);  // not clamped (fit.rs:96)
  P->amp = clampv(std::exp(theta[1]), 1);
  for (int k = 0; k < d; ++k) P->ell[k] = clampv(std::exp(theta[2 + k]), 2 + k);
}

// ---------------------------------------------------------------------------------------------------------------
// timing support for hbegp_problem_time_eval
struct PhaseTimer {
  enum Kind { KMAT = 0, GEMM = 1, LEAF = 2, LAUUM = 3, ALPHA = 4, GRAD = 5, DAG = 6, NKIND = 7 };
  struct Rec {
    hipEvent_t a, b;
    int kind, tile;
    double gflop;
  };
  std::vector<Rec> recs;
  hipStream_t s;
  void begin(int kind, int tile = 0, double gflop = 0) {
    Rec r;
    HIPCHECK(hipEventCreate(&r.a));
    HIPCHECK(hipEventCreate(&r.b));
    r.kind = kind; r.tile = tile; r.gflop = gflop;
    HIPCHECK(hipEventRecord(r.a, s));
    recs.push_back(r);
  }
  void end() { HIPCHECK(hipEventRecord(recs.back().b, s)); }
};

// tile size of a launch, by its number of 128-tiles
static int pick_tile(const GemmLaunch& g) {
  int tiles128 = 0;
  for (int i = 0; i < g.nops; ++i) tiles128 += g.op[i].c_lower ? g.op[i].mi * (g.op[i].mi + 1) / 2 : g.op[i].mi * g.op[i].nj;
  // 128-tiles only when a launch has >= 600 of them (n >= 8192): measured n=8192 15.1 -> 13.7 ms/evaluation with them,
  // n=4096 LAUUM (528 tiles) 0.44 ms with 64-tiles vs 0.77 ms with 128-tiles
  if (tiles128 >= 600) return 128;
  if (tiles128 >= 128) return 64;  // h=1024 SYRK+U (100 tiles): 58 us with 32-tiles vs 83 us with 64-tiles
  return 32;
}

// one tile-GEMM launch without a static schedule: the hardware dispatcher places the tiles
template <typename T>
static void gemm_adhoc(GemmLaunch& g, const int* info, hipStream_t s) {
  g.info = info;
  launch_gemm<T>(g, pick_tile(g), s);
}

// The one-op launch C = A B^T against a lower-triangular B (X = L^-1 or L itself: k <= j, klim 1 / maskB) from tile (0, 0):
// C is mi x nj tiles, the contraction runs over the tiles [0, k1).
static GemmLaunch gemm_lower_b(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int mi, int nj, int k1) {
  GemmLaunch g{};
  g.nops = 1;
  GemmOp& op = g.op[0];
  op.A = A; op.B = B; op.C = C;
  op.lda = lda; op.ldb = ldb; op.ldc = ldc;
  op.mi = mi; op.nj = nj;
  op.k0 = 0; op.k1 = k1;
  op.klim = 1; op.maskB = 1;
  return g;
}

// Cholesky + inverse of the factor of the SPD matrix in W1 (lower) on the diagonal block range [lo, hi) (units of 128), split
// at mid: X = L^-1 -> W2 (lower), diag(L) -> ldiag (by the diagonal blocks).  The TRSM result L21 = A21 X11^T goes to `L21`:
// W2 for the fit, where X21 overwrites it later, or a third matrix that keeps L (the joint posterior: its diagonal blocks store
// L_kk there too).  need_x: form X21 -- always for the fit; a kept factor needs X only where an enclosing left part does, so
// its top node skips it.  left_done: X (and diag(L)) of [lo, mid) are already in place (incremental extend).
// gemm(g, kind) issues one launch, leaf(k) runs diagonal block k.
template <typename T, class Gemm, class Leaf>
static void chol_inv_rec(T* W1, T* W2, T* L21, int ld, int lo, int mid, int hi, bool left_done, bool need_x, Gemm&& gemm,
                         Leaf&& leaf) {
  if (hi - lo == 1) {
    leaf(lo);
    return;
  }
  if (!left_done) chol_inv_rec<T>(W1, W2, L21, ld, lo, lo + (mid - lo) / 2, mid, false, true, gemm, leaf);
  GemmOp base{};
  base.lda = base.ldb = base.ldc = ld;
  {
    // L21 = A21 * X11^T   (TRSM of potrf as a product with the explicit inverse)
    GemmLaunch g{};
    g.nops = 1;
    GemmOp& op = g.op[0];
    op = base;
    op.A = W1; op.B = W2; op.C = L21;
    op.ci0 = mid; op.mi = hi - mid; op.cj0 = lo; op.nj = mid - lo;
    op.k0 = lo; op.k1 = mid; op.klim = 1; op.maskB = 1;
    gemm(g, PhaseTimer::GEMM);
  }
  {
    // A22 -= L21 L21^T (lower)   and, with need_x, U = L21 * X11 -> W1[2,1]   (independent: one launch, one static schedule).
    // Measured alternatives at n=4096: two launches 3.71 ms/evaluation, U forked onto a second stream inside the graph
    // 3.57 ms but 0.76 fit+predict/s in the 3-run bench (multi-branch graphs serialise badly); merged 3.38 ms, 1.10.
    GemmLaunch g{};
    g.nops = need_x ? 2 : 1;
    GemmOp& syrk = g.op[0];
    syrk = base;
    syrk.A = L21; syrk.B = L21; syrk.C = W1;
    syrk.ci0 = mid; syrk.cj0 = mid; syrk.mi = hi - mid; syrk.nj = hi - mid; syrk.c_lower = 1;
    syrk.k0 = lo; syrk.k1 = mid; syrk.alpha_neg = 1; syrk.beta_one = 1;
    GemmOp& u = g.op[1];
    u = base;
    u.A = L21; u.B = W2; u.C = W1;
    u.b_kmajor = 1;
    u.ci0 = mid; u.mi = hi - mid; u.cj0 = lo; u.nj = mid - lo;
    u.k0 = lo; u.k1 = mid; u.klim = 2; u.maskB = 1;
    gemm(g, PhaseTimer::GEMM);
  }
  chol_inv_rec<T>(W1, W2, L21, ld, mid, mid + (hi - mid) / 2, hi, false, need_x, gemm, leaf);
  if (need_x) {
    // X21 = -X22 * U -> W2[2,1]
    GemmLaunch g{};
    g.nops = 1;
    GemmOp& op = g.op[0];
    op = base;
    op.A = W2; op.B = W1; op.C = W2;
    op.b_kmajor = 1;
    op.ci0 = mid; op.mi = hi - mid; op.cj0 = lo; op.nj = mid - lo;
    op.k0 = mid; op.k1 = hi; op.klim = 3; op.maskA = 1; op.alpha_neg = 1;
    gemm(g, PhaseTimer::GEMM);
  }
}

// algorithmic flops of one op (in 128-tile units): 2*128^3 per (tile, k-tile) pair, half for pairs that only
// touch a triangle (storage-diagonal tile of a triangular operand, or a diagonal tile of a symmetric result)
static double op_gflop(const GemmOp& op) {
  double pairs = 0;
  for (int i = 0; i < op.mi; ++i)
    for (int j = 0; j < (op.c_lower ? i + 1 : op.nj); ++j) {
      const int ti = op.ci0 + i, tj = op.cj0 + j;
      int ka = op.k0, kb = op.k1;
      if (op.klim == 1) kb = std::min(kb, tj + 1);
      if (op.klim == 2) ka = std::max(ka, tj);
      if (op.klim == 3) kb = std::min(kb, ti + 1);
      if (op.klim == 4) ka = std::max(ka, ti);
      for (int k = ka; k < kb; ++k) {
        double w = 1.0;
        if ((op.maskA && k == ti) || (op.maskB && k == tj)) w = 0.5;
        if (op.c_lower && ti == tj) w = std::min(w, 0.5);
        pairs += w;
      }
    }
  return pairs * 2.0 * 128.0 * 128.0 * 128.0 * 1e-9;
}

// ---------------------------------------------------------------------------------------------------------------
// Static schedule of one large GEMM launch: tiles are assigned to a fixed number of resident workgroups by
// longest-processing-time-first on their contraction depth, so that triangular operands (depth 1..D per tile) do not
// leave most of the chip waiting for the few deepest tiles.  Built once per problem (shapes repeat every evaluation).
struct Sched {
  int* d_off = nullptr;
  unsigned* d_items = nullptr;
  int nwg = 0;   // 0: plain launch
  int tile = 0;
};

static void tile_krange(const GemmOp& op, int ti, int tj, int* ka, int* kb) {
  *ka = op.k0; *kb = op.k1;
  if (op.klim == 1) *kb = std::min(*kb, tj + 1);
  if (op.klim == 2) *ka = std::max(*ka, tj);
  if (op.klim == 3) *kb = std::min(*kb, ti + 1);
  if (op.klim == 4) *ka = std::max(*ka, ti);
}

// ops in NB units; returns host arrays for `tile`
static bool build_sched(const GemmLaunch& g, int tile, std::vector<int>* off, std::vector<unsigned>* items, int* nwg_out) {
  const int f = NB / tile;
  struct It { double w; unsigned code; };
  std::vector<It> its;
  for (int oi = 0; oi < g.nops; ++oi) {
    GemmOp op = g.op[oi];
    op.ci0 *= f; op.cj0 *= f; op.mi *= f; op.nj *= f; op.k0 *= f; op.k1 *= f;
    for (int i = 0; i < op.mi; ++i)
      for (int j = 0; j < (op.c_lower ? i + 1 : op.nj); ++j) {
        int ka, kb;
        tile_krange(op, op.ci0 + i, op.cj0 + j, &ka, &kb);
        its.push_back({(double)(kb - ka) + 0.75, ((unsigned)oi << 30) | ((unsigned)i << 16) | (unsigned)j});
      }
  }
  const int ntiles = (int)its.size();
  // resident workgroups per CU the kernel can reach (registers: 206 / 168 VGPRs for the 128- / 64-tile kernels)
  const int occmax = tile == 128 ? 2 : 3;  // residency the kernels reach (VGPRs); pinned via the LDS request
  // Above ~2 tiles per resident slot the hardware dispatcher (tiles are listed deepest-first) balances better than a
  // static list (measured: LAUUM at n=4096, 2080 tiles: 50 vs 47 TFLOP/s); below it the static list wins (TRSM 29 -> 44).
  // From 2048 tiles on the dispatcher alone.
  int nwg = 0;
  if (ntiles < 2048)
    for (int occ = occmax; occ >= 1; --occ)
      if (ntiles >= 2 * 256 * occ) { nwg = 256 * occ; break; }
  if (nwg == 0) return false;
  std::stable_sort(its.begin(), its.end(), [](const It& a, const It& b) { return a.w > b.w; });
  typedef std::pair<double, int> Load;  // (load, wg)
  std::priority_queue<Load, std::vector<Load>, std::greater<Load>> pq;
  for (int w = 0; w < nwg; ++w) pq.push({0.0, w});
  std::vector<std::vector<unsigned>> per(nwg);
  for (const It& it : its) {
    Load l = pq.top();
    pq.pop();
    per[l.second].push_back(it.code);
    pq.push({l.first + it.w, l.second});
  }
  off->assign(nwg + 1, 0);
  items->clear();
  for (int w = 0; w < nwg; ++w) {
    (*off)[w] = (int)items->size();
    items->insert(items->end(), per[w].begin(), per[w].end());
  }
  (*off)[nwg] = (int)items->size();
  *nwg_out = nwg;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int DAG_MAX_VARIANTS = 4;  // task-queue launches sized for 1..4 busy slots; with more slots the last one is shared
// ... and, behind those, launch sizes for a CROWDED device: optimiser runs of OTHER fits in flight on the same GPU (several host
// threads fitting side by side on one context -- replicas).  Sized for 6 / 12 / 24 runs in flight.
constexpr int DAG_CROWD_LEVELS = 3;
constexpr int DAG_CROWD_BUSY[DAG_CROWD_LEVELS] = {6, 12, 24};
// ... and, behind those, the two unequal shares of a fit whose runs have drifted apart (slot_share.hpp): lead, then lag
constexpr int DAG_SHARE_VARIANTS = 2;
constexpr int MAX_DEVS = 64;
// What a task-queue plan is built from: Problem::init keeps the plans it builds by this key
struct DagPlanKey {
  int blocks, bk, small_h, nwg, lauum, rl, rl_group, rl_near, lauum_split, chain32, prog, big128;
  int order_wg;  // workers the queue is ordered for where that is not nwg (0: nwg; DAG_ORDER_BY_LEVEL: no count)
  auto tie() const { return std::tie(blocks, bk, small_h, nwg, lauum, rl, rl_group, rl_near, lauum_split, chain32, prog, big128, order_wg); }
  bool operator<(const DagPlanKey& o) const { return tie() < o.tie(); }
};
static std::atomic<int> g_dev_busy[MAX_DEVS];  // optimiser runs in flight per device id, over all fits of the process
static std::atomic<int> g_dev_fits[MAX_DEVS];  // fits in flight per device id, from the moment they are called (hbegp_debug_fits_in_flight)

// What the leave-one-out tail (loo_tail, below the model) reads: the results an evaluation left on the device.  Kinv is read on and
// below the diagonal only (a slot's buffer is not mirrored), P may be a pinned host block.
template <typename T>
struct LooIn {
  int dev;
  hipStream_t s;
  int n, d, np, nu2;
  const T *X, *y, *alpha, *Xinv, *Kinv;
  const EvalParams* P;
};
template <typename T>
static int loo_tail(const LooIn<T>& in, T* mean, T* var, T* lpd, double* loo, double* grad);

// The input-gradient tail (below the model) on the same results: G = d lml / d X [n][d] -> gx (host, may be null),
// and with `chain` (host, 2 d entries) the dot products of G's columns with dlna / dlnb [n][d] (device, fp64).
template <typename T>
static int xgrad_tail(const LooIn<T>& in, double* gx, const double* dlna, const double* dlnb, double* chain);

// A partition of the training rows for leave-group-out cross-validation (lgo_tail): the caller's labels mapped to
// dense ids 0 .. G - 1 in order of first appearance, and the int lists the kernels read (engine.hpp: LgoLists), back to back in
// `lists` in the order member, gid, goff, foff, boff.
struct LgoGroups {
  int n = 0, G = 0, nb = 0, smax = 0;
  size_t f_elems = 0;  // doubles of the packed factors: the sum of s^2
  std::vector<int> lists;
  size_t bytes() const { return sizeof(int) * lists.size(); }
  LgoLists on_device(const int* base) const {
    LgoLists L;
    L.member = base;
    L.gid = L.member + n;
    L.goff = L.gid + n;
    L.foff = L.goff + (G + 1);
    L.boff = L.foff + (G + 1);
    L.G = G; L.nb = nb; L.smax = smax;
    return L;
  }
};
// group == nullptr: every row is its own group.  HBEGP_EINVAL for a group of more than HBEGP_LGO_MAX_GROUP rows.
static int build_lgo_groups(const int* group, int n, LgoGroups* out);
// dlists (may be null: uploaded for the call): gr.lists on the device the tail runs on
template <typename T>
static int lgo_tail(const LooIn<T>& in, const LgoGroups& gr, const int* dlists, T* mean, T* var, T* lpd, double* lgo, double* grad);

template <typename T>
struct Slot {
  int dev = 0;
  hipStream_t stream = nullptr;
  T *Xalt = nullptr, *ldalt = nullptr;  // device-driven small fit: second buffers for L^-1 / diag(L) (they ping-pong with K^-1 / alpha)
  bool x_captured = false;              // ... and after such a fit: (best_idx ? Xalt : W2) IS the captured evaluation's factor
  T *W1 = nullptr, *W2 = nullptr, *Kinv[2] = {nullptr, nullptr}, *alpha[2] = {nullptr, nullptr};
  T* W3 = nullptr;  // right-looking task-queue plan only: the Cholesky factor L (lower)
  T *ldiag = nullptr, *wbuf = nullptr;
  double *part_t = nullptr, *part_g = nullptr;
  EvalParams* dP = nullptr;
  EvalOut* dOut = nullptr;
  int* tickets = nullptr;    // [0] alpha / lml reduction, [1] gradient: "last workgroup finishes the launch's job" counters (zero between launches)
  unsigned long long* dag_trace = nullptr;  // HBEGP_DAG_TRACE: per-task time stamps of the last evaluation
  // HBEGP_DAG_TRACE_EVALS: the traces of a fit's own launches, kept on the host until the problem is released (keep_fit_trace)
  struct KeptTrace { unsigned long long seq; int part, variant, nwg; std::vector<unsigned long long> stamps; };
  std::vector<KeptTrace> kept_traces;
  int* dag_ctrl = nullptr;   // queue head + dependency counters of the task-queue kernel (cleared before every launch)
  EvalParams* hP = nullptr;  // pinned
  EvalOut* hOut = nullptr;   // pinned
  void* small_slab = nullptr;   // one pooled device block behind alpha[2], ldiag, wbuf, part_t, part_g, dP, dOut
  size_t small_slab_bytes = 0;
  void* host_slab = nullptr;    // one pooled pinned block behind hP, hOut
  size_t host_slab_bytes = 0;
  hipGraphExec_t graph[DAG_MAX_VARIANTS + 1 + DAG_CROWD_LEVELS + DAG_SHARE_VARIANTS][2][4] = {};  // [task-queue variant][target][EvalMode]
  // capture state (fit.rs:116-125)
  int best_idx = -1;  // which ping-pong buffer holds the best evaluation so far
  double best_lml = -std::numeric_limits<double>::infinity();
  int best_run = 0, best_eval = 0;
  std::vector<double> best_theta;
  std::vector<double> best_params;  // persistent fit kernel only: the clamped linear parameters the device evaluated the captured theta with
  int last_target = 0;  // buffer written by the most recent evaluation
  int dag_variant = 1;  // which ordering / launch size the next task-queue launch uses (Problem::DagVariant)
  int dag_part = 0;     // which of the variant's queues the last launch ran (launch_queue): the timeout report reads its task list
  unsigned long long seq = 0;  // serial number of the last evaluation handed to the device (EvalParams::seq)
  bool ctrl_cleared = false;   // the evaluation's first kernel clears dag_ctrl itself (EvalPrologue): no memset node
  bool published = false;      // the evaluation ends with publish_out_kernel: the host may spin on hOut->seq
  long long expect_ns[4] = {0, 0, 0, 0};  // per EvalMode: how long the last published evaluation took from launch to publication (wait_eval sleeps through most of it)
};

struct ProblemBase {
  hbegp_ctx* ctx = nullptr;
  int n = 0, d = 0, np = 0, nu2 = 5, n_slots = 1;
  bool is_f32 = false;
  virtual ~ProblemBase() {}
  virtual int eval(int dev, int slot, const double* theta, const double* lo, const double* hi, double* lml, double* grad) = 0;
  virtual int eval_loo(int dev, int slot, const double* theta, const double* lo, const double* hi, double* loo, double* grad) = 0;
  virtual int eval_lgo(int dev, int slot, const double* theta, const double* lo, const double* hi, const LgoGroups& gr, double* lgo,
                       double* grad) = 0;
  virtual int eval_xgrad(int dev, int slot, const double* theta, const double* lo, const double* hi, double* lml, double* grad, double* gx) = 0;
  virtual int eval_warped(int dev, int slot, const double* theta, const double* lo, const double* hi, const double* ab, double* lml,
                          double* grad) = 0;
  virtual int get_rows(int dev, void* out, bool want_f32) = 0;
  virtual int time_eval(int dev, int slot, const double* theta, int reps, double* phase_ms) = 0;
  virtual int time_concurrent(int dev, const double* theta, int reps, double* out) = 0;
};
struct hbegp_problem {
  std::unique_ptr<ProblemBase> impl;
};

template <typename T>
struct Problem : ProblemBase {
  std::vector<T*> Xd, yd;                 // per device
  std::vector<T*> X0d;                    // per device: the caller's rows, kept from the first hbegp_problem_eval_warped on (null: never warped)
  std::vector<double*> warp_ws_;          // per device, with X0d: the warp's parameters and parameter derivatives on the device
  std::vector<double> warp_ab_;
  std::vector<T*> rvd;                    // per device: the rows' known noise variances, n entries (null: none) -- K = c Matern + diag(s2 + v)
  std::vector<std::vector<Slot<T>>> slots;  // [device][slot]
  std::vector<std::vector<Sched>> scheds;   // [device][gemm launch ordinal]
  // device-scheduled factorisation (dag_kernel.inc.hpp): one plan per problem, the same on every device
  bool dag_ = false;
  bool dag_lauum_ = false;                  // the tiles of K^-1 = X^T X are tasks of the queue too (no LAUUM launch)
  bool dag_rl_ = false;                     // right-looking plan (dag_plan.hpp build_rl): the factor L lives in W3
  double dag_gflop_lauum = 0;
  // One ordering of the same task set per number of slots that are busy at the same time (variant v = 1..n_slots): a launch
  // gets the share of the CUs that fits v concurrent launches, and its queue is ordered for that many workgroups.  Same
  // tasks, same arithmetic, same bits for every variant -- only the order in which workgroups pull them differs.  A fit whose
  // optimiser runs end at different times (early stopping, 8 runs over 3 slots) gives the remaining runs the freed CUs.
  struct DagVariant {
    int nwg = 0;
    std::vector<DagTask*> tasks;            // per device
    std::vector<DagTask> host_tasks;        // kept for the trace dump
    // lazy fits (lazy_): the two queues of a line-search trial evaluated in two phases.  p1: the same plan built without the K^-1
    // tiles (what the lml needs); kinv: the full queue's K^-1 tasks alone (dag_plan_kinv_only), run when the gradient is wanted
    int nwg_p1 = 0, ntasks_p1 = 0, nwg_kinv = 0, ntasks_kinv = 0;
    std::vector<DagTask*> tasks_p1, tasks_kinv;  // per device
    std::vector<DagTask> host_tasks_p1, host_tasks_kinv;
  };
  std::vector<DagVariant> dag_var;          // [0] unused, [v] for v busy slots
  std::unique_ptr<std::atomic<int>[]> busy_slots_;  // per device: slots inside an optimiser run (0: not known -> all of them)
  int dag_ntasks = 0, dag_nwg = 0;          // dag_nwg: workgroups of the default variant (all slots busy)
  int dag_nvar_ = 1, dag_ncrowd_ = 0;       // variants [1..dag_nvar_] for this fit's own busy slots, then dag_ncrowd_ crowded-device levels
  // Unequal shares (slot_share.hpp; HBEGP_RUN_BALANCE, read when the problem is created): variants [nvar + ncrowd + 1] = lead and
  // [+ 2] = lag, 0 = none built.  A fit tells the problem which devices run one optimiser run per slot (balance_dev_) and keeps
  // every slot's progress (slot_running_ / slot_done_, [device * n_slots + slot]); variant_now asks the policy with them.
  int dag_nshare_ = 0;
  int share_hyst_ = SLOT_SHARE_HYSTERESIS;
  int slot_maxeval_ = 0;
  std::vector<int> share_force_;            // HBEGP_RUN_BALANCE_FORCE: the class of every slot, pinned (tests)
  std::vector<char> balance_dev_;           // per device
  std::unique_ptr<std::atomic<int>[]> slot_running_, slot_done_;
  // set for good by the first evaluation that finds another fit in flight on its device: such a fit keeps even shares to its
  // end, also after the other fit has left (several fits on a context: the crowded-device levels are their rule)
  mutable std::atomic<int> not_alone_{0};
  unsigned long long dag_wait_ticks_ = 200000000ull;  // bound of one dependency wait (100 MHz ticks), see init()
  size_t dag_ctrl_bytes = 0;                // one region of control words (queue head + counters)
  // A lazy fit's slots hold two regions: the second is the K^-1-only queue's.  The first kernel of every evaluation clears both
  // (EvalPrologue), and nothing but that queue touches the second one, so the second phase of a trial finds it clear: no fill node
  // in front of its launch.
  int dag_ctrl_regions_ = 1;
  double dag_gflop = 0;
  bool adhoc_ = false;                      // single-shot problem: no schedule table, every GEMM launch is ad hoc
  bool small_ = false;                      // np = 128, d <= 32: one evaluation = ONE launch (small_eval_kernel), everything in the LDS
  bool like_fit_ = false;                   // path selection of a fit (task queue from DAG_MIN_BLOCKS_FIT blocks on) although there is one slot
  // HBEGP_LAZY_GRAD (default 1; read when the problem is created; fits only): a line-search trial is evaluated in two phases --
  // everything the lml needs first (EVAL_LML_ONLY), K^-1 and the gradient (EVAL_GRAD_ONLY) only when the optimiser or the capture
  // rule will read them (do_fit).  0: every trial is one fused evaluation.  Same kernels, same tiles, same bits either way.
  bool lazy_ = false;
  std::function<std::shared_ptr<const DagPlan>(int, bool, int)> plan_for_;  // (workgroups, with the K^-1 tiles, ordered for) -> the cached plan
  // HBEGP_HOSTIO (default 1): an evaluation is driven through the slot's pinned blocks -- the first kernel reads the parameters
  // there and prepares the device-side blocks (EvalPrologue), the last one copies the results back and publishes the
  // evaluation's serial number, which the host thread spins on.  0: parameter copy + reset kernel + memset in front, a result
  // copy behind, hipStreamSynchronize (round 1-3).  Measured on config M (three optimiser runs, rocprofv3 kernel trace): the GPU
  // waited 52 + 54 + 29 us per evaluation for the host to enqueue the three extra nodes in front of the long kernel, and 84 us
  // between two evaluations.
  bool hostio_ = true;
  // ONE rule for "this problem's evaluations end by publishing their serial number into the pinned result block": enqueue_eval
  // acts on it when it runs, run_eval when a graph replay skips enqueue_eval (two copies of the condition could drift apart:
  // every evaluation would then sit out wait_eval's two-second fallback, or silently fall back to hipStreamSynchronize)
  bool eval_published() const { return hostio_ && !small_; }
  int leaf_dbg_ = 0;                        // HBEGP_LEAF_DBG: debug bits of the diagonal-block kernel (16: helper waves start late)
  // HBEGP_DAG_ZERO_SKIP (default 1): the 128x128 task-queue tiles skip the MFMAs of structurally zero operand halves (engine.hpp:
  // dag_zero_halves).  Only that tile reads it, so it is on from the size where those tiles are used; 0: every wave multiplies the
  // zeros as before.  Same bits either way.
  bool zero_skip_ = true;

  // Small device arrays of the problem (features, targets, task queues, schedule tables, control words) come from the block
  // pool too and go back to it in release(): hipMalloc / hipFree synchronise the whole device, which serialises host threads
  // that fit side by side on one context (and cost ~2 ms of a 10 ms fit even alone).
  struct Pooled { int dev; void* p; size_t bytes; };
  std::vector<Pooled> pooled_;
  template <typename U>
  U* palloc(int dev, size_t count) {
    bool fresh = false;
    const size_t bytes = std::max<size_t>(16, sizeof(U) * count);
    void* q = g_pool.get(dev, bytes, &fresh);
    pooled_.push_back({dev, q, bytes});
    return static_cast<U*>(q);
  }

  // single_shot: the problem runs one evaluation (extend): skip the static schedule tables, every GEMM launch is ad hoc
  // like_fit: choose the evaluation path (launches / task queue) as a fit of this size does, whatever the slot count --
  // `extend` then repeats the fit's own evaluation of a theta bit for bit
  // rv: n known noise variances (validated by the caller: finite and >= 0 in T) or null; data like X and y, converted once
  Problem(hbegp_ctx* c, const T* X, const T* y, int n_, int d_, double nu, int n_slots_, bool single_shot = false, bool like_fit = false,
          bool lazy_fit = false, const double* rv = nullptr) {
    try {
      adhoc_ = single_shot;
      like_fit_ = like_fit;
      lazy_ = lazy_fit && env_int("HBEGP_LAZY_GRAD", 1) != 0;
      init(c, X, y, n_, d_, nu, n_slots_, rv);
    } catch (...) {
      release();  // a constructor that throws never runs the destructor: give back what was allocated so far
      throw;
    }
  }

  void init(hbegp_ctx* c, const T* X, const T* y, int n_, int d_, double nu, int n_slots_, const double* rv) {
    ctx = c; n = n_; d = d_; np = round_up(n_, NB); n_slots = n_slots_;
    nu2 = std::isinf(nu) ? 0 : (int)std::lround(2 * nu);  // 0 = squared exponential (nu = infinity)
    is_f32 = sizeof(T) == 4;
    leaf_dbg_ = env_int("HBEGP_LEAF_DBG", 0) & 16;  // tests only; the bits that skip work stay with tools/leaf_bench
    zero_skip_ = env_int("HBEGP_DAG_ZERO_SKIP", 1) != 0;
    // The reference's own regime (minimize.rs:118-120: n stays at 100-200): up to 128 rows the five launches of the general path
    // cost more in launch gaps and HBM round trips than in arithmetic; one workgroup does the whole evaluation in its LDS
    // instead (HBEGP_SMALL=0: the general path, which the tests compare it with).
    small_ = np == NB && d <= SMALL_EVAL_MAXD && env_int("HBEGP_SMALL", 1) != 0;
    hostio_ = env_int("HBEGP_HOSTIO", 1) != 0;
    // two phases need the published evaluation (the second phase republishes the result block); the single-launch evaluation
    // of up to 128 rows stays fused
    lazy_ = lazy_ && eval_published() && !adhoc_;
    const size_t nn = (size_t)np * np;
    Xd.assign(c->devs.size(), nullptr);
    yd.assign(c->devs.size(), nullptr);
    rvd.assign(c->devs.size(), nullptr);
    std::vector<T> rv_t;  // the source of asynchronous copies: alive until every device's stream has been waited for below
    if (rv) rv_t.assign(rv, rv + n_);
    slots.resize(c->devs.size());
    for (size_t di = 0; di < c->devs.size(); ++di) {
      HIPCHECK(hipSetDevice(c->devs[di]));
      slots[di].resize(n_slots);
      for (auto& s : slots[di]) {
        s.dev = c->devs[di];
        s.stream = g_stream_pool.get(s.dev);
      }
      // everything this constructor queues goes to the first slot's (non-blocking) stream and is waited for on THAT stream:
      // no null-stream operation, no device-wide synchronisation (other host threads may be fitting on this device)
      hipStream_t st0 = slots[di][0].stream;
      Xd[di] = palloc<T>(c->devs[di], (size_t)n * d);
      yd[di] = palloc<T>(c->devs[di], np);
      HIPCHECK(hipMemsetAsync(yd[di], 0, sizeof(T) * np, st0));
      HIPCHECK(hipMemcpyAsync(Xd[di], X, sizeof(T) * (size_t)n * d, hipMemcpyHostToDevice, st0));
      HIPCHECK(hipMemcpyAsync(yd[di], y, sizeof(T) * n, hipMemcpyHostToDevice, st0));
      if (rv) {
        rvd[di] = palloc<T>(c->devs[di], n);
        HIPCHECK(hipMemcpyAsync(rvd[di], rv_t.data(), sizeof(T) * n, hipMemcpyHostToDevice, st0));
      }
      for (auto& s : slots[di]) {
        bool fresh1 = false, fresh2 = false, fk = false;
        s.W1 = static_cast<T*>(g_pool.get(s.dev, sizeof(T) * nn, &fresh1));
        s.W2 = static_cast<T*>(g_pool.get(s.dev, sizeof(T) * nn, &fresh2));
        for (int b = 0; b < 2; ++b) s.Kinv[b] = static_cast<T*>(g_pool.get(s.dev, sizeof(T) * nn, &fk));
        // W2 carries the triangular operand X = L^-1.  The GEMM loader does not mask: the strict upper triangle of W2 must
        // BE zero (tiles on the diagonal are loaded whole).  Nothing in the engine writes there, so clearing the buffer
        // once per slot is enough -- also when it is recycled from the pool (it may have held a full symmetric K^-1).
        // W1 needs no clear: it is a GEMM operand only through tiles strictly below the diagonal, which kmat_kernel writes
        // whole; of its diagonal tiles the diagonal-block kernels read the lower triangle, and what the SYRK updates leave in
        // their upper right quadrants (whatever was there, NaN included, minus L21 L21^T) is never read.  K^-1 and W3 (L)
        // likewise: only written tiles are read.
        HIPCHECK(hipMemsetAsync(s.W2, 0, sizeof(T) * nn, st0));
        (void)fresh1; (void)fresh2; (void)fk;  // fresh blocks were cleared by the pool
        // the small per-slot arrays: one pooled block
        {
          auto up = [](size_t v) { return (v + 255) / 256 * 256; };
          const size_t b_vec = up(sizeof(T) * np);
          const size_t b_part_t = up(sizeof(double) * ((size_t)((np + 255) / 256) * np + 2 * (size_t)((np + 255) / 256) + 64));
          const size_t b_part_g = up(sizeof(double) * gradtrace_part_elems(np, d));
          const size_t b_p = up(sizeof(EvalParams)), b_o = up(sizeof(EvalOut));
          s.small_slab_bytes = 4 * b_vec + b_part_t + b_part_g + b_p + b_o + 256;
          bool fs = false;
          s.small_slab = g_pool.get(s.dev, s.small_slab_bytes, &fs);
          char* q = static_cast<char*>(s.small_slab);
          s.alpha[0] = reinterpret_cast<T*>(q); q += b_vec;
          s.alpha[1] = reinterpret_cast<T*>(q); q += b_vec;
          s.ldiag = reinterpret_cast<T*>(q); q += b_vec;
          s.wbuf = reinterpret_cast<T*>(q); q += b_vec;
          s.part_t = reinterpret_cast<double*>(q); q += b_part_t;
          s.part_g = reinterpret_cast<double*>(q); q += b_part_g;
          s.dP = reinterpret_cast<EvalParams*>(q); q += b_p;
          s.dOut = reinterpret_cast<EvalOut*>(q); q += b_o;
          s.tickets = reinterpret_cast<int*>(q);
          HIPCHECK(hipMemsetAsync(s.dOut, 0, b_o + 256, st0));  // the result block and, right behind it, the tickets: one fill
          const size_t h_p = up(sizeof(EvalParams));
          s.host_slab_bytes = h_p + up(sizeof(EvalOut));
          s.host_slab = g_host_pool.get(s.host_slab_bytes);
          s.hP = reinterpret_cast<EvalParams*>(s.host_slab);
          s.hOut = reinterpret_cast<EvalOut*>(static_cast<char*>(s.host_slab) + h_p);
          memset(s.hP, 0, sizeof(EvalParams));
          memset(s.hOut, 0, sizeof(EvalOut));
        }
      }
      HIPCHECK(hipStreamSynchronize(st0));
    }
    // Task queue of the factorisation.  The workgroups of one launch hold a CU each while they wait for the diagonal
    // blocks, so a problem whose slots run concurrently shares the CUs between its slots.
    // Default: on for problems whose slots run concurrently (a fit: the optimiser runs share the chip, and a resident
    // task-queue kernel keeps its CUs while another run's tile GEMMs fill the rest: measured 1.30 -> 1.56 fit+predict/s
    // on config M), and for any problem of n > 4608, where the look-ahead hides the chain behind the bulk tiles (one
    // evaluation alone, launches vs task queue: n=4096 2.92 vs 2.98 ms, 6144 7.10 vs 5.90, 8192 12.7 vs 10.6, 16384 86.3 vs
    // 72.1); below that a single evaluation stream is a few per cent faster as a chain of launches.
    // HBEGP_DAG=0/1 forces it (read per problem: the parity tests flip it inside one process).
    const int dag_env = env_int("HBEGP_DAG", -1);
    // measured (config M data, launches vs task queue): one evaluation alone n=1536: 0.75 / 0.78 ms, 2048: 1.05 / 1.02, 4096: 2.89 / 2.19,
    // 8192: 12.7 / 9.9; three concurrent optimiser runs (fits/s) n=512: 21.1 / 19.6, 1024: 11.35 / 11.48, 1536: 6.80 / 7.95, 4096: 1.29 / 1.58
    // round 4 (faster diagonal block, evaluations driven through pinned memory): three runs side by side, fits/s, launches / task
    // queue: n=1024: 14.4 / 13.4, 1536: 7.95 / 8.7, 2048: 5.3 / 6.0 -- the queue from 12 blocks on (round 3: 8)
    // with the row-progressive plan (dag_plan.hpp rl_progressive): n=512: 29.8 / 28.6, 768: 19.9 / 20.7, 896: 17.0 / 18.3, 1024: 14.5 / 15.6,
    // 1280: 10.3 / 12.3; one evaluation alone (ms): n=512 0.202 / 0.218, 768 0.301 / 0.302, 896 0.357 / 0.347, 1024 0.406 / 0.385,
    // 1536 0.650 / 0.572 -- the queue from 6 blocks on, for fits and for single evaluations alike
    const int dag_min_blocks = env_int("HBEGP_DAG_MIN_BLOCKS", DAG_MIN_BLOCKS_FIT);
    dag_ = (dag_env < 0 ? np / NB >= dag_min_blocks : dag_env != 0) && !adhoc_ && np / NB >= 2;
    if (dag_) {
      int cus = 1 << 30;  // the launch sizes are shared by the devices of the context: size them for the smallest one
      for (int dev : c->devs) {
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, dev));
        cus = std::min(cus, std::max(1, prop.multiProcessorCount));
      }
      const int forced = env_int("HBEGP_DAG_WG", 0);
      // Concurrent slots: each launch gets a little more than its share of the CUs (a multiple of 8: the dispatcher deals
      // workgroups round-robin to the 8 XCCs).  The surplus workgroups of a launch start on the CUs another slot's launch has
      // just given back (that slot is in its short kmat / alpha / gradient launches) and leave when their own queue is empty.
      // Measured, 3 slots, n=4096, fit+predict/s: 80 -> 1.58, 85 -> 1.62, 88 -> 1.64, 96 -> 1.68, 104 -> 1.64, 112 -> 1.68,
      // 120 -> 1.54, 128 -> 1.60, 170 -> 1.43, 256 -> 1.14.
      auto share_of = [&](int busy) {
        const int share = busy <= 1 ? cus : std::max(8, (cus * 112 / 100 / busy + 4) / 8 * 8);  // 3 slots: 96
        return forced > 0 ? forced : std::max(1, std::min(cus, share));
      };
      // plans depend only on (blocks, stage depth, tiling and ordering knobs): the caller fits one model per generation with
      // slowly growing n, so they are kept (building + simulating the n=4096 queue costs ~15 ms of host time per fit)
      // HBEGP_DAG_LAUUM (default 1): the tiles of K^-1 = X^T X follow the recursion in the same queue, as 128x64 tile tasks,
      // instead of a gemm_kernel launch behind the task-queue launch
      dag_lauum_ = env_int("HBEGP_DAG_LAUUM", 1) != 0;
      // HBEGP_DAG_RL: right-looking tile Cholesky + divide-and-conquer inverse instead of the recursion that carries the
      // inverse: two 128-deep tiles between consecutive diagonal blocks instead of products as deep as the node is wide
      // (critical path of one evaluation at n = 4096: 2.83 -> 2.02 ms, simulated).  Not bitwise equal to the launch path
      // (another order of operations); the recursion plan stays available (0) and is what the bitwise tests pin.
      // Above ~10k rows one evaluation is bound by the tile work, where the recursion's deeper tiles win again (n=8192: 10.3 /
      // 9.9 ms recursion / right-looking, 12288: 31.4 / 32.0, 16384: 72.3 / 75.5).
      dag_rl_ = env_int("HBEGP_DAG_RL", np / NB <= 80 ? 1 : 0) != 0;
      static std::mutex cache_mu;
      static std::map<DagPlanKey, std::shared_ptr<const DagPlan>> cache;
      plan_for_ = [this](int nwg, bool lauum, int order_wg) {
        const DagPlanKey key = {np / NB, dag_stage_depth(is_f32), env_int("HBEGP_DAG_SMALLH", dag_rl_ ? 4 : 8), nwg, lauum, dag_rl_,
                                env_int("HBEGP_DAG_RL_GROUP", 32), env_int("HBEGP_DAG_RL_NEAR", 1),
                                env_int("HBEGP_DAG_LAUUM_SPLIT", n_slots <= 1 ? 1 : 0),
                                env_int("HBEGP_DAG_CHAIN32", 1),
                                // row-progressive inverse and K^-1 (dag_plan.hpp rl_progressive) up to 20 blocks.  Measured (divide and
                                // conquer / progressive; one evaluation alone in ms, three-run fits per s): n=1536 0.65/0.65, 9.0/10.1;
                                // 2048 0.88/0.80, 6.4/7.1; 2560 1.12/1.05, 4.5/4.7; 3072 1.41/1.30, 3.37/3.21; 3584 1.75/1.67, 2.38/2.21;
                                // 4096 2.08/2.08, 1.67/1.55; C5 (n=2048 f32): 0.85/0.75 ms, 8.9/12.5 fits/s.  Above ~22 blocks the bulk
                                // tiles fill every CU and the chain's tasks wait for a free workgroup; a function of n alone, so that
                                // `extend` repeats a fit's evaluation bit for bit.
                                env_int("HBEGP_DAG_PROG", np / NB <= DAG_PROG_MAX_BLOCKS ? 1 : 0),
                                // 128x128 tiles for the deep products without beta = 1 when several slots share the chip (throughput: half the
                                // tasks, fewer fragment reads per MFMA): three-run fits M f64 1.727 -> 1.740, M f32 2.64 -> 2.77, C4 0.233 ->
                                // 0.245; one evaluation alone gets SLOWER (fewer, longer tasks on 256 workgroups: n=4096 2.08 -> 2.22 ms), so
                                // single-slot problems keep 128x64.  The bits do not depend on the tile shape (one k-ascending chain of MFMA
                                // accumulations per element), so `extend` still repeats a fit's evaluation bit for bit.
                                // Below 32 blocks the fits lose (n=1536 10.4 -> 8.5, 2048 7.0 -> 6.4, 3072 3.36 -> 3.13 fits/s: too few deep
                                // products, the longer tasks only unbalance the end of the launch).
                                // 2: also the tiles with beta = 1 (the trailing updates; the old values are then fetched in the epilogue): M f64
                                // 1.711 / 1.737 / 1.739 -> 1.753 / 1.754 / 1.756 (alternating), M f32 2.76 -> 2.80, C4 0.242 -> 0.249 fits/s.
                                // One evaluation alone: n=6144 4.58 -> 4.73 ms (worse), n=8192 9.69 -> 9.31 ms: from 64 blocks on there too.
                                env_int("HBEGP_DAG_BIG128", ((n_slots >= 2 && np / NB >= 32) || np / NB >= 64) ? 2 : 0),  // one evaluation alone: 2.21 -> 2.17 ms at n=4096, 1.02 -> 0.97 at 2048; a fit: 1.67 -> 1.66
                                (order_wg == nwg || nwg <= 0) ? 0 : order_wg};
        std::shared_ptr<const DagPlan> cached;
        {
          std::lock_guard<std::mutex> lk(cache_mu);
          auto it = cache.find(key);
          if (it != cache.end()) cached = it->second;
        }
        if (!cached) {
          DagBuilder builder(key.bk, key.small_h, key.nwg, true, key.order_wg);
          builder.set_rl(key.rl_group, key.rl_near, key.lauum_split != 0, key.chain32 != 0);
          builder.set_rl_progressive(key.prog != 0);
          builder.set_big128(key.big128 != 0, key.big128 >= 2);
          cached = std::make_shared<const DagPlan>(builder.build(0, np / NB, lauum, dag_rl_));
          // a queue ordered for another count than it is launched with is checked before it runs anywhere, once per cached plan
          if (key.order_wg != 0 && !cached->tasks.empty()) {
            const std::string why = dag_plan_validate(*cached, np / NB);
            if (!why.empty()) throw std::runtime_error("task queue ordered for another worker count is unsound: " + why);
          }
          std::lock_guard<std::mutex> lk(cache_mu);
          if (cache.size() > 256) cache.clear();  // (a lazy fit keeps two plans per launch size)
          cache[key] = cached;
        }
        return cached;
      };
      const int nvar = std::min(n_slots, DAG_MAX_VARIANTS);
      dag_nwg = share_of(n_slots);  // the default variant: every slot busy
      // What a queue is ordered for (dag_plan.hpp: DagBuilder's order_wg), per kind of queue -- 0 the fused one, 1 phase 1, 2 the K^-1
      // tasks alone -- and per share of the launch (slot_share.hpp: even, which the busy-count and crowded-device variants are too,
      // lead, lag).  HBEGP_DAG_ORDER_WG / _P1 / _KINV force it for the three queues of the even variants, _LEAD / _LAG for all three
      // queues of the lead / the lag variant: N > 0 a list schedule for N workers, -1 the count-independent order; unset or 0: the
      // default (dag_default_order_wg).  The answer 0 means the launch's own count -- the queues are then what they always were.
      auto order_wg_for = [this](int queue, int share, int nwg) {
        const char* name = share == SLOT_SHARE_LEAD ? "HBEGP_DAG_ORDER_WG_LEAD"
                           : (share == SLOT_SHARE_LAG ? "HBEGP_DAG_ORDER_WG_LAG"
                              : (queue == 1 ? "HBEGP_DAG_ORDER_WG_P1" : (queue == 2 ? "HBEGP_DAG_ORDER_WG_KINV" : "HBEGP_DAG_ORDER_WG")));
        const int forced = env_int(name, 0);
        return forced != 0 ? std::max(forced, DAG_ORDER_BY_LEVEL) : dag_default_order_wg(queue, share, nwg, dag_nwg, np / NB, n_slots);
      };
      auto plan_for = [this, order_wg_for](int nwg, int share = SLOT_SHARE_EVEN) { return plan_for_(nwg, dag_lauum_, order_wg_for(0, share, nwg)); };
      std::shared_ptr<const DagPlan> cached = plan_for(dag_nwg);
      if (cached->tasks.empty() && dag_rl_) {  // too many counters for 16-bit ids (n > ~12k): the recursion plan needs far fewer
        dag_rl_ = false;
        cached = plan_for(dag_nwg);
      }
      const DagPlan& plan = *cached;
      if (plan.tasks.empty()) dag_ = dag_lauum_ = false;  // too many counters for 16-bit ids (n > 32k): launch-per-product path
      if (dag_ && env_int("HBEGP_DAG_VALIDATE", 0)) {
        const std::string why = dag_plan_validate(plan, np / NB);
        if (!why.empty()) throw std::runtime_error("task queue of the factorisation is unsound: " + why);
      }
      if (dag_) {
        dag_ntasks = (int)plan.tasks.size();
        dag_nwg = std::min(dag_nwg, dag_ntasks);
        dag_gflop = plan.gflop;
        dag_gflop_lauum = plan.gflop_lauum;
        dag_ctrl_bytes = (sizeof(int) * (DAG_CTRL_WORDS + plan.totals.size()) + 15) / 16 * 16;
        dag_ctrl_regions_ = (lazy_ && dag_lauum_) ? 2 : 1;
        // A dependency wait longer than this is reported as a scheduling bug (info = -2).  The clock runs on while the queue is
        // preempted or time-sliced (another process, a profiler serialising dispatches) and single waits grow with the plan, so
        // the bound follows the plan: 200 x its simulated makespan with every slot sharing the chip, at least 2 s.
        dag_wait_ticks_ = (unsigned long long)(std::max(2.0, 200.0 * plan.sim_us * 1e-6 * std::max(1, n_slots)) * 1e8);
        busy_slots_.reset(new std::atomic<int>[c->devs.size()]);
        for (size_t di = 0; di < c->devs.size(); ++di) busy_slots_[di].store(0);
        // the variants: [nvar] = the default (every slot busy), [v < nvar] for v busy slots (HBEGP_DAG_ADAPT=0: default only)
        const bool adapt = env_int("HBEGP_DAG_ADAPT", 1) != 0 && forced <= 0;
        // [nvar + 1 + l]: a crowded device, DAG_CROWD_BUSY[l] runs in flight over all fits (only for problems with several slots: a fit;
        // same tasks, same bits -- fewer workgroups per launch, so that all the launches in flight are resident)
        dag_nvar_ = nvar;
        dag_ncrowd_ = (adapt && n_slots > 1) ? DAG_CROWD_LEVELS : 0;
        // [nvar + ncrowd + 1], [+ 2]: the lead and the lag share of a fit whose runs have drifted apart (slot_share.hpp) -- again the
        // same tasks and bits, ordered for another workgroup count.  Only where the policy can ever be asked: several slots, and the
        // busy-count variants in use.  HBEGP_RUN_BALANCE=0: none are built and variant_now is what it was.
        int share_wg[DAG_SHARE_VARIANTS] = {slot_share_lead_wg(dag_nwg, n_slots, cus), slot_share_lag_wg(dag_nwg, n_slots, cus)};
        if (const char* wgs = getenv("HBEGP_RUN_BALANCE_WG")) {
          int a = 0, b = 0;
          if (sscanf(wgs, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) { share_wg[0] = std::min(a, cus); share_wg[1] = std::min(b, cus); }
        }
        const char* share_force = getenv("HBEGP_RUN_BALANCE_FORCE");
        share_force_.clear();
        if (share_force && *share_force) {
          for (const char* q = share_force; *q;) {
            const size_t len = strcspn(q, ",");
            share_force_.push_back(strncmp(q, "lag", 3) == 0 ? SLOT_SHARE_LAG : (strncmp(q, "lead", 4) == 0 ? SLOT_SHARE_LEAD : SLOT_SHARE_EVEN));
            q += len;
            if (*q == ',') ++q;
          }
          share_force_.resize(n_slots, SLOT_SHARE_EVEN);
        }
        share_hyst_ = std::max(0, env_int("HBEGP_RUN_BALANCE_HYST", SLOT_SHARE_HYSTERESIS));
        dag_nshare_ = (adapt && n_slots > 1 && (env_int("HBEGP_RUN_BALANCE", np / NB >= SLOT_SHARE_MIN_BLOCKS ? 1 : 0) != 0 || !share_force_.empty())) ? DAG_SHARE_VARIANTS : 0;
        if (dag_nshare_) {
          balance_dev_.assign(c->devs.size(), 0);
          slot_running_.reset(new std::atomic<int>[c->devs.size() * n_slots]);
          slot_done_.reset(new std::atomic<int>[c->devs.size() * n_slots]);
          for (size_t i = 0; i < c->devs.size() * n_slots; ++i) { slot_running_[i].store(0); slot_done_[i].store(0); }
        }
        dag_var.assign(nvar + 1 + dag_ncrowd_ + dag_nshare_, DagVariant());
        for (int v = 1; v <= nvar + dag_ncrowd_ + dag_nshare_; ++v) {
          DagVariant& var = dag_var[v];
          std::shared_ptr<const DagPlan> pv = cached;
          var.nwg = dag_nwg;
          const int share = v > nvar + dag_ncrowd_ ? (v == nvar + dag_ncrowd_ + 1 ? SLOT_SHARE_LEAD : SLOT_SHARE_LAG) : SLOT_SHARE_EVEN;
          if (v != nvar && adapt) {
            if (v > nvar + dag_ncrowd_) {
              var.nwg = std::min(share_wg[v - nvar - dag_ncrowd_ - 1], dag_ntasks);
            } else {
              const int busy = v < nvar ? v : DAG_CROWD_BUSY[v - nvar - 1];
              var.nwg = std::min(share_of(busy), dag_ntasks);
              if (v > nvar) var.nwg = std::min(var.nwg, dag_nwg);
            }
            pv = plan_for(var.nwg, share);
            if (pv->tasks.size() != plan.tasks.size()) { pv = cached; var.nwg = dag_nwg; }  // cannot happen: same task set
          }
          var.host_tasks = pv->tasks;
          var.tasks.assign(c->devs.size(), nullptr);
          for (size_t di = 0; di < c->devs.size(); ++di) {
            HIPCHECK(hipSetDevice(c->devs[di]));
            var.tasks[di] = palloc<DagTask>(c->devs[di], pv->tasks.size());
            HIPCHECK(hipMemcpyAsync(var.tasks[di], var.host_tasks.data(), sizeof(DagTask) * var.host_tasks.size(), hipMemcpyHostToDevice, slots[di][0].stream));  // (the source outlives the copy: it is the problem's own)
          }
          if (lazy_ && dag_lauum_) {
            // the two queues of a trial evaluated in two phases, from THIS variant's plan: phase 1 the same plan built without
            // the K^-1 tiles (the planner's lauum = false form, as factor_only's arithmetic: the same tiles of the factorisation),
            // phase 2 the full queue's K^-1 tasks alone, in its order.  Workgroups per launch as the fused launch of the variant.
            const int wg_p1 = lazy_wg(var.nwg, 1), wg_kinv = lazy_wg(var.nwg, 2);
            const std::shared_ptr<const DagPlan> p1 = plan_for_(wg_p1, false, order_wg_for(1, share, wg_p1));
            // (the K^-1 tasks keep the order they have in a full queue: the variant's own, unless theirs is ordered for another count)
            const int order_kinv = order_wg_for(2, share, wg_kinv);
            const std::shared_ptr<const DagPlan> pk = order_kinv == 0 ? pv : plan_for_(var.nwg, true, order_kinv);
            const DagPlan kv = dag_plan_kinv_only(*pk);
            if (p1->tasks.empty() || kv.tasks.empty() || p1->totals.size() > plan.totals.size() || kv.totals.size() > plan.totals.size()) {
              // the full plan exists and these are parts of it: anything else is a planner bug, not a reason to half-disable the path
              throw std::runtime_error("task queues of a two-phase evaluation could not be derived from the plan");
            } else {
              if (env_int("HBEGP_DAG_VALIDATE", 0)) {
                std::string why = dag_plan_validate(*p1, np / NB);
                if (why.empty()) why = dag_plan_validate(kv, np / NB);
                if (!why.empty()) throw std::runtime_error("task queue of a two-phase evaluation is unsound: " + why);
              }
              var.host_tasks_p1 = p1->tasks;
              var.host_tasks_kinv = kv.tasks;
              var.ntasks_p1 = (int)p1->tasks.size();
              var.ntasks_kinv = (int)kv.tasks.size();
              var.nwg_p1 = std::min(wg_p1, var.ntasks_p1);
              var.nwg_kinv = std::min(wg_kinv, var.ntasks_kinv);
              var.tasks_p1.assign(c->devs.size(), nullptr);
              var.tasks_kinv.assign(c->devs.size(), nullptr);
              for (size_t di = 0; di < c->devs.size(); ++di) {
                HIPCHECK(hipSetDevice(c->devs[di]));
                var.tasks_p1[di] = palloc<DagTask>(c->devs[di], var.host_tasks_p1.size());
                var.tasks_kinv[di] = palloc<DagTask>(c->devs[di], var.host_tasks_kinv.size());
                HIPCHECK(hipMemcpyAsync(var.tasks_p1[di], var.host_tasks_p1.data(), sizeof(DagTask) * var.host_tasks_p1.size(), hipMemcpyHostToDevice, slots[di][0].stream));
                HIPCHECK(hipMemcpyAsync(var.tasks_kinv[di], var.host_tasks_kinv.data(), sizeof(DagTask) * var.host_tasks_kinv.size(), hipMemcpyHostToDevice, slots[di][0].stream));
              }
            }
          }
        }
        for (size_t di = 0; di < c->devs.size(); ++di) {
          HIPCHECK(hipSetDevice(c->devs[di]));
          for (auto& s : slots[di]) {
            if (dag_rl_) {
              bool f3 = false;
              s.W3 = static_cast<T*>(g_pool.get(s.dev, sizeof(T) * nn, &f3));  // the factor L: every tile read has been written
            }
            s.dag_ctrl = palloc<int>(s.dev, dag_ctrl_regions_ * dag_ctrl_bytes / sizeof(int));
            HIPCHECK(hipMemsetAsync(s.dag_ctrl, 0, dag_ctrl_regions_ * dag_ctrl_bytes, slots[di][0].stream));
            if (getenv("HBEGP_DAG_TRACE")) {
              s.dag_trace = palloc<unsigned long long>(s.dev, 5 * plan.tasks.size());
              HIPCHECK(hipMemsetAsync(s.dag_trace, 0, sizeof(unsigned long long) * 5 * plan.tasks.size(), slots[di][0].stream));
            }
          }
          HIPCHECK(hipStreamSynchronize(slots[di][0].stream));  // the copies and fills above; the other slots' streams do not wait for this one
        }
      }
    }
    // the static GEMM schedules (per device; shared by its slots): eval_gemms walked with a dispatcher that records instead of
    // launching, so that the i-th launch of an evaluation finds its schedule at index i
    scheds.resize(c->devs.size());
    if (adhoc_ || small_) return;
    for (size_t di = 0; di < c->devs.size(); ++di) {
      HIPCHECK(hipSetDevice(c->devs[di]));
      Slot<T>& s = slots[di][0];
      auto record = [&](GemmLaunch& g, int) {
        Sched sc;
        sc.tile = pick_tile(g);
        std::vector<int> off;
        std::vector<unsigned> items;
        int nwg = 0;
        if (build_sched(g, sc.tile, &off, &items, &nwg)) {
          sc.nwg = nwg;
          sc.d_off = palloc<int>(s.dev, off.size());
          sc.d_items = palloc<unsigned>(s.dev, items.size());
          HIPCHECK(hipMemcpyAsync(sc.d_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, s.stream));
          HIPCHECK(hipMemcpyAsync(sc.d_items, items.data(), sizeof(unsigned) * items.size(), hipMemcpyHostToDevice, s.stream));
          HIPCHECK(hipStreamSynchronize(s.stream));  // off / items are locals
        }
        scheds[di].push_back(sc);
      };
      eval_gemms(s, s.Kinv[0], record, [](int) {}, [] {});
    }
  }
  ~Problem() override { release(); }

  // HBEGP_DAG_TRACE=<prefix> with HBEGP_DAG_TRACE_EVALS=a:b (fits only): the task trace of every task-queue launch a slot makes for
  // its evaluations number a .. b-1, while the other slots run theirs beside it -- what tools/queue_workers.py reads to count the
  // compute units a launch really holds.  Kept in memory (one copy per launch; the slot's stream is idle, the evaluation has been
  // published) and written by release() to <prefix>.s<slot>.e<evaluation>.p<part>: a header line, then tools/dag_trace.py's
  // columns with the task's flags behind them.
  void keep_fit_trace(Slot<T>& s, int mode) {
    static const char* range = getenv("HBEGP_DAG_TRACE_EVALS");
    int a = 0, b = 0;
    if (!range || !dag_ || !s.dag_trace || sscanf(range, "%d:%d", &a, &b) != 2 || s.seq < (unsigned long long)std::max(a, 0) || s.seq >= (unsigned long long)std::max(b, 0)) return;
    const int part = !(lazy_ && dag_lauum_) ? 0 : (mode == EVAL_LML_ONLY ? 1 : (mode == EVAL_GRAD_ONLY ? 2 : 0));
    const DagVariant& var = dag_var[s.dag_variant];
    typename Slot<T>::KeptTrace k;
    k.seq = s.seq; k.part = part; k.variant = s.dag_variant;
    k.nwg = part == 1 ? var.nwg_p1 : (part == 2 ? var.nwg_kinv : var.nwg);
    k.stamps.resize((size_t)5 * (part == 1 ? var.ntasks_p1 : (part == 2 ? var.ntasks_kinv : dag_ntasks)));
    HIPCHECK(hipMemcpyAsync(k.stamps.data(), s.dag_trace, sizeof(unsigned long long) * k.stamps.size(), hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    s.kept_traces.push_back(std::move(k));
  }
  void write_fit_traces() {
    const char* prefix = getenv("HBEGP_DAG_TRACE");
    for (size_t di = 0; prefix && di < slots.size(); ++di)
      for (size_t si = 0; si < slots[di].size(); ++si)
        for (const auto& k : slots[di][si].kept_traces) {
          if (k.variant < 0 || k.variant >= (int)dag_var.size()) continue;
          const DagVariant& var = dag_var[k.variant];
          const std::vector<DagTask>& tasks = k.part == 1 ? var.host_tasks_p1 : (k.part == 2 ? var.host_tasks_kinv : var.host_tasks);
          char name[512];
          snprintf(name, sizeof name, "%s.s%zu.e%llu.p%d", prefix, si, k.seq, k.part);
          FILE* f = fopen(name, "w");
          if (!f) continue;
          fprintf(f, "# slot %zu evaluation %llu part %d variant %d share %d nwg %d tasks %zu\n", si, k.seq, k.part, k.variant, share_of_variant(k.variant), k.nwg, tasks.size());
          for (size_t i = 0; i < tasks.size() && 5 * i + 4 < k.stamps.size(); ++i) {
            const DagTask& t = tasks[i];
            const unsigned long long* tr = k.stamps.data() + 5 * i;
            fprintf(f, "%zu %d %d %d %d %d %llu %llu %llu %llu %llu %llu %d\n", i, t.kind, t.row0, t.col0, t.kend - t.kbeg, t.nwait, tr[0], tr[1], tr[2], tr[3], tr[4] >> 32,
                    tr[4] & 0xffffffffull, t.flags);
          }
          fclose(f);
        }
  }

  void release() {
    write_fit_traces();
    for (size_t di = 0; di < slots.size(); ++di) {
      (void)hipSetDevice(ctx->devs[di]);
      for (auto& s : slots[di]) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        for (int v = 0; v <= DAG_MAX_VARIANTS + DAG_CROWD_LEVELS + DAG_SHARE_VARIANTS; ++v)
          for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 4; ++b)
              if (s.graph[v][a][b]) (void)hipGraphExecDestroy(s.graph[v][a][b]);
        const size_t nnb = sizeof(T) * (size_t)np * np;
        g_pool.put(s.dev, s.W1, nnb); g_pool.put(s.dev, s.W2, nnb); g_pool.put(s.dev, s.W3, nnb);
        for (int b = 0; b < 2; ++b) g_pool.put(s.dev, s.Kinv[b], nnb);
        g_pool.put(s.dev, s.small_slab, s.small_slab_bytes);
        g_host_pool.put(s.host_slab, s.host_slab_bytes);
        g_stream_pool.put(s.dev, s.stream);  // synchronised above
      }
    }
    for (const Pooled& q : pooled_) g_pool.put(q.dev, q.p, q.bytes);  // features, targets, task queues, control words, schedule tables
    pooled_.clear();
    slots.clear();
    scheds.clear();
    dag_var.clear();
    Xd.clear();
    yd.clear();
    rvd.clear();
  }

  // The GEMMs of an evaluation of the launch path are issued by this dispatcher: the i-th launch by the i-th static schedule
  // (init records them by walking eval_gemms); a single-shot problem has no table and issues them ad hoc.
  auto scheduled(Slot<T>& s, size_t di, PhaseTimer* tm, int ord0 = 0) {
    return [this, &s, di, tm, ord = ord0](GemmLaunch& g, int kind) mutable {
      if (adhoc_) return gemm_adhoc<T>(g, &s.dOut->info, s.stream);
      const Sched& sc = scheds[di][ord++];
      g.info = &s.dOut->info;
      g.sched_off = sc.nwg ? sc.d_off : nullptr;
      g.sched_items = sc.nwg ? sc.d_items : nullptr;
      g.sched_nwg = sc.nwg;
      double gf = 0;
      if (tm)
        for (int i = 0; i < g.nops; ++i) gf += op_gflop(g.op[i]);
      if (tm) tm->begin(kind, sc.tile, gf);
      launch_gemm<T>(g, sc.tile, s.stream);
      if (tm) tm->end();
    };
  }

  // Workgroups of the two launches of a lazily evaluated trial (part 1: the queue without K^-1 tasks, 2: the K^-1 tasks alone):
  // the fused launch's count of the same variant, which is the measured optimum for both (config M, three slots, fits/s;
  // profiles/lazy_grad_workgroups_per_launch.txt): phase 1 at 80 / 88 / 96 / 104 / 112 / 128 -> 1.896 / 1.924 / 1.936 / 1.830 / 1.801 /
  // 1.702 -- as sharp as the fused launch's, for the same reason: three launches share 256 CUs; K^-1 alone at 48 / 64 / 80 / 96 / 112 /
  // 128 / 160 -> 1.714 / 1.858 / 1.899 / 1.936 / 1.923 / 1.930 / 1.926 -- flat from 96 on.  HBEGP_DAG_WG_P1 / HBEGP_DAG_WG_KINV force a
  // count (the sweep's knobs).
  static int lazy_wg(int fused_nwg, int part) {
    const int forced = env_int(part == 1 ? "HBEGP_DAG_WG_P1" : "HBEGP_DAG_WG_KINV", 0);
    return forced > 0 ? forced : fused_nwg;
  }

  // the diagonal-block step of the fit's chol_inv_rec: X_kk -> W2, diag(L_kk) -> ldiag
  auto leaf_step(Slot<T>& s, PhaseTimer* tm) {
    return [this, &s, tm](int k) {
      if (tm) tm->begin(PhaseTimer::LEAF);
      launch_leaf<T>(s.W1, s.W2, np, k, s.ldiag, &s.dOut->info, s.stream, leaf_dbg_);
      if (tm) tm->end();
    };
  }

  // The GEMM launches of one evaluation of the launch path in order, and what runs between them: the factorisation
  // (chol_inv_rec; the task queue, launched before, does it instead), `alpha`, then K^-1 = X^T X.  Walked once with a recording
  // dispatcher to build the schedule table, then with the scheduled one for every evaluation.
  // (round 1: a right-looking sweep over 512- / 1024-wide big blocks in front of the recursion -- 3.55 vs 3.43 ms per evaluation at
  // n = 4096, removed in round 5)
  // part: 0 the whole evaluation | 1 without K^-1 (first phase of a lazily evaluated trial) | 2 K^-1 alone (its second phase: the
  // LAUUM launch is the LAST of the sequence, so a dispatcher that starts at scheds[di].size() - 1 hands it its own schedule)
  template <class Gemm, class Leaf, class Alpha>
  void eval_gemms(Slot<T>& s, T* Kinv, Gemm&& gemm, Leaf&& leaf, Alpha&& alpha, int part = 0) {
    const int nb = np / NB;
    if (part != 2) {
      if (!dag_) chol_inv_rec<T>(s.W1, s.W2, s.W2, np, 0, nb / 2, nb, false, true, gemm, leaf);
      alpha();
    }
    if (part != 1 && !(dag_ && dag_lauum_)) {
      // K^-1 = X^T X (lower)  [LAUUM]   (task-queue path: tiles of the same queue, dag_plan.hpp build_lauum)
      GemmLaunch g{};
      g.nops = 1;
      GemmOp& op = g.op[0];
      op.lda = op.ldb = op.ldc = np;
      op.A = s.W2; op.B = s.W2; op.C = Kinv;
      op.a_kmajor = 1; op.b_kmajor = 1;
      op.ci0 = 0; op.cj0 = 0; op.mi = nb; op.nj = nb; op.c_lower = 1;
      op.k0 = 0; op.k1 = nb; op.klim = 4; op.maskA = 1; op.maskB = 1;
      gemm(g, PhaseTimer::LAUUM);
    }
  }

  // Diagnostics of a wait that exceeded its bound (a scheduling bug, never a data property): which task gave up, and
  // where its counters stood.
  void dag_report_timeout(Slot<T>& s) {
    if (!s.dag_ctrl) return;
    std::vector<int> ctrl(dag_ctrl_bytes / sizeof(int));
    if (hipMemcpyAsync(ctrl.data(), s.dag_ctrl + (s.dag_part == 2 ? dag_ctrl_bytes / sizeof(int) : 0), dag_ctrl_bytes, hipMemcpyDeviceToHost, s.stream) != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess) return;
    const int row = ctrl[1] - 1;
    const DagVariant& var = dag_var[s.dag_variant];
    const int ntasks_here = s.dag_part == 1 ? var.ntasks_p1 : (s.dag_part == 2 ? var.ntasks_kinv : dag_ntasks);
    fprintf(stderr, "task queue timeout: queue head %d of %d, first task that gave up: %d\n", ctrl[0], ntasks_here, row);
    const std::vector<DagTask>& host_tasks = s.dag_part == 1 ? var.host_tasks_p1 : (s.dag_part == 2 ? var.host_tasks_kinv : var.host_tasks);
    if (row >= 0 && row < (int)host_tasks.size()) {
      const DagTask& t = host_tasks[row];
      fprintf(stderr, "  kind %d flags %x row0 %d col0 %d k [%d, %d) waits:", t.kind, t.flags, t.row0, t.col0, t.kbeg, t.kend);
      for (int w = 0; w < t.nwait; ++w) fprintf(stderr, " c%d=%d/%d", t.wcnt[w], ctrl[DAG_CTRL_WORDS + t.wcnt[w]], t.wval[w]);
      fprintf(stderr, "\n");
    }
    (void)hipGetLastError();
  }

  // The factorisation as ONE persistent launch of the task queue: workgroups pull diagonal-block and tile tasks from an ordered
  // queue.  With dag_lauum_ its tiles of K^-1 = X^T X go to Kinv (null: factorisation only).
  // part: 0 the variant's full queue | 1 its queue without the K^-1 tasks | 2 its K^-1 tasks alone (X = L^-1 complete in W2)
  void launch_queue(Slot<T>& s, size_t di, T* Kinv, PhaseTimer* tm, int part = 0) {
    // (part 2: its own region of control words, clear since the first phase's kernel-matrix launch)
    if (part != 2 && !s.ctrl_cleared) HIPCHECK(hipMemsetAsync(s.dag_ctrl, 0, dag_ctrl_regions_ * dag_ctrl_bytes, s.stream));
    if (part != 2) s.ctrl_cleared = false;
    DagLaunch g{};
    const DagVariant& var = dag_var[s.dag_variant];
    g.tasks = var.tasks[di]; g.ntasks = dag_ntasks; g.ctrl = s.dag_ctrl;
    int nwg = var.nwg;
    s.dag_part = part;
    if (part == 1) { g.tasks = var.tasks_p1[di]; g.ntasks = var.ntasks_p1; nwg = var.nwg_p1; }
    if (part == 2) { g.tasks = var.tasks_kinv[di]; g.ntasks = var.ntasks_kinv; nwg = var.nwg_kinv; g.ctrl = s.dag_ctrl + dag_ctrl_bytes / sizeof(int); }
    g.W1 = s.W1; g.W2 = s.W2; g.ld = np; g.ldiag = s.ldiag; g.info = &s.dOut->info;
    g.W3 = s.W3;
    g.Kinv = (dag_lauum_ && part != 1) ? Kinv : nullptr;
    g.trace = s.dag_trace;
    g.wait_ticks = dag_wait_ticks_;
    g.leaf_dbg = leaf_dbg_;
    g.zero_skip = zero_skip_ ? 1 : 0;
    if (tm) tm->begin(PhaseTimer::DAG, 0, part == 2 ? dag_gflop_lauum : (g.Kinv ? dag_gflop : dag_gflop - dag_gflop_lauum));
    launch_dag<T>(g, nwg, s.stream);
    if (tm) tm->end();
  }

  void small_eval(Slot<T>& s, size_t di, int target, int mode) {
    SmallEval g{};
    g.X = Xd[di]; g.y = yd[di]; g.n = n; g.d = d;
    g.W2 = s.W2; g.ldiag = s.ldiag; g.Kinv = s.Kinv[target]; g.alpha = s.alpha[target]; g.out = s.dOut; g.mode = mode;
    // The kernel reads the parameters from, and writes its few scalar results to, the slot's pinned host blocks itself: the
    // captured graph of an evaluation is ONE node (no parameter copy, no reset kernel, no result copy -- each was ~2-5 us of
    // a 57 us evaluation).
    g.P = s.hP; g.hout = s.hOut;
    launch_small_eval<T>(g, rvd[di], nu2, s.stream);
  }

  // What one enqueued evaluation computes.  The first two are what `want_grad` = false / true always were (the index of the
  // captured graph is the mode); the last two are the phases of a lazily evaluated line-search trial (lazy_, do_fit):
  // EVAL_LML_ONLY = kmat, factorisation and inverse factor, alpha / lml, publish -- no K^-1; EVAL_GRAD_ONLY = on what that left
  // in W2, alpha[target] and dP: the K^-1 tiles into Kinv[target], gradtrace / finalize_grad, publish again.
  enum EvalMode { EVAL_LML_KINV = 0, EVAL_FULL = 1, EVAL_LML_ONLY = 2, EVAL_GRAD_ONLY = 3 };

  void enqueue_eval(Slot<T>& s, size_t di, int target, int mode, PhaseTimer* tm) {
    const int* info = &s.dOut->info;
    const bool want_grad = mode == EVAL_FULL || mode == EVAL_GRAD_ONLY;
    if (mode == EVAL_GRAD_ONLY) {
      // second phase: nothing in front of the K^-1 tiles (the queue's control words are a region of their own, still clear)
      if (dag_ && dag_lauum_) launch_queue(s, di, s.Kinv[target], tm, 2);
      else eval_gemms(s, s.Kinv[target], scheduled(s, di, tm, (int)scheds[di].size() - 1), leaf_step(s, tm), [] {}, 2);
      const bool fuse_grad = (np / 64) * (np / 64 + 1) / 2 <= 512;  // as below
      if (tm) tm->begin(PhaseTimer::GRAD);
      launch_gradtrace<T>(Xd[di], n, d, np, nu2, s.dP, s.Kinv[target], s.alpha[target], s.part_g, s.dOut, info, s.stream,
                          fuse_grad ? s.tickets + 1 : nullptr, fuse_grad ? s.hOut : nullptr);
      if (tm) tm->end();
      if (!fuse_grad) launch_publish_out(s.dOut, s.hOut, s.dP, s.stream);
      s.published = true;
      CHECK_LAUNCHES();
      return;
    }
    const int part = mode == EVAL_LML_ONLY ? 1 : 0;
    if (small_) {
      if (tm) tm->begin(PhaseTimer::LEAF);
      small_eval(s, di, target, 1 | 2 | (want_grad ? 4 : 0));
      if (tm) tm->end();
      CHECK_LAUNCHES();
      return;
    }
    const bool hostio = eval_published();
    if (hostio) {
      EvalPrologue pro;
      pro.dP = s.dP; pro.out = s.dOut;
      if (dag_) {
        pro.ctrl = s.dag_ctrl; pro.ctrl_words = (int)(dag_ctrl_regions_ * dag_ctrl_bytes / sizeof(int));
        s.ctrl_cleared = true;
      }
      if (tm) tm->begin(PhaseTimer::KMAT);
      launch_kmat<T>(Xd[di], rvd[di], n, d, np, nu2, s.hP, s.W1, info, s.stream, &pro);
      if (tm) tm->end();
    } else {
      HIPCHECK(hipMemcpyAsync(s.dP, s.hP, sizeof(EvalParams), hipMemcpyHostToDevice, s.stream));
      launch_reset_out(s.dOut, s.stream);
      if (tm) tm->begin(PhaseTimer::KMAT);
      launch_kmat<T>(Xd[di], rvd[di], n, d, np, nu2, s.dP, s.W1, info, s.stream);
      if (tm) tm->end();
    }
    if (dag_) launch_queue(s, di, s.Kinv[target], tm, dag_lauum_ ? part : 0);
    eval_gemms(s, s.Kinv[target], scheduled(s, di, tm), leaf_step(s, tm), [&] {
      if (tm) tm->begin(PhaseTimer::ALPHA);
      launch_alpha_lml<T>(s.W2, np, n, yd[di], s.ldiag, s.wbuf, s.part_t, s.alpha[target], s.dOut, info, s.stream, hostio ? s.tickets : nullptr);
      if (tm) tm->end();
    }, part);
    bool fuse_grad = false;
    if (want_grad) {
      if (tm) tm->begin(PhaseTimer::GRAD);
      // hostio: the launch's last workgroup also finalises the gradient and publishes the evaluation -- where the launch is a
      // few hundred workgroups (latency-bound sizes).  Every workgroup drains its write-through partials before it takes its
      // ticket (~2 us at the end of its life): with the 2,080 workgroups of n = 4096 queueing for the ~60 CUs the other two
      // task-queue launches leave free that made the launch 138 -> 182 us; there the two tiny launches behind it are free.
      fuse_grad = hostio && (np / 64) * (np / 64 + 1) / 2 <= 512;
      launch_gradtrace<T>(Xd[di], n, d, np, nu2, s.dP, s.Kinv[target], s.alpha[target], s.part_g, s.dOut, info, s.stream,
                          fuse_grad ? s.tickets + 1 : nullptr, fuse_grad ? s.hOut : nullptr);
      if (tm) tm->end();
    }
    if (hostio) {
      if (!want_grad || !fuse_grad) launch_publish_out(s.dOut, s.hOut, s.dP, s.stream);
      s.published = true;
    }
    CHECK_LAUNCHES();
    if (!hostio) {
      HIPCHECK(hipMemcpyAsync(s.hOut, s.dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s.stream));
      s.published = false;
    }
  }

  // The host side of the end of an evaluation.  Published evaluations (HBEGP_HOSTIO): spin on the serial number the last kernel
  // stores into the pinned result block behind a system-scope fence; hipStreamSynchronize sleeps on an interrupt and wakes up
  // ~50 us late, which three optimiser runs pay 150 times each.  A kernel that faults never publishes: after two seconds the
  // thread falls back to hipStreamSynchronize, which reports the fault (or simply waits for a very long evaluation).
  // Long evaluations are slept through first: the thread remembers how long this slot's last evaluation took (they are all
  // alike) and, from 1.5 ms on, sleeps until an eighth of it (at least 300 us) before that: a fit at n = 4096 then keeps 1.4 cores busy
  // instead of 4 (hipStreamSynchronize spins as well: 4 cores with HBEGP_HOSTIO=0 too; tools/cpu_cost_probe.py).  A sleep that ran past the end shortens the next one.
  void wait_eval(Slot<T>& s, std::chrono::steady_clock::time_point t_launch, int mode) {
    long long& expect_ns = s.expect_ns[mode];
    if (s.published) {
      using namespace std::chrono;
      const volatile unsigned long long* q = &s.hOut->seq;
      if (expect_ns > 1500000) {  // below ~1.5 ms a timer's wake-up jitter (50-100 us) costs more than it saves: n=512 fits 29.7 -> 21.6 /s with a 0.4 ms threshold
        const long long margin = std::max<long long>(300000, expect_ns / 8);  // concurrent runs stretch each other by a few per cent, unevenly
        std::this_thread::sleep_until(t_launch + nanoseconds(expect_ns - margin));
        if (*q == s.seq) {  // slept too long: the measurement below would include the oversleep
          std::atomic_thread_fence(std::memory_order_acquire);
          expect_ns = expect_ns * 9 / 10;
          return;
        }
      }
      const auto t0 = steady_clock::now();
      for (unsigned it = 1;; ++it) {
        if (*q == s.seq) {
          std::atomic_thread_fence(std::memory_order_acquire);
          expect_ns = duration_cast<nanoseconds>(steady_clock::now() - t_launch).count();
          return;
        }
        __builtin_ia32_pause();
        if ((it & 4095u) == 0 && steady_clock::now() - t0 > seconds(2)) {
          // never in normal operation: a faulted kernel, an evaluation longer than two seconds, or a mismatch between what was
          // captured and what run_eval expects (eval_published) -- say so once, the fallback below still returns the result
          static std::atomic<bool> said{false};
          if (!said.exchange(true))
            fprintf(stderr, "hbegp: an evaluation did not publish its serial number within 2 s; falling back to hipStreamSynchronize\n");
          break;
        }
      }
    }
    HIPCHECK(hipStreamSynchronize(s.stream));
  }

  // Kernel matrix + Cholesky/inverse-factor recursion only (no alpha, no K^-1): leaves X = L^-1 in the slot's W2.
  // Used when a model is built: X of the captured theta is recomputed (bitwise the same arithmetic as in the evaluation, from the
  // same parameters: a device-driven fit hands over the numbers its evaluation ran with, SmallFitResult::best_params).
  int factor_only(size_t di, int si) {
    Slot<T>& s = slots[di][si];
    HIPCHECK(hipSetDevice(s.dev));
    s.dag_variant = variant_now(di);
    HIPCHECK(hipMemcpyAsync(s.dP, s.hP, sizeof(EvalParams), hipMemcpyHostToDevice, s.stream));
    launch_reset_out(s.dOut, s.stream);
    if (small_) {
      small_eval(s, di, 0, 0);  // factor + inverse factor only: alpha and K^-1 of the captured evaluation stay as they are
      CHECK_LAUNCHES();
      HIPCHECK(hipStreamSynchronize(s.stream));
      return s.hOut->info != 0 ? HBEGP_NOT_PD : HBEGP_OK;
    }
    launch_kmat<T>(Xd[di], rvd[di], n, d, np, nu2, s.dP, s.W1, &s.dOut->info, s.stream);
    // the captured K^-1 stays as it is; the recursion's launches are the first ones of eval_gemms, whose schedules they take
    const int nb = np / NB;
    if (dag_) launch_queue(s, di, nullptr, nullptr);
    else chol_inv_rec<T>(s.W1, s.W2, s.W2, np, 0, nb / 2, nb, false, true, scheduled(s, di, nullptr), leaf_step(s, nullptr));
    CHECK_LAUNCHES();
    HIPCHECK(hipMemcpyAsync(s.hOut, s.dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    if (s.hOut->info < 0) {
      dag_report_timeout(s);
      throw HipError{hipErrorLaunchTimeOut, "factorisation task queue: a dependency wait exceeded its bound", __LINE__};
    }
    return s.hOut->info != 0 ? HBEGP_NOT_PD : HBEGP_OK;
  }

  // Incremental extend (the reference refactorises from scratch, fit.rs:33-68): the prior model was
  // built at the same theta on a prefix of these rows, so the leading q0 = floor(n_prior / 128) diagonal blocks of L,
  // X = L^-1 and the matching block of K^-1 are reused:
  //   [X11 0; X21 X22]:  T = A21 X11^T,  A22 -= T T^T,  U = T X11,  chol_inv(A22),  X21 = -X22 U          O(n^2 k)
  //   K^-1 = [K11^-1 + X21^T X21, .; X22^T X21, X22^T X22]                                                   O(n^2 k)
  // Results go to ping-pong buffer 0 of slot (di, si).  Returns HBEGP_EINVAL when nothing can be reused.
  // prv: the prior's known row variances (pn entries) or null; a side without them counts as zeros
  int extend_from(size_t di, int si, const T* pX, const T* prv, const T* pXinv, const T* pKinv, const T* pldiag, int pn, int pnp) {
    Slot<T>& s = slots[di][si];
    HIPCHECK(hipSetDevice(s.dev));
    const int nb = np / NB, q0 = std::min(pn / NB, nb - 1);
    if (q0 < 1 || pn > n) return HBEGP_EINVAL;
    const int* info = &s.dOut->info;
    HIPCHECK(hipMemcpyAsync(s.dP, s.hP, sizeof(EvalParams), hipMemcpyHostToDevice, s.stream));
    launch_reset_out(s.dOut, s.stream);
    // same leading rows?  (only the kept blocks matter, compare the whole prior prefix anyway)
    launch_prefix_differs<T>(Xd[di], pX, (size_t)pn * d, &s.dOut->n_warn, s.stream);
    if (rvd[di] || prv) {
      const T* zeros = nullptr;
      if (!rvd[di] || !prv) {
        // one side has no v: it is compared as zeros.  The block is the problem's (palloc): it lives until release(), past the launch
        T* z = palloc<T>(s.dev, pn);
        HIPCHECK(hipMemsetAsync(z, 0, sizeof(T) * pn, s.stream));
        zeros = z;
      }
      launch_prefix_differs<T>(rvd[di] ? rvd[di] : zeros, prv ? prv : zeros, (size_t)pn, &s.dOut->n_warn, s.stream);
    }
    CHECK_LAUNCHES();
    HIPCHECK(hipMemcpyAsync(s.hOut, s.dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    if (s.hOut->n_warn != 0) {
      HIPCHECK(hipMemsetAsync(&s.dOut->n_warn, 0, sizeof(int), s.stream));
      return HBEGP_EINVAL;
    }
    const size_t w = (size_t)q0 * NB;
    HIPCHECK(hipMemcpy2DAsync(s.W2, sizeof(T) * np, pXinv, sizeof(T) * pnp, sizeof(T) * w, w, hipMemcpyDeviceToDevice, s.stream));
    HIPCHECK(hipMemcpy2DAsync(s.Kinv[0], sizeof(T) * np, pKinv, sizeof(T) * pnp, sizeof(T) * w, w, hipMemcpyDeviceToDevice, s.stream));
    HIPCHECK(hipMemcpyAsync(s.ldiag, pldiag, sizeof(T) * w, hipMemcpyDeviceToDevice, s.stream));
    launch_kmat<T>(Xd[di], rvd[di], n, d, np, nu2, s.dP, s.W1, info, s.stream);
    // a launch sequence other than the evaluation's: every GEMM ad hoc
    chol_inv_rec<T>(s.W1, s.W2, s.W2, np, 0, q0, nb, true, true, [&](GemmLaunch& g, int) { gemm_adhoc<T>(g, info, s.stream); },
                    leaf_step(s, nullptr));
    launch_alpha_lml<T>(s.W2, np, n, yd[di], s.ldiag, s.wbuf, s.part_t, s.alpha[0], s.dOut, info, s.stream);
    if (pnp / NB > q0) {
      // the prior's K^-1 also holds X^T X contributions of its own trailing (partial) block, which is being replaced:
      // take them out of the kept block first
      GemmLaunch gf{};
      gf.nops = 1;
      GemmOp& fix = gf.op[0];
      fix.A = pXinv; fix.B = pXinv; fix.C = s.Kinv[0];
      fix.lda = fix.ldb = pnp; fix.ldc = np;
      fix.a_kmajor = 1; fix.b_kmajor = 1;
      fix.mi = fix.nj = q0; fix.c_lower = 1;
      fix.k0 = q0; fix.k1 = pnp / NB; fix.alpha_neg = 1; fix.beta_one = 1;
      gemm_adhoc<T>(gf, info, s.stream);
    }
    GemmLaunch g{};
    GemmOp base{};
    base.lda = base.ldb = base.ldc = np;
    base.A = s.W2; base.B = s.W2; base.C = s.Kinv[0];
    base.a_kmajor = 1; base.b_kmajor = 1;
    base.k0 = q0; base.k1 = nb; base.maskA = 1; base.maskB = 1;
    GemmOp& keep = g.op[g.nops++];   // kept block: += X21^T X21
    keep = base; keep.mi = keep.nj = q0; keep.c_lower = 1; keep.beta_one = 1;
    GemmOp& rect = g.op[g.nops++];   // new rows x kept columns: X22^T X21 (k >= i)
    rect = base; rect.ci0 = q0; rect.mi = nb - q0; rect.nj = q0; rect.klim = 4;
    GemmOp& tri = g.op[g.nops++];    // new rows x new columns (lower)
    tri = base; tri.ci0 = tri.cj0 = q0; tri.mi = tri.nj = nb - q0; tri.c_lower = 1; tri.klim = 4;
    gemm_adhoc<T>(g, info, s.stream);
    CHECK_LAUNCHES();
    HIPCHECK(hipMemcpyAsync(s.hOut, s.dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    s.last_target = 0;
    if (s.hOut->info == 0 && !(s.hOut->done & 1)) throw HipError{hipErrorLaunchFailure, "extend: the evaluation kernels did not run", __LINE__};
    // a non-finite lml (a NaN target: the factor itself is fine) is handled like a failed factorisation, as run_eval handles it on
    // the full path: no model with NaN alpha and lml is handed out
    if (s.hOut->info == 0 && !std::isfinite(s.hOut->lml)) return HBEGP_NOT_PD;
    return s.hOut->info != 0 ? HBEGP_NOT_PD : HBEGP_OK;
  }

  // The task-queue variant for an evaluation that starts now on device di: sized for the slots that are inside an optimiser
  // run at this moment (a fit keeps the count; outside a fit every slot is assumed busy).
  // si >= 0: the slot that starts the evaluation, inside a fit's optimiser run -- the one caller for which the share policy
  // (slot_share.hpp) is asked, and only when every slot of the problem is busy on the device, each with a run of its own, and the
  // device is not crowded.  Everything else gets the busy-count / crowded-device variant as ever.
  int variant_now(size_t di, int si = -1) const {
    if (!dag_ || dag_var.size() < 2) return 1;
    const int nvar = dag_nvar_;
    const int busy = busy_slots_ ? busy_slots_[di].load(std::memory_order_relaxed) : 0;
    if (dag_ncrowd_ > 0) {
      // runs in flight on this GPU over ALL fits of the process: beyond what this fit alone accounts for, the device is crowded
      const int dev = ctx->devs[di];
      const int total = dev < MAX_DEVS ? g_dev_busy[dev].load(std::memory_order_relaxed) : 0;
      if (total > std::max(busy, nvar)) {
        int l = 0;
        while (l + 1 < dag_ncrowd_ && DAG_CROWD_BUSY[l] < total) ++l;
        return nvar + 1 + l;
      }
    }
    if (si >= 0 && dag_nshare_ > 0 && ctx->devs[di] < MAX_DEVS && g_dev_fits[ctx->devs[di]].load(std::memory_order_relaxed) > 1)
      not_alone_.store(1, std::memory_order_relaxed);
    if (si >= 0 && dag_nshare_ > 0 && busy == n_slots && n_slots >= 2 && n_slots <= SLOT_SHARE_MAX_SLOTS && balance_dev_[di] &&
        !not_alone_.load(std::memory_order_relaxed)) {
      int share[SLOT_SHARE_MAX_SLOTS];
      if (!share_force_.empty()) {
        for (int i = 0; i < n_slots; ++i) share[i] = share_force_[i];
      } else {
        int running[SLOT_SHARE_MAX_SLOTS], done[SLOT_SHARE_MAX_SLOTS], cap[SLOT_SHARE_MAX_SLOTS];
        for (int i = 0; i < n_slots; ++i) {
          running[i] = slot_running_[di * n_slots + i].load(std::memory_order_relaxed);
          done[i] = slot_done_[di * n_slots + i].load(std::memory_order_relaxed);
          cap[i] = slot_maxeval_;
        }
        slot_shares(n_slots, running, done, cap, share_hyst_, share);
      }
      if (share[si] != SLOT_SHARE_EVEN) return nvar + dag_ncrowd_ + (share[si] == SLOT_SHARE_LEAD ? 1 : 2);
    }
    return busy <= 0 ? nvar : std::min(busy, nvar);
  }
  // SLOT_SHARE_LEAD / _LAG when variant v is one of the two unequal shares, SLOT_SHARE_EVEN otherwise
  int share_of_variant(int v) const {
    if (!dag_ || dag_nshare_ <= 0 || v <= dag_nvar_ + dag_ncrowd_) return SLOT_SHARE_EVEN;
    return v == dag_nvar_ + dag_ncrowd_ + 1 ? SLOT_SHARE_LEAD : SLOT_SHARE_LAG;
  }
  // Run one evaluation on (device index di, slot si) into ping-pong buffer `target`; blocks until the result is on the host.
  // mode: EvalMode (a bool converts as it always meant: false = lml + K^-1, true = the whole evaluation).  EVAL_GRAD_ONLY continues
  // the slot's last EVAL_LML_ONLY evaluation (same target, parameters still in dP): *lml is not touched, grad must not be null.
  int run_eval(size_t di, int si, int target, int mode, bool use_graph, double* lml, double* grad, bool in_run = false) {
    Slot<T>& s = slots[di][si];
    HIPCHECK(hipSetDevice(s.dev));
    static const bool graphs_on = env_int("HBEGP_NO_GRAPH", 0) == 0;
    const bool want_grad = mode == EVAL_FULL || mode == EVAL_GRAD_ONLY;
    if (mode == EVAL_GRAD_ONLY) {
      // the same evaluation, published a second time under the same serial number (dP still carries it): the host takes the
      // number back first, so that the word it spins on changes again when the second phase is over.  The queue variant stays the
      // first phase's: both phases of a trial come from one plan.
      if (!lazy_ || !eval_published() || !grad) throw std::logic_error("run_eval: the gradient phase needs a lazily evaluated, published problem");
      reinterpret_cast<volatile unsigned long long*>(&s.hOut->seq)[0] = 0;
      std::atomic_thread_fence(std::memory_order_seq_cst);
    } else {
      s.dag_variant = variant_now(di, in_run ? si : -1);
      s.hP->seq = ++s.seq;
    }
    const auto t_launch = std::chrono::steady_clock::now();
    if (use_graph && graphs_on) {
      hipGraphExec_t& ge = s.graph[s.dag_variant][target][mode];
      if (!ge) {
        hipGraph_t gr = nullptr;
        HIPCHECK(hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal));
        try {
          enqueue_eval(s, di, target, mode, nullptr);
        } catch (...) {
          (void)hipStreamEndCapture(s.stream, &gr);
          throw;
        }
        HIPCHECK(hipStreamEndCapture(s.stream, &gr));
        HIPCHECK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
        HIPCHECK(hipGraphDestroy(gr));
      }
      HIPCHECK(hipGraphLaunch(ge, s.stream));
    } else {
      enqueue_eval(s, di, target, mode, nullptr);
    }
    s.published = eval_published();  // what enqueue_eval records when it is not replayed from a graph (ONE rule for both: eval_published)
    wait_eval(s, t_launch, mode);
    if (s.dag_trace) keep_fit_trace(s, mode);
    s.last_target = target;
    const int p = d + 2;
    if (s.hOut->info < 0) {
      dag_report_timeout(s);
      throw HipError{hipErrorLaunchTimeOut, "factorisation task queue: a dependency wait exceeded its bound", __LINE__};
    }
    if (s.hOut->info != 0) {
      if (mode != EVAL_GRAD_ONLY) *lml = -std::numeric_limits<double>::infinity();
      if (grad) for (int j = 0; j < p; ++j) grad[j] = 0.0;  // fit.rs:105-112
      return HBEGP_NOT_PD;
    }
    double lml_kept = s.hOut->lml;
    if (mode == EVAL_GRAD_ONLY) lml = &lml_kept;  // (already handed out by the first phase; checked again below all the same)
    // the evaluation starts by poisoning its outputs and clearing `done`: a kernel that was skipped cannot pass for a result
    if (!(s.hOut->done & 1) || (want_grad && !(s.hOut->done & 2)))
      throw HipError{hipErrorLaunchFailure, "evaluation: the lml/gradient kernels did not run", __LINE__};
    *lml = s.hOut->lml;
    if (grad) for (int j = 0; j < p; ++j) grad[j] = s.hOut->grad[j];
    // the outputs were poisoned with NaN before the launches: a block of the gradient reduction that never ran, or a genuinely
    // non-finite trace, must not reach the optimiser as a number
    bool finite = std::isfinite(*lml);
    if (grad) for (int j = 0; j < p; ++j) finite = finite && std::isfinite(grad[j]);
    if (!finite) {
      // Which of the two?  launch_reset_out poisons the outputs with ONE bit pattern (a quiet NaN with payload 0x5eed) that no
      // arithmetic produces: an output that still carries it was never written -- an engine bug, reported as such, not a
      // property of the data.  Any other non-finite value is a genuine one (NaN features, overflow).
      auto poisoned = [](double v) { unsigned long long b; memcpy(&b, &v, 8); return b == 0x7ff8000000005eedull; };
      bool never_written = poisoned(s.hOut->lml);
      if (grad) for (int j = 0; j < p; ++j) never_written = never_written || poisoned(s.hOut->grad[j]);
      if (never_written) throw HipError{hipErrorLaunchFailure, "evaluation: an output of the lml/gradient kernels was never written", __LINE__};
    }
    if (!finite) {  // handled like a failed factorisation (lml.rs:47-50 -> fit.rs:105-112): objective +inf, zero gradient, never captured
      *lml = -std::numeric_limits<double>::infinity();
      if (grad) for (int j = 0; j < p; ++j) grad[j] = 0.0;
      return HBEGP_NOT_PD;
    }
    return HBEGP_OK;
  }

  int eval(int dev, int slot, const double* theta, const double* lo, const double* hi, double* lml, double* grad) override {
    if (dev < 0 || dev >= (int)slots.size() || slot < 0 || slot >= n_slots) return fail(HBEGP_EINVAL, "bad device/slot index");
    Slot<T>& s = slots[dev][slot];
    theta_to_params(theta, lo, hi, d, s.hP);
    // never overwrite the captured best: write into the other buffer
    const int target = (s.best_idx < 0) ? 0 : 1 - s.best_idx;
    return run_eval((size_t)dev, slot, target, grad != nullptr, true, lml, grad);
  }

  // The leave-one-out tail on what the slot's last evaluation left behind: L^-1 in W2 (every evaluation path -- the single launch
  // in the LDS, the launches, the task queue -- writes it there), K^-1 and alpha in the buffer it wrote, the parameters in the
  // pinned block.  Reads only; its work arrays are borrowed for the call.
  int loo_on_slot(size_t di, int si, double* loo, double* grad) {
    Slot<T>& s = slots[di][si];
    const LooIn<T> in{s.dev, s.stream, n, d, np, nu2, Xd[di], yd[di], s.alpha[s.last_target], s.W2, s.Kinv[s.last_target], s.hP};
    return loo_tail<T>(in, nullptr, nullptr, nullptr, loo, grad);
  }

  int eval_loo(int dev, int slot, const double* theta, const double* lo, const double* hi, double* loo, double* grad) override {
    double lml;
    const int st = eval(dev, slot, theta, lo, hi, &lml, nullptr);
    if (st != HBEGP_OK) {
      if (st == HBEGP_NOT_PD) {
        *loo = -std::numeric_limits<double>::infinity();
        if (grad) for (int j = 0; j < d + 2; ++j) grad[j] = 0.0;
      }
      return st;
    }
    return loo_on_slot((size_t)dev, slot, loo, grad);
  }

  // The leave-group-out tail on the same results; dlists as in lgo_tail.
  int lgo_on_slot(size_t di, int si, const LgoGroups& gr, const int* dlists, double* lgo, double* grad) {
    Slot<T>& s = slots[di][si];
    const LooIn<T> in{s.dev, s.stream, n, d, np, nu2, Xd[di], yd[di], s.alpha[s.last_target], s.W2, s.Kinv[s.last_target], s.hP};
    return lgo_tail<T>(in, gr, dlists, nullptr, nullptr, nullptr, lgo, grad);
  }

  int eval_lgo(int dev, int slot, const double* theta, const double* lo, const double* hi, const LgoGroups& gr, double* lgo,
               double* grad) override {
    if (gr.n != n) return fail(HBEGP_EINVAL, "the groups cover %d rows, the problem has %d", gr.n, n);
    double lml;
    const int st = eval(dev, slot, theta, lo, hi, &lml, nullptr);
    if (st != HBEGP_OK) {
      if (st == HBEGP_NOT_PD) {
        *lgo = -std::numeric_limits<double>::infinity();
        if (grad) for (int j = 0; j < d + 2; ++j) grad[j] = 0.0;
      }
      return st;
    }
    return lgo_on_slot((size_t)dev, slot, gr, nullptr, lgo, grad);
  }

  // The slot's normal evaluation, then the input-gradient tail on what it left behind (as loo_on_slot: every path leaves alpha and
  // the lower triangle of K^-1 in the buffer it wrote, the clamped parameters in the pinned block).
  int eval_xgrad(int dev, int slot, const double* theta, const double* lo, const double* hi, double* lml, double* grad, double* gx) override {
    const int st = eval(dev, slot, theta, lo, hi, lml, grad);
    if (st != HBEGP_OK) {
      if (st == HBEGP_NOT_PD) std::fill(gx, gx + (size_t)n * d, 0.0);
      return st;
    }
    Slot<T>& s = slots[dev][slot];
    const LooIn<T> in{s.dev, s.stream, n, d, np, nu2, Xd[dev], yd[dev], s.alpha[s.last_target], s.W2, s.Kinv[s.last_target], s.hP};
    return xgrad_tail<T>(in, gx, nullptr, nullptr, nullptr);
  }

  // lml(w(X; a, b), theta) and its p + 2 d gradient.  The device's feature buffer is shared by the problem's
  // slots and this call rewrites it, hence one slot only.  Everything is ordered on the slot's stream: the warp writes U over Xd,
  // the evaluation and the tail read it, the caller's rows (kept in X0d from the first call on) are copied back -- also when the
  // evaluation fails or throws.  Nothing derived from X is cached between evaluations (kmat, gradtrace, the single-launch
  // evaluation and the tails read Xd anew every time; the captured graphs hold the pointer, not the contents).
  int eval_warped(int dev, int slot, const double* theta, const double* lo, const double* hi, const double* ab, double* lml,
                  double* grad) override {
    if (n_slots != 1)
      return fail(HBEGP_EINVAL, "hbegp_problem_eval_warped rewrites the device's feature buffer, which the slots of a problem share: "
                  "it needs a problem created with n_slots == 1 (this one has %d)", n_slots);
    if (dev < 0 || dev >= (int)slots.size() || slot != 0) return fail(HBEGP_EINVAL, "bad device/slot index");
    for (int k = 0; k < 2 * d; ++k)
      if (!std::isfinite(ab[k]) || !(ab[k] > 0.0)) return fail(HBEGP_EINVAL, "warp parameter %d is not a positive finite number", k);
    Slot<T>& s = slots[dev][slot];
    HIPCHECK(hipSetDevice(s.dev));
    const size_t nd = (size_t)n * d;
    const int p = d + 2;
    if (X0d.empty()) X0d.assign(slots.size(), nullptr);
    if (!X0d[dev]) {
      // first use: the warp is defined on [0, 1] -- look at the rows once
      std::vector<T> rows(nd);
      HIPCHECK(hipMemcpyAsync(rows.data(), Xd[dev], sizeof(T) * nd, hipMemcpyDeviceToHost, s.stream));
      HIPCHECK(hipStreamSynchronize(s.stream));
      for (size_t e = 0; e < nd; ++e)
        if (!(rows[e] >= T(0) && rows[e] <= T(1)))
          return fail(HBEGP_EINVAL, "input warping needs features in [0, 1]: row %zu, feature %zu is %g", e / d, e % d, (double)rows[e]);
      T* keep = palloc<T>(s.dev, nd);
      HIPCHECK(hipMemcpyAsync(keep, Xd[dev], sizeof(T) * nd, hipMemcpyDeviceToDevice, s.stream));
      X0d[dev] = keep;
      if (warp_ws_.empty()) warp_ws_.assign(slots.size(), nullptr);
      warp_ws_[dev] = palloc<double>(s.dev, 2 * (size_t)d + 2 * nd);
    }
    double* dab = warp_ws_[dev];  // [2 d] the parameters, then dU/dln a and dU/dln b [n d] each
    double* dlna = grad ? dab + 2 * d : nullptr;
    double* dlnb = grad ? dlna + nd : nullptr;
    warp_ab_.assign(ab, ab + 2 * d);  // the source of an asynchronous copy: the problem's, not the caller's
    ab = warp_ab_.data();
    struct Restore {  // the caller's rows go back behind whatever the stream still holds, whichever way the call ends
      T* dst; const T* src; size_t bytes; hipStream_t st; bool keep;
      ~Restore() {
        if (!keep) (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
        (void)hipStreamSynchronize(st);
      }
      // HBEGP_WARP_DEBUG_KEEP=1 (tests; read per call): the warped rows stay in the feature buffer, where hbegp_problem_debug_rows_*
      // reads what the evaluation read.  The next call warps from the kept rows again and, without the variable, restores them.
    } restore{Xd[dev], X0d[dev], sizeof(T) * nd, s.stream, env_int("HBEGP_WARP_DEBUG_KEEP", 0) != 0};
    HIPCHECK(hipMemcpyAsync(dab, ab, sizeof(double) * 2 * d, hipMemcpyHostToDevice, s.stream));
    launch_warp<T>(X0d[dev], n, d, dab, Xd[dev], dlna, dlnb, s.stream);
    CHECK_LAUNCHES();
    const int st = eval(dev, slot, theta, lo, hi, lml, grad);
    if (st != HBEGP_OK) {
      if (st == HBEGP_NOT_PD && grad) std::fill(grad + p, grad + p + 2 * d, 0.0);
      return st;
    }
    if (!grad) return HBEGP_OK;
    const LooIn<T> in{s.dev, s.stream, n, d, np, nu2, Xd[dev], yd[dev], s.alpha[s.last_target], s.W2, s.Kinv[s.last_target], s.hP};
    const int st2 = xgrad_tail<T>(in, nullptr, dlna, dlnb, grad + p);
    if (st2 == HBEGP_NOT_PD) {
      *lml = -std::numeric_limits<double>::infinity();
      std::fill(grad, grad + p + 2 * d, 0.0);
    }
    return st2;
  }

  // the rows the device's feature buffer holds right now (tests: what warp_kernel wrote is what the evaluation read)
  int get_rows(int dev, void* out, bool want_f32) override {
    if (want_f32 != is_f32) return fail(HBEGP_EINVAL, "element type mismatch");
    if (dev < 0 || dev >= (int)slots.size()) return fail(HBEGP_EINVAL, "bad device index");
    Slot<T>& s = slots[dev][0];
    HIPCHECK(hipSetDevice(s.dev));
    HIPCHECK(hipMemcpyAsync(out, Xd[dev], sizeof(T) * (size_t)n * d, hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    return HBEGP_OK;
  }

  int time_eval(int dev, int slot, const double* theta, int reps, double* phase_ms) override {
    if (dev < 0 || dev >= (int)slots.size() || slot < 0 || slot >= n_slots) return fail(HBEGP_EINVAL, "bad device/slot index");
    Slot<T>& s = slots[dev][slot];
    HIPCHECK(hipSetDevice(s.dev));
    theta_to_params(theta, nullptr, nullptr, d, s.hP);
    double lml;
    std::vector<double> grad(d + 2);
    int st = run_eval((size_t)dev, slot, 0, true, true, &lml, grad.data());  // warm-up + graph instantiation
    if (st != HBEGP_OK) return st;
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    HIPCHECK(hipEventRecord(e0, s.stream));
    hipGraphExec_t timed_graph = s.graph[s.dag_variant][0][1];  // what the warm-up evaluation instantiated
    for (int r = 0; r < reps; ++r) {
      if (timed_graph) HIPCHECK(hipGraphLaunch(timed_graph, s.stream));
      else enqueue_eval(s, (size_t)dev, 0, true, nullptr);  // HBEGP_NO_GRAPH=1
    }
    HIPCHECK(hipEventRecord(e1, s.stream));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    if (phase_ms) {
      for (int i = 0; i < 24; ++i) phase_ms[i] = 0;
      phase_ms[6] = ms / reps;
      // eager pass with one event pair per launch
      const int treps = std::max(1, std::min(reps, 3));
      for (int r = 0; r < treps; ++r) {
        PhaseTimer tm;
        tm.s = s.stream;
        hipEvent_t t0, t1;
        HIPCHECK(hipEventCreate(&t0));
        HIPCHECK(hipEventCreate(&t1));
        HIPCHECK(hipEventRecord(t0, s.stream));
        enqueue_eval(s, (size_t)dev, 0, true, &tm);
        HIPCHECK(hipEventRecord(t1, s.stream));
        HIPCHECK(hipStreamSynchronize(s.stream));
        float tot = 0;
        HIPCHECK(hipEventElapsedTime(&tot, t0, t1));
        phase_ms[14] += tot / treps;
        for (auto& rec : tm.recs) {
          float dt = 0;
          HIPCHECK(hipEventElapsedTime(&dt, rec.a, rec.b));
          const double v = dt / treps;
          if (rec.kind == PhaseTimer::KMAT) phase_ms[0] += v;
          if (rec.kind == PhaseTimer::GEMM) { phase_ms[1] += v; phase_ms[7] += 1.0 / treps; }
          if (rec.kind == PhaseTimer::LEAF) { phase_ms[2] += v; phase_ms[15] += 1.0 / treps; }
          if (rec.kind == PhaseTimer::LAUUM) phase_ms[3] += v;
          if (rec.kind == PhaseTimer::ALPHA) phase_ms[4] += v;
          if (rec.kind == PhaseTimer::GRAD) phase_ms[5] += v;
          if (rec.kind == PhaseTimer::DAG) { phase_ms[19] += v; phase_ms[20] += rec.gflop / treps; }
          if (rec.kind == PhaseTimer::GEMM || rec.kind == PhaseTimer::LAUUM) {
            const int o = rec.tile == 128 ? 8 : (rec.tile == 64 ? 10 : 12);
            phase_ms[o] += v;
            phase_ms[o + 1] += rec.gflop / treps;
            phase_ms[rec.tile == 128 ? 16 : (rec.tile == 64 ? 17 : 18)] += 1.0 / treps;  // launches per evaluation
          }
          (void)hipEventDestroy(rec.a);
          (void)hipEventDestroy(rec.b);
        }
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
      }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (s.dag_trace && getenv("HBEGP_DAG_TRACE")) {
      // one more graph replay on a quiet device, then dump: idx kind row col depth nwait | pulled ready computed published (ticks of 10 ns) | xcc hwid
      if (timed_graph) HIPCHECK(hipGraphLaunch(timed_graph, s.stream));
      HIPCHECK(hipStreamSynchronize(s.stream));
      const std::vector<DagTask>& dag_host_tasks = dag_var[s.dag_variant].host_tasks;
      std::vector<unsigned long long> tr((size_t)5 * dag_ntasks);
      HIPCHECK(hipMemcpyAsync(tr.data(), s.dag_trace, sizeof(unsigned long long) * tr.size(), hipMemcpyDeviceToHost, s.stream));
      HIPCHECK(hipStreamSynchronize(s.stream));
      if (FILE* f = fopen(getenv("HBEGP_DAG_TRACE"), "w")) {
        for (int i = 0; i < dag_ntasks; ++i) {
          const DagTask& t = dag_host_tasks[i];
          fprintf(f, "%d %d %d %d %d %d %llu %llu %llu %llu %llu %llu\n", i, t.kind, t.row0, t.col0, t.kend - t.kbeg, t.nwait, tr[5 * i], tr[5 * i + 1],
                  tr[5 * i + 2], tr[5 * i + 3], tr[5 * i + 4] >> 32, tr[5 * i + 4] & 0xffffffffull);
        }
        fclose(f);
      }
    }
    return HBEGP_OK;
  }

  int time_concurrent(int dev, const double* theta, int reps, double* out) override {
    if (dev < 0 || dev >= (int)slots.size()) return fail(HBEGP_EINVAL, "bad device index");
    const size_t di = (size_t)dev;
    const int ns = n_slots;
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[1] = ns;
    out[10] = dag_ ? dag_nwg : 0;
    std::string err;
    std::mutex err_mu;
    // pass 0: warm-up (graph instantiation), pass 1: graph replay, pass 2: eager with events
    std::vector<double> acc(12, 0.0);
    std::mutex acc_mu;
    for (int pass = 0; pass < 3; ++pass) {
      std::atomic<int> arrived{0};
      std::vector<double> wall(ns, 0.0);
      auto worker = [&](int si) {
        try {
          Slot<T>& s = slots[di][si];
          HIPCHECK(hipSetDevice(s.dev));
          theta_to_params(theta, nullptr, nullptr, d, s.hP);
          std::vector<double> grad(d + 2);
          double lml;
          arrived.fetch_add(1);
          while (arrived.load() < ns) std::this_thread::yield();  // start together
          const auto t0 = std::chrono::steady_clock::now();
          const int nrep = pass == 0 ? 1 : reps;
          for (int r = 0; r < nrep; ++r) {
            if (pass < 2) {
              const int st = run_eval(di, si, 0, true, true, &lml, grad.data());
              if (st != HBEGP_OK) throw std::runtime_error("evaluation failed (not positive definite) at the timing theta");
            } else {
              PhaseTimer tm;
              tm.s = s.stream;
              enqueue_eval(s, di, 0, true, &tm);
              HIPCHECK(hipStreamSynchronize(s.stream));
              std::vector<double> loc(12, 0.0);
              for (auto& rec : tm.recs) {
                float dt = 0;
                HIPCHECK(hipEventElapsedTime(&dt, rec.a, rec.b));
                if (rec.kind == PhaseTimer::KMAT) loc[3] += dt;
                if (rec.kind == PhaseTimer::DAG || rec.kind == PhaseTimer::GEMM || rec.kind == PhaseTimer::LEAF) { loc[4] += dt; loc[5] += rec.gflop; loc[11] += 1; }
                if (rec.kind == PhaseTimer::LAUUM) { loc[6] += dt; loc[7] += rec.gflop; }
                if (rec.kind == PhaseTimer::ALPHA) loc[8] += dt;
                if (rec.kind == PhaseTimer::GRAD) loc[9] += dt;
                (void)hipEventDestroy(rec.a);
                (void)hipEventDestroy(rec.b);
              }
              std::lock_guard<std::mutex> lk(acc_mu);
              for (int i = 0; i < 12; ++i) acc[i] += loc[i] / ((double)nrep * ns);
            }
          }
          wall[si] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / nrep;
        } catch (const HipError& he) {
          hip_fail(he);
          std::lock_guard<std::mutex> lk(err_mu);
          err = g_last_error;
          arrived.fetch_add(ns);  // never leave the others spinning at the start line
        } catch (const std::exception& e) {
          std::lock_guard<std::mutex> lk(err_mu);
          err = e.what();
          arrived.fetch_add(ns);
        }
      };
      std::vector<std::thread> threads;
      try {
        for (int si = 0; si < ns; ++si) threads.emplace_back(worker, si);
      } catch (...) {
        arrived.fetch_add(ns);
        for (auto& t : threads) t.join();
        throw;
      }
      for (auto& t : threads) t.join();
      if (!err.empty()) return fail(HBEGP_EHIP, "%s", err.c_str());
      const double wmax = *std::max_element(wall.begin(), wall.end());
      if (pass == 1) out[0] = wmax;
      if (pass == 2) out[2] = wmax;
    }
    for (int i = 3; i < 12; ++i)
      if (i != 10) out[i] = acc[i];
    return HBEGP_OK;
  }
};

// ---------------------------------------------------------------------------------------------------------------
// model
struct hbegp_model {
  std::atomic<int> refs{1};
  int dev = 0, n = 0, d = 0, np = 0, nu2 = 5;
  bool is_f32 = false;
  double lml = 0;
  std::vector<double> theta;  // clamped, log space
  std::vector<double> warp_ab;  // hbegp_fit_warped_*: [a_1..a_d, b_1..b_d] of the input warp the model's rows went through (empty: none)
  void *X = nullptr, *alpha = nullptr, *Kinv = nullptr;  // device
  void* y = nullptr;     // the (normalised) targets, n entries: the residual of a sample path (hbegp_paths_create) starts from them
  void* rv = nullptr;    // the rows' known noise variances, n entries in the element type (null: none)
  void* Xinv = nullptr;  // L^-1 (lower), for the predictive variance as c + 1e-5 - |L^-1 k*|^2
  void* ldiag = nullptr; // diag(L), np entries (incremental extend needs the log-determinant of the kept part)
  size_t kinv_bytes = 0;
  EvalParams* dP = nullptr;
  EvalOut* dOut = nullptr;
  hipStream_t stream = nullptr;
  // predict scratch (grow-only)
  int cap_m = 0;
  void *Xs = nullptr, *Ks = nullptr, *Q = nullptr, *mean = nullptr, *var = nullptr;
  // gradient scratch (grow-only): G = dKstar/dx*, W = G X^T [d x cap_g x np], the chunk partial sums, dmean / dvar [cap_g x d]
  int cap_g = 0;
  void *G = nullptr, *W = nullptr, *gpart = nullptr, *dmean = nullptr, *dvar = nullptr;
  // joint posterior: the model's parameters with noise = 1e-5 + jitter (its m_p x m_p work matrices are borrowed per call)
  EvalParams* dPcov = nullptr;
  // scratch of the path for a handful of candidates (allocated on first use): device [Xs | Ks | out], partial sums, and
  // pinned host staging so that a single-point predict costs one H2D and one D2H
  void *sm_Xs = nullptr, *sm_Ks = nullptr, *sm_out = nullptr, *sm_hin = nullptr, *sm_hout = nullptr;
  double *sm_pmean = nullptr, *sm_w = nullptr;
  std::mutex mu;
  // every device array of the model comes from the block pool and goes back to it (no hipMalloc / hipFree on the caller's
  // path: they synchronise the whole device, i.e. every other host thread's fit); pinned blocks and the stream likewise
  struct Pooled { void* p; size_t bytes; };
  std::vector<Pooled> pooled;
  size_t sm_hin_bytes = 0, sm_hout_bytes = 0;
  void* palloc(size_t bytes) {
    bool fresh = false;
    bytes = std::max<size_t>(16, bytes);
    void* q = g_pool.get(dev, bytes, &fresh);
    pooled.push_back({q, bytes});
    return q;
  }
  void pfree(void* q) {
    for (size_t i = 0; i < pooled.size(); ++i)
      if (pooled[i].p == q) {
        g_pool.put(dev, q, pooled[i].bytes);
        pooled.erase(pooled.begin() + (long)i);
        return;
      }
  }
  ~hbegp_model() {
    (void)hipSetDevice(dev);
    if (stream) (void)hipStreamSynchronize(stream);
    g_pool.put(dev, Kinv, kinv_bytes); g_pool.put(dev, Xinv, kinv_bytes);
    for (const Pooled& q : pooled) g_pool.put(dev, q.p, q.bytes);
    g_host_pool.put(sm_hin, sm_hin_bytes); g_host_pool.put(sm_hout, sm_hout_bytes);
    g_stream_pool.put(dev, stream, STREAM_MODEL);  // synchronised above
  }
};

template <typename T>
static hbegp_model* make_model(Problem<T>& prob, size_t di, int si, const double* theta_clamped, double lml,
                               bool w2_current = false, const double* params_linear = nullptr) {
  Slot<T>& s = prob.slots[di][si];
  HIPCHECK(hipSetDevice(s.dev));
  std::unique_ptr<hbegp_model> m(new hbegp_model());
  m->dev = s.dev; m->n = prob.n; m->d = prob.d; m->np = prob.np; m->nu2 = prob.nu2; m->is_f32 = prob.is_f32; m->lml = lml;
  m->theta.assign(theta_clamped, theta_clamped + prob.d + 2);
  const size_t nn = (size_t)prob.np * prob.np;
  // (a model that took over its fit's first slot stream instead -- one stream fewer per fit in flight -- was tried in round 5:
  // nothing gained for fits side by side, and the slot streams then change hands from fit to fit, so that two slots of one fit
  // end up on one hardware queue now and then: bench 1.777 -> 1.739, solo fits at n = 1024 16.4 -> 6.7 per s in some processes)
  m->stream = g_stream_pool.get(m->dev, STREAM_MODEL);
  m->X = m->palloc(sizeof(T) * (size_t)prob.n * prob.d);
  m->alpha = m->palloc(sizeof(T) * prob.np);
  m->y = m->palloc(sizeof(T) * prob.n);
  if (prob.rvd[di]) m->rv = m->palloc(sizeof(T) * prob.n);
  { bool fr; m->Kinv = g_pool.get(m->dev, sizeof(T) * nn, &fr); m->Xinv = g_pool.get(m->dev, sizeof(T) * nn, &fr); m->kinv_bytes = sizeof(T) * nn; }
  m->dP = static_cast<EvalParams*>(m->palloc(sizeof(EvalParams)));
  m->dOut = static_cast<EvalOut*>(m->palloc(sizeof(EvalOut)));
  const int b = s.best_idx < 0 ? s.last_target : s.best_idx;
  // X = L^-1 at the model's theta (the evaluation slots only keep K^-1 and alpha of the captured evaluation)
  // (w2_current: the slot's last evaluation WAS at this theta -- extend -- so W2 and ldiag already hold them)
  auto fill_params = [&](EvalParams* P) {
    if (params_linear) {  // a device-driven fit: the very numbers the captured evaluation ran with
      P->noise = params_linear[0];
      P->amp = params_linear[1];
      for (int k = 0; k < prob.d; ++k) P->ell[k] = params_linear[2 + k];
    } else {
      theta_to_params(theta_clamped, nullptr, nullptr, prob.d, P);
    }
  };
  // (x_captured: a device-driven small fit kept the captured evaluation's own factor: buffer b of the ping-pong pair)
  const T* Xsrc = (s.x_captured && b == 1) ? s.Xalt : s.W2;
  const T* ldsrc = (s.x_captured && b == 1) ? s.ldalt : s.ldiag;
  if (!w2_current && !s.x_captured) {
    fill_params(s.hP);
    if (prob.factor_only(di, si) != HBEGP_OK) throw HipError{hipErrorUnknown, "factorisation at the captured theta failed", __LINE__};
  }
  m->ldiag = m->palloc(sizeof(T) * prob.np);
  HIPCHECK(hipMemcpyAsync(m->ldiag, ldsrc, sizeof(T) * prob.np, hipMemcpyDeviceToDevice, m->stream));
  HIPCHECK(hipMemcpyAsync(m->Xinv, Xsrc, sizeof(T) * nn, hipMemcpyDeviceToDevice, m->stream));
  HIPCHECK(hipMemcpyAsync(m->X, prob.Xd[di], sizeof(T) * (size_t)prob.n * prob.d, hipMemcpyDeviceToDevice, m->stream));
  HIPCHECK(hipMemcpyAsync(m->alpha, s.alpha[b], sizeof(T) * prob.np, hipMemcpyDeviceToDevice, m->stream));
  HIPCHECK(hipMemcpyAsync(m->y, prob.yd[di], sizeof(T) * prob.n, hipMemcpyDeviceToDevice, m->stream));
  if (m->rv) HIPCHECK(hipMemcpyAsync(m->rv, prob.rvd[di], sizeof(T) * prob.n, hipMemcpyDeviceToDevice, m->stream));
  HIPCHECK(hipMemcpyAsync(m->Kinv, s.Kinv[b], sizeof(T) * nn, hipMemcpyDeviceToDevice, m->stream));
  launch_symmetrize<T>(static_cast<T*>(m->Kinv), prob.np, m->stream);  // invc_into() returns the full matrix (fit.rs:60,168)
  CHECK_LAUNCHES();
  EvalParams P;
  memset(&P, 0, sizeof(P));
  fill_params(&P);
  HIPCHECK(hipMemcpyAsync(m->dP, &P, sizeof(P), hipMemcpyHostToDevice, m->stream));
  HIPCHECK(hipStreamSynchronize(m->stream));
  return m.release();
}

// The batched predict path: scratch for mp (a multiple of NB) candidate rows, grown on demand ...
template <typename T>
static void predict_batched_reserve(hbegp_model* m, int mp) {
  if (mp <= m->cap_m) return;
  HIPCHECK(hipStreamSynchronize(m->stream));  // nothing of an earlier predict is still using the smaller arrays
  m->pfree(m->Xs); m->pfree(m->Ks); m->pfree(m->Q); m->pfree(m->mean); m->pfree(m->var);
  m->Xs = m->Ks = m->Q = m->mean = m->var = nullptr;
  m->cap_m = 0;
  m->Xs = m->palloc(sizeof(T) * (size_t)mp * m->d);
  m->Ks = m->palloc(sizeof(T) * (size_t)mp * m->np);
  m->Q = m->palloc(sizeof(T) * (size_t)mp * m->np);
  m->mean = m->palloc(sizeof(T) * mp);
  m->var = m->palloc(sizeof(T) * mp);
  m->cap_m = mp;
}
// ... and its launches on the model stream, the candidates already in m->Xs: Kstar, the mean and, with want_var, the variance
template <typename T>
static void predict_batched_launches(hbegp_model* m, int cnt, int mp, bool want_var) {
  hipStream_t s = m->stream;
  HIPCHECK(hipMemsetAsync(m->dOut, 0, sizeof(EvalOut), s));
  launch_kstar<T>(static_cast<T*>(m->Xs), cnt, mp, static_cast<T*>(m->X), m->n, m->d, m->np, m->nu2, m->dP,
                  static_cast<T*>(m->Ks), s);
  launch_pred_mean<T>(static_cast<T*>(m->Ks), cnt, m->np, static_cast<T*>(m->alpha), static_cast<T*>(m->mean), s);
  if (want_var) {
    // The reference's k*^T K^-1 k* (predict.rs:30-37) as |L^-1 k*|^2: Q = Kstar * X^T (X = L^-1 lower: k <= j, half the
    // flops), then var = c + 1e-5 - rowsum(Q o Q).  A sum of squares has no cancellation inside the quadratic form, so the
    // result is at least as close to the exact value as the K^-1 form.
    GemmLaunch g = gemm_lower_b(m->Ks, m->np, m->Xinv, m->np, m->Q, m->np, mp / NB, m->np / NB, m->np / NB);
    gemm_adhoc<T>(g, &m->dOut->info, s);
    launch_pred_var<T>(static_cast<T*>(m->Q), static_cast<T*>(m->Q), cnt, m->np, m->dP, static_cast<T*>(m->var), m->dOut, s);
  }
  CHECK_LAUNCHES();
}

template <typename T>
static int model_predict(hbegp_model* m, const T* Xs, int cnt, T* mean, T* var, int* n_warn) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  if (cnt <= 8) {
    // a handful of candidates (the caller's scalar predict_* loops): read L^-1 once instead of a padded 128-row tile GEMM
    const size_t out_bytes = sizeof(T) * 2 * PRED_SMALL_MAX + 16;
    if (!m->sm_Xs) {
      m->sm_Xs = m->palloc(sizeof(T) * PRED_SMALL_MAX * m->d);
      m->sm_Ks = m->palloc(sizeof(T) * (size_t)PRED_SMALL_MAX * m->np);
      m->sm_out = m->palloc(out_bytes);
      m->sm_pmean = static_cast<double*>(m->palloc(sizeof(double) * (size_t)((m->np + 255) / 256) * PRED_SMALL_MAX));
      m->sm_w = static_cast<double*>(m->palloc(sizeof(double) * (size_t)m->n * PRED_SMALL_MAX));
      m->sm_hin_bytes = sizeof(T) * PRED_SMALL_MAX * m->d;
      m->sm_hout_bytes = out_bytes;
      m->sm_hin = g_host_pool.get(m->sm_hin_bytes);
      m->sm_hout = g_host_pool.get(m->sm_hout_bytes);
    }
    hipStream_t s = m->stream;
    memcpy(m->sm_hin, Xs, sizeof(T) * (size_t)cnt * m->d);
    HIPCHECK(hipMemcpyAsync(m->sm_Xs, m->sm_hin, sizeof(T) * (size_t)cnt * m->d, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(m->sm_out, 0, out_bytes, s));
    T* dmean = static_cast<T*>(m->sm_out);
    T* dvar = dmean + PRED_SMALL_MAX;
    int* dwarn = reinterpret_cast<int*>(dvar + PRED_SMALL_MAX);
    launch_predict_small<T>(static_cast<T*>(m->sm_Xs), cnt, static_cast<T*>(m->X), m->n, m->d, m->np, m->nu2, m->dP, static_cast<T*>(m->alpha),
                            static_cast<T*>(m->Xinv), static_cast<T*>(m->sm_Ks), m->sm_pmean, m->sm_w, var ? 1 : 0, dmean, dvar, dwarn, s);
    CHECK_LAUNCHES();
    HIPCHECK(hipMemcpyAsync(m->sm_hout, m->sm_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const T* hmean = static_cast<const T*>(m->sm_hout);
    memcpy(mean, hmean, sizeof(T) * cnt);
    if (var) memcpy(var, hmean + PRED_SMALL_MAX, sizeof(T) * cnt);
    if (n_warn) *n_warn = var ? *reinterpret_cast<const int*>(hmean + 2 * PRED_SMALL_MAX) : 0;
    return HBEGP_OK;
  }
  const int mp = round_up(std::max(cnt, 1), NB);
  predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  HIPCHECK(hipMemcpyAsync(m->Xs, Xs, sizeof(T) * (size_t)cnt * m->d, hipMemcpyHostToDevice, s));
  predict_batched_launches<T>(m, cnt, mp, var != nullptr);
  HIPCHECK(hipMemcpyAsync(mean, m->mean, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  if (var) HIPCHECK(hipMemcpyAsync(var, m->var, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, m->dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (n_warn) *n_warn = var ? out.n_warn : 0;
  return HBEGP_OK;
}

// the gradient scratch for mp (a multiple of NB) rows, grown on demand (predict_batched_reserve's arrays too)
template <typename T>
static void predict_grad_reserve(hbegp_model* m, int mp) {
  predict_batched_reserve<T>(m, mp);
  if (mp <= m->cap_g) return;
  HIPCHECK(hipStreamSynchronize(m->stream));
  m->pfree(m->G); m->pfree(m->W); m->pfree(m->gpart); m->pfree(m->dmean); m->pfree(m->dvar);
  m->G = m->W = m->gpart = m->dmean = m->dvar = nullptr;
  m->cap_g = 0;
  m->G = m->palloc(sizeof(T) * (size_t)m->d * mp * m->np);
  m->W = m->palloc(sizeof(T) * (size_t)m->d * mp * m->np);
  m->gpart = m->palloc(sizeof(double) * (size_t)pred_grad_chunks(m->n) * mp * m->d);
  m->dmean = m->palloc(sizeof(T) * (size_t)mp * m->d);
  m->dvar = m->palloc(sizeof(T) * (size_t)mp * m->d);
  m->cap_g = mp;
}
// What those arrays take for `rows` padded candidate rows, with or without the gradient's, as a double: a call counts its bytes with
// this before it takes anything, so that a size far beyond the device is ENOMEM, not an overflow.
static double padded_rows(double cnt) { return std::ceil(std::max(1.0, cnt) / NB) * NB; }
template <typename T>
static double predict_bytes(const hbegp_model* m, double rows, bool want_grad) {
  const int d = m->d;
  return (double)sizeof(T) * ((2.0 + (want_grad ? 2.0 * d : 0.0)) * rows * m->np + rows * (d + 2) + (want_grad ? 2.0 * rows * d : 0.0)) +
         8.0 * (want_grad ? (double)pred_grad_chunks(m->n) * rows * d : 0.0);
}
// W = G X^T on the model stream, the candidates in m->Xs: G = dKstar/dx* (d matrices [mp x np] stacked into one operand), then the
// triangular tile GEMM that makes Q = Kstar X^T.  Row k mp + i of W is L^-1 dk*_i / dx*_i,k.
template <typename T>
static void predict_grad_w_launches(hbegp_model* m, int cnt, int mp) {
  hipStream_t s = m->stream;
  launch_kstar_grad<T>(static_cast<T*>(m->Xs), cnt, mp, static_cast<T*>(m->X), m->n, m->d, m->np, m->nu2, m->dP,
                       static_cast<T*>(m->G), s);
  GemmLaunch g = gemm_lower_b(m->G, m->np, m->Xinv, m->np, m->W, m->np, m->d * mp / NB, m->np / NB, m->np / NB);  // X = L^-1 lower, as for Q
  gemm_adhoc<T>(g, &m->dOut->info, s);
}

// The gradient launches behind predict_batched_launches, on the model stream: dmean, then with want_w W = G X^T and with
// want_dvar (needs W, and Q: the batched launches' variance) dvar.
template <typename T>
static void predict_grad_launches(hbegp_model* m, int cnt, int mp, bool want_w, bool want_dvar) {
  hipStream_t s = m->stream;
  launch_pred_grad<T>(static_cast<T*>(m->Xs), cnt, static_cast<T*>(m->X), m->n, m->d, m->nu2, m->dP, static_cast<T*>(m->alpha),
                      static_cast<double*>(m->gpart), static_cast<T*>(m->dmean), s);
  if (want_w) predict_grad_w_launches<T>(m, cnt, mp);
  if (want_dvar)
    launch_pred_dvar<T>(static_cast<T*>(m->W), static_cast<T*>(m->Q), cnt, mp, m->np, m->d, static_cast<T*>(m->var),
                        static_cast<T*>(m->dvar), s);
}

// Posterior mean / variance as the batched predict computes them (for every m, also m <= 8) plus their gradients w.r.t. the
// candidates (kernels.hip, pred_grad_kernel ..).  dvar = -2 (L^-1 dk*/dx_k) . (L^-1 k*): the d gradient matrices G_k stacked
// into one [d*mp x np] operand of the same triangular tile GEMM that makes Q = Kstar X^T for the variance, then one fp64 row
// dot per (k, row) against Q.  (The explicit V = Kstar K^-1 -- one GEMM against the symmetric K^-1, or V = Q X through the
// triangular options -- costs 2 or 1 m n^2 instead of d m n^2 flops, but V grows with cond(K) and its sum cancels: on the
// fitted config-M model both V forms were off by the whole scale of the gradient.  DESIGN section 10.)
template <typename T>
static int model_predict_grad(hbegp_model* m, const T* Xs, int cnt, T* mean, T* var, T* dmean, T* dvar, int* n_warn) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int mp = round_up(cnt, NB);
  predict_grad_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  const bool want_var = var != nullptr;
  HIPCHECK(hipMemcpyAsync(m->Xs, Xs, sizeof(T) * (size_t)cnt * m->d, hipMemcpyHostToDevice, s));
  predict_batched_launches<T>(m, cnt, mp, want_var);
  predict_grad_launches<T>(m, cnt, mp, want_var, want_var);
  CHECK_LAUNCHES();
  HIPCHECK(hipMemcpyAsync(mean, m->mean, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(dmean, m->dmean, sizeof(T) * (size_t)cnt * m->d, hipMemcpyDeviceToHost, s));
  if (want_var) {
    HIPCHECK(hipMemcpyAsync(var, m->var, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(dvar, m->dvar, sizeof(T) * (size_t)cnt * m->d, hipMemcpyDeviceToHost, s));
  }
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, m->dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (n_warn) *n_warn = want_var ? out.n_warn : 0;
  return HBEGP_OK;
}

// ---- joint posterior at m candidates (hbegp_predict_cov / hbegp_sample_posterior) ----------------------------------------
// Work matrices of m_p^2 elements come from the block pool for ONE call and go back at its end (a model that once sampled
// m = 8192 keeps no gigabyte).  They go back cleared, as the pool hands out fresh blocks: a later owner of the same size (a fit's
// work matrix) then finds zeros above the diagonal, never Sigma's upper triangle or the NaN of a factor that failed (m = 8192
// f64: 3 x 512 MiB cleared in ~0.3 ms).
struct CallScratch {
  int dev;
  hipStream_t s;
  std::vector<std::pair<void*, size_t>> held;
  void* get(size_t bytes) {
    bool fresh = false;
    bytes = std::max<size_t>(16, bytes);
    void* p = g_pool.get(dev, bytes, &fresh);
    held.push_back({p, bytes});
    return p;
  }
  ~CallScratch() {
    for (auto& h : held) (void)hipMemsetAsync(h.first, 0, h.second, s);
    (void)hipStreamSynchronize(s);  // nothing on the stream still uses them
    for (auto& h : held) g_pool.put(dev, h.first, h.second);
  }
};

// ---- phase times of the posterior-side calls (hbegp_debug_*_phases) ----------------------------------------------------------
// One record per kind and calling thread: whether the thread's calls of that kind are timed, and the phase times (ms) of its last
// timed call of that kind that reached its end.
enum PhaseKind { PH_POSTERIOR, PH_SELECT, PH_KG, PH_NEI, PH_SENS, PH_EHVI, PH_QEI, PH_LOO, PH_PATHS, PH_CEI, PH_LCEI, PH_MES, PH_EHVI_ND, PH_CB, PH_LGO, PH_KINDS };
struct PhaseRecord {
  bool on = false;
  double ms[5] = {0, 0, 0, 0, 0};
};
static thread_local PhaseRecord t_phase[PH_KINDS];

// hbegp_debug_X_phases: hands out the kind's stored phases, then switches its timing on or off
static int debug_phases(PhaseKind kind, int count, int enable, double* phase_ms) {
  PhaseRecord& r = t_phase[kind];
  if (phase_ms)
    for (int i = 0; i < count; ++i) phase_ms[i] = r.ms[i];
  r.on = enable != 0;
  return HBEGP_OK;
}

// The events of one timed call.  Disabled, every method does nothing and returns nothing; enabled, mark() creates an event and
// records it, and the destructor destroys every event however the call ends (a throwing HIPCHECK, an early return).
class PhaseClock {
 public:
  PhaseClock(bool enabled, size_t capacity) : on_(enabled) {
    if (on_) ev_.reserve(capacity);
  }
  ~PhaseClock() {
    for (auto& e : ev_) (void)hipEventDestroy(e);
  }
  PhaseClock(const PhaseClock&) = delete;
  PhaseClock& operator=(const PhaseClock&) = delete;
  bool on() const { return on_; }
  int marks() const { return (int)ev_.size(); }
  // an event the callee records itself (launch_sens_eval: between its two kernels)
  hipEvent_t slot() {
    if (!on_) return nullptr;
    hipEvent_t e = nullptr;
    HIPCHECK(hipEventCreate(&e));
    ev_.push_back(e);
    return e;
  }
  void mark(hipStream_t s) {
    if (hipEvent_t e = slot()) HIPCHECK(hipEventRecord(e, s));
  }
  // ms from mark i to mark j, waiting for j first: it may sit on another stream than the one the caller synchronised
  double elapsed_ms(int i, int j) {
    float ms = 0;
    HIPCHECK(hipEventSynchronize(ev_[j]));
    HIPCHECK(hipEventElapsedTime(&ms, ev_[i], ev_[j]));
    return ms;
  }
  // the successful end of a timed call whose phases are the intervals between consecutive marks
  void store(PhaseKind kind, int count) {
    if (!on_) return;
    for (int i = 0; i < count; ++i) t_phase[kind].ms[i] = elapsed_ms(i, i + 1);
  }

 private:
  bool on_;
  std::vector<hipEvent_t> ev_;
};

// The stored phases, by kind (include/hbegp.h has each one's meaning):
//   posterior  Q, Sigma, factor, draws -- sampling calls only, predict_cov is never timed
//   select     Sigma, select                      kg    Sigma, kg
//   nei        Sigma, baseline factor, products, reductions
//   sens       upload, substituted means, chunk and row sums, reduction and download (summed over the slabs)
//   ehvi       the predict of objective 0 and of objective 1 (each on its model's stream: they overlap), the EHVI kernels
//   qei        the shared launches, the qEI kernel
//   loo        diagonal pass, u and Y, the SYRK, the weighted trace -- calls with a gradient only
//   paths      hbegp_paths_create: uploads + frequency scaling, the feature projection, the two triangular products
//   cei        the K predicts (the objective's upload .. the join of the K streams), the cEI kernel with the arg-max
//   lcei       as cei, the second phase being the log-space kernel with the arg-max
//   mes        the predict (the uploads .. the last predict or gradient launch), the MES kernel with the arg-max
//   ehvi_nd    as ehvi with n_obj predicts: each objective's predict on its model's stream, then the box kernel with the arg-max
//   cb         as mes: the predict, the confidence-bound kernel with the arg-min
//   lgo        group pass, u and Y, the SYRK, the weighted trace -- calls with a gradient only

// Sigma = K** + noise I - Q Q^T at the candidates into W (lower tiles; m_p x m_p, kmat's identity padding): the candidates'
// upload, the batched predict's launches (Kstar, the mean, Q = Kstar X^T; the variance too, unused), then kmat_kernel over
// the candidates with a parameter block whose noise is *noise and one tile GEMM.  `noise` is copied from the caller's variable:
// it has to outlive the stream work.  clk_q (may be null) gets a mark behind Q.
template <typename T>
static void posterior_sigma(hbegp_model* m, const T* Xs, int cnt, int mp, const double* noise, T* W, PhaseClock* clk_q) {
  hipStream_t s = m->stream;
  int* info = &m->dOut->info;
  if (!m->dPcov) m->dPcov = static_cast<EvalParams*>(m->palloc(sizeof(EvalParams)));
  HIPCHECK(hipMemcpyAsync(m->Xs, Xs, sizeof(T) * (size_t)cnt * m->d, hipMemcpyHostToDevice, s));
  predict_batched_launches<T>(m, cnt, mp, true);
  if (clk_q) clk_q->mark(s);
  HIPCHECK(hipMemcpyAsync(m->dPcov, m->dP, sizeof(EvalParams), hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(&m->dPcov->noise, noise, sizeof(double), hipMemcpyHostToDevice, s));
  launch_kmat<T>(static_cast<T*>(m->Xs), nullptr, cnt, m->d, mp, m->nu2, m->dPcov, W, info, s);
  {
    // Sigma -= Q Q^T (lower tiles), contraction over the training points
    GemmLaunch g{};
    g.nops = 1;
    GemmOp& op = g.op[0];
    op.A = m->Q; op.B = m->Q; op.C = W;
    op.lda = m->np; op.ldb = m->np; op.ldc = mp;
    op.mi = mp / NB; op.nj = mp / NB; op.c_lower = 1;
    op.k0 = 0; op.k1 = m->np / NB;
    op.alpha_neg = 1; op.beta_one = 1;
    gemm_adhoc<T>(g, info, s);
  }
}

// Sigma = K** + (1e-5 + jitter) I - Q Q^T at the candidates (Q = Kstar X^T of the batched predict), then either
//   cov != nullptr: Sigma mirrored to the full matrix and copied out (hbegp_predict_cov), or
//   the draws mean + L_S z_s with L_S the Cholesky factor of Sigma: Y = Z L^T (tile GEMM), then the epilogue adds the mean and
//   finds each draw's argmin (hbegp_sample_posterior).
// Padding: Kstar's padded rows are zero, so Q's are too, and kmat's identity padding survives the product; L's padding is the
// identity.  Z's padded rows and columns are zero.
template <typename T>
static int model_posterior(hbegp_model* m, const T* Xs, int cnt, double jitter, T* mean, T* cov, const T* z, int S, T* samples,
                           int* argmin, int* info_out) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int mp = round_up(cnt, NB);
  const int Sp = cov ? 0 : round_up(S, NB);
  const size_t nn = (size_t)mp * mp;
  // everything the call borrows, counted before anything is taken: an m far beyond the device is ENOMEM, not an overflow
  const double need = (double)sizeof(T) * ((cov ? 1.0 : 3.0) * (double)mp * mp + 2.0 * (double)Sp * mp + 2.0 * (double)mp * m->np);
  if (need > 1e15) return fail(HBEGP_ENOMEM, "the joint posterior of %d points needs %.3g bytes of device memory", cnt, need);
  predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  int* info = &m->dOut->info;
  const double noise = 1e-5 + jitter;  // predict.rs:25-29's min_noise, plus the caller's jitter (copied from here: outlives the stream work)
  CallScratch ws{m->dev, s, {}};
  T* W1 = static_cast<T*>(ws.get(sizeof(T) * nn));
  PhaseClock clk(t_phase[PH_POSTERIOR].on && !cov, 5);  // the sampling branch only
  clk.mark(s);
  posterior_sigma<T>(m, Xs, cnt, mp, &noise, W1, &clk);
  if (cov) {
    launch_symmetrize<T>(W1, mp, s);
    CHECK_LAUNCHES();
    if (mean) HIPCHECK(hipMemcpyAsync(mean, m->mean, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpy2DAsync(cov, sizeof(T) * cnt, W1, sizeof(T) * mp, sizeof(T) * cnt, cnt, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return HBEGP_OK;
  }
  clk.mark(s);
  T* W2 = static_cast<T*>(ws.get(sizeof(T) * nn));
  T* W3 = static_cast<T*>(ws.get(sizeof(T) * nn));
  T* ld = static_cast<T*>(ws.get(sizeof(T) * mp));
  // the tile GEMMs read X and L as triangular operands: what the diagonal blocks do not write above the diagonal (the strict
  // upper 16 x 16 blocks of X's diagonal blocks) must be zero in memory, and a recycled block holds its earlier owner's numbers
  HIPCHECK(hipMemsetAsync(W2, 0, sizeof(T) * nn, s));
  HIPCHECK(hipMemsetAsync(W3, 0, sizeof(T) * nn, s));
  // the fit's recursion with L kept: L21 -> W3, where the diagonal blocks store L_kk too (leaf_keep_kernel)
  const int nbm = mp / NB;
  chol_inv_rec<T>(W1, W2, W3, mp, 0, nbm / 2, nbm, false, false, [&](GemmLaunch& g, int) { gemm_adhoc<T>(g, info, s); },
                  [&](int k) { launch_leaf_keep<T>(W1, W2, W3, mp, k, ld, info, s); });
  clk.mark(s);
  T* Z = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * mp));
  T* Y = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * mp));
  int* amin = static_cast<int*>(ws.get(sizeof(int) * (size_t)S));
  HIPCHECK(hipMemsetAsync(Z, 0, sizeof(T) * (size_t)Sp * mp, s));
  HIPCHECK(hipMemcpy2DAsync(Z, sizeof(T) * mp, z, sizeof(T) * cnt, sizeof(T) * cnt, S, hipMemcpyHostToDevice, s));
  {
    // Y = Z L^T: Y[s][i] = sum_{k <= i} z_s[k] L[i][k]  (L lower: k <= j, as for Q = Kstar X^T)
    GemmLaunch g = gemm_lower_b(Z, mp, W3, mp, Y, mp, Sp / NB, mp / NB, mp / NB);
    gemm_adhoc<T>(g, info, s);
  }
  launch_sample_epilogue<T>(Y, mp, static_cast<T*>(m->mean), cnt, S, samples != nullptr, amin, info, s);
  clk.mark(s);
  CHECK_LAUNCHES();
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, m->dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_POSTERIOR, 4);
  if (info_out) *info_out = out.info;
  if (out.info != 0) return fail(HBEGP_NOT_PD, "Sigma is not positive definite (pivot panel at column %d); a larger jitter may help",
                                 out.info - 1);
  if (samples) HIPCHECK(hipMemcpy2DAsync(samples, sizeof(T) * cnt, Y, sizeof(T) * mp, sizeof(T) * cnt, S, hipMemcpyDeviceToHost, s));
  if (argmin) HIPCHECK(hipMemcpyAsync(argmin, amin, sizeof(int) * (size_t)S, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return HBEGP_OK;
}


// Greedy batch selection by EI with fantasised observations (hbegp_select_batch): Sigma at jitter 0 as predict_cov builds it
// (posterior_sigma, then mirrored), then the whole k-step loop in one launch of batch_select_kernel.  Only idx / ei (k each) and
// the optional mean / variance after the k conditionings leave the device; the m_p^2 Sigma and the fp64 workspace
// (C [k][m_p], v, mu; the picked flags, idx, ei and the T outputs) are borrowed for the call and go back cleared.
template <typename T>
static int model_select_batch(hbegp_model* m, const T* Xs, int cnt, int k, double fmin, const double* lie, int* idx, double* ei,
                              T* mean_out, T* var_out) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int mp = round_up(cnt, NB);
  // everything the call borrows, counted before anything is taken: an m far beyond the device is ENOMEM, not an overflow
  const double need = (double)sizeof(T) * ((double)mp * mp + 2.0 * (double)mp * m->np + 2.0 * mp) +
                      8.0 * ((double)k * mp + 2.0 * mp + k) + 4.0 * ((double)mp + k);
  if (need > 1e15) return fail(HBEGP_ENOMEM, "the batch selection over %d points needs %.3g bytes of device memory", cnt, need);
  predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  const double noise = 1e-5;  // jitter 0: predict_cov's Sigma, whose diagonal is hbegp_predict's variance before clamping
  CallScratch ws{m->dev, s, {}};
  T* W1 = static_cast<T*>(ws.get(sizeof(T) * (size_t)mp * mp));
  double* Cw = static_cast<double*>(ws.get(sizeof(double) * ((size_t)k * mp + 2 * (size_t)mp + k)));
  double* v = Cw + (size_t)k * mp;
  double* mu = v + mp;
  double* dei = mu + mp;
  int* picked = static_cast<int*>(ws.get(sizeof(int) * ((size_t)mp + k)));
  int* didx = picked + mp;
  T* dmean = static_cast<T*>(ws.get(sizeof(T) * 2 * (size_t)mp));
  T* dvar = dmean + mp;
  PhaseClock clk(t_phase[PH_SELECT].on, 3);
  clk.mark(s);
  posterior_sigma<T>(m, Xs, cnt, mp, &noise, W1, nullptr);
  launch_symmetrize<T>(W1, mp, s);  // the kernel reads row j of Sigma
  clk.mark(s);
  launch_batch_select<T>(W1, mp, static_cast<const T*>(m->mean), cnt, k, m->dP, fmin, lie ? 1 : 0, lie ? *lie : 0.0, Cw, v, mu, picked,
                         didx, dei, dmean, dvar, s);
  clk.mark(s);
  CHECK_LAUNCHES();
  HIPCHECK(hipMemcpyAsync(idx, didx, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, s));
  if (ei) HIPCHECK(hipMemcpyAsync(ei, dei, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
  if (mean_out) HIPCHECK(hipMemcpyAsync(mean_out, dmean, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  if (var_out) HIPCHECK(hipMemcpyAsync(var_out, dvar, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_SELECT, 2);
  return HBEGP_OK;
}


// Knowledge gradient over a candidate set (hbegp_knowledge_gradient): Sigma at jitter 0 as predict_cov builds it (posterior_sigma,
// then mirrored), then kg_kernel with one workgroup per candidate and the epilogue (best, imin, the clamped diagonal).  Only the mc
// values, two ints and the optional mean / variance leave the device; Sigma and the workspace are borrowed for the call and go back
// cleared.  Beyond KG_LDS_ROWS padded rows the lines live in a global workspace of kg_global_workgroups(m, mc) workgroups.
template <typename T>
static int model_knowledge_gradient(hbegp_model* m, const T* Xs, int cnt, int mc, double* kg, int* best, int* imin, T* mean_out,
                                    T* var_out) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int mp = round_up(cnt, NB);
  const size_t ws_lines = (size_t)kg_global_workgroups(cnt, mc) * (size_t)kg_padded_rows(cnt);
  // everything the call borrows, counted before anything is taken: an m far beyond the device is ENOMEM, not an overflow
  const double need = (double)sizeof(T) * ((double)mp * mp + 2.0 * (double)mp * m->np + 2.0 * mp) + 8.0 * mc + 16.0 * (double)ws_lines;
  if (need > 1e15) return fail(HBEGP_ENOMEM, "the knowledge gradient over %d points needs %.3g bytes of device memory", cnt, need);
  predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  const double noise = 1e-5;  // jitter 0: predict_cov's Sigma, whose diagonal is hbegp_predict's variance before clamping
  CallScratch ws{m->dev, s, {}};
  T* W1 = static_cast<T*>(ws.get(sizeof(T) * (size_t)mp * mp));
  double* dkg = static_cast<double*>(ws.get(sizeof(double) * (size_t)std::max(mc, 1)));
  int* dres = static_cast<int*>(ws.get(sizeof(int) * 2));
  T* dvar = static_cast<T*>(ws.get(sizeof(T) * (size_t)mp));
  void* lines = ws_lines ? ws.get(16 * ws_lines) : nullptr;
  PhaseClock clk(t_phase[PH_KG].on, 3);
  clk.mark(s);
  posterior_sigma<T>(m, Xs, cnt, mp, &noise, W1, nullptr);
  launch_symmetrize<T>(W1, mp, s);  // the kernel reads row j of Sigma
  clk.mark(s);
  launch_knowledge_gradient<T>(W1, mp, static_cast<const T*>(m->mean), cnt, mc, m->dP, lines, dkg, dres, dvar, s);
  clk.mark(s);
  CHECK_LAUNCHES();
  int res[2] = {-1, -1};
  if (mc > 0) HIPCHECK(hipMemcpyAsync(kg, dkg, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(res, dres, sizeof(res), hipMemcpyDeviceToHost, s));
  if (mean_out) HIPCHECK(hipMemcpyAsync(mean_out, m->mean, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  if (var_out) HIPCHECK(hipMemcpyAsync(var_out, dvar, sizeof(T) * cnt, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (best) *best = res[0];
  if (imin) *imin = res[1];
  clk.store(PH_KG, 2);
  return HBEGP_OK;
}


// Noisy expected improvement over a candidate set (hbegp_noisy_ei).  On the device the baseline rows come first,
// padded to mbp (a multiple of NB) with copies of row 0, then the candidates, so that the baseline block of Sigma is whole
// 128-blocks: Sigma's lower tiles as predict_cov builds them (posterior_sigma; all of them, the cc block's off-diagonal tiles too),
// the gap turned into identity padding, then
//   the fit's recursion with L kept on the leading nbb blocks only: L_b -> W3, X_b = L_b^-1 -> W2 (rows >= mbp of W1 are not touched)
//   A = Sigma_cb X_b^T -> W3 below L_b (one tile GEMM of the recursion's TRSM shape)
//   Y = Z [L_b; A]^T (one tile GEMM; Z [Sp][mbp] zero-padded)
//   the reductions (kernels.hip: nei_*_kernel).
// Only Sigma_bb is ever factored: the candidates may repeat.  Only S + 2 mc doubles and two ints leave the device, and nothing is
// written when the factor fails; the work matrices are borrowed for the call and go back cleared.
template <typename T>
static int model_noisy_ei(hbegp_model* m, const T* Xs, int cnt, int mb, const T* z, int S, double jitter, double* nei, int* best,
                          double* fmin_draws, double* rho, int* info_out) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int mc = cnt - mb;
  const int mbp = round_up(mb, NB);
  const int rows = mc > 0 ? mbp + mc : mb;  // rows of the device copy of the points
  const int mp = round_up(rows, NB);
  const int Sp = round_up(S, NB);
  const int nbb = mbp / NB;
  // everything the call borrows, counted before anything is taken: an m far beyond the device is ENOMEM, not an overflow
  const double need = (double)sizeof(T) * (2.0 * (double)mp * mp + (double)mbp * mp + (double)Sp * mbp + (double)Sp * mp + (double)mbp +
                                           2.0 * (double)mp * m->np) + 8.0 * ((double)S + 2.0 * mc);
  if (need > 1e15) return fail(HBEGP_ENOMEM, "the noisy expected improvement over %d points needs %.3g bytes of device memory", cnt, need);
  std::vector<T> hx;  // declared before the scratch: it outlives the stream work
  if (mc > 0 && mbp > mb) {
    const size_t d = (size_t)m->d;
    hx.resize((size_t)rows * d);
    std::copy(Xs, Xs + (size_t)mb * d, hx.begin());
    for (int g = mb; g < mbp; ++g) std::copy(Xs, Xs + d, hx.begin() + (size_t)g * d);
    std::copy(Xs + (size_t)mb * d, Xs + (size_t)cnt * d, hx.begin() + (size_t)mbp * d);
  }
  predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  int* info = &m->dOut->info;
  const double noise = 1e-5 + jitter;  // as model_posterior (copied from here: outlives the stream work)
  CallScratch ws{m->dev, s, {}};
  T* W1 = static_cast<T*>(ws.get(sizeof(T) * (size_t)mp * mp));
  T* W2 = static_cast<T*>(ws.get(sizeof(T) * (size_t)mbp * mp));  // X_b: the baseline's rows only
  T* W3 = static_cast<T*>(ws.get(sizeof(T) * (size_t)mp * mp));
  T* ld = static_cast<T*>(ws.get(sizeof(T) * (size_t)mbp));
  T* Z = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * mbp));
  T* Y = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * mp));
  double* dfmin = static_cast<double*>(ws.get(sizeof(double) * ((size_t)S + 2 * (size_t)mc)));
  double* drho = dfmin + S;
  double* dnei = drho + mc;
  int* dbest = static_cast<int*>(ws.get(sizeof(int)));
  PhaseClock clk(t_phase[PH_NEI].on, 5);
  clk.mark(s);
  posterior_sigma<T>(m, hx.empty() ? Xs : hx.data(), rows, mp, &noise, W1, nullptr);
  if (mc > 0) launch_nei_pad<T>(W1, mp, mb, mbp, s);  // without candidates kmat's own identity padding follows the baseline
  clk.mark(s);
  // triangular operands must be zero above the diagonal in memory, and a recycled block holds its earlier owner's numbers
  HIPCHECK(hipMemsetAsync(W2, 0, sizeof(T) * (size_t)mbp * mp, s));
  HIPCHECK(hipMemsetAsync(W3, 0, sizeof(T) * (size_t)mp * mp, s));
  chol_inv_rec<T>(W1, W2, W3, mp, 0, nbb / 2, nbb, false, true, [&](GemmLaunch& g, int) { gemm_adhoc<T>(g, info, s); },
                  [&](int k) { launch_leaf_keep<T>(W1, W2, W3, mp, k, ld, info, s); });
  clk.mark(s);
  if (mp > mbp) {
    // A = Sigma_cb X_b^T below L_b  (X_b lower: k <= j)
    GemmLaunch g{};
    g.nops = 1;
    GemmOp& op = g.op[0];
    op.A = W1; op.B = W2; op.C = W3;
    op.lda = mp; op.ldb = mp; op.ldc = mp;
    op.ci0 = nbb; op.mi = mp / NB - nbb; op.cj0 = 0; op.nj = nbb;
    op.k0 = 0; op.k1 = nbb; op.klim = 1; op.maskB = 1;
    gemm_adhoc<T>(g, info, s);
  }
  HIPCHECK(hipMemsetAsync(Z, 0, sizeof(T) * (size_t)Sp * mbp, s));
  HIPCHECK(hipMemcpy2DAsync(Z, sizeof(T) * mbp, z, sizeof(T) * mb, sizeof(T) * mb, S, hipMemcpyHostToDevice, s));
  {
    // Y = Z [L_b; A]^T: Y[s][i] = sum_k z_s[k] W3[i][k] over the baseline's columns (L_b lower: k <= j inside its block range)
    GemmLaunch g = gemm_lower_b(Z, mbp, W3, mp, Y, mp, Sp / NB, mp / NB, nbb);
    gemm_adhoc<T>(g, info, s);
  }
  clk.mark(s);
  launch_nei_reduce<T>(W1, W3, Y, mp, static_cast<const T*>(m->mean), mb, mbp, mc, S, dfmin, drho, dnei, dbest, info, s);
  clk.mark(s);
  CHECK_LAUNCHES();
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, m->dOut, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_NEI, 4);
  if (info_out) *info_out = out.info;
  if (out.info != 0) return fail(HBEGP_NOT_PD, "the baseline block of Sigma is not positive definite (pivot panel at column %d); a larger "
                                 "jitter may help", out.info - 1);
  int b = -1;
  if (mc > 0) HIPCHECK(hipMemcpyAsync(nei, dnei, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
  if (mc > 0 && best) HIPCHECK(hipMemcpyAsync(&b, dbest, sizeof(int), hipMemcpyDeviceToHost, s));
  if (mc > 0 && rho) HIPCHECK(hipMemcpyAsync(rho, drho, sizeof(double) * (size_t)mc, hipMemcpyDeviceToHost, s));
  if (fmin_draws) HIPCHECK(hipMemcpyAsync(fmin_draws, dfmin, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (best) *best = b;
  return HBEGP_OK;
}

// the chunk partial sums of one slab of base rows stay under this many bytes (one row's worth where a single row needs more)
constexpr size_t SENS_PART_CAP = (size_t)128 << 20;

// Sobol indices (G = 0: A, B [N][d] -> first, total, f0, variance and the optional f_a, f_b [N], f_ab [d][N]) and main-effect
// curves (G > 0: A [N][d], grid [d][G] -> effect [d][G] and the optional f_a) of the posterior mean.  The base
// rows (A, then B) go to the device once; they are evaluated in slabs of rows so that sens_kernel's chunk partial sums stay under
// SENS_PART_CAP (HBEGP_SENS_SLAB_ROWS, read per call, forces a slab size: tests).  Every value depends on its own row only and
// the row sums of the main effects continue from slab to slab in ascending row order, so the slab size never shows in a result.
// No query matrix and no Kstar exist; everything is borrowed for the call and goes back cleared.
template <typename T>
static int model_sensitivity(hbegp_model* m, const T* A, const T* B, int N, const T* grid, int G, double* first, double* total, double* f0,
                             double* variance, T* f_a, T* f_b, T* f_ab, double* effect) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int d = m->d, nch = sens_chunks(m->n);
  const bool sobol = G == 0;
  const size_t mrows = (size_t)N * (sobol ? 2 : 1);
  const size_t nv = 1 + (size_t)d * (sobol ? 1 : G);
  const size_t row_bytes = sizeof(double) * (size_t)nch * nv;
  size_t slab = std::max<size_t>(1, SENS_PART_CAP / row_bytes);
  if (slab >= 4) slab = slab / 4 * 4;  // whole workgroups of four rows
  const int forced = env_int("HBEGP_SENS_SLAB_ROWS", 0);
  if (forced > 0) slab = (size_t)forced;
  slab = std::min(slab, mrows);
  // everything the call borrows, counted before anything is taken: an N or G far beyond the device is ENOMEM, not an overflow
  const double need = (double)sizeof(T) * ((double)mrows * (d + 1) + (double)d * G + (sobol ? (double)d * N : 0.0)) +
                      (double)row_bytes * (double)slab + 8.0 * (double)nv;
  if (need > 1e15 || mrows > ((size_t)1 << 29) || nv > ((size_t)1 << 28) || mrows * d > ((size_t)1 << 40))
    return fail(HBEGP_ENOMEM, "the sensitivity call over %d rows (G = %d) needs %.3g bytes of device memory", N, G, need);
  hipStream_t s = m->stream;
  CallScratch ws{m->dev, s, {}};
  T* dXb = static_cast<T*>(ws.get(sizeof(T) * mrows * d));
  T* dsub = sobol ? dXb + (size_t)N * d : static_cast<T*>(ws.get(sizeof(T) * (size_t)d * G));
  double* part = static_cast<double*>(ws.get(row_bytes * slab));
  T* fbase = static_cast<T*>(ws.get(sizeof(T) * mrows));
  T* fsub = sobol ? static_cast<T*>(ws.get(sizeof(T) * (size_t)d * N)) : nullptr;
  double* dres = static_cast<double*>(ws.get(sizeof(double) * (sobol ? (size_t)2 * d + 2 : (size_t)d * G)));
  PhaseClock clk(t_phase[PH_SENS].on, 3 + 2 * ((mrows + slab - 1) / slab));
  clk.mark(s);
  HIPCHECK(hipMemcpyAsync(dXb, A, sizeof(T) * (size_t)N * d, hipMemcpyHostToDevice, s));
  if (sobol) {
    HIPCHECK(hipMemcpyAsync(dsub, B, sizeof(T) * (size_t)N * d, hipMemcpyHostToDevice, s));
  } else {
    HIPCHECK(hipMemcpyAsync(dsub, grid, sizeof(T) * (size_t)d * G, hipMemcpyHostToDevice, s));
    launch_sens_scale_grid<T>(dsub, d, G, m->dP, s);
    HIPCHECK(hipMemsetAsync(dres, 0, sizeof(double) * (size_t)d * G, s));  // the row sums start from zero
  }
  clk.mark(s);
  for (size_t r0 = 0; r0 < mrows; r0 += slab) {
    const int rows = (int)std::min(slab, mrows - r0);
    hipEvent_t mid = clk.slot();
    launch_sens_eval<T>(dXb, (int)r0, rows, N, dsub, G, static_cast<const T*>(m->X), m->n, d, m->nu2, m->dP, static_cast<const T*>(m->alpha),
                        part, fbase, fsub, s, mid);
    if (!sobol) launch_sens_effect(part, rows, d, G, dres, N, r0 + slab >= mrows, s);
    clk.mark(s);
  }
  if (sobol) launch_sobol_reduce<T>(fbase, fsub, N, d, dres, s);
  CHECK_LAUNCHES();
  std::vector<double> res(sobol ? (size_t)2 * d + 2 : 0);
  if (sobol) {
    HIPCHECK(hipMemcpyAsync(res.data(), dres, sizeof(double) * res.size(), hipMemcpyDeviceToHost, s));
    if (f_b) HIPCHECK(hipMemcpyAsync(f_b, fbase + N, sizeof(T) * (size_t)N, hipMemcpyDeviceToHost, s));
    if (f_ab) HIPCHECK(hipMemcpyAsync(f_ab, fsub, sizeof(T) * (size_t)d * N, hipMemcpyDeviceToHost, s));
  } else {
    HIPCHECK(hipMemcpyAsync(effect, dres, sizeof(double) * (size_t)d * G, hipMemcpyDeviceToHost, s));
  }
  if (f_a) HIPCHECK(hipMemcpyAsync(f_a, fbase, sizeof(T) * (size_t)N, hipMemcpyDeviceToHost, s));
  clk.mark(s);
  HIPCHECK(hipStreamSynchronize(s));
  if (sobol) {
    for (int k = 0; k < d; ++k) {
      first[k] = res[k];
      total[k] = res[d + k];
    }
    if (f0) *f0 = res[2 * (size_t)d];
    if (variance) *variance = res[2 * (size_t)d + 1];
  }
  if (clk.on()) {
    // marks: start, uploaded, then (mid, end) per slab, then the end of the call
    double* ms = t_phase[PH_SENS].ms;
    const int last = clk.marks() - 1;
    ms[0] = clk.elapsed_ms(0, 1);
    ms[1] = ms[2] = 0;
    for (int i = 2; i + 1 < last; i += 2) {
      ms[1] += clk.elapsed_ms(i - 1, i);
      ms[2] += clk.elapsed_ms(i, i + 1);
    }
    ms[3] = clk.elapsed_ms(last - 1, last);
  }
  return HBEGP_OK;
}

// Expected improvement of acquisition.rs:141-171 (estimator.expected_improvement) at mean mu and variance var, and its gradient
// from the posterior gradients: dEI = -Phi(z) dmu + phi(z) dsigma, dsigma = dvar / (2 sigma); sigma = 0: -dmu where mu < fmin.
static double ei_with_gradient(double mu, double var, const double* dmu, const double* dvar, double fmin, int d, double* g) {
  const double sd = std::sqrt(var);
  if (sd <= 0.0 || std::fabs(sd) <= std::numeric_limits<double>::epsilon()) {  // ulps_eq!(std, 0.0)
    for (int k = 0; k < d; ++k) g[k] = mu < fmin ? -dmu[k] : 0.0;
    return mu < fmin ? -(mu - fmin) : 0.0;
  }
  const double z = -(mu - fmin) / sd;
  const double cdf = 0.5 * std::erfc(-z / std::sqrt(2.0));
  const double pdf = std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI);
  const double ei = -(mu - fmin) * cdf + sd * pdf;
  for (int k = 0; k < d; ++k) g[k] = -cdf * dmu[k] + pdf * (dvar[k] / (2.0 * sd));
  return std::max(ei, 0.0);
}

// the lockstep driver's options for the posterior-side optimisers: the fit optimiser's constants
static LockstepOptions lockstep_options(int maxeval, bool maximize) {
  const LbfgsOptions o;
  return LockstepOptions{maxeval, o.memory, o.pgtol, o.ftol, maximize};
}

// S bounded L-BFGS runs on -EI in lockstep (lockstep.hpp): every round evaluates the points of the unfinished runs with ONE
// model_predict_grad.  Each run returns the best point it evaluated; a prediction that is not finite is a failed evaluation.
template <typename T>
static int model_maximize_ei(hbegp_model* m, const T* starts, int S, const double* lo, const double* hi, double fmin, int maxeval,
                             T* x_out, double* ei_out, int* nevals_out) {
  const int d = m->d;
  std::vector<T> mu(S), var(S), dmu((size_t)S * d), dvar((size_t)S * d);
  std::vector<double> dmu_d(d), dvar_d(d);
  auto eval = [&](const T* xs, const int*, int cnt, double* val, double* grad, char* ok) {
    const int rc = model_predict_grad<T>(m, xs, cnt, mu.data(), var.data(), dmu.data(), dvar.data(), nullptr);
    if (rc != HBEGP_OK) return rc;
    for (int i = 0; i < cnt; ++i) {
      for (int k = 0; k < d; ++k) {
        dmu_d[k] = (double)dmu[(size_t)i * d + k];
        dvar_d[k] = (double)dvar[(size_t)i * d + k];
      }
      const double mu_i = (double)mu[i], var_i = (double)var[i];
      ok[i] = std::isfinite(mu_i) && std::isfinite(var_i);
      if (ok[i]) val[i] = ei_with_gradient(mu_i, var_i, dmu_d.data(), dvar_d.data(), fmin, d, grad + (size_t)i * d);
    }
    return (int)HBEGP_OK;
  };
  return lockstep_optimize<T, LbfgsState>(starts, S, d, lo, hi, lockstep_options(maxeval, true), eval, x_out, ei_out, nevals_out);
}

// ---- acquisition functions of K independent models' marginal posteriors: EHVI, cEI, log-cEI, MES, EHVI over boxes

// the mutexes of K models, taken in the order of the models' addresses: calls that name the same models in any order cannot wait
// for each other
struct ModelsLock {
  std::vector<std::unique_lock<std::mutex>> locks;
  ModelsLock(hbegp_model* const* M, int K) {
    std::vector<hbegp_model*> order(M, M + K);
    std::sort(order.begin(), order.end(), std::less<hbegp_model*>());
    locks.reserve((size_t)K);
    for (hbegp_model* m : order) locks.emplace_back(m->mu);
  }
};

// the events M[0]'s stream waits on, one per further model, for the length of one C call (a maximiser's rounds share them)
struct JoinEvents {
  std::vector<hipEvent_t> ev;
  JoinEvents() = default;  // one model: nothing to join, no device call
  JoinEvents(int dev, int n) {
    HIPCHECK(hipSetDevice(dev));
    ev.reserve((size_t)n);
    for (int k = 0; k < n; ++k) {
      hipEvent_t e = nullptr;
      HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ev.push_back(e);
    }
  }
  ~JoinEvents() {
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  JoinEvents(const JoinEvents&) = delete;
  JoinEvents& operator=(const JoinEvents&) = delete;
};

// what marginal_acquisition hands the entry point's launch, all of it on the device
template <typename T>
struct MarginalCall {
  CeiArgs<T> p;          // K and the K posteriors: mean / var [cnt], dmean / dvar [cnt][d] (null without a gradient); thr is the launch's
  int cnt, d, want_grad;
  const double* params;  // the uploaded parameters
  const void* bytes;     // the uploaded byte parameters (null without any)
  void* scratch;         // the call's device scratch (null without any; its contents are whatever the pool block held)
  double* val;           // [n_val][cnt], the first cnt the acquisition value the arg-max runs over
  T* grad;               // [cnt][d] (null without a gradient)
  int* best;
  hipStream_t s;         // M[0]'s stream
};

// An acquisition function at cnt >= 1 candidates that reads nothing of the K models (M[0] first) but each one's marginal posterior
// at every candidate.  The call's bytes are counted before anything is taken (an m far beyond the device is ENOMEM, not an
// overflow; what_fmt names the call over (cnt, K)), then all K mutexes are taken (ModelsLock).  Each model's upload and predict
// launches -- hbegp_predict's batched ones, or hbegp_predict_grad's with a gradient, in their order -- go to its own stream; every
// further model's stream records its event (join: K - 1 of them); M[0]'s stream also uploads params [n_params] (thresholds, y*;
// may be empty) behind its candidates -- ahead of its launches: a copy behind them would wait for them, and with one model nothing
// hides that -- waits for all the events and runs launch(MarginalCall) -- the entry point's kernel and the arg-max -- and every copy
// back: vals (n_val = vals.size() arrays of cnt, each may be null but the first), best, grad (null: no gradient is computed) and
// mean_out / var_out [cnt][K] (may be null): the K posteriors of a row, M[0]'s first.  Parameters and outputs are borrowed for the
// call (CallScratch) and go back cleared; each is written in full before it is read.
// The marks of a timed call: EHVI, whose record is each model's own interval and then the kernel's, marks around every model's
// upload and launches on that model's stream (2 k, 2 k + 1); the others, whose record runs from before M[0]'s upload to the join and
// then over the kernel, mark before M[0]'s upload alone.  Both then mark behind the join and behind the arg-max on M[0]'s stream.
// A call may also upload byte parameters (x.bytes [x.n_bytes]: EHVI over boxes' index list, behind params on M[0]'s stream) and borrow
// x.scratch_bytes of device scratch for its kernel; a call without either issues exactly the copies and launches described above.
struct MarginalExtra {
  const void* bytes = nullptr;
  size_t n_bytes = 0;
  double scratch_bytes = 0.0;  // a double: counted before anything is taken, it may be far beyond the device
};
template <typename T, class Launch>
static int marginal_acquisition(hbegp_model* const* M, int K, const T* Xs, int cnt, const JoinEvents& join, PhaseKind kind,
                                const char* what_fmt, const double* params, size_t n_params, const MarginalExtra& x,
                                std::initializer_list<double*> vals, T* grad, int* best, T* mean_out, T* var_out, Launch&& launch) {
  const bool want_grad = grad != nullptr;
  const int d = M[0]->d;
  const size_t n_val = vals.size();
  const double rows = padded_rows((double)cnt);
  double need = 8.0 * n_val * cnt + 8.0 * n_params + (want_grad ? (double)sizeof(T) * cnt * d : 0.0) + (double)x.n_bytes + x.scratch_bytes;
  for (int k = 0; k < K; ++k) need += predict_bytes<T>(M[k], rows, want_grad);
  if (need > 1e15 || rows > (double)(1 << 30)) {
    char what[96];
    snprintf(what, sizeof(what), what_fmt, cnt, K);
    return fail(HBEGP_ENOMEM, "%s needs %.3g bytes of device memory", what, need);
  }
  ModelsLock lock(M, K);
  HIPCHECK(hipSetDevice(M[0]->dev));
  const int mp = round_up(cnt, NB);
  for (int k = 0; k < K; ++k) {
    if (want_grad) predict_grad_reserve<T>(M[k], mp);
    else predict_batched_reserve<T>(M[k], mp);
  }
  hipStream_t s0 = M[0]->stream;
  CallScratch ws{M[0]->dev, s0, {}};
  MarginalCall<T> c{};
  c.cnt = cnt;
  c.d = d;
  c.want_grad = want_grad ? 1 : 0;
  c.s = s0;
  double* dparams = n_params ? static_cast<double*>(ws.get(sizeof(double) * n_params)) : nullptr;
  c.params = dparams;
  void* dbytes = x.n_bytes ? ws.get(x.n_bytes) : nullptr;
  c.bytes = dbytes;
  c.scratch = x.scratch_bytes > 0.0 ? ws.get((size_t)x.scratch_bytes) : nullptr;
  c.val = static_cast<double*>(ws.get(sizeof(double) * n_val * (size_t)cnt));
  c.best = static_cast<int*>(ws.get(sizeof(int)));
  c.grad = want_grad ? static_cast<T*>(ws.get(sizeof(T) * (size_t)cnt * d)) : nullptr;
  const bool per_model = kind == PH_EHVI || kind == PH_EHVI_ND;  // the record times every model's stream, not M[0]'s alone
  PhaseClock clk(t_phase[kind].on, 2 * (size_t)K + 2);
  c.p.K = K;
  for (int k = 0; k < K; ++k) {
    hbegp_model* m = M[k];
    hipStream_t s = m->stream;
    if (per_model || k == 0) clk.mark(s);
    HIPCHECK(hipMemcpyAsync(m->Xs, Xs, sizeof(T) * (size_t)cnt * d, hipMemcpyHostToDevice, s));
    if (k == 0 && n_params) HIPCHECK(hipMemcpyAsync(dparams, params, sizeof(double) * n_params, hipMemcpyHostToDevice, s0));
    if (k == 0 && x.n_bytes) HIPCHECK(hipMemcpyAsync(dbytes, x.bytes, x.n_bytes, hipMemcpyHostToDevice, s0));
    predict_batched_launches<T>(m, cnt, mp, true);
    if (want_grad) predict_grad_launches<T>(m, cnt, mp, true, true);
    CHECK_LAUNCHES();
    if (per_model) clk.mark(s);
    if (k > 0) HIPCHECK(hipEventRecord(join.ev[(size_t)k - 1], s));
    c.p.mean[k] = static_cast<const T*>(m->mean);
    c.p.var[k] = static_cast<const T*>(m->var);
    c.p.dmean[k] = want_grad ? static_cast<const T*>(m->dmean) : nullptr;  // (not read without a gradient)
    c.p.dvar[k] = want_grad ? static_cast<const T*>(m->dvar) : nullptr;
  }
  for (int k = 1; k < K; ++k) HIPCHECK(hipStreamWaitEvent(s0, join.ev[(size_t)k - 1], 0));
  const int joined = clk.marks();
  clk.mark(s0);
  launch(c);
  clk.mark(s0);
  CHECK_LAUNCHES();
  int hbest = -1;
  std::vector<T> hm, hv;
  size_t at = 0;
  for (double* v : vals) {
    if (v) HIPCHECK(hipMemcpyAsync(v, c.val + at * cnt, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, s0));
    ++at;
  }
  HIPCHECK(hipMemcpyAsync(&hbest, c.best, sizeof(int), hipMemcpyDeviceToHost, s0));
  if (want_grad) HIPCHECK(hipMemcpyAsync(grad, c.grad, sizeof(T) * (size_t)cnt * d, hipMemcpyDeviceToHost, s0));
  if (mean_out) {
    hm.resize((size_t)K * cnt);
    for (int k = 0; k < K; ++k)
      HIPCHECK(hipMemcpyAsync(hm.data() + (size_t)k * cnt, M[k]->mean, sizeof(T) * (size_t)cnt, hipMemcpyDeviceToHost, s0));
  }
  if (var_out) {
    hv.resize((size_t)K * cnt);
    for (int k = 0; k < K; ++k)
      HIPCHECK(hipMemcpyAsync(hv.data() + (size_t)k * cnt, M[k]->var, sizeof(T) * (size_t)cnt, hipMemcpyDeviceToHost, s0));
  }
  HIPCHECK(hipStreamSynchronize(s0));  // behind the events: every further model's stream has finished this call's work too
  if (best) *best = hbest;
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < cnt; ++i) {
      if (mean_out) mean_out[(size_t)K * i + k] = hm[(size_t)k * cnt + i];
      if (var_out) var_out[(size_t)K * i + k] = hv[(size_t)k * cnt + i];
    }
  if (clk.on()) {
    double* ms = t_phase[kind].ms;
    if (per_model)
      for (int k = 0; k < K; ++k) ms[k] = clk.elapsed_ms(2 * k, 2 * k + 1);
    else ms[0] = clk.elapsed_ms(0, joined);
    ms[per_model ? K : 1] = clk.elapsed_ms(joined, joined + 1);
    if (kind == PH_EHVI_ND)
      for (int k = K + 1; k < 5; ++k) ms[k] = 0.0;  // a record of n_obj + 1 phases: nothing of an earlier call with more objectives stays
  }
  return HBEGP_OK;
}
// the call without byte parameters or scratch (EHVI, cEI, log-cEI, MES)
template <typename T, class Launch>
static int marginal_acquisition(hbegp_model* const* M, int K, const T* Xs, int cnt, const JoinEvents& join, PhaseKind kind,
                                const char* what_fmt, const double* params, size_t n_params, std::initializer_list<double*> vals,
                                T* grad, int* best, T* mean_out, T* var_out, Launch&& launch) {
  return marginal_acquisition<T>(M, K, Xs, cnt, join, kind, what_fmt, params, n_params, MarginalExtra{}, vals, grad, best, mean_out, var_out,
                                 launch);
}

// S bounded L-BFGS runs on the negative of such a function in lockstep (lockstep.hpp), as model_maximize_ei: every round is ONE call
// of rows(xs, cnt, val, gr) -- the entry point's call with a gradient: one batched gradient predict per model, then its kernel.
// Each run returns the best point it evaluated; a value or a gradient component that is not finite is a failed evaluation (in
// log space a row at -inf is one).
template <typename T, class Rows>
static int maximize_marginal(const T* starts, int S, int d, const double* lo, const double* hi, int maxeval, Rows rows, T* x_out,
                             double* f_out, int* nevals_out) {
  return lockstep_optimize<T, LbfgsState>(starts, S, d, lo, hi, lockstep_options(maxeval, true), finite_gradient_eval<T>(S, d, rows), x_out,
                                          f_out, nevals_out);
}
// The same runs on the function itself (hbegp_minimize_confidence_bound): maximize = false is the driver's only difference.
// nan_start[r] != 0 marks a run whose start has a NaN coordinate: lbfgs_begin would clip that coordinate to lo and the run would
// set off from a point the caller never named, so every evaluation of such a run counts as failed -- it ends after one, keeps
// its start and reports +inf; the other runs never see it.
template <typename T, class Rows>
static int minimize_marginal(const T* starts, int S, int d, const double* lo, const double* hi, int maxeval, Rows rows, T* x_out,
                             double* f_out, int* nevals_out) {
  std::vector<char> nan_start((size_t)S, 0);
  for (int r = 0; r < S; ++r)
    for (int k = 0; k < d; ++k)
      if (starts[(size_t)r * d + k] != starts[(size_t)r * d + k]) nan_start[r] = 1;
  auto inner = finite_gradient_eval<T>(S, d, rows);
  auto eval = [&](const T* xs, const int* runs, int cnt, double* val, double* grad, char* ok) mutable -> int {
    if (const int rc = inner(xs, runs, cnt, val, grad, ok)) return rc;
    for (int i = 0; i < cnt; ++i)
      if (nan_start[runs[i]]) ok[i] = 0;
    return 0;
  };
  return lockstep_optimize<T, LbfgsState>(starts, S, d, lo, hi, lockstep_options(maxeval, false), eval, x_out, f_out, nevals_out);
}

// ---- expected hypervolume improvement of two independent objectives (hbegp_ehvi / hbegp_maximize_ehvi) ----------

// The caller's front reduced to the non-dominated points strictly inside the reference box, a ascending (so b descends), as the
// kernel's strips: thr = [up | hb], ns = P' + 1 each; up = a_1 .. a_P', r1 and hb = r2, b_1 .. b_P'.  The result depends on the set
// of points only: not on their order, on duplicates, on dominated points or on points outside the box.
static int ehvi_thresholds(const double* front, int P, const double* ref, std::vector<double>* thr) {
  std::vector<std::pair<double, double>> pts;
  pts.reserve((size_t)P);
  for (int i = 0; i < P; ++i)
    if (front[2 * (size_t)i] < ref[0] && front[2 * (size_t)i + 1] < ref[1]) pts.push_back({front[2 * (size_t)i], front[2 * (size_t)i + 1]});
  std::sort(pts.begin(), pts.end());
  std::vector<double> a, b;
  double bmin = ref[1];
  for (const auto& p : pts)
    if (p.second < bmin) {  // among equal a the lowest b comes first and dominates the others
      a.push_back(p.first);
      b.push_back(p.second);
      bmin = p.second;
    }
  const int ns = (int)a.size() + 1;
  thr->assign(2 * (size_t)ns, 0.0);
  for (int i = 0; i + 1 < ns; ++i) {
    (*thr)[i] = a[i];
    (*thr)[ns + i + 1] = b[i];
  }
  (*thr)[ns - 1] = ref[0];
  (*thr)[ns] = ref[1];
  return ns;
}

// EHVI at cnt >= 1 candidates: marginal_acquisition over the two objectives' models, the thresholds its parameters
template <typename T>
static int model_ehvi(hbegp_model* const* M, const T* Xs, int cnt, const std::vector<double>& thr, int ns, const JoinEvents& join,
                      double* ehvi, T* grad, int* best, T* mean_out, T* var_out) {
  return marginal_acquisition<T>(M, 2, Xs, cnt, join, PH_EHVI, "EHVI at %d points", thr.data(), 2 * (size_t)ns, {ehvi}, grad, best, mean_out,
                                 var_out, [&](const MarginalCall<T>& c) {
                                   launch_ehvi<T>(c.p.mean[0], c.p.var[0], c.p.dmean[0], c.p.dvar[0], c.p.mean[1], c.p.var[1], c.p.dmean[1],
                                                  c.p.dvar[1], cnt, c.d, c.params, ns, c.want_grad, c.val, c.grad, c.best, c.s);
                                 });
}

// ---- expected hypervolume improvement of 2 .. 4 independent objectives (hbegp_ehvi_nd / hbegp_maximize_ehvi_nd) ---

// What one C call makes of its front, once, on the host (a maximiser's rounds share it): objective k's thresholds thr[k] = -inf, the
// distinct k-th coordinates of the reduced front ascending, r_k; and the disjoint boxes [l, u) whose union is the part of (-inf, r)
// that no front point weakly dominates, per box (l_0, u_0, l_1, u_1, ..) as indices into the thresholds (0 = -inf).
struct EhviNdPlan {
  int n_obj = 0;
  std::vector<double> thr[EHVI_ND_MAX_OBJ];
  std::vector<int> boxes;
  size_t n_boxes = 0;
};
typedef std::array<int, EHVI_ND_MAX_OBJ> EhviNdPt;

// The non-dominated ones among distinct points, looking at the coordinates k0 .. M - 1 only, sorted by those coordinates
// lexicographically: a canonical form of the set.  A point is dropped when another one is <= it in every coordinate looked at (so
// of points equal there one stays).  Sorted, only an earlier point can dominate a later one; with two coordinates that is "the
// second coordinate is not below the running minimum", with one only the first point stays.
template <typename P>
static void ehvi_nd_reduce(std::vector<P>* pts, int k0, int M) {
  auto less = [&](const P& a, const P& b) {
    for (int k = k0; k < M; ++k)
      if (a[k] != b[k]) return a[k] < b[k];
    return false;
  };
  std::sort(pts->begin(), pts->end(), less);
  std::vector<P> keep;
  for (const P& p : *pts) {
    bool dominated = false;
    if (M - k0 <= 2) {
      dominated = !keep.empty() && (M - k0 == 1 || !(p[M - 1] < keep.back()[M - 1]));
    } else {
      for (const P& q : keep) {
        bool le = true;
        for (int k = k0; k < M && le; ++k) le = q[k] <= p[k];
        if (le) { dominated = true; break; }
      }
    }
    if (!dominated) keep.push_back(p);
  }
  pts->swap(keep);
}

// The sweep over objective k of points that are reduced in the objectives k .. M - 1 (as ranks: indices into the thresholds): the
// slab below the lowest k-th coordinate holds no point, the slab from the s-th distinct coordinate to the next one (the last: to
// r_k) the points up to the s-th; each slab's points are projected onto the objectives behind k, reduced and swept in turn.  With
// one objective left the free region is (-inf, the lowest coordinate); with two, the slabs of the points sorted by the first are
// the free strips directly (the second coordinate descends).  box holds the (l, u) of the objectives before k.  False once the
// boxes would pass cap.
static bool ehvi_nd_sweep(int k, int M, const std::vector<EhviNdPt>& pts, const int* top, int* box, EhviNdPlan* plan, size_t cap) {
  auto emit = [&]() {
    if (plan->n_boxes == cap) return false;
    plan->boxes.insert(plan->boxes.end(), box, box + 2 * M);
    ++plan->n_boxes;
    return true;
  };
  if (k == M - 1) {
    int u = top[k];
    for (const EhviNdPt& p : pts) u = std::min(u, p[k]);
    box[2 * k] = 0;
    box[2 * k + 1] = u;
    return emit();
  }
  const size_t n = pts.size();  // sorted by (k, k + 1, ..): ehvi_nd_reduce's order
  if (k == M - 2) {
    for (size_t s = 0; s <= n; ++s) {
      box[2 * k] = s ? pts[s - 1][k] : 0;
      box[2 * k + 1] = s < n ? pts[s][k] : top[k];
      box[2 * k + 2] = 0;
      box[2 * k + 3] = s ? pts[s - 1][k + 1] : top[k + 1];
      if (!emit()) return false;
    }
    return true;
  }
  std::vector<EhviNdPt> proj;  // the reduced projection of the points [0, s): the previous slab's with the new points, reduced again
  size_t taken = 0;
  for (size_t s = 0; s <= n;) {  // the points [0, s) lie at or below the slab's lower edge
    size_t e = s;                // the slab's upper edge: the next distinct coordinate
    if (s < n)
      while (e < n && pts[e][k] == pts[s][k]) ++e;
    box[2 * k] = s ? pts[s - 1][k] : 0;
    box[2 * k + 1] = s < n ? pts[s][k] : top[k];
    if (s > taken) {
      proj.insert(proj.end(), pts.begin() + (long)taken, pts.begin() + (long)s);
      taken = s;
      ehvi_nd_reduce(&proj, k + 1, M);
    }
    if (!ehvi_nd_sweep(k + 1, M, proj, top, box, plan, cap)) return false;
    if (s == n) break;
    s = e;
  }
  return true;
}

// The plan of a front [P][M] below ref: the front reduced to its distinct non-dominated points strictly inside the box -- the result
// depends on that set only -- then the thresholds and the sweep.  HBEGP_ENOMEM past HBEGP_EHVI_ND_MAX_BOXES boxes.
static int ehvi_nd_plan(const double* front, int P, int M, const double* ref, EhviNdPlan* plan) {
  typedef std::array<double, EHVI_ND_MAX_OBJ> Pt;
  std::vector<Pt> pts;
  pts.reserve((size_t)P);
  for (int i = 0; i < P; ++i) {
    Pt p{};
    bool inside = true;
    for (int k = 0; k < M; ++k) {
      p[k] = front[(size_t)M * i + k];
      inside = inside && p[k] < ref[k];
    }
    if (inside) pts.push_back(p);
  }
  ehvi_nd_reduce(&pts, 0, M);
  plan->n_obj = M;
  plan->boxes.clear();
  plan->n_boxes = 0;
  int top[EHVI_ND_MAX_OBJ];
  for (int k = 0; k < M; ++k) {
    std::vector<double>& t = plan->thr[k];
    t.clear();
    for (const Pt& p : pts) t.push_back(p[k]);
    std::sort(t.begin(), t.end());
    t.erase(std::unique(t.begin(), t.end()), t.end());
    t.insert(t.begin(), -std::numeric_limits<double>::infinity());
    t.push_back(ref[k]);
    top[k] = (int)t.size() - 1;
  }
  std::vector<EhviNdPt> ranks(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) {
    ranks[i] = EhviNdPt{};
    for (int k = 0; k < M; ++k)
      ranks[i][k] = (int)(std::lower_bound(plan->thr[k].begin() + 1, plan->thr[k].end(), pts[i][k]) - plan->thr[k].begin());
  }
  int box[2 * EHVI_ND_MAX_OBJ];
  if (!ehvi_nd_sweep(0, M, ranks, top, box, plan, (size_t)HBEGP_EHVI_ND_MAX_BOXES))
    return fail(HBEGP_ENOMEM, "the front's free region splits into more than %d boxes (%d objectives, %d non-dominated points)",
                HBEGP_EHVI_ND_MAX_BOXES, M, (int)pts.size());
  return HBEGP_OK;
}

// what the kernel reads of a plan: the thresholds in one array, the boxes' indices moved to each objective's place in it
struct EhviNdUpload {
  EhviNdGeom g{};
  std::vector<double> thr;
  std::vector<int> boxes;
  explicit EhviNdUpload(const EhviNdPlan& plan) {
    const int M = plan.n_obj;
    g.n_obj = M;
    for (int k = 0; k < M; ++k) {
      g.T[k] = (int)plan.thr[k].size();
      g.off[k] = (int)thr.size();
      thr.insert(thr.end(), plan.thr[k].begin(), plan.thr[k].end());
    }
    g.nt = (int)thr.size();
    g.n_boxes = (int)plan.n_boxes;
    boxes = plan.boxes;
    for (size_t i = 0; i < boxes.size(); ++i) boxes[i] += g.off[(i % (2 * (size_t)M)) / 2];
  }
};

// EHVI over boxes at cnt >= 1 candidates: marginal_acquisition over the n_obj objectives' models, the thresholds its parameters, the
// boxes its byte parameters, the table of a front past the LDS regimes its scratch
template <typename T>
static int model_ehvi_nd(hbegp_model* const* M, const T* Xs, int cnt, const EhviNdUpload& u, const JoinEvents& join, double* ehvi, T* grad,
                         int* best, T* mean_out, T* var_out) {
  MarginalExtra x;
  x.bytes = u.boxes.data();
  x.n_bytes = sizeof(int) * u.boxes.size();
  x.scratch_bytes = u.g.nt > EHVI_ND_LDS1_ENTRIES ? 24.0 * u.g.nt * cnt : 0.0;
  return marginal_acquisition<T>(M, u.g.n_obj, Xs, cnt, join, PH_EHVI_ND, "EHVI over boxes at %d points under %d models", u.thr.data(),
                                 u.thr.size(), x, {ehvi}, grad, best, mean_out, var_out, [&](const MarginalCall<T>& c) {
                                   launch_ehvi_nd<T>(c.p, cnt, c.d, c.params, static_cast<const int*>(c.bytes), u.g,
                                                     static_cast<double*>(c.scratch), c.want_grad, c.val, c.grad, c.best, c.s);
                                 });
}

// ---- constrained expected improvement over an objective and C constraint models (hbegp_constrained_ei /
// hbegp_maximize_constrained_ei) ----------------------------------------------------------------------------

// cEI at cnt >= 1 candidates under K = 1 + C models, M[0] the objective: marginal_acquisition without parameters -- thr[0] = fmin,
// thr[k] = limits[k - 1] travel in the kernel's arguments -- and with three values, cei | ei | pof.  log_space
// (hbegp_log_constrained_ei) changes the kernel that follows the join -- lcei_kernel: cei / ei / pof receive
// lcei / lei / lpof -- and the phase record, nothing else.
template <typename T>
static int model_constrained_ei(hbegp_model* const* M, int K, const T* Xs, int cnt, const double* thr, const JoinEvents& join, double* cei,
                                T* grad, int* best, double* ei, double* pof, T* mean_out, T* var_out, bool log_space) {
  return marginal_acquisition<T>(M, K, Xs, cnt, join, log_space ? PH_LCEI : PH_CEI, "constrained EI at %d points under %d models", nullptr, 0,
                                 {cei, ei, pof}, grad, best, mean_out, var_out, [&](const MarginalCall<T>& c) {
                                   CeiArgs<T> a = c.p;
                                   std::copy(thr, thr + K, a.thr);
                                   double* v = c.val;
                                   if (log_space) launch_lcei<T>(a, cnt, c.d, c.want_grad, v, v + cnt, v + 2 * (size_t)cnt, c.grad, c.best, c.s);
                                   else launch_cei<T>(a, cnt, c.d, c.want_grad, v, v + cnt, v + 2 * (size_t)cnt, c.grad, c.best, c.s);
                                 });
}

// ---- max-value entropy search (hbegp_mes / hbegp_maximize_mes) ----------------------------------------------

// MES at cnt >= 1 candidates under ONE model and S sampled minimum values: marginal_acquisition over that model (nothing to join:
// all of it runs on the model's stream under the model's mutex), y* its parameters
template <typename T>
static int model_mes(hbegp_model* m, const T* Xs, int cnt, const double* ystar, int S, double* mes, T* grad, int* best, T* mean_out,
                     T* var_out) {
  const JoinEvents none;
  return marginal_acquisition<T>(&m, 1, Xs, cnt, none, PH_MES, "max-value entropy search at %d points", ystar, (size_t)S, {mes}, grad, best,
                                 mean_out, var_out, [&](const MarginalCall<T>& c) {
                                   launch_mes<T>(c.p.mean[0], c.p.var[0], c.p.dmean[0], c.p.dvar[0], cnt, c.d, c.params, S, c.want_grad, c.val,
                                                 c.grad, c.best, c.s);
                                 });
}

// ---- the confidence bound mu + kappa sigma (hbegp_confidence_bound / hbegp_minimize_confidence_bound) -----------

// The bound at cnt >= 1 candidates under ONE model: marginal_acquisition over that model without parameters -- kappa travels in the
// kernel's arguments, as cEI's thresholds do -- and *best the FIRST index of the minimum
template <typename T>
static int model_cb(hbegp_model* m, const T* Xs, int cnt, double kappa, double* cb, T* grad, int* best, T* mean_out, T* var_out) {
  const JoinEvents none;
  return marginal_acquisition<T>(&m, 1, Xs, cnt, none, PH_CB, "the confidence bound at %d points", nullptr, 0, {cb}, grad, best, mean_out,
                                 var_out, [&](const MarginalCall<T>& c) {
                                   launch_cb<T>(c.p.mean[0], c.p.var[0], c.p.dmean[0], c.p.dvar[0], cnt, c.d, kappa, c.want_grad, c.val, c.grad,
                                                c.best, c.s);
                                 });
}

// Batch expected improvement by Monte Carlo (hbegp_qei) for B batches of q points: the B q points go through the batched predict's
// launches (Kstar, mean, Q) and, with a gradient, the gradient's (dmean; G and W = G X^T), in the order hbegp_predict_grad issues
// them; then qei_batch_kernel, one workgroup per batch (kernels.hip).  Only qei[B], info[B] and grad[B q d] leave the device;
// z and the outputs are borrowed for the call (CallScratch), Q / W / dmean are the model's grow-only arrays.
template <typename T>
static int model_qei(hbegp_model* m, const T* Xb, int B, int q, const T* z, int S, double fmin, double jitter, double* qei, T* grad,
                     int* info_out) {
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const bool want_grad = grad != nullptr;
  const int d = m->d;
  // everything the call borrows, counted before anything is taken: a B far beyond the device is ENOMEM, not an overflow
  const double rows = padded_rows((double)B * q);
  const double need = predict_bytes<T>(m, rows, want_grad) + (double)sizeof(T) * S * q + 12.0 * B;
  if (need > 1e15 || rows > (double)(1 << 30))
    return fail(HBEGP_ENOMEM, "qEI of %d batches of %d points needs %.3g bytes of device memory", B, q, need);
  const int cnt = B * q;
  const int mp = round_up(cnt, NB);
  if (want_grad) predict_grad_reserve<T>(m, mp);
  else predict_batched_reserve<T>(m, mp);
  hipStream_t s = m->stream;
  const double noise = 1e-5 + jitter;  // predict_cov's diagonal
  CallScratch ws{m->dev, s, {}};
  T* dz = static_cast<T*>(ws.get(sizeof(T) * (size_t)S * q));
  double* dq = static_cast<double*>(ws.get(sizeof(double) * (size_t)B));
  int* dinfo = static_cast<int*>(ws.get(sizeof(int) * (size_t)B));
  T* dg = want_grad ? static_cast<T*>(ws.get(sizeof(T) * (size_t)cnt * d)) : nullptr;
  PhaseClock clk(t_phase[PH_QEI].on, 3);
  clk.mark(s);
  HIPCHECK(hipMemcpyAsync(m->Xs, Xb, sizeof(T) * (size_t)cnt * d, hipMemcpyHostToDevice, s));
  predict_batched_launches<T>(m, cnt, mp, true);
  if (want_grad) predict_grad_launches<T>(m, cnt, mp, true, false);
  HIPCHECK(hipMemcpyAsync(dz, z, sizeof(T) * (size_t)S * q, hipMemcpyHostToDevice, s));
  clk.mark(s);
  const T* W = want_grad ? static_cast<const T*>(m->W) : static_cast<const T*>(m->Q);         // (not read without a gradient)
  const T* dmean = want_grad ? static_cast<const T*>(m->dmean) : static_cast<const T*>(m->mean);
  launch_qei_batch<T>(static_cast<const T*>(m->Xs), B, q, d, static_cast<const T*>(m->Q), W, mp, m->np, static_cast<const T*>(m->mean),
                      dmean, m->dP, noise, m->nu2, dz, S, fmin, want_grad ? 1 : 0, dq, dg, dinfo, s);
  clk.mark(s);
  CHECK_LAUNCHES();
  std::vector<int> hinfo(B);
  HIPCHECK(hipMemcpyAsync(qei, dq, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(hinfo.data(), dinfo, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  if (want_grad) HIPCHECK(hipMemcpyAsync(grad, dg, sizeof(T) * (size_t)cnt * d, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_QEI, 2);
  if (info_out) memcpy(info_out, hinfo.data(), sizeof(int) * (size_t)B);
  for (int b = 0; b < B; ++b)
    if (hinfo[b] != 0)
      return fail(HBEGP_NOT_PD, "Sigma of batch %d is not positive definite (pivot at column %d); a larger jitter may help", b,
                  hinfo[b] - 1);
  return HBEGP_OK;
}

// R bounded L-BFGS runs on -qEI over q d coordinates each (the host state sized per run: q d exceeds LbfgsState's LBFGS_MAXN), the
// box [lo, hi] applied to every point, in lockstep (lockstep.hpp): every round is ONE model_qei over the runs still going, with
// the same z (a deterministic sample-average objective).  A batch whose factor failed is a failed evaluation, not an error of the
// call; a run whose every evaluation failed (its start batch included) keeps its start with qei_out = -inf, as maximize_ei does.
template <typename T>
static int model_maximize_qei(hbegp_model* m, const T* starts, int R, int q, const double* lo, const double* hi, const T* z, int S,
                              double fmin, double jitter, int maxeval, T* x_out, double* qei_out, int* nevals_out) {
  const int d = m->d, n = q * d;
  std::vector<double> lof(n), hif(n);
  for (int e = 0; e < n; ++e) {
    lof[e] = lo[e % d];
    hif[e] = hi[e % d];
  }
  std::vector<int> info(R);
  std::vector<T> gr((size_t)R * n);
  auto eval = [&](const T* xs, const int*, int cnt, double* val, double* grad, char* ok) {
    const int rc = model_qei<T>(m, xs, cnt, q, z, S, fmin, jitter, val, gr.data(), info.data());
    if (rc != HBEGP_OK && rc != HBEGP_NOT_PD) return rc;
    for (int i = 0; i < cnt; ++i) {
      ok[i] = info[i] == 0 && std::isfinite(val[i]);
      for (int e = 0; e < n; ++e) grad[(size_t)i * n + e] = (double)gr[(size_t)i * n + e];
    }
    return (int)HBEGP_OK;
  };
  const int rc = lockstep_optimize<T, LbfgsStateHost>(starts, R, n, lof.data(), hif.data(), lockstep_options(maxeval, true), eval, x_out,
                                                      qei_out, nevals_out);
  if (rc == HBEGP_OK) g_last_error.clear();  // a failed batch inside a round has left its message behind
  return rc;
}

// ---- leave-one-out cross-validation (hbegp_model_loo / hbegp_problem_eval_loo / hbegp_fit_loo) ----------

// The diagnostics from L^-1 and alpha (one memory-bound pass), and with `grad` the gradient of their sum: u = K^-1 a and
// Y = K^-1 diag(sqrt b) in one pass over K^-1, C = Y Y^T by ONE tile GEMM for all p parameters, and gradtrace's pass with the
// weight u alpha^T + alpha u^T - 2 C.  Y and C (np^2 elements each) are borrowed only with `grad`; everything borrowed goes
// back cleared.  Any of the outputs may be null.  A result that is not finite (NaN data) is HBEGP_NOT_PD: loo = -inf, grad = 0.
template <typename T>
static int loo_tail(const LooIn<T>& in, T* mean, T* var, T* lpd, double* loo, double* grad) {
  HIPCHECK(hipSetDevice(in.dev));
  const int n = in.n, np = in.np, p = in.d + 2;
  const size_t nn = (size_t)np * np;
  if (grad && 2.0 * (double)sizeof(T) * (double)np * np > 1e15)
    return fail(HBEGP_ENOMEM, "the leave-one-out gradient of %d rows needs %.3g bytes of device memory", n, 2.0 * sizeof(T) * (double)np * np);
  hipStream_t s = in.s;
  CallScratch ws{in.dev, s, {}};
  // the small arrays: one borrowed block
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t b_vec = up(sizeof(T) * np), b_dvec = up(sizeof(double) * np), b_out = up(sizeof(EvalOut));
  const size_t b_part = up(sizeof(double) * loo_diag_part_elems(np, n));
  const size_t b_pu = grad ? up(sizeof(double) * loo_u_part_elems(np)) : 0;
  const size_t b_pg = grad ? up(sizeof(double) * gradtrace_part_elems(np, in.d)) : 0;
  char* q = static_cast<char*>(ws.get(b_out + 4 * b_vec + 2 * b_dvec + b_part + b_pu + b_pg));
  EvalOut* dout = reinterpret_cast<EvalOut*>(q); q += b_out;
  T* dmean = reinterpret_cast<T*>(q); q += b_vec;
  T* dvar = reinterpret_cast<T*>(q); q += b_vec;
  T* dlpd = reinterpret_cast<T*>(q); q += b_vec;
  T* du = reinterpret_cast<T*>(q); q += b_vec;
  double* avec = reinterpret_cast<double*>(q); q += b_dvec;
  double* sbvec = reinterpret_cast<double*>(q); q += b_dvec;
  double* part = reinterpret_cast<double*>(q); q += b_part;
  double* pu = reinterpret_cast<double*>(q); q += b_pu;
  double* part_g = reinterpret_cast<double*>(q);
  HIPCHECK(hipMemsetAsync(dout, 0, sizeof(EvalOut), s));  // info = 0, done = 0 (a recycled block holds its earlier owner's numbers)
  PhaseClock clk(t_phase[PH_LOO].on && grad, 5);
  clk.mark(s);
  launch_loo_diag<T>(in.Xinv, np, n, in.y, in.alpha, part, dmean, dvar, dlpd, avec, sbvec, dout, s);
  clk.mark(s);
  if (grad) {
    T* Y = static_cast<T*>(ws.get(sizeof(T) * nn));
    T* Cm = static_cast<T*>(ws.get(sizeof(T) * nn));
    launch_loo_uy<T>(in.Kinv, np, n, avec, sbvec, Y, pu, du, s);
    clk.mark(s);
    {
      // C = Y Y^T (lower tiles), contraction over all columns of Y
      GemmLaunch g{};
      g.nops = 1;
      GemmOp& op = g.op[0];
      op.A = Y; op.B = Y; op.C = Cm;
      op.lda = op.ldb = op.ldc = np;
      op.mi = np / NB; op.nj = np / NB; op.c_lower = 1;
      op.k0 = 0; op.k1 = np / NB;
      gemm_adhoc<T>(g, &dout->info, s);
    }
    clk.mark(s);
    launch_loo_trace<T>(in.X, n, in.d, np, in.nu2, in.P, Cm, in.alpha, du, part_g, dout, s);
    clk.mark(s);
  }
  CHECK_LAUNCHES();
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, dout, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  if (mean) HIPCHECK(hipMemcpyAsync(mean, dmean, sizeof(T) * n, hipMemcpyDeviceToHost, s));
  if (var) HIPCHECK(hipMemcpyAsync(var, dvar, sizeof(T) * n, hipMemcpyDeviceToHost, s));
  if (lpd) HIPCHECK(hipMemcpyAsync(lpd, dlpd, sizeof(T) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_LOO, 4);
  if (!(out.done & 1) || (grad && !(out.done & 2)))
    throw HipError{hipErrorLaunchFailure, "leave-one-out: the kernels did not run", __LINE__};
  bool finite = std::isfinite(out.lml);
  if (grad) for (int j = 0; j < p; ++j) finite = finite && std::isfinite(out.grad[j]);
  if (!finite) {
    if (loo) *loo = -std::numeric_limits<double>::infinity();
    if (grad) for (int j = 0; j < p; ++j) grad[j] = 0.0;
    return fail(HBEGP_NOT_PD, "the leave-one-out pseudo-likelihood is not finite");
  }
  if (loo) *loo = out.lml;
  if (grad) for (int j = 0; j < p; ++j) grad[j] = out.grad[j];
  return HBEGP_OK;
}

// ---- input warping (hbegp_problem_eval_xgrad / _eval_warped) ------------------------------------------------

// G = d lml / d X from what an evaluation left behind; reads only, its work arrays are borrowed for the call.  A result that is
// not finite is HBEGP_NOT_PD with zeros, as the evaluations handle it.
template <typename T>
static int xgrad_tail(const LooIn<T>& in, double* gx, const double* dlna, const double* dlnb, double* chain) {
  HIPCHECK(hipSetDevice(in.dev));
  const int n = in.n, d = in.d;
  const size_t nd = (size_t)n * d;
  hipStream_t s = in.s;
  CallScratch ws{in.dev, s, {}};
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t b_tk = 256, b_g = up(sizeof(double) * nd), b_part = up(sizeof(double) * xgrad_part_elems(n, d));
  const size_t b_ch = up(sizeof(double) * 2 * d);
  char* q = static_cast<char*>(ws.get(b_tk + b_g + b_part + b_ch));
  int* ticket = reinterpret_cast<int*>(q); q += b_tk;
  double* G = reinterpret_cast<double*>(q); q += b_g;
  double* part = reinterpret_cast<double*>(q); q += b_part;
  double* ch = reinterpret_cast<double*>(q);
  HIPCHECK(hipMemsetAsync(ticket, 0, b_tk, s));  // a recycled block holds its earlier owner's numbers
  launch_xgrad<T>(in.X, n, d, in.np, in.nu2, in.P, in.Kinv, in.alpha, part, G, ticket, s);
  if (chain) launch_warp_chain(G, dlna, dlnb, n, d, ch, s);
  CHECK_LAUNCHES();
  std::vector<double> gh;
  if (!gx) {  // looked at for NaN all the same
    gh.resize(nd);
    gx = gh.data();
  }
  HIPCHECK(hipMemcpyAsync(gx, G, sizeof(double) * nd, hipMemcpyDeviceToHost, s));
  if (chain) HIPCHECK(hipMemcpyAsync(chain, ch, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  bool finite = true;
  for (size_t e = 0; e < nd; ++e) finite = finite && std::isfinite(gx[e]);
  if (chain) for (int k = 0; k < 2 * d; ++k) finite = finite && std::isfinite(chain[k]);
  if (!finite) {
    std::fill(gx, gx + nd, 0.0);
    if (chain) std::fill(chain, chain + 2 * d, 0.0);
    return fail(HBEGP_NOT_PD, "the gradient with respect to the training inputs is not finite");
  }
  return HBEGP_OK;
}

template <typename T>
static int model_loo(hbegp_model* m, T* mean, T* var, T* lpd, double* loo, double* grad) {
  std::lock_guard<std::mutex> lock(m->mu);
  const LooIn<T> in{m->dev, m->stream, m->n, m->d, m->np, m->nu2, static_cast<const T*>(m->X), static_cast<const T*>(m->y),
                    static_cast<const T*>(m->alpha), static_cast<const T*>(m->Xinv), static_cast<const T*>(m->Kinv), m->dP};
  return loo_tail<T>(in, mean, var, lpd, loo, grad);
}

// ---- leave-group-out cross-validation (hbegp_model_lgo / hbegp_problem_eval_lgo / hbegp_fit_lgo) ---------

static int build_lgo_groups(const int* group, int n, LgoGroups* out) {
  LgoGroups& gr = *out;
  gr = LgoGroups{};
  gr.n = n;
  std::vector<int> id(n), size, label;
  if (group) {
    std::unordered_map<int, int> dense;
    dense.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
      auto it = dense.find(group[i]);
      if (it == dense.end()) {
        it = dense.emplace(group[i], (int)size.size()).first;
        size.push_back(0);
        label.push_back(group[i]);
      }
      id[i] = it->second;
      size[it->second]++;
    }
  } else {
    size.assign(n, 1);
    for (int i = 0; i < n; ++i) id[i] = i;
  }
  const int G = (int)size.size();
  for (int g = 0; g < G; ++g)
    if (size[g] > HBEGP_LGO_MAX_GROUP)
      return fail(HBEGP_EINVAL, "group %d holds %d rows: leave-group-out takes at most %d rows per group", label[g], size[g], HBEGP_LGO_MAX_GROUP);
  gr.G = G;
  std::vector<int> boff{0};
  for (int g = 0, held = 0; g < G; ++g) {  // bundles: consecutive groups, at most 64 rows together
    if (held + size[g] > 64) { boff.push_back(g); held = 0; }
    held += size[g];
    gr.smax = std::max(gr.smax, size[g]);
  }
  boff.push_back(G);
  gr.nb = (int)boff.size() - 1;
  gr.lists.assign((size_t)2 * n + 2 * (G + 1) + boff.size(), 0);
  int* member = gr.lists.data();
  int* gid = member + n;
  int* goff = gid + n;
  int* foff = goff + (G + 1);
  std::copy(boff.begin(), boff.end(), foff + (G + 1));
  for (int g = 0; g < G; ++g) {
    goff[g + 1] = goff[g] + size[g];
    foff[g + 1] = foff[g] + size[g] * size[g];
  }
  gr.f_elems = (size_t)foff[G];
  std::vector<int> fill(goff, goff + G);
  for (int i = 0; i < n; ++i) {  // rows ascending inside a group
    const int pos = fill[id[i]]++;
    member[pos] = i;
    gid[pos] = id[i];
  }
  return HBEGP_OK;
}

// The diagnostics of every group from L^-1 and alpha (one workgroup per group: the Gram matrix M_II, its factor, r_g, Sigma_g, lpd_g,
// F_g), and with `grad` the gradient of their sum: u = K^-1 a and Y[:, I] = K^-1[:, I] F_g in one pass over K^-1, then loo_tail's
// SYRK and weighted trace as they are.  Y and C are borrowed only with `grad`; everything borrowed goes back cleared.  lpd has G
// entries.  A pivot that is not positive in a group, or a result that is not finite, is HBEGP_NOT_PD: lgo = -inf, grad = 0.
template <typename T>
static int lgo_tail(const LooIn<T>& in, const LgoGroups& gr, const int* dlists, T* mean, T* var, T* lpd, double* lgo, double* grad) {
  HIPCHECK(hipSetDevice(in.dev));
  const int n = in.n, np = in.np, p = in.d + 2, G = gr.G;
  const size_t nn = (size_t)np * np;
  if (grad && 2.0 * (double)sizeof(T) * (double)np * np > 1e15)
    return fail(HBEGP_ENOMEM, "the leave-group-out gradient of %d rows needs %.3g bytes of device memory", n, 2.0 * sizeof(T) * (double)np * np);
  hipStream_t s = in.s;
  CallScratch ws{in.dev, s, {}};
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t b_vec = up(sizeof(T) * np), b_dvec = up(sizeof(double) * np), b_out = up(sizeof(EvalOut));
  const size_t b_lists = dlists ? 0 : up(gr.bytes()), b_F = up(sizeof(double) * gr.f_elems);
  const size_t b_gram = up(sizeof(double) * gr.f_elems * (size_t)lgo_gram_chunks(n, gr.smax));
  const size_t b_pu = grad ? up(sizeof(double) * (size_t)gr.nb * np) : 0;
  const size_t b_pg = grad ? up(sizeof(double) * gradtrace_part_elems(np, in.d)) : 0;
  char* q = static_cast<char*>(ws.get(b_out + 4 * b_vec + 2 * b_dvec + b_lists + b_F + b_gram + b_pu + b_pg));
  EvalOut* dout = reinterpret_cast<EvalOut*>(q); q += b_out;
  T* dmean = reinterpret_cast<T*>(q); q += b_vec;
  T* dvar = reinterpret_cast<T*>(q); q += b_vec;
  T* dlpd = reinterpret_cast<T*>(q); q += b_vec;  // G <= n entries
  T* du = reinterpret_cast<T*>(q); q += b_vec;
  double* avec = reinterpret_cast<double*>(q); q += b_dvec;
  double* share = reinterpret_cast<double*>(q); q += b_dvec;
  int* lists = reinterpret_cast<int*>(q); q += b_lists;
  double* F = reinterpret_cast<double*>(q); q += b_F;
  double* gram = reinterpret_cast<double*>(q); q += b_gram;
  double* pu = reinterpret_cast<double*>(q); q += b_pu;
  double* part_g = reinterpret_cast<double*>(q);
  HIPCHECK(hipMemsetAsync(dout, 0, sizeof(EvalOut), s));  // info = 0, done = 0 (a recycled block holds its earlier owner's numbers)
  HIPCHECK(hipMemsetAsync(avec, 0, sizeof(double) * np, s));  // the padding rows of a
  if (!dlists) {
    HIPCHECK(hipMemcpyAsync(lists, gr.lists.data(), gr.bytes(), hipMemcpyHostToDevice, s));
    dlists = lists;
  }
  const LgoLists L = gr.on_device(dlists);
  PhaseClock clk(t_phase[PH_LGO].on && grad, 5);
  clk.mark(s);
  launch_lgo_group<T>(in.Xinv, np, n, in.y, in.alpha, L, gr.f_elems, gram, dmean, dvar, dlpd, avec, F, share, dout, s);
  clk.mark(s);
  if (grad) {
    T* Y = static_cast<T*>(ws.get(sizeof(T) * nn));
    T* Cm = static_cast<T*>(ws.get(sizeof(T) * nn));
    if (np > n) HIPCHECK(hipMemsetAsync(Y, 0, sizeof(T) * nn, s));  // the padding columns (the kernel writes every row of the others)
    launch_lgo_uy<T>(in.Kinv, np, n, L, avec, F, Y, pu, du, &dout->info, s);
    clk.mark(s);
    {
      // C = Y Y^T (lower tiles), contraction over all columns of Y
      GemmLaunch g{};
      g.nops = 1;
      GemmOp& op = g.op[0];
      op.A = Y; op.B = Y; op.C = Cm;
      op.lda = op.ldb = op.ldc = np;
      op.mi = np / NB; op.nj = np / NB; op.c_lower = 1;
      op.k0 = 0; op.k1 = np / NB;
      gemm_adhoc<T>(g, &dout->info, s);
    }
    clk.mark(s);
    launch_loo_trace<T>(in.X, n, in.d, np, in.nu2, in.P, Cm, in.alpha, du, part_g, dout, s);
    clk.mark(s);
  }
  CHECK_LAUNCHES();
  EvalOut out;
  HIPCHECK(hipMemcpyAsync(&out, dout, sizeof(EvalOut), hipMemcpyDeviceToHost, s));
  if (mean) HIPCHECK(hipMemcpyAsync(mean, dmean, sizeof(T) * n, hipMemcpyDeviceToHost, s));
  if (var) HIPCHECK(hipMemcpyAsync(var, dvar, sizeof(T) * n, hipMemcpyDeviceToHost, s));
  if (lpd) HIPCHECK(hipMemcpyAsync(lpd, dlpd, sizeof(T) * G, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_LGO, 4);
  if (!(out.done & 1) || (grad && out.info == 0 && !(out.done & 2)))
    throw HipError{hipErrorLaunchFailure, "leave-group-out: the kernels did not run", __LINE__};
  bool finite = out.info == 0 && std::isfinite(out.lml);
  if (grad && finite) for (int j = 0; j < p; ++j) finite = finite && std::isfinite(out.grad[j]);
  if (!finite) {
    if (lgo) *lgo = -std::numeric_limits<double>::infinity();
    if (grad) for (int j = 0; j < p; ++j) grad[j] = 0.0;
    if (out.info != 0) return fail(HBEGP_NOT_PD, "leave-group-out: the group of row %d is not positive definite", out.info - 1);
    return fail(HBEGP_NOT_PD, "the leave-group-out predictive density is not finite");
  }
  if (lgo) *lgo = out.lml;
  if (grad) for (int j = 0; j < p; ++j) grad[j] = out.grad[j];
  return HBEGP_OK;
}

template <typename T>
static int model_lgo(hbegp_model* m, const int* group, T* mean, T* var, T* lpd, int* n_groups, double* lgo, double* grad) {
  LgoGroups gr;
  if (int rc = build_lgo_groups(group, m->n, &gr)) return rc;
  if (n_groups) *n_groups = gr.G;
  std::lock_guard<std::mutex> lock(m->mu);
  const LooIn<T> in{m->dev, m->stream, m->n, m->d, m->np, m->nu2, static_cast<const T*>(m->X), static_cast<const T*>(m->y),
                    static_cast<const T*>(m->alpha), static_cast<const T*>(m->Xinv), static_cast<const T*>(m->Kinv), m->dP};
  return lgo_tail<T>(in, gr, nullptr, mean, var, lpd, lgo, grad);
}

// ---- posterior sample paths (hbegp_paths_*) ------------------------------------------------------------
// The handle keeps, on the model's device: om^T [d][F] = omega0^T / ell, the phases [F] and the weights [S][F] in fp64, and
// V^T [S_p][n_p] (one path per row: the tile GEMMs' operand layout).  Its calls run on the model's stream under the model's
// mutex (they read the model's arrays and share its device), so a handle is safe from any number of threads.
struct hbegp_paths {
  hbegp_model* model = nullptr;  // retained
  int F = 0, S = 0, Sp = 0;
  bool is_f32 = false;
  double *omT = nullptr, *phase = nullptr, *Wf = nullptr;
  void* Vt = nullptr;
  // evaluation scratch (grow-only): points, chunk partial sums, outputs
  size_t cap_x = 0, cap_part = 0, cap_f = 0, cap_df = 0;
  void *Xs = nullptr, *part = nullptr, *f = nullptr, *df = nullptr;
  std::vector<std::pair<void*, size_t>> pooled;
  void* palloc(size_t bytes) {
    bool fresh = false;
    bytes = std::max<size_t>(16, bytes);
    void* q = g_pool.get(model->dev, bytes, &fresh);
    pooled.push_back({q, bytes});
    return q;
  }
  // Blocks go back to the pool cleared, as CallScratch's do: a NaN query row leaves NaN in the scratch, a later owner of the same
  // size (a fit's work matrix) must find zeros.  The caller has synchronised the stream or does so before the block is reused.
  void pfree(void* q) {
    for (size_t i = 0; i < pooled.size(); ++i)
      if (pooled[i].first == q) {
        (void)hipMemsetAsync(q, 0, pooled[i].second, model->stream);
        (void)hipStreamSynchronize(model->stream);
        g_pool.put(model->dev, q, pooled[i].second);
        pooled.erase(pooled.begin() + (long)i);
        return;
      }
  }
  void grow(void** q, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return;
    HIPCHECK(hipStreamSynchronize(model->stream));  // nothing of an earlier call still uses the smaller array
    if (*q) pfree(*q);
    *q = nullptr; *cap = 0;
    *q = palloc(bytes);
    *cap = bytes;
  }
  ~hbegp_paths() {
    if (!model) return;
    (void)hipSetDevice(model->dev);
    {
      std::lock_guard<std::mutex> lock(model->mu);
      for (auto& q : pooled) (void)hipMemsetAsync(q.first, 0, q.second, model->stream);
      (void)hipStreamSynchronize(model->stream);
      for (auto& q : pooled) g_pool.put(model->dev, q.first, q.second);
    }
    hbegp_model_release(model);
  }
};


template <typename T>
static int paths_create(hbegp_model* m, const T* omega0, const T* phase, const T* w, const T* eps, int F, int S, hbegp_paths** out) {
  std::unique_ptr<hbegp_paths> p(new hbegp_paths());
  hbegp_model_retain(m);
  p->model = m; p->F = F; p->S = S; p->Sp = round_up(S, NB); p->is_f32 = m->is_f32;
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  hipStream_t s = m->stream;
  const int n = m->n, d = m->d, np = m->np, Sp = p->Sp;
  p->omT = static_cast<double*>(p->palloc(sizeof(double) * (size_t)F * d));
  p->phase = static_cast<double*>(p->palloc(sizeof(double) * (size_t)F));
  p->Wf = static_cast<double*>(p->palloc(sizeof(double) * (size_t)S * F));
  p->Vt = p->palloc(sizeof(T) * (size_t)Sp * np);
  // the weights and phases go up as fp64 (every feature sum is fp64 for both element types)
  std::vector<double> hw((size_t)S * F + F);
  for (size_t i = 0; i < (size_t)S * F; ++i) hw[i] = (double)w[i];
  for (int j = 0; j < F; ++j) hw[(size_t)S * F + j] = (double)phase[j];
  CallScratch ws{m->dev, s, {}};
  T* om0 = static_cast<T*>(ws.get(sizeof(T) * (size_t)F * d));
  T* deps = eps ? static_cast<T*>(ws.get(sizeof(T) * (size_t)S * n)) : nullptr;
  double* part = static_cast<double*>(ws.get(sizeof(double) * (size_t)paths_project_chunks(F, n, S) * S * n));
  T* Rt = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * np));
  T* T1 = static_cast<T*>(ws.get(sizeof(T) * (size_t)Sp * np));
  PhaseClock clk(t_phase[PH_PATHS].on, 4);
  clk.mark(s);
  HIPCHECK(hipMemcpyAsync(p->Wf, hw.data(), sizeof(double) * (size_t)S * F, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(p->phase, hw.data() + (size_t)S * F, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(om0, omega0, sizeof(T) * (size_t)F * d, hipMemcpyHostToDevice, s));
  if (eps) HIPCHECK(hipMemcpyAsync(deps, eps, sizeof(T) * (size_t)S * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(m->dOut, 0, sizeof(EvalOut), s));
  launch_paths_scale_omega<T>(om0, F, d, m->dP, p->omT, s);
  clk.mark(s);
  launch_paths_project<T>(static_cast<T*>(m->X), n, d, np, p->omT, p->phase, F, p->Wf, S, Sp, static_cast<T*>(m->y), deps, static_cast<const T*>(m->rv), m->dP, part, Rt, s);
  clk.mark(s);
  {
    // v = L^-T (L^-1 r) for all paths, one path per row: T1 = R^T X^T (X = L^-1 lower: k <= j, as Q = Kstar X^T), then
    // V^T = T1 X (k >= j).  Never through the stored K^-1 (section 10).
    GemmLaunch g = gemm_lower_b(Rt, np, m->Xinv, np, T1, np, Sp / NB, np / NB, np / NB);
    gemm_adhoc<T>(g, &m->dOut->info, s);
    GemmLaunch g2 = gemm_lower_b(T1, np, m->Xinv, np, p->Vt, np, Sp / NB, np / NB, np / NB);
    g2.op[0].b_kmajor = 1; g2.op[0].klim = 2;
    gemm_adhoc<T>(g2, &m->dOut->info, s);
  }
  clk.mark(s);
  CHECK_LAUNCHES();
  HIPCHECK(hipStreamSynchronize(s));
  clk.store(PH_PATHS, 3);
  *out = p.release();
  return HBEGP_OK;
}

// the points go through the kernels in blocks: at most PATHS_EVAL_ROWS (path, point) pairs and PATHS_EVAL_PART bytes of partial sums
constexpr size_t PATHS_EVAL_ROWS = 262144;
constexpr size_t PATHS_EVAL_PART = (size_t)256 << 20;
// bytes of partial sums per point of a call, and the points per block of a call of cnt points (host only: hbegp_debug_paths_eval_blocks)
static size_t paths_eval_per_point(int n, int d, int F, int S) { return sizeof(double) * (size_t)paths_eval_chunks(n, F) * S * (d + 1); }
static int paths_eval_block(int n, int d, int F, int S, int cnt) {
  return (int)std::max<size_t>(1, std::min<size_t>({(size_t)cnt, PATHS_EVAL_ROWS / (size_t)S, PATHS_EVAL_PART / paths_eval_per_point(n, d, F, S)}));
}

// the caller holds the model's mutex
template <typename T>
static void paths_eval_locked(hbegp_paths* p, const T* Xs, int cnt, int per_path, T* f, T* df) {
  hbegp_model* m = p->model;
  hipStream_t s = m->stream;
  const int d = m->d, S = p->S;
  const size_t per_point = paths_eval_per_point(m->n, d, p->F, S);
  const int mb = paths_eval_block(m->n, d, p->F, S, cnt);
  p->grow(&p->Xs, &p->cap_x, sizeof(T) * (size_t)(per_path ? S : 1) * mb * d);
  p->grow(&p->part, &p->cap_part, per_point * mb);
  p->grow(&p->f, &p->cap_f, sizeof(T) * (size_t)S * mb);
  if (df) p->grow(&p->df, &p->cap_df, sizeof(T) * (size_t)S * mb * d);
  for (int p0 = 0; p0 < cnt; p0 += mb) {
    const int c = std::min(mb, cnt - p0);
    if (per_path)
      HIPCHECK(hipMemcpy2DAsync(p->Xs, sizeof(T) * (size_t)c * d, Xs + (size_t)p0 * d, sizeof(T) * (size_t)cnt * d, sizeof(T) * (size_t)c * d, S,
                                hipMemcpyHostToDevice, s));
    else
      HIPCHECK(hipMemcpyAsync(p->Xs, Xs + (size_t)p0 * d, sizeof(T) * (size_t)c * d, hipMemcpyHostToDevice, s));
    launch_paths_eval<T>(static_cast<T*>(p->Xs), c, per_path, S, static_cast<T*>(m->X), m->n, d, m->np, m->nu2, m->dP, static_cast<T*>(p->Vt),
                         p->omT, p->phase, p->Wf, p->F, df ? 1 : 0, static_cast<double*>(p->part), static_cast<T*>(p->f),
                         static_cast<T*>(p->df), s);
    CHECK_LAUNCHES();
    HIPCHECK(hipMemcpy2DAsync(f + p0, sizeof(T) * (size_t)cnt, p->f, sizeof(T) * (size_t)c, sizeof(T) * (size_t)c, S, hipMemcpyDeviceToHost, s));
    if (df)
      HIPCHECK(hipMemcpy2DAsync(df + (size_t)p0 * d, sizeof(T) * (size_t)cnt * d, p->df, sizeof(T) * (size_t)c * d, sizeof(T) * (size_t)c * d, S,
                                hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));  // the next block reuses the scratch; the caller's arrays are pageable
  }
}

template <typename T>
static int paths_eval(hbegp_paths* p, const T* Xs, int cnt, int per_path, T* f, T* df) {
  std::lock_guard<std::mutex> lock(p->model->mu);
  HIPCHECK(hipSetDevice(p->model->dev));
  paths_eval_locked<T>(p, Xs, cnt, per_path, f, df);
  return HBEGP_OK;
}

// S R bounded L-BFGS descents, R per path, in lockstep (lockstep.hpp; run sp R + r is run r of path sp): every round evaluates the
// points of the unfinished runs with ONE per-path evaluation ([S][mr] points, mr the largest number of unfinished runs of any path;
// a path with fewer repeats its last point, one with none its best point so far).  Each path returns the best point any of its runs
// evaluated: the earliest evaluation on ties, rounds in order and a round's runs in order (a value or a gradient component that is
// not finite is a failed evaluation; a path without a finite value returns its first start and +inf).
template <typename T>
static int paths_minimize(hbegp_paths* p, const T* starts, int R, const double* lo, const double* hi, int maxeval, T* x_best, double* f_best,
                          int* n_evals) {
  hbegp_model* m = p->model;
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const int d = m->d, S = p->S;
  const size_t NR = (size_t)S * R;
  std::vector<T> x_run(NR * d), xs, fv, dfv;
  std::vector<double> f_run(NR);
  std::vector<int> nev(NR), slot(NR), na(S);
  for (int sp = 0; sp < S; ++sp) {
    f_best[sp] = std::numeric_limits<double>::infinity();
    for (int k = 0; k < d; ++k) x_best[(size_t)sp * d + k] = starts[(size_t)sp * R * d + k];
  }
  // the driver keeps every run's best; a path's best follows them after every round, in run order
  auto fold = [&]() {
    for (size_t r = 0; r < NR; ++r)
      if (f_run[r] < f_best[r / R]) {
        f_best[r / R] = f_run[r];
        for (int k = 0; k < d; ++k) x_best[(r / R) * d + k] = x_run[r * d + k];
      }
  };
  auto eval = [&](const T* pts, const int* runs, int cnt, double* val, double* grad, char* ok) {
    fold();
    std::fill(na.begin(), na.end(), 0);
    for (int i = 0; i < cnt; ++i) slot[i] = na[runs[i] / R]++;
    const int mr = *std::max_element(na.begin(), na.end());
    xs.assign((size_t)S * mr * d, T(0));
    fv.resize((size_t)S * mr);
    dfv.resize((size_t)S * mr * d);
    for (int i = 0; i < cnt; ++i) std::copy(pts + (size_t)i * d, pts + (size_t)(i + 1) * d, xs.begin() + ((size_t)(runs[i] / R) * mr + slot[i]) * d);
    for (int sp = 0; sp < S; ++sp) {
      T* row = xs.data() + (size_t)sp * mr * d;
      for (int i = na[sp]; i < mr; ++i) {
        const T* src = i > 0 ? row + (size_t)(i - 1) * d : x_best + (size_t)sp * d;
        for (int k = 0; k < d; ++k) row[(size_t)i * d + k] = src[k];
      }
    }
    paths_eval_locked<T>(p, xs.data(), mr, 1, fv.data(), dfv.data());
    for (int i = 0; i < cnt; ++i) {
      const size_t at = (size_t)(runs[i] / R) * mr + slot[i];
      val[i] = (double)fv[at];
      ok[i] = std::isfinite(val[i]);
      for (int k = 0; k < d; ++k) {
        grad[(size_t)i * d + k] = (double)dfv[at * d + k];
        ok[i] = ok[i] && std::isfinite(grad[(size_t)i * d + k]);
      }
    }
    return (int)HBEGP_OK;
  };
  const int rc = lockstep_optimize<T, LbfgsState>(starts, (int)NR, d, lo, hi, lockstep_options(maxeval, false), eval, x_run.data(), f_run.data(),
                                                  nev.data());
  if (rc != HBEGP_OK) return rc;
  fold();
  if (n_evals)
    for (int sp = 0; sp < S; ++sp) n_evals[sp] = std::accumulate(nev.begin() + (size_t)sp * R, nev.begin() + (size_t)(sp + 1) * R, 0);
  return HBEGP_OK;
}

// argument checks of the sample-path entry points: everything is refused before any device call
template <typename T>
static int check_paths_create(hbegp_model* model, const T* omega0, const T* phase, const T* w, int F, int S, hbegp_paths** paths) {
  if (F < 1 || F > HBEGP_PATHS_MAX_FEATURES) return fail(HBEGP_EINVAL, "F must be in [1, %d] (got %d)", HBEGP_PATHS_MAX_FEATURES, F);
  if (S < 1 || S > HBEGP_PATHS_MAX_PATHS) return fail(HBEGP_EINVAL, "S must be in [1, %d] (got %d)", HBEGP_PATHS_MAX_PATHS, S);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (!omega0 || !phase || !w || !paths) return fail(HBEGP_EINVAL, "omega0/phase/w/paths is NULL");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
template <typename T>
static int check_paths_eval(hbegp_paths* paths, const T* Xs, int m, int per_path, T* f) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (per_path != 0 && per_path != 1) return fail(HBEGP_EINVAL, "per_path must be 0 or 1 (got %d)", per_path);
  if (!paths) return fail(HBEGP_EINVAL, "NULL paths handle");
  if (paths->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "paths handle holds %s data", paths->is_f32 ? "f32" : "f64");
  if (m > 0 && (!Xs || !f)) return fail(HBEGP_EINVAL, "Xs/f is NULL");
  return HBEGP_OK;
}
template <typename T>
static int check_paths_minimize(hbegp_paths* paths, const T* starts, int R, const double* lo, const double* hi, int maxeval, T* x_best,
                                double* f_best) {
  if (R < 1) return fail(HBEGP_EINVAL, "R must be >= 1 (got %d)", R);
  if (maxeval < 1) return fail(HBEGP_EINVAL, "maxeval must be >= 1 (got %d)", maxeval);
  if (!paths) return fail(HBEGP_EINVAL, "NULL paths handle");
  if (!starts || !lo || !hi || !x_best || !f_best) return fail(HBEGP_EINVAL, "starts/lo/hi/x_best/f_best is NULL");
  if (paths->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "paths handle holds %s data", paths->is_f32 ? "f32" : "f64");
  const int d = paths->model->d;
  if (d > LBFGS_MAXN) return fail(HBEGP_EINVAL, "d = %d exceeds the optimiser's %d variables", d, LBFGS_MAXN);
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return fail(HBEGP_EINVAL, "lo[%d] > hi[%d] (%g > %g)", k, k, lo[k], hi[k]);
  for (size_t r = 0; r < (size_t)paths->S * R; ++r)
    for (int k = 0; k < d; ++k) {
      const double v = (double)starts[r * d + k];
      if (!(v >= lo[k] && v <= hi[k])) return fail(HBEGP_EINVAL, "start %zu lies outside the box (feature %d: %g)", r, k, v);
    }
  return HBEGP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fit (fit.rs:71-176 + gradmin.rs:7-60)
// The caller's options struct may be older (shorter) or newer (longer) than this library's: copy what both know, the rest
// stays zero / NULL.  Nothing is read or written beyond min(struct_size, sizeof).
// What the calling thread's most recent fit did (hbegp_last_fit_stats): evaluations, failed ones, and the line-search trials
// that ended after their first phase (lml only: no K^-1, no gradient).
// Per optimiser run (the first HBEGP_STATS_MAX_RUNS of them): when its last evaluation was over, in ms since the fit was called,
// and what it launched -- whole evaluations, first phases that stayed alone, first phases followed by a second one, and how many of
// its evaluations ran with a lead / a lag share of the compute units (slot_share.hpp).
struct RunStats { double end_ms = 0; int fused = 0, lml_only = 0, phase2 = 0, lead = 0, lag = 0; };
struct LastFitStats {
  int n_evals = 0, n_not_pd = 0, n_lml_only = 0, n_runs = 0;
  RunStats run[HBEGP_STATS_MAX_RUNS];
};
static thread_local LastFitStats g_last_fit_stats;

static int read_fit_options(const hbegp_fit_options* in, hbegp_fit_options* out) {
  *out = hbegp_fit_options{};
  out->struct_size = sizeof(hbegp_fit_options);
  if (!in) return HBEGP_OK;
  if (in->struct_size < offsetof(hbegp_fit_options, maxeval) + sizeof(int) || in->struct_size > ((size_t)1 << 16))
    return fail(HBEGP_EINVAL, "hbegp_fit_options.struct_size = %zu: set it to sizeof(hbegp_fit_options) (HBEGP_FIT_OPTIONS_INIT)",
                in->struct_size);
  memcpy(out, in, std::min(in->struct_size, sizeof(*out)));
  return HBEGP_OK;
}

template <typename T>
static int do_extend(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model_out);

// loo: the objective is the leave-one-out log pseudo-likelihood (hbegp_fit_loo_*) -- every evaluation is the slot's normal one
// without the lml gradient plus the leave-one-out tail on its results, always under the host-driven optimiser, and the model
// is `extend` at the captured theta.  Nothing else differs; FIT_LML is the fit as it always was.  FIT_LGO (hbegp_fit_lgo_*) is the
// same with the leave-group-out tail over `groups`, whose lists are uploaded once per device for the whole fit.
enum FitObjective { FIT_LML = 0, FIT_LOO = 1, FIT_LGO = 2 };
// gr.lists on every device of a fit, in pool blocks that go back cleared
struct LgoDeviceLists {
  size_t bytes = 0;
  std::vector<std::pair<int, void*>> held;  // (device id, block), one per device of the context in its order
  void upload(const std::vector<int>& devs, const LgoGroups& gr) {
    bytes = std::max<size_t>(16, gr.bytes());
    for (int dev : devs) {
      HIPCHECK(hipSetDevice(dev));
      bool fresh = false;
      void* p = g_pool.get(dev, bytes, &fresh);
      held.push_back({dev, p});
      HIPCHECK(hipMemcpy(p, gr.lists.data(), gr.bytes(), hipMemcpyHostToDevice));
    }
  }
  const int* on(size_t di) const { return static_cast<const int*>(held[di].second); }
  ~LgoDeviceLists() {
    for (auto& h : held) {
      (void)hipSetDevice(h.first);
      (void)hipMemset(h.second, 0, bytes);
      (void)hipDeviceSynchronize();
      g_pool.put(h.first, h.second, bytes);
    }
  }
};
template <typename T>
static int do_fit(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta0,
                  const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt_in,
                  double* theta_best, double* lml_best, hbegp_model** model_out, int objective = FIT_LML,
                  const LgoGroups* groups = nullptr) {
  const bool loo = objective != FIT_LML;  // a cross-validation objective: the slot's evaluation plus a tail
  hbegp_fit_options opt{};
  g_last_fit_stats = LastFitStats{};  // a fit that fails leaves zeros, not the previous fit's numbers
  if (int e = read_fit_options(opt_in, &opt)) return e;
  if (opt.maxeval <= 0) opt.maxeval = 150;
  const int p = d + 2;
  const int nruns = 1 + std::max(0, n_restarts);
  const int ndev = (int)ctx->devs.size();
  const int max_conc = std::max(1, env_int("HBEGP_MAX_CONCURRENT", 3));  // measured (C3, 8 runs): 1: 3.29, 2: 2.36, 3: 2.09, 4: 2.33, 8: 2.10 ms per evaluation
  // workers: device di gets min(runs on that device, max_conc) slots; run r -> device r % ndev
  std::vector<int> runs_on(ndev, 0);
  for (int r = 0; r < nruns; ++r) runs_on[r % ndev]++;
  int n_slots = 1;
  for (int di = 0; di < ndev; ++di) n_slots = std::max(n_slots, std::min(runs_on[di], max_conc));
  // Up to 128 rows an optimiser run is ONE persistent launch on ONE compute unit (small_fit_kernel: evaluation + L-BFGS step +
  // capture on the device): every run gets a slot of its own and all of them run side by side
  constexpr int SMALL_FIT_MAX_RUNS = 64;  // per device
  bool small_fit = !loo && round_up(n, NB) == NB && d <= SMALL_EVAL_MAXD && env_int("HBEGP_SMALL", 1) != 0 && env_int("HBEGP_SMALL_FIT", 1) != 0;
  for (int di = 0; di < ndev; ++di) small_fit = small_fit && runs_on[di] <= SMALL_FIT_MAX_RUNS;
  if (small_fit)
    for (int di = 0; di < ndev; ++di) n_slots = std::max(n_slots, runs_on[di]);
  static const int timing = env_int("HBEGP_TIMING", 0);
  const auto tf0 = std::chrono::steady_clock::now();
  auto since_start_ms = [tf0] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count(); };
  std::vector<RunStats> run_stats(nruns);  // every run is written by the one thread that drives it
  struct FitsInFlight {  // counted from here on, not from the first evaluation: a second fit sees this one while it still sets up
    const hbegp_ctx* c;
    explicit FitsInFlight(const hbegp_ctx* cc) : c(cc) { for (int dev : c->devs) if (dev < MAX_DEVS) g_dev_fits[dev].fetch_add(1); }
    ~FitsInFlight() { for (int dev : c->devs) if (dev < MAX_DEVS) g_dev_fits[dev].fetch_sub(1); }
  } fits_in_flight(ctx);
  // like_fit: the evaluation path (launches / task queue) is a function of n alone, also for a fit with one slot per device
  // (n_restarts = 0, or no more runs than devices): `extend` at the fitted theta then repeats the fit's own evaluation bit for bit
  SmallArrival arrival;  // other threads' small fits wait (briefly) for this one's runs before they launch: SmallBatcher
  if (small_fit) arrival.announce();
  // The host-side phases of a small fit (set-up; model + release: ~35 runtime calls together) run one thread at a time: sixteen
  // native threads that enter them at the same instant queue on the runtime's locks for 2-3 ms each, one after the other they take
  // 0.1-0.2 ms (measured, n = 128, fits/s at 4 / 8 / 16 native threads: 312 / 507 / 865 -> 351 / 658 / 1,157; Python threads, which
  // the interpreter lock staggers already: 1,198 -> 1,104 at 16).  Only while at most HBEGP_SMALL_HOST_SERIAL (16; 0 = never) threads
  // are inside small fits: beyond that the turns themselves are the queue (24 threads: 1,031 without / 862 with; 32 threads on 16
  // cores: 744 / 238), and a bounded wait for the turn (1-10 ms) keeps none of the gain (16 threads: 740-770).
  static const int host_serial_max = env_int("HBEGP_SMALL_HOST_SERIAL", 16);
  struct SmallActive {
    bool on = false;
    int enter() { on = true; return g_small_active.fetch_add(1) + 1; }
    ~SmallActive() { if (on) g_small_active.fetch_sub(1); }
  } small_active;
  const bool host_serial = small_fit && small_active.enter() <= host_serial_max;
  std::unique_lock<std::mutex> host_lk(g_small_host_mu, std::defer_lock);
  if (host_serial) host_lk.lock();
  const auto th0 = std::chrono::steady_clock::now();  // (HBEGP_TIMING: how long the turns are)
  double held_ms = 0;
  LgoDeviceLists lgo_lists;  // (declared before the problem: its slots are released first)
  if (objective == FIT_LGO) lgo_lists.upload(ctx->devs, *groups);
  Problem<T> prob(ctx, X, y, n, d, nu, n_slots, false, true, !loo, rv);
  const auto tf1 = std::chrono::steady_clock::now();
  if (!(small_fit && prob.small_)) arrival.arrived();
  if (!(small_fit && prob.small_) && host_lk.owns_lock()) host_lk.unlock();

  std::vector<double> lnlo(p), lnhi(p);
  for (int i = 0; i < p; ++i) {
    lnlo[i] = std::log(lo[i]);
    lnhi[i] = std::log(hi[i]);
  }
  std::mutex trace_mu;
  int trace_n = 0;
  std::atomic<int> n_evals{0}, n_not_pd{0}, n_lml_only{0};
  // lazy evaluation of line-search trials (Problem::lazy_: HBEGP_LAZY_GRAD, published evaluations, not the single-launch path).  A
  // trace that records gradients reads every evaluation's gradient: such a fit evaluates every trial whole.
  const bool lazy = prob.lazy_ && !loo && !(opt.trace_cap > 0 && opt.trace_grad);
  std::string err;
  std::mutex err_mu;

  if (small_fit && prob.small_) {
    struct RunWs {
      int di = 0, si = 0, run = 0;
      LbfgsState* st = nullptr;
      SmallFitResult* res = nullptr;
      double *x0 = nullptr, *tr_theta = nullptr, *tr_lml = nullptr, *tr_grad = nullptr;
    };
    const int cap = opt.trace_cap > 0 ? opt.maxeval : 0;  // per run; the merged trace is cut at opt.trace_cap below
    std::vector<RunWs> ws(nruns);
    // per run, in pinned memory: the result and the word the kernel sets when the run is over (SmallFit::hres / hdone)
    struct alignas(64) HostRun {
      SmallFitResult res;
      unsigned long long done;
    };
    const size_t hruns_bytes = (sizeof(HostRun) * (size_t)nruns + 4095) / 4096 * 4096;
    HostRun* hruns = static_cast<HostRun*>(g_host_pool.get(hruns_bytes));
    std::vector<std::shared_ptr<SmallBatch>> batches(ndev);
    bool runs_over = false;
    auto free_all = [&]() {  // (the trace arrays belong to the problem's pooled allocations, released with it)
      for (auto& b : batches) small_batch_leave(b, runs_over);
      batches.clear();
      g_host_pool.put(hruns, hruns_bytes);
    };
    try {
      std::vector<int> next_slot(ndev, 0);
      // the runs of a device are the workgroups of ONE launch on the device's first slot stream (one stream per fit and device:
      // fits side by side on one GPU then do not queue behind each other's persistent kernels, see small_fit_kernel)
      std::vector<std::vector<SmallFit>> fits_on(ndev);
      std::vector<double*> boxes_dev(ndev, nullptr);
      std::vector<std::vector<double>> boxes_host(ndev);  // the source of an asynchronous copy: alive until the stream has been waited for below
      for (int r = 0; r < nruns; ++r) {
        RunWs& w = ws[r];
        w.di = r % ndev; w.si = next_slot[w.di]++; w.run = r;
        HIPCHECK(hipSetDevice(ctx->devs[w.di]));
        Slot<T>& s = prob.slots[w.di][w.si];
        hipStream_t st = prob.slots[w.di][0].stream;
        // the run's workspace: the slot's W1 (the kernel matrix never leaves the LDS on this path, so the buffer is free) --
        // a hipMalloc / hipFree pair per array cost more than the run's arithmetic
        static_assert(sizeof(LbfgsState) + sizeof(SmallFitResult) + 3 * MAXP * sizeof(double) + 64 <= (size_t)NB * NB * sizeof(float),
                      "the run's workspace fits the slot's W1");
        char* base = reinterpret_cast<char*>(s.W1);
        w.st = reinterpret_cast<LbfgsState*>(base);
        w.res = reinterpret_cast<SmallFitResult*>(base + (sizeof(LbfgsState) + 15) / 16 * 16);
        // start point and box of every run of a device: one array, one copy (a copy per run was a runtime call per run inside the turn)
        if (!boxes_dev[w.di]) {
          boxes_dev[w.di] = prob.template palloc<double>(s.dev, (size_t)runs_on[w.di] * 3 * p);
          boxes_host[w.di].assign((size_t)runs_on[w.di] * 3 * p, 0.0);
        }
        w.x0 = boxes_dev[w.di] + (size_t)w.si * 3 * p;
        if (cap > 0) {
          w.tr_theta = prob.template palloc<double>(s.dev, (size_t)cap * p);
          w.tr_lml = prob.template palloc<double>(s.dev, cap);
          w.tr_grad = prob.template palloc<double>(s.dev, (size_t)cap * p);
        }
        const double* start = r == 0 ? theta0 : starts + (size_t)(r - 1) * p;
        double* box = boxes_host[w.di].data() + (size_t)w.si * 3 * p;  // start point, lower and upper bounds
        memcpy(box, start, sizeof(double) * p);
        memcpy(box + p, lo, sizeof(double) * p);
        memcpy(box + 2 * p, hi, sizeof(double) * p);
        SmallFit f{};
        f.ev.X = prob.Xd[w.di]; f.ev.y = prob.yd[w.di]; f.rv = prob.rvd[w.di]; f.ev.n = n; f.ev.d = d; f.ev.P = s.dP;
        f.ev.W2 = s.W2; f.ev.ldiag = s.ldiag; f.ev.out = s.dOut; f.ev.hout = s.dOut;
        f.Kinv[0] = s.Kinv[0]; f.Kinv[1] = s.Kinv[1]; f.alpha[0] = s.alpha[0]; f.alpha[1] = s.alpha[1];
        // L^-1 and diag(L) ping-pong too: the captured evaluation's factor survives the run, the model takes it as it is (no
        // factorisation at the captured theta behind the fit: one small launch and a wait less inside the model's turn)
        if (!s.Xalt) {
          s.Xalt = prob.template palloc<T>(s.dev, (size_t)NB * NB);
          s.ldalt = prob.template palloc<T>(s.dev, NB);
          HIPCHECK(hipMemsetAsync(s.Xalt, 0, sizeof(T) * NB * NB, st));  // the strict upper triangle must be zero, like W2's
        }
        f.Xinv[0] = s.W2; f.Xinv[1] = s.Xalt; f.ldiag[0] = s.ldiag; f.ldiag[1] = s.ldalt;
        s.x_captured = true;
        f.st = w.st; f.x0 = w.x0; f.lo = w.x0 + p; f.hi = w.x0 + 2 * p;
        LbfgsOptions lo_opt;
        f.maxeval = opt.maxeval; f.memory = opt.lbfgs_memory > 0 ? opt.lbfgs_memory : lo_opt.memory; f.fixed_work = opt.fixed_work != 0;
        f.pgtol = lo_opt.pgtol; f.ftol = lo_opt.ftol;
        f.res = w.res; f.trace_theta = w.tr_theta; f.trace_lml = w.tr_lml; f.trace_grad = w.tr_grad; f.trace_cap = cap;
        hruns[r].done = 0;
        f.hres = &hruns[r].res; f.hdone = &hruns[r].done;
        fits_on[w.di].push_back(f);
      }
      for (int di = 0; di < ndev; ++di) {
        if (fits_on[di].empty()) continue;
        HIPCHECK(hipSetDevice(ctx->devs[di]));
        HIPCHECK(hipMemcpyAsync(boxes_dev[di], boxes_host[di].data(), sizeof(double) * boxes_host[di].size(), hipMemcpyHostToDevice, prob.slots[di][0].stream));
        // the grid runs on the batch's stream: what this fit queued on its own (features, observations, start points) is there first
        HIPCHECK(hipStreamSynchronize(prob.slots[di][0].stream));
      }
      held_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
      if (host_lk.owns_lock()) host_lk.unlock();
      for (int di = 0; di < ndev; ++di) {
        if (fits_on[di].empty()) continue;
        HIPCHECK(hipSetDevice(ctx->devs[di]));
        batches[di] = small_batch_submit<T>(ctx->devs[di], prob.nu2, fits_on[di], arrival);
      }
      // every run's word, in run order.  The stream is asked now and then: a grid that is over without the word (a fault) must not
      // leave this thread spinning.
      auto wait_run = [&](int r, int di) {
        using namespace std::chrono;
        const volatile unsigned long long* q = &hruns[r].done;
        auto last_query = steady_clock::now();
        for (unsigned it = 1;; ++it) {
          if (*q == 1ull) break;
          if (it < 256) {
            __builtin_ia32_pause();
          } else {
            std::this_thread::sleep_for(microseconds(40));
            if (steady_clock::now() - last_query > milliseconds(20)) {
              last_query = steady_clock::now();
              const hipError_t e = hipStreamQuery(batches[di]->stream);
              if (e == hipSuccess) {
                if (*q == 1ull) break;
                throw HipError{hipErrorLaunchFailure, "small fit: the launch is over and a run never reported", __LINE__};
              }
              if (e != hipErrorNotReady) throw HipError{e, "hipStreamQuery (small-fit launch)", __LINE__};
            }
          }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
      };
      for (int r = 0; r < nruns; ++r) {
        wait_run(r, ws[r].di);
        run_stats[r].end_ms = since_start_ms();  // (when the host saw the run's word: the runs are waited for in run order)
        run_stats[r].fused = hruns[r].res.n_evals;
      }
      runs_over = true;
      int total_evals = 0, total_not_pd = 0, trace_n = 0;
      for (int r = 0; r < nruns; ++r) {
        RunWs& w = ws[r];
        HIPCHECK(hipSetDevice(ctx->devs[w.di]));
        Slot<T>& s = prob.slots[w.di][w.si];
        hipStream_t st = prob.slots[w.di][0].stream;
        const SmallFitResult hr = hruns[r].res;
        total_evals += hr.n_evals;
        total_not_pd += hr.n_not_pd;
        s.best_idx = hr.best_idx;
        s.best_lml = hr.best_lml;
        s.best_run = r;
        s.best_eval = hr.best_eval;
        s.best_theta.assign(hr.best_theta, hr.best_theta + p);
        s.best_params.assign(hr.best_params, hr.best_params + p);
        s.last_target = hr.best_idx < 0 ? 0 : hr.best_idx;
        if (cap > 0 && trace_n < opt.trace_cap) {  // the trace, run by run
          const int take = std::min(std::min(hr.n_evals, cap), opt.trace_cap - trace_n);
          if (opt.trace_theta) HIPCHECK(hipMemcpyAsync(opt.trace_theta + (size_t)trace_n * p, w.tr_theta, sizeof(double) * (size_t)take * p, hipMemcpyDeviceToHost, st));
          if (opt.trace_lml) HIPCHECK(hipMemcpyAsync(opt.trace_lml + trace_n, w.tr_lml, sizeof(double) * take, hipMemcpyDeviceToHost, st));
          if (opt.trace_grad) HIPCHECK(hipMemcpyAsync(opt.trace_grad + (size_t)trace_n * p, w.tr_grad, sizeof(double) * (size_t)take * p, hipMemcpyDeviceToHost, st));
          HIPCHECK(hipStreamSynchronize(st));
          if (opt.trace_run) for (int e = 0; e < take; ++e) opt.trace_run[trace_n + e] = r;
          trace_n += take;
        }
      }
      if (opt.trace_count) *opt.trace_count = trace_n;
      if (opt.n_evals) *opt.n_evals = total_evals;
      if (opt.n_not_pd) *opt.n_not_pd = total_not_pd;
      g_last_fit_stats.n_evals = total_evals;
      g_last_fit_stats.n_not_pd = total_not_pd;
      g_last_fit_stats.n_lml_only = 0;  // the persistent kernel evaluates every point whole
      n_evals.store(total_evals);
    } catch (...) {
      for (int di = 0; di < ndev && di < (int)prob.slots.size(); ++di) {  // let the launched kernels finish before their workspaces go
        if (prob.slots[di].empty()) continue;
        (void)hipSetDevice(ctx->devs[di]);
        (void)hipStreamSynchronize(prob.slots[di][0].stream);
      }
      free_all();
      throw;
    }
    free_all();
  } else {
  // how many slots of each device are inside an optimiser run: the task-queue launches are sized for that (Problem::DagVariant)
  if (prob.busy_slots_)
    for (int di = 0; di < ndev; ++di) prob.busy_slots_[di].store(std::min(runs_on[di], max_conc));
  // unequal shares (slot_share.hpp) only on devices where every slot drives ONE run: a slot that takes several runs in turn (8 runs
  // over 3 slots) has no single progress count to compare
  if (prob.dag_nshare_ > 0) {
    prob.slot_maxeval_ = opt.maxeval;
    for (int di = 0; di < ndev; ++di) prob.balance_dev_[di] = runs_on[di] <= max_conc && runs_on[di] == prob.n_slots;
  }
  auto worker = [&](int di, int si) {
    struct Leave {
      std::atomic<int>* busy;
      std::atomic<int>* dev_busy;
      ~Leave() {
        if (busy) busy->fetch_sub(1);
        if (dev_busy) dev_busy->fetch_sub(1);
      }
    } leave{prob.busy_slots_ ? &prob.busy_slots_[di] : nullptr, ctx->devs[di] < MAX_DEVS ? &g_dev_busy[ctx->devs[di]] : nullptr};
    if (leave.dev_busy) leave.dev_busy->fetch_add(1);
    try {
      HIPCHECK(hipSetDevice(ctx->devs[di]));
      Slot<T>& s = prob.slots[di][si];
      const int nslots_here = std::min(runs_on[di], max_conc);
      // runs assigned to this device: r = di, di+ndev, ...; this worker takes every nslots_here-th of them
      int local = 0;
      for (int r = di; r < nruns; r += ndev, ++local) {
        if (local % nslots_here != si) continue;
        std::vector<double> x(p);
        if (r == 0) for (int i = 0; i < p; ++i) x[i] = theta0[i];
        else for (int i = 0; i < p; ++i) x[i] = starts[(size_t)(r - 1) * p + i];
        int eval_idx = 0;
        RunStats& rs = run_stats[r];
        std::atomic<int>* progress = prob.dag_nshare_ > 0 ? &prob.slot_done_[(size_t)di * prob.n_slots + si] : nullptr;
        if (progress) {
          progress->store(0, std::memory_order_relaxed);
          prob.slot_running_[(size_t)di * prob.n_slots + si].store(1, std::memory_order_relaxed);
        }
        // trial: the evaluation is a line-search trial of `ls` (lbfgs_is_trial) and the problem evaluates those lazily -- the lml
        // first; K^-1 and the gradient only if lbfgs_advance will read the gradient (the Armijo test accepts the value:
        // lbfgs_trial_accepted) or the capture rule below will keep the evaluation (a new best lml: a rejected trial can lie
        // between f + 1e-4 gs and f).  Every other evaluation -- a run's start point, the fixed-work burn -- is one fused launch
        // sequence as ever.  The values the optimiser reads have the same bits either way, so the iterates do.
        auto obj = [&](const double* th, double* grad, const LbfgsState* ls) -> double {
          theta_to_params(th, lo, hi, d, s.hP);
          const int target = (s.best_idx < 0) ? 0 : 1 - s.best_idx;
          double lml;
          int st;
          if (ls) {
            st = prob.run_eval((size_t)di, si, target, Problem<T>::EVAL_LML_ONLY, true, &lml, nullptr, true);
            const bool new_best = st == HBEGP_OK && (s.best_idx < 0 || lml > s.best_lml);
            if (st == HBEGP_OK && (new_best || lbfgs_trial_accepted(*ls, -lml))) {
              // (a gradient that is not finite fails the whole evaluation here as in the fused form: +inf, never captured.  The one
              // difference from the fused form is on the other branch: a trial with a finite lml whose gradient WOULD be non-finite,
              // rejected and not a new best, keeps its finite lml and is not counted in n_not_pd -- its gradient is never formed)
              st = prob.run_eval((size_t)di, si, target, Problem<T>::EVAL_GRAD_ONLY, true, nullptr, grad);
              if (st != HBEGP_OK) lml = -std::numeric_limits<double>::infinity();
              rs.phase2++;
            } else {
              for (int j = 0; j < p; ++j) grad[j] = 0.0;  // never read
              n_lml_only.fetch_add(1);
              rs.lml_only++;
            }
          } else {
            st = prob.run_eval((size_t)di, si, target, !loo, true, &lml, loo ? nullptr : grad, true);
            rs.fused++;
          }
          const int share = prob.share_of_variant(s.dag_variant);
          if (share == SLOT_SHARE_LEAD) rs.lead++;
          if (share == SLOT_SHARE_LAG) rs.lag++;
          if (loo) {
            if (st == HBEGP_OK)
              st = objective == FIT_LGO ? prob.lgo_on_slot((size_t)di, si, *groups, lgo_lists.on((size_t)di), &lml, grad)
                                        : prob.loo_on_slot((size_t)di, si, &lml, grad);
            else for (int j = 0; j < p; ++j) grad[j] = 0.0;
            if (st != HBEGP_OK && st != HBEGP_NOT_PD) throw std::runtime_error(g_last_error);
          }
          const int my_eval = eval_idx++;
          if (progress) progress->store(eval_idx, std::memory_order_relaxed);
          n_evals.fetch_add(1);
          if (st != HBEGP_OK) n_not_pd.fetch_add(1);
          if (opt.trace_cap > 0) {
            std::lock_guard<std::mutex> lk(trace_mu);
            if (trace_n < opt.trace_cap) {
              const int tI = trace_n++;
              if (opt.trace_theta) memcpy(opt.trace_theta + (size_t)tI * p, th, sizeof(double) * p);
              if (opt.trace_lml) opt.trace_lml[tI] = lml;
              if (opt.trace_grad) memcpy(opt.trace_grad + (size_t)tI * p, grad, sizeof(double) * p);
              if (opt.trace_run) opt.trace_run[tI] = r;
            }
          }
          if (st != HBEGP_OK) return std::numeric_limits<double>::infinity();  // fit.rs:105-112
          // capture (fit.rs:116-125): strictly greater lml wins; ties keep the earlier (run, eval)
          if (s.best_idx < 0 || lml > s.best_lml) {
            s.best_idx = target;
            s.best_lml = lml;
            s.best_run = r;
            s.best_eval = my_eval;
            s.best_theta.assign(th, th + p);
          }
          for (int j = 0; j < p; ++j) grad[j] = -grad[j];  // fit.rs:128-133
          return -lml;
        };
        LbfgsOptions lo_opt;
        lo_opt.maxeval = opt.maxeval;
        lo_opt.fixed_work = opt.fixed_work != 0;
        if (opt.lbfgs_memory > 0) lo_opt.memory = opt.lbfgs_memory;
        // lbfgsb_minimize's loop around the state machine (lbfgsb.hpp), with the objective told which evaluations are trials
        static_assert(MAXP <= LBFGS_MAXN, "the GP's parameters fit the fixed-size optimiser state");
        std::vector<double> g(p);
        std::unique_ptr<LbfgsState> ls(new LbfgsState);
        lbfgs_begin(*ls, x.data(), lnlo.data(), lnhi.data(), p, lo_opt.maxeval, lo_opt.memory, lo_opt.pgtol, lo_opt.ftol, lo_opt.fixed_work);
        for (;;) {
          const bool trial = lazy && lbfgs_is_trial(*ls);
          const double f = obj(lbfgs_request(*ls), g.data(), trial ? ls.get() : nullptr);
          if (!lbfgs_advance(*ls, f, g.data())) break;
        }
        rs.end_ms = since_start_ms();
        if (progress) prob.slot_running_[(size_t)di * prob.n_slots + si].store(0, std::memory_order_relaxed);
      }
    } catch (const HipError& he) {
      hip_fail(he);
      std::lock_guard<std::mutex> lk(err_mu);
      err = g_last_error;
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> lk(err_mu);
      err = std::string("worker thread: ") + e.what();
    }
  };

  std::vector<std::thread> threads;
  try {
    for (int di = 0; di < ndev; ++di)
      for (int si = 0; si < std::min(runs_on[di], max_conc); ++si) threads.emplace_back(worker, di, si);
  } catch (...) {
    // thread creation failed part-way (std::system_error): the workers already started own device state -- let them
    // finish before the error leaves this frame (destroying a joinable std::thread terminates the process)
    for (auto& t : threads) t.join();
    throw;
  }
  for (auto& t : threads) t.join();
  // the workers append to the trace as their evaluations complete; hand it back in (run, eval) order
  if (opt.trace_cap > 0 && trace_n > 1 && opt.trace_run) {
    std::vector<int> order(trace_n);
    for (int i = 0; i < trace_n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return opt.trace_run[a] < opt.trace_run[b]; });
    auto permute = [&](auto* arr, int width) {
      if (!arr) return;
      std::vector<typename std::remove_pointer<decltype(arr)>::type> tmp((size_t)trace_n * width);
      for (int i = 0; i < trace_n; ++i) memcpy(&tmp[(size_t)i * width], arr + (size_t)order[i] * width, sizeof(tmp[0]) * width);
      memcpy(arr, tmp.data(), sizeof(tmp[0]) * tmp.size());
    };
    permute(opt.trace_theta, p);
    permute(opt.trace_lml, 1);
    permute(opt.trace_grad, p);
    permute(opt.trace_run, 1);
  }
  if (opt.trace_count) *opt.trace_count = trace_n;
  if (opt.n_evals) *opt.n_evals = n_evals.load();
  if (opt.n_not_pd) *opt.n_not_pd = n_not_pd.load();
  g_last_fit_stats.n_evals = n_evals.load();
  g_last_fit_stats.n_not_pd = n_not_pd.load();
  g_last_fit_stats.n_lml_only = n_lml_only.load();
  if (!err.empty()) return fail(HBEGP_EHIP, "%s", err.c_str());
  }  // host-driven optimiser runs

  g_last_fit_stats.n_runs = std::min(nruns, (int)HBEGP_STATS_MAX_RUNS);
  for (int r = 0; r < g_last_fit_stats.n_runs; ++r) g_last_fit_stats.run[r] = run_stats[r];
  if (timing)
    for (int r = 0; r < nruns; ++r)
      fprintf(stderr, "fit: run %d ended at %.2f ms: %d fused, %d lml-only, %d two-phase evaluations; %d with a lead share, %d with a lag share\n", r,
              run_stats[r].end_ms, run_stats[r].fused, run_stats[r].lml_only, run_stats[r].phase2, run_stats[r].lead, run_stats[r].lag);

  // global arg-max over the per-slot captures, ties -> lowest (run, eval)
  int bdi = -1, bsi = -1;
  for (int di = 0; di < ndev; ++di)
    for (int si = 0; si < (int)prob.slots[di].size(); ++si) {
      const Slot<T>& s = prob.slots[di][si];
      if (s.best_idx < 0) continue;
      bool better = bdi < 0;
      if (!better) {
        const Slot<T>& b = prob.slots[bdi][bsi];
        better = s.best_lml > b.best_lml ||
                 (s.best_lml == b.best_lml && (s.best_run < b.best_run || (s.best_run == b.best_run && s.best_eval < b.best_eval)));
      }
      if (better) { bdi = di; bsi = si; }
    }
  if (bdi < 0) return fail(HBEGP_ALL_FAILED, "every evaluation of the fit failed (kernel matrix not positive definite)");
  Slot<T>& best = prob.slots[bdi][bsi];
  // clamp the captured parameters (fit.rs:155-164)
  std::vector<double> th(p);
  for (int i = 0; i < p; ++i) {
    double v = std::exp(best.best_theta[i]);
    if (v < lo[i]) v = lo[i];
    if (hi[i] < v) v = hi[i];
    th[i] = std::log(v);
  }
  if (theta_best) memcpy(theta_best, th.data(), sizeof(double) * p);
  if (lml_best) *lml_best = best.best_lml;
  if (loo) {
    // the model is what `extend` gives at theta_best, bit for bit: built through that very path, once the fit's slots are back
    // in the pool
    prob.release();
    return model_out ? do_extend<T>(ctx, X, y, rv, n, d, nu, th.data(), nullptr, nullptr, model_out) : HBEGP_OK;
  }
  const auto tf2 = std::chrono::steady_clock::now();
  if (host_serial && prob.small_ && !host_lk.owns_lock()) host_lk.lock();
  const auto th1 = std::chrono::steady_clock::now();
  if (model_out) *model_out = make_model<T>(prob, (size_t)bdi, bsi, th.data(), best.best_lml, false, best.best_params.empty() ? nullptr : best.best_params.data());
  if (host_lk.owns_lock()) {
    prob.release();  // (again, harmlessly, when the problem goes out of scope)
    held_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th1).count();
    host_lk.unlock();
    if (timing) fprintf(stderr, "fit: host-side turns held for %.3f ms (set-up + model / release)\n", held_ms);
  }
  if (timing) {
    const auto tf3 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "fit: problem %.2f ms, optimiser runs %.2f ms (%d evaluations), model %.2f ms\n", ms(tf0, tf1), ms(tf1, tf2), n_evals.load(), ms(tf2, tf3));
  }
  return HBEGP_OK;
}

template <typename T>
static int do_extend(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model_out) {
  hbegp_ctx one;
  one.devs = {ctx->devs[0]};
  // One order of operations for one theta: the evaluation runs the way a fit's evaluations do at this size -- through the task
  // queue from 6 blocks on (its K^-1 split gives the undivided tiles' bits, DAGF_CINIT), as ad-hoc launches below that (a tile's
  // arithmetic does not depend on how the launch is scheduled).
  const int dag_env = env_int("HBEGP_DAG", -1);
  const bool queue_like_fit = (dag_env < 0 ? round_up(n, NB) / NB >= env_int("HBEGP_DAG_MIN_BLOCKS", DAG_MIN_BLOCKS_FIT) : dag_env != 0) && round_up(n, NB) / NB >= 2;
  Problem<T> prob(&one, X, y, n, d, nu, 1, !queue_like_fit, true, false, rv);
  const int p = d + 2;
  Slot<T>& s = prob.slots[0][0];
  theta_to_params(theta, lo, hi, d, s.hP);
  double lml;
  const int st = prob.run_eval(0, 0, 0, false, false, &lml, nullptr);
  if (st != HBEGP_OK) return fail(HBEGP_NOT_PD, "Kernel matrix must be invertible.");  // fit.rs:55
  s.best_idx = 0;
  std::vector<double> th(theta, theta + p);
  if (lo && hi)
    for (int i = 0; i < p; ++i) {
      double v = std::exp(theta[i]);
      if (v < lo[i]) v = lo[i];
      if (hi[i] < v) v = hi[i];
      th[i] = std::log(v);
    }
  if (model_out) *model_out = make_model<T>(prob, 0, 0, th.data(), lml, true);
  return HBEGP_OK;
}

// extend with a prior model fitted on a prefix of the rows (minimize.rs:629-644 appends the validation samples to the
// data the last model was built from): same theta, incremental factorisation; falls back to the full path when the
// prefix does not match or is shorter than one 128-block.
template <typename T>
static int do_extend_from(hbegp_ctx* ctx, hbegp_model* prior, const T* X, const T* y, const double* rv, int n, hbegp_model** model_out,
                          int* incremental) {
  if (incremental) *incremental = 0;
  const int d = prior->d, p = d + 2;
  const double nu = prior->nu2 == 0 ? std::numeric_limits<double>::infinity() : prior->nu2 / 2.0;
  if (prior->dev != ctx->devs[0] || n < prior->n || prior->n < NB || !prior->ldiag)
    return do_extend<T>(ctx, X, y, rv, n, d, nu, prior->theta.data(), nullptr, nullptr, model_out);
  hbegp_ctx one;
  one.devs = {ctx->devs[0]};
  static const int timing = env_int("HBEGP_TIMING", 0);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  Problem<T> prob(&one, X, y, n, d, nu, 1, true, false, false, rv);
  const auto t1 = now();
  Slot<T>& s = prob.slots[0][0];
  theta_to_params(prior->theta.data(), nullptr, nullptr, d, s.hP);
  int st;
  {
    std::lock_guard<std::mutex> lock(prior->mu);
    st = prob.extend_from(0, 0, static_cast<const T*>(prior->X), static_cast<const T*>(prior->rv), static_cast<const T*>(prior->Xinv),
                          static_cast<const T*>(prior->Kinv), static_cast<const T*>(prior->ldiag), prior->n, prior->np);
  }
  if (st == HBEGP_EINVAL) return do_extend<T>(ctx, X, y, rv, n, d, nu, prior->theta.data(), nullptr, nullptr, model_out);
  if (st != HBEGP_OK) return fail(HBEGP_NOT_PD, "Kernel matrix must be invertible.");  // fit.rs:55
  s.best_idx = 0;
  if (incremental) *incremental = 1;
  (void)p;
  const auto t2 = now();
  if (model_out) *model_out = make_model<T>(prob, 0, 0, prior->theta.data(), s.hOut->lml, true);
  const auto t3 = now();
  if (timing) fprintf(stderr, "extend_from: problem %.3f ms, factor %.3f ms, model %.3f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3));
  return HBEGP_OK;
}

static int check_args(hbegp_ctx* ctx, const void* X, const void* y, int n, int d, double nu) {
  if (!ctx) return fail(HBEGP_EINVAL, "ctx is NULL");
  if (!X || !y) return fail(HBEGP_EINVAL, "X/y is NULL");
  if (n < 1) return fail(HBEGP_EINVAL, "n must be >= 1 (got %d)", n);
  if (d < 1 || d > MAXD) return fail(HBEGP_EINVAL, "d must be in 1..%d (got %d)", MAXD, d);
  if (!(nu == 0.5 || nu == 1.5 || nu == 2.5 || (std::isinf(nu) && nu > 0)))  // infinity: squared exponential (extension)
    return fail(HBEGP_EINVAL, "Matern kernel with arbitrary values for nu is unimplemented (got %g)", nu);  // matern_kernel.rs:79
  return HBEGP_OK;
}

#define GUARD_BEGIN try {
#define GUARD_END                                   \
  }                                                 \
  catch (const HipError& he) { return hip_fail(he); } \
  catch (const std::bad_alloc&) { return fail(HBEGP_ENOMEM, "host allocation failed"); } \
  catch (const std::exception& e) { return fail(HBEGP_EHIP, "internal error: %s", e.what()); } \
  catch (...) { return fail(HBEGP_EHIP, "internal error: unknown exception"); }

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int hbegp_version(void) { return HBEGP_VERSION; }

int hbegp_device_count(void) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < cnt; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

const char* hbegp_last_error(void) { return g_last_error.c_str(); }

int hbegp_ctx_create(int n_devices, const int* device_ids, hbegp_ctx** out) {
  if (!out || n_devices < 1) return fail(HBEGP_EINVAL, "n_devices must be >= 1");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1)
    return fail(HBEGP_ENODEV, "no HIP device available: libhbegp has no CPU fallback");
  GUARD_BEGIN
  std::unique_ptr<hbegp_ctx> ctx(new hbegp_ctx());
  for (int i = 0; i < n_devices; ++i) {
    const int id = device_ids ? device_ids[i] : i;
    if (id < 0 || id >= cnt) return fail(HBEGP_ENODEV, "device %d not present (%d visible)", id, cnt);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(HBEGP_ENODEV, "device %d is %s; this library only carries gfx950 code", id, prop.gcnArchName);
    HIPCHECK(hipSetDevice(id));
    init_kernels();
    ctx->devs.push_back(id);
  }
  *out = ctx.release();
  g_live_ctx.fetch_add(1);
  return HBEGP_OK;
  GUARD_END
}
void hbegp_ctx_destroy(hbegp_ctx* ctx) {
  if (!ctx) return;
  delete ctx;
  if (g_live_ctx.fetch_sub(1) == 1) {
    g_pool.trim();
    g_host_pool.trim();
    g_stream_pool.trim();
  }
}

int hbegp_problem_create_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, int n_slots,
                             hbegp_problem** out) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!out || n_slots < 1) return fail(HBEGP_EINVAL, "bad out/n_slots");
  GUARD_BEGIN
  std::unique_ptr<hbegp_problem> p(new hbegp_problem());
  p->impl.reset(new Problem<double>(ctx, X, y, n, d, nu, n_slots));
  *out = p.release();
  return HBEGP_OK;
  GUARD_END
}
int hbegp_problem_create_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, int n_slots,
                             hbegp_problem** out) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!out || n_slots < 1) return fail(HBEGP_EINVAL, "bad out/n_slots");
  GUARD_BEGIN
  std::unique_ptr<hbegp_problem> p(new hbegp_problem());
  p->impl.reset(new Problem<float>(ctx, X, y, n, d, nu, n_slots));
  *out = p.release();
  return HBEGP_OK;
  GUARD_END
}
void hbegp_problem_destroy(hbegp_problem* prob) { delete prob; }

int hbegp_problem_eval(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                       double* lml, double* grad) {
  if (!prob || !theta || !lml) return fail(HBEGP_EINVAL, "NULL argument");
  GUARD_BEGIN
  return prob->impl->eval(dev, slot, theta, lo, hi, lml, grad);
  GUARD_END
}

int hbegp_problem_eval_loo(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           double* loo, double* grad) {
  if (!prob) return fail(HBEGP_EINVAL, "NULL problem");
  if (!theta || !loo) return fail(HBEGP_EINVAL, "theta / loo is NULL");
  GUARD_BEGIN
  return prob->impl->eval_loo(dev, slot, theta, lo, hi, loo, grad);
  GUARD_END
}

int hbegp_problem_eval_lgo(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           const int* group, double* lgo, double* grad) {
  if (!prob) return fail(HBEGP_EINVAL, "NULL problem");
  if (!theta || !lgo) return fail(HBEGP_EINVAL, "theta / lgo is NULL");
  GUARD_BEGIN
  LgoGroups gr;
  if (int e = build_lgo_groups(group, prob->impl->n, &gr)) return e;
  return prob->impl->eval_lgo(dev, slot, theta, lo, hi, gr, lgo, grad);
  GUARD_END
}

int hbegp_problem_eval_xgrad(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                             double* lml, double* grad, double* gx) {
  if (!prob) return fail(HBEGP_EINVAL, "NULL problem");
  if (!theta || !lml || !gx) return fail(HBEGP_EINVAL, "theta / lml / gx is NULL");
  GUARD_BEGIN
  return prob->impl->eval_xgrad(dev, slot, theta, lo, hi, lml, grad, gx);
  GUARD_END
}

int hbegp_problem_eval_warped(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                              const double* ab, double* lml, double* grad) {
  if (!prob) return fail(HBEGP_EINVAL, "NULL problem");
  if (!theta || !ab || !lml) return fail(HBEGP_EINVAL, "theta / ab / lml is NULL");
  GUARD_BEGIN
  return prob->impl->eval_warped(dev, slot, theta, lo, hi, ab, lml, grad);
  GUARD_END
}

int hbegp_problem_debug_rows_f64(hbegp_problem* prob, int dev, double* out) {
  if (!prob || !out) return fail(HBEGP_EINVAL, "NULL argument");
  GUARD_BEGIN
  return prob->impl->get_rows(dev, out, false);
  GUARD_END
}
int hbegp_problem_debug_rows_f32(hbegp_problem* prob, int dev, float* out) {
  if (!prob || !out) return fail(HBEGP_EINVAL, "NULL argument");
  GUARD_BEGIN
  return prob->impl->get_rows(dev, out, true);
  GUARD_END
}

static int warp_check_ab(const double* ab, int d) {
  if (!ab || d < 1) return fail(HBEGP_EINVAL, "warp: NULL parameters or d < 1");
  for (int k = 0; k < 2 * d; ++k)
    if (!std::isfinite(ab[k]) || !(ab[k] > 0.0)) return fail(HBEGP_EINVAL, "warp parameter %d is not a positive finite number", k);
  return HBEGP_OK;
}
int hbegp_warp_apply(const double* ab, int d, const double* X, int m, double* U, double* dU_dlna, double* dU_dlnb, double* dU_dx) {
  if (int e = warp_check_ab(ab, d)) return e;
  if (m < 0 || (m > 0 && !X)) return fail(HBEGP_EINVAL, "warp: m < 0 or NULL X");
  const size_t count = (size_t)m * d;
  for (size_t e = 0; e < count; ++e)
    if (!(X[e] >= 0.0 && X[e] <= 1.0)) return fail(HBEGP_EINVAL, "warp: row %zu, feature %zu is outside [0, 1]", e / d, e % d);
  for (size_t e = 0; e < count; ++e) {
    const int k = (int)(e % d);
    hbegp::warp::apply(ab[k], ab[d + k], X[e], U ? U + e : nullptr, dU_dlna ? dU_dlna + e : nullptr, dU_dlnb ? dU_dlnb + e : nullptr,
                       dU_dx ? dU_dx + e : nullptr);
  }
  return HBEGP_OK;
}
int hbegp_warp_invert(const double* ab, int d, const double* U, int m, double* X) {
  if (int e = warp_check_ab(ab, d)) return e;
  if (m < 0 || (m > 0 && (!U || !X))) return fail(HBEGP_EINVAL, "warp: m < 0 or NULL U / X");
  const size_t count = (size_t)m * d;
  for (size_t e = 0; e < count; ++e)
    if (!(U[e] >= 0.0 && U[e] <= 1.0)) return fail(HBEGP_EINVAL, "warp: row %zu, feature %zu is outside [0, 1]", e / d, e % d);
  for (size_t e = 0; e < count; ++e) {
    const int k = (int)(e % d);
    X[e] = hbegp::warp::invert(ab[k], ab[d + k], U[e]);
  }
  return HBEGP_OK;
}

int hbegp_problem_time_concurrent(hbegp_problem* prob, int dev, const double* theta, int reps, double* out) {
  if (!prob || !theta || !out || reps < 1) return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  return prob->impl->time_concurrent(dev, theta, reps, out);
  GUARD_END
}

int hbegp_problem_time_eval(hbegp_problem* prob, int dev, int slot, const double* theta, int reps, double* phase_ms) {
  if (!prob || !theta || reps < 1) return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  return prob->impl->time_eval(dev, slot, theta, reps, phase_ms);
  GUARD_END
}

}  // extern "C"
template <typename T>
static int problem_get(hbegp_problem* prob, int dev, int slot, T* alpha, T* kinv, T* ldiag) {
  if (!prob) return fail(HBEGP_EINVAL, "NULL problem");
  auto* p = dynamic_cast<Problem<T>*>(prob->impl.get());
  if (!p) return fail(HBEGP_EINVAL, "element type mismatch");
  if (dev < 0 || dev >= (int)p->slots.size() || slot < 0 || slot >= p->n_slots) return fail(HBEGP_EINVAL, "bad device/slot index");
  GUARD_BEGIN
  Slot<T>& s = p->slots[dev][slot];
  HIPCHECK(hipSetDevice(s.dev));
  const int b = s.last_target, n = p->n, np = p->np;
  // (copies on the slot's own stream: a null-stream copy fails while another host thread captures a graph)
  if (alpha) HIPCHECK(hipMemcpyAsync(alpha, s.alpha[b], sizeof(T) * n, hipMemcpyDeviceToHost, s.stream));
  if (ldiag) HIPCHECK(hipMemcpyAsync(ldiag, s.ldiag, sizeof(T) * n, hipMemcpyDeviceToHost, s.stream));
  HIPCHECK(hipStreamSynchronize(s.stream));
  if (kinv) {
    std::vector<T> tmp((size_t)np * np);
    HIPCHECK(hipMemcpyAsync(tmp.data(), s.Kinv[b], sizeof(T) * tmp.size(), hipMemcpyDeviceToHost, s.stream));
    HIPCHECK(hipStreamSynchronize(s.stream));
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) kinv[(size_t)i * n + j] = kinv[(size_t)j * n + i] = tmp[(size_t)i * np + j];
  }
  return HBEGP_OK;
  GUARD_END
}
template <typename T>
static int problem_debug_get(hbegp_problem* prob, int dev, int slot, int which, T* out) {
  if (!prob || !out) return fail(HBEGP_EINVAL, "NULL argument");
  auto* p = dynamic_cast<Problem<T>*>(prob->impl.get());
  if (!p) return fail(HBEGP_EINVAL, "element type mismatch");
  if (dev < 0 || dev >= (int)p->slots.size() || slot < 0 || slot >= p->n_slots || which < 1 || which > 4)
    return fail(HBEGP_EINVAL, "bad device/slot/which");
  GUARD_BEGIN
  Slot<T>& s = p->slots[dev][slot];
  HIPCHECK(hipSetDevice(s.dev));
  HIPCHECK(hipStreamSynchronize(s.stream));
  const T* src = which == 1 ? s.W1 : (which == 2 ? s.W2 : (which == 3 ? s.W3 : s.Kinv[s.last_target]));
  if (!src) return fail(HBEGP_EINVAL, "this problem has no such work matrix");
  HIPCHECK(hipMemcpyAsync(out, src, sizeof(T) * (size_t)p->np * p->np, hipMemcpyDeviceToHost, s.stream));
  HIPCHECK(hipStreamSynchronize(s.stream));
  return HBEGP_OK;
  GUARD_END
}
extern "C" {
int hbegp_problem_debug_get_f64(hbegp_problem* prob, int dev, int slot, int which, double* out) {
  return problem_debug_get<double>(prob, dev, slot, which, out);
}
int hbegp_problem_debug_get_f32(hbegp_problem* prob, int dev, int slot, int which, float* out) {
  return problem_debug_get<float>(prob, dev, slot, which, out);
}
int hbegp_problem_get_f64(hbegp_problem* prob, int dev, int slot, double* alpha, double* kinv, double* ldiag) {
  return problem_get<double>(prob, dev, slot, alpha, kinv, ldiag);
}
int hbegp_problem_get_f32(hbegp_problem* prob, int dev, int slot, float* alpha, float* kinv, float* ldiag) {
  return problem_get<float>(prob, dev, slot, alpha, kinv, ldiag);
}

}  // extern "C"
template <typename T>
static int problem_kmat(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi, T* K) {
  if (!prob || !theta || !K) return fail(HBEGP_EINVAL, "NULL argument");
  auto* p = dynamic_cast<Problem<T>*>(prob->impl.get());
  if (!p) return fail(HBEGP_EINVAL, "element type mismatch");
  if (dev < 0 || dev >= (int)p->slots.size() || slot < 0 || slot >= p->n_slots) return fail(HBEGP_EINVAL, "bad device/slot index");
  GUARD_BEGIN
  Slot<T>& s = p->slots[dev][slot];
  HIPCHECK(hipSetDevice(s.dev));
  theta_to_params(theta, lo, hi, p->d, s.hP);
  HIPCHECK(hipMemcpyAsync(s.dP, s.hP, sizeof(EvalParams), hipMemcpyHostToDevice, s.stream));
  launch_reset_out(s.dOut, s.stream);
  launch_kmat<T>(p->Xd[dev], p->rvd[dev], p->n, p->d, p->np, p->nu2, s.dP, s.W1, &s.dOut->info, s.stream);
  CHECK_LAUNCHES();
  const int n = p->n, np = p->np;
  std::vector<T> tmp((size_t)np * np);
  HIPCHECK(hipMemcpyAsync(tmp.data(), s.W1, sizeof(T) * tmp.size(), hipMemcpyDeviceToHost, s.stream));
  HIPCHECK(hipStreamSynchronize(s.stream));
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) K[(size_t)i * n + j] = K[(size_t)j * n + i] = tmp[(size_t)i * np + j];
  return HBEGP_OK;
  GUARD_END
}
extern "C" {
int hbegp_problem_kmat_f64(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           double* K) {
  return problem_kmat<double>(prob, dev, slot, theta, lo, hi, K);
}
int hbegp_problem_kmat_f32(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           float* K) {
  return problem_kmat<float>(prob, dev, slot, theta, lo, hi, K);
}

int hbegp_fit_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta0,
                  const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                  double* theta_best, double* lml_best, hbegp_model** model) {
  {
    hbegp_fit_options probe;
    if (int e = read_fit_options(opt, &probe)) return e;  // before anything else: a mis-sized struct is a build problem
  }
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "theta0/lo/hi/starts is NULL");
  GUARD_BEGIN
  return do_fit<double>(ctx, X, y, nullptr, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model);
  GUARD_END
}
int hbegp_fit_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta0,
                  const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                  double* theta_best, double* lml_best, hbegp_model** model) {
  {
    hbegp_fit_options probe;
    if (int e = read_fit_options(opt, &probe)) return e;  // before anything else: a mis-sized struct is a build problem
  }
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "theta0/lo/hi/starts is NULL");
  GUARD_BEGIN
  return do_fit<float>(ctx, X, y, nullptr, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model);
  GUARD_END
}

int hbegp_fit_loo_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta0,
                      const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model) {
  {
    hbegp_fit_options probe;
    if (int e = read_fit_options(opt, &probe)) return e;
  }
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "NULL theta0/lo/hi/starts");
  GUARD_BEGIN
  return do_fit<double>(ctx, X, y, nullptr, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, loo_best, model, FIT_LOO);
  GUARD_END
}
int hbegp_fit_loo_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta0,
                      const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model) {
  {
    hbegp_fit_options probe;
    if (int e = read_fit_options(opt, &probe)) return e;
  }
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "NULL theta0/lo/hi/starts");
  GUARD_BEGIN
  return do_fit<float>(ctx, X, y, nullptr, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, loo_best, model, FIT_LOO);
  GUARD_END
}

int hbegp_extend_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta) return fail(HBEGP_EINVAL, "theta is NULL");
  GUARD_BEGIN
  return do_extend<double>(ctx, X, y, nullptr, n, d, nu, theta, lo, hi, model);
  GUARD_END
}
int hbegp_extend_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta) return fail(HBEGP_EINVAL, "theta is NULL");
  GUARD_BEGIN
  return do_extend<float>(ctx, X, y, nullptr, n, d, nu, theta, lo, hi, model);
  GUARD_END
}

int hbegp_extend_from_f64(hbegp_ctx* ctx, hbegp_model* prior, const double* X, const double* y, int n, hbegp_model** model,
                          int* incremental) {
  if (!ctx || !prior || !X || !y) return fail(HBEGP_EINVAL, "ctx/prior/X/y is NULL");
  if (prior->is_f32) return fail(HBEGP_EINVAL, "prior model holds f32 data");
  if (n < 1) return fail(HBEGP_EINVAL, "n must be >= 1 (got %d)", n);
  if (prior->rv) return fail(HBEGP_EINVAL, "the prior model carries row variances: extend it with hbegp_extend_from_rv_*");
  GUARD_BEGIN
  return do_extend_from<double>(ctx, prior, X, y, nullptr, n, model, incremental);
  GUARD_END
}
int hbegp_extend_from_f32(hbegp_ctx* ctx, hbegp_model* prior, const float* X, const float* y, int n, hbegp_model** model,
                          int* incremental) {
  if (!ctx || !prior || !X || !y) return fail(HBEGP_EINVAL, "ctx/prior/X/y is NULL");
  if (!prior->is_f32) return fail(HBEGP_EINVAL, "prior model holds f64 data");
  if (n < 1) return fail(HBEGP_EINVAL, "n must be >= 1 (got %d)", n);
  if (prior->rv) return fail(HBEGP_EINVAL, "the prior model carries row variances: extend it with hbegp_extend_from_rv_*");
  GUARD_BEGIN
  return do_extend_from<float>(ctx, prior, X, y, nullptr, n, model, incremental);
  GUARD_END
}

int hbegp_predict_f64(hbegp_model* model, const double* Xs, int m, double* mean, double* var, int* n_warn) {
  if (!model || !Xs || !mean || m < 0) return fail(HBEGP_EINVAL, "bad argument");
  if (model->is_f32) return fail(HBEGP_EINVAL, "model holds f32 data");
  if (m == 0) { if (n_warn) *n_warn = 0; return HBEGP_OK; }
  GUARD_BEGIN
  return model_predict<double>(model, Xs, m, mean, var, n_warn);
  GUARD_END
}
int hbegp_predict_f32(hbegp_model* model, const float* Xs, int m, float* mean, float* var, int* n_warn) {
  if (!model || !Xs || !mean || m < 0) return fail(HBEGP_EINVAL, "bad argument");
  if (!model->is_f32) return fail(HBEGP_EINVAL, "model holds f64 data");
  if (m == 0) { if (n_warn) *n_warn = 0; return HBEGP_OK; }
  GUARD_BEGIN
  return model_predict<float>(model, Xs, m, mean, var, n_warn);
  GUARD_END
}

}  // extern "C"
// ---- known per-row noise variances (hbegp.h: "row variances"): the entry points above with `rv` behind y ---------------------
// Refused before any device call: a variance that is negative or not finite (in the element type it is converted to).
template <typename T>
static int check_rv(const double* rv, int n) {
  if (!rv) return HBEGP_OK;
  for (int i = 0; i < n; ++i)
    if (!(rv[i] >= 0.0) || !std::isfinite((T)rv[i]))
      return fail(HBEGP_EINVAL, "rv[%d] = %g: a row variance must be finite and >= 0", i, rv[i]);
  return HBEGP_OK;
}
template <typename T>
static int problem_create_rv(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, int n_slots,
                             hbegp_problem** out) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!out || n_slots < 1) return fail(HBEGP_EINVAL, "bad out/n_slots");
  if (int e = check_rv<T>(rv, n)) return e;
  GUARD_BEGIN
  std::unique_ptr<hbegp_problem> p(new hbegp_problem());
  p->impl.reset(new Problem<T>(ctx, X, y, n, d, nu, n_slots, false, false, false, rv));
  *out = p.release();
  return HBEGP_OK;
  GUARD_END
}
template <typename T>
static int fit_rv(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta0, const double* lo,
                  const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt, double* theta_best, double* best,
                  hbegp_model** model, int objective, const int* group = nullptr) {
  {
    hbegp_fit_options probe;
    if (int e = read_fit_options(opt, &probe)) return e;  // the order of the plain entry points: options, arguments, then rv
  }
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "theta0/lo/hi/starts is NULL");
  if (int e = check_rv<T>(rv, n)) return e;
  GUARD_BEGIN
  LgoGroups gr;
  if (objective == FIT_LGO)
    if (int e = build_lgo_groups(group, n, &gr)) return e;
  return do_fit<T>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, best, model, objective, &gr);
  GUARD_END
}
// The warped fit (hbegp_fit_warped_*): bounded L-BFGS (lbfgsb_minimize) over the p + 2 d log-space variables
// [theta, ln a, ln b] with hbegp_problem_eval_warped's value and gradient, on ONE single-slot problem with the fit's path selection,
// 1 + n_restarts runs one after another (the feature buffer is rewritten by every evaluation: runs side by side would need one per
// slot).  The capture rule is do_fit's: the best lml wins, ties keep the earlier (run, evaluation); a failed evaluation counts as
// +inf with a zero gradient.  The model is do_extend at theta_best on the rows warped by ab_best.
template <typename T>
static int fit_warped(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta0,
                      const double* lo, const double* hi, const double* ab0, const double* ab_lo, const double* ab_hi,
                      const double* starts, int n_restarts, const hbegp_fit_options* opt_in, double* theta_best, double* ab_best,
                      double* lml_best, hbegp_model** model_out) {
  hbegp_fit_options opt{};
  if (int e = read_fit_options(opt_in, &opt)) return e;
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta0 || !lo || !hi || (n_restarts > 0 && !starts)) return fail(HBEGP_EINVAL, "theta0/lo/hi/starts is NULL");
  if (int e = check_rv<T>(rv, n)) return e;
  const int p = d + 2, q = p + 2 * d;
  std::vector<double> lnlo(q), lnhi(q), wlo(2 * d), whi(2 * d);
  for (int k = 0; k < 2 * d; ++k) {
    wlo[k] = ab_lo ? ab_lo[k] : 0.2;
    whi[k] = ab_hi ? ab_hi[k] : 5.0;
    if (!std::isfinite(wlo[k]) || !std::isfinite(whi[k]) || !(wlo[k] > 0.0) || !(wlo[k] <= whi[k]))
      return fail(HBEGP_EINVAL, "warp bounds %d: need 0 < lo <= hi, both finite (got %g, %g)", k, wlo[k], whi[k]);
    if (ab0 && (!std::isfinite(ab0[k]) || !(ab0[k] > 0.0))) return fail(HBEGP_EINVAL, "ab0[%d] is not a positive finite number", k);
  }
  for (size_t e = 0; e < (size_t)n * d; ++e)
    if (!(X[e] >= T(0) && X[e] <= T(1)))
      return fail(HBEGP_EINVAL, "input warping needs features in [0, 1]: row %zu, feature %zu is %g", e / d, e % d, (double)X[e]);
  GUARD_BEGIN
  if (opt.maxeval <= 0) opt.maxeval = 150;
  for (int i = 0; i < p; ++i) {
    lnlo[i] = std::log(lo[i]);
    lnhi[i] = std::log(hi[i]);
  }
  for (int k = 0; k < 2 * d; ++k) {
    lnlo[p + k] = std::log(wlo[k]);
    lnhi[p + k] = std::log(whi[k]);
  }
  hbegp_ctx one;
  one.devs = {ctx->devs[0]};
  const int nruns = 1 + std::max(0, n_restarts);
  int n_evals = 0, n_not_pd = 0, trace_n = 0;
  double best_lml = -std::numeric_limits<double>::infinity();
  std::vector<double> best_v;
  {
    Problem<T> prob(&one, X, y, n, d, nu, 1, false, true, false, rv);
    std::vector<double> ab(2 * d), x(q);
    for (int r = 0; r < nruns; ++r) {
      if (r == 0) {
        for (int i = 0; i < p; ++i) x[i] = theta0[i];
        for (int k = 0; k < 2 * d; ++k) x[p + k] = ab0 ? std::log(ab0[k]) : 0.0;
      } else {
        for (int i = 0; i < q; ++i) x[i] = starts[(size_t)(r - 1) * q + i];
      }
      Objective obj = [&](const double* v, double* grad) -> double {
        for (int k = 0; k < 2 * d; ++k) ab[k] = std::min(std::max(std::exp(v[p + k]), wlo[k]), whi[k]);
        double lml;
        const int st = prob.eval_warped(0, 0, v, lo, hi, ab.data(), &lml, grad);
        if (st != HBEGP_OK && st != HBEGP_NOT_PD) throw std::runtime_error(g_last_error);
        ++n_evals;
        if (st != HBEGP_OK) {
          ++n_not_pd;
          lml = -std::numeric_limits<double>::infinity();
          for (int j = 0; j < q; ++j) grad[j] = 0.0;
        }
        if (opt.trace_cap > 0 && trace_n < opt.trace_cap) {
          const int tI = trace_n++;
          if (opt.trace_theta) memcpy(opt.trace_theta + (size_t)tI * q, v, sizeof(double) * q);
          if (opt.trace_lml) opt.trace_lml[tI] = lml;
          if (opt.trace_grad) memcpy(opt.trace_grad + (size_t)tI * q, grad, sizeof(double) * q);
          if (opt.trace_run) opt.trace_run[tI] = r;
        }
        if (st != HBEGP_OK) return std::numeric_limits<double>::infinity();
        if (best_v.empty() || lml > best_lml) {  // runs and evaluations come in order: a tie keeps the earlier one
          best_lml = lml;
          best_v.assign(v, v + q);
        }
        for (int j = 0; j < q; ++j) grad[j] = -grad[j];
        return -lml;
      };
      LbfgsOptions lo_opt;
      lo_opt.maxeval = opt.maxeval;
      lo_opt.fixed_work = opt.fixed_work != 0;
      if (opt.lbfgs_memory > 0) lo_opt.memory = opt.lbfgs_memory;
      lbfgsb_minimize(obj, x.data(), lnlo.data(), lnhi.data(), q, lo_opt);
    }
  }  // the fit's slot is back in the pool before the model is built
  if (opt.trace_count) *opt.trace_count = trace_n;
  if (opt.n_evals) *opt.n_evals = n_evals;
  if (opt.n_not_pd) *opt.n_not_pd = n_not_pd;
  if (best_v.empty()) return fail(HBEGP_ALL_FAILED, "every evaluation of the fit failed (kernel matrix not positive definite)");
  std::vector<double> th(p), abw(2 * d);
  for (int i = 0; i < p; ++i) th[i] = std::log(std::min(std::max(std::exp(best_v[i]), lo[i]), hi[i]));
  for (int k = 0; k < 2 * d; ++k) abw[k] = std::min(std::max(std::exp(best_v[p + k]), wlo[k]), whi[k]);
  if (theta_best) memcpy(theta_best, th.data(), sizeof(double) * p);
  if (ab_best) memcpy(ab_best, abw.data(), sizeof(double) * 2 * d);
  if (lml_best) *lml_best = best_lml;
  if (!model_out) return HBEGP_OK;
  // the rows the captured evaluation read: hbegp_warp_apply's U rounded once to T (the device's warp is the same function)
  std::vector<T> U((size_t)n * d);
  for (size_t e = 0; e < U.size(); ++e) {
    double u;
    hbegp::warp::apply(abw[e % d], abw[d + e % d], (double)X[e], &u, nullptr, nullptr, nullptr);
    U[e] = (T)u;
  }
  const int st = do_extend<T>(ctx, U.data(), y, rv, n, d, nu, th.data(), nullptr, nullptr, model_out);
  if (st == HBEGP_OK) (*model_out)->warp_ab = abw;
  return st;
  GUARD_END
}

template <typename T>
static int extend_rv(hbegp_ctx* ctx, const T* X, const T* y, const double* rv, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model) {
  if (int e = check_args(ctx, X, y, n, d, nu)) return e;
  if (!theta) return fail(HBEGP_EINVAL, "theta is NULL");
  if (int e = check_rv<T>(rv, n)) return e;
  GUARD_BEGIN
  return do_extend<T>(ctx, X, y, rv, n, d, nu, theta, lo, hi, model);
  GUARD_END
}
template <typename T>
static int extend_from_rv(hbegp_ctx* ctx, hbegp_model* prior, const T* X, const T* y, const double* rv, int n, hbegp_model** model,
                          int* incremental) {
  if (!ctx || !prior || !X || !y) return fail(HBEGP_EINVAL, "ctx/prior/X/y is NULL");
  if (prior->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, prior->is_f32 ? "prior model holds f32 data" : "prior model holds f64 data");
  if (n < 1) return fail(HBEGP_EINVAL, "n must be >= 1 (got %d)", n);
  if (int e = check_rv<T>(rv, n)) return e;
  // rv = NULL is the plain call, and the plain call refuses such a prior
  if (!rv && prior->rv) return fail(HBEGP_EINVAL, "the prior model carries row variances: extend it with hbegp_extend_from_rv_* and the rows' rv");
  GUARD_BEGIN
  return do_extend_from<T>(ctx, prior, X, y, rv, n, model, incremental);
  GUARD_END
}
extern "C" {
int hbegp_problem_create_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu, int n_slots,
                                hbegp_problem** out) {
  return problem_create_rv<double>(ctx, X, y, rv, n, d, nu, n_slots, out);
}
int hbegp_problem_create_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu, int n_slots,
                                hbegp_problem** out) {
  return problem_create_rv<float>(ctx, X, y, rv, n, d, nu, n_slots, out);
}
int hbegp_fit_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu, const double* theta0,
                     const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                     double* theta_best, double* lml_best, hbegp_model** model) {
  return fit_rv<double>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model, false);
}
int hbegp_fit_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu, const double* theta0,
                     const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                     double* theta_best, double* lml_best, hbegp_model** model) {
  return fit_rv<float>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model, false);
}
int hbegp_fit_lgo_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, const int* group, int n, int d, double nu,
                      const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* lgo_best, hbegp_model** model) {
  return fit_rv<double>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lgo_best, model, FIT_LGO, group);
}
int hbegp_fit_lgo_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, const int* group, int n, int d, double nu,
                      const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* lgo_best, hbegp_model** model) {
  return fit_rv<float>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lgo_best, model, FIT_LGO, group);
}
int hbegp_fit_loo_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu, const double* theta0,
                         const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                         double* theta_best, double* loo_best, hbegp_model** model) {
  return fit_rv<double>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, loo_best, model, FIT_LOO);
}
int hbegp_fit_loo_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu, const double* theta0,
                         const double* lo, const double* hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                         double* theta_best, double* loo_best, hbegp_model** model) {
  return fit_rv<float>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, loo_best, model, FIT_LOO);
}
int hbegp_extend_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu, const double* theta,
                        const double* lo, const double* hi, hbegp_model** model) {
  return extend_rv<double>(ctx, X, y, rv, n, d, nu, theta, lo, hi, model);
}
int hbegp_extend_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu, const double* theta,
                        const double* lo, const double* hi, hbegp_model** model) {
  return extend_rv<float>(ctx, X, y, rv, n, d, nu, theta, lo, hi, model);
}
int hbegp_extend_from_rv_f64(hbegp_ctx* ctx, hbegp_model* prior, const double* X, const double* y, const double* rv, int n,
                             hbegp_model** model, int* incremental) {
  return extend_from_rv<double>(ctx, prior, X, y, rv, n, model, incremental);
}
int hbegp_extend_from_rv_f32(hbegp_ctx* ctx, hbegp_model* prior, const float* X, const float* y, const double* rv, int n,
                             hbegp_model** model, int* incremental) {
  return extend_from_rv<float>(ctx, prior, X, y, rv, n, model, incremental);
}
int hbegp_model_warp(const hbegp_model* model, double* ab) {
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->warp_ab.empty()) return 0;
  if (ab) memcpy(ab, model->warp_ab.data(), sizeof(double) * model->warp_ab.size());
  return 1;
}
int hbegp_fit_warped_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu, const double* theta0,
                         const double* lo, const double* hi, const double* ab0, const double* ab_lo, const double* ab_hi,
                         const double* starts, int n_restarts, const hbegp_fit_options* opt, double* theta_best, double* ab_best,
                         double* lml_best, hbegp_model** model) {
  return fit_warped<double>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, ab0, ab_lo, ab_hi, starts, n_restarts, opt, theta_best, ab_best,
                            lml_best, model);
}
int hbegp_fit_warped_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu, const double* theta0,
                         const double* lo, const double* hi, const double* ab0, const double* ab_lo, const double* ab_hi,
                         const double* starts, int n_restarts, const hbegp_fit_options* opt, double* theta_best, double* ab_best,
                         double* lml_best, hbegp_model** model) {
  return fit_warped<float>(ctx, X, y, rv, n, d, nu, theta0, lo, hi, ab0, ab_lo, ab_hi, starts, n_restarts, opt, theta_best, ab_best,
                           lml_best, model);
}
int hbegp_model_row_variance(const hbegp_model* model, double* rv) {
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (!model->rv) return 0;
  if (!rv) return 1;
  GUARD_BEGIN
  hbegp_model* m = const_cast<hbegp_model*>(model);
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  const size_t n = (size_t)m->n;
  if (m->is_f32) {
    std::vector<float> tmp(n);
    HIPCHECK(hipMemcpyAsync(tmp.data(), m->rv, sizeof(float) * n, hipMemcpyDeviceToHost, m->stream));
    HIPCHECK(hipStreamSynchronize(m->stream));
    for (size_t i = 0; i < n; ++i) rv[i] = (double)tmp[i];
  } else {
    HIPCHECK(hipMemcpyAsync(rv, m->rv, sizeof(double) * n, hipMemcpyDeviceToHost, m->stream));
    HIPCHECK(hipStreamSynchronize(m->stream));
  }
  return 1;
  GUARD_END
}
}  // extern "C"

// argument checks of the gradient entry points: everything is refused before any device call
template <typename T>
static int check_predict_grad(hbegp_model* model, const T* Xs, int m, T* mean, T* var, T* dmean, T* dvar) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (!Xs || !mean || !dmean) return fail(HBEGP_EINVAL, "Xs/mean/dmean is NULL");
  if ((var == nullptr) != (dvar == nullptr)) return fail(HBEGP_EINVAL, "var and dvar must be given together or both be NULL");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
template <typename T>
static int check_maximize_ei(hbegp_model* model, const T* starts, int S, const double* lo, const double* hi, double fmin, int maxeval,
                             T* x_out, double* ei_out) {
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (!starts || !lo || !hi || !x_out || !ei_out) return fail(HBEGP_EINVAL, "starts/lo/hi/x_out/ei_out is NULL");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  if (maxeval < 1) return fail(HBEGP_EINVAL, "maxeval must be >= 1 (got %d)", maxeval);
  if (!std::isfinite(fmin)) return fail(HBEGP_EINVAL, "fmin_normalized is not finite");
  const int d = model->d;
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return fail(HBEGP_EINVAL, "lo[%d] > hi[%d] (%g > %g)", k, k, lo[k], hi[k]);
  for (int r = 0; r < S; ++r)
    for (int k = 0; k < d; ++k) {
      const double v = (double)starts[(size_t)r * d + k];
      if (!(v >= lo[k] && v <= hi[k])) return fail(HBEGP_EINVAL, "start %d lies outside the box (feature %d: %g)", r, k, v);
    }
  return HBEGP_OK;
}
extern "C" {
int hbegp_predict_grad_f64(hbegp_model* model, const double* Xs, int m, double* mean, double* var, double* dmean, double* dvar,
                           int* n_warn) {
  if (int rc = check_predict_grad<double>(model, Xs, m, mean, var, dmean, dvar)) return rc;
  if (m == 0) { if (n_warn) *n_warn = 0; return HBEGP_OK; }
  GUARD_BEGIN
  return model_predict_grad<double>(model, Xs, m, mean, var, dmean, dvar, n_warn);
  GUARD_END
}
int hbegp_predict_grad_f32(hbegp_model* model, const float* Xs, int m, float* mean, float* var, float* dmean, float* dvar, int* n_warn) {
  if (int rc = check_predict_grad<float>(model, Xs, m, mean, var, dmean, dvar)) return rc;
  if (m == 0) { if (n_warn) *n_warn = 0; return HBEGP_OK; }
  GUARD_BEGIN
  return model_predict_grad<float>(model, Xs, m, mean, var, dmean, dvar, n_warn);
  GUARD_END
}
int hbegp_maximize_ei_f64(hbegp_model* model, const double* starts, int S, const double* lo, const double* hi, double fmin_normalized,
                          int maxeval, double* x_out, double* ei_out, int* nevals_out) {
  if (int rc = check_maximize_ei<double>(model, starts, S, lo, hi, fmin_normalized, maxeval, x_out, ei_out)) return rc;
  GUARD_BEGIN
  return model_maximize_ei<double>(model, starts, S, lo, hi, fmin_normalized, maxeval, x_out, ei_out, nevals_out);
  GUARD_END
}
int hbegp_maximize_ei_f32(hbegp_model* model, const float* starts, int S, const double* lo, const double* hi, double fmin_normalized,
                          int maxeval, float* x_out, double* ei_out, int* nevals_out) {
  if (int rc = check_maximize_ei<float>(model, starts, S, lo, hi, fmin_normalized, maxeval, x_out, ei_out)) return rc;
  GUARD_BEGIN
  return model_maximize_ei<float>(model, starts, S, lo, hi, fmin_normalized, maxeval, x_out, ei_out, nevals_out);
  GUARD_END
}

}  // extern "C"
// argument checks of the joint-posterior entry points: everything is refused before any device call
template <typename T>
static int check_posterior(hbegp_model* model, const T* Xs, int m, double jitter) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(HBEGP_EINVAL, "jitter must be finite and >= 0 (got %g)", jitter);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  if (m > 0 && !Xs) return fail(HBEGP_EINVAL, "Xs is NULL");
  const size_t cnt = (size_t)m * model->d;
  for (size_t i = 0; i < cnt; ++i)
    if (!std::isfinite((double)Xs[i]))
      return fail(HBEGP_EINVAL, "query point %d has a non-finite coordinate (feature %d)", (int)(i / model->d), (int)(i % model->d));
  return HBEGP_OK;
}
// the checks that need no model come first, so that each one has its own message whatever else is wrong
template <typename T>
static int check_sample(hbegp_model* model, const T* Xs, int m, const T* z, int S, double jitter, T* samples, int* argmin) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (m > 0 && !z) return fail(HBEGP_EINVAL, "z is NULL");
  if (!samples && !argmin) return fail(HBEGP_EINVAL, "samples and argmin are both NULL");
  return check_posterior<T>(model, Xs, m, jitter);
}
extern "C" {
int hbegp_predict_cov_f64(hbegp_model* model, const double* Xs, int m, double jitter, double* mean, double* cov) {
  if (int rc = check_posterior<double>(model, Xs, m, jitter)) return rc;
  if (m > 0 && !cov) return fail(HBEGP_EINVAL, "cov is NULL");
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_posterior<double>(model, Xs, m, jitter, mean, cov, nullptr, 0, nullptr, nullptr, nullptr);
  GUARD_END
}
int hbegp_predict_cov_f32(hbegp_model* model, const float* Xs, int m, double jitter, float* mean, float* cov) {
  if (int rc = check_posterior<float>(model, Xs, m, jitter)) return rc;
  if (m > 0 && !cov) return fail(HBEGP_EINVAL, "cov is NULL");
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_posterior<float>(model, Xs, m, jitter, mean, cov, nullptr, 0, nullptr, nullptr, nullptr);
  GUARD_END
}
int hbegp_sample_posterior_f64(hbegp_model* model, const double* Xs, int m, const double* z, int S, double jitter, double* samples,
                               int* argmin, int* info) {
  if (int rc = check_sample<double>(model, Xs, m, z, S, jitter, samples, argmin)) return rc;
  if (info) *info = 0;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_posterior<double>(model, Xs, m, jitter, nullptr, nullptr, z, S, samples, argmin, info);
  GUARD_END
}
int hbegp_sample_posterior_f32(hbegp_model* model, const float* Xs, int m, const float* z, int S, double jitter, float* samples,
                               int* argmin, int* info) {
  if (int rc = check_sample<float>(model, Xs, m, z, S, jitter, samples, argmin)) return rc;
  if (info) *info = 0;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_posterior<float>(model, Xs, m, jitter, nullptr, nullptr, z, S, samples, argmin, info);
  GUARD_END
}
}  // extern "C"
// argument checks of hbegp_qei_* / hbegp_maximize_qei_*: everything is refused before any device call, the checks that need no
// model first
template <typename T>
static int check_qei(hbegp_model* model, const T* Xb, int B, int q, const T* z, int S, double fmin, double jitter) {
  if (q < 1 || q > QEI_MAXQ) return fail(HBEGP_EINVAL, "q must be in [1, %d] (got %d)", QEI_MAXQ, q);
  if (B < 0) return fail(HBEGP_EINVAL, "B must be >= 0 (got %d)", B);
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (!z) return fail(HBEGP_EINVAL, "z is NULL");
  if (!std::isfinite(fmin)) return fail(HBEGP_EINVAL, "fmin must be finite (got %g)", fmin);
  if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(HBEGP_EINVAL, "jitter must be finite and >= 0 (got %g)", jitter);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  if (B > 0 && !Xb) return fail(HBEGP_EINVAL, "Xb is NULL");
  const size_t cnt = (size_t)B * q * model->d;
  for (size_t i = 0; i < cnt; ++i)
    if (!std::isfinite((double)Xb[i]))
      return fail(HBEGP_EINVAL, "query point %d has a non-finite coordinate (feature %d)", (int)(i / model->d), (int)(i % model->d));
  return HBEGP_OK;
}
template <typename T>
static int check_maximize_qei(hbegp_model* model, const T* starts, int R, int q, const double* lo, const double* hi, const T* z, int S,
                              double fmin, double jitter, int maxeval, T* x_out, double* qei_out) {
  if (R < 1) return fail(HBEGP_EINVAL, "R must be >= 1 (got %d)", R);
  if (maxeval < 1) return fail(HBEGP_EINVAL, "maxeval must be >= 1 (got %d)", maxeval);
  if (!starts || !lo || !hi || !x_out || !qei_out) return fail(HBEGP_EINVAL, "starts/lo/hi/x_out/qei_out is NULL");
  if (int rc = check_qei<T>(model, starts, R, q, z, S, fmin, jitter)) return rc;
  const int d = model->d;
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return fail(HBEGP_EINVAL, "lo[%d] > hi[%d] (%g > %g)", k, k, lo[k], hi[k]);
  for (int r = 0; r < R; ++r)
    for (int e = 0; e < q * d; ++e) {
      const double v = (double)starts[(size_t)r * q * d + e];
      if (!(v >= lo[e % d] && v <= hi[e % d]))
        return fail(HBEGP_EINVAL, "start %d lies outside the box (point %d, feature %d: %g)", r, e / d, e % d, v);
    }
  return HBEGP_OK;
}
extern "C" {
int hbegp_qei_f64(hbegp_model* model, const double* Xb, int B, int q, const double* z, int S, double fmin_normalized, double jitter,
                  double* qei, double* grad, int* info) {
  if (int rc = check_qei<double>(model, Xb, B, q, z, S, fmin_normalized, jitter)) return rc;
  if (B > 0 && !qei) return fail(HBEGP_EINVAL, "qei is NULL");
  if (B == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_qei<double>(model, Xb, B, q, z, S, fmin_normalized, jitter, qei, grad, info);
  GUARD_END
}
int hbegp_qei_f32(hbegp_model* model, const float* Xb, int B, int q, const float* z, int S, double fmin_normalized, double jitter,
                  double* qei, float* grad, int* info) {
  if (int rc = check_qei<float>(model, Xb, B, q, z, S, fmin_normalized, jitter)) return rc;
  if (B > 0 && !qei) return fail(HBEGP_EINVAL, "qei is NULL");
  if (B == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_qei<float>(model, Xb, B, q, z, S, fmin_normalized, jitter, qei, grad, info);
  GUARD_END
}
int hbegp_maximize_qei_f64(hbegp_model* model, const double* starts, int R, int q, const double* lo, const double* hi, const double* z,
                           int S, double fmin_normalized, double jitter, int maxeval, double* x_out, double* qei_out, int* nevals_out) {
  if (int rc = check_maximize_qei<double>(model, starts, R, q, lo, hi, z, S, fmin_normalized, jitter, maxeval, x_out, qei_out)) return rc;
  GUARD_BEGIN
  return model_maximize_qei<double>(model, starts, R, q, lo, hi, z, S, fmin_normalized, jitter, maxeval, x_out, qei_out, nevals_out);
  GUARD_END
}
int hbegp_maximize_qei_f32(hbegp_model* model, const float* starts, int R, int q, const double* lo, const double* hi, const float* z,
                           int S, double fmin_normalized, double jitter, int maxeval, float* x_out, double* qei_out, int* nevals_out) {
  if (int rc = check_maximize_qei<float>(model, starts, R, q, lo, hi, z, S, fmin_normalized, jitter, maxeval, x_out, qei_out)) return rc;
  GUARD_BEGIN
  return model_maximize_qei<float>(model, starts, R, q, lo, hi, z, S, fmin_normalized, jitter, maxeval, x_out, qei_out, nevals_out);
  GUARD_END
}
int hbegp_paths_create_f64(hbegp_model* model, const double* omega0, const double* phase, const double* w, const double* eps, int F, int S,
                           hbegp_paths** paths) {
  if (int rc = check_paths_create<double>(model, omega0, phase, w, F, S, paths)) return rc;
  GUARD_BEGIN
  return paths_create<double>(model, omega0, phase, w, eps, F, S, paths);
  GUARD_END
}
int hbegp_paths_create_f32(hbegp_model* model, const float* omega0, const float* phase, const float* w, const float* eps, int F, int S,
                           hbegp_paths** paths) {
  if (int rc = check_paths_create<float>(model, omega0, phase, w, F, S, paths)) return rc;
  GUARD_BEGIN
  return paths_create<float>(model, omega0, phase, w, eps, F, S, paths);
  GUARD_END
}
int hbegp_paths_eval_f64(hbegp_paths* paths, const double* Xs, int m, int per_path, double* f, double* df) {
  if (int rc = check_paths_eval<double>(paths, Xs, m, per_path, f)) return rc;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return paths_eval<double>(paths, Xs, m, per_path, f, df);
  GUARD_END
}
int hbegp_paths_eval_f32(hbegp_paths* paths, const float* Xs, int m, int per_path, float* f, float* df) {
  if (int rc = check_paths_eval<float>(paths, Xs, m, per_path, f)) return rc;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return paths_eval<float>(paths, Xs, m, per_path, f, df);
  GUARD_END
}
int hbegp_paths_minimize_f64(hbegp_paths* paths, const double* starts, int R, const double* lo, const double* hi, int maxeval,
                             double* x_best, double* f_best, int* n_evals) {
  if (int rc = check_paths_minimize<double>(paths, starts, R, lo, hi, maxeval, x_best, f_best)) return rc;
  GUARD_BEGIN
  return paths_minimize<double>(paths, starts, R, lo, hi, maxeval, x_best, f_best, n_evals);
  GUARD_END
}
int hbegp_paths_minimize_f32(hbegp_paths* paths, const float* starts, int R, const double* lo, const double* hi, int maxeval,
                             float* x_best, double* f_best, int* n_evals) {
  if (int rc = check_paths_minimize<float>(paths, starts, R, lo, hi, maxeval, x_best, f_best)) return rc;
  GUARD_BEGIN
  return paths_minimize<float>(paths, starts, R, lo, hi, maxeval, x_best, f_best, n_evals);
  GUARD_END
}
int hbegp_paths_info(const hbegp_paths* paths, int* n, int* d, int* n_features, int* n_paths, int* is_f32) {
  if (!paths) return fail(HBEGP_EINVAL, "NULL paths handle");
  if (n) *n = paths->model->n;
  if (d) *d = paths->model->d;
  if (n_features) *n_features = paths->F;
  if (n_paths) *n_paths = paths->S;
  if (is_f32) *is_f32 = paths->is_f32 ? 1 : 0;
  return HBEGP_OK;
}
void hbegp_paths_release(hbegp_paths* paths) { delete paths; }
int hbegp_debug_paths_phases(int enable, double* phase_ms) { return debug_phases(PH_PATHS, 3, enable, phase_ms); }
// The two size-dependent splits of the sample paths, as the engine itself computes them (host only, no device): the points per
// block of an evaluation of m points (paths_eval_locked calls the same function) and the feature chunks of the projection.
static int check_paths_sizes(int n, int F, int S) {
  if (n < 1) return fail(HBEGP_EINVAL, "n must be >= 1 (got %d)", n);
  if (F < 1 || F > HBEGP_PATHS_MAX_FEATURES) return fail(HBEGP_EINVAL, "F must be in [1, %d] (got %d)", HBEGP_PATHS_MAX_FEATURES, F);
  if (S < 1 || S > HBEGP_PATHS_MAX_PATHS) return fail(HBEGP_EINVAL, "S must be in [1, %d] (got %d)", HBEGP_PATHS_MAX_PATHS, S);
  return HBEGP_OK;
}
int hbegp_debug_paths_eval_blocks(int n, int d, int F, int S, int m, int* mb) {
  if (int rc = check_paths_sizes(n, F, S)) return rc;
  if (d < 1) return fail(HBEGP_EINVAL, "d must be >= 1 (got %d)", d);
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (!mb) return fail(HBEGP_EINVAL, "mb is NULL");
  *mb = paths_eval_block(n, d, F, S, m);
  return HBEGP_OK;
}
int hbegp_debug_paths_project_chunks(int F, int n, int S, int* cap, int* nch, int* fch) {
  if (int rc = check_paths_sizes(n, F, S)) return rc;
  int c = 0, f = 0;
  const int k = paths_project_chunks(F, n, S, &f, &c);
  if (cap) *cap = c;
  if (nch) *nch = k;
  if (fch) *fch = f;
  return HBEGP_OK;
}
// the check that needs no model comes first, so that each one has its own message whatever else is wrong
static int check_model_loo(hbegp_model* model, bool want_f32, bool any_output) {
  if (!any_output) return fail(HBEGP_EINVAL, "every output is NULL");
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != want_f32) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
int hbegp_model_loo_f64(hbegp_model* model, double* mean, double* var, double* lpd, double* loo, double* grad) {
  if (int rc = check_model_loo(model, false, mean || var || lpd || loo || grad)) return rc;
  GUARD_BEGIN
  return model_loo<double>(model, mean, var, lpd, loo, grad);
  GUARD_END
}
int hbegp_model_loo_f32(hbegp_model* model, float* mean, float* var, float* lpd, double* loo, double* grad) {
  if (int rc = check_model_loo(model, true, mean || var || lpd || loo || grad)) return rc;
  GUARD_BEGIN
  return model_loo<float>(model, mean, var, lpd, loo, grad);
  GUARD_END
}
int hbegp_debug_loo_phases(int enable, double* phase_ms) { return debug_phases(PH_LOO, 4, enable, phase_ms); }
int hbegp_model_lgo_f64(hbegp_model* model, const int* group, double* mean, double* var, double* lpd, int* n_groups, double* lgo,
                        double* grad) {
  if (int rc = check_model_loo(model, false, mean || var || lpd || n_groups || lgo || grad)) return rc;
  GUARD_BEGIN
  return model_lgo<double>(model, group, mean, var, lpd, n_groups, lgo, grad);
  GUARD_END
}
int hbegp_model_lgo_f32(hbegp_model* model, const int* group, float* mean, float* var, float* lpd, int* n_groups, double* lgo,
                        double* grad) {
  if (int rc = check_model_loo(model, true, mean || var || lpd || n_groups || lgo || grad)) return rc;
  GUARD_BEGIN
  return model_lgo<float>(model, group, mean, var, lpd, n_groups, lgo, grad);
  GUARD_END
}
int hbegp_debug_lgo_phases(int enable, double* phase_ms) { return debug_phases(PH_LGO, 4, enable, phase_ms); }
int hbegp_debug_qei_phases(int enable, double* phase_ms) { return debug_phases(PH_QEI, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_select_batch_*: everything is refused before any device call, the checks that need no model first
template <typename T>
static int check_select(hbegp_model* model, const T* Xs, int m, int k, double fmin, const double* lie, int* idx) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (k < 0) return fail(HBEGP_EINVAL, "k must be >= 0 (got %d)", k);
  if (k > m) return fail(HBEGP_EINVAL, "k must be <= m (got k = %d, m = %d)", k, m);
  if (k > 0 && !idx) return fail(HBEGP_EINVAL, "idx is NULL");
  if (!std::isfinite(fmin)) return fail(HBEGP_EINVAL, "fmin must be finite (got %g)", fmin);
  if (lie && !std::isfinite(*lie)) return fail(HBEGP_EINVAL, "the lie must be finite (got %g)", *lie);
  return check_posterior<T>(model, Xs, m, 0.0);
}
extern "C" {
int hbegp_select_batch_f64(hbegp_model* model, const double* Xs, int m, int k, double fmin_normalized, const double* lie, int* idx,
                           double* ei, double* mean_out, double* var_out) {
  if (int rc = check_select<double>(model, Xs, m, k, fmin_normalized, lie, idx)) return rc;
  if (k == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_select_batch<double>(model, Xs, m, k, fmin_normalized, lie, idx, ei, mean_out, var_out);
  GUARD_END
}
int hbegp_select_batch_f32(hbegp_model* model, const float* Xs, int m, int k, double fmin_normalized, const double* lie, int* idx,
                           double* ei, float* mean_out, float* var_out) {
  if (int rc = check_select<float>(model, Xs, m, k, fmin_normalized, lie, idx)) return rc;
  if (k == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_select_batch<float>(model, Xs, m, k, fmin_normalized, lie, idx, ei, mean_out, var_out);
  GUARD_END
}
int hbegp_debug_batch_select_phases(int enable, double* phase_ms) { return debug_phases(PH_SELECT, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_knowledge_gradient_*: everything is refused before any device call, the checks that need no model first
template <typename T>
static int check_kg(hbegp_model* model, const T* Xs, int m, int mc, const double* kg) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (mc < 0) return fail(HBEGP_EINVAL, "mc must be >= 0 (got %d)", mc);
  if (mc > m) return fail(HBEGP_EINVAL, "mc must be <= m (got mc = %d, m = %d)", mc, m);
  if (mc > 0 && !kg) return fail(HBEGP_EINVAL, "kg is NULL");
  return check_posterior<T>(model, Xs, m, 0.0);
}
extern "C" {
int hbegp_knowledge_gradient_f64(hbegp_model* model, const double* Xs, int m, int mc, double* kg, int* best, int* imin, double* mean_out,
                                 double* var_out) {
  if (int rc = check_kg<double>(model, Xs, m, mc, kg)) return rc;
  if (best) *best = -1;
  if (imin) *imin = -1;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_knowledge_gradient<double>(model, Xs, m, mc, kg, best, imin, mean_out, var_out);
  GUARD_END
}
int hbegp_knowledge_gradient_f32(hbegp_model* model, const float* Xs, int m, int mc, double* kg, int* best, int* imin, float* mean_out,
                                 float* var_out) {
  if (int rc = check_kg<float>(model, Xs, m, mc, kg)) return rc;
  if (best) *best = -1;
  if (imin) *imin = -1;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_knowledge_gradient<float>(model, Xs, m, mc, kg, best, imin, mean_out, var_out);
  GUARD_END
}
int hbegp_debug_kg_phases(int enable, double* phase_ms) { return debug_phases(PH_KG, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_noisy_ei_*: everything is refused before any device call, the checks that need no model first
template <typename T>
static int check_nei(hbegp_model* model, const T* Xs, int m, int mb, const T* z, int S, double jitter, const double* nei) {
  if (m < 1) return fail(HBEGP_EINVAL, "m must be >= 1 (got %d): without a baseline there is no incumbent", m);
  if (mb < 1) return fail(HBEGP_EINVAL, "mb must be >= 1 (got %d)", mb);
  if (mb > m) return fail(HBEGP_EINVAL, "mb must be <= m (got mb = %d, m = %d)", mb, m);
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (!z) return fail(HBEGP_EINVAL, "z is NULL");
  if (m > mb && !nei) return fail(HBEGP_EINVAL, "nei is NULL");
  return check_posterior<T>(model, Xs, m, jitter);
}
extern "C" {
int hbegp_noisy_ei_f64(hbegp_model* model, const double* Xs, int m, int mb, const double* z, int S, double jitter, double* nei, int* best,
                       double* fmin_draws, double* rho, int* info) {
  if (int rc = check_nei<double>(model, Xs, m, mb, z, S, jitter, nei)) return rc;
  GUARD_BEGIN
  return model_noisy_ei<double>(model, Xs, m, mb, z, S, jitter, nei, best, fmin_draws, rho, info);
  GUARD_END
}
int hbegp_noisy_ei_f32(hbegp_model* model, const float* Xs, int m, int mb, const float* z, int S, double jitter, double* nei, int* best,
                       double* fmin_draws, double* rho, int* info) {
  if (int rc = check_nei<float>(model, Xs, m, mb, z, S, jitter, nei)) return rc;
  GUARD_BEGIN
  return model_noisy_ei<float>(model, Xs, m, mb, z, S, jitter, nei, best, fmin_draws, rho, info);
  GUARD_END
}
int hbegp_debug_nei_phases(int enable, double* phase_ms) { return debug_phases(PH_NEI, 4, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_ehvi_* / hbegp_maximize_ehvi_*: everything is refused before any device call, the checks that need no
// model first
template <typename T>
static int check_ehvi_models(hbegp_model* const* models, int n_obj, const double* front, int P, const double* ref) {
  if (n_obj != 2) return fail(HBEGP_EINVAL, "n_obj must be 2 (got %d)", n_obj);
  if (P < 0) return fail(HBEGP_EINVAL, "P must be >= 0 (got %d)", P);
  if (!models) return fail(HBEGP_EINVAL, "models is NULL");
  if (!models[0] || !models[1]) return fail(HBEGP_EINVAL, "NULL model");
  if (models[0] == models[1]) return fail(HBEGP_EINVAL, "the same model was passed for both objectives");
  for (int k = 0; k < 2; ++k)
    if (models[k]->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model %d holds %s data", k, models[k]->is_f32 ? "f32" : "f64");
  if (models[0]->d != models[1]->d) return fail(HBEGP_EINVAL, "the models differ in d (%d and %d)", models[0]->d, models[1]->d);
  if (models[0]->dev != models[1]->dev)
    return fail(HBEGP_EINVAL, "the models live on different devices (%d and %d)", models[0]->dev, models[1]->dev);
  if (!ref) return fail(HBEGP_EINVAL, "ref is NULL");
  if (P > 0 && !front) return fail(HBEGP_EINVAL, "front is NULL");
  if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) return fail(HBEGP_EINVAL, "non-finite reference point");
  for (size_t i = 0; i < 2 * (size_t)P; ++i)
    if (!std::isfinite(front[i])) return fail(HBEGP_EINVAL, "non-finite front value (point %d)", (int)(i / 2));
  return HBEGP_OK;
}
template <typename T>
static int do_ehvi(hbegp_model* const* models, int n_obj, const T* Xs, int m, const double* front, int P, const double* ref, double* ehvi,
                   T* grad, int* best, T* mean, T* var) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (int rc = check_ehvi_models<T>(models, n_obj, front, P, ref)) return rc;
  if (m > 0 && (!Xs || !ehvi)) return fail(HBEGP_EINVAL, "Xs/ehvi is NULL");
  if (best) *best = -1;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  std::vector<double> thr;
  const int ns = ehvi_thresholds(front, P, ref, &thr);
  JoinEvents join(models[0]->dev, 1);
  return model_ehvi<T>(models, Xs, m, thr, ns, join, ehvi, grad, best, mean, var);
  GUARD_END
}
template <typename T>
static int do_maximize_ehvi(hbegp_model* const* models, int n_obj, const T* starts, int S, const double* lo, const double* hi,
                            const double* front, int P, const double* ref, int maxeval, T* x_out, double* ehvi_out, int* nevals_out) {
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (int rc = check_ehvi_models<T>(models, n_obj, front, P, ref)) return rc;
  if (int rc = check_maximize_ei<T>(models[0], starts, S, lo, hi, 0.0, maxeval, x_out, ehvi_out)) return rc;
  GUARD_BEGIN
  std::vector<double> thr;
  const int ns = ehvi_thresholds(front, P, ref, &thr);
  JoinEvents join(models[0]->dev, 1);
  return maximize_marginal<T>(
      starts, S, models[0]->d, lo, hi, maxeval,
      [&](const T* xs, int cnt, double* val, T* gr) { return model_ehvi<T>(models, xs, cnt, thr, ns, join, val, gr, nullptr, nullptr, nullptr); },
      x_out, ehvi_out, nevals_out);
  GUARD_END
}
extern "C" {
int hbegp_ehvi_f64(hbegp_model* const* models, int n_obj, const double* Xs, int m, const double* front, int P, const double* ref,
                   double* ehvi, double* grad, int* best, double* mean, double* var) {
  return do_ehvi<double>(models, n_obj, Xs, m, front, P, ref, ehvi, grad, best, mean, var);
}
int hbegp_ehvi_f32(hbegp_model* const* models, int n_obj, const float* Xs, int m, const double* front, int P, const double* ref,
                   double* ehvi, float* grad, int* best, float* mean, float* var) {
  return do_ehvi<float>(models, n_obj, Xs, m, front, P, ref, ehvi, grad, best, mean, var);
}
int hbegp_maximize_ehvi_f64(hbegp_model* const* models, int n_obj, const double* starts, int S, const double* lo, const double* hi,
                            const double* front, int P, const double* ref, int maxeval, double* x_out, double* ehvi_out, int* nevals_out) {
  return do_maximize_ehvi<double>(models, n_obj, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals_out);
}
int hbegp_maximize_ehvi_f32(hbegp_model* const* models, int n_obj, const float* starts, int S, const double* lo, const double* hi,
                            const double* front, int P, const double* ref, int maxeval, float* x_out, double* ehvi_out, int* nevals_out) {
  return do_maximize_ehvi<float>(models, n_obj, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals_out);
}
int hbegp_debug_ehvi_phases(int enable, double* phase_ms) { return debug_phases(PH_EHVI, 3, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_ehvi_nd_* / hbegp_maximize_ehvi_nd_* / hbegp_debug_ehvi_boxes that need no model
static int check_ehvi_nd_front(int n_obj, const double* front, int P, const double* ref) {
  if (n_obj < 2 || n_obj > EHVI_ND_MAX_OBJ) return fail(HBEGP_EINVAL, "n_obj must be 2, 3 or 4 (got %d)", n_obj);
  if (P < 0) return fail(HBEGP_EINVAL, "P must be >= 0 (got %d)", P);
  if (!ref) return fail(HBEGP_EINVAL, "ref is NULL");
  if (P > 0 && !front) return fail(HBEGP_EINVAL, "front is NULL");
  for (int k = 0; k < n_obj; ++k)
    if (!std::isfinite(ref[k])) return fail(HBEGP_EINVAL, "non-finite reference point");
  for (size_t i = 0; i < (size_t)n_obj * (size_t)P; ++i)
    if (!std::isfinite(front[i])) return fail(HBEGP_EINVAL, "non-finite front value (point %d)", (int)(i / (size_t)n_obj));
  return HBEGP_OK;
}
// the checks of the models, as check_ehvi_models' with n_obj of them
template <typename T>
static int check_ehvi_nd_models(hbegp_model* const* models, int n_obj) {
  if (!models) return fail(HBEGP_EINVAL, "models is NULL");
  for (int k = 0; k < n_obj; ++k)
    if (!models[k]) return fail(HBEGP_EINVAL, "NULL model");
  for (int k = 0; k < n_obj; ++k)
    for (int i = 0; i < k; ++i)
      if (models[i] == models[k]) return fail(HBEGP_EINVAL, "the same model was passed for objectives %d and %d", i, k);
  for (int k = 0; k < n_obj; ++k)
    if (models[k]->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model %d holds %s data", k, models[k]->is_f32 ? "f32" : "f64");
  for (int k = 1; k < n_obj; ++k) {
    if (models[0]->d != models[k]->d) return fail(HBEGP_EINVAL, "the models differ in d (%d and %d)", models[0]->d, models[k]->d);
    if (models[0]->dev != models[k]->dev)
      return fail(HBEGP_EINVAL, "the models live on different devices (%d and %d)", models[0]->dev, models[k]->dev);
  }
  return HBEGP_OK;
}
// Everything is refused before any device call: the arguments that need no model, then the front's decomposition (ENOMEM past the
// box cap), then the models.
template <typename T>
static int do_ehvi_nd(hbegp_model* const* models, int n_obj, const T* Xs, int m, const double* front, int P, const double* ref,
                      double* ehvi, T* grad, int* best, T* mean, T* var) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (int rc = check_ehvi_nd_front(n_obj, front, P, ref)) return rc;
  GUARD_BEGIN
  EhviNdPlan plan;
  if (int rc = ehvi_nd_plan(front, P, n_obj, ref, &plan)) return rc;
  if (int rc = check_ehvi_nd_models<T>(models, n_obj)) return rc;
  if (m > 0 && (!Xs || !ehvi)) return fail(HBEGP_EINVAL, "Xs/ehvi is NULL");
  if (best) *best = -1;
  if (m == 0) return HBEGP_OK;
  const EhviNdUpload up(plan);
  JoinEvents join(models[0]->dev, n_obj - 1);
  return model_ehvi_nd<T>(models, Xs, m, up, join, ehvi, grad, best, mean, var);
  GUARD_END
}
template <typename T>
static int do_maximize_ehvi_nd(hbegp_model* const* models, int n_obj, const T* starts, int S, const double* lo, const double* hi,
                               const double* front, int P, const double* ref, int maxeval, T* x_out, double* ehvi_out, int* nevals_out) {
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (int rc = check_ehvi_nd_front(n_obj, front, P, ref)) return rc;
  GUARD_BEGIN
  EhviNdPlan plan;
  if (int rc = ehvi_nd_plan(front, P, n_obj, ref, &plan)) return rc;
  if (int rc = check_ehvi_nd_models<T>(models, n_obj)) return rc;
  if (int rc = check_maximize_ei<T>(models[0], starts, S, lo, hi, 0.0, maxeval, x_out, ehvi_out)) return rc;
  const EhviNdUpload up(plan);
  JoinEvents join(models[0]->dev, n_obj - 1);
  return maximize_marginal<T>(
      starts, S, models[0]->d, lo, hi, maxeval,
      [&](const T* xs, int cnt, double* val, T* gr) { return model_ehvi_nd<T>(models, xs, cnt, up, join, val, gr, nullptr, nullptr, nullptr); },
      x_out, ehvi_out, nevals_out);
  GUARD_END
}
extern "C" {
int hbegp_ehvi_nd_f64(hbegp_model* const* models, int n_obj, const double* Xs, int m, const double* front, int P, const double* ref,
                      double* ehvi, double* grad, int* best, double* mean, double* var) {
  return do_ehvi_nd<double>(models, n_obj, Xs, m, front, P, ref, ehvi, grad, best, mean, var);
}
int hbegp_ehvi_nd_f32(hbegp_model* const* models, int n_obj, const float* Xs, int m, const double* front, int P, const double* ref,
                      double* ehvi, float* grad, int* best, float* mean, float* var) {
  return do_ehvi_nd<float>(models, n_obj, Xs, m, front, P, ref, ehvi, grad, best, mean, var);
}
int hbegp_maximize_ehvi_nd_f64(hbegp_model* const* models, int n_obj, const double* starts, int S, const double* lo, const double* hi,
                               const double* front, int P, const double* ref, int maxeval, double* x_out, double* ehvi_out,
                               int* nevals_out) {
  return do_maximize_ehvi_nd<double>(models, n_obj, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals_out);
}
int hbegp_maximize_ehvi_nd_f32(hbegp_model* const* models, int n_obj, const float* starts, int S, const double* lo, const double* hi,
                               const double* front, int P, const double* ref, int maxeval, float* x_out, double* ehvi_out,
                               int* nevals_out) {
  return do_maximize_ehvi_nd<float>(models, n_obj, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals_out);
}
int hbegp_debug_ehvi_nd_phases(int enable, double* phase_ms) { return debug_phases(PH_EHVI_ND, 5, enable, phase_ms); }
int hbegp_debug_ehvi_boxes(const double* front, int P, int n_obj, const double* ref, int* thr_count, double* thr, int thr_cap, int* n_boxes,
                           int* boxes, int box_cap) {
  if (int rc = check_ehvi_nd_front(n_obj, front, P, ref)) return rc;
  if (thr_cap < 0 || box_cap < 0) return fail(HBEGP_EINVAL, "thr_cap and box_cap must be >= 0 (got %d and %d)", thr_cap, box_cap);
  if (!thr_count || !n_boxes) return fail(HBEGP_EINVAL, "thr_count/n_boxes is NULL");
  if ((thr_cap > 0 && !thr) || (box_cap > 0 && !boxes)) return fail(HBEGP_EINVAL, "thr/boxes is NULL with a cap > 0");
  GUARD_BEGIN
  EhviNdPlan plan;
  if (int rc = ehvi_nd_plan(front, P, n_obj, ref, &plan)) return rc;
  size_t nt = 0;
  for (int k = 0; k < n_obj; ++k) {
    thr_count[k] = (int)plan.thr[k].size();
    nt += plan.thr[k].size();
  }
  *n_boxes = (int)plan.n_boxes;
  if (thr_cap == 0 && box_cap == 0) return HBEGP_OK;
  if ((size_t)thr_cap < nt || (size_t)box_cap < plan.n_boxes)
    return fail(HBEGP_EINVAL, "the caps (%d thresholds, %d boxes) are below the counts (%d, %d)", thr_cap, box_cap, (int)nt, (int)plan.n_boxes);
  for (int k = 0; k < n_obj; ++k) thr = std::copy(plan.thr[k].begin(), plan.thr[k].end(), thr);
  std::copy(plan.boxes.begin(), plan.boxes.end(), boxes);
  return HBEGP_OK;
  GUARD_END
}
}  // extern "C"

// argument checks of hbegp_constrained_ei_* / hbegp_maximize_constrained_ei_*: everything is refused before any device call, the
// checks that need no model first.  On success M = (objective, constraints ..) and thr = (fmin, limits ..).
template <typename T>
static int check_cei_models(hbegp_model* objective, hbegp_model* const* constraints, int n_con, double fmin, const double* limits,
                            std::vector<hbegp_model*>* M, std::vector<double>* thr) {
  if (n_con < 0 || n_con > HBEGP_CEI_MAX_CONSTRAINTS)
    return fail(HBEGP_EINVAL, "n_con must lie in [0, %d] (got %d)", HBEGP_CEI_MAX_CONSTRAINTS, n_con);
  if (std::isnan(fmin) || fmin == -std::numeric_limits<double>::infinity())
    return fail(HBEGP_EINVAL, "fmin_normalized must be finite or +inf (got %g)", fmin);
  if (n_con == 0 && std::isinf(fmin)) return fail(HBEGP_EINVAL, "n_con = 0 with fmin_normalized = +inf: nothing to compute");
  if (!objective) return fail(HBEGP_EINVAL, "NULL objective");
  if (n_con > 0 && (!constraints || !limits)) return fail(HBEGP_EINVAL, "constraints/limits is NULL");
  M->assign(1, objective);
  thr->assign(1, fmin);
  for (int k = 0; k < n_con; ++k) {
    if (!constraints[k]) return fail(HBEGP_EINVAL, "NULL model (constraint %d)", k);
    for (hbegp_model* seen : *M)
      if (seen == constraints[k])
        return fail(HBEGP_EINVAL, seen == objective ? "constraint %d is the objective's model" : "the same model was passed twice (constraint %d)", k);
    M->push_back(constraints[k]);
  }
  for (int k = 0; k <= n_con; ++k)
    if ((*M)[k]->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model %d holds %s data", k, (*M)[k]->is_f32 ? "f32" : "f64");
  for (int k = 1; k <= n_con; ++k) {
    if ((*M)[k]->d != objective->d) return fail(HBEGP_EINVAL, "the models differ in d (%d and %d)", objective->d, (*M)[k]->d);
    if ((*M)[k]->dev != objective->dev)
      return fail(HBEGP_EINVAL, "the models live on different devices (%d and %d)", objective->dev, (*M)[k]->dev);
  }
  for (int k = 0; k < n_con; ++k) {
    if (!std::isfinite(limits[k])) return fail(HBEGP_EINVAL, "non-finite limit (constraint %d)", k);
    thr->push_back(limits[k]);
  }
  return HBEGP_OK;
}
template <typename T>
static int do_cei(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const T* Xs, int m, double fmin, const double* limits,
                  double* cei, T* grad, int* best, double* ei, double* pof, T* mean, T* var, bool log_space = false) {
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  GUARD_BEGIN
  std::vector<hbegp_model*> M;
  std::vector<double> thr;
  if (int rc = check_cei_models<T>(objective, constraints, n_con, fmin, limits, &M, &thr)) return rc;
  if (m > 0 && (!Xs || !cei)) return fail(HBEGP_EINVAL, log_space ? "Xs/lcei is NULL" : "Xs/cei is NULL");
  if (best) *best = -1;
  if (m == 0) return HBEGP_OK;
  JoinEvents join(objective->dev, n_con);
  return model_constrained_ei<T>(M.data(), 1 + n_con, Xs, m, thr.data(), join, cei, grad, best, ei, pof, mean, var, log_space);
  GUARD_END
}
template <typename T>
static int do_maximize_cei(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const T* starts, int S, const double* lo,
                           const double* hi, double fmin, const double* limits, int maxeval, T* x_out, double* cei_out, int* nevals_out,
                           bool log_space = false) {
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  GUARD_BEGIN
  std::vector<hbegp_model*> M;
  std::vector<double> thr;
  if (int rc = check_cei_models<T>(objective, constraints, n_con, fmin, limits, &M, &thr)) return rc;
  if (int rc = check_maximize_ei<T>(objective, starts, S, lo, hi, 0.0, maxeval, x_out, cei_out)) return rc;
  JoinEvents join(objective->dev, n_con);
  return maximize_marginal<T>(
      starts, S, objective->d, lo, hi, maxeval,
      [&](const T* xs, int cnt, double* val, T* gr) {
        return model_constrained_ei<T>(M.data(), 1 + n_con, xs, cnt, thr.data(), join, val, gr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       log_space);
      },
      x_out, cei_out, nevals_out);
  GUARD_END
}
extern "C" {
int hbegp_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* Xs, int m,
                             double fmin_normalized, const double* limits, double* cei, double* grad, int* best, double* ei, double* pof,
                             double* mean, double* var) {
  return do_cei<double>(objective, constraints, n_con, Xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var);
}
int hbegp_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* Xs, int m,
                             double fmin_normalized, const double* limits, double* cei, float* grad, int* best, double* ei, double* pof,
                             float* mean, float* var) {
  return do_cei<float>(objective, constraints, n_con, Xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var);
}
int hbegp_maximize_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* starts, int S,
                                      const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                      double* x_out, double* cei_out, int* nevals_out) {
  return do_maximize_cei<double>(objective, constraints, n_con, starts, S, lo, hi, fmin_normalized, limits, maxeval, x_out, cei_out,
                                 nevals_out);
}
int hbegp_maximize_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* starts, int S,
                                      const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                      float* x_out, double* cei_out, int* nevals_out) {
  return do_maximize_cei<float>(objective, constraints, n_con, starts, S, lo, hi, fmin_normalized, limits, maxeval, x_out, cei_out,
                                nevals_out);
}
int hbegp_debug_cei_phases(int enable, double* phase_ms) { return debug_phases(PH_CEI, 2, enable, phase_ms); }
int hbegp_log_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* Xs, int m,
                                 double fmin_normalized, const double* limits, double* lcei, double* grad, int* best, double* lei,
                                 double* lpof, double* mean, double* var) {
  return do_cei<double>(objective, constraints, n_con, Xs, m, fmin_normalized, limits, lcei, grad, best, lei, lpof, mean, var, true);
}
int hbegp_log_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* Xs, int m,
                                 double fmin_normalized, const double* limits, double* lcei, float* grad, int* best, double* lei,
                                 double* lpof, float* mean, float* var) {
  return do_cei<float>(objective, constraints, n_con, Xs, m, fmin_normalized, limits, lcei, grad, best, lei, lpof, mean, var, true);
}
int hbegp_maximize_log_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* starts, int S,
                                          const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                          double* x_out, double* lcei_out, int* nevals_out) {
  return do_maximize_cei<double>(objective, constraints, n_con, starts, S, lo, hi, fmin_normalized, limits, maxeval, x_out, lcei_out,
                                 nevals_out, true);
}
int hbegp_maximize_log_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* starts, int S,
                                          const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                          float* x_out, double* lcei_out, int* nevals_out) {
  return do_maximize_cei<float>(objective, constraints, n_con, starts, S, lo, hi, fmin_normalized, limits, maxeval, x_out, lcei_out,
                                nevals_out, true);
}
int hbegp_debug_lcei_phases(int enable, double* phase_ms) { return debug_phases(PH_LCEI, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_mes_* / hbegp_maximize_mes_*: everything is refused before any device call
template <typename T>
static int check_mes(hbegp_model* model, const double* ystar, int S) {
  if (S < 1 || S > HBEGP_MES_MAX_SAMPLES) return fail(HBEGP_EINVAL, "S must lie in [1, %d] (got %d)", HBEGP_MES_MAX_SAMPLES, S);
  if (!ystar) return fail(HBEGP_EINVAL, "ystar is NULL");
  for (int s = 0; s < S; ++s)
    if (!std::isfinite(ystar[s])) return fail(HBEGP_EINVAL, "ystar[%d] is not finite", s);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
template <typename T>
static int do_mes(hbegp_model* model, const T* Xs, int m, const double* ystar, int S, double* mes, T* grad, int* best, T* mean, T* var) {
  if (int rc = check_mes<T>(model, ystar, S)) return rc;
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (m > 0 && (!Xs || !mes)) return fail(HBEGP_EINVAL, "Xs/mes is NULL");
  if (best) *best = -1;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_mes<T>(model, Xs, m, ystar, S, mes, grad, best, mean, var);
  GUARD_END
}
template <typename T>
static int do_maximize_mes(hbegp_model* model, const T* starts, int R, const double* lo, const double* hi, const double* ystar, int S,
                           int maxeval, T* x_out, double* mes_out, int* nevals_out) {
  if (R < 1) return fail(HBEGP_EINVAL, "R must be >= 1 (got %d)", R);
  if (int rc = check_mes<T>(model, ystar, S)) return rc;
  if (int rc = check_maximize_ei<T>(model, starts, R, lo, hi, 0.0, maxeval, x_out, mes_out)) return rc;
  GUARD_BEGIN
  return maximize_marginal<T>(
      starts, R, model->d, lo, hi, maxeval,
      [&](const T* xs, int cnt, double* val, T* gr) { return model_mes<T>(model, xs, cnt, ystar, S, val, gr, nullptr, nullptr, nullptr); }, x_out,
      mes_out, nevals_out);
  GUARD_END
}
extern "C" {
int hbegp_mes_f64(hbegp_model* model, const double* Xs, int m, const double* ystar, int S, double* mes, double* grad, int* best,
                  double* mean, double* var) {
  return do_mes<double>(model, Xs, m, ystar, S, mes, grad, best, mean, var);
}
int hbegp_mes_f32(hbegp_model* model, const float* Xs, int m, const double* ystar, int S, double* mes, float* grad, int* best, float* mean,
                  float* var) {
  return do_mes<float>(model, Xs, m, ystar, S, mes, grad, best, mean, var);
}
int hbegp_maximize_mes_f64(hbegp_model* model, const double* starts, int R, const double* lo, const double* hi, const double* ystar, int S,
                           int maxeval, double* x_out, double* mes_out, int* nevals_out) {
  return do_maximize_mes<double>(model, starts, R, lo, hi, ystar, S, maxeval, x_out, mes_out, nevals_out);
}
int hbegp_maximize_mes_f32(hbegp_model* model, const float* starts, int R, const double* lo, const double* hi, const double* ystar, int S,
                           int maxeval, float* x_out, double* mes_out, int* nevals_out) {
  return do_maximize_mes<float>(model, starts, R, lo, hi, ystar, S, maxeval, x_out, mes_out, nevals_out);
}
int hbegp_debug_mes_phases(int enable, double* phase_ms) { return debug_phases(PH_MES, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_confidence_bound_* / hbegp_minimize_confidence_bound_*: everything is refused before any device call,
// the checks that need no model first, so that each one has its own message whatever else is wrong
template <typename T>
static int check_cb_model(hbegp_model* model) {
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
template <typename T>
static int do_cb(hbegp_model* model, const T* Xs, int m, double kappa, double* cb, T* grad, int* best, T* mean, T* var) {
  if (!std::isfinite(kappa)) return fail(HBEGP_EINVAL, "kappa is not finite");
  if (m < 0) return fail(HBEGP_EINVAL, "m must be >= 0 (got %d)", m);
  if (m > 0 && (!Xs || !cb)) return fail(HBEGP_EINVAL, "Xs/cb is NULL");
  if (int rc = check_cb_model<T>(model)) return rc;
  if (best) *best = -1;
  if (m == 0) return HBEGP_OK;
  GUARD_BEGIN
  return model_cb<T>(model, Xs, m, kappa, cb, grad, best, mean, var);
  GUARD_END
}
// hbegp_maximize_ei_*'s checks of S, the box, maxeval and the outputs (the box's order and the starts' places need the model's d, so
// they follow the model's check); a start has to lie inside the box unless one of its coordinates is a NaN (that run fails alone:
// minimize_marginal)
template <typename T>
static int do_minimize_cb(hbegp_model* model, const T* starts, int S, const double* lo, const double* hi, double kappa, int maxeval, T* x_out,
                          double* cb_out, int* nevals_out) {
  if (S < 1) return fail(HBEGP_EINVAL, "S must be >= 1 (got %d)", S);
  if (!std::isfinite(kappa)) return fail(HBEGP_EINVAL, "kappa is not finite");
  if (!starts || !lo || !hi || !x_out || !cb_out) return fail(HBEGP_EINVAL, "starts/lo/hi/x_out/cb_out is NULL");
  if (maxeval < 1) return fail(HBEGP_EINVAL, "maxeval must be >= 1 (got %d)", maxeval);
  if (int rc = check_cb_model<T>(model)) return rc;
  const int d = model->d;
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return fail(HBEGP_EINVAL, "lo[%d] > hi[%d] (%g > %g)", k, k, lo[k], hi[k]);
  for (int r = 0; r < S; ++r)
    for (int k = 0; k < d; ++k) {
      const double v = (double)starts[(size_t)r * d + k];
      if (v < lo[k] || v > hi[k]) return fail(HBEGP_EINVAL, "start %d lies outside the box (feature %d: %g)", r, k, v);
    }
  GUARD_BEGIN
  return minimize_marginal<T>(
      starts, S, d, lo, hi, maxeval,
      [&](const T* xs, int cnt, double* val, T* gr) { return model_cb<T>(model, xs, cnt, kappa, val, gr, nullptr, nullptr, nullptr); }, x_out,
      cb_out, nevals_out);
  GUARD_END
}
extern "C" {
int hbegp_confidence_bound_f64(hbegp_model* model, const double* Xs, int m, double kappa, double* cb, double* grad, int* best, double* mean,
                               double* var) {
  return do_cb<double>(model, Xs, m, kappa, cb, grad, best, mean, var);
}
int hbegp_confidence_bound_f32(hbegp_model* model, const float* Xs, int m, double kappa, double* cb, float* grad, int* best, float* mean,
                               float* var) {
  return do_cb<float>(model, Xs, m, kappa, cb, grad, best, mean, var);
}
int hbegp_minimize_confidence_bound_f64(hbegp_model* model, const double* starts, int S, const double* lo, const double* hi, double kappa,
                                        int maxeval, double* x_out, double* cb_out, int* nevals_out) {
  return do_minimize_cb<double>(model, starts, S, lo, hi, kappa, maxeval, x_out, cb_out, nevals_out);
}
int hbegp_minimize_confidence_bound_f32(hbegp_model* model, const float* starts, int S, const double* lo, const double* hi, double kappa,
                                        int maxeval, float* x_out, double* cb_out, int* nevals_out) {
  return do_minimize_cb<float>(model, starts, S, lo, hi, kappa, maxeval, x_out, cb_out, nevals_out);
}
int hbegp_debug_cb_phases(int enable, double* phase_ms) { return debug_phases(PH_CB, 2, enable, phase_ms); }
}  // extern "C"

// argument checks of hbegp_sobol_* / hbegp_main_effects_*: everything is refused before any device call, the checks that need no
// model first.  The sample rows are not screened: a NaN coordinate propagates to that row's values (include/hbegp.h).
static int check_sens(hbegp_model* model, bool want_f32, const void* A, const void* second, const char* second_name, int N, int min_n,
                      const void* out1, const char* out1_name, const void* out2, const char* out2_name) {
  if (N < min_n) return fail(HBEGP_EINVAL, "N must be >= %d (got %d)", min_n, N);
  if (!A) return fail(HBEGP_EINVAL, "A is NULL");
  if (!second) return fail(HBEGP_EINVAL, "%s is NULL", second_name);
  if (!out1) return fail(HBEGP_EINVAL, "%s is NULL", out1_name);
  if (!out2) return fail(HBEGP_EINVAL, "%s is NULL", out2_name);
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (model->is_f32 != want_f32) return fail(HBEGP_EINVAL, "model holds %s data", model->is_f32 ? "f32" : "f64");
  return HBEGP_OK;
}
extern "C" {
int hbegp_sobol_f64(hbegp_model* model, const double* A, const double* B, int N, double* first, double* total, double* f0, double* variance,
                    double* f_a, double* f_b, double* f_ab) {
  if (int rc = check_sens(model, false, A, B, "B", N, 2, first, "first", total, "total")) return rc;
  GUARD_BEGIN
  return model_sensitivity<double>(model, A, B, N, nullptr, 0, first, total, f0, variance, f_a, f_b, f_ab, nullptr);
  GUARD_END
}
int hbegp_sobol_f32(hbegp_model* model, const float* A, const float* B, int N, double* first, double* total, double* f0, double* variance,
                    float* f_a, float* f_b, float* f_ab) {
  if (int rc = check_sens(model, true, A, B, "B", N, 2, first, "first", total, "total")) return rc;
  GUARD_BEGIN
  return model_sensitivity<float>(model, A, B, N, nullptr, 0, first, total, f0, variance, f_a, f_b, f_ab, nullptr);
  GUARD_END
}
int hbegp_main_effects_f64(hbegp_model* model, const double* A, int N, const double* grid, int G, double* effect, double* f_a) {
  if (G < 1) return fail(HBEGP_EINVAL, "G must be >= 1 (got %d)", G);
  if (int rc = check_sens(model, false, A, grid, "grid", N, 1, effect, "effect", effect, "effect")) return rc;
  GUARD_BEGIN
  return model_sensitivity<double>(model, A, nullptr, N, grid, G, nullptr, nullptr, nullptr, nullptr, f_a, nullptr, nullptr, effect);
  GUARD_END
}
int hbegp_main_effects_f32(hbegp_model* model, const float* A, int N, const float* grid, int G, double* effect, float* f_a) {
  if (G < 1) return fail(HBEGP_EINVAL, "G must be >= 1 (got %d)", G);
  if (int rc = check_sens(model, true, A, grid, "grid", N, 1, effect, "effect", effect, "effect")) return rc;
  GUARD_BEGIN
  return model_sensitivity<float>(model, A, nullptr, N, grid, G, nullptr, nullptr, nullptr, nullptr, f_a, nullptr, nullptr, effect);
  GUARD_END
}
int hbegp_debug_sens_phases(int enable, double* phase_ms) { return debug_phases(PH_SENS, 4, enable, phase_ms); }
int hbegp_debug_posterior_phases(int enable, double* phase_ms) { return debug_phases(PH_POSTERIOR, 4, enable, phase_ms); }

int hbegp_model_info(const hbegp_model* model, int* n, int* d, int* is_f32, double* nu, double* lml) {
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (n) *n = model->n;
  if (d) *d = model->d;
  if (is_f32) *is_f32 = model->is_f32 ? 1 : 0;
  if (nu) *nu = model->nu2 == 0 ? std::numeric_limits<double>::infinity() : model->nu2 / 2.0;
  if (lml) *lml = model->lml;
  return HBEGP_OK;
}

}  // extern "C"
template <typename T>
static int model_get(hbegp_model* m, double* theta, T* alpha, T* kinv) {
  if (!m) return fail(HBEGP_EINVAL, "NULL model");
  if (m->is_f32 != (sizeof(T) == 4)) return fail(HBEGP_EINVAL, "element type mismatch");
  GUARD_BEGIN
  std::lock_guard<std::mutex> lock(m->mu);
  HIPCHECK(hipSetDevice(m->dev));
  if (theta) memcpy(theta, m->theta.data(), sizeof(double) * m->theta.size());
  if (alpha) HIPCHECK(hipMemcpyAsync(alpha, m->alpha, sizeof(T) * m->n, hipMemcpyDeviceToHost, m->stream));
  if (kinv) HIPCHECK(hipMemcpy2DAsync(kinv, sizeof(T) * m->n, m->Kinv, sizeof(T) * m->np, sizeof(T) * m->n, m->n, hipMemcpyDeviceToHost, m->stream));
  HIPCHECK(hipStreamSynchronize(m->stream));
  return HBEGP_OK;
  GUARD_END
}
extern "C" {
int hbegp_model_get_f64(hbegp_model* model, double* theta, double* alpha, double* kinv) {
  return model_get<double>(model, theta, alpha, kinv);
}
int hbegp_model_get_f32(hbegp_model* model, double* theta, float* alpha, float* kinv) {
  return model_get<float>(model, theta, alpha, kinv);
}
int hbegp_debug_pool_poisoned(long long* blocks, long long* bytes) {
  if (blocks) *blocks = g_pool.poisoned_blocks.load(std::memory_order_relaxed);
  if (bytes) *bytes = g_pool.poisoned_bytes.load(std::memory_order_relaxed);
  return HBEGP_OK;
}
int hbegp_model_debug_params(hbegp_model* model, double* out) {
  if (!model) return fail(HBEGP_EINVAL, "NULL model");
  if (!out) return fail(HBEGP_EINVAL, "NULL out");
  GUARD_BEGIN
  std::lock_guard<std::mutex> lock(model->mu);
  HIPCHECK(hipSetDevice(model->dev));
  EvalParams P;
  HIPCHECK(hipMemcpyAsync(&P, model->dP, sizeof(P), hipMemcpyDeviceToHost, model->stream));
  HIPCHECK(hipStreamSynchronize(model->stream));
  out[0] = P.noise;
  out[1] = P.amp;
  for (int k = 0; k < model->d; ++k) out[2 + k] = P.ell[k];
  return HBEGP_OK;
  GUARD_END
}
void hbegp_model_retain(hbegp_model* model) {
  if (model) model->refs.fetch_add(1);
}
void hbegp_model_release(hbegp_model* model) {
  if (model && model->refs.fetch_sub(1) == 1) delete model;
}

int hbegp_last_fit_stats(hbegp_fit_stats* out) {
  if (!out || out->struct_size < offsetof(hbegp_fit_stats, n_evals) + sizeof(int) || out->struct_size > ((size_t)1 << 16))
    return fail(HBEGP_EINVAL, "hbegp_fit_stats.struct_size: set it to sizeof(hbegp_fit_stats) (HBEGP_FIT_STATS_INIT)");
  hbegp_fit_stats full{};
  full.struct_size = out->struct_size;
  full.n_evals = g_last_fit_stats.n_evals;
  full.n_not_pd = g_last_fit_stats.n_not_pd;
  full.n_lml_only = g_last_fit_stats.n_lml_only;
  full.n_runs = g_last_fit_stats.n_runs;
  for (int r = 0; r < full.n_runs; ++r) {
    const RunStats& rs = g_last_fit_stats.run[r];
    full.run_end_ms[r] = rs.end_ms;
    full.run_fused[r] = rs.fused; full.run_lml_only[r] = rs.lml_only; full.run_phase2[r] = rs.phase2;
    full.run_lead[r] = rs.lead; full.run_lag[r] = rs.lag;
  }
  memcpy(out, &full, std::min(out->struct_size, sizeof(full)));  // nothing beyond the caller's struct is written
  return HBEGP_OK;
}

// The optimiser's state machine replayed on a recorded sequence of values (tests): ONE loop behind hbegp_debug_lbfgs_replay and
// hbegp_debug_lbfgs_decisions.  trial / accepted / took (all three or none): per evaluation, lbfgs_is_trial, what
// lbfgs_trial_accepted said of f[i] BEFORE lbfgs_advance took it, and whether lbfgs_advance then took its accepted branch.
static int lbfgs_replay_impl(int n, const double* x0, const double* lo, const double* hi, int maxeval, int memory, int fixed_work, int count,
                             const double* f, const double* g, double* requested, int* trial, int* accepted, int* took, int* n_requested) {
  LbfgsOptions o;
  std::unique_ptr<LbfgsState> st(new LbfgsState);
  lbfgs_begin(*st, x0, lo, hi, n, maxeval, memory > 0 ? memory : o.memory, o.pgtol, o.ftol, fixed_work != 0);
  memcpy(requested, lbfgs_request(*st), sizeof(double) * n);
  int produced = 1;
  for (int i = 0; i < count; ++i) {
    if (trial) {
      trial[i] = lbfgs_is_trial(*st) ? 1 : 0;
      accepted[i] = lbfgs_trial_accepted(*st, f[i]) ? 1 : 0;
    }
    const int it0 = st->iterations;
    const bool more = lbfgs_advance(*st, f[i], g + (size_t)i * n);
    if (took) took[i] = st->iterations != it0 ? 1 : 0;
    if (!more) break;
    if (i + 1 < count) {
      memcpy(requested + (size_t)(i + 1) * n, lbfgs_request(*st), sizeof(double) * n);
      produced = i + 2;
    }
  }
  *n_requested = produced;
  return HBEGP_OK;
}

int hbegp_debug_lbfgs_decisions(int n, const double* x0, const double* lo, const double* hi, int maxeval, int memory, int fixed_work,
                                int count, const double* f, const double* g, double* requested, int* trial, int* accepted, int* took,
                                int* n_requested) {
  if (n < 1 || n > LBFGS_MAXN || count < 0 || !x0 || !lo || !hi || !requested || !n_requested || !trial || !accepted || !took ||
      (count > 0 && (!f || !g)))
    return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  return lbfgs_replay_impl(n, x0, lo, hi, maxeval, memory, fixed_work, count, f, g, requested, trial, accepted, took, n_requested);
  GUARD_END
}

// The share policy of a fit's slots as it is (slot_share.hpp), for the tests.  hysteresis < 0: the default.  lead_wg / lag_wg (may
// be NULL): the launch sizes the defaults give for `even_wg` workgroups per even launch on `cus` compute units.
int hbegp_debug_slot_shares(int n_slots, const int* running, const int* done, const int* maxeval, int hysteresis, int* share, int even_wg,
                            int cus, int* lead_wg, int* lag_wg) {
  if (n_slots < 1 || !running || !done || !maxeval || !share) return fail(HBEGP_EINVAL, "bad argument");
  slot_shares(n_slots, running, done, maxeval, hysteresis < 0 ? SLOT_SHARE_HYSTERESIS : hysteresis, share);
  if (lead_wg) *lead_wg = slot_share_lead_wg(even_wg, n_slots, cus);
  if (lag_wg) *lag_wg = slot_share_lag_wg(even_wg, n_slots, cus);
  return HBEGP_OK;
}

// Fits in flight on a device id, counted from the moment hbegp_fit_* is called (tests: start a second fit beside a first one).
int hbegp_debug_fits_in_flight(int device_id) {
  return device_id >= 0 && device_id < MAX_DEVS ? g_dev_fits[device_id].load() : 0;
}

// The three queues of a task-queue evaluation for the tests: which = 0 the full plan (with the K^-1 tiles), 1 the plan without
// them (first phase of a lazily evaluated trial), 2 the K^-1 tasks alone (dag_plan_kinv_only of the full plan).  fine as in
// hbegp_debug_dag_plan (bit 2 is implied).  tasks (may be NULL): 6 ints per task -- kind, flags, row0, col0, kbeg, kend -- for the
// first `cap` tasks in queue order.  The plan is validated; err receives the reason when it is unsound.
int hbegp_debug_dag_queues(int nblocks, int bk, int small_h, int nwg, int fine, int big128, int which, int* ntasks, int* tasks, int cap,
                           char* err, int errlen) {
  if (nblocks < 1 || (bk != 16 && bk != 32) || small_h < 0 || nwg < 0 || which < 0 || which > 2 || !ntasks) return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  DagBuilder builder(bk, small_h, nwg, (fine & 1) != 0);
  builder.set_rl_progressive((fine & 16) != 0);
  builder.set_big128(big128 != 0, big128 >= 2);
  builder.set_rl(32, 1, (fine & 32) == 0, true);  // the engine's grouping; bit 5: no split K^-1 sums (a fit with several slots)
  DagPlan plan = builder.build(0, nblocks, which != 1, (fine & 8) != 0);
  if (which == 2) plan = dag_plan_kinv_only(plan);
  const std::string why = plan.tasks.empty() ? std::string("no tasks") : dag_plan_validate(plan, nblocks);
  *ntasks = (int)plan.tasks.size();
  if (tasks)
    for (int i = 0; i < std::min(cap, (int)plan.tasks.size()); ++i) {
      const DagTask& t = plan.tasks[i];
      const int v[6] = {t.kind, t.flags, t.row0, t.col0, t.kbeg, t.kend};
      memcpy(tasks + (size_t)6 * i, v, sizeof v);
    }
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", why.c_str());
  return why.empty() ? HBEGP_OK : fail(HBEGP_EINVAL, "%s", why.c_str());
  GUARD_END
}

// A queue ordered for order_wg workers (0: nwg; -1: the count-independent order) and its in-order replay on `workers` workgroups
// (dag_plan_replay), for the tests and tools/queue_order.py.  The other arguments as hbegp_debug_dag_queues.  tasks (may be NULL):
// 18 ints per task -- kind, flags, row0, col0, kbeg, kend, nwait, wcnt[4], wval[4], sig[3] (65535: unused) -- for the first `cap`
// tasks in queue order; out (may be NULL): makespan, waiting and busy time of the replay (us, CU x us, CU x us), the planner's
// sim_us and crit_us, and the planner cost of the tasks carrying DAGF_ACC on a 128x128 tile (CU x us).  The queue is validated.
int hbegp_debug_dag_replay(int nblocks, int bk, int small_h, int nwg, int order_wg, int fine, int big128, int which, int workers,
                           int* ntasks, int* tasks, int cap, double* out, char* err, int errlen) {
  if (nblocks < 1 || (bk != 16 && bk != 32) || small_h < 0 || nwg < 1 || which < 0 || which > 2 || !ntasks || workers < 0)
    return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  DagBuilder builder(bk, small_h, nwg, (fine & 1) != 0, order_wg);
  builder.set_rl_progressive((fine & 16) != 0);
  builder.set_big128(big128 != 0, big128 >= 2);
  builder.set_rl(32, 1, (fine & 32) == 0, true);
  DagPlan plan = builder.build(0, nblocks, which != 1, (fine & 8) != 0);
  if (which == 2) plan = dag_plan_kinv_only(plan);
  const std::string why = plan.tasks.empty() ? std::string("no tasks") : dag_plan_validate(plan, nblocks);
  *ntasks = (int)plan.tasks.size();
  if (tasks)
    for (int i = 0; i < std::min(cap, (int)plan.tasks.size()); ++i) {
      const DagTask& t = plan.tasks[i];
      int* v = tasks + (size_t)18 * i;
      v[0] = t.kind; v[1] = t.flags; v[2] = t.row0; v[3] = t.col0; v[4] = t.kbeg; v[5] = t.kend; v[6] = t.nwait;
      for (int w = 0; w < DAG_MAXWAIT; ++w) { v[7 + w] = w < t.nwait ? t.wcnt[w] : 0; v[11 + w] = w < t.nwait ? t.wval[w] : 0; }
      for (int q = 0; q < DAG_MAXSIG; ++q) v[15 + q] = t.sig[q];
    }
  if (out) {
    const DagReplay r = workers > 0 ? dag_plan_replay(plan, workers) : DagReplay();
    double acc128 = 0;
    for (const DagTask& t : plan.tasks)
      if (t.kind == DAG_GEMM_128x128 && (t.flags & DAGF_ACC)) acc128 += t.cost * 0.1;
    out[0] = r.makespan_us; out[1] = r.wait_us; out[2] = r.busy_us; out[3] = plan.sim_us; out[4] = plan.crit_us; out[5] = acc128;
  }
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", why.c_str());
  return why.empty() ? HBEGP_OK : fail(HBEGP_EINVAL, "%s", why.c_str());
  GUARD_END
}

// dag_zero_halves (engine.hpp) for the tests: out receives 8 ints -- leading stages of A half 0, A half 1, B half 0, B half 1, then
// the trailing stages in the same order.
int hbegp_debug_dag_zero_halves(int flags, int row0, int col0, int kbeg, int kend, int bk, int* out) {
  if (bk < 1 || !out) return fail(HBEGP_EINVAL, "bad argument");
  const DagZeroHalf z = dag_zero_halves(flags, row0, col0, kbeg, kend, bk);
  for (int side = 0; side < 2; ++side)
    for (int h = 0; h < 2; ++h) { out[2 * side + h] = z.lead[side][h]; out[4 + 2 * side + h] = z.trail[side][h]; }
  return HBEGP_OK;
}

// What dag_default_order_wg answers (0: the launch's own count), for the tests: the defaults must be covered by the CPU checks.
int hbegp_debug_dag_order_wg(int queue, int share, int nwg, int even_wg, int nblocks, int n_slots) {
  return dag_default_order_wg(queue, share, nwg, even_wg, nblocks, n_slots);
}

int hbegp_debug_lbfgs_replay(int n, const double* x0, const double* lo, const double* hi, int maxeval, int memory, int fixed_work,
                             int count, const double* f, const double* g, double* requested, int* n_requested) {
  if (n < 1 || n > LBFGS_MAXN || count < 0 || !x0 || !lo || !hi || !requested || !n_requested || (count > 0 && (!f || !g)))
    return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  return lbfgs_replay_impl(n, x0, lo, hi, maxeval, memory, fixed_work, count, f, g, requested, nullptr, nullptr, nullptr, n_requested);
  GUARD_END
}

int hbegp_debug_dag_plan(int nblocks, int bk, int small_h, int nwg, int fine, int* ntasks, int* ncounters, int* nleaf,
                         double* gflop, double* crit_us, double* sim_us, char* err, int errlen) {
  if (nblocks < 1 || (bk != 16 && bk != 32) || small_h < 0 || nwg < 0) return fail(HBEGP_EINVAL, "bad argument");
  GUARD_BEGIN
  DagBuilder builder(bk, small_h, nwg, (fine & 1) != 0);
  builder.set_rl_progressive((fine & 16) != 0);
  builder.set_big128(getenv("HBEGP_DAG_BIG128") && atoi(getenv("HBEGP_DAG_BIG128")) != 0, getenv("HBEGP_DAG_BIG128") && atoi(getenv("HBEGP_DAG_BIG128")) >= 2);
  // bit 1: unused (rounds 2-4: kernel-matrix tiles and alpha / lml reductions as tasks too); bit 2: the K^-1 = X^T X tiles behind
  // the recursion; bit 3: the right-looking plan; bit 4: its row-progressive inverse and K^-1
  if (fine & 2) return fail(HBEGP_EINVAL, "fine bit 1 (kernel-matrix / reduction tasks in the queue) no longer exists");
  DagPlan plan = builder.build(0, nblocks, (fine & 4) != 0, (fine & 8) != 0);
  // fault injection for the validator's own test: HBEGP_DAG_TEST_FAULT = "drop:<i>" (task i loses its first wait) or
  // "move:<i>:<j>" (task i is moved to queue position j)
  if (const char* fault = getenv("HBEGP_DAG_TEST_FAULT")) {
    int a = 0, b = 0;
    if (sscanf(fault, "drop:%d", &a) == 1 && a >= 0 && a < (int)plan.tasks.size() && plan.tasks[a].nwait > 0) {
      DagTask& t = plan.tasks[a];
      for (int w = 1; w < t.nwait; ++w) { t.wcnt[w - 1] = t.wcnt[w]; t.wval[w - 1] = t.wval[w]; }
      t.nwait--;
    } else if (sscanf(fault, "move:%d:%d", &a, &b) == 2 && a >= 0 && b >= 0 && a < (int)plan.tasks.size() && b < (int)plan.tasks.size()) {
      const DagTask t = plan.tasks[a];
      plan.tasks.erase(plan.tasks.begin() + a);
      plan.tasks.insert(plan.tasks.begin() + b, t);
    }
  }
  const std::string why = plan.tasks.empty() ? std::string("too many counters") : dag_plan_validate(plan, nblocks);
  if (ntasks) *ntasks = (int)plan.tasks.size();
  if (ncounters) *ncounters = (int)plan.totals.size();
  if (nleaf) *nleaf = plan.n_leaf;
  if (gflop) *gflop = plan.gflop;
  if (crit_us) *crit_us = plan.crit_us;
  if (sim_us) *sim_us = plan.sim_us;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", why.c_str());
  return why.empty() ? HBEGP_OK : fail(HBEGP_EINVAL, "%s", why.c_str());
  GUARD_END
}

double hbegp_minimize_by_gradient(hbegp_objective_fn f, void* user, double* x, const double* lo, const double* hi, int n,
                                  int maxeval) {
  if (!f || !x || !lo || !hi || n < 1) {
    fail(HBEGP_EINVAL, "hbegp_minimize_by_gradient: NULL argument or n < 1");
    return std::numeric_limits<double>::quiet_NaN();
  }
  try {
    LbfgsOptions opt;
    opt.maxeval = maxeval > 0 ? maxeval : 150;
    Objective obj = [&](const double* xx, double* g) { return f(xx, g, user); };
    return lbfgsb_minimize(obj, x, lo, hi, n, opt).f;
  } catch (const std::exception& e) {
    fail(HBEGP_EHIP, "hbegp_minimize_by_gradient: %s", e.what());
  } catch (...) {
    fail(HBEGP_EHIP, "hbegp_minimize_by_gradient: unknown exception");
  }
  return std::numeric_limits<double>::quiet_NaN();
}

}  // extern "C"
