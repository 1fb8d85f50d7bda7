// C ABI of the gfx950 SSG engine -- the edge list, the maps, the losses, the fused step, the operator and the process-wide
// settings: argument checking, workspace carving and kernel dispatch.  See include/ssg_hip.h for the contract of every
// entry point and the reference interface it replaces.  Every other family's entry points are defined beside its kernels.
#include "../../include/ssg_hip.h"

#include <atomic>
#include <climits>
#include <cstdlib>
#include <mutex>

#include "ssg_host.hpp"

using namespace ssg;

// Edge pixels per dense tile (8 x 32 for k_s 25, 4 x 32 for k_s 49) from which the shared-term kernels take the tile
// (0 = never).  The marginal costs of the two paths are equal between 16 and 28 pixels per tile; below ~16 the direct
// kernels win.  Round-4 sweeps (tools/r4_thr_sweep2.sh, r4_thr_sweep3.sh; same box): 20 against 28: C2
// 1.308 vs 1.318 ms, stride-3 C4 0.540 vs 0.560, Bernoulli 4 % 0.513 vs 0.512, C5 7.78 vs 7.78; again at the end of the
// round, after the direct forward had lost 9 % of its instructions (profiles/r4_dense_threshold_18_vs_20.txt, three
// alternations): 18 against 20: C2 1.2771 vs 1.2849, fused 1.2225 vs 1.2309, C4 0.5024 vs 0.5196, Bernoulli 4 % 0.4925
// vs 0.4868, 1 % equal (16 costs the Bernoulli masks 3 %, 24 and above cost C4 4 %).  Round 6, after the dense-tile
// kernels lost 6-7 % of their time (profiles/r6_dense_threshold_sweep.txt, three alternations): 16 against 18: C2 1.1936
// vs 1.2034, C4 0.446 vs 0.444, Bernoulli 4 % 0.456 vs 0.459, 1 % equal; 14: 1.1987 / 0.439; 12: 1.208 / 0.428 (C4's
// best); 10 costs Bernoulli 4 % 20 %.  Default 16.
// ssg_set_dense_threshold(n) overrides it (profiling build: also the environment variable SSG_DENSE_THR at first use).
constexpr int DENSE_THR_DEFAULT = 16;
// A process-wide setting behind a set function of the ABI: unset (negative) until its first read, which takes init() --
// the default; in the profiling build an environment variable.  (atomic: the ABI may be called from several host threads)
template <class Init>
static int setting(std::atomic<int> &s, Init init) {
  int v = s.load(std::memory_order_relaxed);
  if (v < 0) s.store(v = init(), std::memory_order_relaxed);
  return v;
}
static std::atomic<int> g_dense_thr{-1};
static int dense_threshold() {
  return setting(g_dense_thr, [] { const int v = env_int("SSG_DENSE_THR", DENSE_THR_DEFAULT); return v < 0 ? 0 : v; });
}

// Small (11,5) steps in two launches (ssg_tiny.hip); on by default, ssg_set_tiny_step(0) keeps every call on the general path.
static std::atomic<int> g_tiny_step{1};
extern "C" int ssg_set_tiny_step(int on) { return g_tiny_step.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed); }
extern "C" int ssg_set_operator_plan_threshold(int positions);
extern "C" int ssg_set_dense_threshold(int edge_pixels_per_tile) {
  const int prev = dense_threshold();
  g_dense_thr.store(edge_pixels_per_tile > 0 ? edge_pixels_per_tile : 0, std::memory_order_relaxed);
  return prev;
}

// Profiling build only (-DSSG_PROFILE -> libssg_hip_prof.so): SSG_DEBUG_SKIP=<bitmask> / ssg_set_profile_mask ablate
// kernel phases or skip whole launches (results are then WRONG).  Bits 0-7 direct forward phases, 8-15 backward
// phases, 16-23 dense forward phases, 24 no split backward; launches skipped: 25 dense forward, 26 direct forward,
// 27 dense backward, 28 direct backward (split mode), 29 G rows.  The product library has neither the symbol nor the
// environment variable: its mask is the constant 0 and every test on it folds away.
#ifdef SSG_PROFILE
static std::atomic<int> g_dbg{-1};
static int dbg_mask() {
  return setting(g_dbg, [] { const int v = env_int("SSG_DEBUG_SKIP", 0); return v < 0 ? 0 : v; });
}
// LDS poison (ssg_common.hpp): one workgroup per CU at a time (all 160 KB), several rounds so that every CU gets one
static std::atomic<int> g_lds_poison_on{0};
static std::atomic<unsigned> g_lds_poison_pat{0};
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned pat, int words) {
  extern __shared__ unsigned s_poison[];
  volatile unsigned *w = s_poison;
  for (int i = threadIdx.x; i < words; i += 256) w[i] = pat;
}
namespace ssg {
void prof_poison_lds(hipStream_t st) {
  if (!g_lds_poison_on.load(std::memory_order_relaxed)) return;
  constexpr int BYTES = 160 * 1024;
  static std::atomic<unsigned long long> lds_set{0};
  if (ensure_dynamic_lds(lds_poison_kernel, BYTES, lds_set)) return;
  lds_poison_kernel<<<dim3(1024), dim3(256), BYTES, st>>>(g_lds_poison_pat.load(std::memory_order_relaxed), BYTES / 4);
}
}  // namespace ssg
extern "C" int ssg_prof_set_lds_poison(int on, unsigned pattern) {
  const int prev = g_lds_poison_on.load(std::memory_order_relaxed);
  g_lds_poison_pat.store(pattern, std::memory_order_relaxed);
  g_lds_poison_on.store(on ? 1 : 0, std::memory_order_relaxed);
  return prev;
}
extern "C" int ssg_prof_strip_times(unsigned long long *host, int n) { return ssg::strip_times(host, n); }
extern "C" int ssg_prof_occupancy(int which) { return which == 0 ? ssg::strip_occupancy() : -1; }
extern "C" int ssg_set_profile_mask(int mask) {
  const int prev = dbg_mask();
  g_dbg.store(mask > 0 ? mask : 0, std::memory_order_relaxed);
  return prev;
}
#else
static constexpr int dbg_mask() { return 0; }
#endif

// The dense-tile kernel and the direct kernel of a pass work on disjoint SSG rows (and add into the gradient with
// atomics), so the direct one runs on a side stream beside the dense one: fork = side waits for an event on the
// caller's stream, join = the caller's stream waits for the side's event.  Both are plain event edges, so a stream
// capture of the caller's stream (hipGraph) records the fork as two parallel branches.  One side stream and four
// events per (host thread, device); ssg_set_overlap(0) keeps every launch on the caller's stream.  Measured on MI355X:
// C2 (k_s 25) 1.541 -> 1.510 ms per step; C5 (k_s 49, every kernel already fills the chip for its whole run)
// 9.15 -> 9.64 ms -- so the fork is taken for k_s <= 25 only.
struct SideStream {
  hipStream_t side = nullptr;
  hipEvent_t forked = nullptr, joined = nullptr, gate = nullptr, gate2 = nullptr;
};
static std::atomic<int> g_overlap{-1};
// 0 off, 1 dense-tile kernel on the caller's stream, 2 direct kernel on the caller's stream, 3 (default) whichever of the
// two the previous plan built on this device makes the longer branch
static int overlap_mode() {
  return setting(g_overlap, [] { const int v = env_int("SSG_OVERLAP", 3); return v < 0 ? 0 : (v > 3 ? 3 : v); });
}

// Index of the calling thread's current device in the library's per-device tables (plan hint, side stream, status word,
// operator pool); -1: no current device, or one beyond the tables -- such a call runs without the table's service.
constexpr int MAXDEV = 64;
static int current_device_slot() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAXDEV ? dev : -1;
}

static bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// What the last plan built on a device looked like: {rows left to the direct kernels, dense tiles}, written by the
// edge-list builder's scan kernel with a plain store into host-mapped pinned memory (one 64-byte block per device,
// allocated at the first build, never freed; a posted PCIe write, no stream operation) and read by the HOST once per
// call (schedule() below) -- no synchronisation: whatever has landed is a hint, and every schedule gives the same results.
struct PlanHint {
  int *host = nullptr, *dev = nullptr;
};
constexpr bool NEVER_ALLOCATE = true;   // (plan_hint: a reader's call)
static PlanHint plan_hint(bool allocate_never = false) {
  static std::mutex mu;
  static PlanHint tab[MAXDEV];
  const int dev = current_device_slot();
  if (dev < 0) return PlanHint{};
  std::lock_guard<std::mutex> lk(mu);
  if (!tab[dev].host) {
    // hipHostMalloc is not allowed while the calling stream is being captured (it fails, and in the global / thread-local
    // capture modes invalidates the capture): the block is allocated by the first call per device made OUTSIDE capture;
    // a first call under capture runs without a hint (gated chains, dense kernels on the caller's stream).
    if (allocate_never) return PlanHint{};
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) return PlanHint{};
    ((int *)h)[0] = ((int *)h)[1] = -1;   // nothing seen yet
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipHostFree(h);
      return PlanHint{};
    }
    tab[dev] = PlanHint{(int *)h, (int *)d};
  }
  return tab[dev];
}
namespace ssg {
int *plan_hint_device_word(hipStream_t st) {
  if (overlap_mode() != 3) return nullptr;
  return plan_hint(stream_capturing(st)).dev;
}
}

// The schedule of one entry-point call: which stream takes the dense-tile kernels and which the direct ones, and -- in
// a fused step or a loss backward at k_s <= 25 -- whether the two classes run as two CHAINS.  The dense-tile chain
// (forward, its rows' ssg_grad_rows pass, backward) and the direct chain (the same three for the rows of the plan's
// sparse list) then share nothing until ONE join at the end: the row passes are per class anyway (split_backward), the
// fixed-point scale of the deterministic accumulation comes from the a-priori bound of |G| (no maximum over all rows to
// wait for), integer sums do not care who adds first, the criteria sums go to separate slots.  Same bits as fork / join
// around each pass -- only the streams differ -- with one cross-stream round trip less, and the memory-bound row pass of
// one chain runs beside the VALU-bound kernels of the other.
// FREE-RUNNING chains pay when the direct chain carries the step (Bernoulli 4 %: 0.485 -> 0.463 ms) or the dense kernels
// are too few workgroups to keep the chip to themselves (C4, 330 tiles: 0.50 -> 0.466).  Where long dense kernels
// dominate (C2: 1,287 tiles, direct 0.38 ms of kernel time against 0.95) free-running direct kernels spend themselves
// beside the dense FORWARD and the dense backward runs alone with its tail unfilled (+8 %); there the chains are GATED:
// the direct backward waits, one way, for the dense chain (split_backward; C2 1.271 -> 1.248 against fork / join around
// each pass; a low-priority side stream: no effect).
struct Schedule {
  hipStream_t st = nullptr;     // the caller's stream
  bool may_fork = false;        // k_s <= 25, and overlap not off (ssg_set_overlap(0))
  int assign = 0;               // 1: dense-tile kernels on st, direct ones on the side stream; 2: the other way round
  bool chains = false;          // two chains: the forward's fork stays open for the backward (or it opens at the row passes)
  bool gated = false;           // ... with the direct backward held behind the dense forward (dense chain on st)
  int rows_hint = 0;            // rows the last plan left to the direct kernels (FwdParams / BwdParams::rows_hint); 0 unknown
  SideStream *side = nullptr;   // (fork_side)
  bool open = false;            // forked, not yet joined
  hipStream_t dense() const { return open && assign == 2 ? side->side : st; }
  hipStream_t direct() const { return open && assign == 1 ? side->side : st; }
};

// One read of the overlap mode, of the plan hint and (where it decides) of the capture state per call: the hint is
// written by the GPU asynchronously, and decisions taken from two reads could disagree (a flip between them could record
// a gated pair into a capturing stream).  `chains`: the call can run two chains (a fused step with a gradient and a plan;
// a loss backward, whose split_backward checks the rest).
enum class Chains { never, possible };
static Schedule schedule(hipStream_t st, int ks, Chains chains) {
  Schedule s;
  s.st = st;
  const int mode = overlap_mode();
  int n_sparse = -1, n_tiles = -1;
  if (mode == 3) {
    const PlanHint h = plan_hint(NEVER_ALLOCATE);   // (readers never allocate: the builder's launch does, outside capture)
    if (h.host) {
      n_sparse = ((volatile int *)h.host)[0];
      n_tiles = ((volatile int *)h.host)[1];
    }
  }
  const bool known = n_sparse >= 0 && n_tiles >= 0;
  // whole-chip costs at (25,9), MI355X: a dense tile 0.74 us through forward + backward, a direct row 38 ns
  const bool direct_longer = known && (long long)n_sparse * 38 > (long long)n_tiles * 740;
  s.assign = mode == 3 ? (direct_longer ? 2 : 1) : mode;
  s.rows_hint = n_sparse > 0 ? n_sparse : 0;
  s.may_fork = ks <= 25 && mode != 0;
  // free-running: the direct chain carries the step, or the dense kernels' grids (two images per tile) are at most two
  // resident rounds of 512 workgroups -- too short to keep the chip to themselves anyway; no hint = gated
  const bool free = mode == 3 && known && (direct_longer || n_tiles <= 512);
  // (under stream capture only free-running chains: they replay well -- C4 0.452 ms as a graph, 0.495 joined --, a
  // GATED pair does not: C2 as a graph 1.44 ms gated, 1.26 with fork / join around each pass, which it keeps)
  s.chains = chains == Chains::possible && s.may_fork && (free || !stream_capturing(st));
  s.gated = !free && s.assign == 1;   // (dense chain on the side stream -- a forced ssg_set_overlap(2): free-running)
  return s;
}

static thread_local int t_last_assignment = 0;
// (diagnostics: the assignment the calling thread's last forked pass used -- 0 none, 1 dense-tile kernel on the caller's
// stream, 2 direct kernel on the caller's stream)
extern "C" int ssg_last_overlap_assignment(void) { return t_last_assignment; }
// ssg_set_overlap(0): every launch on the caller's stream (per-kernel rocprofv3 durations: profiles/*_kernel_stats.csv
// are taken that way; same results -- the two branches work on disjoint rows).  1 (default): the dense-tile kernel on
// the caller's stream, the direct one on the side stream -- right where dense tiles carry most rows (Laplacian masks:
// C2).  2: the other way round -- right for masks WITHOUT dense tiles (Bernoulli / thin strided masks), whose whole
// critical path then sits on one stream and whose join finds the side stream's empty launches finished.  Measured on one
// box (profiles/r5_ab_stream_assignment.txt): mode 2 against 1: Bernoulli 1 % 0.213 -> 0.182 ms, 4 % 0.491 -> 0.466,
// C4 0.498 -> 0.508, C2 1.275 -> 1.317 (the fork's latency lands on whichever kernel runs on the side stream).
// 3 (default since round 5): 1 or 2 per call, from the shape of the last plan built on the device (PlanHint above): the
// branch expected to run longer stays on the caller's stream.  Steady streams of similar masks settle after one call.
// Returns the previous setting.
extern "C" int ssg_set_overlap(int mode) {
  const int prev = overlap_mode();
  g_overlap.store(mode < 0 ? 0 : (mode > 3 ? 3 : mode), std::memory_order_relaxed);
  return prev;
}
static SideStream *side_stream() {
  thread_local SideStream tab[MAXDEV];
  const int dev = current_device_slot();
  if (dev < 0) return nullptr;
  SideStream &s = tab[dev];
  if (!s.side) {
    if (hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s.forked, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.joined, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.gate, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.gate2, hipEventDisableTiming) != hipSuccess) {
      s.side = nullptr;
      return nullptr;
    }
  }
  return &s;
}
// Fork at a pass that can fork: the side stream takes what follows after everything queued on the caller's so far (no
// fork: every launch on the caller's stream; `skip`, profiling build: a launch of the pass is masked out).
static void fork_side(Schedule &s, bool skip = false) {
  s.side = s.may_fork && !skip ? side_stream() : nullptr;
  s.open = s.side && hipEventRecord(s.side->forked, s.st) == hipSuccess &&
           hipStreamWaitEvent(s.side->side, s.side->forked, 0) == hipSuccess;
  t_last_assignment = s.open ? s.assign : 0;
}
static int join_side(Schedule &s) {
  if (!s.open) return 0;
  s.open = false;
  int rc = (int)hipEventRecord(s.side->joined, s.side->side);
  if (!rc) rc = (int)hipStreamWaitEvent(s.st, s.side->joined, 0);
  return rc;
}

// One 4-byte status word per device, owned by the library (allocated at the first call that can set it, never freed):
// kernels that refuse their input without a host-visible error -- a dense kernel handed a plan cut for another tile
// height -- set a bit in it; ssg_device_status() reads and clears it.
static int *device_status_word() {
  static std::mutex mu;
  static int *tab[MAXDEV] = {};
  const int dev = current_device_slot();
  if (dev < 0) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!tab[dev]) {
    int *w = nullptr;
    if (hipMalloc(&w, sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemset(w, 0, sizeof(int)) != hipSuccess) {
      (void)hipFree(w);
      return nullptr;
    }
    tab[dev] = w;
  }
  return tab[dev];
}

static bool sizes_ok(int ks, int kw) { return ks > 0 && kw > 0 && (ks & 1) && (kw & 1) && kw <= ks; }

// Waves per tile of the dense-tile backward (each takes a contiguous range of offset rows): by default chosen on the
// device so that the launch fills the chip about once; SSG_BWD_QSPLIT fixes it in the profiling build (experiments).
static int bwd_qsplit() {   // 0 = chosen on the device from the number of dense tiles (DenseBwdParams::qsplit)
  static const int env = env_int("SSG_BWD_QSPLIT", 0), v = env < 0 ? 0 : (env > 25 ? 25 : env);
  return v;
}

// a capacity as the sizes below count it: room for one row at least
static size_t rows_of(int capacity) { return (size_t)(capacity > 0 ? capacity : 1); }

// Scratch of the split backward (ssg_grad_rows -> dense-tile kernel + direct kernel), carved in one place: the sizes
// (ssg_backward_scratch_bytes, ssg_loss_scratch_bytes), split_backward and loss_backward use it.  GRAD_LOSS: a loss step's
// scratch, which has the criteria sums' partials in front (none of B, H, W is looked at otherwise).
struct BackwardScratch {
  size_t partials, G, sum_b, gmax_part, dot, end;
};
static BackwardScratch carve_backward_scratch(int B, int H, int W, int n_rows, int ks, GradMode mode) {
  const size_t n = rows_of(n_rows);
  BackwardScratch s{};
  Carver c;
  s.partials = c.take(mode == GRAD_LOSS ? 2 * sizeof(float) * bwd_max_partials(B, H, W, n_rows) + 64 : 0);
  s.G = c.take(sizeof(float) * n * ks * ks);   // (n, k_s^2)
  s.sum_b = c.take(sizeof(float) * n);         // (n)
  s.gmax_part = c.take(sizeof(float) * n);     // max|G| parts
  s.dot = c.take(sizeof(float) * n);
  s.end = c.end;
  return s;
}

// Tile-major scratch rows of the fused step at k_s = 49 (TmRowsParams, ssg_common.hpp): the dense tiles in the first
// `slots` places of the plan keep their e rows in a second rows region, tile by tile, and the three kernels that touch
// them move whole 256-byte runs.  (Profiling build: SSG_TILE_MAJOR=0 keeps every row row-major, SSG_STRIPS=0 leaves
// every tile-major tile to the tile kernel -- A/B measurements; a product caller gets the row-major step by not giving
// the workspace the tile-major bytes, LossStep(tile_major=False).)
struct TileMajor {
  float *rows[2] = {nullptr, nullptr};
  int slots = 0;
};
static bool strips_enabled() {   // SSG_STRIPS=0: the tile kernel computes every tile-major tile (A/B measurements)
  static const bool on = env_int("SSG_STRIPS", 1) != 0;
  return on;
}
static bool tile_major_enabled() {
  static const bool on = env_int("SSG_TILE_MAJOR", 1) != 0;
  return on;
}

// One description of an entry-point call: what the map, loss and operator entry points are given, under one set of
// names.  Each entry point fills it once; map_forward_impl, loss_backward, split_backward and the functions that build
// the kernels' parameter structs below read it (with the call's Schedule, which holds the streams).  The operator is a
// call with (Y, X) positions (estride 2), one image, raw output and sigma 1.
struct Call {
  const float *img = nullptr, *img2 = nullptr;   // (B,C,H,W): the image (sr); the second image of a forward (gt)
  int B = 0, C = 0, H = 0, W = 0;
  const int *edges = nullptr;
  int estride = 3;                 // 3: (b,y,x) rows of an edge list; 2: the operator's (Y,X) positions
  const int *order = nullptr;      // nullable: tile-major order of the rows
  const int *rank = nullptr;       // nullable: rank map (with plan: the dense-tile kernels)
  const int *plan = nullptr;       // nullable: forward plan
  const int *n_dev = nullptr;      // nullable: the device's row count
  int n_rows = 0;                  // the host's bound on the rows
  int ks = 0, kw = 0;
  float sigma = 1.f, eps = 0.f;
  int generalization = 0;
  int raw = 0;                     // 1: the reference operator's forward (out += D)
  float w_l1 = 0.f, w_kl = 0.f;
  const float *upstream = nullptr;   // nullable device {dL/dl1, dL/dkl}
  float *ssg = nullptr, *ssg2 = nullptr;   // the SSG tensors (forward: outputs; GRAD_S: S saved; GRAD_LOSS: S_sr, S_gt)
  const float *gin = nullptr;      // GRAD_D: dL/dD; GRAD_S: dL/dS
  float *loss_out = nullptr;
  float *grad = nullptr;           // nullable in a loss call: loss only
  void *grad_fix = nullptr;        // nullable: deterministic mode (grad_fix_bytes)
  double *row_scale = nullptr;     // nullable: deferred normalisation (written by the dense forward, read by the row passes)
  void *scratch = nullptr;         // the backward's scratch (BackwardScratch)
  TileMajor tm;                    // the tile-major regions (slots 0: none)
  bool row_scale_zeroed = false;   // the row scales were cleared by the edge-list builder's first kernel
  bool rows_scratch = false;       // the SSG tensors are the engine's own scratch: nothing is written back
  bool fix_zeroed = false;         // the fixed-point sums were cleared by the edge-list builder's first kernel
  bool grad_is_output = false;     // the gradient is an OUTPUT of the call: the deterministic flush assigns it (fp32 atomics: cleared first)
  bool nan_on_overflow = false;    // the loss finalize / tiny step report an overflowed edge list as NaN
};

// The checks of the map and loss entry points, in the order the ABI documents: bad sizes, then an image too small for
// reflect padding, then "nothing to do" (a loss call zero-fills loss_out), then the null checks of the kind of call.
// true: the call ends here with `rc`.
enum CallKind { MAP_FORWARD, MAP_BACKWARD, LOSS_BACKWARD };
static bool call_ends(const Call &c, CallKind kind, hipStream_t st, int &rc) {
  rc = SSG_E_BADARG;
  if (c.n_rows < 0 || !sizes_ok(c.ks, c.kw) || c.B <= 0 || c.C <= 0 || (kind == LOSS_BACKWARD && !c.loss_out)) return true;
  rc = SSG_E_IMAGESMALL;
  if (c.H <= c.ks / 2 || c.W <= c.ks / 2) return true;
  if (c.n_rows == 0) {
    rc = kind == LOSS_BACKWARD ? (int)hipMemsetAsync(c.loss_out, 0, 2 * sizeof(float), st) : 0;
    return true;
  }
  rc = SSG_E_BADARG;
  if (!c.img || !c.edges || !c.ssg) return true;
  switch (kind) {
    case MAP_FORWARD: return (c.img2 != nullptr) != (c.ssg2 != nullptr);
    case MAP_BACKWARD: return !c.gin || !c.grad;
    case LOSS_BACKWARD: return !c.ssg2 || !c.scratch;
  }
  return true;
}

// ---- the kernels' parameter structs (ssg_common.hpp), each value-initialised and filled in ONE function ----
static FwdParams fwd_params(const Call &c) {
  FwdParams p{};
  p.img[0] = c.img;
  p.img[1] = c.img2;
  p.out[0] = c.ssg;
  p.out[1] = c.ssg2;
  p.nimg = c.img2 ? 2 : 1;
  p.edges = c.edges;
  p.estride = c.estride;
  p.order = c.order;
  p.n_dev = c.n_dev;
  p.n_host = c.n_rows;
  p.B = c.B;
  p.C = c.C;
  p.H = c.H;
  p.W = c.W;
  p.sigma = c.sigma;
  p.eps = c.eps;
  p.generalization = c.generalization;
  p.raw = c.raw;
  p.ks = c.ks;
  p.kw = c.kw;
  p.dbg = dbg_mask() & 0xff;
  return p;
}

// dense tiles -> shared-term kernel (the operator: in raw mode)
static DenseParams dense_params(const Call &c, const PlanView &pv) {
  DenseParams d{};
  d.img[0] = c.img;
  d.img[1] = c.img2;
  d.out[0] = c.ssg;
  d.out[1] = c.ssg2;
  d.nimg = c.img2 ? 2 : 1;
  d.rank = c.rank;
  d.n_dense = pv.dense_hdr;
  d.tiles = pv.tiles;
  d.max_tiles = dense_max_tiles(c.B, c.H, c.W, c.ks);
  d.n_dev = c.n_dev;
  d.n_host = c.n_rows;
  d.B = c.B;
  d.H = c.H;
  d.W = c.W;
  d.sigma = c.sigma;
  d.eps = c.eps;
  d.generalization = c.generalization;
  d.dbg = (dbg_mask() >> 16) & 0xff;
  d.row_scale = c.row_scale;
  d.status = device_status_word();
  d.raw = c.raw;
  if (c.tm.slots > 0 && c.row_scale && c.img2) {
    d.tm[0] = c.tm.rows[0];
    d.tm[1] = c.tm.rows[1];
    d.tm_slots = c.tm.slots;
    d.max_strips = strips_enabled() ? dense_max_strips(c.B, c.H, c.W, c.ks) : 0;   // (k_s 49: whole strips of heavy tiles)
    d.strips = d.max_strips ? pv.strips : nullptr;
  }
  return d;
}

// The three gradient modes differ only in which sources they set.  Deterministic mode: the kernels add into the
// caller's zeroed fixed-point buffer (det_begin), one flush folds it into grad (det_end).
static BwdParams bwd_params(const Call &c, GradMode mode) {
  BwdParams p{};
  p.img = c.img;
  p.grad = c.grad;
  p.gfix = c.grad_fix && c.grad ? (long long *)c.grad_fix : nullptr;
  p.edges = c.edges;
  p.estride = c.estride;
  p.order = c.order;
  p.n_dev = c.n_dev;
  p.n_host = c.n_rows;
  p.B = c.B;
  p.C = c.C;
  p.H = c.H;
  p.W = c.W;
  p.mode = mode;
  p.sigma = c.sigma;
  p.generalization = c.generalization;
  p.ks = c.ks;
  p.kw = c.kw;
  p.dbg = (dbg_mask() >> 8) & 0xff;
  switch (mode) {
    case GRAD_D:
      p.gin = c.gin;
      break;
    case GRAD_S:
      p.gin = c.gin;
      p.ssg = c.ssg;
      break;
    case GRAD_LOSS:
      p.ssg = c.ssg;
      p.ssg2 = c.ssg2;
      p.w_l1 = c.w_l1;
      p.w_kl = c.w_kl;
      p.upstream = c.upstream;
      p.row_scale = c.row_scale;
      p.rows_scratch = c.rows_scratch ? 1 : 0;
      p.partials = (float *)((char *)c.scratch + carve_backward_scratch(c.B, c.H, c.W, c.n_rows, c.ks, mode).partials);
      break;
  }
  return p;
}

// nparts of a split backward's criteria sums: ssg_grad_rows' workgroups, then ssg_rows_tm's
static int split_tm_tiles(const BwdParams &p, const TileMajor &tm) {
  if (tm.slots <= 0) return 0;
  const int mt = dense_max_tiles(p.B, p.H, p.W, p.ks);
  return tm.slots < mt ? tm.slots : mt;
}

// per-class row passes (split_backward): the criteria sums then take two sets of grow_grid(n_rows) slots
static bool split_row_classes(const BwdParams &p, int n_tm) {
  return p.mode == GRAD_LOSS && n_tm == 0 && p.row_scale && p.ks <= 25;
}

// What split_backward adds to a call's BwdParams for its three kernels: the pieces of the scratch, the plan's parts,
// the tile-major regions in use and where the fixed-point scale comes from.
struct SplitParts {
  float *G, *sum_b, *gmax_part, *dot;
  PlanView pv;
  const int *rank;
  const TileMajor *tm;
  int n_tm;           // tile-major tiles of the call (split_tm_tiles; 0: row-major rows only)
  bool apriori;       // the fixed-point scale comes from the a-priori bound of |G|
};

static GrowParams grow_params(const BwdParams &p, const SplitParts &x) {
  GrowParams g{};
  g.mode = p.mode;
  g.gin = p.gin;
  g.ssg = p.ssg;
  g.ssg2 = p.ssg2;
  g.row_scale = p.row_scale;
  g.rows_scratch = p.rows_scratch;
  g.n_dev = p.n_dev;
  g.n_host = p.n_host;
  g.C = p.C;
  g.sigma = p.sigma;
  g.generalization = p.generalization;
  g.w_l1 = p.w_l1;
  g.w_kl = p.w_kl;
  g.upstream = p.upstream;
  g.G = p.grad ? x.G : nullptr;
  g.sum_b = p.grad ? x.sum_b : nullptr;
  g.partials = p.partials;
  g.gmax_part = p.gfix ? x.gmax_part : nullptr;
  if (x.n_tm > 0) {   // (tile-major call: ssg_grad_rows walks the plan's list of sparse rows with a capped grid)
    g.grid_cap = 4096;
    g.tm_hdr = x.pv.dense_hdr;
    g.tm_slots = x.tm->slots;
    g.sparse_order = x.pv.sparse_order;
  }
  if (x.apriori) {   // (ssg_grad_rows' first workgroup writes the bound into the word behind the fixed-point sums)
    g.gmax_part = nullptr;
    g.fix_word = (unsigned *)(p.gfix + (size_t)p.B * p.C * p.H * p.W);
  }
  return g;
}

// the rows of the tile-major tiles (ssg_grad_rows skips them: negative row scale)
static TmRowsParams tm_rows_params(const BwdParams &p, const SplitParts &x) {
  TmRowsParams t{};
  t.tm[0] = x.tm->rows[0];
  t.tm[1] = x.tm->rows[1];
  t.row_scale = p.row_scale;
  t.rank = x.rank;
  t.n_dense = x.pv.dense_hdr;
  t.tiles = x.pv.tiles;
  t.n_tiles = x.n_tm;
  t.tm_slots = x.tm->slots;
  t.n_dev = p.n_dev;
  t.n_host = p.n_host;
  t.B = p.B;
  t.H = p.H;
  t.W = p.W;
  t.C = p.C;
  t.sigma = p.sigma;
  t.w_l1 = p.w_l1;
  t.w_kl = p.w_kl;
  t.upstream = p.upstream;
  t.dot = x.dot;
  t.sum_b = x.sum_b;
  t.partials = p.partials + 2 * (size_t)grow_grid(p.n_host);
  t.gmax_part = p.gfix ? x.gmax_part + grow_grid(p.n_host) : nullptr;
  if (!p.rows_scratch) {   // materialising call: the normalised rows of the tile-major tiles are written here
    t.out[0] = p.ssg;
    t.out[1] = p.ssg2;
  }
  return t;
}

static DenseBwdParams dense_bwd_params(const BwdParams &p, const SplitParts &x) {
  DenseBwdParams d{};
  d.img = p.img;
  d.grad = p.grad;
  d.gfix = p.gfix;
  d.G = p.mode == GRAD_D ? p.gin : x.G;   // (GRAD_D: the caller's rows ARE the G rows)
  d.sum_b = x.sum_b;
  d.rank = x.rank;
  d.n_dense = x.pv.dense_hdr;
  d.tiles = x.pv.tiles;
  d.max_tiles = dense_max_tiles(p.B, p.H, p.W, p.ks);
  d.n_dev = p.n_dev;
  d.n_host = p.n_host;
  d.B = p.B;
  d.H = p.H;
  d.W = p.W;
  d.qsplit = bwd_qsplit();
  d.dbg = p.dbg;
  d.status = device_status_word();
  if (x.n_tm > 0) {
    d.tm[0] = x.tm->rows[0];
    d.tm[1] = x.tm->rows[1];
    d.row_scale = p.row_scale;
    d.dot = x.dot;
    d.tm_slots = x.tm->slots;
    d.sigma = p.sigma;
    d.w_l1 = p.w_l1;
    d.w_kl = p.w_kl;
    d.upstream = p.upstream;
  }
  return d;
}

// the fused step of a small (11,5) call; `ticket`: the word tiny_edge_list zeroed
static TinyParams tiny_params(const Call &c, int *ticket) {
  TinyParams t{};
  t.img[0] = c.img;
  t.img[1] = c.img2;
  t.out[0] = c.rows_scratch ? nullptr : c.ssg;
  t.out[1] = c.rows_scratch ? nullptr : c.ssg2;
  t.edges = c.edges;
  t.n_dev = c.n_dev;
  t.n_host = c.n_rows;
  t.B = c.B;
  t.H = c.H;
  t.W = c.W;
  t.sigma = c.sigma;
  t.eps = c.eps;
  t.generalization = c.generalization;
  t.w_l1 = c.w_l1;
  t.w_kl = c.w_kl;
  t.grad = c.grad;
  t.gfix = c.grad_fix && c.grad ? (long long *)c.grad_fix : nullptr;
  t.assign = c.grad_is_output ? 1 : 0;
  t.partials = (float *)c.scratch;
  t.loss_out = c.loss_out;
  t.ticket = ticket;
  t.nan_on_overflow = c.nan_on_overflow ? 1 : 0;
  t.dbg = env_int("SSG_TINY_DBG", 0);
  return t;
}

// Backward over a forward plan: G rows (+ criteria sums) by ssg_grad_rows, the dense tiles by the shared-term
// kernel, the remaining rows by the direct kernel in GRAD_D mode.  `p` carries the call's sources as for launch_bwd.
// `fin` (with `fin_done`): the loss finalize of a GRAD_LOSS step, launched here where the schedule has a place for it
// off the critical path.  Joins the call's fork behind the backward kernels.
static int split_backward(const Call &c, const BwdParams &p, Schedule &sc, const LossFinalize *fin = nullptr,
                          bool *fin_done = nullptr) {
  const hipStream_t st = sc.st;
  const BackwardScratch bs = carve_backward_scratch(p.B, p.H, p.W, p.n_host, p.ks, (GradMode)p.mode);
  char *const scratch = (char *)c.scratch;
  SplitParts x{};
  x.G = (float *)(scratch + bs.G);
  x.sum_b = (float *)(scratch + bs.sum_b);
  x.gmax_part = (float *)(scratch + bs.gmax_part);
  x.dot = (float *)(scratch + bs.dot);
  x.pv = plan_view(c.plan, p.B, p.H, p.W);
  x.rank = c.rank;
  x.tm = &c.tm;
  x.n_tm = split_tm_tiles(p, c.tm);
  const int n_tm = x.n_tm;
  // GRAD_LOSS without tile-major rows (every k_s <= 25 call): the fixed-point scale comes from the a-priori bound of |G|
  // (ssg_grad_rows' first workgroup writes it: no maximum over the rows, no reduction launch); and with deferred row
  // scales the rows are passed over PER CLASS -- the dense-tile kernels' rows (non-zero scale), then the plan's sparse
  // list -- whatever the schedule, so that the criteria sums are grouped the same way on one stream and on two.
  const size_t n_fix = (size_t)p.B * p.C * p.H * p.W;
  x.apriori = p.gfix && p.mode == GRAD_LOSS && n_tm == 0;
  const bool classes = split_row_classes(p, n_tm);
  const GrowParams g = grow_params(p, x);
  // A backward on its own (ssg_loss_backward: the deferred loop's node, the module) forks HERE and runs the same two
  // chains from the row passes on: the sparse list's pass beside the dense-tile rows' instead of behind it.
  if (sc.chains && !sc.open && classes && p.grad) fork_side(sc, dbg_mask() & ((1 << 27) | (1 << 28) | (1 << 29)));
  // Gated chains: the direct backward is released once the dense FORWARD is through and runs beside the memory-bound
  // dense row pass -- C2 1.1996 -> 1.178 ms against a release behind that row pass, three alternations
  // (profiles/r6_schedule_ab.txt; holding the direct FORWARD until the dense forward is through as well: 1.184 alone,
  // 1.20 together).  The loss finalize follows the direct backward on its stream, behind a second event for the dense
  // chain's row pass.
  const bool gated = sc.open && sc.gated;
  int rc = gated ? (int)hipEventRecord(sc.side->gate, st) : 0;   // (behind the dense forward, in front of its row pass)
  if (!rc && !(dbg_mask() & (1 << 29))) {
    if (classes) {
      GrowParams gd = g;   // the dense-tile rows
      gd.only = 1;
      rc = launch_grad_rows(gd, p.ks, p.kw, sc.dense());
      GrowParams gs = g;   // the plan's sparse list; its criteria sums behind the first pass's
      gs.only = 2;
      gs.grid_cap = 4096;
      gs.tm_hdr = x.pv.dense_hdr;
      gs.tm_slots = 0;
      gs.sparse_order = x.pv.sparse_order;
      gs.partials = p.partials + 2 * (size_t)grow_grid(p.n_host);
      if (!rc) rc = launch_grad_rows(gs, p.ks, p.kw, sc.direct());
    } else {
      rc = launch_grad_rows(g, p.ks, p.kw, st);
    }
  }
  if (!rc && n_tm > 0) rc = (dbg_mask() & (1 << 29)) ? 0 : launch_rows_tm(tm_rows_params(p, x), p.ks, p.kw, st);
  if (rc || !p.grad) return rc;   // (two chains still forked: the entry point joins them)
  if (p.gfix && !x.apriori) {
    rc = launch_grad_fix_reduce(x.gmax_part, (int)grow_grid(p.n_host) + rows_tm_parts(n_tm), p.gfix, n_fix, st);
    if (rc) return rc;
  }
  const DenseBwdParams d = dense_bwd_params(p, x);
  if (gated) {   // the direct backward waits for the dense FORWARD only; the finalize, behind it, for the dense row pass
    rc = (int)hipStreamWaitEvent(sc.direct(), sc.side->gate, 0);
    if (!rc) rc = (int)hipEventRecord(sc.side->gate2, sc.dense());
  }
  if (!sc.open) {   // fork / join around this pass
    fork_side(sc, dbg_mask() & ((1 << 27) | (1 << 28)));
    // (with a side stream the loss finalize -- it needs ssg_grad_rows' partial sums only -- is queued there ahead of
    // that stream's kernel, off the critical path (7 us); on one stream it rides in the last workgroup of
    // grad_fix_flush (det_end, round 5) or, without a fixed-point buffer, follows the backward)
    if (!rc && fin && sc.open) {
      rc = launch_loss_finalize(*fin, sc.side->side);
      if (!rc) *fin_done = true;
    }
  }
  if (!rc && !(dbg_mask() & (1 << 27))) rc = launch_bwd_dense(d, p.ks, p.kw, p.C, sc.dense());
  if (!rc && !(dbg_mask() & (1 << 28))) {
    BwdParams s = p;
    s.mode = GRAD_D;
    s.gin = d.G;
    s.order = x.pv.sparse_order;
    s.n_dev = x.pv.n_sparse;
    s.partials = nullptr;
    s.rows_hint = sc.rows_hint;
    rc = launch_bwd(s, sc.direct());
  }
  if (!rc && gated && fin) {   // (both passes' criteria sums are complete behind gate2)
    rc = (int)hipStreamWaitEvent(sc.direct(), sc.side->gate2, 0);
    if (!rc) rc = launch_loss_finalize(*fin, sc.direct());
    if (!rc) *fin_done = true;
  }
  const int rcj = join_side(sc);
  return rc ? rc : rcj;
}

// Deterministic mode: the kernels add into the caller's zeroed fixed-point buffer; one flush folds it into grad.
// the fixed-point gradient sums of a (B,C,H,W) image and, behind them, the word with the bound of |G| (8 sums' room)
static size_t grad_fix_bytes(int B, int C, int H, int W) { return sizeof(long long) * ((size_t)B * C * H * W + 8); }
static int det_begin(const Call &c, const BwdParams &p, hipStream_t st) {
  if (!p.gfix || c.fix_zeroed) return 0;   // (the fused step: cleared by the edge-list builder's first kernel)
  return (int)hipMemsetAsync(p.gfix, 0, grad_fix_bytes(p.B, p.C, p.H, p.W), st);
}
static int det_end(const Call &c, const BwdParams &p, hipStream_t st, const LossFinalize *fin = nullptr, bool *fin_done = nullptr) {
  if (!p.gfix) return 0;
  const int rc = launch_grad_fix_flush(p.gfix, p.grad, (size_t)p.B * p.C * p.H * p.W, c.grad_is_output ? 1 : 0, st, fin);
  if (!rc && fin && fin_done) *fin_done = true;
  return rc;
}

// ---- the reference operator with many positions: plan built inside the call -------------------------------------------
// similarity.h's interface has no workspace argument, so the plan's buffers come from a library-owned, stream-ordered
// memory pool (one per device, release threshold = never: after the first call an allocation is a free-list lookup).
// Measured (profiles/r4_operator_vs_plan.txt): the plan costs ~45 us per call and a handful of dense tiles are one
// resident round whatever their number, so the direct kernels in `pos` order win below ~10 k positions (0.134 vs 0.180
// ms forward at 4,820) and lose above (0.251 vs 0.197 ms at 18,417; forward + backward 0.733 vs 0.454).
constexpr int OP_PLAN_FROM_DEFAULT = 8192;
static std::atomic<int> g_op_plan_from{-1};
// positions from which a call takes the plan path (0x7fffffff = never); ssg_set_operator_plan_threshold
// (n <= 0: never)
static int op_plan_from() {
  return setting(g_op_plan_from, [] { const int v = env_int("SSG_OP_PLAN_FROM", OP_PLAN_FROM_DEFAULT); return v <= 0 ? 0x7fffffff : v; });
}

static hipMemPool_t op_pool() {
  static std::mutex mu;
  static hipMemPool_t tab[MAXDEV] = {};
  static bool failed[MAXDEV] = {};
  const int dev = current_device_slot();
  if (dev < 0) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!tab[dev] && !failed[dev]) {
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
      failed[dev] = true;
      (void)hipGetLastError();
      return nullptr;
    }
    unsigned long long keep = ~0ull;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    tab[dev] = pool;
  }
  return tab[dev];
}

struct OpPlan {
  char *base = nullptr;
  uint8_t *mask = nullptr;
  int *edges = nullptr, *counts = nullptr, *rank = nullptr, *plan = nullptr, *perm = nullptr, *dup = nullptr, *ndup = nullptr;
  void *escratch = nullptr, *bscratch = nullptr;
};

// true: the call qualifies for the plan path (enough positions, a size with shared-term kernels, not inside a stream capture)
// (the forward gains less from the shared-term kernel than the backward -- measured at 18,417 positions: forward 0.196 ms
// direct / 0.231 with the plan, backward 0.462 / 0.258 -- so it takes the plan from three times as many positions)
enum OpPass { OP_FORWARD, OP_BACKWARD };
static bool op_wants_plan(int mc, int ks, int kw, int C, hipStream_t st, OpPass pass) {
  const long from = (long)op_plan_from() * (pass == OP_FORWARD && op_plan_from() > 1 ? 3 : 1);
  if (from >= 0x7fffffffL || (long)mc < from || !dense_supported(ks, kw, C) || !dense_bwd_supported(ks, kw, C) || !grow_supported(ks, kw)) return false;
  if (!stream_capturing(st)) return true;
  (void)hipGetLastError();
  return false;
}

// rank map, plan and duplicate list of `pos` (padded coordinates on a (Hp, Wp) image), everything relabelled to the
// caller's row numbers.  rc != 0 or o.base == nullptr: fall back to the direct path.
static int op_plan_build(const int *pos, int mc, int ks, int Hp, int Wp, size_t bwd_scratch_bytes, hipStream_t st, OpPlan &o) {
  hipMemPool_t pool = op_pool();
  if (!pool) return 0;
  const size_t npix = (size_t)Hp * Wp;
  Carver c;
  const size_t o_mask = c.take(npix), o_edges = c.take(sizeof(int) * 3 * (size_t)mc), o_counts = c.take(sizeof(int) * 8),
               o_rank = c.take(sizeof(int) * npix), o_plan = c.take(fwd_plan_bytes(1, Hp, Wp, mc)),
               o_perm = c.take(sizeof(int) * (size_t)mc), o_dup = c.take(sizeof(int) * (size_t)mc), o_ndup = c.take(sizeof(int) * 4),
               o_es = c.take(edge_scratch_bytes(1, Hp, Wp)), o_bs = c.take(bwd_scratch_bytes);
  void *base = nullptr;
  if (hipMallocFromPoolAsync(&base, c.end, pool, st) != hipSuccess || !base) {
    (void)hipGetLastError();
    return 0;
  }
  o.base = (char *)base;
  o.mask = (uint8_t *)(o.base + o_mask);
  o.edges = (int *)(o.base + o_edges);
  o.counts = (int *)(o.base + o_counts);
  o.rank = (int *)(o.base + o_rank);
  o.plan = (int *)(o.base + o_plan);
  o.perm = (int *)(o.base + o_perm);
  o.dup = (int *)(o.base + o_dup);
  o.ndup = (int *)(o.base + o_ndup);
  o.escratch = o.base + o_es;
  o.bscratch = bwd_scratch_bytes ? o.base + o_bs : nullptr;
  int rc = (int)hipMemsetAsync(o.mask, 0, npix, st);
  if (!rc) rc = (int)hipMemsetAsync(o.perm, 0xff, sizeof(int) * (size_t)mc, st);
  if (!rc) rc = (int)hipMemsetAsync(o.ndup, 0, sizeof(int) * 4, st);
  if (!rc) rc = launch_pos_to_mask(pos, mc, Hp, Wp, o.mask, st);
  if (!rc)
    rc = launch_edge_list(o.mask, 1, 1, 1, Hp, Wp, 0, 0.f, o.edges, mc, o.counts, o.rank, nullptr, o.plan, dense_threshold(),
                          dense_tile_rows(ks), o.escratch, nullptr, 0, nullptr, 0, nullptr, 0, st);
  if (!rc) rc = launch_pos_relabel(pos, mc, Hp, Wp, o.rank, o.perm, o.dup, o.ndup, o.plan, o.plan + fwd_plan_order_offset(1, Hp, Wp), st);
  return rc;
}

static int op_plan_free(OpPlan &o, hipStream_t st) {
  if (!o.base) return 0;
  const int rc = (int)hipFreeAsync(o.base, st);
  o.base = nullptr;
  return rc;
}

static bool split_ok(const Call &c) {
  return c.rank && c.plan && c.scratch && grow_supported(c.ks, c.kw) && dense_bwd_supported(c.ks, c.kw, c.C) &&
         !(dbg_mask() & (1 << 24));
}

extern "C" {

int ssg_abi_version(void) { return 6; }

const char *ssg_status_string(int status) {
  switch (status) {
    case 0: return "ok";
    case SSG_E_BADARG: return "ssg: bad argument (null pointer, even/non-positive kernel size, bad kind)";
    case SSG_E_TOOLARGE: return "ssg: search tile does not fit the 160 KiB LDS of a CU";
    case SSG_E_WORKSPACE: return "ssg: workspace too small";
    case SSG_E_IMAGESMALL: return "ssg: image side <= k_s/2, reflect padding undefined";
    case SSG_E_ALIGN: return "ssg: workspace / grad_fix / grad_sr of the fused step must be 16-byte aligned";
    case SSG_E_PLAN: return "ssg: a dense kernel was handed a plan cut for another tile height (k_s 25 vs 49); that launch did nothing";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "ssg: unknown status";
  }
}

int ssg_compute_similarity(const float *image, const int *pos, float *out, int mc, int psize, int ksize, int height,
                           int width, int channel, ssg_stream_t stream) {
  if (mc < 0 || !sizes_ok(psize, ksize) || channel <= 0 || height <= 0 || width <= 0) return SSG_E_BADARG;
  if (mc == 0) return 0;
  if (!image || !pos || !out) return SSG_E_BADARG;
  Call c;
  c.img = image;
  c.ssg = out;
  c.edges = pos;
  c.estride = 2;
  c.n_rows = mc;
  c.B = 1;
  c.C = channel;
  c.H = height;
  c.W = width;
  c.raw = 1;
  c.ks = psize;
  c.kw = ksize;
  const FwdParams p = fwd_params(c);
  hipStream_t st = (hipStream_t)stream;
  if (op_wants_plan(mc, psize, ksize, channel, st, OP_FORWARD)) {
    OpPlan o;
    int rc = op_plan_build(pos, mc, psize, height, width, 0, st, o);
    if (!rc && o.base) {
      // dense tiles -> shared-term kernel in raw mode, the rest (the plan's tile order, caller's row numbers) -> the
      // direct kernels, duplicates of a position -> a direct launch of their own
      c.rank = o.rank;
      c.plan = o.plan;
      const PlanView pv = plan_view(c.plan, 1, height, width);
      const DenseParams d = dense_params(c, pv);
      Schedule sc = schedule(st, psize, Chains::never);
      fork_side(sc);
      rc = launch_fwd_dense(d, psize, ksize, channel, sc.dense());
      FwdParams q = p;
      q.order = pv.sparse_order;
      q.n_dev = pv.n_sparse;
      if (!rc) rc = launch_fwd(q, sc.direct());
      const int rcj = join_side(sc);
      if (!rc) rc = rcj;
      q.order = o.dup;
      q.n_dev = o.ndup;
      if (!rc) rc = launch_fwd(q, st);
    }
    const bool used = o.base != nullptr;
    const int rcf = op_plan_free(o, st);
    if (used || rc) return rc ? rc : rcf;
  }
  return launch_fwd(p, st);
}

int ssg_compute_similarity_backward(const float *image, const float *grads, const int *pos, float *image_grads,
                                    int mc, int psize, int ksize, int height, int width, int channel,
                                    ssg_stream_t stream) {
  if (mc < 0 || !sizes_ok(psize, ksize) || channel <= 0 || height <= 0 || width <= 0) return SSG_E_BADARG;
  if (mc == 0) return 0;
  if (!image || !grads || !pos || !image_grads) return SSG_E_BADARG;
  Call c;
  c.img = image;
  c.grad = image_grads;
  c.gin = grads;
  c.edges = pos;
  c.estride = 2;
  c.n_rows = mc;
  c.B = 1;
  c.C = channel;
  c.H = height;
  c.W = width;
  c.ks = psize;
  c.kw = ksize;
  const BwdParams p = bwd_params(c, GRAD_D);
  hipStream_t st = (hipStream_t)stream;
  if (op_wants_plan(mc, psize, ksize, channel, st, OP_BACKWARD)) {
    OpPlan o;
    int rc = op_plan_build(pos, mc, psize, height, width, ssg_backward_scratch_bytes(mc, psize), st, o);
    if (!rc && o.base) {
      // the split backward in GRAD_D mode (`grads` ARE the G rows): border sums by ssg_grad_rows, dense tiles by the
      // shared-term kernel, the plan's sparse rows by the direct one; then the duplicates of a position on their own
      c.rank = o.rank;
      c.plan = o.plan;
      c.scratch = o.bscratch;
      Schedule sc = schedule(st, psize, Chains::never);
      rc = split_backward(c, p, sc);
      BwdParams q = p;
      q.order = o.dup;
      q.n_dev = o.ndup;
      if (!rc) rc = launch_bwd(q, st);
    }
    const bool used = o.base != nullptr;
    const int rcf = op_plan_free(o, st);
    if (used || rc) return rc ? rc : rcf;
  }
  return launch_bwd(p, st);
}

size_t ssg_edge_scratch_bytes(int B, int H, int W) { return edge_scratch_bytes(B, H, W); }

size_t ssg_forward_plan_bytes(int B, int H, int W, int capacity) { return fwd_plan_bytes(B, H, W, capacity); }

static int edge_list_impl(const void *mask, int mask_kind, int mask_channels, int B, int H, int W, int mask_stride,
                          float lap_threshold, int plan_ks, int *edges, int capacity, int *counts, int *rank_map,
                          int *tile_order, int *fwd_plan, void *scratch, void *zero_a, size_t zero_a_bytes, void *zero_b,
                          size_t zero_b_bytes, void *zero_c, size_t zero_c_bytes, ssg_stream_t stream) {
  if (!mask || !edges || !counts || !scratch || B <= 0 || H <= 0 || W <= 0 || capacity < 0 || mask_kind < 0 ||
      mask_kind > 2 || mask_channels <= 0 || ((tile_order || fwd_plan) && !rank_map))
    return SSG_E_BADARG;
  // (the plan is always built when asked for -- with threshold 0 it lists no dense tile and every row in its
  // direct order -- so that the kernels consuming it never depend on the process-wide threshold)
  return launch_edge_list(mask, mask_kind, mask_channels, B, H, W, mask_stride, lap_threshold, edges, capacity,
                          counts, rank_map, tile_order, fwd_plan, dense_threshold(), dense_tile_rows(plan_ks), scratch,
                          zero_a, zero_a_bytes, zero_b, zero_b_bytes, zero_c, zero_c_bytes, (hipStream_t)stream);
}

int ssg_edge_list(const void *mask, int mask_kind, int mask_channels, int B, int H, int W, int mask_stride,
                  float lap_threshold, int plan_ks, int *edges, int capacity, int *counts, int *rank_map,
                  int *tile_order, int *fwd_plan, void *scratch, ssg_stream_t stream) {
  return edge_list_impl(mask, mask_kind, mask_channels, B, H, W, mask_stride, lap_threshold, plan_ks, edges, capacity,
                        counts, rank_map, tile_order, fwd_plan, scratch, nullptr, 0, nullptr, 0, nullptr, 0, stream);
}

int ssg_edge_mask_laplacian(const float *gt, int B, int H, int W, float lap_threshold, int mask_stride,
                            uint8_t *mask_out, ssg_stream_t stream) {
  if (!gt || !mask_out || B <= 0 || H <= 0 || W <= 0) return SSG_E_BADARG;
  return launch_edge_mask(gt, B, H, W, lap_threshold, mask_stride, mask_out, (hipStream_t)stream);
}

static int map_forward_impl(const Call &c, Schedule &sc) {
  int rc = 0;
  if (call_ends(c, MAP_FORWARD, sc.st, rc)) return rc;
  FwdParams p = fwd_params(c);
  if (c.plan && c.rank && dense_supported(c.ks, c.kw, c.C)) {
    // dense tiles -> shared-term kernel; the rest (plan's own tile-major order) -> direct kernels
    const PlanView pv = plan_view(c.plan, c.B, c.H, c.W);
    const DenseParams d = dense_params(c, pv);
    if (c.row_scale && !c.row_scale_zeroed) {   // 0 = "this row is already normalised" (the rows of the direct kernels)
      const int rc0 = (int)hipMemsetAsync(c.row_scale, 0, sizeof(double) * 2 * (size_t)c.n_rows, sc.st);
      if (rc0) return rc0;
    }
    fork_side(sc, dbg_mask() & ((1 << 25) | (1 << 26)));   // (ssg_set_overlap)
    rc = (dbg_mask() & (1 << 25)) ? 0 : launch_fwd_dense(d, c.ks, c.kw, c.C, sc.dense());
    p.order = pv.sparse_order;
    p.n_dev = pv.n_sparse;
    p.rows_hint = sc.rows_hint;
    if (!rc && !(dbg_mask() & (1 << 26))) rc = launch_fwd(p, sc.direct());
    if (sc.chains) return rc;   // two chains: the backward's kernels follow on the same two streams (the caller joins)
    const int rcj = join_side(sc);
    return rc ? rc : rcj;
  }
  return launch_fwd(p, sc.st);
}

int ssg_map_forward(const float *img, const float *img2, int B, int C, int H, int W, const int *edges,
                    const int *tile_order, const int *rank_map, const int *fwd_plan, const int *n_edges_dev, int n_rows,
                    int ks, int kw, float sigma, float eps, int generalization, float *ssg, float *ssg2,
                    double *row_scale, ssg_stream_t stream) {
  Call c;
  c.img = img;
  c.img2 = img2;
  c.B = B;
  c.C = C;
  c.H = H;
  c.W = W;
  c.edges = edges;
  c.order = tile_order;
  c.rank = rank_map;
  c.plan = fwd_plan;
  c.n_dev = n_edges_dev;
  c.n_rows = n_rows;
  c.ks = ks;
  c.kw = kw;
  c.sigma = sigma;
  c.eps = eps;
  c.generalization = generalization;
  c.ssg = ssg;
  c.ssg2 = ssg2;
  c.row_scale = row_scale;
  Schedule sc = schedule((hipStream_t)stream, ks, Chains::never);
  return map_forward_impl(c, sc);
}

size_t ssg_backward_scratch_bytes(int n_rows, int ks) { return carve_backward_scratch(0, 0, 0, n_rows, ks, GRAD_S).end; }

int ssg_map_backward(const float *img, int B, int C, int H, int W, const int *edges, const int *tile_order,
                     const int *rank_map, const int *fwd_plan, const int *n_edges_dev, int n_rows, int ks, int kw,
                     float sigma, int generalization, const float *ssg, const float *grad_ssg, float *grad_img,
                     void *scratch, void *grad_fix, ssg_stream_t stream) {
  const hipStream_t st = (hipStream_t)stream;
  Call c;
  c.img = img;
  c.B = B;
  c.C = C;
  c.H = H;
  c.W = W;
  c.edges = edges;
  c.order = tile_order;
  c.rank = rank_map;
  c.plan = fwd_plan;
  c.n_dev = n_edges_dev;
  c.n_rows = n_rows;
  c.ks = ks;
  c.kw = kw;
  c.sigma = sigma;
  c.generalization = generalization;
  c.ssg = const_cast<float *>(ssg);   // (GRAD_S: S saved, read only)
  c.gin = grad_ssg;
  c.grad = grad_img;
  c.scratch = scratch;
  c.grad_fix = grad_fix;
  int rc = 0;
  if (call_ends(c, MAP_BACKWARD, st, rc)) return rc;
  const BwdParams p = bwd_params(c, GRAD_S);
  rc = det_begin(c, p, st);
  if (rc) return rc;
  if (split_ok(c)) {
    Schedule sc = schedule(st, ks, Chains::never);
    rc = split_backward(c, p, sc);
  } else {
    if (p.gfix) rc = launch_grad_fix_bound(p, st);
    if (!rc) rc = launch_bwd(p, st);
  }
  return rc ? rc : det_end(c, p, st);
}

size_t ssg_grad_fix_bytes(int B, int C, int H, int W) { return grad_fix_bytes(B, C, H, W); }

size_t ssg_loss_scratch_bytes(int B, int H, int W, int n_rows, int ks) {
  return carve_backward_scratch(B, H, W, n_rows, ks, GRAD_LOSS).end;
}

static int loss_backward(const Call &c, Schedule &sc) {
  const hipStream_t st = sc.st;
  int rc = 0;
  if (call_ends(c, LOSS_BACKWARD, st, rc)) return rc;
  BwdParams p = bwd_params(c, GRAD_LOSS);
  const bool split = split_ok(c);
  if (c.row_scale && !split) return SSG_E_BADARG;  // only ssg_grad_rows rescales
  rc = det_begin(c, p, st);
  if (rc) return rc;
  // criteria sums: the backward kernel's workgroups, or ssg_grad_rows' -- per-class row passes: two sets of
  // grow_grid(n_rows) slots -- and ssg_rows_tm's
  // (ssg_grad_rows' slots come in sets of grow_grid(n_rows), live up to the device's row count: LossFinalize::set_size)
  const int n_tm = split ? split_tm_tiles(p, c.tm) : 0;
  const int nparts = !split ? (int)bwd_grid(p)
                            : (split_row_classes(p, n_tm) ? 2 : 1) * (int)grow_grid(c.n_rows) + rows_tm_parts(n_tm);
  const int set_size = split && n_tm == 0 ? (int)grow_grid(c.n_rows) : 0;
  const LossFinalize fin{p.partials, nparts, c.n_dev, c.n_rows, c.ks * c.ks, c.w_l1, c.w_kl, c.loss_out, c.nan_on_overflow ? 1 : 0, set_size};
  bool fin_done = false;
  if (split) {
    rc = split_backward(c, p, sc, &fin, &fin_done);
  } else {
    p.fix_inline = p.gfix ? 1 : 0;   // (GRAD_LOSS: the backward kernel derives the a-priori scale itself -- one launch less)
    rc = launch_bwd(p, st);
  }
  // (the finalize rides in the flush's last workgroup when its partial sums are few -- 256 threads play its 1,024 lanes: C5's
  // 70 k partials took 30 us there against 10 + 11 as two launches)
  // (sets of slots are read up to the device's row count only: what counts is their live prefix, bounded by the host's)
  const int fin_reads = set_size > 0 ? (nparts / set_size) * ((c.n_rows + 3) / 4) : nparts;
  if (!rc) rc = det_end(c, p, st, (fin_done || fin_reads > 8192) ? nullptr : &fin, &fin_done);
  if (rc || fin_done) return rc;
  return launch_loss_finalize(fin, st);
}

int ssg_loss_backward(const float *sr, int B, int C, int H, int W, const int *edges, const int *tile_order,
                      const int *rank_map, const int *fwd_plan, const int *n_edges_dev, int n_rows, int ks, int kw,
                      float sigma, int generalization,
                      float *ssg_sr, float *ssg_gt, float w_l1, float w_kl, const float *upstream,
                      float *loss_out, float *grad_sr, void *scratch, void *grad_fix, const double *row_scale,
                      int rows_are_scratch, ssg_stream_t stream) {
  Call c;
  c.img = sr;
  c.B = B;
  c.C = C;
  c.H = H;
  c.W = W;
  c.edges = edges;
  c.order = tile_order;
  c.rank = rank_map;
  c.plan = fwd_plan;
  c.n_dev = n_edges_dev;
  c.n_rows = n_rows;
  c.ks = ks;
  c.kw = kw;
  c.sigma = sigma;
  c.generalization = generalization;
  c.ssg = ssg_sr;
  c.ssg2 = ssg_gt;
  c.w_l1 = w_l1;
  c.w_kl = w_kl;
  c.upstream = upstream;
  c.loss_out = loss_out;
  c.grad = grad_sr;
  c.scratch = scratch;
  c.grad_fix = grad_fix;
  c.row_scale = const_cast<double *>(row_scale);   // (a backward only reads the row scales)
  c.rows_scratch = rows_are_scratch != 0;
  Schedule sc = schedule((hipStream_t)stream, ks, Chains::possible);
  const int rc = loss_backward(c, sc);
  const int rcj = join_side(sc);   // (an error between the row passes' fork and the backward's join leaves it open)
  return rc ? rc : rcj;
}

// two row-major regions (sr, gt); at k_s = 49 two tile-major regions of the same size behind them
static size_t rows_region_bytes(int capacity, int ks) { return align_up(sizeof(float) * rows_of(capacity) * ks * ks, 256); }
// (a tile-major region: capacity / 128 slots and a spare one for the short strips of ssg_fwd_strip)
static size_t tm_region_bytes(int capacity, int ks) {
  return align_up(sizeof(float) * (rows_of(capacity) / TM_PX + 1) * ks * ks * TM_PX, 256);
}
size_t ssg_loss_tm_bytes(int capacity, int ks) { return ks == 49 ? 2 * tm_region_bytes(capacity, ks) : 0; }
size_t ssg_loss_rows_bytes(int capacity, int ks) {
  return 2 * rows_region_bytes(capacity, ks) + ssg_loss_tm_bytes(capacity, ks);
}

// carving of the fused call's workspace (one place: the size, loss_fwd_bwd_impl and ssg_loss_workspace_layout use it)
struct LossWorkspace {
  size_t edges, rank, order, plan, escratch, lscratch, row_scale, base_bytes, rows[2], tm[2];
  int tm_slots;
};
static LossWorkspace carve_workspace(int B, int H, int W, int capacity, int ks, bool fused = true) {
  LossWorkspace w{};
  Carver c;
  w.edges = c.take(sizeof(int) * 3 * rows_of(capacity));
  w.rank = c.take(sizeof(int) * (size_t)B * H * W);
  w.order = c.take(sizeof(int) * rows_of(capacity));
  w.plan = c.take(fwd_plan_bytes(B, H, W, capacity));
  w.escratch = c.take(edge_scratch_bytes(B, H, W));
  w.lscratch = c.take(ssg_loss_scratch_bytes(B, H, W, capacity, ks));
  w.row_scale = c.take(2 * sizeof(double) * rows_of(capacity));
  w.base_bytes = c.end;
  const size_t region = rows_region_bytes(capacity, ks);
  w.rows[0] = w.base_bytes;
  w.rows[1] = w.rows[0] + region;
  if (ks == 49) {   // (a materialising call has no row-major scratch rows: the tile-major regions follow the base)
    w.tm[0] = fused ? w.rows[1] + region : w.base_bytes;
    w.tm[1] = w.tm[0] + tm_region_bytes(capacity, ks);
    w.tm_slots = capacity / TM_PX;
  }
  if (!fused) w.rows[0] = w.rows[1] = 0;
  return w;
}

size_t ssg_loss_workspace_bytes(int B, int H, int W, int capacity, int ks) {
  return carve_workspace(B, H, W, capacity, ks).base_bytes;
}

int ssg_loss_workspace_layout(int B, int H, int W, int capacity, int ks, int fused, size_t out[9]) {
  if (!out || B <= 0 || H <= 0 || W <= 0 || capacity <= 0 || ks <= 0) return SSG_E_BADARG;
  const LossWorkspace w = carve_workspace(B, H, W, capacity, ks, fused != 0);
  out[0] = w.edges;
  out[1] = w.rank;
  out[2] = w.plan;
  out[3] = w.row_scale;
  out[4] = w.rows[0];
  out[5] = w.rows[1];
  out[6] = w.tm[0];
  out[7] = w.tm[1];
  out[8] = (size_t)w.tm_slots;
  return 0;
}

// ssg_loss_fwd_bwd adds into the caller's gradient, ssg_loss_step writes it
enum class GradientIs { accumulated, output };
static int loss_fwd_bwd_impl(const float *sr, const float *gt, const void *mask, int mask_kind, int mask_channels, int B,
                             int C, int H, int W, int ks, int kw, float sigma, float eps, int generalization, float w_l1,
                             float w_kl, int mask_stride, float lap_threshold, int capacity, float *ssg_sr,
                             float *ssg_gt, int *counts, float *loss_out, float *grad_sr, void *workspace,
                             size_t workspace_bytes, void *grad_fix, GradientIs gradient, ssg_stream_t stream) {
  if (!sr || !gt || !counts || !loss_out || !workspace || capacity <= 0) return SSG_E_BADARG;
  if ((ssg_sr == nullptr) != (ssg_gt == nullptr)) return SSG_E_BADARG;
  if (mask_kind != 2 && !mask) return SSG_E_BADARG;
  // fused step (no SSG output): the rows are the engine's scratch, behind the regular workspace
  const bool fused = ssg_sr == nullptr;
  const LossWorkspace lw = carve_workspace(B, H, W, capacity, ks, fused);
  const size_t base_bytes = lw.base_bytes;
  if (workspace_bytes < base_bytes + (fused ? ssg_loss_rows_bytes(capacity, ks) : 0)) return SSG_E_WORKSPACE;
  // the edge-list builder's first kernel clears the row scales, the fixed-point sums and (ssg_loss_step) the gradient
  // with 16-byte stores: offset views of a larger buffer must keep that alignment (include/ssg_hip.h)
  if ((((uintptr_t)workspace) | ((uintptr_t)grad_fix) | ((uintptr_t)grad_sr)) & 15) return SSG_E_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  const bool grad_is_output = gradient == GradientIs::output;
  char *ws = (char *)workspace;
  int *edges = (int *)(ws + lw.edges);
  int *rank = (int *)(ws + lw.rank);
  Call c;
  c.img = sr;
  c.img2 = gt;
  c.B = B;
  c.C = C;
  c.H = H;
  c.W = W;
  c.edges = edges;
  c.rank = rank;
  c.n_dev = counts;
  c.n_rows = capacity;
  c.ks = ks;
  c.kw = kw;
  c.sigma = sigma;
  c.eps = eps;
  c.generalization = generalization;
  c.w_l1 = w_l1;
  c.w_kl = w_kl;
  c.ssg = fused ? (float *)(ws + lw.rows[0]) : ssg_sr;
  c.ssg2 = fused ? (float *)(ws + lw.rows[1]) : ssg_gt;
  c.loss_out = loss_out;
  c.grad = grad_sr;
  c.grad_fix = grad_fix;
  c.scratch = ws + lw.lscratch;
  c.rows_scratch = fused;
  c.grad_is_output = grad_is_output;
  c.nan_on_overflow = true;
  // tile-major rows: always in the fused step; in a materialising call when the caller's workspace has room for the
  // two regions (ssg_loss_tm_bytes) -- ssg_rows_tm_mat then writes the normalised SSG rows from them
  // (ssg_fwd_strip addresses a region with 32-bit ELEMENT offsets: regions of 2^32 floats = 16 GB and more -- from 1.78 M
  // rows per call -- stay on row-major rows)
  if (ks == 49 && kw == 13 && C == 3 && generalization && tile_major_enabled() &&
      (size_t)(lw.tm_slots + 1) * (size_t)(ks * ks) * TM_PX < (1ull << 32) &&
      (fused || workspace_bytes >= base_bytes + ssg_loss_tm_bytes(capacity, ks))) {
    c.tm.rows[0] = (float *)(ws + lw.tm[0]);
    c.tm.rows[1] = (float *)(ws + lw.tm[1]);
    c.tm.slots = lw.tm_slots;
  }
  // the mask of the call (kind 2: the Laplacian of gt's three channels), the gradient's bytes and whether the
  // deterministic sums are in use: the tiny path and the general path both take them from here
  const void *mask_src = mask_kind == 2 ? (const void *)gt : mask;
  const int mask_ch = mask_kind == 2 ? 3 : mask_channels;
  const size_t grad_bytes = sizeof(float) * (size_t)B * C * H * W, fix_bytes = grad_fix_bytes(B, C, H, W);
  // the fixed-point gradient sums start at zero: cleared by the edge-list builder's first kernel
  const bool zero_fix = grad_fix && grad_sr;
  // a gradient that is an OUTPUT: the deterministic flush assigns it; with fp32 atomics it is cleared by the builder's
  // first kernel (whole 16-byte granules; a tail of < 16 bytes by the memset below)
  void *const zero_grad = (grad_is_output && grad_sr && !zero_fix) ? (void *)grad_sr : nullptr;
  c.fix_zeroed = zero_fix;
  // small (11,5) steps: one workgroup builds the edge list, one workgroup per edge pixel does the rest (ssg_tiny.hip)
  if (g_tiny_step.load(std::memory_order_relaxed) && tiny_step_supported(ks, kw, C, capacity) && tiny_edge_list_ok(B, H, W) &&
      B > 0 && H > ks / 2 && W > ks / 2 && mask_kind >= 0 && mask_kind <= 2 && (mask_kind == 2 || mask_channels > 0)) {
    int *ticket = (int *)(ws + lw.escratch);
    const int rc = launch_tiny_edge_list(mask_src, mask_kind, mask_ch, B, H, W, mask_stride, lap_threshold, edges, capacity, counts,
                                         rank, ticket, 16, zero_fix ? grad_fix : nullptr, fix_bytes, zero_grad, grad_bytes, st);
    if (rc) return rc;
    return launch_tiny_step(tiny_params(c, ticket), C, st);
  }
  int *order = (int *)(ws + lw.order);
  int *plan = (int *)(ws + lw.plan);
  void *escratch = ws + lw.escratch;
  double *row_scale = (double *)(ws + lw.row_scale);
  c.plan = plan;
  // (deferred normalisation wherever the split backward -- whose ssg_grad_rows pass rescales -- follows)
  const bool defer = split_ok(c) && dense_supported(ks, kw, C);
  if (!defer) c.tm.slots = 0;
  // with the plan in use every kernel takes its job order from it: the full tile-major order is not built (3 launches)
  if (defer) order = nullptr;
  // kernel sizes without shared-term kernels ((11,5), other channel counts) have no use for a plan: not built
  // (4 launches of 4-5 us each: BASELINE's C1 step is 14 dependent launches long)
  if (!dense_supported(ks, kw, C)) plan = nullptr;
  c.order = order;
  c.plan = plan;
  // the row scales start at zero like the fixed-point sums: cleared by the edge-list builder's first kernel
  // (16-byte granules: both sizes are multiples of 16)
  c.row_scale = defer ? row_scale : nullptr;
  c.row_scale_zeroed = defer;
  // the schedule of the whole step, from the hint the builder below has not overwritten yet: two chains where there is a
  // gradient and the sizes have a dense / direct split
  Schedule sc = schedule(st, ks, defer && grad_sr ? Chains::possible : Chains::never);
  const size_t rs_bytes = 2 * sizeof(double) * (size_t)capacity;
  int rc = edge_list_impl(mask_src, mask_kind, mask_ch, B, H, W, mask_stride, lap_threshold, ks, edges, capacity, counts, rank,
                          order, plan, escratch, c.row_scale, rs_bytes, zero_fix ? grad_fix : nullptr, fix_bytes, zero_grad,
                          grad_bytes, stream);
  if (!rc && zero_grad && (grad_bytes & 15))
    rc = (int)hipMemsetAsync((char *)grad_sr + (grad_bytes & ~(size_t)15), 0, grad_bytes & 15, st);
  if (rc) return rc;
  rc = map_forward_impl(c, sc);
  if (!rc) rc = loss_backward(c, sc);
  const int rcj = join_side(sc);   // (an error between the forward's fork and the backward's join leaves it open)
  return rc ? rc : rcj;
}

int ssg_loss_fwd_bwd(const float *sr, const float *gt, const void *mask, int mask_kind, int mask_channels, int B,
                     int C, int H, int W, int ks, int kw, float sigma, float eps, int generalization, float w_l1,
                     float w_kl, int mask_stride, float lap_threshold, int capacity, float *ssg_sr, float *ssg_gt,
                     int *counts, float *loss_out, float *grad_sr, void *workspace, size_t workspace_bytes,
                     void *grad_fix, ssg_stream_t stream) {
  return loss_fwd_bwd_impl(sr, gt, mask, mask_kind, mask_channels, B, C, H, W, ks, kw, sigma, eps, generalization, w_l1,
                           w_kl, mask_stride, lap_threshold, capacity, ssg_sr, ssg_gt, counts, loss_out, grad_sr,
                           workspace, workspace_bytes, grad_fix, GradientIs::accumulated, stream);
}

int ssg_loss_step(const float *sr, const float *gt, const void *mask, int mask_kind, int mask_channels, int B, int C,
                  int H, int W, int ks, int kw, float sigma, float eps, int generalization, float w_l1, float w_kl,
                  int mask_stride, float lap_threshold, int capacity, float *ssg_sr, float *ssg_gt, int *counts,
                  float *loss_out, float *grad_sr, void *workspace, size_t workspace_bytes, void *grad_fix,
                  ssg_stream_t stream) {
  return loss_fwd_bwd_impl(sr, gt, mask, mask_kind, mask_channels, B, C, H, W, ks, kw, sigma, eps, generalization, w_l1,
                           w_kl, mask_stride, lap_threshold, capacity, ssg_sr, ssg_gt, counts, loss_out, grad_sr,
                           workspace, workspace_bytes, grad_fix, GradientIs::output, stream);
}

int ssg_operator_pool_trim(void) {
  hipMemPool_t pool = op_pool();
  return pool ? (int)hipMemPoolTrimTo(pool, 0) : 0;
}

int ssg_set_operator_plan_threshold(int positions) {
  const int prev = op_plan_from();
  g_op_plan_from.store(positions > 0 ? positions : 0x7fffffff, std::memory_order_relaxed);
  return prev;
}

int ssg_device_status(ssg_stream_t stream) {
  int *w = device_status_word();
  if (!w) return 0;
  int v = 0;
  int rc = (int)hipMemcpyAsync(&v, w, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (!rc && v) rc = (int)hipMemsetAsync(w, 0, sizeof(int), (hipStream_t)stream);
  if (!rc) rc = (int)hipStreamSynchronize((hipStream_t)stream);
  if (rc) return rc;
  return (v & 1) ? SSG_E_PLAN : 0;
}

const char *ssg_kernel_name(int ks, int kw, int backward) {
  if (!backward && ks == 25 && kw == 9 && dense_threshold() > 0)
    return "ssg_fwd_dense<25,9,3>+ssg_fwd_tiled<Geo<25,9,5,128>,merged|single>";
  return backward ? bwd_kernel_name(ks, kw) : fwd_kernel_name(ks, kw);
}

}  // extern "C"
