// The tally sink of the threshold profiles (profile_raw.hip, profile_levels.hip): the top-k kernels with this object in
// place of TopLists (top_k_lists.hpp) count the hits of a whole ladder of thresholds t[0] < ... < t[T-1] (T <= 64) and
// keep the best score per left and per right item, instead of per-row lists.  Same interface (eff, beats, offer_lanes,
// group_of, changes, flush), so no kernel body exists twice.
//
//   * no floor: eff() is the threshold the kernel was given -- t[0] -- and beats() is always true; `changes` never
//     moves, so the class walk and every bound prune against t[0] only;
//   * the ladder is "one threshold per lane": lane k holds t[k] and the number of offered scores >= t[k].  An offer of up
//     to 64 scores walks the ladder upwards with one ballot per step (the exact double comparison, no margin) and stops at
//     the first threshold no lane reaches: pairs[k] itself is counted, the suffix sum of the bins never has to be
//     formed.  No LDS, no dynamically indexed registers; the wave adds its counts to `pairs` once, at the end;
//   * left_best: row g's best so far sits in lane g; a wave-wide max is only formed when some lane beats it.  A left
//     row belongs to one wave: a plain vector store at the end;
//   * right_best: a lane sees the same right row for all of the wave's G rows, so it folds them into one pending value
//     and publishes it with ONE 64-bit atomic max when it moves on to the next right row -- and only when a relaxed
//     load says the stored value is smaller (the stored value only grows, so a stale load costs an atomic, never a
//     result).  Scores are >= 0, so their bit patterns order like the values; the word holds bits + 1 and 0 means "no
//     hit" (a score of 0.0 stays distinguishable); tally_finish_kernel turns the words into doubles;
//   * counts are integers, bests are maxima: the results do not depend on scheduling.
#pragma once
#include "top_k_lists.hpp"

namespace nsm {

constexpr int kTallyMaxT = kWave;  // one threshold per lane

// What a tally kernel gets besides its tables (by value: the ladder travels in the kernel arguments).
struct TallyOut {
  double t[kTallyMaxT];            // the ladder, +inf beyond n
  int32_t n;                       // T
  unsigned long long* pairs;       // [T]
  double* left_best;               // by left caller id, -1.0 where the call found nothing
  unsigned long long* right_bits;  // by right caller id: bits of the best score + 1, 0 = none (right_best in the making)
};

struct ScoreTally {
  using Extra = TallyOut;
  static constexpr int changes = 0;  // no floor ever moves

  unsigned long long* pairs;
  double* left_best;
  unsigned long long* right_bits;
  int n;
  int lane;
  double t_v;                      // lane k: t[k]
  unsigned long long cnt_v = 0;    // lane k: offered scores >= t[k]
  double best_v = -1.0;            // lane g: best score of row g
  int id_v = 0;                    // lane g: caller id of row g (valid once best_v >= 0)
  int pend_j = -1;                 // this lane's right row with an unpublished best
  double pend_s = 0.0;

  __device__ static ScoreTally open(nsm_hit*, int32_t*, int, int, int lane, const TallyOut& o) {
    return ScoreTally{o.pairs, o.left_best, o.right_bits, o.n, lane, o.t[lane]};
  }

  __device__ double eff(int, double threshold) const { return threshold; }
  __device__ bool beats(int, double, int) const { return true; }
  __device__ static int group_of(const int32_t*, int) { return 0; }

  __device__ void publish() {
    if (pend_j < 0) return;
    const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(pend_s)) + 1ull;
    unsigned long long* slot = right_bits + pend_j;
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < word) atomicMax(slot, word);
  }

  // lanes with `ok` hold a hit (s, j) of row g, whose caller id is i (wave-uniform call, all lanes enabled)
  __device__ void offer_lanes(int g, bool ok, double s, int i, int j, int) {
    if (!__ballot(ok)) return;
    for (int k = 0; k < n; ++k) {
      const unsigned long long reach = __ballot(ok && s >= readlane_f64(t_v, k));
      if (!reach) break;
      if (lane == k) cnt_v += static_cast<unsigned long long>(__popcll(reach));
    }
    if (__ballot(ok && s > readlane_f64(best_v, g))) {
      double m = ok ? s : -1.0;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) m = fmax(m, __shfl_xor(m, off));
      if (lane == g) { best_v = m; id_v = i; }
    }
    if (ok) {
      if (j != pend_j) {
        publish();
        pend_j = j;
        pend_s = s;
      } else {
        pend_s = fmax(pend_s, s);
      }
    }
  }

  __device__ void flush(int rows, nsm_hit*, unsigned long long*, unsigned long long* __restrict__ stats,
                        const unsigned long long (&st)[4]) {
    publish();
    if (lane < n && cnt_v) atomicAdd(pairs + lane, cnt_v);
    if (lane < rows && best_v >= 0.0) left_best[id_v] = best_v;
    wave_add_stats(stats, st, lane);
  }
};

// ------------------------------------------------------------------------------------------------------------- host side
// The outputs before and after the sweep.  Both kernels go by the tables' caller ids (`orig`), so the arrays need no
// length: an entry is written for every row of the table.  The ids of a table must be distinct (nsm_hip.h says so): one
// thread per row initialises / converts the row's entry, and a shared id would be converted twice.
static __global__ void tally_init_kernel(const int32_t* __restrict__ lorig, int n_left, const int32_t* __restrict__ rorig, int n_right,
                                  int n_thr, unsigned long long* __restrict__ pairs, double* __restrict__ left_best,
                                  unsigned long long* __restrict__ right_bits) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_thr) pairs[e] = 0ull;
  if (e < n_left) left_best[lorig[e]] = -1.0;
  if (e < n_right) right_bits[rorig[e]] = 0ull;
}

static __global__ void tally_finish_kernel(const int32_t* __restrict__ rorig, int n_right, unsigned long long* __restrict__ right_bits) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_right) return;
  unsigned long long* slot = right_bits + rorig[e];
  const unsigned long long word = *slot;
  *reinterpret_cast<double*>(slot) = word ? __longlong_as_double(static_cast<long long>(word - 1ull)) : -1.0;
}

// The ladder of a profile call: 1 .. 64 thresholds, strictly ascending, no NaN; null outputs.  Reported before any launch.
static int check_profile_args(const char* who, const double* thresholds, int32_t n_thresholds, const void* pairs,
                              const void* left_best, const void* right_best) {
  if (!thresholds || !pairs || !left_best || !right_best) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (n_thresholds < 1 || n_thresholds > kTallyMaxT) {
    set_error("%s: %d thresholds (1 .. %d)", who, n_thresholds, kTallyMaxT);
    return NSM_E_BADARG;
  }
  for (int k = 0; k < n_thresholds; ++k) {
    if (thresholds[k] != thresholds[k] || (k && !(thresholds[k - 1] < thresholds[k]))) {
      set_error("%s: thresholds must be strictly ascending numbers (entry %d)", who, k);
      return NSM_E_BADARG;
    }
  }
  return 0;
}

// One profile call around its sweep: initialise the outputs, `sweep(TallyOut)` launches the tally kernel, finish.
template <class F>
static int run_profile(const double* thresholds, int32_t n_thresholds, const int32_t* lorig, int n_left, const int32_t* rorig,
                       int n_right, uint64_t* pairs, double* left_best, double* right_best, hipStream_t s, F&& sweep) {
  TallyOut o;
  for (int k = 0; k < kTallyMaxT; ++k) o.t[k] = k < n_thresholds ? thresholds[k] : __builtin_inf();
  o.n = n_thresholds;
  o.pairs = reinterpret_cast<unsigned long long*>(pairs);
  o.left_best = left_best;
  o.right_bits = reinterpret_cast<unsigned long long*>(right_best);
  const int most = n_left > n_right ? (n_left > kTallyMaxT ? n_left : kTallyMaxT) : (n_right > kTallyMaxT ? n_right : kTallyMaxT);
  hipLaunchKernelGGL(tally_init_kernel, dim3((most + 255) / 256), dim3(256), 0, s, lorig, n_left, rorig, n_right, n_thresholds,
                     o.pairs, o.left_best, o.right_bits);
  if (int st = hip_status(hipGetLastError(), "tally_init_kernel launch")) return st;
  if (n_left && n_right) {
    if (int st = sweep(o)) return st;
  }
  if (n_right == 0) return 0;
  hipLaunchKernelGGL(tally_finish_kernel, dim3((n_right + 255) / 256), dim3(256), 0, s, rorig, n_right, o.right_bits);
  return hip_status(hipGetLastError(), "tally_finish_kernel launch");
}

}  // namespace nsm
