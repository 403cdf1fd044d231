// The RAW per-item queries of the token-set measures beside Jaccard (nsm_hip_measures.h): nsm_set_raw_top_k(_grouped),
// nsm_set_raw_profile, nsm_set_raw_floor_grid.  The sweep is the one of top_k_raw.hip -- jaccard_top_k_kernel
// (top_k_raw_kernels.hpp) with its three sinks -- instantiated ONCE more with RuntimeMeasure (set_measure.hpp) in place of
// the Jaccard quotient: score, the least intersection that matters, the class bound and the order of the class walk are
// the measure's, everything else (work split, lists, signatures, merge) is unchanged.  NSM_MEASURE_UNION is forwarded to
// the nsm_jaccard_* entry, whose instantiations are the only Jaccard ones in the library.
#include "floor_gate.hpp"
#include "score_tally.hpp"
#include "top_k_raw_kernels.hpp"

namespace nsm {

static TopJacParams set_params(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, int32_t k,
                               double threshold) {
  TopJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = k;
  p.measure = measure;
  p.threshold = threshold;
  return p;
}

// F: the kernel's instantiation for (W, PRUNE) as f(width tag, pruned tag) -> launch status
template <class F>
static int by_width_pruned(int width, bool prune, F&& f) {
  return by_width(width, [&](auto wc) { return prune ? f(wc, std::true_type{}) : f(wc, std::false_type{}); });
}

static int set_raw_top_k(const char* who, bool grouped, const nsm_set_table* left, const nsm_set_table* right,
                         int32_t measure, const int32_t* right_group, double threshold, int32_t k, uint32_t flags,
                         nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream) {
  if (!left || !right || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return grouped ? nsm_jaccard_raw_top_k_grouped(left, right, right_group, threshold, k, flags, out, out_count, stats, stream)
                   : nsm_jaccard_raw_top_k(left, right, threshold, k, flags, out, out_count, stats, stream);
  if (int st = check_k(who, k)) return st;
  if (grouped && !right_group) {
    set_error("%s: right_group is null", who);
    return NSM_E_BADARG;
  }
  if (int st = check_raw_set_query(who, left, right)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  const TopJacParams p = set_params(left, right, measure, keff, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, grouped)) return st;
  const int32_t* rg = grouped ? right_group : nullptr;
  return o.sc.release(by_width_pruned(left->width, prune, [&](auto wc, auto pruned) {
    return by_grouped(grouped, [&](auto gr) {
      constexpr bool G = decltype(gr)::value;
      hipLaunchKernelGGL((jaccard_top_k_kernel<decltype(wc)::value, decltype(pruned)::value, G, TopLists<G>, RuntimeMeasure>),
                         dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), 0, o.sc.s, left->ids, left->cnt, left->sig,
                         left->sig2, left->orig, right->ids, right->size_start, right->sig, right->sig2, right->orig,
                         o.sc.list, o.out, o.out_count, o.stats, p, rg, o.sc.glist, typename TopLists<G>::Extra{});
      return hip_status(hipGetLastError(), "set top-k kernel launch");
    });
  }));
}

// The profile and floor-grid launch: the sweep with sink S, whose argument is `o`.
template <class S>
static int launch_set_sweep(const char* what, const nsm_set_table* l, const nsm_set_table* r, bool prune, const TopJacParams& p,
                            const typename S::Extra& o, unsigned long long* stats, hipStream_t s) {
  return by_width_pruned(l->width, prune, [&](auto wc, auto pruned) {
    hipLaunchKernelGGL((jaccard_top_k_kernel<decltype(wc)::value, decltype(pruned)::value, false, S, RuntimeMeasure>),
                       dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), 0, s, l->ids, l->cnt, l->sig, l->sig2, l->orig,
                       r->ids, r->size_start, r->sig, r->sig2, r->orig, static_cast<nsm_hit*>(nullptr),
                       static_cast<nsm_hit*>(nullptr), static_cast<unsigned long long*>(nullptr), stats, p,
                       static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), o);
    return hip_status(hipGetLastError(), what);
  });
}

}  // namespace nsm

extern "C" int nsm_set_raw_top_k(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold,
                                 int32_t k, uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats,
                                 void* stream) {
  return nsm::set_raw_top_k("nsm_set_raw_top_k", false, left, right, measure, nullptr, threshold, k, flags, out, out_count,
                            stats, stream);
}

extern "C" int nsm_set_raw_top_k_grouped(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                                         const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                                         unsigned long long* out_count, uint64_t* stats, void* stream) {
  return nsm::set_raw_top_k("nsm_set_raw_top_k_grouped", true, left, right, measure, right_group, threshold, k, flags, out,
                            out_count, stats, stream);
}

extern "C" int nsm_set_raw_profile(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                                   const double* thresholds, int32_t n_thresholds, uint32_t flags, uint64_t* pairs,
                                   double* left_best, double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_raw_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_raw_profile(left, right, thresholds, n_thresholds, flags, pairs, left_best, right_best, stats, stream);
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_raw_set_query(who, left, right)) return st;
  const TopJacParams p = set_params(left, right, measure, 0, thresholds[0]);
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return launch_set_sweep<ScoreTally>("set profile kernel launch", left, right, prune, p, o, st64, s);
                     });
}

extern "C" int nsm_set_raw_floor_grid(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold,
                                      const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                                      uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_raw_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_raw_floor_grid(left, right, threshold, left_floor, right_floor, flags, hits, capacity, hit_count, stats,
                                      stream);
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_raw_set_query(who, left, right)) return st;
  const TopJacParams p = set_params(left, right, measure, 0, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  return launch_set_sweep<FloorGate>("set floor kernel launch", left, right, prune, p, o,
                                     reinterpret_cast<unsigned long long*>(stats), static_cast<hipStream_t>(stream));
}
