// Floor grids of the RAW grids: the hits of nsm_*_raw_grid at `threshold` that also reach a floor of their own left item
// and one of their own right item -- a threshold grid whose threshold is per item.  With the best scores of a profile call
// (nsm_*_raw_profile) minus a margin as floors this is the best-match query: every item's best match with everything that
// is as good or nearly as good, from one side or from both (reciprocal best hits).
//
// The sweep is the one of top_k_raw.hip -- the same kernels (top_k_raw_kernels.hpp), same work split, class walk and
// bounds -- instantiated with the gate sink (floor_gate.hpp) in place of the lists: the floors are final from the first
// pair on, so everything prunes against max(threshold, left floor), and a scored pair that passes is appended to the
// caller's hit buffer as the threshold grids append theirs.  The scores are the doubles the RAW grids emit.
#include "floor_gate.hpp"
#include "top_k_raw_kernels.hpp"

namespace nsm {

template <int W, bool PRUNE, bool HIST>
static int launch_indel_floors(const nsm_str_table* l, const nsm_str_table* r, const TopIndelParams& p, const FloorOut& o,
                               unsigned long long* stats, hipStream_t s) {
  auto* kern = indel_top_k_kernel<W, PRUNE, HIST, false, FloorGate>;
  const size_t lds = static_cast<size_t>(kTopG) * p.pm_stride * W * 8;
  if (lds > 64 * 1024) {
    const int st = hip_status(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  static_cast<int>(lds)), "indel floor kernel LDS");
    if (st) return st;
  }
  hipLaunchKernelGGL(kern, dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), lds, s, l->codes, l->len, l->orig,
                     reinterpret_cast<const uint32_t*>(l->hist), r->codes, r->len_start, r->orig,
                     reinterpret_cast<const uint32_t*>(r->hist), static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                     static_cast<unsigned long long*>(nullptr), stats, p, static_cast<const int32_t*>(nullptr),
                     static_cast<int32_t*>(nullptr), o);
  return hip_status(hipGetLastError(), "indel floor kernel launch");
}

template <int W>
static int dispatch_indel_floors(bool prune, bool hist, const nsm_str_table* l, const nsm_str_table* r, const TopIndelParams& p,
                                 const FloorOut& o, unsigned long long* stats, hipStream_t s) {
  if (!prune) return launch_indel_floors<W, false, false>(l, r, p, o, stats, s);
  if (hist) return launch_indel_floors<W, true, true>(l, r, p, o, stats, s);
  return launch_indel_floors<W, true, false>(l, r, p, o, stats, s);
}

template <int W>
static int dispatch_jaccard_floors(bool prune, const nsm_set_table* l, const nsm_set_table* r, const TopJacParams& p,
                                   const FloorOut& o, unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    hipLaunchKernelGGL((jaccard_top_k_kernel<W, decltype(pruned)::value, false, FloorGate>), dim3((p.n_left + kTopG - 1) / kTopG),
                       dim3(kWave), 0, s, l->ids, l->cnt, l->sig, l->sig2, l->orig, r->ids, r->size_start, r->sig, r->sig2,
                       r->orig, static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                       static_cast<unsigned long long*>(nullptr), stats, p, static_cast<const int32_t*>(nullptr),
                       static_cast<int32_t*>(nullptr), o);
    return hip_status(hipGetLastError(), "jaccard floor kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace nsm

extern "C" int nsm_indel_raw_floor_grid(const nsm_str_table* left, const nsm_str_table* right, double threshold,
                                        const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                                        uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_raw_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_raw_str_query(who, left, right)) return st;
  TopIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.pm_stride = ((left->alphabet + 1) + 63) / 64 * 64;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const bool hist = prune && left->hist && right->hist && left->stride <= 128;  // (as in nsm_indel_raw_top_k)
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return by_stride(left->stride, [&](auto kc) {
    return dispatch_indel_floors<decltype(kc)::value>(prune, hist, left, right, p, o, st64, s);
  });
}

extern "C" int nsm_jaccard_raw_floor_grid(const nsm_set_table* left, const nsm_set_table* right, double threshold,
                                          const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                                          uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_raw_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_raw_set_query(who, left, right)) return st;
  TopJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return by_width(left->width, [&](auto wc) {
    return dispatch_jaccard_floors<decltype(wc)::value>(prune, left, right, p, o, st64, s);
  });
}
