// The LEVELS per-item queries of the Levenshtein metrics (nsm_hip_edit.h): nsm_edit_levels_top_k, nsm_edit_levels_profile,
// nsm_edit_levels_floor_grid -- compare_terms with the metric as score_func.  The sweep is the one of top_k_levels.hip --
// one wavefront owns a left item, its current level's match masks sit in LDS (wide_build_pm), the lanes' right level
// strings in the LDS text image, the pairs leave through one of the three sinks -- as a sibling of
// indel_levels_top_k_kernel with the distance core and its bounds exchanged (edit_distance.hpp):
//   * step 1 is at most 0.5 * edit_bound of the step-1 strings, every later step at most 2^-s (a score is at most 1);
//     under NSM_METRIC_EDIT the 32-bucket histogram bound d >= ceil(L1 / 2) (edit_raw.hip has the argument; it holds with
//     saturated buckets) tightens step 1.  The +1e-6 and +1e-9 slacks against the rounding of the double sum are those of
//     the Indel sweep;
//   * the lanes of a wave hold right level strings of DIFFERENT lengths and the wave walks to the longest.  A symbol past
//     a text's end would cost that text one edit (it adds nothing to an LCS), so a lane steps its column only while the
//     position is below its own lb: its result is read at its own length.
// The two metrics share one set of instantiations; `metric` is wave-uniform.  NSM_METRIC_INDEL is forwarded to the
// nsm_indel_* entry.
#include "edit_distance.hpp"
#include "floor_gate.hpp"
#include "score_tally.hpp"
#include "top_k_levels_kernels.hpp"

namespace nsm {

// d or w of the wave's pattern (masks in pm, K words per symbol of which the first W are live, wave-uniform) and the
// lane's text: its first lb code units.  nchars: the wave's longest text.
template <int K, int W>
__device__ __forceinline__ int wide_edit_words(const unsigned long long* pm, const uint32_t* text, int nchars, int lane, int la,
                                               int lb, int metric) {
  const unsigned long long top = metric == NSM_METRIC_EDIT ? 1ull : 0ull;
  EditColumn<W> col;
  col.open(la);
  const int nw = (nchars + 3) >> 2;
  for (int w = 0; w < nw; ++w) {
    const uint32_t word = text[w * kWave + lane];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (4 * w + b < lb) {  // the lane's own length: no padded column
        const unsigned long long* e = pm + ((word >> (8 * b)) & 0xffu) * kPmWords<K>;
        unsigned long long m[W];
#pragma unroll
        for (int k = 0; k < W; ++k) m[k] = lds_word(e + k);
        col.step(m, top);
      }
    }
  }
  return col.result(metric);
}

template <int K>
__device__ __forceinline__ int wide_edit(const unsigned long long* pm, const uint32_t* text, int nchars, int lane, int la, int lb,
                                         int metric) {
  const int words = (la + kWave - 1) >> 6;  // wave-uniform
  if (words <= 1) return wide_edit_words<K, 1>(pm, text, nchars, lane, la, lb, metric);
  if (K >= 2 && words == 2) return wide_edit_words<K, (K >= 2 ? 2 : 1)>(pm, text, nchars, lane, la, lb, metric);
  if (K >= 4 && words <= 4) return wide_edit_words<K, (K >= 4 ? 4 : 1)>(pm, text, nchars, lane, la, lb, metric);
  return wide_edit_words<K, K>(pm, text, nchars, lane, la, lb, metric);
}

struct TopLevEditParams {
  int32_t n_left, n_right, k, pm_stride, cat_mode, hist, metric;
  double threshold;
};

// Arguments, LDS layout, work split and sinks as indel_levels_top_k_kernel.
template <int K, bool PRUNE, class Sink = TopLists<false>>
__global__ __launch_bounds__(kWave) void edit_levels_top_k_kernel(
    const int32_t* __restrict__ lfirst, const int32_t* __restrict__ lnlev, const int32_t* __restrict__ lorig,
    const uint64_t* __restrict__ lcat, const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen,
    const uint8_t* __restrict__ lhist, const int32_t* __restrict__ rfirst, const int32_t* __restrict__ rnlev,
    const int32_t* __restrict__ rorig, const uint64_t* __restrict__ rcat, const uint8_t* __restrict__ rcodes,
    const int32_t* __restrict__ rlen, const uint8_t* __restrict__ rhist, const int32_t* __restrict__ banned_start,
    const int32_t* __restrict__ banned_j, nsm_hit* __restrict__ list, nsm_hit* __restrict__ out,
    unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats, const TopLevEditParams p,
    const typename Sink::Extra sx) {
  constexpr int kRow = kWave * K;  // bytes per string row
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_pm[];
  unsigned long long* pm = s_pm;
  uint32_t* text = reinterpret_cast<uint32_t*>(s_pm + p.pm_stride * kPmWords<K>);
  const int lane = threadIdx.x;
  const int row = blockIdx.x;
  const double thr = p.threshold;
  const int metric = p.metric;
  const bool use_cat = p.cat_mode != NSM_CAT_NONE;

  const int ll = lnlev[row];
  const int lf = lfirst[row];
  const int io = lorig[row];
  const uint64_t catl = use_cat ? lcat[row] : 0ull;
  Sink L = Sink::open(list, nullptr, p.k, row, lane, sx);
  unsigned long long st[4] = {0, 0, 0, 0};

  // the text image starts as code 0 (a real symbol): a lane that never stored a row still reads defined masks
#pragma unroll
  for (int q = 0; q < 16 * K; ++q) text[q * kWave + lane] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  if (ll > 0) {
    const int lrow1 = lf + min(1, ll - 1);  // the left level step 1 compares
    const int la1 = min(llen[lrow1], kRow);
    const bool use_hist = PRUNE && p.hist && metric == NSM_METRIC_EDIT;
    uint32_t lh[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) lh[q] = use_hist ? reinterpret_cast<const uint32_t*>(lhist + static_cast<size_t>(lrow1) * 32)[q] : 0u;
    int pm_level = -1;
    for (int base = 0; base < p.n_right; base += kWave) {
      const int j = base + lane;
      const bool valid = j < p.n_right;
      const int jc = valid ? j : p.n_right - 1;
      const int lr = rnlev[jc];
      const int rf = rfirst[jc];
      const int jo = rorig[jc];
      const int S = max(ll, lr);
      bool cand = valid && lr > 0 && (!use_cat || category_match(catl, rcat[jc], p.cat_mode));
      const double eff = L.eff(0, thr);
      st[0] += valid ? 1u : 0u;
      const int rrow1 = rf + max(0, min(1, lr - 1));
      const int lb1 = cand ? min(rlen[rrow1], kRow) : 0;
      if (PRUNE && cand) {
        // step 1 at most the length bound, the later steps at most 1 each
        cand = 0.5 * edit_bound(la1, lb1, metric) + lev_top_tail(S) + 1e-6 >= eff;
      }
      st[1] += cand ? 1u : 0u;
      if (use_hist && cand) {
        const uint4* hp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(rrow1) * 32);
        const uint4 h0 = hp[0], h1 = hp[1];
        const uint32_t hr[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        uint32_t l1 = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) l1 = __builtin_amdgcn_sad_u8(lh[q], hr[q], l1);
        const int d_lb = max(edit_least(la1, lb1, metric), (static_cast<int>(l1) + 1) >> 1);
        cand = 0.5 * edit_score(la1, lb1, d_lb, metric) + lev_top_tail(S) + 1e-6 >= eff;
      }
      st[2] += cand ? 1u : 0u;
      st[3] += cand ? 1u : 0u;  // a candidate gets step 1 exactly
      if (!__any(cand)) continue;

      // ---- exact steps, wave-uniform left level, per-lane right level
      const int smax = wave_max_i32(cand ? S : 0);
      bool live = cand;
      double score = 0.0, factor = 1.0;
      int text_row = -1;
      for (int s = 1; s <= smax && __any(live); ++s) {
        factor *= 0.5;
        const int a = min(s, ll - 1);
        const int la = min(llen[lf + a], kRow);
        if (a != pm_level) {
          wide_build_pm<K>(pm, p.pm_stride, lcodes + static_cast<size_t>(lf + a) * kRow, la, lane);
          pm_level = a;
        }
        const bool act = live && s <= S;
        const int rrow = rf + max(0, min(s, lr - 1));
        if (act && rrow != text_row) {  // the lane's own column of the text image
          const uint4* tp = reinterpret_cast<const uint4*>(rcodes + static_cast<size_t>(rrow) * kRow);
#pragma unroll
          for (int q = 0; q < 4 * K; ++q) {
            const uint4 v = tp[q];
            text[(4 * q + 0) * kWave + lane] = v.x;
            text[(4 * q + 1) * kWave + lane] = v.y;
            text[(4 * q + 2) * kWave + lane] = v.z;
            text[(4 * q + 3) * kWave + lane] = v.w;
          }
          text_row = rrow;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int lb = act ? min(rlen[rrow], kRow) : 0;
        const int nchars = wave_max_i32(max(lb, 0));
        const int x = wide_edit<K>(pm, text, nchars, lane, la, lb, metric);
        if (act) {
          score += edit_score(la, lb, x, metric) * factor;
          if (s == S) live = false;                                        // all steps of the pair are in
          else if (PRUNE && score + factor + 1e-9 < eff) cand = live = false;  // the rest (< factor) cannot lift it
        }
      }
      lev_top_offer(L, cand, score, thr, io, jo, banned_start, banned_j);
    }
  }
  L.flush(ll > 0 ? 1 : 0, out, out_count, stats, st);
}

static TopLevEditParams edit_levels_params(const nsm_level_items* left, const nsm_str_table* left_strings,
                                           const nsm_level_items* right, const nsm_str_table* right_strings, int32_t metric,
                                           int32_t k, int32_t category_mode, double threshold) {
  TopLevEditParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = k;
  p.pm_stride = ((left_strings->alphabet + 1) + 63) / 64 * 64;
  p.cat_mode = category_mode;
  p.hist = (left_strings->hist && right_strings->hist) ? 1 : 0;
  p.metric = metric;
  p.threshold = threshold;
  return p;
}

// The sweep with sink S: list / out / out_count are the top-k query's, `sx` the sink's own argument.
template <class S>
static int launch_edit_levels(const char* what, const nsm_level_items* li, const nsm_str_table* ls, const nsm_level_items* ri,
                              const nsm_str_table* rs, bool prune, const int32_t* bs, const int32_t* bj,
                              const TopLevEditParams& p, nsm_hit* list, nsm_hit* out, unsigned long long* out_count,
                              unsigned long long* stats, const typename S::Extra& sx, hipStream_t s) {
  return by_stride(ls->stride, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    auto launch = [&](auto pruned) {
      const size_t lds = static_cast<size_t>(p.pm_stride) * kPmWords<K> * 8 + static_cast<size_t>(16 * K) * kWave * 4;
      hipLaunchKernelGGL((edit_levels_top_k_kernel<K, decltype(pruned)::value, S>), dim3(p.n_left), dim3(kWave), lds, s,
                         li->first, li->nlev, li->orig, li->cat, ls->codes, ls->len, ls->hist, ri->first, ri->nlev, ri->orig,
                         ri->cat, rs->codes, rs->len, rs->hist, bs, bj, list, out, out_count, stats, p, sx);
      return hip_status(hipGetLastError(), what);
    };
    return prune ? launch(std::true_type{}) : launch(std::false_type{});
  });
}

}  // namespace nsm

extern "C" int nsm_edit_levels_top_k(const nsm_level_items* left, const nsm_str_table* left_strings,
                                     const nsm_level_items* right, const nsm_str_table* right_strings, int32_t metric,
                                     double threshold, int32_t k, int32_t category_mode, uint32_t flags,
                                     const int32_t* banned_start, const int32_t* banned_j, nsm_hit* out,
                                     unsigned long long* out_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_levels_top_k";
  if (!left || !right || !left_strings || !right_strings || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_levels_top_k(left, left_strings, right, right_strings, threshold, k, category_mode, flags, banned_start,
                                  banned_j, out, out_count, stats, stream);
  if (int st = check_k(who, k)) return st;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  const TopLevEditParams p = edit_levels_params(left, left_strings, right, right_strings, metric, keff, category_mode, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, false)) return st;
  return o.sc.release(launch_edit_levels<TopLists<false>>("edit levels top-k kernel launch", left, left_strings, right,
                                                          right_strings, prune, banned_start, banned_j, p, o.sc.list, o.out,
                                                          o.out_count, o.stats, TopLists<false>::Extra{}, o.sc.s));
}

extern "C" int nsm_edit_levels_profile(const nsm_level_items* left, const nsm_str_table* left_strings,
                                       const nsm_level_items* right, const nsm_str_table* right_strings, int32_t metric,
                                       const double* thresholds, int32_t n_thresholds, int32_t category_mode, uint32_t flags,
                                       const int32_t* banned_start, const int32_t* banned_j, uint64_t* pairs, double* left_best,
                                       double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_levels_profile";
  if (!left || !right || !left_strings || !right_strings) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_levels_profile(left, left_strings, right, right_strings, thresholds, n_thresholds, category_mode, flags,
                                    banned_start, banned_j, pairs, left_best, right_best, stats, stream);
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  const TopLevEditParams p = edit_levels_params(left, left_strings, right, right_strings, metric, 0, category_mode, thresholds[0]);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return launch_edit_levels<ScoreTally>("edit levels profile kernel launch", left, left_strings, right,
                                                             right_strings, prune, banned_start, banned_j, p, nullptr, nullptr,
                                                             nullptr, st64, o, s);
                     });
}

extern "C" int nsm_edit_levels_floor_grid(const nsm_level_items* left, const nsm_str_table* left_strings,
                                          const nsm_level_items* right, const nsm_str_table* right_strings, int32_t metric,
                                          double threshold, const double* left_floor, const double* right_floor,
                                          int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                                          const int32_t* banned_j, nsm_hit* hits, uint64_t capacity, unsigned long long* hit_count,
                                          uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_levels_floor_grid";
  if (int st = check_floor_out(who, left && right && left_strings && right_strings, hits, capacity, hit_count)) return st;
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_levels_floor_grid(left, left_strings, right, right_strings, threshold, left_floor, right_floor,
                                       category_mode, flags, banned_start, banned_j, hits, capacity, hit_count, stats, stream);
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  const TopLevEditParams p = edit_levels_params(left, left_strings, right, right_strings, metric, 0, category_mode, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  return launch_edit_levels<FloorGate>("edit levels floor kernel launch", left, left_strings, right, right_strings, prune,
                                       banned_start, banned_j, p, nullptr, nullptr, nullptr,
                                       reinterpret_cast<unsigned long long*>(stats), o, static_cast<hipStream_t>(stream));
}
