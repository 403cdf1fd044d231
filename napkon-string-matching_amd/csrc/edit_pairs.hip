// Listed pairs under the Levenshtein metrics (nsm_hip_edit.h): nsm_edit_raw_pairs and nsm_edit_levels_pairs.  Sibling
// kernels of the Indel ones in pairs_kernels.hpp with the same walk (for_each_pair), levels sum (levels_sum), checks and
// launch helper: ONE WAVEFRONT SCORES ONE PAIR, everything about the pair is wave-uniform.  The distance core is the
// column update of edit_distance.hpp on wave-uniform words: the match mask of pattern word w is __ballot(pattern_w ==
// unit) and the add carry and both shift carries are handed from word w to w + 1 in one ascending pass.
//
// Unlike wave_lcs the LEFT string is always the pattern and the right one the text, whichever is shorter: the occurrence
// distance of NSM_METRIC_EDIT_WITHIN is not symmetric.  The text is walked to its own length lb.  The two metrics share
// one instantiation per stride; `metric` is a wave-uniform kernel argument.  NSM_METRIC_INDEL is forwarded to the
// nsm_indel_* entry.
#include "edit_distance.hpp"
#include "pairs_kernels.hpp"

namespace nsm {

// d(a, b) or w(a, b) of two rows of K * 64 code units, la and lb of them live (both >= 1), by one wavefront.
template <int K>
__device__ __forceinline__ int wave_edit(const uint8_t* __restrict__ prow, int la, const uint8_t* __restrict__ trow, int lb,
                                         int lane, int metric) {
  const bool within = metric != NSM_METRIC_EDIT;
  const int nwp = (la + 63) >> 6;
  const int lw = (la - 1) >> 6, lbit = (la - 1) & 63;
  int pat[K], txt[K];
  unsigned long long vp[K], vn[K], live[K];  // live: the pattern positions of word w (a row's padding never takes part)
#pragma unroll
  for (int w = 0; w < K; ++w) {
    pat[w] = w < nwp ? static_cast<int>(prow[w * 64 + lane]) : 0;
    txt[w] = w * 64 < lb ? static_cast<int>(trow[w * 64 + lane]) : 0;
    const int bits = la - w * 64;
    live[w] = bits >= 64 ? ~0ull : bits > 0 ? (1ull << bits) - 1 : 0ull;
    vp[w] = ~0ull;
    vn[w] = 0ull;
  }
  int score = la, best = la;
#pragma unroll
  for (int tw = 0; tw < K; ++tw) {
    const int n = min(64, lb - tw * 64);
    for (int t = 0; t < n; ++t) {
      const int unit = __builtin_amdgcn_readlane(txt[tw], t);
      EditCarry c(within);
#pragma unroll
      for (int w = 0; w < K; ++w) {
        if (w < nwp) {  // wave-uniform
          const unsigned long long m = __ballot(pat[w] == unit) & live[w];
          unsigned long long hp, hn;
          edit_word(vp[w], vn[w], m, c, hp, hn);
          if (w == lw) score += static_cast<int>((hp >> lbit) & 1ull) - static_cast<int>((hn >> lbit) & 1ull);
        }
      }
      best = min(best, score);
    }
  }
  return within ? best : score;
}

template <int K>
__device__ __forceinline__ double wave_edit_score(const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, int rl,
                                                  const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen, int rr,
                                                  int lane, int metric) {
  // (a length beyond the row is the row's: clamped once, for the column and the score alike, as in the sweeps)
  const int la = min(wave_first(llen[rl]), K * 64), lb = min(wave_first(rlen[rr]), K * 64);
  if (la <= 0 || lb <= 0) return edit_score(0, 0, 0, metric);  // an empty string against anything: 0.0, as in the grids
  const int x = wave_edit<K>(lcodes + static_cast<size_t>(rl) * (K * 64), la, rcodes + static_cast<size_t>(rr) * (K * 64), lb,
                             lane, metric);
  return edit_score(la, lb, x, metric);
}

template <int K>
__global__ __launch_bounds__(kBlock) void edit_raw_pairs_kernel(const uint8_t* __restrict__ lcodes,
                                                                const int32_t* __restrict__ llen,
                                                                const uint8_t* __restrict__ rcodes,
                                                                const int32_t* __restrict__ rlen, const PairList l,
                                                                const int metric) {
  for_each_pair(l, [&](int rl, int rr, int lane) { return wave_edit_score<K>(lcodes, llen, rl, rcodes, rlen, rr, lane, metric); });
}

template <int K>
__global__ __launch_bounds__(kBlock) void edit_levels_pairs_kernel(
    const int32_t* __restrict__ lfirst, const int32_t* __restrict__ lnlev, const uint8_t* __restrict__ lcodes,
    const int32_t* __restrict__ llen, int l_rows, const int32_t* __restrict__ rfirst, const int32_t* __restrict__ rnlev,
    const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen, int r_rows, const PairList l, const int metric) {
  for_each_pair(l, [&](int il, int ir, int lane) {
    const int ll = wave_first(lnlev[il]), lr = wave_first(rnlev[ir]);
    const int lf = wave_first(lfirst[il]), rf = wave_first(rfirst[ir]);
    // an item without levels, or one whose level rows are not rows of its string table: no score
    if (ll <= 0 || lr <= 0 || lf < 0 || rf < 0 || lf + ll > l_rows || rf + lr > r_rows) return kNoScore;
    return levels_sum(ll, lr, [&](int a, int b, bool&) {
      return wave_edit_score<K>(lcodes, llen, lf + a, rcodes, rlen, rf + b, lane, metric);
    });
  });
}

}  // namespace nsm

extern "C" int nsm_edit_raw_pairs(const nsm_str_table* left, const nsm_str_table* right, int32_t metric,
                                  const int32_t* left_row, int32_t left_ids, const int32_t* right_row, int32_t right_ids,
                                  nsm_hit* pairs, uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_raw_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_raw_pairs(left, right, left_row, left_ids, right_row, right_ids, pairs, n_pairs, stream);
  if (int st = check_pair_strings(who, left, right)) return st;
  if (int st = check_pair_rows(who, left->n, right->n, left->codes && left->len, right->codes && right->len)) return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_stride(left->stride, [&](auto kc) {
    return launch_pairs("edit_raw_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((edit_raw_pairs_kernel<decltype(kc)::value>), grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                         left->codes, left->len, right->codes, right->len, l, static_cast<int>(metric));
    });
  });
}

extern "C" int nsm_edit_levels_pairs(const nsm_level_items* left, const nsm_str_table* left_strings,
                                     const nsm_level_items* right, const nsm_str_table* right_strings, int32_t metric,
                                     const int32_t* left_row, int32_t left_ids, const int32_t* right_row, int32_t right_ids,
                                     nsm_hit* pairs, uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_levels_pairs";
  if (int st = check_pair_args(who, left && right && left_strings && right_strings, pairs, n_pairs, left_row, left_ids,
                               right_row, right_ids))
    return st;
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_levels_pairs(left, left_strings, right, right_strings, left_row, left_ids, right_row, right_ids, pairs,
                                  n_pairs, stream);
  if (int st = check_pair_strings(who, left_strings, right_strings)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) return partitioned(who);
  if (left_strings->n < 0 || right_strings->n < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if (int st = check_pair_rows(who, left->n, right->n, left->first && left->nlev && left_strings->codes && left_strings->len,
                               right->first && right->nlev && right_strings->codes && right_strings->len))
    return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_stride(left_strings->stride, [&](auto kc) {
    return launch_pairs("edit_levels_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((edit_levels_pairs_kernel<decltype(kc)::value>), grid, dim3(kBlock), 0,
                         static_cast<hipStream_t>(stream), left->first, left->nlev, left_strings->codes, left_strings->len,
                         left_strings->n, right->first, right->nlev, right_strings->codes, right_strings->len,
                         right_strings->n, l, static_cast<int>(metric));
    });
  });
}
