// The kernels, checks and launch helper of pairs.hip (see there for the mapping to CDNA4), in a header so that the
// nsm_set_*_pairs entries (set_pairs.hip) instantiate the Jaccard kernels with another measure (set_measure.hpp).
#pragma once
#include "indel_score.hpp"
#include "top_k_levels_kernels.hpp"
#include "top_k_raw_kernels.hpp"

namespace nsm {

constexpr double kNoScore = -1.0;
constexpr int kPairsMaxBlocks = 256 * 8;  // 256 CUs x 8 blocks of 4 waves: every SIMD's 8 wave slots

struct PairList {
  nsm_hit* pairs;  // read: i, j; written: score (not restrict: the same records)
  unsigned long long n_pairs;
  const int32_t* left_row;
  const int32_t* right_row;
  int32_t left_ids, right_ids, n_left, n_right;
};

// Table row of caller id `id`, or -1: outside the map, mapped to none, or mapped outside the table.
__device__ __forceinline__ int pair_row(const int32_t* __restrict__ map, int ids, int id, int n) {
  if (id < 0 || id >= ids) return -1;
  const int r = map[id];
  return (r >= 0 && r < n) ? r : -1;
}

// The grid-stride walk of a wave over the list: f(left row, right row) -> score, rows >= 0.  Everything is wave-uniform.
template <class F>
__device__ __forceinline__ void for_each_pair(const PairList& l, F&& f) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  const unsigned long long wave = static_cast<unsigned long long>(blockIdx.x) * kWavesPerBlock +
                                  static_cast<unsigned>(wave_first(static_cast<int>(threadIdx.x >> 6)));
  const unsigned long long step = static_cast<unsigned long long>(gridDim.x) * kWavesPerBlock;
  for (unsigned long long p = wave; p < l.n_pairs; p += step) {
    const int i = wave_first(l.pairs[p].i), j = wave_first(l.pairs[p].j);
    const int rl = wave_first(pair_row(l.left_row, l.left_ids, i, l.n_left));
    const int rr = wave_first(pair_row(l.right_row, l.right_ids, j, l.n_right));
    double score = kNoScore;
    if (rl >= 0 && rr >= 0) score = f(rl, rr, lane);
    if (lane == 0) l.pairs[p].score = score;
  }
}

// The levels sum of compare_terms (types/comparable_data.py:248-265) for items of ll and lr levels (both >= 1):
// part(a, b, &ok) scores one level pair; a pair whose part says !ok has no score.
template <class Part>
__device__ __forceinline__ double levels_sum(int ll, int lr, Part&& part) {
  const int S = max(ll, lr);
  double score = 0.0, factor = 1.0, cur = 0.0;
  int prev_a = -1, prev_b = -1;
  bool ok = true;
  for (int s = 1; s <= S; ++s) {
    const int a = min(s, ll - 1), b = min(s, lr - 1);
    if (a != prev_a || b != prev_b) {
      cur = part(a, b, ok);
      prev_a = a;
      prev_b = b;
    }
    factor *= 0.5;
    score += cur * factor;
  }
  return ok ? score : kNoScore;
}

// ------------------------------------------------------------------------------------------------------------------ Indel
// LCS of two rows of K * 64 code units, la and lb of them live (both >= 1), by one wavefront.
template <int K>
__device__ __forceinline__ int wave_lcs(const uint8_t* __restrict__ row_a, int la, const uint8_t* __restrict__ row_b, int lb,
                                        int lane) {
  const bool swap = lb < la;  // the shorter string is the pattern
  const uint8_t* __restrict__ prow = swap ? row_b : row_a;
  const uint8_t* __restrict__ trow = swap ? row_a : row_b;
  const int lp = swap ? lb : la, lt = swap ? la : lb;
  const int nwp = (lp + 63) >> 6;
  int pat[K], txt[K];
  unsigned long long v[K], live[K];  // live: the pattern positions of word w (a row's padding never takes part)
#pragma unroll
  for (int w = 0; w < K; ++w) {
    pat[w] = w < nwp ? static_cast<int>(prow[w * 64 + lane]) : 0;
    txt[w] = w * 64 < lt ? static_cast<int>(trow[w * 64 + lane]) : 0;
    const int bits = lp - w * 64;
    live[w] = bits >= 64 ? ~0ull : bits > 0 ? (1ull << bits) - 1 : 0ull;
    v[w] = ~0ull;
  }
#pragma unroll
  for (int tw = 0; tw < K; ++tw) {
    const int n = min(64, lt - tw * 64);
    for (int t = 0; t < n; ++t) {
      const int unit = __builtin_amdgcn_readlane(txt[tw], t);
      unsigned long long carry = 0;
#pragma unroll
      for (int w = 0; w < K; ++w) {
        if (w < nwp) {  // wave-uniform
          const unsigned long long m = __ballot(pat[w] == unit) & live[w];
          const unsigned long long u = v[w] & m;
          const unsigned long long s1 = v[w] + u;
          const unsigned long long s2 = s1 + carry;
          carry = static_cast<unsigned long long>(s1 < v[w]) | static_cast<unsigned long long>(s2 < s1);
          v[w] = s2 | (v[w] ^ u);
        }
      }
    }
  }
  int lcs = 0;
#pragma unroll
  for (int w = 0; w < K; ++w) lcs += __popcll(~v[w] & live[w]);
  return lcs;
}

template <int K>
__device__ __forceinline__ double wave_indel(const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, int rl,
                                             const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen, int rr,
                                             int lane) {
  const int la = wave_first(llen[rl]), lb = wave_first(rlen[rr]);
  if (la <= 0 || lb <= 0) return indel_score(0, 0, 0);  // an empty string against anything: 0.0, as in the grids
  const int lcs = wave_lcs<K>(lcodes + static_cast<size_t>(rl) * (K * 64), min(la, K * 64),
                              rcodes + static_cast<size_t>(rr) * (K * 64), min(lb, K * 64), lane);
  return indel_score(la, lb, lcs);
}

template <int K>
__global__ __launch_bounds__(kBlock) void indel_raw_pairs_kernel(const uint8_t* __restrict__ lcodes,
                                                                 const int32_t* __restrict__ llen,
                                                                 const uint8_t* __restrict__ rcodes,
                                                                 const int32_t* __restrict__ rlen, const PairList l) {
  for_each_pair(l, [&](int rl, int rr, int lane) { return wave_indel<K>(lcodes, llen, rl, rcodes, rlen, rr, lane); });
}

template <int K>
__global__ __launch_bounds__(kBlock) void indel_levels_pairs_kernel(
    const int32_t* __restrict__ lfirst, const int32_t* __restrict__ lnlev, const uint8_t* __restrict__ lcodes,
    const int32_t* __restrict__ llen, int l_rows, const int32_t* __restrict__ rfirst, const int32_t* __restrict__ rnlev,
    const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen, int r_rows, const PairList l) {
  for_each_pair(l, [&](int il, int ir, int lane) {
    const int ll = wave_first(lnlev[il]), lr = wave_first(rnlev[ir]);
    const int lf = wave_first(lfirst[il]), rf = wave_first(rfirst[ir]);
    // an item without levels, or one whose level rows are not rows of its string table: no score
    if (ll <= 0 || lr <= 0 || lf < 0 || rf < 0 || lf + ll > l_rows || rf + lr > r_rows) return kNoScore;
    return levels_sum(ll, lr, [&](int a, int b, bool&) {
      return wave_indel<K>(lcodes, llen, lf + a, rcodes, rlen, rf + b, lane);
    });
  });
}

// ---------------------------------------------------------------------------------------------------------------- Jaccard
// Lane q: the position of left id q among the first nb right ids, 64 when it is not there (or q >= na).
template <int W>
__device__ __forceinline__ int wave_match(const int32_t* __restrict__ lids, int rl, int na, const int32_t* __restrict__ rids,
                                          int rr, int nb, int lane) {
  // (lanes past a row's ids hold a value the other side never has: ids are >= 0)
  const int a = lane < na ? lids[static_cast<size_t>(rl) * W + lane] : -1;
  const int b = lane < nb ? rids[static_cast<size_t>(rr) * W + lane] : -2;
  int pos = 64;
  for (int q = 0; q < na; ++q) {
    const int id = __builtin_amdgcn_readlane(a, q);
    const unsigned long long m = __ballot(b == id);
    if (lane == q && m != 0ull) pos = __builtin_ctzll(m);
  }
  return pos;
}

// M, meas: the measure (set_measure.hpp); the default is the Jaccard quotient, the nsm_jaccard_*_pairs entries' kernels.
template <int W, class M = JaccardMeasure>
__global__ __launch_bounds__(kBlock) void jaccard_raw_pairs_kernel(const int32_t* __restrict__ lids,
                                                                   const int32_t* __restrict__ lcnt,
                                                                   const int32_t* __restrict__ rids,
                                                                   const int32_t* __restrict__ rcnt, const PairList l,
                                                                   const M meas) {
  for_each_pair(l, [&](int rl, int rr, int lane) {
    const int na = min(W, max(0, wave_first(lcnt[rl]))), nb = min(W, max(0, wave_first(rcnt[rr])));
    if (!meas.defined(na, nb)) return kNoScore;  // a zero denominator (Jaccard: two empty sets): the host's ZeroDivisionError
    const int pos = wave_match<W>(lids, rl, na, rids, rr, nb, lane);
    return meas.score(na, nb, __popcll(__ballot(lane < na && pos < nb)));
  });
}

template <int W, class M = JaccardMeasure>
__global__ __launch_bounds__(kBlock) void jaccard_levels_pairs_kernel(
    const int32_t* __restrict__ lids, const int32_t* __restrict__ lcnt, const int32_t* __restrict__ lnlev,
    const uint8_t* __restrict__ lplen, int lev_stride_l, const int32_t* __restrict__ rids, const int32_t* __restrict__ rcnt,
    const int32_t* __restrict__ rnlev, const uint8_t* __restrict__ rplen, int lev_stride_r, const PairList l, const M meas) {
  for_each_pair(l, [&](int rl, int rr, int lane) {
    const int ll = wave_first(lnlev[rl]), lr = wave_first(rnlev[rr]);
    if (ll <= 0 || lr <= 0) return kNoScore;
    const int na = min(W, max(0, wave_first(lcnt[rl]))), nb = min(W, max(0, wave_first(rcnt[rr])));
    const int pos = wave_match<W>(lids, rl, na, rids, rr, nb, lane);
    const uint8_t* __restrict__ lpl = lplen + static_cast<size_t>(rl) * lev_stride_l;
    const uint8_t* __restrict__ rpl = rplen + static_cast<size_t>(rr) * lev_stride_r;
    return levels_sum(ll, lr, [&](int a, int b, bool& ok) {
      const int pl = min(na, wave_first(static_cast<int>(lpl[min(a, lev_stride_l - 1)])));
      const int pr = min(nb, wave_first(static_cast<int>(rpl[min(b, lev_stride_r - 1)])));
      if (!meas.defined(pl, pr)) ok = false;  // a zero denominator (Jaccard: two empty levels): the host's ZeroDivisionError
      return meas.part(pl, pr, __popcll(__ballot(lane < pl && pos < pr)));
    });
  });
}

// ----------------------------------------------------------------------------------------------------------------- checks
static int check_pair_args(const char* who, bool tables, const nsm_hit* pairs, uint64_t n_pairs, const int32_t* left_row,
                           int32_t left_ids, const int32_t* right_row, int32_t right_ids) {
  if (!tables || (!pairs && n_pairs) || (!left_row && left_ids > 0) || (!right_row && right_ids > 0)) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (left_ids < 0 || right_ids < 0) {
    set_error("%s: negative id count (%d, %d)", who, left_ids, right_ids);
    return NSM_E_BADARG;
  }
  return 0;
}

static int check_pair_strings(const char* who, const nsm_str_table* l, const nsm_str_table* r) {
  const auto known = [](int s) { return s == 64 || s == 128 || s == 256 || s == 512; };
  if (l->stride != r->stride || !known(l->stride)) {
    set_error("%s: stride %d/%d unsupported (both sides 64, 128, 256 or 512 code units)", who, l->stride, r->stride);
    return NSM_E_UNSUPPORTED;
  }
  if (l->alphabet != r->alphabet || l->alphabet < 1 || l->alphabet > 255) {
    set_error("%s: alphabets differ or exceed 255 (%d, %d)", who, l->alphabet, r->alphabet);
    return NSM_E_BADARG;
  }
  return 0;
}

static int check_pair_rows(const char* who, int32_t n_left, int32_t n_right, bool left_columns, bool right_columns) {
  if (n_left < 0 || n_right < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if ((n_left > 0 && !left_columns) || (n_right > 0 && !right_columns)) {  // (a table without rows is never read)
    set_error("%s: table has a null column", who);
    return NSM_E_BADARG;
  }
  return 0;
}

static int partitioned(const char* who) {
  set_error("%s: partitioned tables are not supported (an item must be one row: encode with partition=False)", who);
  return NSM_E_UNSUPPORTED;
}

template <class Launch>
static int launch_pairs(const char* what, uint64_t n_pairs, Launch&& launch) {
  const uint64_t blocks = (n_pairs + kWavesPerBlock - 1) / kWavesPerBlock;
  launch(dim3(static_cast<unsigned>(blocks < static_cast<uint64_t>(kPairsMaxBlocks) ? blocks : kPairsMaxBlocks)));
  return hip_status(hipGetLastError(), what);
}

}  // namespace nsm
