// The RAW per-item queries of the Levenshtein metrics (nsm_hip_edit.h): nsm_edit_raw_top_k(_grouped),
// nsm_edit_raw_profile, nsm_edit_raw_floor_grid.  The sweep is the one of top_k_raw.hip -- one wavefront owns G left rows
// whose match masks sit in LDS, the lanes stream right rows class by class, the pairs leave through one of the three
// sinks (TopLists, ScoreTally, FloorGate) -- as a sibling of indel_top_k_kernel with the distance core and its bounds
// exchanged (edit_distance.hpp):
//   * class bound: edit_bound, exact and non-increasing away from la, so the class walk and its `alive` test carry over;
//     the first direction is taken by comparing the two bounds;
//   * per class and row the greatest distance that still matters (edit_most), recomputed when a floor may have risen;
//   * histogram filter, NSM_METRIC_EDIT only: one edit moves the true symbol histograms of a pair by at most 2 in L1
//     (a substitution takes one from a count and adds one to another, an insertion or deletion moves one count), and
//     bucketing and the saturation at 255 are 1-Lipschitz per symbol count, so d >= ceil(L1 / 2) for the SAD L1 of the
//     two 32-bucket rows at every stride.  The occurrence distance has no such bound where a bucket saturates and prunes
//     on lengths alone;
//   * the text is a right row of the class, so every lane walks exactly lb symbols: no lane reads a padded column.
// With NSM_FLAG_PRUNE off only the 0.0 convention of an empty string decides a pair without its column.  The two metrics
// share one set of instantiations; `metric` is wave-uniform.  NSM_METRIC_INDEL is forwarded to the nsm_indel_* entry.
#include "edit_distance.hpp"
#include "floor_gate.hpp"
#include "score_tally.hpp"
#include "top_k_raw_kernels.hpp"

namespace nsm {

struct TopEditParams {
  int32_t n_left, n_right, k, pm_stride, metric;
  double threshold;
};

// Arguments, LDS layout, work split and sinks as indel_top_k_kernel.
template <int W, bool PRUNE, bool HIST, bool GROUPED, class Sink = TopLists<GROUPED>>
__global__ __launch_bounds__(kWave) void edit_top_k_kernel(
    const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, const int32_t* __restrict__ lorig,
    const uint32_t* __restrict__ lhist, const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen_start,
    const int32_t* __restrict__ rorig, const uint32_t* __restrict__ rhist, nsm_hit* __restrict__ list,
    nsm_hit* __restrict__ out, unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats,
    const TopEditParams p, const int32_t* __restrict__ rgroup, int32_t* __restrict__ glist, const typename Sink::Extra sx) {
  constexpr int G = kTopG, STRIDE = 64 * W;
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_pm[];
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * G;
  const int rows = min(G, p.n_left - row0);
  const double thr = p.threshold;
  const int metric = p.metric;
  const unsigned long long top = metric == NSM_METRIC_EDIT ? 1ull : 0ull;

  // lane g < rows: row g's length and caller id
  const int la_v = lane < rows ? min(llen[row0 + lane], STRIDE) : 0;
  const int io_v = lane < rows ? lorig[row0 + lane] : 0;
  auto la = [&](int g) { return __builtin_amdgcn_readlane(la_v, g); };
  uint32_t lh[G][8];
  if constexpr (HIST) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int r = row0 + min(g, rows - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) lh[g][q] = lhist[static_cast<size_t>(r) * 8 + q];
    }
  }
  // match masks of the rows: clear, then code unit u of row g ORs bit u % 64 into word u / 64 of pm[g][code]
  for (int e = lane; e < G * p.pm_stride * W; e += kWave) s_pm[e] = 0ull;
  __syncthreads();
  for (int g = 0; g < rows; ++g) {
    const int n = la(g);
    for (int u = lane; u < n; u += kWave) {
      const int c = min(static_cast<int>(lcodes[static_cast<size_t>(row0 + g) * STRIDE + u]), p.pm_stride - 1);
      atomicOr(&s_pm[(static_cast<size_t>(g) * p.pm_stride + c) * W + u / kWave], 1ull << (u % kWave));
    }
  }
  __syncthreads();

  Sink L = Sink::open(list, glist, p.k, row0, lane, sx);
  unsigned long long st[4] = {0, 0, 0, 0};

  auto bound = [&](int g, int lb) { return edit_bound(la(g), lb, metric); };
  auto alive = [&](int from, int to) {
    if (from > to) return false;
    if (!PRUNE) return true;
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; ++g) any = any || (g < rows && bound(g, min(max(la(g), from), to)) >= L.eff(g, thr));
    return any;
  };

  const int la0 = la(0);
  ClassWalk w{la0, la0 - 1};
  while (true) {
    const bool up = alive(w.hi, STRIDE), down = alive(0, w.lo);
    if (!up && !down) break;
    // the larger bound for la0 first (only the order of the sweep, never its records)
    const int lb = (up && (!down || edit_bound(la0, w.hi, metric) >= edit_bound(la0, w.lo, metric))) ? w.hi++ : w.lo--;
    const int s = rlen_start[STRIDE - lb], e = rlen_start[STRIDE - lb + 1];
    // rows that can still gain from this class, and the greatest distance that matters to each: recomputed when a record
    // has entered a list since (only then can a floor have risen)
    uint32_t active = 0;
    int most[G];
    int seen = -1;
    for (int base = s; base < e; base += kWave) {
      if (seen != L.changes) {
        seen = L.changes;
        active = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double eff = L.eff(g, thr);
          active |= (g < rows && (!PRUNE || bound(g, lb) >= eff)) ? (1u << g) : 0u;
          most[g] = (PRUNE && la(g) > 0 && lb > 0) ? edit_most(la(g), lb, eff, metric) : STRIDE;
        }
      }
      if (!active) break;
      const int j = base + lane;
      const bool valid = j < e;
      const int jc = valid ? j : e - 1;
      if (lane == 0) {
        const unsigned long long nv = static_cast<unsigned long long>(min(kWave, e - base));
        st[0] += nv * static_cast<unsigned long long>(rows);
        st[1] += nv * static_cast<unsigned long long>(__popc(active));
      }
      uint32_t cand = valid ? active : 0u;
      if constexpr (PRUNE && HIST) {  // (the host asks for HIST under NSM_METRIC_EDIT alone)
        const uint4* hp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jc) * 8);
        const uint4 h0 = hp[0], h1 = hp[1];
        const uint32_t hr[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int g = 0; g < G; ++g) {
          uint32_t l1 = 0;
#pragma unroll
          for (int q = 0; q < 8; ++q) l1 = __builtin_amdgcn_sad_u8(lh[g][q], hr[q], l1);
          // d >= ceil(L1 / 2) > most: the pair cannot reach eff (an empty string's 0.0 is never filtered: most = STRIDE)
          if (static_cast<int>(l1) > 2 * most[g]) cand &= ~(1u << g);
        }
      }
      st[2] += __popc(cand);
      const int jo = rorig[jc];
      for (int g = 0; g < rows; ++g) {
        const bool mine = (cand >> g) & 1u;
        if (!__any(mine)) continue;
        const int a = la(g);
        int x = 0;
        if (mine && a > 0 && lb > 0) {
          const unsigned long long* pm = s_pm + static_cast<size_t>(g) * p.pm_stride * W;
          EditColumn<W> col;
          col.open(a);
          unsigned long long m[W];
          const uint4* tp = reinterpret_cast<const uint4*>(rcodes + static_cast<size_t>(jc) * STRIDE);
          for (int u16 = 0; u16 < lb; u16 += 16) {
            const uint4 t4 = tp[u16 / 16];
            const uint32_t xs[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
              if (u16 + b < lb) {
                const uint32_t code = min((xs[b / 4] >> (8 * (b % 4))) & 0xffu, static_cast<uint32_t>(p.pm_stride - 1));
#pragma unroll
                for (int q = 0; q < W; ++q) m[q] = pm[code * W + q];
                col.step(m, top);
              }
            }
          }
          x = col.result(metric);
        }
        st[3] += mine ? 1u : 0u;
        const double sc = edit_score(a, lb, x, metric);
        L.offer_lanes(g, mine && sc >= thr && L.beats(g, sc, jo), sc, __builtin_amdgcn_readlane(io_v, g), jo,
                      L.group_of(rgroup, jo));
      }
    }
  }
  L.flush(rows, out, out_count, stats, st);
}

static TopEditParams edit_params(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, int32_t k,
                                 double threshold) {
  TopEditParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = k;
  p.pm_stride = ((left->alphabet + 1) + 63) / 64 * 64;
  p.metric = metric;
  p.threshold = threshold;
  return p;
}

// (a saturated bucket only weakens the bound of NSM_METRIC_EDIT: every stride; none for the occurrence distance)
static bool edit_hist(bool prune, const nsm_str_table* left, const nsm_str_table* right, int32_t metric) {
  return prune && left->hist && right->hist && metric == NSM_METRIC_EDIT;
}

// F: the kernel's instantiation for (W, PRUNE, HIST) as f(stride tag, pruned tag, hist tag) -> launch status
template <class F>
static int by_stride_pruned(int stride, bool prune, bool hist, F&& f) {
  return by_stride(stride, [&](auto kc) {
    if (!prune) return f(kc, std::false_type{}, std::false_type{});
    return hist ? f(kc, std::true_type{}, std::true_type{}) : f(kc, std::true_type{}, std::false_type{});
  });
}

// The kernel `kern` over the left table's groups; more than 64 KB of match masks need the attribute first.
template <class Kern, class... Args>
static int launch_edit_sweep(const char* what, Kern* kern, const TopEditParams& p, int words, hipStream_t s, Args... args) {
  const size_t lds = static_cast<size_t>(kTopG) * p.pm_stride * words * 8;
  if (lds > 64 * 1024) {
    const int st = hip_status(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  static_cast<int>(lds)), what);
    if (st) return st;
  }
  hipLaunchKernelGGL(kern, dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), lds, s, args...);
  return hip_status(hipGetLastError(), what);
}

static int edit_raw_top_k(const char* who, bool grouped, const nsm_str_table* left, const nsm_str_table* right, int32_t metric,
                          const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                          unsigned long long* out_count, uint64_t* stats, void* stream) {
  if (!left || !right || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return grouped ? nsm_indel_raw_top_k_grouped(left, right, right_group, threshold, k, flags, out, out_count, stats, stream)
                   : nsm_indel_raw_top_k(left, right, threshold, k, flags, out, out_count, stats, stream);
  if (int st = check_k(who, k)) return st;
  if (grouped && !right_group) {
    set_error("%s: right_group is null", who);
    return NSM_E_BADARG;
  }
  if (int st = check_raw_str_query(who, left, right)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  const TopEditParams p = edit_params(left, right, metric, keff, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, grouped)) return st;
  const int32_t* rg = grouped ? right_group : nullptr;
  return o.sc.release(by_stride_pruned(left->stride, prune, edit_hist(prune, left, right, metric), [&](auto kc, auto pr, auto hi) {
    return by_grouped(grouped, [&](auto gr) {
      constexpr bool GR = decltype(gr)::value;
      constexpr int W = decltype(kc)::value;
      return launch_edit_sweep("edit top-k kernel launch", edit_top_k_kernel<W, decltype(pr)::value, decltype(hi)::value, GR>, p, W,
                               o.sc.s, left->codes, left->len, left->orig, reinterpret_cast<const uint32_t*>(left->hist),
                               right->codes, right->len_start, right->orig, reinterpret_cast<const uint32_t*>(right->hist),
                               o.sc.list, o.out, o.out_count, o.stats, p, rg, o.sc.glist, typename TopLists<GR>::Extra{});
    });
  }));
}

// The profile and floor-grid launch: the sweep with sink S, whose argument is `o`.
template <class S>
static int launch_edit_sink(const char* what, const nsm_str_table* l, const nsm_str_table* r, bool prune, const TopEditParams& p,
                            const typename S::Extra& o, unsigned long long* stats, hipStream_t s) {
  return by_stride_pruned(l->stride, prune, edit_hist(prune, l, r, p.metric), [&](auto kc, auto pr, auto hi) {
    constexpr int W = decltype(kc)::value;
    return launch_edit_sweep(what, edit_top_k_kernel<W, decltype(pr)::value, decltype(hi)::value, false, S>, p, W, s, l->codes,
                             l->len, l->orig, reinterpret_cast<const uint32_t*>(l->hist), r->codes, r->len_start, r->orig,
                             reinterpret_cast<const uint32_t*>(r->hist), static_cast<nsm_hit*>(nullptr),
                             static_cast<nsm_hit*>(nullptr), static_cast<unsigned long long*>(nullptr), stats, p,
                             static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), o);
  });
}

}  // namespace nsm

extern "C" int nsm_edit_raw_top_k(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, double threshold,
                                  int32_t k, uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats,
                                  void* stream) {
  return nsm::edit_raw_top_k("nsm_edit_raw_top_k", false, left, right, metric, nullptr, threshold, k, flags, out, out_count,
                             stats, stream);
}

extern "C" int nsm_edit_raw_top_k_grouped(const nsm_str_table* left, const nsm_str_table* right, int32_t metric,
                                          const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                                          unsigned long long* out_count, uint64_t* stats, void* stream) {
  return nsm::edit_raw_top_k("nsm_edit_raw_top_k_grouped", true, left, right, metric, right_group, threshold, k, flags, out,
                             out_count, stats, stream);
}

extern "C" int nsm_edit_raw_profile(const nsm_str_table* left, const nsm_str_table* right, int32_t metric,
                                    const double* thresholds, int32_t n_thresholds, uint32_t flags, uint64_t* pairs,
                                    double* left_best, double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_raw_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_raw_profile(left, right, thresholds, n_thresholds, flags, pairs, left_best, right_best, stats, stream);
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_raw_str_query(who, left, right)) return st;
  const TopEditParams p = edit_params(left, right, metric, 0, thresholds[0]);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return launch_edit_sink<ScoreTally>("edit profile kernel launch", left, right, prune, p, o, st64, s);
                     });
}

extern "C" int nsm_edit_raw_floor_grid(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, double threshold,
                                       const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                                       uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_edit_raw_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  if (int st = check_metric(who, metric)) return st;
  if (metric == NSM_METRIC_INDEL)
    return nsm_indel_raw_floor_grid(left, right, threshold, left_floor, right_floor, flags, hits, capacity, hit_count, stats,
                                    stream);
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_raw_str_query(who, left, right)) return st;
  const TopEditParams p = edit_params(left, right, metric, 0, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  return launch_edit_sink<FloorGate>("edit floor kernel launch", left, right, prune, p, o,
                                     reinterpret_cast<unsigned long long*>(stats), static_cast<hipStream_t>(stream));
}
