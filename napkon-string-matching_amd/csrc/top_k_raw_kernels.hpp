// The kernels of top_k_raw.hip, as templates over the sink that receives the scored pairs: TopLists (top_k_lists.hpp)
// for the top-k queries, ScoreTally (score_tally.hpp) for the threshold profiles of profile_raw.hip.
#pragma once
#include "indel_score.hpp"
#include "indel_wide.hpp"
#include "set_measure.hpp"
#include "top_k_lists.hpp"

namespace nsm {

constexpr int kTopG = 8;         // left rows per wavefront

// Least LCS whose score reaches `eff` (la, lb >= 1), or min(la, lb) + 1 when none does.  The start
// ceil(eff (la + lb) / 2) - 1 is below the answer (the rounding of the score is far smaller than one LCS step), the walk
// up uses the exact double score: the bound is never rounded away from a pair that could still enter the list.
__device__ __forceinline__ int indel_need(int la, int lb, double eff) {
  if (eff <= 0.0) return 0;
  const int top = min(la, lb);
  int need = static_cast<int>(ceil(eff * static_cast<double>(la + lb) * 0.5)) - 1;
  need = max(0, min(need, top + 1));
  while (need <= top && indel_score(la, lb, need) < eff) ++need;
  return need;
}

// (The same for the intersection of two id sets: jaccard_need and the measures' need, set_measure.hpp.)

// The class walk: classes are indexed by their size z = 0 .. top (length / set size); starting at z0 -- the group's first
// row's -- the walk goes to whichever neighbour, up (hi) or down (lo), has the larger bound for z0, and drops a direction
// once no row of the group can gain from what is left of it.  A row's class bound is non-increasing away from its own
// size, so the best class left in [from, to] for a row of size z is the one closest to z.
struct ClassWalk {
  int hi, lo;
};

// ------------------------------------------------------------------------------------------------------------------ Indel
struct TopIndelParams {
  int32_t n_left, n_right, k, pm_stride;
  double threshold;
};

// W 64-bit words per pattern (stride 64 W).  LDS: [G][pm_stride][W] match masks of the group's rows.  GROUPED: rgroup[jo]
// is the group of the right row with caller id jo and glist the group ids of the lists' records (top_k_lists.hpp), both
// unused otherwise; the work split, the class walk and every bound are those of the ungrouped query.
template <int W, bool PRUNE, bool HIST, bool GROUPED, class Sink = TopLists<GROUPED>>  // (sx: the sink's own argument)
__global__ __launch_bounds__(kWave) void indel_top_k_kernel(
    const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, const int32_t* __restrict__ lorig,
    const uint32_t* __restrict__ lhist, const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen_start,
    const int32_t* __restrict__ rorig, const uint32_t* __restrict__ rhist, nsm_hit* __restrict__ list,
    nsm_hit* __restrict__ out, unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats,
    const TopIndelParams p, const int32_t* __restrict__ rgroup, int32_t* __restrict__ glist, const typename Sink::Extra sx) {
  constexpr int G = kTopG, STRIDE = 64 * W;
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_pm[];
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * G;
  const int rows = min(G, p.n_left - row0);
  const double thr = p.threshold;

  // lane g < rows: row g's length and caller id
  const int la_v = lane < rows ? llen[row0 + lane] : 0;
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
      const int c = lcodes[static_cast<size_t>(row0 + g) * STRIDE + u];
      atomicOr(&s_pm[(static_cast<size_t>(g) * p.pm_stride + c) * W + u / kWave], 1ull << (u % kWave));
    }
  }
  __syncthreads();

  Sink L = Sink::open(list, glist, p.k, row0, lane, sx);
  unsigned long long st[4] = {0, 0, 0, 0};

  // upper bound of a pair of row g with a right row of length lb: all of the shorter string in common
  auto bound = [&](int g, int lb) { const int a = la(g); return indel_score(a, lb, min(a, lb)); };
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
    // bound of class hi for la0: 2 la0 / (la0 + hi); of class lo: 2 lo / (la0 + lo)
    const int lb = (up && (!down || static_cast<long long>(la0) * (la0 + w.lo) >= static_cast<long long>(w.lo) * (la0 + w.hi)))
                       ? w.hi++ : w.lo--;
    const int s = rlen_start[STRIDE - lb], e = rlen_start[STRIDE - lb + 1];
    // rows that can still gain from this class, and the least LCS that matters to each: recomputed when a record has
    // entered a list since (only then can a floor have risen)
    uint32_t active = 0;
    int need[G];
    int seen = -1;
    for (int base = s; base < e; base += kWave) {
      if (seen != L.changes) {
        seen = L.changes;
        active = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double eff = L.eff(g, thr);
          active |= (g < rows && (!PRUNE || bound(g, lb) >= eff)) ? (1u << g) : 0u;
          need[g] = (PRUNE && la(g) > 0 && lb > 0) ? indel_need(la(g), lb, eff) : 0;
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
      if constexpr (PRUNE && HIST) {
        const uint4* hp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jc) * 8);
        const uint4 h0 = hp[0], h1 = hp[1];
        const uint32_t hr[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int g = 0; g < G; ++g) {
          uint32_t l1 = 0;
#pragma unroll
          for (int q = 0; q < 8; ++q) l1 = __builtin_amdgcn_sad_u8(lh[g][q], hr[q], l1);
          if (static_cast<int>(l1) > la(g) + lb - 2 * need[g]) cand &= ~(1u << g);
        }
      }
      st[2] += __popc(cand);
      const int jo = rorig[jc];
      for (int g = 0; g < rows; ++g) {
        const bool mine = (cand >> g) & 1u;
        if (!__any(mine)) continue;
        const int a = la(g);
        int lcs = 0;
        if (mine && a > 0 && lb > 0) {
          const unsigned long long* pm = s_pm + static_cast<size_t>(g) * p.pm_stride * W;
          unsigned long long v[W], m[W], u[W], t[W];
#pragma unroll
          for (int q = 0; q < W; ++q) v[q] = ~0ull;
          const uint4* tp = reinterpret_cast<const uint4*>(rcodes + static_cast<size_t>(jc) * STRIDE);
          for (int u16 = 0; u16 < lb; u16 += 16) {
            const uint4 x = tp[u16 / 16];
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
              if (u16 + b < lb) {
                const uint32_t code = (xs[b / 4] >> (8 * (b % 4))) & 0xffu;
#pragma unroll
                for (int q = 0; q < W; ++q) {
                  m[q] = pm[code * W + q];
                  u[q] = v[q] & m[q];
                }
                add_chain<W>(v, u, t);
#pragma unroll
                for (int q = 0; q < W; ++q) v[q] = t[q] | (v[q] & ~m[q]);
              }
            }
          }
#pragma unroll
          for (int q = 0; q < W; ++q) lcs += __popcll(~v[q]);
        }
        st[3] += mine ? 1u : 0u;
        const double sc = indel_score(a, lb, lcs);
        L.offer_lanes(g, mine && sc >= thr && L.beats(g, sc, jo), sc, __builtin_amdgcn_readlane(io_v, g), jo,
                      L.group_of(rgroup, jo));
      }
    }
  }
  L.flush(rows, out, out_count, stats, st);
}

// ---------------------------------------------------------------------------------------------------------------- Jaccard
struct TopJacParams {
  int32_t n_left, n_right, k;
  int32_t measure = NSM_MEASURE_UNION;  // read by RuntimeMeasure alone
  double threshold;
};

// M: the measure (set_measure.hpp); the default is the Jaccard quotient, the nsm_jaccard_* entries' instantiations.
template <int W, bool PRUNE, bool GROUPED, class Sink = TopLists<GROUPED>, class M = JaccardMeasure>  // (GROUPED, rgroup, glist, sx: as in the Indel kernel)
__global__ __launch_bounds__(kWave) void jaccard_top_k_kernel(
    const int32_t* __restrict__ lids, const int32_t* __restrict__ lcnt, const uint64_t* __restrict__ lsig,
    const uint64_t* __restrict__ lsig2, const int32_t* __restrict__ lorig, const int32_t* __restrict__ rids,
    const int32_t* __restrict__ rsize_start, const uint64_t* __restrict__ rsig, const uint64_t* __restrict__ rsig2,
    const int32_t* __restrict__ rorig, nsm_hit* __restrict__ list, nsm_hit* __restrict__ out,
    unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats, const TopJacParams p,
    const int32_t* __restrict__ rgroup, int32_t* __restrict__ glist, const typename Sink::Extra sx) {
  constexpr int G = kTopG;
  __shared__ int32_t s_ids[G * W];
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * G;
  const int rows = min(G, p.n_left - row0);
  const double thr = p.threshold;
  const bool two_sigs = PRUNE && lsig2 && rsig2;
  const M meas(p.measure);

  const int na_v = lane < rows ? lcnt[row0 + lane] : 0;
  const int io_v = lane < rows ? lorig[row0 + lane] : 0;
  auto na = [&](int g) { return __builtin_amdgcn_readlane(na_v, g); };
  uint64_t sl[G], sl2[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int r = row0 + min(g, rows - 1);
    sl[g] = PRUNE ? lsig[r] : 0ull;
    sl2[g] = two_sigs ? lsig2[r] : 0ull;
  }
  for (int e = lane; e < G * W; e += kWave) s_ids[e] = (e / W < rows) ? lids[static_cast<size_t>(row0) * W + e] : -1;
  __syncthreads();

  Sink L = Sink::open(list, glist, p.k, row0, lane, sx);
  unsigned long long st[4] = {0, 0, 0, 0};

  // upper bound with a set of b ids (Jaccard: min / max -- 0 when exactly one side is empty); an undefined pair never scores
  auto bound = [&](int g, int b) { return meas.bound(na(g), b); };
  auto alive = [&](int from, int to) {
    if (from > to) return false;
    if (!PRUNE) return true;
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      int b = min(max(na(g), from), to);
      if (b == 0 && na(g) == 0 && to >= 1) b = 1;  // (an empty row's own class is undefined; class 1 is its best)
      any = any || (g < rows && bound(g, b) >= L.eff(g, thr));
    }
    return any;
  };

  const int a0 = na(0);
  ClassWalk w{a0, a0 - 1};
  while (true) {
    const bool up = alive(w.hi, W), down = alive(0, w.lo);
    if (!up && !down) break;
    const int b = (up && (!down || meas.up_first(a0, w.lo, w.hi))) ? w.hi++ : w.lo--;  // the larger bound for a0 first
    const int s = rsize_start[W - b], e = rsize_start[W - b + 1];
    uint32_t active = 0;
    int need[G];
    int seen = -1;
    for (int base = s; base < e; base += kWave) {
      if (seen != L.changes) {  // (as in the Indel kernel: only a record entering a list moves a floor)
        seen = L.changes;
        active = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double eff = L.eff(g, thr);
          active |= (g < rows && meas.defined(na(g), b) && (!PRUNE || bound(g, b) >= eff)) ? (1u << g) : 0u;
          need[g] = (PRUNE && meas.defined(na(g), b)) ? meas.need(na(g), b, eff) : 0;
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
      if constexpr (PRUNE) {
        // |A n B| <= popcount(sigA & sigB) with the right word's top 6 bits set (nsm_hip.h), under both signatures
        const uint64_t sr = rsig[jc] | kCollBits;
        const uint64_t sr2 = two_sigs ? (rsig2[jc] | kCollBits) : 0ull;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          int ub = __popcll(sl[g] & sr);
          if (two_sigs) ub = min(ub, __popcll(sl2[g] & sr2));
          if (ub < need[g]) cand &= ~(1u << g);
        }
      }
      st[2] += __popc(cand);
      const int jo = rorig[jc];
      const int4* rp = reinterpret_cast<const int4*>(rids + static_cast<size_t>(jc) * W);
      for (int g = 0; g < rows; ++g) {
        const bool mine = (cand >> g) & 1u;
        if (!__any(mine)) continue;
        const int a = na(g);
        int inter = 0;
        if (mine) {
          // merge: the right row's ids (ascending) against the left row's (ascending, in LDS)
          const int32_t* li = s_ids + g * W;
          int q = 0;
          for (int v = 0; v < b; v += 4) {
            const int4 y4 = rp[v / 4];
            const int ys[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (v + t < b) {
                const int y = ys[t];
                while (q < a && li[q] < y) ++q;
                if (q < a && li[q] == y) { ++inter; ++q; }
              }
            }
          }
        }
        st[3] += mine ? 1u : 0u;
        const double sc = mine ? meas.score(a, b, inter) : 0.0;
        L.offer_lanes(g, mine && sc >= thr && L.beats(g, sc, jo), sc, __builtin_amdgcn_readlane(io_v, g), jo,
                      L.group_of(rgroup, jo));
      }
    }
  }
  L.flush(rows, out, out_count, stats, st);
}

}  // namespace nsm
