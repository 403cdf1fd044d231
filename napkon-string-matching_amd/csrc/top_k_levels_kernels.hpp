// The kernels of top_k_levels.hip, as templates over the sink that receives the scored pairs: TopLists
// (top_k_lists.hpp) for the top-k queries, ScoreTally (score_tally.hpp) for the threshold profiles of profile_levels.hip.
#pragma once
#include "indel_score.hpp"
#include "indel_wide.hpp"
#include "set_measure.hpp"
#include "top_k_lists.hpp"

namespace nsm {

// Is (i, j) -- caller ids -- on the blacklist?  banned_j[banned_start[i] .. banned_start[i + 1]) is sorted ascending.
__device__ __forceinline__ bool lev_top_banned(const int32_t* __restrict__ banned_start, const int32_t* __restrict__ banned_j,
                                               int i, int j) {
  int lo = banned_start[i], hi = banned_start[i + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int v = banned_j[mid];
    if (v == j) return true;
    if (v < j) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// Weight of the steps after step 1 of a pair with S steps: 1/2 - 2^-S (exact in double).
__device__ __forceinline__ double lev_top_tail(int S) { return 0.5 - __builtin_ldexp(1.0, -S); }

// Offer the lanes' finished pairs to the wave's list (all 64 lanes enabled).
template <class Sink>
__device__ __forceinline__ void lev_top_offer(Sink& L, bool ok, double score, double thr, int io, int jo,
                                              const int32_t* __restrict__ banned_start,
                                              const int32_t* __restrict__ banned_j) {
  ok = ok && score >= thr && L.beats(0, score, jo);
  if (ok && banned_start) ok = !lev_top_banned(banned_start, banned_j, io, jo);
  L.offer_lanes(0, ok, score, io, jo, 0);
}

// ------------------------------------------------------------------------------------------------------------------ Indel
struct TopLevIndelParams {
  int32_t n_left, n_right, k, pm_stride, cat_mode, hist;
  double threshold;
};

// K 64-bit words per string (stride 64 K).  LDS: [pm_stride][kPmWords<K>] match masks of the current left level, then
// the lanes' right level strings, [16 K][64] dwords (indel_wide.hpp).
template <int K, bool PRUNE, class Sink = TopLists<false>>  // (sx: the sink's own argument)
__global__ __launch_bounds__(kWave) void indel_levels_top_k_kernel(
    const int32_t* __restrict__ lfirst, const int32_t* __restrict__ lnlev, const int32_t* __restrict__ lorig,
    const uint64_t* __restrict__ lcat, const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen,
    const uint8_t* __restrict__ lhist, const int32_t* __restrict__ rfirst, const int32_t* __restrict__ rnlev,
    const int32_t* __restrict__ rorig, const uint64_t* __restrict__ rcat, const uint8_t* __restrict__ rcodes,
    const int32_t* __restrict__ rlen, const uint8_t* __restrict__ rhist, const int32_t* __restrict__ banned_start,
    const int32_t* __restrict__ banned_j, nsm_hit* __restrict__ list, nsm_hit* __restrict__ out,
    unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats, const TopLevIndelParams p,
    const typename Sink::Extra sx) {
  constexpr int kRow = kWave * K;  // bytes per string row
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_pm[];
  unsigned long long* pm = s_pm;
  uint32_t* text = reinterpret_cast<uint32_t*>(s_pm + p.pm_stride * kPmWords<K>);
  const int lane = threadIdx.x;
  const int row = blockIdx.x;
  const double thr = p.threshold;
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
    const int la1 = llen[lrow1];
    const bool use_hist = PRUNE && p.hist && la1 <= 255;  // (a bucket of a longer string can saturate its uint8)
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
      const int lb1 = cand ? rlen[rrow1] : 0;
      if (PRUNE && cand) {
        // step 1 at most the length bound, the later steps at most 1 each
        cand = 0.5 * indel_score(la1, lb1, min(la1, lb1)) + lev_top_tail(S) + 1e-6 >= eff;
      }
      st[1] += cand ? 1u : 0u;
      if (use_hist && cand && lb1 <= 255) {
        const uint4* hp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(rrow1) * 32);
        const uint4 h0 = hp[0], h1 = hp[1];
        const uint32_t hr[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        uint32_t l1 = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) l1 = __builtin_amdgcn_sad_u8(lh[q], hr[q], l1);
        const int lcs_ub = min(min(la1, lb1), (la1 + lb1 - static_cast<int>(l1)) >> 1);
        cand = 0.5 * indel_score(la1, lb1, lcs_ub) + lev_top_tail(S) + 1e-6 >= eff;
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
        const int la = llen[lf + a];
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
        const int lb = act ? rlen[rrow] : 0;
        const int nchars = wave_max_i32(lb);
        const int lcs = wide_lcs<K>(pm, text, nchars, lane, la);
        if (act) {
          score += indel_score(la, lb, lcs) * factor;
          if (s == S) live = false;                                        // all steps of the pair are in
          else if (PRUNE && score + factor + 1e-9 < eff) cand = live = false;  // the rest (< factor) cannot lift it
        }
      }
      lev_top_offer(L, cand, score, thr, io, jo, banned_start, banned_j);
    }
  }
  L.flush(ll > 0 ? 1 : 0, out, out_count, stats, st);
}

// ---------------------------------------------------------------------------------------------------------------- Jaccard
struct TopLevJacParams {
  int32_t n_left, n_right, k, lev_stride_l, lev_stride_r, cat_mode;
  double threshold;
  int32_t measure = NSM_MEASURE_UNION;  // read by RuntimeMeasure alone
};

// M: the measure (set_measure.hpp: part, later); the default is the Jaccard quotient lev_top_jac, the nsm_jaccard_*
// entries' instantiations.
template <int W, bool PRUNE, class Sink = TopLists<false>, class M = JaccardMeasure>
__global__ __launch_bounds__(kWave) void jaccard_levels_top_k_kernel(
    const int32_t* __restrict__ lids, const int32_t* __restrict__ lcnt, const int32_t* __restrict__ lnlev,
    const uint8_t* __restrict__ lplen, const uint64_t* __restrict__ lcat, const uint32_t* __restrict__ lfilt,
    const int32_t* __restrict__ lorig, const int32_t* __restrict__ rids, const int32_t* __restrict__ rcnt,
    const int32_t* __restrict__ rnlev, const uint8_t* __restrict__ rplen, const uint64_t* __restrict__ rcat,
    const uint32_t* __restrict__ rfilt, const int32_t* __restrict__ rorig, const int32_t* __restrict__ banned_start,
    const int32_t* __restrict__ banned_j, nsm_hit* __restrict__ list, nsm_hit* __restrict__ out,
    unsigned long long* __restrict__ out_count, unsigned long long* __restrict__ stats, const TopLevJacParams p,
    const typename Sink::Extra sx) {
  __shared__ uint32_t s_ids[W];                        // the left item's ids << 6
  const int lane = threadIdx.x;
  const int row = blockIdx.x;
  const double thr = p.threshold;
  const bool use_cat = p.cat_mode != NSM_CAT_NONE;
  const bool use_sig = PRUNE && lfilt && rfilt;
  const M meas(p.measure);

  const int ll = lnlev[row];
  const int nl = lcnt[row];
  const int io = lorig[row];
  const uint64_t catl = use_cat ? lcat[row] : 0ull;
  const uint8_t* __restrict__ lpl = lplen + static_cast<size_t>(row) * p.lev_stride_l;
  for (int e = lane; e < W; e += kWave) s_ids[e] = static_cast<uint32_t>(lids[static_cast<size_t>(row) * W + e]) << 6;
  __syncthreads();
  uint64_t sl = 0, sl1 = 0;
  if (use_sig) {
    const uint32_t* f = lfilt + static_cast<size_t>(row) * 8;
    sl = (static_cast<uint64_t>(f[1]) << 32) | f[0];
    sl1 = (static_cast<uint64_t>(f[6]) << 32) | f[5];
  }
  Sink L = Sink::open(list, nullptr, p.k, row, lane, sx);
  unsigned long long st[4] = {0, 0, 0, 0};

  if (ll > 0) {
    const int a1 = lpl[min(min(1, ll - 1), p.lev_stride_l - 1)];  // the left set step 1 compares
    for (int base = 0; base < p.n_right; base += kWave) {
      const int j = base + lane;
      const bool valid = j < p.n_right;
      const int jc = valid ? j : p.n_right - 1;
      const int lr = rnlev[jc];
      const int nr = rcnt[jc];
      const int jo = rorig[jc];
      const int S = max(ll, lr);
      const uint8_t* __restrict__ rpl = rplen + static_cast<size_t>(jc) * p.lev_stride_r;
      bool cand = valid && lr > 0 && (!use_cat || category_match(catl, rcat[jc], p.cat_mode));
      const double eff = L.eff(0, thr);
      st[0] += valid ? 1u : 0u;
      const int b1 = cand ? rpl[min(min(1, lr - 1), p.lev_stride_r - 1)] : 0;
      // step 1 <= its score with inter1 in common, every later step <= the measure's `later` (Jaccard: min(1, inter / max(a1,
      // b1)): its sets contain the step-1 sets)
      auto bound = [&](int inter1, int inter) {
        return 0.5 * meas.part(a1, b1, inter1) + lev_top_tail(S) * meas.later(a1, b1, inter) + 1e-6;
      };
      if (PRUNE && cand) cand = bound(min(a1, b1), min(nl, nr)) >= eff;
      st[1] += cand ? 1u : 0u;
      if (use_sig && cand) {
        const uint32_t* f = rfilt + static_cast<size_t>(jc) * 8;
        const uint64_t sr = ((static_cast<uint64_t>(f[1]) << 32) | f[0]) | kCollBits;
        const uint64_t sr1 = ((static_cast<uint64_t>(f[6]) << 32) | f[5]) | kCollBits;
        cand = bound(min(min(a1, b1), __popcll(sl1 & sr1)), min(min(nl, nr), __popcll(sl & sr))) >= eff;
      }
      st[2] += cand ? 1u : 0u;
      st[3] += cand ? 1u : 0u;
      if (!__any(cand)) continue;

      // ---- exact: position of every left id in the right row (>= 64: absent), then a byte-parallel count per step
      uint32_t r[W];
      const int4* rp = reinterpret_cast<const int4*>(rids + static_cast<size_t>(jc) * W);
#pragma unroll
      for (int q = 0; q < W / 4; ++q) {
        const int4 v = rp[q];
        r[4 * q + 0] = (static_cast<uint32_t>(v.x) << 6) | (4 * q + 0);
        r[4 * q + 1] = (static_cast<uint32_t>(v.y) << 6) | (4 * q + 1);
        r[4 * q + 2] = (static_cast<uint32_t>(v.z) << 6) | (4 * q + 2);
        r[4 * q + 3] = (static_cast<uint32_t>(v.w) << 6) | (4 * q + 3);
      }
      uint32_t posw[W / 4];
#pragma unroll
      for (int q = 0; q < W / 4; ++q) {
        posw[q] = 0xffffffffu;
        if (4 * q < nl) {  // wave-uniform
          uint32_t word = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t la = s_ids[4 * q + e];
            uint32_t mm = min3_u32(la ^ r[0], la ^ r[1], 255u);
#pragma unroll
            for (int b = 2; b < W; b += 2) mm = min3_u32(mm, la ^ r[b], la ^ r[b + 1]);
            word |= mm << (8 * e);  // mm <= 255: the position of the match, or >= 64
          }
          posw[q] = word;
        }
      }
      double score = 0.0, factor = 1.0;
      if (cand) {
        for (int s = 1; s <= S; ++s) {
          const int pl = lpl[min(min(s, ll - 1), p.lev_stride_l - 1)];
          const int pr = rpl[min(min(s, lr - 1), p.lev_stride_r - 1)];
          const uint32_t prrep = static_cast<uint32_t>(pr) * 0x01010101u;
          int inter = 0;
#pragma unroll
          for (int q = 0; q < W / 4; ++q) {
            if (4 * q < pl) {
              uint32_t x = posw[q];
              const int keep = pl - 4 * q;  // bytes of this word that belong to the level
              if (keep < 4) x |= 0xffffffffu << (8 * keep);
              const uint32_t y = (x | 0x80808080u) - prrep;  // per byte: x < pr (pr <= 64; bytes >= 128 never count)
              inter += __popc(~(y | x) & 0x80808080u);
            }
          }
          const double part = meas.part(pl, pr, inter);
          factor *= 0.5;
          score += part * factor;
          if (PRUNE && s < S && score + factor + 1e-9 < eff) {  // the rest (< factor) cannot lift it
            cand = false;
            break;
          }
        }
      }
      lev_top_offer(L, cand, score, thr, io, jo, banned_start, banned_j);
    }
  }
  L.flush(ll > 0 ? 1 : 0, out, out_count, stats, st);
}

}  // namespace nsm
