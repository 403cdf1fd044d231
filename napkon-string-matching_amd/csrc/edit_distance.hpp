// The Levenshtein primitive of the nsm_edit_* entries (nsm_hip_edit.h): the bit-vector edit-distance column update of
// Myers (1999) in Hyyro's (2003) form, the two scores built on it and the bounds the sweeps prune with.  It sits beside the
// bit-parallel LCS of the Indel kernels and reads the same match masks.
//
// The LEFT string is the pattern, la code units in ceil(la / 64) words.  VP = ~0, VN = 0, score = la; per text symbol c
//   D0 = (((PM[c] & VP) + VP) ^ VP) | PM[c] | VN          (the add carries across the words)
//   HP = VN | ~(D0 | VP);  HN = D0 & VP
//   score += bit la-1 of HP;  score -= bit la-1 of HN
//   HP = (HP << 1) | top;  HN = HN << 1                   (both shifts carry bit 63 into the next word)
//   VP = HN | ~(D0 | HP);  VN = HP & D0
// top = 1: score after the last symbol is the distance d(a, b).  top = 0: the minimum of score over its start value and
// its value after every symbol is w(a, b), the distance of a to its best occurrence in b (Sellers).  Bits above la - 1
// never reach lower ones (the add and both shifts only carry upwards), so the padding of the last word and every word
// above it are harmless.  A text symbol the pattern does not hold (an all-zero mask) still costs one edit: a text must
// end at its own length, never at a padded one.
#pragma once
#include "indel_wide.hpp"
#include "nsm_hip_edit.h"

namespace nsm {

// x: the distance d (NSM_METRIC_EDIT) or the occurrence distance w (NSM_METRIC_EDIT_WITHIN).  An empty string on either
// side: 0.0, the convention of indel_score.  Non-increasing in x (an IEEE division and subtraction are monotone).
__device__ __forceinline__ double edit_score(int la, int lb, int x, int metric) {
  if (la <= 0 || lb <= 0) return 0.0;
  const int den = metric == NSM_METRIC_EDIT ? max(la, lb) : la;
  return 1.0 - static_cast<double>(x) / static_cast<double>(den);
}

// The least x any pair of these lengths can have: |la - lb| edits only make the lengths agree; an occurrence is at most
// lb code units long.
__device__ __forceinline__ int edit_least(int la, int lb, int metric) {
  return metric == NSM_METRIC_EDIT ? abs(la - lb) : max(0, la - lb);
}

// Upper bound of the score of a row of la code units with a row of lb: the class bound of the RAW walk.  Exact (the
// score is monotone in x), and non-increasing away from la in lb: 1 - |la - lb| / max(la, lb) is lb / la below la and
// la / lb above; the occurrence bound is lb / la below la and flat 1 above.  0.0 where a side is empty.
__device__ __forceinline__ double edit_bound(int la, int lb, int metric) {
  return edit_score(la, lb, edit_least(la, lb, metric), metric);
}

// The greatest x whose score still reaches `eff` (la, lb >= 1), -1 when not even x = 0 does: the counterpart of
// indel_need.  The start is one above floor((1 - eff) den); score(x) >= eff means x / den <= 1 - eff up to roundings of a
// few 2^-53, far less than the 1 / den one step of x moves the quotient, so the start is never below the answer.  The
// walk down uses the exact double score: no pair is rounded away.
__device__ __forceinline__ int edit_most(int la, int lb, double eff, int metric) {
  const int den = metric == NSM_METRIC_EDIT ? max(la, lb) : la;
  if (eff <= 0.0) return den;  // every score is >= 0
  const double guess = floor((1.0 - eff) * static_cast<double>(den)) + 1.0;
  int x = static_cast<int>(fmax(-1.0, fmin(guess, static_cast<double>(den))));
  while (x >= 0 && edit_score(la, lb, x, metric) < eff) --x;
  return x;
}

// The carries between two words of the column update.
struct EditCarry {
  unsigned long long add = 0, hp, hn = 0;
  __device__ __forceinline__ explicit EditCarry(bool within) : hp(within ? 0ull : 1ull) {}
};

// One WORD of the column update on plain 64-bit values, words in ascending order with `c` handed on (the wave-per-pair
// kernels: every value is wave-uniform).  hp / hn: the word's horizontal deltas before the shift.
__device__ __forceinline__ void edit_word(unsigned long long& vp, unsigned long long& vn, unsigned long long m, EditCarry& c,
                                          unsigned long long& hp, unsigned long long& hn) {
  const unsigned long long u = m & vp;
  const unsigned long long s1 = vp + u;
  const unsigned long long s2 = s1 + c.add;
  c.add = static_cast<unsigned long long>(s1 < vp) | static_cast<unsigned long long>(s2 < s1);
  const unsigned long long d0 = (s2 ^ vp) | m | vn;
  hp = vn | ~(d0 | vp);
  hn = d0 & vp;
  const unsigned long long hps = (hp << 1) | c.hp, hns = (hn << 1) | c.hn;
  c.hp = hp >> 63;
  c.hn = hn >> 63;
  vp = hns | ~(d0 | hps);
  vn = hps & d0;
}

// The column of one lane: W words in registers (1..8), the add as one carry chain (add_chain, indel_wide.hpp).
template <int W>
struct EditColumn {
  unsigned long long vp[W], vn[W];
  unsigned long long last[W];  // bit la - 1, where the score is read
  int score, best;

  __device__ __forceinline__ void open(int la) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
      vp[q] = ~0ull;
      vn[q] = 0ull;
      last[q] = (la > 0 && ((la - 1) >> 6) == q) ? 1ull << ((la - 1) & 63) : 0ull;
    }
    score = best = la;
  }

  // one text symbol with the match masks m of the pattern; top: 1 for the distance, 0 for the occurrence
  __device__ __forceinline__ void step(const unsigned long long (&m)[W], unsigned long long top) {
    unsigned long long u[W], t[W], d0[W], hp[W], hn[W];
#pragma unroll
    for (int q = 0; q < W; ++q) u[q] = m[q] & vp[q];
    add_chain<W>(vp, u, t);
    unsigned long long up = 0ull, down = 0ull;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      d0[q] = (t[q] ^ vp[q]) | m[q] | vn[q];
      hp[q] = vn[q] | ~(d0[q] | vp[q]);
      hn[q] = d0[q] & vp[q];
      up |= hp[q] & last[q];
      down |= hn[q] & last[q];
    }
    score += static_cast<int>(up != 0ull) - static_cast<int>(down != 0ull);
    best = min(best, score);
#pragma unroll
    for (int q = W - 1; q >= 0; --q) {
      const unsigned long long hps = (hp[q] << 1) | (q ? hp[q - 1] >> 63 : top);
      const unsigned long long hns = (hn[q] << 1) | (q ? hn[q - 1] >> 63 : 0ull);
      vp[q] = hns | ~(d0[q] | hps);
      vn[q] = hps & d0[q];
    }
  }

  __device__ __forceinline__ int result(int metric) const { return metric == NSM_METRIC_EDIT ? score : best; }
};

// Host side: the name of a metric code for messages, nullptr for a code no entry accepts.
inline const char* metric_name(int32_t metric) {
  switch (metric) {
    case NSM_METRIC_INDEL: return "indel";
    case NSM_METRIC_EDIT: return "edit";
    case NSM_METRIC_EDIT_WITHIN: return "edit_within";
    default: return nullptr;
  }
}

// The check every nsm_edit_* entry runs right after its null-argument check, before any HIP call.
inline int check_metric(const char* who, int32_t metric) {
  if (metric_name(metric)) return 0;
  set_error("%s: unknown metric %d (0 indel, 1 edit, 2 edit_within)", who, metric);
  return NSM_E_BADARG;
}

}  // namespace nsm
