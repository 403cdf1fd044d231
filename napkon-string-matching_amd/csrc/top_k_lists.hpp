// Per-row top-k lists shared by the top-k kernels (top_k_raw.hip, top_k_levels.hip): a wavefront keeps the lists of its
// rows in stream-ordered scratch, each row's worst record is its floor, and the wave copies its lists out at the end.
// Below the lists, the host side the four entry functions share: scratch, argument checks, the clamping of k.
#pragma once
#include "nsm_common.hpp"

namespace nsm {

constexpr int kTopMaxK = 4096;   // largest k (after clamping to the right table's rows)

// add a wave's counters to stats (one atomic per counter)
__device__ __forceinline__ void wave_add_stats(unsigned long long* __restrict__ stats, const unsigned long long (&st)[4], int lane) {
  if (stats) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned long long v = st[c];
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off);
      if (lane == 0 && v) atomicAdd(stats + c, v);
    }
  }
}

// The lists of the wave's G rows.  Row g's records are list[(row0 + g) k .. + cnt(g)); only this wave reads or writes
// them, so a workgroup-scope fence orders lane 0's store before the wave's reloads (nothing else is needed).  The rows'
// state is held "one row per lane" -- lane g of cnt_v is row g's count -- and read with v_readlane: a loop over the rows
// needs no dynamically indexed register array (which would live in scratch).
//
// GROUPED: lists that hold at most ONE record per group of right rows, the group's best row so far (its representative),
// so a full list is k distinct groups.  The group ids of the records sit in a parallel int32 slice (grp[(row0 + g) k + q]
// is the group of list[(row0 + g) k + q]): a look-up scans that slice, it never gathers group[h.j] again.  Ungrouped
// lists never touch grp (nullptr) and ignore the group ids they are handed.
//
// The floor of a grouped list stays what it is for an ungrouped one -- the worst record of a full list -- and stays
// exact: it is a representative's score, a group's representative only ever improves, and the list holds k distinct
// groups, so the final k-th best representative is never below it.  A candidate that would improve its own group's
// record comes before a record of the list, hence before (or in place of) the worst one: beats() in front of an offer
// drops nothing that matters.
//
// TopLists is one of the two SINKS the kernels are templates over (the other: ScoreTally, score_tally.hpp).  A sink is
// opened from the kernel's list arguments plus its own `Extra` kernel argument (nothing here).
template <bool GROUPED>
struct TopLists {
  struct Extra {};
  __device__ static TopLists open(nsm_hit* list, int32_t* grp, int k, int row0, int lane, const Extra&) {
    return TopLists{list, grp, k, row0, lane};
  }

  nsm_hit* list;
  int32_t* grp;
  int k;
  int row0;
  int lane;
  int cnt_v = 0;
  double worst_v = 0.0;  // the floor, valid when the list is full
  int wj_v = 0;
  int wp_v = 0;
  int changes = 0;  // records that entered a list so far: the floors can only have moved when this did

  __device__ int cnt(int g) const { return __builtin_amdgcn_readlane(cnt_v, g); }
  __device__ bool full(int g) const { return cnt(g) == k; }
  __device__ double worst(int g) const { return readlane_f64(worst_v, g); }
  // max(threshold, floor): what a pair's upper bound must reach to matter to row g
  __device__ double eff(int g, double threshold) const { return full(g) ? fmax(threshold, worst(g)) : threshold; }
  // an eligible record (score >= threshold) enters row g's list
  __device__ bool beats(int g, double s, int j) const {
    if (!full(g)) return true;
    const double w = worst(g);
    return s > w || (s == w && j < __builtin_amdgcn_readlane(wj_v, g));
  }
  // the group of the right row with caller id jo, for offer_lanes (ungrouped: nothing is loaded)
  __device__ static int group_of(const int32_t* __restrict__ rgroup, int jo) {
    if constexpr (GROUPED) return rgroup[jo];
    else return 0;
  }

  // the worst record of row g's full list (lowest score, then largest j): one wave-wide reduction
  __device__ void rescan(int g) {
    const nsm_hit* row = list + static_cast<size_t>(row0 + g) * k;
    double s = __builtin_inf();
    int j = -1, pos = -1;
    for (int q = lane; q < k; q += kWave) {
      const nsm_hit h = row[q];
      if (h.score < s || (h.score == s && h.j > j)) { s = h.score; j = h.j; pos = q; }
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const double s2 = __shfl_xor(s, off);
      const int j2 = __shfl_xor(j, off), p2 = __shfl_xor(pos, off);
      if (s2 < s || (s2 == s && j2 > j)) { s = s2; j = j2; pos = p2; }
    }
    if (lane == g) { worst_v = s; wj_v = j; wp_v = pos; }
  }

  // wave-uniform call, all lanes enabled: (s, i, j) of group gid enters row g's list if it belongs there
  __device__ void offer(int g, double s, int i, int j, int gid) {
    if (!beats(g, s, j)) return;
    const size_t row = static_cast<size_t>(row0 + g) * k;
    const int n = cnt(g);
    int pos = -1;  // of the group's record in the list
    if constexpr (GROUPED) {
      // is the group in the list, and does the candidate come before its record?  64 group ids per pass
      bool improves = false;
      for (int base = 0; base < n; base += kWave) {
        const int q = base + lane;
        const bool same = q < n && grp[row + q] == gid;
        bool better = false;
        if (same) {
          const nsm_hit cur = list[row + q];
          better = s > cur.score || (s == cur.score && j < cur.j);
        }
        const unsigned long long found = __ballot(same);
        if (found) {
          pos = base + __builtin_ctzll(found);
          improves = __ballot(better) != 0ull;
          break;
        }
      }
      if (pos >= 0 && !improves) return;
    }
    const bool was_full = n == k;
    const bool append = pos < 0 && !was_full;
    const int worst_pos = __builtin_amdgcn_readlane(wp_v, g);
    // present: its own slot; absent: the next free slot, or the worst record's
    const int slot = pos >= 0 ? pos : (was_full ? worst_pos : n);
    if (lane == 0) {
      nsm_hit h;
      h.score = s;
      h.i = i;
      h.j = j;
      list[row + slot] = h;
      if constexpr (GROUPED) grp[row + slot] = gid;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    ++changes;
    if (append && lane == g) ++cnt_v;
    // the worst record is unknown (the list has just filled up) or has just been overwritten
    if (append ? slot + 1 == k : (was_full && slot == worst_pos)) rescan(g);
  }

  // lanes with `ok` hold an eligible record (s, j) of group gid for row g: offer them one by one (the floor rises on
  // the way)
  __device__ void offer_lanes(int g, bool ok, double s, int i, int j, int gid) {
    for (unsigned long long todo = __ballot(ok); todo; todo &= todo - 1ull) {
      const int leader = __builtin_ctzll(todo);
      offer(g, readlane_f64(s, leader), i, __builtin_amdgcn_readlane(j, leader),
            GROUPED ? __builtin_amdgcn_readlane(gid, leader) : 0);
    }
  }

  // copy the lists to out[*out_count ..] (one atomic per wave) and add the wave's counters to stats
  __device__ void flush(int rows, nsm_hit* __restrict__ out, unsigned long long* __restrict__ out_count,
                        unsigned long long* __restrict__ stats, const unsigned long long (&st)[4]) {
    int total = 0;
    for (int g = 0; g < rows; ++g) total += cnt(g);
    unsigned long long base = 0;
    if (lane == 0 && total) base = atomicAdd(out_count, static_cast<unsigned long long>(total));
    base = readlane_u64(base, 0);
    for (int g = 0; g < rows; ++g) {
      const nsm_hit* row = list + static_cast<size_t>(row0 + g) * k;
      const int n = cnt(g);
      for (int q = lane; q < n; q += kWave) out[base + q] = row[q];
      base += n;
    }
    wave_add_stats(stats, st, lane);
  }
};

// ------------------------------------------------------------------------------------------------------------- host side
// The stream-ordered scratch of one top-k launch: the lists, and for a grouped query the group ids of their records.
struct ListScratch {
  hipStream_t s;
  nsm_hit* list = nullptr;
  int32_t* glist = nullptr;  // stays null for an ungrouped query

  int alloc(int n_left, int k, bool grouped) {
    const size_t n = static_cast<size_t>(n_left) * static_cast<size_t>(k);
    if (int st = hip_status(hipMallocAsync(reinterpret_cast<void**>(&list), n ? n * sizeof(nsm_hit) : 1, s), "top_k list scratch"))
      return st;
    if (!grouped) return 0;
    const int st = hip_status(hipMallocAsync(reinterpret_cast<void**>(&glist), n ? n * sizeof(int32_t) : 1, s), "top_k group scratch");
    if (st) (void)hipFreeAsync(list, s);
    return st;
  }
  // Free behind the kernel on the same stream.  The call's status: the launch's, else the list's, else the groups'.
  int release(int launch_status) {
    const int fst = hip_status(hipFreeAsync(list, s), "top_k list scratch");
    const int gst = glist ? hip_status(hipFreeAsync(glist, s), "top_k group scratch") : 0;
    return launch_status ? launch_status : (fst ? fst : gst);
  }
};

// What every launch gets besides its tables: the scratch, the output and the stream (sc.s).
struct TopOut {
  ListScratch sc;
  nsm_hit* out;
  unsigned long long* out_count;
  unsigned long long* stats;
};

// Both string tables of a query: equal strides, a stride the kernels have, equal alphabets of at most 255 symbols.
static int check_str_tables(const char* who, const nsm_str_table* l, const nsm_str_table* r) {
  if (l->stride != r->stride) {
    set_error("%s: strides differ (%d, %d)", who, l->stride, r->stride);
    return NSM_E_BADARG;
  }
  if (l->stride != 64 && l->stride != 128 && l->stride != 256 && l->stride != 512) {
    set_error("%s: stride %d unsupported (64, 128, 256 or 512 code units)", who, l->stride);
    return NSM_E_UNSUPPORTED;
  }
  if (l->alphabet != r->alphabet || l->alphabet < 1 || l->alphabet > 255) {
    set_error("%s: alphabets differ or exceed 255 (%d, %d)", who, l->alphabet, r->alphabet);
    return NSM_E_BADARG;
  }
  return 0;
}

static int check_set_tables(const char* who, const nsm_set_table* l, const nsm_set_table* r) {
  if (l->width != r->width || (l->width != 16 && l->width != 32 && l->width != 64)) {
    set_error("%s: width %d/%d unsupported (both sides 16, 32 or 64)", who, l->width, r->width);
    return NSM_E_BADARG;
  }
  return 0;
}

// ---- the table checks of a whole query, shared by the top-k entries and the profile entries (profile_*.hip)
static int check_raw_str_query(const char* who, const nsm_str_table* left, const nsm_str_table* right) {
  if (int st = check_str_tables(who, left, right)) return st;
  if (left->n < 0 || right->n < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if (!left->codes || !left->len || !left->orig || !right->codes || !right->len_start || !right->orig) {
    set_error("%s: table has a null column (the right table needs len_start)", who);
    return NSM_E_BADARG;
  }
  return 0;
}

static int check_raw_set_query(const char* who, const nsm_set_table* left, const nsm_set_table* right) {
  if (int st = check_set_tables(who, left, right)) return st;
  if (left->n < 0 || right->n < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if (!left->ids || !left->cnt || !left->orig || !right->ids || !right->size_start || !right->orig) {
    set_error("%s: table has a null column (the right table needs size_start)", who);
    return NSM_E_BADARG;
  }
  return 0;
}

// category predicate and blacklist of a levels query
static int check_common(const char* who, int32_t category_mode, bool has_cat, const int32_t* bs, const int32_t* bj) {
  if (category_mode != NSM_CAT_NONE && category_mode != NSM_CAT_INTERSECT && category_mode != NSM_CAT_INTERSECT_OR_BOTH_EMPTY) {
    set_error("%s: unknown category_mode %d", who, category_mode);
    return NSM_E_BADARG;
  }
  if (category_mode != NSM_CAT_NONE && !has_cat) {
    set_error("%s: a category predicate needs `cat` on both sides", who);
    return NSM_E_BADARG;
  }
  if ((bs == nullptr) != (bj == nullptr)) {
    set_error("%s: banned_start and banned_j go together", who);
    return NSM_E_BADARG;
  }
  return 0;
}

static int check_levels_str_query(const char* who, const nsm_level_items* left, const nsm_str_table* left_strings,
                                  const nsm_level_items* right, const nsm_str_table* right_strings, int32_t category_mode,
                                  const int32_t* banned_start, const int32_t* banned_j) {
  if (int st = check_str_tables(who, left_strings, right_strings)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) {
    set_error("%s: partitioned item tables are not supported (an item must be one row: encode with partition=False)", who);
    return NSM_E_UNSUPPORTED;
  }
  if (left->n < 0 || right->n < 0) {
    set_error("%s: negative item count", who);
    return NSM_E_BADARG;
  }
  if (!left->first || !left->nlev || !left->orig || !right->first || !right->nlev || !right->orig || !left_strings->codes ||
      !left_strings->len || !right_strings->codes || !right_strings->len) {
    set_error("%s: table has a null column", who);
    return NSM_E_BADARG;
  }
  if (int st = check_common(who, category_mode, left->cat && right->cat, banned_start, banned_j)) return st;
  return 0;
}

static int check_levels_set_query(const char* who, const nsm_set_table* left, const nsm_set_table* right, int32_t category_mode,
                                  const int32_t* banned_start, const int32_t* banned_j) {
  if (int st = check_set_tables(who, left, right)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) {
    set_error("%s: partitioned tables are not supported (an item must be one row: encode with partition=False)", who);
    return NSM_E_UNSUPPORTED;
  }
  if (left->n < 0 || right->n < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if (!left->ids || !left->cnt || !left->nlev || !left->plen || !left->orig || !right->ids || !right->cnt || !right->nlev ||
      !right->plen || !right->orig || left->max_levels < 1 || right->max_levels < 1) {
    set_error("%s: table has a null column (levels tables need nlev and plen)", who);
    return NSM_E_BADARG;
  }
  if (int st = check_common(who, category_mode, left->cat && right->cat, banned_start, banned_j)) return st;
  return 0;
}

static int check_k(const char* who, int32_t k) {
  if (k < 1) {
    set_error("%s: k = %d (must be >= 1)", who, k);
    return NSM_E_BADARG;
  }
  return 0;
}

// k after clamping to the right side, or an error status (k < 1: NSM_E_BADARG, beyond kTopMaxK: NSM_E_UNSUPPORTED)
static int clamp_k(const char* who, int32_t k, int32_t n_right, int* k_eff) {
  if (int st = check_k(who, k)) return st;
  *k_eff = k < n_right ? k : n_right;
  if (*k_eff > kTopMaxK) {
    set_error("%s: k = %d exceeds the supported %d", who, *k_eff, kTopMaxK);
    return NSM_E_UNSUPPORTED;
  }
  return 0;
}

}  // namespace nsm
