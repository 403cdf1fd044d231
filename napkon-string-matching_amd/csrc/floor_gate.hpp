// The gate sink of the floor grids (floors_raw.hip, floors_levels.hip): the top-k kernels with this object in place of
// TopLists (top_k_lists.hpp) emit every pair that reaches the threshold AND its own items' floors -- a threshold grid whose
// threshold is per item.  Same interface as the other two sinks (eff, beats, offer_lanes, group_of, changes, flush), so no
// kernel body exists twice.
//
//   * the floors are the caller's, indexed by caller id (the tables' `orig`), and never move: `changes` is a constant 0
//     and eff() is max(threshold, left floor) from the first pair on, so the class walk and every bound prune against the
//     FINAL value -- at least as hard as a profile sweep at the same threshold, which prunes against the threshold alone;
//   * left floors are "one row per lane": lane g holds the floor of row row0 + g (-inf without a left array), read with
//     v_readlane; the right floor is a per-lane load of right_floor[jo], made only for a score that passed the left one;
//   * the comparisons are the exact IEEE >=, no margin.  A NaN floor admits nothing (every >= against it is false) and
//     prunes nothing (fmax drops it): less pruning, never a lost record;
//   * an accepted wave appends with one ballot and one atomic (emit_hits_wave, nsm_common.hpp): the threshold grids'
//     protocol -- records go behind what *hit_count already holds, the counter keeps counting past `capacity` -- so the
//     caller's grow-and-retry works unchanged.  The output size is data-dependent (a cohort of identical items has N M
//     best records), hence capacity and retry instead of a bound known in advance.
#pragma once
#include "top_k_lists.hpp"

namespace nsm {

// What a floor kernel gets besides its tables.  `open` is only handed a row number, so the left table's caller ids and
// row count travel here.
struct FloorOut {
  const double* left_floor;    // by left caller id, or nullptr
  const double* right_floor;   // by right caller id, or nullptr
  const int32_t* lorig;        // the left table's orig
  int32_t n_left;
  nsm_hit* hits;
  unsigned long long capacity;
  unsigned long long* hit_count;
};

struct FloorGate {
  using Extra = FloorOut;
  static constexpr int changes = 0;  // the floors never move

  const double* right_floor;
  nsm_hit* hits;
  unsigned long long capacity;
  unsigned long long* hit_count;
  int lane;
  double floor_v;  // lane g: the floor of row row0 + g

  __device__ static FloorGate open(nsm_hit*, int32_t*, int, int row0, int lane, const FloorOut& o) {
    double f = -__builtin_inf();
    if (o.left_floor && row0 + lane < o.n_left) f = o.left_floor[o.lorig[row0 + lane]];  // (the last group is partial)
    return FloorGate{o.right_floor, o.hits, o.capacity, o.hit_count, lane, f};
  }

  __device__ double eff(int g, double threshold) const { return fmax(threshold, readlane_f64(floor_v, g)); }
  // an eligible record (score >= threshold) of row g and the right row with caller id jo passes both floors
  __device__ bool beats(int g, double s, int jo) const {
    return s >= readlane_f64(floor_v, g) && (!right_floor || s >= right_floor[jo]);
  }
  __device__ static int group_of(const int32_t*, int) { return 0; }

  // lanes with `ok` hold a record (s, i, j) that passed the gate (wave-uniform call, all lanes enabled)
  __device__ void offer_lanes(int, bool ok, double s, int i, int j, int) {
    emit_hits_wave(hits, capacity, hit_count, ok, s, i, j);
  }

  __device__ void flush(int, nsm_hit*, unsigned long long*, unsigned long long* __restrict__ stats,
                        const unsigned long long (&st)[4]) {
    wave_add_stats(stats, st, lane);
  }
};

// ------------------------------------------------------------------------------------------------------------- host side
// What the four entries check first: null tables, the hit buffer.
static int check_floor_out(const char* who, bool tables, const nsm_hit* hits, uint64_t capacity, const void* hit_count) {
  if (!tables || !hit_count || (!hits && capacity)) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  return 0;
}

// ... then the row counts: NSM_E_BADARG for a negative one, else 0 with *empty saying whether a side has no rows (the
// entry then returns 0 before it looks at the columns, as the threshold grids do).
static int check_floor_rows(const char* who, int32_t n_left, int32_t n_right, bool* empty) {
  if (n_left < 0 || n_right < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  *empty = n_left == 0 || n_right == 0;
  return 0;
}

}  // namespace nsm
