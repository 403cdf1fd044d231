// Edge support and truss peeling of hit lists (include/nsm_hip_support.h): per record the number of common neighbours of
// its two ends, in the graph of all lists together or in its (min_support + 2)-truss -- match groups that do not chain.
//
//   * gather   one pass over the lists: the id check, the number of edge records, and two arcs (u : v) and (v : u) per
//              edge record, packed as (u << b) | v with b the bits `nodes` needs.  Appends are wave-aggregated: one atomic
//              per wavefront (as emit_hits_wave does for hits).  The host reads verdict and count once.
//   * index    ONE radix sort (rocPRIM) over the 2b bits of the arcs, equal neighbours dropped (rocPRIM unique), then a
//              row offset per node by binary search: the sorted adjacency of the graph, every edge held twice.
//   * count    the support ONCE per distinct edge (the arc with u < v): the intersection of two sorted neighbour rows.
//              The shorter row is walked, the longer one binary-searched.  A lane takes an edge whose shorter row has fewer
//              than NSM_SUPPORT_WAVE_MIN arcs; the others are queued (wave-aggregated) and a second launch gives each a whole
//              wavefront: the shorter row strided over the lanes, a ballot count per stride.
//   * kill     (min_support > 0) clears the alive flag of BOTH arcs of every alive edge below min_support and counts them;
//              the host reads the count and stops after a round that removed nothing.  The count launches of the next round
//              skip dead arcs.  Rounds are ordered by kernel boundaries alone: no kernel waits for another workgroup.
//   * write    per record: look its edge up (duplicates and the second orientation cost a lookup, not an intersection).
// Why the kill launch races with nothing: it reads alive[t] and sup[t] of arcs with u < v only, each by the one lane that
// owns t, and writes alive[t] and the flag of the mirror arc (v : u), which no lane of that launch reads.
#include "nsm_common.hpp"

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "nsm_hip_support.h"

namespace nsm {

// The length of an edge's SHORTER neighbour row from which a whole wavefront intersects it (DESIGN.md section 4.18 has the
// sweep).  Below it a single lane walks the row.
#ifndef NSM_SUPPORT_WAVE_MIN
#define NSM_SUPPORT_WAVE_MIN 32
#endif
constexpr uint32_t kSupportWaveMin = NSM_SUPPORT_WAVE_MIN;
constexpr unsigned kMaxSupportBlocks = 2048;

// control words of the call's scratch (64 bits each), zeroed per call
enum { kSupBad = 0, kSupEdges = 1, kSupArcs = 2, kSupQueue = 3, kSupRemoved = 4, kSupWords = 8 };

using arc_t = unsigned long long;

__device__ __forceinline__ unsigned long long support_wave_sum(unsigned long long x) {
  for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d, kWave);
  return x;
}

// The lane's rank among the lanes of `who` below it.
__device__ __forceinline__ uint32_t lane_rank(unsigned long long who) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(who >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(who), 0u));
}

// The first arc of [lo, hi) that is not below `key` (hi if none).
__device__ __forceinline__ uint32_t arc_lower_bound(const arc_t* __restrict__ arcs, uint32_t lo, uint32_t hi, arc_t key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (arcs[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Every wavefront walks whole 64-record strides (the loop bound is wave-uniform), so that the ballot sees all lanes.
__global__ __launch_bounds__(kBlock) void support_gather_kernel(const nsm_hit* __restrict__ hits, unsigned long long n, uint32_t nl,
                                                                uint32_t nr, uint32_t left_base, uint32_t right_base,
                                                                double min_score, int bits, arc_t* __restrict__ arcs,
                                                                unsigned long long* __restrict__ ctrl) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  bool bad = false;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kBlock + (threadIdx.x - lane); base < n;
       base += stride) {
    const unsigned long long r = base + lane;
    bool edge = false;
    uint32_t u = 0, v = 0;
    if (r < n) {
      const nsm_hit h = hits[r];
      const bool out = static_cast<uint32_t>(h.i) >= nl || static_cast<uint32_t>(h.j) >= nr;  // (a negative id is a huge unsigned)
      bad |= out;
      u = left_base + static_cast<uint32_t>(h.i);
      v = right_base + static_cast<uint32_t>(h.j);
      edge = !out && h.score >= min_score && u != v;  // (a NaN is no edge)
    }
    const unsigned long long who = __ballot(edge);
    if (who == 0ull) continue;
    const int leader = __builtin_ctzll(who);
    unsigned long long pos = 0;
    if (lane == leader) pos = atomicAdd(ctrl + kSupEdges, static_cast<unsigned long long>(__popcll(who)));
    pos = readlane_u64(pos, leader);
    if (edge) {
      // (pos + rank < the edge records of all lists <= the records the arcs were sized for)
      const unsigned long long at = 2ull * (pos + lane_rank(who));
      arcs[at] = (static_cast<arc_t>(u) << bits) | v;
      arcs[at + 1] = (static_cast<arc_t>(v) << bits) | u;
    }
  }
  if (bad) ctrl[kSupBad] = 1ull;
}

// off[w] = the first distinct arc whose source is >= w, for w = 0 .. nodes (off[nodes] = the number of distinct arcs).
__global__ __launch_bounds__(kBlock) void support_offsets_kernel(const arc_t* __restrict__ arcs,
                                                                 const unsigned long long* __restrict__ ctrl, uint32_t nodes,
                                                                 int bits, uint32_t* __restrict__ off) {
  const uint32_t d = static_cast<uint32_t>(ctrl[kSupArcs]);
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long w = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; w <= nodes; w += stride)
    off[w] = arc_lower_bound(arcs, 0u, d, static_cast<arc_t>(w) << bits);
}

// The two neighbour rows of the edge (u, v): the shorter one [a0, a1), the longer one [b0, b1), which is node b's.
struct EdgeRows {
  uint32_t a0, a1, b0, b1, b;
};
__device__ __forceinline__ EdgeRows edge_rows(const uint32_t* __restrict__ off, uint32_t u, uint32_t v) {
  EdgeRows e;
  e.a0 = off[u], e.a1 = off[u + 1], e.b0 = off[v], e.b1 = off[v + 1], e.b = v;
  if (e.a1 - e.a0 > e.b1 - e.b0) {
    const uint32_t s0 = e.a0, s1 = e.a1;
    e.a0 = e.b0, e.a1 = e.b1, e.b0 = s0, e.b1 = s1, e.b = u;
  }
  return e;
}

// One lane per distinct arc.  `alive` is null while nothing can be dead (min_support == 0).
__global__ __launch_bounds__(kBlock) void support_count_kernel(const arc_t* __restrict__ arcs,
                                                               unsigned long long* __restrict__ ctrl,
                                                               const uint32_t* __restrict__ off,
                                                               const uint8_t* __restrict__ alive, int32_t* __restrict__ sup,
                                                               uint32_t* __restrict__ queue, int bits, uint32_t wave_min) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  const uint32_t d = static_cast<uint32_t>(ctrl[kSupArcs]);
  const arc_t mask = (1ull << bits) - 1ull;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kBlock + (threadIdx.x - lane); base < d;
       base += stride) {
    const unsigned long long t = base + lane;
    bool wide = false;
    if (t < d) {
      const arc_t key = arcs[t];
      const uint32_t u = static_cast<uint32_t>(key >> bits), v = static_cast<uint32_t>(key & mask);
      if (u < v && (!alive || alive[t])) {
        const EdgeRows e = edge_rows(off, u, v);
        if (e.a1 - e.a0 >= wave_min) {
          wide = true;
        } else {
          const arc_t row = static_cast<arc_t>(e.b) << bits;
          int32_t c = 0;
          uint32_t lo = e.b0;  // (both rows ascend: the search goes on from the last landing place)
          for (uint32_t p = e.a0; p < e.a1 && lo < e.b1; ++p) {
            if (alive && !alive[p]) continue;
            const arc_t want = row | (arcs[p] & mask);
            lo = arc_lower_bound(arcs, lo, e.b1, want);
            if (lo < e.b1 && arcs[lo] == want && (!alive || alive[lo])) c += 1;
          }
          sup[t] = c;
        }
      }
    }
    const unsigned long long who = __ballot(wide);
    if (who == 0ull) continue;
    const int leader = __builtin_ctzll(who);
    unsigned long long pos = 0;
    if (lane == leader) pos = atomicAdd(ctrl + kSupQueue, static_cast<unsigned long long>(__popcll(who)));
    pos = readlane_u64(pos, leader);
    if (wide) queue[pos + lane_rank(who)] = static_cast<uint32_t>(t);  // (at most one entry per arc with u < v: <= d / 2)
  }
}

// One wavefront per queued edge: the shorter row strided over the lanes, each lane binary-searches the longer row.
__global__ __launch_bounds__(kBlock) void support_count_wave_kernel(const arc_t* __restrict__ arcs,
                                                                    const unsigned long long* __restrict__ ctrl,
                                                                    const uint32_t* __restrict__ off,
                                                                    const uint8_t* __restrict__ alive, int32_t* __restrict__ sup,
                                                                    const uint32_t* __restrict__ queue, int bits) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t queued = static_cast<uint32_t>(ctrl[kSupQueue]);
  const arc_t mask = (1ull << bits) - 1ull;
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  for (uint32_t e = static_cast<uint32_t>(wave_first(static_cast<int>(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave)));
       e < queued; e += waves) {
    const uint32_t t = queue[e];
    const arc_t key = arcs[t];
    const EdgeRows rows = edge_rows(off, static_cast<uint32_t>(key >> bits), static_cast<uint32_t>(key & mask));
    const arc_t row = static_cast<arc_t>(rows.b) << bits;
    int32_t c = 0;
    for (uint32_t p0 = rows.a0; p0 < rows.a1; p0 += kWave) {
      const uint32_t p = p0 + lane;
      bool hit = false;
      if (p < rows.a1 && (!alive || alive[p])) {
        const arc_t want = row | (arcs[p] & mask);
        const uint32_t at = arc_lower_bound(arcs, rows.b0, rows.b1, want);
        hit = at < rows.b1 && arcs[at] == want && (!alive || alive[at]);
      }
      c += __popcll(__ballot(hit));
    }
    if (lane == 0) sup[t] = c;
  }
}

__global__ __launch_bounds__(kBlock) void support_kill_kernel(const arc_t* __restrict__ arcs, unsigned long long* __restrict__ ctrl,
                                                              const uint32_t* __restrict__ off, uint8_t* __restrict__ alive,
                                                              const int32_t* __restrict__ sup, int bits, int32_t min_support) {
  const uint32_t d = static_cast<uint32_t>(ctrl[kSupArcs]);
  const arc_t mask = (1ull << bits) - 1ull;
  unsigned long long removed = 0;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; t < d; t += stride) {
    const arc_t key = arcs[t];
    const uint32_t u = static_cast<uint32_t>(key >> bits), v = static_cast<uint32_t>(key & mask);
    if (u >= v || !alive[t] || sup[t] >= min_support) continue;
    const uint32_t hi = off[v + 1];
    const uint32_t mirror = arc_lower_bound(arcs, off[v], hi, (static_cast<arc_t>(v) << bits) | u);
    alive[t] = 0;
    if (mirror < hi) alive[mirror] = 0;  // (always: every edge is held as both arcs)
    removed += 1;
  }
  removed = support_wave_sum(removed);  // (the lanes meet again here: whole waves were launched)
  if ((threadIdx.x & (kWave - 1)) == 0 && removed) atomicAdd(ctrl + kSupRemoved, removed);
}

__global__ __launch_bounds__(kBlock) void support_write_kernel(const nsm_hit* __restrict__ hits, unsigned long long n,
                                                               uint32_t left_base, uint32_t right_base, double min_score,
                                                               int bits, const arc_t* __restrict__ arcs,
                                                               const uint32_t* __restrict__ off,
                                                               const uint8_t* __restrict__ alive,
                                                               const int32_t* __restrict__ sup, int32_t* __restrict__ out) {
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long r = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += stride) {
    const nsm_hit h = hits[r];
    const uint32_t u = left_base + static_cast<uint32_t>(h.i), v = right_base + static_cast<uint32_t>(h.j);
    int32_t word = -1;
    if (h.score >= min_score && u != v) {
      const uint32_t a = u < v ? u : v, b = u < v ? v : u;
      const arc_t key = (static_cast<arc_t>(a) << bits) | b;
      const uint32_t hi = off[a + 1];
      const uint32_t at = arc_lower_bound(arcs, off[a], hi, key);
      if (at < hi && arcs[at] == key) word = (!alive || alive[at]) ? sup[at] : -2;  // (always found: the record made the arc)
    }
    out[r] = word;
  }
}

__global__ __launch_bounds__(kBlock) void support_stats_kernel(const arc_t* __restrict__ arcs,
                                                               const unsigned long long* __restrict__ ctrl,
                                                               const uint8_t* __restrict__ alive, const int32_t* __restrict__ sup,
                                                               int bits, unsigned long long rounds,
                                                               unsigned long long* __restrict__ stats) {
  const uint32_t d = static_cast<uint32_t>(ctrl[kSupArcs]);
  const arc_t mask = (1ull << bits) - 1ull;
  unsigned long long edges = 0, sum = 0;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; t < d; t += stride) {
    const arc_t key = arcs[t];
    if (static_cast<uint32_t>(key >> bits) < static_cast<uint32_t>(key & mask) && (!alive || alive[t])) {
      edges += 1;
      sum += static_cast<unsigned long long>(sup[t]);
    }
  }
  edges = support_wave_sum(edges);
  sum = support_wave_sum(sum);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (edges) atomicAdd(stats + 2, edges);
    if (sum) atomicAdd(stats + 4, sum);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicAdd(stats + 0, ctrl[kSupEdges]);
    atomicAdd(stats + 1, static_cast<unsigned long long>(d / 2u));
    atomicAdd(stats + 3, rounds);
  }
}

static unsigned support_blocks(unsigned long long n) {
  const unsigned long long b = (n + kBlock - 1) / kBlock;
  return b < kMaxSupportBlocks ? static_cast<unsigned>(b ? b : 1u) : kMaxSupportBlocks;
}

// Stream-ordered scratch, freed when the call leaves.
struct SupportScratch {
  hipStream_t s;
  void* p[3] = {nullptr, nullptr, nullptr};
  explicit SupportScratch(hipStream_t stream) : s(stream) {}
  ~SupportScratch() {
    for (void* q : p)
      if (q) (void)hipFreeAsync(q, s);
  }
};

static size_t round_up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

static int support_run(const nsm_hit_list* lists, int32_t n_lists, uint32_t nodes, double min_score, int32_t min_support,
                       int32_t* const* support, unsigned long long* stats, hipStream_t s, unsigned long long records) {
  int bits = 1;
  while ((1ull << bits) < nodes) ++bits;  // nodes <= 2^31 - 1: at most 31 bits, 62 per arc
  SupportScratch scratch(s);
  // first block: control words | row offsets [nodes + 1] | arcs [2 per record]
  const size_t off_at = round_up(kSupWords * sizeof(unsigned long long));
  const size_t arcs_at = off_at + round_up((static_cast<size_t>(nodes) + 1) * sizeof(uint32_t));
  hipError_t e = hipMallocAsync(&scratch.p[0], arcs_at + 2 * records * sizeof(arc_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_support_hits: stream-ordered scratch");
  char* const first = static_cast<char*>(scratch.p[0]);
  unsigned long long* const ctrl = reinterpret_cast<unsigned long long*>(first);
  uint32_t* const off = reinterpret_cast<uint32_t*>(first + off_at);
  arc_t* const gathered = reinterpret_cast<arc_t*>(first + arcs_at);
  e = hipMemsetAsync(ctrl, 0, kSupWords * sizeof(unsigned long long), s);
  if (e != hipSuccess) return hip_status(e, "nsm_support_hits: control words");
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (l.n)
      hipLaunchKernelGGL(support_gather_kernel, dim3(support_blocks(l.n)), dim3(kBlock), 0, s, l.hits, l.n,
                         static_cast<uint32_t>(l.left_ids), static_cast<uint32_t>(l.right_ids),
                         static_cast<uint32_t>(l.left_base), static_cast<uint32_t>(l.right_base), min_score, bits, gathered, ctrl);
  }
  unsigned long long verdict[2] = {0, 0};  // bad, edge records
  e = hipMemcpyAsync(verdict, ctrl, sizeof(verdict), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_status(e, "nsm_support_hits: checks");
  if (verdict[0]) {
    set_error("nsm_support_hits: a record's id is outside its list's [0, left_ids) x [0, right_ids)");
    return NSM_E_BADARG;
  }
  const unsigned long long m = 2 * verdict[1];  // arcs, before equal ones are dropped
  const arc_t* arcs = gathered;
  uint8_t* alive = nullptr;
  int32_t* sup = nullptr;
  unsigned long long rounds = 1;  // (no edge at all: one counting pass over nothing)
  if (m) {
    // second block: the sort's other buffer [m] | supports [m] | queue [m / 2] | alive flags [m]
    const size_t sup_at = round_up(m * sizeof(arc_t));
    const size_t queue_at = sup_at + round_up(m * sizeof(int32_t));
    const size_t alive_at = queue_at + round_up((m / 2) * sizeof(uint32_t));
    e = hipMallocAsync(&scratch.p[1], alive_at + m, s);
    if (e != hipSuccess) return hip_status(e, "nsm_support_hits: stream-ordered scratch");
    char* const second = static_cast<char*>(scratch.p[1]);
    sup = reinterpret_cast<int32_t*>(second + sup_at);
    uint32_t* const queue = reinterpret_cast<uint32_t*>(second + queue_at);
    ::rocprim::double_buffer<arc_t> keys(gathered, reinterpret_cast<arc_t*>(second));
    const unsigned end_bit = static_cast<unsigned>(2 * bits);
    size_t sort_bytes = 0, unique_bytes = 0;
    e = ::rocprim::radix_sort_keys(nullptr, sort_bytes, keys, static_cast<size_t>(m), 0u, end_bit, s);
    if (e != hipSuccess) return hip_status(e, "radix_sort_keys (size)");
    e = ::rocprim::unique(nullptr, unique_bytes, gathered, gathered, ctrl + kSupArcs, static_cast<size_t>(m),
                          ::rocprim::equal_to<arc_t>(), s);
    if (e != hipSuccess) return hip_status(e, "unique (size)");
    const size_t temp_bytes = sort_bytes > unique_bytes ? sort_bytes : unique_bytes;
    e = hipMallocAsync(&scratch.p[2], temp_bytes ? temp_bytes : 1, s);
    if (e != hipSuccess) return hip_status(e, "nsm_support_hits: stream-ordered scratch");
    e = ::rocprim::radix_sort_keys(scratch.p[2], sort_bytes, keys, static_cast<size_t>(m), 0u, end_bit, s);
    if (e != hipSuccess) return hip_status(e, "radix_sort_keys");
    // (the distinct arcs go to whichever buffer the last digit pass left free)
    e = ::rocprim::unique(scratch.p[2], unique_bytes, keys.current(), keys.alternate(), ctrl + kSupArcs, static_cast<size_t>(m),
                          ::rocprim::equal_to<arc_t>(), s);
    if (e != hipSuccess) return hip_status(e, "unique");
    arcs = keys.alternate();
    hipLaunchKernelGGL(support_offsets_kernel, dim3(support_blocks(static_cast<unsigned long long>(nodes) + 1)), dim3(kBlock), 0, s,
                       arcs, ctrl, nodes, bits, off);
    if (min_support > 0) {
      alive = reinterpret_cast<uint8_t*>(second + alive_at);
      e = hipMemsetAsync(alive, 1, m, s);
      if (e != hipSuccess) return hip_status(e, "nsm_support_hits: alive flags");
    }
    const unsigned wave_blocks = support_blocks((m / 2) * kWave);
    for (rounds = 0;;) {
      rounds += 1;
      e = hipMemsetAsync(ctrl + kSupQueue, 0, 2 * sizeof(unsigned long long), s);  // the queue's length, the removed edges
      if (e != hipSuccess) return hip_status(e, "nsm_support_hits: round words");
      hipLaunchKernelGGL(support_count_kernel, dim3(support_blocks(m)), dim3(kBlock), 0, s, arcs, ctrl, off, alive, sup, queue, bits,
                         kSupportWaveMin);
      hipLaunchKernelGGL(support_count_wave_kernel, dim3(wave_blocks), dim3(kBlock), 0, s, arcs, ctrl, off, alive, sup, queue, bits);
      if (min_support == 0) break;
      hipLaunchKernelGGL(support_kill_kernel, dim3(support_blocks(m)), dim3(kBlock), 0, s, arcs, ctrl, off, alive, sup, bits,
                         min_support);
      unsigned long long round_words[3] = {0, 0, 0};  // distinct arcs, queued edges, removed edges
      e = hipMemcpyAsync(round_words, ctrl + kSupArcs, sizeof(round_words), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_status(e, "nsm_support_hits: round");
      if (round_words[2] == 0) break;
      // every round so far removed an edge, so there are at most as many as distinct edges
      if (rounds > round_words[0] / 2) {
        set_error("nsm_support_hits: %llu removing rounds for %llu distinct edges", rounds, round_words[0] / 2);
        return NSM_E_SUPPORT_ROUNDS;
      }
    }
  }
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (l.n)
      hipLaunchKernelGGL(support_write_kernel, dim3(support_blocks(l.n)), dim3(kBlock), 0, s, l.hits, l.n,
                         static_cast<uint32_t>(l.left_base), static_cast<uint32_t>(l.right_base), min_score, bits, arcs, off, alive,
                         sup, support[k]);
  }
  if (stats)
    hipLaunchKernelGGL(support_stats_kernel, dim3(support_blocks(m)), dim3(kBlock), 0, s, arcs, ctrl, alive, sup, bits, rounds, stats);
  return hip_status(hipGetLastError(), "nsm_support_hits");
}

}  // namespace nsm

extern "C" int nsm_support_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, int32_t min_support,
                                int32_t* const* support, uint64_t* stats, void* stream) {
  using namespace nsm;
  if ((!lists || !support) && n_lists > 0) {
    set_error("nsm_support_hits: null %s with n_lists > 0", !lists ? "lists" : "support");
    return NSM_E_BADARG;
  }
  if (n_lists < 0 || nodes < 0 || min_support < 0) {
    set_error("nsm_support_hits: negative count (n_lists %d, nodes %d, min_support %d)", n_lists, nodes, min_support);
    return NSM_E_BADARG;
  }
  unsigned long long records = 0;
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (!l.hits && l.n > 0) {
      set_error("nsm_support_hits: list %d has null hits with n > 0", k);
      return NSM_E_BADARG;
    }
    if (!support[k] && l.n > 0) {
      set_error("nsm_support_hits: list %d has null support with n > 0", k);
      return NSM_E_BADARG;
    }
    if (l.left_base < 0 || l.left_ids < 0 || l.right_base < 0 || l.right_ids < 0) {
      set_error("nsm_support_hits: list %d has a negative base or id count (left %d + %d, right %d + %d)", k, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
    if (static_cast<long long>(l.left_base) + l.left_ids > nodes || static_cast<long long>(l.right_base) + l.right_ids > nodes) {
      set_error("nsm_support_hits: list %d reaches beyond the %d nodes (left %d + %d, right %d + %d)", k, nodes, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
    records += l.n < (1ull << 32) ? l.n : (1ull << 32);
  }
  if (nodes == 0 || records == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capture) != hipSuccess) capture = hipStreamCaptureStatusNone;
  if (capture != hipStreamCaptureStatusNone) {
    set_error("nsm_support_hits: the stream is being captured; the call synchronises and cannot be part of a graph");
    return NSM_E_UNSUPPORTED;
  }
  if (records >= (1ull << 31)) {  // (two arcs per record are indexed with 32 bits)
    set_error("nsm_support_hits: %llu records; fewer than 2^31 are supported", records);
    return NSM_E_UNSUPPORTED;
  }
  return support_run(lists, n_lists, static_cast<uint32_t>(nodes), min_score, min_support, support,
                     reinterpret_cast<unsigned long long*>(stats), s, records);
}
