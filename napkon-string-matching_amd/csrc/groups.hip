// Match groups (include/nsm_hip_groups.h): the connected components of hit lists, labelled by their smallest node -- the
// merge of pairs that share an item which Mapping.update_mapping runs on the host (reference:
// napkon_string_matching/types/mapping.py).
//
// Lock-free union-find in the ECL-CC / Jayanti-Tarjan style on the `label` array itself; label[v] <= v throughout, a
// node with label[v] == v is a root.
//   * init     label[v] = v (not under NSM_GROUP_CONTINUE).
//   * link     one record per lane, grid-stride.  Read both ends' labels; equal labels are a common ancestor and the
//              record is done (the fate of almost every record of a list with giant components).  Else find both roots
//              with path halving; while they differ, CAS the LARGER root from itself to the smaller one.  A lost CAS
//              returns what someone else hooked that root under: go on from there.  Hooking larger under smaller makes
//              the last root the component's minimum, whatever the order.
//   * flatten  label[v] = root(v), after the last link launch.
// Why no fence is needed: a non-root never becomes a root again; halving writes only non-roots (it has read
// label[v] != v) and only an ancestor of v; hooks CAS only roots.  So any value ever stored in label[v] is v or an
// ancestor of v, a stale read is an older ancestor, and a root read stale is caught by the CAS, which is the one
// operation that needs the truth.  The words are read and written past L1 with relaxed agent-scope atomics.  Values
// strictly decrease along a path, so every find ends; no workgroup waits for another, and a CAS is retried only after
// someone else's succeeded.
#include "nsm_common.hpp"

#include "nsm_hip_groups.h"

namespace nsm {

// Workgroups of a link launch at most (grid-stride beyond).  FEW on purpose: every record in flight has read its roots
// before the others' hooks land, so the threads in flight are the CAS that are lost and the finds that are repeated --
// Term's list links in 8.9 ms from 2048 workgroups and in 0.95 ms from 128 (DESIGN.md section 4.14 has the sweep).
#ifndef NSM_GROUP_LINK_BLOCKS
#define NSM_GROUP_LINK_BLOCKS 128
#endif
constexpr unsigned kMaxLinkBlocks = NSM_GROUP_LINK_BLOCKS;
constexpr unsigned kMaxGroupBlocks = 2048;  // the streaming launches: checks, init, flatten

// control words of the call's scratch, zeroed per call: the checks' verdict; the NSM_GROUP_STATS counters
enum { kGroupBad = 0, kGroupCas = 2, kGroupLost = 4, kGroupHops = 6, kGroupWords = 8 };

__device__ __forceinline__ uint32_t label_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void label_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#ifdef NSM_GROUP_STATS
#define NSM_GROUP_COUNT(x) (x)
#else
#define NSM_GROUP_COUNT(x) ((void)0)
#endif

// The root above v, whose label `p` the caller has read.  Path halving: every other node on the way is pointed at its
// grandparent.
__device__ __forceinline__ uint32_t find_root(uint32_t* __restrict__ label, uint32_t v, uint32_t p, unsigned long long& hops) {
  for (;;) {
    if (p == v) return v;
    const uint32_t g = label_load(label + p);
    NSM_GROUP_COUNT(hops += 1);
    if (g == p) return p;
    label_store(label + v, g);
    v = g;
    p = label_load(label + v);
  }
}
__device__ __forceinline__ uint32_t find_root(uint32_t* __restrict__ label, uint32_t v, unsigned long long& hops) {
  return find_root(label, v, label_load(label + v), hops);
}

// The sum of `x` over the wave, in every lane (all 64 lanes call it).
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
  for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d, kWave);
  return x;
}

// Every i in [0, left_ids), every j in [0, right_ids): they index `label` behind the list's bases.
__global__ __launch_bounds__(kBlock) void group_check_kernel(const nsm_hit* __restrict__ hits, unsigned long long n, uint32_t nl,
                                                             uint32_t nr, uint32_t* __restrict__ ctrl) {
  bool bad = false;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long r = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += stride) {
    const nsm_hit h = hits[r];
    bad |= static_cast<uint32_t>(h.i) >= nl || static_cast<uint32_t>(h.j) >= nr;  // (a negative id is a huge unsigned)
  }
  if (bad) ctrl[kGroupBad] = 1u;
}

// NSM_GROUP_CONTINUE: label[v] in [0, v] -- a forest whose roots are its components' minima.
__global__ __launch_bounds__(kBlock) void group_forest_check_kernel(const uint32_t* __restrict__ label, uint32_t nodes,
                                                                    uint32_t* __restrict__ ctrl) {
  bool bad = false;
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) bad |= label[v] > v;
  if (bad) ctrl[kGroupBad] = 2u;
}

__global__ __launch_bounds__(kBlock) void group_init_kernel(uint32_t* __restrict__ label, uint32_t nodes) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) label[v] = v;
}

__global__ __launch_bounds__(kBlock) void group_link_kernel(const nsm_hit* __restrict__ hits, unsigned long long n,
                                                            uint32_t left_base, uint32_t right_base, double min_score,
                                                            uint32_t* __restrict__ label, unsigned long long* __restrict__ stats,
                                                            uint32_t* __restrict__ ctrl) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  unsigned long long counted = 0, hooks = 0, cas = 0, lost = 0, hops = 0;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  for (unsigned long long r = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += stride) {
    const nsm_hit h = hits[r];
    if (!(h.score >= min_score)) continue;  // (a NaN is no edge)
    counted += 1;
    const uint32_t u = left_base + static_cast<uint32_t>(h.i), v = right_base + static_cast<uint32_t>(h.j);
    if (u == v) continue;
    // Both labels in flight at once.  Equal labels are a common ancestor: the record is redundant, which is what almost
    // every record of a list with giant components is once the first hooks are made -- two independent loads, no find.
    const uint32_t pu = label_load(label + u), pv = label_load(label + v);
    if (pu == pv) continue;
    uint32_t a = find_root(label, u, pu, hops), b = find_root(label, v, pv, hops);
    while (a != b) {
      const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
      NSM_GROUP_COUNT(cas += 1);
      const uint32_t seen = atomicCAS(label + hi, hi, lo);
      if (seen == hi) {
        hooks += 1;
        break;
      }
      // someone else hooked `hi` under `seen` first: both ends go on from what is known now
      NSM_GROUP_COUNT(lost += 1);
      a = find_root(label, seen, hops);
      b = find_root(label, lo, hops);
    }
  }
  // one atomic per wave and counter, none without `stats` (the lanes meet again here: whole waves were launched)
  if (stats) {
    counted = wave_sum(counted);
    hooks = wave_sum(hooks);
    if (lane == 0) {
      if (counted) atomicAdd(stats + 0, counted);
      if (hooks) atomicAdd(stats + 1, hooks);
    }
  }
#ifdef NSM_GROUP_STATS
  cas = wave_sum(cas);
  lost = wave_sum(lost);
  hops = wave_sum(hops);
  if (lane == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(ctrl + kGroupCas), cas);
    atomicAdd(reinterpret_cast<unsigned long long*>(ctrl + kGroupLost), lost);
    atomicAdd(reinterpret_cast<unsigned long long*>(ctrl + kGroupHops), hops);
  }
#else
  (void)cas, (void)lost, (void)hops, (void)ctrl;
#endif
}

// No hook runs any more: the roots are final, and a word another lane flattens meanwhile reads as an ancestor either way.
__global__ __launch_bounds__(kBlock) void group_flatten_kernel(uint32_t* __restrict__ label, uint32_t nodes) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) {
    uint32_t root = label_load(label + v);
    if (root == v) continue;
    for (uint32_t p = label_load(label + root); p != root; p = label_load(label + root)) root = p;
    label_store(label + v, root);
  }
}

static unsigned group_blocks(unsigned long long n, unsigned most = kMaxGroupBlocks) {
  const unsigned long long b = (n + kBlock - 1) / kBlock;
  return b < most ? static_cast<unsigned>(b ? b : 1u) : most;
}

#ifdef NSM_GROUP_STATS
static unsigned long long g_group_counters[3];  // CAS attempts, lost CAS, find hops
#endif

static int group_run(const nsm_hit_list* lists, int32_t n_lists, uint32_t nodes, double min_score, bool keep, uint32_t* label,
                     unsigned long long* stats, hipStream_t s, uint32_t* ctrl) {
  unsigned long long records = 0;
  for (int32_t k = 0; k < n_lists; ++k) records += lists[k].n;
  hipError_t e = hipMemsetAsync(ctrl, 0, kGroupWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_group_hits: control words");
  if (records || keep) {
    for (int32_t k = 0; k < n_lists; ++k) {
      const nsm_hit_list& l = lists[k];
      if (l.n)
        hipLaunchKernelGGL(group_check_kernel, dim3(group_blocks(l.n)), dim3(kBlock), 0, s, l.hits, l.n,
                           static_cast<uint32_t>(l.left_ids), static_cast<uint32_t>(l.right_ids), ctrl);
    }
    if (keep) hipLaunchKernelGGL(group_forest_check_kernel, dim3(group_blocks(nodes)), dim3(kBlock), 0, s, label, nodes, ctrl);
    uint32_t bad = 0;
    e = hipMemcpyAsync(&bad, ctrl + kGroupBad, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "nsm_group_hits: checks");
    if (bad) {
      // (the forest check runs last: its verdict is the one left standing when both fail)
      if (bad == 2u)
        set_error("nsm_group_hits: NSM_GROUP_CONTINUE with a label[v] outside [0, v]");
      else
        set_error("nsm_group_hits: a record's id is outside its list's [0, left_ids) x [0, right_ids)");
      return NSM_E_BADARG;
    }
  }
  if (!keep) hipLaunchKernelGGL(group_init_kernel, dim3(group_blocks(nodes)), dim3(kBlock), 0, s, label, nodes);
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (l.n)
      hipLaunchKernelGGL(group_link_kernel, dim3(group_blocks(l.n, kMaxLinkBlocks)), dim3(kBlock), 0, s, l.hits, l.n,
                         static_cast<uint32_t>(l.left_base), static_cast<uint32_t>(l.right_base), min_score, label, stats, ctrl);
  }
  if (records || keep) hipLaunchKernelGGL(group_flatten_kernel, dim3(group_blocks(nodes)), dim3(kBlock), 0, s, label, nodes);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e, "nsm_group_hits");
#ifdef NSM_GROUP_STATS
  unsigned long long counted[3] = {0, 0, 0};
  e = hipMemcpyAsync(counted, ctrl + kGroupCas, sizeof(counted), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_status(e, "nsm_group_hits: counters");
  for (int c = 0; c < 3; ++c) g_group_counters[c] += counted[c];
#endif
  return 0;
}

}  // namespace nsm

#ifdef NSM_GROUP_STATS
// Variant build only: CAS attempts, lost CAS and find hops, summed over the calls so far.
extern "C" void nsm_group_counters(unsigned long long out[3]) {
  for (int c = 0; c < 3; ++c) out[c] = nsm::g_group_counters[c];
}
#endif

extern "C" int nsm_group_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, uint32_t flags,
                              int32_t* label, uint64_t* stats, void* stream) {
  using namespace nsm;
  if (!lists && n_lists > 0) {
    set_error("nsm_group_hits: null lists with n_lists > 0");
    return NSM_E_BADARG;
  }
  if (n_lists < 0 || nodes < 0) {
    set_error("nsm_group_hits: negative count (n_lists %d, nodes %d)", n_lists, nodes);
    return NSM_E_BADARG;
  }
  if (!label && nodes > 0) {
    set_error("nsm_group_hits: null label with nodes > 0");
    return NSM_E_BADARG;
  }
  if (flags & ~NSM_GROUP_CONTINUE) {
    set_error("nsm_group_hits: unknown flag bits 0x%x", flags & ~NSM_GROUP_CONTINUE);
    return NSM_E_BADARG;
  }
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (!l.hits && l.n > 0) {
      set_error("nsm_group_hits: list %d has null hits with n > 0", k);
      return NSM_E_BADARG;
    }
    if (l.left_base < 0 || l.left_ids < 0 || l.right_base < 0 || l.right_ids < 0) {
      set_error("nsm_group_hits: list %d has a negative base or id count (left %d + %d, right %d + %d)", k, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
    if (static_cast<long long>(l.left_base) + l.left_ids > nodes || static_cast<long long>(l.right_base) + l.right_ids > nodes) {
      set_error("nsm_group_hits: list %d reaches beyond the %d nodes (left %d + %d, right %d + %d)", k, nodes, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
  }
  if (nodes == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capture) != hipSuccess) capture = hipStreamCaptureStatusNone;
  if (capture != hipStreamCaptureStatusNone) {
    set_error("nsm_group_hits: the stream is being captured; the call synchronises and cannot be part of a graph");
    return NSM_E_UNSUPPORTED;
  }
  void* scratch = nullptr;
  hipError_t e = hipMallocAsync(&scratch, kGroupWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_group_hits: stream-ordered scratch");
  const int status = group_run(lists, n_lists, static_cast<uint32_t>(nodes), min_score, (flags & NSM_GROUP_CONTINUE) != 0,
                               reinterpret_cast<uint32_t*>(label), reinterpret_cast<unsigned long long*>(stats), s,
                               static_cast<uint32_t*>(scratch));
  (void)hipFreeAsync(scratch, s);
  return status;
}
