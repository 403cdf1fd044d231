// Merge forests (include/nsm_hip_span.h): the maximum spanning forest of hit lists under the canonical record order -- the
// single-linkage hierarchy of the merge Mapping.update_mapping runs on the host (reference:
// napkon_string_matching/types/mapping.py).  Cut at any threshold it gives nsm_group_hits's labels at that threshold.
//
// Boruvka over ranks.
//   * gather   one pass over the lists: the id check, the count of records >= min_score, and the edges (score, lo, hi)
//              appended to scratch.
//   * order    nsm_sort_hits on that scratch with id_limit = nodes.  An edge's rank is its position afterwards, so the
//              tie-break is a 32-bit integer and a component's best edge is one atomicMin on a 32-bit word.  Equal
//              values (duplicates) get different ranks: the order on ranks is STRICT.
//   * rounds   ordered by kernel boundaries; no kernel waits for another workgroup.
//       propose  every edge whose ends have different roots mins its rank into both roots' `best` words.
//       hook     a root c with best rank r, whose other end's root is o, sets parent[c] = o and appends record r -- unless
//                best[o] is r too and c < o: then c stays a root (and o hooks under it).
//       flatten  root[v] = the end of the parent chain above root[v]; best[v] is reset.
//     The host reads the hook count after each round and stops when a round hooks nothing, or when nodes - 1 hooks have
//     left one component.  Every component with an edge to another one hooks or is hooked under in a round, so their
//     number at least halves: at most floor(log2(nodes)) hooking rounds, plus the one that finds nothing.
//     Every round visits every edge.  Dropping the edges inside one component from a live list between the rounds was
//     built and measured, and did not pay: Boruvka's early rounds merge pairs, so a dense list
//     keeps nearly all its edges until the last rounds -- Term's 10.5 M records took 11.6 ms with the pass after every
//     round and 6.1 ms without, and no list gained from a pass run only once half the edges had died.  So
//     NSM_SPAN_NO_COMPACT names the only route there is.
//   * labels   atomicMin of v into its root's word, then label[v] = that word.
// Three words per node: root[v] (the root of v's component as of the round's start: read-only in propose and hook),
// parent[c] (meaningful for roots: itself, or what this round's hook put it under) and best[c].
//
// Why the hooks of a round make no cycle.  Let pick(c) = the rank root c hooks along.  It is the minimum rank over ALL
// edges leaving c's component, and the edge also leaves o's component, so pick(o) <= pick(c).  Along any chain
// c -> o -> o' -> ... the picks never increase, so a cycle has ONE pick all the way round; one edge has two ends, so the
// cycle is a mutual pair c <-> o with pick(c) == pick(o), and in such a pair the smaller root does not hook.  The
// strict order on ranks is what this needs (with a partial order, three components could pick three different edges of
// equal score round a triangle).  Hence every parent chain ends in a root after fewer than `nodes` steps, and the
// appended records join two different components each: a forest.  The flatten loop is nevertheless BOUNDED by `nodes`
// steps and raises the control word when it runs out: a logic error becomes an error code, never a spinning kernel.
// Why the result is the definition: with a strict order the maximum spanning forest is unique, and the minimum-rank
// edge leaving a component belongs to it (the cut property); of equal values the smallest rank is taken and the others
// then join one component.
//
// The shared words are read and written past L1 with relaxed agent-scope atomics, as groups.hip and assign.hip do.  Within
// a launch: propose only mins `best` (monotone: a stale read is too large and costs a redundant atomic at worst); hook
// reads `best` and `root`, which no hook writes, and each root writes its own parent word only; flatten's thread v
// writes root[v] and best[v], which no other thread of that launch reads, and the parent words it compresses hold an
// ancestor before and after.
#include "nsm_common.hpp"

#include "nsm_hip_span.h"

namespace nsm {

// Workgroups of a propose launch at most (grid-stride beyond).  groups.hip found the threads in flight to be the cost of
// contended words; propose's atomicMin is skipped whenever the word already holds a smaller rank, so it tolerates more
// (DESIGN.md section 4.15).
#ifndef NSM_SPAN_PROPOSE_BLOCKS
#define NSM_SPAN_PROPOSE_BLOCKS 1024
#endif
constexpr unsigned kMaxProposeBlocks = NSM_SPAN_PROPOSE_BLOCKS;
constexpr unsigned kMaxSpanBlocks = 2048;  // the streaming launches
constexpr uint32_t kNoRank = 0xffffffffu;

// control words of the call's scratch (64 bytes, zeroed per call).  The 64-bit ones sit at even indices.
// The hooks are a running total over the rounds.
enum { kSpanEdges = 0, kSpanCounted = 2, kSpanBad = 4, kSpanHooks = 5, kSpanWords = 16 };

__device__ __forceinline__ uint32_t span_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void span_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One list: ids checked (ALL records), records >= min_score counted, edges appended as (score, lo, hi).  `edges` has room
// for every record of every list, so the append cannot overflow.
__global__ __launch_bounds__(kBlock) void span_gather_kernel(const nsm_hit* __restrict__ hits, unsigned long long n, uint32_t nl,
                                                             uint32_t nr, uint32_t left_base, uint32_t right_base,
                                                             double min_score, nsm_hit* __restrict__ edges,
                                                             unsigned long long cap, uint32_t* __restrict__ ctrl) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  bool bad = false;
  unsigned long long counted = 0;
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * kBlock;
  // (whole waves run every trip: the append is wave-wide)
  for (unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kBlock; base < n; base += stride) {
    const unsigned long long r = base + threadIdx.x;
    bool edge = false;
    nsm_hit h = {0.0, 0, 0};
    uint32_t lo = 0, hi = 0;
    if (r < n) {
      h = hits[r];
      const bool out = static_cast<uint32_t>(h.i) >= nl || static_cast<uint32_t>(h.j) >= nr;  // (a negative id is a huge unsigned)
      bad |= out;
      if (!out && h.score >= min_score) {  // (a NaN is no edge)
        counted += 1;
        const uint32_t u = left_base + static_cast<uint32_t>(h.i), v = right_base + static_cast<uint32_t>(h.j);
        lo = u < v ? u : v;
        hi = u < v ? v : u;
        edge = u != v;
      }
    }
    emit_hits_wave(edges, cap, reinterpret_cast<unsigned long long*>(ctrl + kSpanEdges), edge, h.score, static_cast<int>(lo),
                   static_cast<int>(hi));
  }
  if (bad) ctrl[kSpanBad] = 1u;
  for (int d = kWave / 2; d > 0; d >>= 1) counted += __shfl_xor(counted, d, kWave);
  if (lane == 0 && counted) atomicAdd(reinterpret_cast<unsigned long long*>(ctrl + kSpanCounted), counted);
}

__global__ __launch_bounds__(kBlock) void span_init_kernel(uint32_t* __restrict__ root, uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ best, uint32_t nodes) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) {
    root[v] = v;
    parent[v] = v;
    best[v] = kNoRank;
  }
}

__global__ __launch_bounds__(kBlock) void span_propose_kernel(const nsm_hit* __restrict__ edges, uint32_t n_edges,
                                                              const uint32_t* __restrict__ root, uint32_t* __restrict__ best) {
  for (uint32_t r = blockIdx.x * kBlock + threadIdx.x; r < n_edges; r += gridDim.x * kBlock) {
    const nsm_hit h = edges[r];
    const uint32_t a = root[static_cast<uint32_t>(h.i)], b = root[static_cast<uint32_t>(h.j)];
    if (a == b) continue;
    // The min is monotone within this launch, so a value read past L1 is only ever too large: a rank that is not smaller
    // than what it reads cannot become the minimum and skips the atomic.
    if (r < span_load(best + a)) atomicMin(best + a, r);
    if (r < span_load(best + b)) atomicMin(best + b, r);
  }
}

__global__ __launch_bounds__(kBlock) void span_hook_kernel(const nsm_hit* __restrict__ edges, const uint32_t* __restrict__ root,
                                                           uint32_t* __restrict__ parent, const uint32_t* __restrict__ best,
                                                           uint32_t nodes, nsm_hit* __restrict__ forest, unsigned long long cap,
                                                           unsigned long long* __restrict__ forest_count,
                                                           uint32_t* __restrict__ ctrl) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  uint32_t hooks = 0;
  // (whole waves run every trip: the append is wave-wide)
  for (uint32_t base = blockIdx.x * kBlock; base < nodes; base += gridDim.x * kBlock) {
    const uint32_t c = base + threadIdx.x;
    bool hook = false;
    nsm_hit h = {0.0, 0, 0};
    if (c < nodes && root[c] == c) {
      const uint32_t r = span_load(best + c);
      if (r != kNoRank) {
        h = edges[r];
        const uint32_t a = root[static_cast<uint32_t>(h.i)], b = root[static_cast<uint32_t>(h.j)];
        const uint32_t o = a == c ? b : a;
        hook = !(span_load(best + o) == r && c < o);
        if (hook) span_store(parent + c, o);
      }
    }
    hooks += hook ? 1u : 0u;
    emit_hits_wave(forest, cap, forest_count, hook, h.score, h.i, h.j);
  }
  for (int d = kWave / 2; d > 0; d >>= 1) hooks += __shfl_xor(hooks, d, kWave);
  if (lane == 0 && hooks) atomicAdd(ctrl + kSpanHooks, hooks);
}

// root[v] = the root above it.  Only words of nodes that were roots when the round began are followed: theirs are the
// parent words the hooks wrote.  The loop is bounded (see the file's header): a chain longer than `nodes` is a cycle.
__global__ __launch_bounds__(kBlock) void span_flatten_kernel(uint32_t* __restrict__ root, uint32_t* __restrict__ parent,
                                                              uint32_t* __restrict__ best, uint32_t nodes,
                                                              uint32_t* __restrict__ ctrl) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) {
    const uint32_t start = root[v];
    uint32_t c = start, p = span_load(parent + c), steps = 0;
    while (p != c && steps < nodes) {
      c = p;
      p = span_load(parent + c);
      steps += 1;
    }
    if (p != c) {
      ctrl[kSpanBad] = 2u;
      continue;
    }
    if (steps > 1) span_store(parent + start, c);  // (an ancestor before and after: later chains through `start` are short)
    root[v] = c;
    best[v] = kNoRank;
  }
}

// `best` is kNoRank everywhere (init, or the last flatten): it becomes the smallest node per root.
__global__ __launch_bounds__(kBlock) void span_label_min_kernel(const uint32_t* __restrict__ root, uint32_t* __restrict__ best,
                                                                uint32_t nodes) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) {
    uint32_t* w = best + root[v];
    if (v < span_load(w)) atomicMin(w, v);
  }
}

__global__ __launch_bounds__(kBlock) void span_label_write_kernel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ best,
                                                                  uint32_t nodes, uint32_t* __restrict__ label) {
  for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nodes; v += gridDim.x * kBlock) label[v] = best[root[v]];
}

__global__ void span_stats_kernel(const uint32_t* __restrict__ ctrl, unsigned long long* __restrict__ stats, unsigned long long rounds,
                                  unsigned long long visits) {
  stats[0] += *reinterpret_cast<const unsigned long long*>(ctrl + kSpanCounted);
  stats[1] += ctrl[kSpanHooks];
  stats[2] += rounds;
  stats[3] += visits;
}

static unsigned span_blocks(unsigned long long n, unsigned most = kMaxSpanBlocks) {
  const unsigned long long b = (n + kBlock - 1) / kBlock;
  return b < most ? static_cast<unsigned>(b ? b : 1u) : most;
}

struct SpanScratch {
  uint32_t* ctrl;
  nsm_hit* edges;
  nsm_hit* sort_scratch;  // nullptr when at most 8192 records can be live
  uint32_t *root, *parent, *best;
};

static int span_run(const nsm_hit_list* lists, int32_t n_lists, unsigned long long records, uint32_t nodes, double min_score,
                    nsm_hit* forest, unsigned long long* forest_count, uint32_t* label, unsigned long long* stats,
                    hipStream_t s, const SpanScratch& m) {
  hipError_t e = hipMemsetAsync(m.ctrl, 0, kSpanWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_span_hits: control words");
  uint32_t edges = 0;
  if (records) {
    for (int32_t k = 0; k < n_lists; ++k) {
      const nsm_hit_list& l = lists[k];
      if (l.n)
        hipLaunchKernelGGL(span_gather_kernel, dim3(span_blocks(l.n)), dim3(kBlock), 0, s, l.hits, l.n,
                           static_cast<uint32_t>(l.left_ids), static_cast<uint32_t>(l.right_ids), static_cast<uint32_t>(l.left_base),
                           static_cast<uint32_t>(l.right_base), min_score, m.edges, records, m.ctrl);
    }
    uint32_t head[kSpanHooks + 1];
    e = hipMemcpyAsync(head, m.ctrl, sizeof(head), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "nsm_span_hits: gather");
    if (head[kSpanBad]) {
      set_error("nsm_span_hits: a record's id is outside its list's [0, left_ids) x [0, right_ids)");
      return NSM_E_BADARG;
    }
    edges = head[kSpanEdges];  // (below 2^31: the records are)
  }
  if (edges > 1) {
    const int status = nsm_sort_hits(m.edges, m.sort_scratch, records, reinterpret_cast<const unsigned long long*>(m.ctrl + kSpanEdges),
                                     edges, nodes, s);
    if (status != 0) return status;
  }
  hipLaunchKernelGGL(span_init_kernel, dim3(span_blocks(nodes)), dim3(kBlock), 0, s, m.root, m.parent, m.best, nodes);

  const unsigned long long cap = nodes - 1;
  const unsigned node_blocks = span_blocks(nodes);
  unsigned long long rounds = 0, visits = 0;
  uint32_t hooked = 0;
  unsigned max_rounds = 2;  // ceil(log2(max(nodes, 2))) + 1
  while ((1ull << (max_rounds - 1)) < nodes) ++max_rounds;
  while (edges > 0) {
    if (rounds >= max_rounds) {
      set_error("nsm_span_hits: %llu rounds and still hooking (at most %u rounds for %u nodes)", rounds, max_rounds, nodes);
      return static_cast<int>(hipErrorUnknown);
    }
    hipLaunchKernelGGL(span_propose_kernel, dim3(span_blocks(edges, kMaxProposeBlocks)), dim3(kBlock), 0, s, m.edges, edges, m.root,
                       m.best);
    hipLaunchKernelGGL(span_hook_kernel, dim3(node_blocks), dim3(kBlock), 0, s, m.edges, m.root, m.parent, m.best, nodes, forest,
                       cap, forest_count, m.ctrl);
    hipLaunchKernelGGL(span_flatten_kernel, dim3(node_blocks), dim3(kBlock), 0, s, m.root, m.parent, m.best, nodes, m.ctrl);
    uint32_t tail[2];  // bad, hooks
    e = hipMemcpyAsync(tail, m.ctrl + kSpanBad, sizeof(tail), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "nsm_span_hits: round");
    rounds += 1;
    visits += edges;
    if (tail[0]) {
      set_error("nsm_span_hits: round %llu left a parent chain of more than %u steps", rounds, nodes);
      return static_cast<int>(hipErrorUnknown);
    }
    const uint32_t hooks_now = tail[1] - hooked;
    hooked = tail[1];
    if (hooks_now == 0 || hooked == nodes - 1) break;  // (one component: nothing is left to hook)
  }
  if (label) {
    hipLaunchKernelGGL(span_label_min_kernel, dim3(node_blocks), dim3(kBlock), 0, s, m.root, m.best, nodes);
    hipLaunchKernelGGL(span_label_write_kernel, dim3(node_blocks), dim3(kBlock), 0, s, m.root, m.best, nodes, label);
  }
  if (stats) hipLaunchKernelGGL(span_stats_kernel, dim3(1), dim3(1), 0, s, m.ctrl, stats, rounds, visits);
  return hip_status(hipGetLastError(), "nsm_span_hits");
}

}  // namespace nsm

extern "C" int nsm_span_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, uint32_t flags,
                             nsm_hit* forest, unsigned long long* forest_count, int32_t* label, uint64_t* stats, void* stream) {
  using namespace nsm;
  if (!lists && n_lists > 0) {
    set_error("nsm_span_hits: null lists with n_lists > 0");
    return NSM_E_BADARG;
  }
  if (n_lists < 0 || nodes < 0) {
    set_error("nsm_span_hits: negative count (n_lists %d, nodes %d)", n_lists, nodes);
    return NSM_E_BADARG;
  }
  if (!forest && nodes > 1) {
    set_error("nsm_span_hits: null forest with nodes > 1");
    return NSM_E_BADARG;
  }
  if (!forest_count) {
    set_error("nsm_span_hits: null forest_count");
    return NSM_E_BADARG;
  }
  if (flags & ~NSM_SPAN_NO_COMPACT) {
    set_error("nsm_span_hits: unknown flag bits 0x%x", flags & ~NSM_SPAN_NO_COMPACT);
    return NSM_E_BADARG;
  }
  unsigned long long records = 0;
  for (int32_t k = 0; k < n_lists; ++k) {
    const nsm_hit_list& l = lists[k];
    if (!l.hits && l.n > 0) {
      set_error("nsm_span_hits: list %d has null hits with n > 0", k);
      return NSM_E_BADARG;
    }
    if (l.left_base < 0 || l.left_ids < 0 || l.right_base < 0 || l.right_ids < 0) {
      set_error("nsm_span_hits: list %d has a negative base or id count (left %d + %d, right %d + %d)", k, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
    if (static_cast<long long>(l.left_base) + l.left_ids > nodes || static_cast<long long>(l.right_base) + l.right_ids > nodes) {
      set_error("nsm_span_hits: list %d reaches beyond the %d nodes (left %d + %d, right %d + %d)", k, nodes, l.left_base,
                l.left_ids, l.right_base, l.right_ids);
      return NSM_E_BADARG;
    }
  }
  for (int32_t k = 0; k < n_lists; ++k) {
    const unsigned long long n = lists[k].n;
    if (n >= (1ull << 31) || (records += n) >= (1ull << 31)) {
      set_error("nsm_span_hits: 2^31 or more records in all lists together, ranks are 32-bit");
      return NSM_E_UNSUPPORTED;
    }
  }
  if (nodes == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capture) != hipSuccess) capture = hipStreamCaptureStatusNone;
  if (capture != hipStreamCaptureStatusNone) {
    set_error("nsm_span_hits: the stream is being captured; the call synchronises and cannot be part of a graph");
    return NSM_E_UNSUPPORTED;
  }
  const uint32_t n32 = static_cast<uint32_t>(nodes);
  // one allocation: control words | edges | sort scratch | root, parent, best   (16-byte records first)
  const size_t edge_records = static_cast<size_t>(records);
  const size_t sort_records = records > 8192 ? edge_records : 0;
  const size_t node_words = 3 * static_cast<size_t>(n32);
  const size_t bytes = kSpanWords * sizeof(uint32_t) + (edge_records + sort_records) * sizeof(nsm_hit) +
                       node_words * sizeof(uint32_t);
  void* scratch = nullptr;
  hipError_t e = hipMallocAsync(&scratch, bytes, s);
  if (e != hipSuccess) return hip_status(e, "nsm_span_hits: stream-ordered scratch");
  SpanScratch m;
  m.ctrl = static_cast<uint32_t*>(scratch);
  m.edges = reinterpret_cast<nsm_hit*>(m.ctrl + kSpanWords);
  m.sort_scratch = sort_records ? m.edges + edge_records : nullptr;
  m.root = reinterpret_cast<uint32_t*>(m.edges + edge_records + sort_records);
  m.parent = m.root + n32;
  m.best = m.parent + n32;
  const int status = span_run(lists, n_lists, records, n32, min_score, forest, forest_count,
                              reinterpret_cast<uint32_t*>(label), reinterpret_cast<unsigned long long*>(stats), s, m);
  (void)hipFreeAsync(scratch, s);
  // the rounds were driven from the host; the labels and the stats are the caller's to read after the return
  e = hipStreamSynchronize(s);
  if (status != 0) return status;
  return hip_status(e, "nsm_span_hits");
}
