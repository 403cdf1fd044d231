// One-to-one assignment of a canonically ordered hit list (include/nsm_hip_assign.h): the greedy walk "take a record iff
// both its items are free" that a consumer of Comparable.sort_by_score's frame (reference:
// napkon_string_matching/types/comparable.py:69-70) runs on the host to turn matches into a mapping.
//
// One 32-bit word per item (left ids first, right ids behind them): kFree, 0 = taken, or rank + 1 of the smallest live
// record that proposed to the item in the current round.  Two stages share one invariant -- the matched records are a
// subset of the walk's answer and the live records are exactly those with both items free:
//   * rounds (whole GPU, three launches each, ordered by kernel boundaries; no kernel waits for another workgroup):
//     propose = every live record mins its rank into both its items' words; match = a record that holds both words is the
//     smallest live record of both its items, so the walk takes it: append it, mark both items; prune = records with a
//     taken item die, survivors reset their items' words and are appended to the next live list.  The host reads the
//     live count after every round.  Distinct scores die out geometrically; ties do not (an all-ties complete list
//     makes ONE match per round), hence
//   * stream (one workgroup): walks the live records in rank order, a batch of 1024 at a time.  All 16 waves gather both
//     items' taken state and ballot the candidates (both items free) into LDS in rank order; wave 0 resolves them 64 at
//     a time: lowest live lane wins, its (i, j) is broadcast with v_readlane, every lane that shares an item is cleared.
//     One loop iteration per match, one batch latency per batch; a dead record costs its gather and nothing else.
//     The taken state stays in the global words and is read and written with relaxed agent-scope atomics (the L2 is the
//     point of coherence; L1 is bypassed), so one path serves any number of ids.
#include "nsm_common.hpp"

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "nsm_hip_assign.h"

// Routing of the default route, DESIGN.md section 4.13: a list of at most NSM_ASSIGN_STREAM_BELOW live records goes to
// the stream stage; rounds go on while a round leaves at most NUM/DEN of its live records, at most MAX_ROUNDS of them.
#ifndef NSM_ASSIGN_STREAM_BELOW
#define NSM_ASSIGN_STREAM_BELOW 1024
#endif
#ifndef NSM_ASSIGN_MAX_ROUNDS
#define NSM_ASSIGN_MAX_ROUNDS 8
#endif
#ifndef NSM_ASSIGN_PAY_NUM
#define NSM_ASSIGN_PAY_NUM 1
#endif
#ifndef NSM_ASSIGN_PAY_DEN
#define NSM_ASSIGN_PAY_DEN 2
#endif

namespace nsm {

constexpr uint32_t kFree = 0xffffffffu;  // no proposal yet; 0 = taken; else rank + 1
constexpr int kStreamThreads = 1024;     // one batch: one record per lane, 16 waves
constexpr int kStreamWaves = kStreamThreads / kWave;
constexpr unsigned kMaxRoundBlocks = 4096;

// control words at the start of the scratch: 64 bytes, zeroed per call
enum { kCtrlBad = 0, kCtrlLiveA = 1, kCtrlLiveB = 2, kCtrlAtomics = 3, kCtrlProposals = 4, kCtrlWords = 16 };

__device__ __forceinline__ uint32_t word_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void word_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int lane_rank(unsigned long long mask) {
  return static_cast<int>(
      __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u)));
}

// Every id must index the words: i in [0, nl), j in [0, nr).
__global__ __launch_bounds__(kBlock) void assign_check_kernel(const nsm_hit* __restrict__ hits, uint32_t n, uint32_t nl,
                                                              uint32_t nr, uint32_t* __restrict__ ctrl) {
  bool bad = false;
  for (uint32_t r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
    const nsm_hit h = hits[r];
    bad |= static_cast<uint32_t>(h.i) >= nl || static_cast<uint32_t>(h.j) >= nr;  // (a negative id is a huge unsigned)
  }
  if (bad) ctrl[kCtrlBad] = 1u;
}

// live == nullptr: the live list is the whole list, rank = position.
__device__ __forceinline__ uint32_t live_rank(const uint32_t* __restrict__ live, uint32_t idx) { return live ? live[idx] : idx; }

__global__ __launch_bounds__(kBlock) void assign_propose_kernel(const nsm_hit* __restrict__ hits,
                                                                const uint32_t* __restrict__ live, uint32_t n_live,
                                                                uint32_t* __restrict__ words, uint32_t nl,
                                                                uint32_t* __restrict__ ctrl) {
  for (uint32_t idx = blockIdx.x * kBlock + threadIdx.x; idx < n_live; idx += gridDim.x * kBlock) {
    const uint32_t r = live_rank(live, idx);
    const nsm_hit h = hits[r];
    uint32_t* wl = words + static_cast<uint32_t>(h.i);
    uint32_t* wr = words + nl + static_cast<uint32_t>(h.j);
    // The min is monotone within this launch, so a value read past L1 is only ever too large: a record whose rank is
    // not smaller than what it reads cannot become the minimum and skips the atomic.
    const bool pl = r + 1u < word_load(wl);
    const bool pr = r + 1u < word_load(wr);
    if (pl) atomicMin(wl, r + 1u);
    if (pr) atomicMin(wr, r + 1u);
#ifdef NSM_ASSIGN_STATS
    atomicAdd(ctrl + kCtrlAtomics, static_cast<uint32_t>(pl) + static_cast<uint32_t>(pr));
    atomicAdd(ctrl + kCtrlProposals, 1u);
#endif
  }
}

__global__ __launch_bounds__(kBlock) void assign_match_kernel(const nsm_hit* __restrict__ hits,
                                                              const uint32_t* __restrict__ live, uint32_t n_live,
                                                              uint32_t* __restrict__ words, uint32_t nl,
                                                              nsm_hit* __restrict__ out, unsigned long long cap,
                                                              unsigned long long* __restrict__ out_count) {
  // (whole waves run every trip: the append below is wave-wide)
  for (uint32_t base = blockIdx.x * kBlock; base < n_live; base += gridDim.x * kBlock) {
    const uint32_t idx = base + threadIdx.x;
    bool won = false;
    nsm_hit h = {0.0, 0, 0};
    if (idx < n_live) {
      const uint32_t r = live_rank(live, idx);
      h = hits[r];
      uint32_t* wl = words + static_cast<uint32_t>(h.i);
      uint32_t* wr = words + nl + static_cast<uint32_t>(h.j);
      // (only this record writes a word it holds; a word another winner marks meanwhile is not this record's either way)
      const uint32_t vl = word_load(wl), vr = word_load(wr);
      won = (vl == r + 1u) & (vr == r + 1u);
      if (won) {
        word_store(wl, 0u);
        word_store(wr, 0u);
      }
    }
    emit_hits_wave(out, cap, out_count, won, h.score, h.i, h.j);
  }
}

__global__ __launch_bounds__(kBlock) void assign_prune_kernel(const nsm_hit* __restrict__ hits,
                                                              const uint32_t* __restrict__ live, uint32_t n_live,
                                                              uint32_t* __restrict__ words, uint32_t nl,
                                                              uint32_t* __restrict__ next, uint32_t* __restrict__ next_count) {
  const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
  for (uint32_t base = blockIdx.x * kBlock; base < n_live; base += gridDim.x * kBlock) {
    const uint32_t idx = base + threadIdx.x;
    bool keep = false;
    uint32_t r = 0;
    if (idx < n_live) {
      r = live_rank(live, idx);
      const nsm_hit h = hits[r];
      uint32_t* wl = words + static_cast<uint32_t>(h.i);
      uint32_t* wr = words + nl + static_cast<uint32_t>(h.j);
      // (a word is 0 since the match launch, or a proposal, or kFree from another survivor of this launch: the test
      // reads the same answer from all three)
      const uint32_t vl = word_load(wl), vr = word_load(wr);
      keep = (vl != 0u) & (vr != 0u);
      if (keep) {
        word_store(wl, kFree);
        word_store(wr, kFree);
      }
    }
    const unsigned long long who = __ballot(keep);
    if (who == 0ull) continue;
    const int leader = __builtin_ctzll(who);
    uint32_t pos = 0;
    if (lane == leader) pos = atomicAdd(next_count, static_cast<uint32_t>(__popcll(who)));
    pos = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(pos), leader));
    if (keep) next[pos + lane_rank(who)] = r;
  }
}

// Stage 2.  `live` (nullptr: the whole list) is in rank order.  Also the call's bookkeeping: *out_count and stats.
__global__ __launch_bounds__(kStreamThreads) void assign_stream_kernel(
    const nsm_hit* __restrict__ hits, const uint32_t* __restrict__ live, uint32_t n_live, uint32_t* __restrict__ words,
    uint32_t nl, nsm_hit* __restrict__ out, unsigned long long cap, unsigned long long* __restrict__ out_count,
    unsigned long long* __restrict__ stats, uint32_t rounds) {
  __shared__ nsm_hit s_rec[kStreamThreads];
  __shared__ int s_wcnt[kStreamWaves];
  const int t = static_cast<int>(threadIdx.x), lane = t & (kWave - 1), wave = t / kWave;
  const unsigned long long c0 = *out_count;  // what the rounds matched
  unsigned long long made = 0;               // wave 0's, wave-uniform
  nsm_hit next = {0.0, -1, -1};
  bool next_valid = static_cast<uint32_t>(t) < n_live;
  if (next_valid) next = hits[live_rank(live, static_cast<uint32_t>(t))];
  for (uint32_t base = 0; base < n_live; base += kStreamThreads) {
    const nsm_hit h = next;
    bool cand = false;
    if (next_valid) {  // (both loads in flight at once)
      const uint32_t wl = word_load(words + static_cast<uint32_t>(h.i)), wr = word_load(words + nl + static_cast<uint32_t>(h.j));
      cand = (wl != 0u) & (wr != 0u);
    }
    const unsigned long long who = __ballot(cand);
    if (lane == 0) s_wcnt[wave] = __popcll(who);
    __syncthreads();
    int off = 0, total = 0;
    for (int w = 0; w < kStreamWaves; ++w) {
      const int c = s_wcnt[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (cand) s_rec[off + lane_rank(who)] = h;
    // the next batch's records do not depend on this batch's winners; only the gather above does
    const uint32_t ahead = base + kStreamThreads + static_cast<uint32_t>(t);
    next_valid = ahead < n_live;
    if (next_valid) next = hits[live_rank(live, ahead)];
    __syncthreads();
    if (wave == 0) {
      bool stale = false;  // a winner of this batch may have taken an item of a later chunk's candidate
      for (int c = 0; c < total; c += kWave) {
        bool alive_lane = c + lane < total;
        nsm_hit r = {0.0, -1, -1};
        if (alive_lane) r = s_rec[c + lane];
        if (stale && alive_lane) {
          const uint32_t wl = word_load(words + static_cast<uint32_t>(r.i)), wr = word_load(words + nl + static_cast<uint32_t>(r.j));
          alive_lane = (wl != 0u) & (wr != 0u);
        }
        unsigned long long alive = __ballot(alive_lane);
        unsigned long long win = 0ull;
        while (alive != 0ull) {
          const int l = __builtin_ctzll(alive);
          const int i0 = __builtin_amdgcn_readlane(r.i, l);
          const int j0 = __builtin_amdgcn_readlane(r.j, l);
          win |= 1ull << l;
          alive &= ~__ballot(r.i == i0 || r.j == j0);  // (lane l itself among them)
        }
        if (win != 0ull) {
          if ((win >> lane) & 1ull) {
            word_store(words + static_cast<uint32_t>(r.i), 0u);
            word_store(words + nl + static_cast<uint32_t>(r.j), 0u);
            const unsigned long long pos = c0 + made + static_cast<unsigned long long>(lane_rank(win));
            if (pos < cap) out[pos] = r;
          }
          made += static_cast<unsigned long long>(__popcll(win));
          stale = true;
          // the marks must have reached the L2 before the next gather reads them there (this wave's next chunk, every
          // wave's next batch behind the barrier below)
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  if (t == 0) {
    *out_count = c0 + made;
    if (stats) {
      stats[0] += rounds;
      stats[1] += n_live;
      stats[2] += c0;
      stats[3] += made;
    }
  }
}

static unsigned round_blocks(uint32_t n_live) {
  const unsigned b = (n_live + kBlock - 1) / kBlock;
  return b < kMaxRoundBlocks ? (b ? b : 1u) : kMaxRoundBlocks;
}

#ifdef NSM_ASSIGN_STATS
static unsigned long long g_assign_atomics[2];  // atomics issued, proposals made (records x rounds)
#endif

static int assign_run(const nsm_hit* hits, uint32_t n, uint32_t nl, uint32_t nr, uint32_t flags, nsm_hit* out,
                      unsigned long long* out_count, unsigned long long* stats, hipStream_t s, uint32_t* scratch) {
  const bool rounds_only = (flags & NSM_ASSIGN_ROUNDS_ONLY) != 0, stream_only = (flags & NSM_ASSIGN_STREAM_ONLY) != 0;
  const size_t n_words = static_cast<size_t>(nl) + nr;
  const size_t words_padded = (n_words + 3) & ~static_cast<size_t>(3);
  uint32_t* ctrl = scratch;
  uint32_t* words = scratch + kCtrlWords;
  uint32_t* lists[2] = {words + words_padded, words + words_padded + n};
  const unsigned long long cap = n < nl ? (n < nr ? n : nr) : (nl < nr ? nl : nr);

  hipError_t e = hipMemsetAsync(ctrl, 0, kCtrlWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: control words");
  if (n_words) {
    e = hipMemsetAsync(words, 0xff, n_words * sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: item words");
  }
  hipLaunchKernelGGL(assign_check_kernel, dim3(round_blocks(n)), dim3(kBlock), 0, s, hits, n, nl, nr, ctrl);
  uint32_t bad = 0;
  e = hipMemcpyAsync(&bad, ctrl + kCtrlBad, sizeof(bad), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: id check");
  if (bad) {
    set_error("nsm_assign_hits: a record's id is outside [0, %u) x [0, %u)", nl, nr);
    return NSM_E_BADARG;
  }

  uint32_t live = n, rounds = 0;
  const uint32_t* cur = nullptr;  // the whole list
  int nxt = 0;
  while (live > 0 && !stream_only) {
    if (!rounds_only && (live <= NSM_ASSIGN_STREAM_BELOW || rounds >= NSM_ASSIGN_MAX_ROUNDS)) break;
    const unsigned blocks = round_blocks(live);
    hipLaunchKernelGGL(assign_propose_kernel, dim3(blocks), dim3(kBlock), 0, s, hits, cur, live, words, nl, ctrl);
    hipLaunchKernelGGL(assign_match_kernel, dim3(blocks), dim3(kBlock), 0, s, hits, cur, live, words, nl, out, cap, out_count);
    e = hipMemsetAsync(ctrl + kCtrlLiveA + nxt, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: live counter");
    hipLaunchKernelGGL(assign_prune_kernel, dim3(blocks), dim3(kBlock), 0, s, hits, cur, live, words, nl, lists[nxt],
                       ctrl + kCtrlLiveA + nxt);
    uint32_t left = 0;
    e = hipMemcpyAsync(&left, ctrl + kCtrlLiveA + nxt, sizeof(left), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: round");
    ++rounds;
    const uint32_t before = live;
    if (left >= before) {
      // (the smallest live record holds both its words: every round matches at least one record)
      set_error("nsm_assign_hits: round %u left %u of %u records live", rounds, left, before);
      return static_cast<int>(hipErrorUnknown);
    }
    live = left;
    cur = lists[nxt];
    nxt ^= 1;
    if (!rounds_only && static_cast<unsigned long long>(live) * NSM_ASSIGN_PAY_DEN >
                            static_cast<unsigned long long>(before) * NSM_ASSIGN_PAY_NUM)
      break;
  }

  if (cur && live > 1) {
    // the prune's appends are in no order; the stream stage walks in rank order
    int bits = 1;
    while ((1ull << bits) < n) ++bits;
    uint32_t* sorted = lists[nxt];
    size_t bytes = 0;
    e = ::rocprim::radix_sort_keys(nullptr, bytes, cur, sorted, static_cast<size_t>(live), 0u, static_cast<unsigned>(bits), s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: radix_sort_keys (size)");
    void* temp = nullptr;
    e = hipMallocAsync(&temp, bytes ? bytes : 1, s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: stream-ordered sort scratch");
    e = ::rocprim::radix_sort_keys(temp, bytes, cur, sorted, static_cast<size_t>(live), 0u, static_cast<unsigned>(bits), s);
    (void)hipFreeAsync(temp, s);
    if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: radix_sort_keys");
    cur = sorted;
  }
  hipLaunchKernelGGL(assign_stream_kernel, dim3(1), dim3(kStreamThreads), 0, s, hits, cur, live, words, nl, out, cap,
                     out_count, stats, rounds);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e, "nsm_assign_hits");
#ifdef NSM_ASSIGN_STATS
  uint32_t counted[2] = {0, 0};
  e = hipMemcpyAsync(counted, ctrl + kCtrlAtomics, sizeof(counted), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: atomics count");
  g_assign_atomics[0] += counted[0];
  g_assign_atomics[1] += counted[1];
#endif
  return 0;
}

}  // namespace nsm

#ifdef NSM_ASSIGN_STATS
// Variant build only: atomics issued by the propose launches and the proposals (live records x rounds) behind them,
// summed over the calls so far.
extern "C" void nsm_assign_atomics(unsigned long long out[2]) {
  out[0] = nsm::g_assign_atomics[0];
  out[1] = nsm::g_assign_atomics[1];
}
#endif

extern "C" int nsm_assign_hits(const nsm_hit* hits, uint64_t n, int32_t left_ids, int32_t right_ids, uint32_t flags,
                               nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  if (!hits && n > 0) {
    set_error("nsm_assign_hits: null hits with n > 0");
    return NSM_E_BADARG;
  }
  if (!out && n > 0) {
    set_error("nsm_assign_hits: null out with n > 0");
    return NSM_E_BADARG;
  }
  if (!out_count) {
    set_error("nsm_assign_hits: null out_count");
    return NSM_E_BADARG;
  }
  if (left_ids < 0 || right_ids < 0) {
    set_error("nsm_assign_hits: negative ids bound (left_ids %d, right_ids %d)", left_ids, right_ids);
    return NSM_E_BADARG;
  }
  if ((flags & NSM_ASSIGN_ROUNDS_ONLY) && (flags & NSM_ASSIGN_STREAM_ONLY)) {
    set_error("nsm_assign_hits: NSM_ASSIGN_ROUNDS_ONLY and NSM_ASSIGN_STREAM_ONLY exclude each other");
    return NSM_E_BADARG;
  }
  if (n >= (1ull << 31)) {
    set_error("nsm_assign_hits: %llu records, ranks are 32-bit (at most 2^31 - 1)", static_cast<unsigned long long>(n));
    return NSM_E_UNSUPPORTED;
  }
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capture) != hipSuccess) capture = hipStreamCaptureStatusNone;
  if (capture != hipStreamCaptureStatusNone) {
    set_error("nsm_assign_hits: the stream is being captured; the call synchronises and cannot be part of a graph");
    return NSM_E_UNSUPPORTED;
  }
  const uint32_t n32 = static_cast<uint32_t>(n), nl = static_cast<uint32_t>(left_ids), nr = static_cast<uint32_t>(right_ids);
  const size_t n_words = static_cast<size_t>(nl) + nr;
  const size_t words_padded = (n_words + 3) & ~static_cast<size_t>(3);
  const size_t lists = (flags & NSM_ASSIGN_STREAM_ONLY) ? 0 : 2 * static_cast<size_t>(n32);
  void* scratch = nullptr;
  hipError_t e = hipMallocAsync(&scratch, (kCtrlWords + words_padded + lists) * sizeof(uint32_t), s);
  if (e != hipSuccess) return hip_status(e, "nsm_assign_hits: stream-ordered scratch");
  const int status = assign_run(hits, n32, nl, nr, flags, out, out_count, reinterpret_cast<unsigned long long*>(stats), s,
                                static_cast<uint32_t*>(scratch));
  (void)hipFreeAsync(scratch, s);
  // the rounds were driven from the host; the stream stage's bookkeeping is the caller's to read after the return
  e = hipStreamSynchronize(s);
  if (status != 0) return status;
  return hip_status(e, "nsm_assign_hits");
}
