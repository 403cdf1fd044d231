// RAW Indel-ratio grid, pruning kernel with a TWO-STAGE histogram filter (included by indel_raw.hip).
//
// The one-stage kernel (indel_raw_kernel<true>) spends its time in eight half-rate v_sad_u8 per pair: the L1 distance of two
// 32-bucket symbol histograms.  Merging bucket b with bucket b + 16 gives a 16-bucket histogram whose L1 distance can only be
// SMALLER (|a1 + a2 - b1 - b2| <= |a1 - b1| + |a2 - b2|), so "coarse L1 <= limit" is a necessary condition too and costs four
// v_sad_u8.  On configs[2] it passes 1 % of the pairs -- far too many for a wave-wide second look (some lane of a row's 64
// passes in 20 % of the rows), so the survivors are handled PER PAIR:
//
//   scan    per push of 16 left rows (two groups of R = 8; a group's 128 bytes of coarse histograms arrive with two
//           s_load_dwordx16, the second group re-uses the first one's 32 SGPRs) and T = 2 right tiles: ONE accumulator
//           register per left row carries both tiles -- 4 v_sad_u8 add tile 0's L1 into the low half, 4 v_sad_hi_u8 tile 1's
//           into the high half -- and the verdict is a CARRY, not a sign: row position r seeds each half with
//           2^(8 + r) - 1 - limit, so bit 8 + r of the half comes out set exactly when L1 > limit (L1 <= 128 and limit >= -1
//           keep the seed in [0, 2^15] and the sum below 2^16: nothing leaves tile 0's half).  One v_bitop3_b32 per row
//           (with a wave-uniform mask) folds bits 8 + r and 24 + r into the group's word, one v_perm_b32 per push puts the
//           first group's verdicts in the odd bytes and the second group's in the even ones, one v_not makes them passes;
//   stack   lanes whose mask is not empty push (first row, lane, mask) on the wave's LDS stack -- one ballot and one
//           ds_write per PUSH of 32 pairs, nothing per pair.  The last 1..15 rows of a length class are scanned one at a
//           time at row position 0 and pushed once;
//   drain   whenever the stack holds more than 128 entries, 64 at a time (64 of 64 lanes busy): lane = one entry, ONE of
//           its pairs (an entry with more pairs goes back on the stack) -- the 32-bucket L1 of the pair (the left histogram
//           gathered from global memory, the right one read from the tile's copy in LDS, 8 v_sad_u8: 1 % of the pairs), then,
//           for the 1e-5 that remain, the bit-parallel LCS of the pair on the SCALAR unit (raw_lcs_pair).  Entries carry
//           their row and its length, so the stack outlives the length classes and is emptied once, at the end.
//
// Every test that drops a pair is an upper bound of the LCS: the hits are the one-stage kernel's, the exhaustive kernel's and
// the oracle's.  Where the time goes on configs[2] (200k x 200k, threshold 0.8, same box, variant builds NSM_C3C_X_*):
// scan 2.71 ms (VALU-bound, every op of it half-rate: 128 v_sad_u8 / v_sad_hi_u8 + 14 v_bitop3 + 1 v_perm + one push of 8
// ops per 16 rows ~ 151 issues of 4.3-4.5 cycles, x 1.02e7 pushes / 1024 SIMDs = 2.75 ms at 2.4 GHz), pop / re-push 0.10,
// the 32-bucket test of 4e8 pairs 0.41, 4.1e5 LCS 0.11 -- 3.32 ms.  Before (a sign per pair shifted into the mask with
// v_alignbit, one push per 8 rows: 176 issues per 16 rows): scan 3.11, kernel 3.76; the one-stage kernel: 5.11 (two tiles
// per wave; 6.54 with one tile and the wave-wide LCS).
#pragma once

namespace nsm {

#ifndef NSM_C3C_TILES
#define NSM_C3C_TILES 2
#endif
#ifndef NSM_C3C_ROWS
#define NSM_C3C_ROWS 8
#endif
constexpr int kC3cStack = 192;  // entries per wave; drained when fewer than 64 slots are left
constexpr int kC3cGroups = 2;   // groups of R left rows per push
// a stack entry: low word = the pass mask of 2 groups x R rows x T tiles = 32 pairs, high word = (first row - chunk start)
// << 13 | la << 6 | lane  (a chunk has at most 2^15 rows: nsm_indel_raw_grid).  Bit p of the mask: byte = p >> 3,
// tile = byte >> 1, group = 1 - (byte & 1), row = 8 group + (p & 7)

// dynamic LDS: [wave][kC3cStack] u64 stack | [wave][T][8][64] u32 right histograms | [wave][T][64] u8 right lengths
//              | lcsmin bytes
static inline size_t c3c_lds_bytes(int tiles) {
  return static_cast<size_t>(kWavesPerBlock) * (kC3cStack * 8 + static_cast<size_t>(tiles) * (8 * kWave * 4 + kWave)) + 136;
}

#ifndef NSM_C3C_OCC
#define NSM_C3C_OCC
#endif
template <int T, int R>
__global__ __launch_bounds__(kBlock) NSM_C3C_OCC void indel_raw_coarse_kernel(
    const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, const int32_t* __restrict__ lstart,
    const int32_t* __restrict__ lorig, const uint32_t* __restrict__ lhist, const uint32_t* __restrict__ lh16,
    const uint8_t* __restrict__ rcodes, const int32_t* __restrict__ rlen, const int32_t* __restrict__ rorig,
    const uint32_t* __restrict__ rhist, const uint32_t* __restrict__ rh16, nsm_hit* __restrict__ hits,
    unsigned long long* __restrict__ count, const IndelRawParams p) {
  // T = 2: one accumulator register per left row carries both tiles (its two 16-bit halves); R = 8: a row's verdicts sit at
  // bits 8 + r and 24 + r, so a group of 8 rows fills bytes 1 and 3; kC3cGroups groups share one 32-bit mask and one push
  static_assert(T == 2 && R == 8 && kC3cGroups == 2 && kC3cGroups * R * T == 32, "two groups of 8 rows x 2 tiles: one mask bit each");
  static_assert(kC3cStack >= 3 * kWave, "a push needs 64 free slots; the drain runs on full passes");
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
  unsigned long long* s_stack = s_mem;
  uint32_t* s_rh = reinterpret_cast<uint32_t*>(s_stack + kWavesPerBlock * kC3cStack);
  uint8_t* s_rl = reinterpret_cast<uint8_t*>(s_rh + kWavesPerBlock * T * 8 * kWave);
  uint8_t* s_lcsmin = s_rl + kWavesPerBlock * T * kWave;
  for (int t = threadIdx.x; t < 132; t += kBlock) s_lcsmin[t] = p.lcsmin[t];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int tile0 = (blockIdx.x * kWavesPerBlock + wave) * T;
  if (tile0 * kWave >= p.n_right) return;
  unsigned long long* stack = s_stack + wave * kC3cStack;
  uint32_t* rh_lds = s_rh + wave * T * 8 * kWave;  // [t][q][lane]
  uint8_t* rl_lds = s_rl + wave * T * kWave;

  bool valid[T];
  int jc[T], lbj[T];
  uint32_t hc[T][4];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int j = (tile0 + t) * kWave + lane;
    valid[t] = j < p.n_right;
    jc[t] = valid[t] ? j : p.n_right - 1;
    lbj[t] = valid[t] ? rlen[jc[t]] : 0;
    const uint4 h = reinterpret_cast<const uint4*>(rh16)[jc[t]];
    hc[t][0] = h.x; hc[t][1] = h.y; hc[t][2] = h.z; hc[t][3] = h.w;
    const uint4* fp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jc[t]) * 8);
    const uint4 f0 = fp[0], f1 = fp[1];
    uint32_t* dst = rh_lds + t * 8 * kWave + lane;
    dst[0 * kWave] = f0.x; dst[1 * kWave] = f0.y; dst[2 * kWave] = f0.z; dst[3 * kWave] = f0.w;
    dst[4 * kWave] = f1.x; dst[5 * kWave] = f1.y; dst[6 * kWave] = f1.z; dst[7 * kWave] = f1.w;
    rl_lds[t * kWave + lane] = static_cast<uint8_t>(lbj[t]);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int i0 = blockIdx.y * p.rows_per_chunk;
  const int i1 = min(p.n_left, i0 + p.rows_per_chunk);
  int q_cnt = 0;  // wave-uniform: entries on the stack

  auto need_of = [&](int la, int lb) -> int { return (la == 0 || lb == 0) ? p.zero_need : static_cast<int>(s_lcsmin[la + lb]); };

  // pop up to 64 entries: lane = one entry, its first pair; entries with more pairs go back on the stack
  auto drain_pass = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n = min(q_cnt, kWave);
    const int base = q_cnt - n;
    const bool active = lane < n;
#ifdef NSM_C3C_X_NODRAIN  // (timing experiments: the entries are dropped)
    q_cnt = base;
    return;
#endif
    const unsigned long long e = stack[base + (active ? lane : 0)];
    uint32_t bits = active ? static_cast<uint32_t>(e) : 0u;
    const uint32_t ehi = static_cast<uint32_t>(e >> 32);
    const int tl = static_cast<int>(ehi & 63u);
    const int la = static_cast<int>((ehi >> 6) & 127u);
    const int ib = i0 + static_cast<int>(ehi >> 13);
    const int pos = active ? 31 - __clz(bits) : 0;  // (an entry on the stack has a bit set)
    bits &= ~(1u << pos);
    const int byte = pos >> 3;  // (the entry format above: the first group of a push sits in the odd bytes)
    const int t = byte >> 1;
    const int r = R * (1 - (byte & 1)) + (pos & 7);
    const int row = active ? ib + r : i0;
    // the 32-bucket filter of the pair
    const uint4* lp = reinterpret_cast<const uint4*>(lhist + static_cast<size_t>(row) * 8);
    const uint4 l0 = lp[0], l1v = lp[1];
    const int lb = rl_lds[t * kWave + tl];
    uint32_t rq[8];
    {
      const uint32_t* rp = rh_lds + t * 8 * kWave + tl;
#pragma unroll
      for (int q = 0; q < 8; ++q) rq[q] = rp[q * kWave];
    }
    uint32_t l1 = 0;
    l1 = __builtin_amdgcn_sad_u8(l0.x, rq[0], l1);
    l1 = __builtin_amdgcn_sad_u8(l0.y, rq[1], l1);
    l1 = __builtin_amdgcn_sad_u8(l0.z, rq[2], l1);
    l1 = __builtin_amdgcn_sad_u8(l0.w, rq[3], l1);
    l1 = __builtin_amdgcn_sad_u8(l1v.x, rq[4], l1);
    l1 = __builtin_amdgcn_sad_u8(l1v.y, rq[5], l1);
    l1 = __builtin_amdgcn_sad_u8(l1v.z, rq[6], l1);
    l1 = __builtin_amdgcn_sad_u8(l1v.w, rq[7], l1);
    const int nd = need_of(la, lb);
    bool pass = active && min(la, lb) >= nd && static_cast<int>(l1) <= la + lb - 2 * nd;
    // entries with pairs left go back (every lane has read its entry: the slots [base, base + n) are free)
    __builtin_amdgcn_wave_barrier();
    const bool more = bits != 0u;
    const unsigned long long mm = __ballot(more);
    if (more) {
      const int slot = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mm >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mm), 0u));
      stack[slot] = (static_cast<unsigned long long>(ehi) << 32) | bits;
    }
    q_cnt = base + __popcll(mm);
    // the pairs that remain (1e-5 of all on configs[2]), one after the other on the scalar unit
#ifdef NSM_C3C_X_NOLCS  // (timing experiments)
    pass = false;
#endif
#ifdef NSM_C3C_X_FINEONLY  // (timing experiments: the 32-bucket test runs, nobody passes -- not known at compile time)
    pass = pass && p.n_left < 0;
#endif
    const int jp = (tile0 + t) * kWave + tl;
    for (unsigned long long todo = __ballot(pass); todo; todo &= todo - 1ull) {
      const int leader = __builtin_ctzll(todo);
      const int row_s = __builtin_amdgcn_readlane(row, leader);
      const int j_s = __builtin_amdgcn_readlane(jp, leader);
      const int la_s = __builtin_amdgcn_readlane(la, leader);
      const int lb_s = __builtin_amdgcn_readlane(lb, leader);
      const int lcs = raw_lcs_pair(lcodes, row_s, la_s, rcodes, j_s, lb_s, lane);
#ifdef NSM_C3C_X_COUNTLCS  // (experiments: one record per LCS call)
      if (lane == 0)
#else
      if (lcs >= need_of(la_s, lb_s) && lane == 0)
#endif
        emit_hit(hits, p.cap, count, indel_score(la_s, lb_s, lcs), lorig[row_s], rorig[j_s]);
    }
  };

  // rows are sorted by length (descending): rows of length 64 - c are [lstart[c], lstart[c + 1])
  const int c_first = 64 - llen[i0];
  const int c_last = 64 - llen[i1 - 1];
  for (int c = c_first; c <= c_last; ++c) {
    const int a = max(i0, lstart[c]);
    const int b = min(i1, lstart[c + 1]);
    if (a >= b) continue;
    const int la = 64 - c;
    // per tile: the pair can only hit if L1 <= limit = la + lb - 2 need (-1: it cannot fit).  Row position r of a group seeds
    // its 16-bit half of the SAD chain with 2^(8 + r) - 1 - limit >= 0 (L1 <= 128): bit 8 + r of the half comes out set <=>
    // L1 > limit, and since seed + L1 < 2^16 nothing carries from tile 0's half into tile 1's
    uint32_t seed[R];
    bool some = false;
    {
      uint32_t below = 0;  // (-1 - limit) of both tiles, one per half
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int need = valid[t] ? need_of(la, lbj[t]) : static_cast<int>(kNever);
        const bool fits = min(la, lbj[t]) >= need;  // exact length filter: LCS <= min(la, lb)
        some = some || fits;
        const int limit = fits ? la + lbj[t] - 2 * need : -1;
        below |= (static_cast<uint32_t>(-1 - limit) & 0xffffu) << (16 * t);
      }
      // (2^(8 + r) + (-1 - limit)) per half: the sum of the halves never borrows, -1 - limit >= -129 > -2^8
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t lo = ((0x100u << r) + (below & 0xffffu)) & 0xffffu;
        const uint32_t hi = ((0x100u << r) + (below >> 16)) & 0xffffu;
        seed[r] = hi << 16 | lo;
      }
    }
    if (!__any(some)) continue;

    const uint32_t* __restrict__ hp = lh16 + static_cast<size_t>(a) * 4;
    const uint32_t lane_field = (static_cast<uint32_t>(la) << 6) | static_cast<uint32_t>(lane);
    // one full group, its 128 bytes of histograms in 32 SGPRs: bits 8 + r / 24 + r of the result = pair (row r, tile 0 / 1)
    // FAILED the coarse test (the other bits: junk)
    auto scan_group = [&](const uint32_t* __restrict__ hp_) -> uint32_t {
      uint32_t h[4 * R];
#pragma unroll
      for (int q = 0; q < 4 * R; ++q) h[q] = hp_[q];
      uint32_t acc = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uint32_t x = seed[r];
#pragma unroll
        for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_sad_u8(h[4 * r + q], hc[0][q], x);
#pragma unroll
        for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_sad_hi_u8(h[4 * r + q], hc[1][q], x);
        // acc = (x & m) | (acc & ~m), m = 0x01000100 << r wave-uniform: one v_bitop3_b32 per row
        acc = r == 0 ? x : __builtin_amdgcn_bitop3_b32(x, 0x01000100u << r, acc, 0xE2);
      }
      return acc;
    };
    // lanes with a pair that passed push (first row, lane, mask): one ballot and one ds_write per push
    auto push = [&](uint32_t acc, int i) {
      const bool nz = acc != 0u;
      const unsigned long long m = __ballot(nz);
      if (m != 0ull) {
        if (nz) {
          const int slot = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), static_cast<uint32_t>(q_cnt)));
          stack[slot] = (static_cast<unsigned long long>((static_cast<uint32_t>(i - i0) << 13) | lane_field) << 32) | acc;
        }
        q_cnt += __popcll(m);
      }
    };
    constexpr int kPush = kC3cGroups * R;  // left rows per push
    const int b_full = a + (b - a) / kPush * kPush;
    for (int i = a; i < b_full;) {
      for (; i < b_full && q_cnt <= kC3cStack - kWave; i += kPush, hp += 4 * kPush) {
        const uint32_t fail_a = scan_group(hp);
        const uint32_t fail_b = scan_group(hp + 4 * R);
        // the first group's verdicts stay in the odd bytes, the second group's move into the even ones: one v_perm_b32
        push(~__builtin_amdgcn_perm(fail_a, fail_b, 0x07030501u), i);
      }
      while (q_cnt >= kWave) drain_pass();  // full passes only: the rest waits for more
    }
    if (b_full < b) {
      // the class's last 1..15 rows, one at a time at row position 0 (verdicts at bits 8 and 24), each moved to its place
      while (q_cnt > kC3cStack - kWave) drain_pass();
      uint32_t acc = 0;
#pragma unroll 1
      for (int r = 0; r < b - b_full; ++r, hp += 4) {
        uint32_t x = seed[0];
#pragma unroll
        for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_sad_u8(hp[q], hc[0][q], x);
#pragma unroll
        for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_sad_hi_u8(hp[q], hc[1][q], x);
        acc |= ((~x >> 8) & 0x00010001u) << ((r < R ? 8 : 0) + (r & (R - 1)));
      }
      push(acc, b_full);
      while (q_cnt >= kWave) drain_pass();
    }
  }
  while (q_cnt > 0) drain_pass();
}

}  // namespace nsm
