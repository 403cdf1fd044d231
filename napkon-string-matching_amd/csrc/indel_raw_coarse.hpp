// RAW Indel-ratio grid, pruning kernel with a TWO-STAGE histogram filter (included by indel_raw.hip).
//
// The one-stage kernel (indel_raw_kernel<true>) spends its time in eight half-rate v_sad_u8 per pair: the L1 distance of two
// 32-bucket symbol histograms.  This kernel asks a cheaper question first, and asks it on the MATRIX pipe, which the
// one-stage kernel leaves idle.  With a_b, r_b the counts of bucket b (symbol & 31) in the left and the right string,
// LCS <= sum_b min(a_b, r_b), and a minimum is a dot product of thermometer codes: min(a, r) = sum_k [a >= k][r >= k].
// The scan computes a bound D = sum_b D_b >= sum_b min(a_b, r_b) >= LCS, so "D >= need" is a NECESSARY condition of a hit,
// need = lcsmin[la + lb].  The exact length filter min(la, lb) >= need stays in front as need = kNever, which no D reaches,
// and need = 0 passes everything.
//
// The codes (NSM_C3C_FP4, the default): FOUR slots per bucket in FP4 (E2M1: 0, 0.5, 1, 1.5, 2, 3, 4, 6), K = 128, in TWO
// v_mfma_f32_32x32x64_f8f6f4 per tile of 32 x 32 pairs, each of the cycles of ONE of the three v_mfma_i32_32x32x32_i8 that
// the i8 codes below take (tools/mfma_fp4_probe: 16.9 ns against 16.0 in a chain, profiles/c3_fp4_ab.txt).  Indicators on
// the left, the count on the right:
//
//   slot   left nibble          right nibble                                      MFMA, nibble of the count's byte
//   1      2.0 [a_b >= 1]       0.5 [r_b >= 1]                                    first (unscaled form), low
//   2      2.0 [a_b >= 2]       0.5 [r_b >= 2]                                    first, high
//   3      2.0 [a_b >= 3]       0.5 [r_b >= 3]                                    second (B scale 2^k), low
//   4      2.0 [a_b >= 4]       E / 2, E = ceil((r_b - 3) / 2^k) rounded UP to    second, high
//                               the next of 0, 1, 2, 3, 4, 6, 8, 12
//
// D_b = [a>=1][r>=1] + [a>=2][r>=2] + 2^k ([a>=3][r>=3] + [a>=4] E).
//
//   scale   k is the right string's block scale exponent: the smallest with max_b r_b - 3 <= 12 x 2^k over ALL its 32
//           buckets.  Both lanes of a string get the same E8M0 byte, so nothing depends on how the hardware maps lanes to
//           scale blocks.  k = 0 where no count exceeds 15, which is every string of the benchmark; k <= 3.
//   bound   for a <= 3: D_b = min(a, r, 2) + 2^k [a >= 3][r >= 3] >= min(a, r), with equality where k = 0;
//           for a >= 4: D_b >= min(r, 3) + max(r - 3, 0) = r >= min(a, r).
//   exact   every value is a multiple of 1/2 far below 2^24, so the f32 accumulation is exact; D <= 128 < kNever
//           (test_no_bound_reaches_never), and the test is D > need - 1/2.  No value is negative, so the f32 bits order
//           as integers do: the fold and the compare are the integer ones of the i8 scan, against the bits of need - 1/2
//           (those of -1/2, need = 0, are a negative integer).
//   layout  both operands of a slot put the same 16 buckets in lane half l >> 5 and the same slot in the same nibble, so
//           the order of k inside the instruction does not matter.
//   left    six instructions a loaded word for both MFMAs: (w + 0x3c3c3c3c) & 0x43434343 is, byte by byte, the count
//           where it is below 4 and 0x40 or more where it is not.  As the selector of v_perm_b32 it reads a four-byte
//           table for 0 .. 3 and gives 0xff from 13 on, which a mask turns into "both nibbles set".
//           (NSM_C3C_FP4_PERM=0: two adds, two ands, a shift and an or a word and MFMA; slower)
//   packed  the left words depend on the row alone, and a row is scanned by every right wave that fits its class: about
//           800 times a launch of configs[2].  Where the grid is large enough (NSM_C3C_PACK_MIN_PAIRS; NSM_FLAG_PACK /
//           NSM_FLAG_NO_PACK) c3c_pack_left_kernel makes them ONCE per call, 64 bytes a row in the stream's kept buffer,
//           and the scan is indel_raw_coarse_kernel<.., true>: a lane loads its two operand fragments, 2 x 16 bytes, and
//           the chains read the loaded registers (no A fragment is made, none is copied; the two sets still swap from
//           block to block).  A captured call never packs.  DESIGN 4.3 step 12, profiles/c3_pack_ab.txt.
//   or fold the packed scan (NSM_C3C_ORFOLD) puts TWO tiles on an accumulator.  A lane's 16 results of a tile are integers of at
//           most 128, so tiles 2 p ("hi") and 2 p + 1 ("lo") of the wave share a register as two 9-bit fixed-point fields on
//           a bias that carries the threshold:
//             acc = BIAS + 2^9 (A.m1 B[hi].m1 + 2^k_hi A.m2 B[hi].m2) + (A.m1 B[lo].m1 + 2^k_lo A.m2 B[lo].m2)
//             BIAS = 2^23 + (256 - need_hi) 2^9 + (256 - need_lo)
//           FOUR chained MFMAs, all in the scaled form: the first reads BIAS as srcC (a tuple of 16 equal registers, made
//           once per run of blocks); the B scale bytes are 0x7f + 9 and 0x7f + 9 + k for an even tile, 0x7f and 0x7f + k for
//           an odd one, in two registers (slots 1 and 2: bytes 0x88, 0x7f in turn; slots 3 and 4: those + k).  Every term
//           is an integer and the sum is below 2^24, so every partial sum is exact and the result, in [2^23, 2^24), has the
//           integer as its mantissa bits: field lo = D_lo + 256 - need_lo in bits 0 .. 8, field hi in bits 9 .. 17.  A field
//           is at most 128 + 256 = 384 < 512: no carry.  Bit 8 of a field is [D >= need]: need = kNever gives at most 129,
//           never flagged; need = 0 always.  The fold is the OR of the 16 registers under the mask 0x20100, seven
//           v_or3_b32 and a v_bitop3_b32, and one v_cmp_ne_u32 and one branch a tile PAIR: 9 VALU for 2048 pairs where the
//           max fold takes 18.  Where the branch is taken, a ballot per flag pushes for tile 2 p (bit 17) and 2 p + 1
//           (bit 8), a column that does not exist masked out, in the same entry format.
//           ONE bias serves the wave's tile pairs, so need_hi is the SMALLEST need of the lane's even tiles and need_lo
//           that of its odd ones (kNever where a column fits no row of the class or does not exist).  A wave whose 128 right
//           strings straddle a length boundary pushes a few entries too many; the drain tests every pair by its own need.
//           tools/mfma_fp4_probe checks the chain bit for bit (k = 0 .. 3) and times it: no slower than two chains of two.
//           128 VGPRs at four waves (amdgpu_waves_per_eu(4): under the budget of two waves the compiler keeps hoisted
//           constants in 133), no scratch, no AGPRs; for that nothing lives across a drain (below), and what a class needs
//           once (the column, the half) is worked out again from the lane.  The unpacked scan keeps the max fold: the grids
//           that do not pack scan short runs of blocks, where the bias tuple and the longer chain cost more than the fold
//           saves.  tests/support/scan_orfold.py restates it.  DESIGN 4.3 step 13, profiles/c3_orfold_ab.txt.
//   codes2  the PACKED scan (NSM_C3C_CODES2) keeps slots 1 and 2 and makes slots 3 and 4 VALUE TABLES on both sides, found by
//           tools/c3_code_search.py: D_b = min(a, r, 2) + 2^k (x3(a) y3(r') + x4(a) y4(r')), tables over the counts 0 .. 15 with
//           x3 y3 + x4 y4 >= max(min(a, r) - 2, 0); a left count above 15 reads entry 15, a scaled right count entry
//           r' = 2 + ceil((r - 2) / 2^k).  The code of before gives r where a >= 4 (ten times looser than sum of min on the
//           benchmark's strings, whose 37 symbols put two in five of the 32 buckets); the tables pass 0.30 of its pairs on the
//           tool's sample and pushed 1.21 million entries a launch where it pushed 3.52 (200k x 200k).  The left words are made
//           by the pre-pass (c3c_fp4_left_packed), the right ones by other constants in the same ten instructions a word, so
//           the scan loop's instructions are those of before.  Products are multiples of 1/4 and D <= 162, so the OR fold keeps
//           4 D in two 11-bit fields: field = 4 D + 1024 - 4 need, flags in bits 10 and 21, B scale bytes 0x7f + 2 and 0x7f + 13
//           (+ k), BIAS = 2^23 + (1024 - 4 need_hi) 2^11 + (1024 - 4 need_lo); the sum stays below 2^24 and every term is an
//           integer (tools/mfma_fp4_probe, chain4 quarters).  The unpacked scan, and NSM_C3C_CODES2=0, keep the codes above and
//           the 9-bit fields below.  tests/support/scan_codes2.py restates it.  DESIGN 4.3 step 15, profiles/c3_codes2_ab.txt.
//   right   made once by the wave and again behind a drain.  k = 0: byte tables too, v_perm_b32 with the count's low
//           three bits as the selector and the table of 0 .. 7 or of 8 .. 15 by its bit 3.  k > 0: byte by byte, the
//           excess through a 13-nibble table in a 64-bit constant.
//
// tests/support/scan_fp4.py restates the codes; tests/test_cpu_indel_raw_scan_fp4.py checks every count.
//
// The i8 codes (NSM_C3C_FP4=0, the scan of before: DESIGN 4.3 steps 6 to 10): D_b = min(a_b, r_b) where r_b < CAP and a_b
// where r_b >= CAP, CAP slots of MIXED weight per bucket (K = 32 CAP, CAP v_mfma_i32_32x32x32_i8 per tile):
//
//   left row,  slot s < CAP - 1:  64 [a_b >= s + 1]   right row, slot s < CAP - 1:  [r_b >= s + 1] - [r_b >= CAP]   (0 or 1)
//   left row,  last slot:         a_b                 right row, last slot:         64 [r_b >= CAP]
//
// The dot product is D' = 64 D exactly, tested as D' > 64 need - 1; every operand byte is 0 .. 64 (a stride-64 row has
// a_b <= 64), D' <= 4096 < 64 kNever.  64 [c >= k] of four counts in a word is (w + (0x40 - k) 0x01010101) & 0x40404040, and
// the last left slot is the loaded word itself.
//
//   waves   a wave owns NT right tiles of 32 strings and one chunk of left rows.  Where none of its right strings fits any
//           length class of the chunk (46 % of the waves of configs[2]) it returns before it builds anything
//           (NSM_C3C_EARLY_OUT): the left lengths that fit a right string are an interval around its own length, so the
//           class nearest to it decides;
//   scan    the B fragments of the wave's tiles: lane = column l & 31, buckets 16 (l >> 5) .. + 15.  FP4: two fragments
//           of four registers a tile and one register with the four tiles' scale bytes, picked with op_sel; a lane reads
//           both halves of its string at the start, for the scale.  i8: CAP fragments a tile.  They are built from the
//           right fine histograms at the start, and again from the wave's LDS copy behind a drain between the tiles,
//           which needs their registers.
//           Left rows come in blocks of 32 of one length class: lane l loads 16 bytes of row l & 31 (a 32-bit offset from
//           the chunk's first row) and makes its A fragments: two with FP4; CAP - 1 with i8, where the last slot is the
//           loaded words as they are.  Per tile the MFMAs are chained on an accumulator.  The words of consecutive blocks
//           go to two register sets in turn (the block loop is unrolled by two), so no word is copied.
//           The 16 results of a lane (rows (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the block, column l & 31 of the tile: the
//           C layout of the 32x32 MFMA does not depend on the operand type) are folded with v_max3_i32 and compared with
//           the lane's need once, and that is all the scan asks: WHICH of the 16 rows passed is left to the drain, so the
//           accumulator is dead after its fold and a tile's epilogue is the fold, a compare and a ballot.  The last block
//           of a class in a chunk repeats its last row where it is short of 32; the repeated rows take part in the fold,
//           and the drain leaves them out;
//   order   TWO accumulators, tile t in acc[t & 1] (NSM_C3C_PIPE, NT even): the chain of tile t + 1 -- after a block's last
//           tile that of tile 0 of the class's next block, whose A fragments are made just before -- is issued before the
//           branch and the push of tile t, with the v_max3_i32 of tile t's fold between and behind its MFMAs (a chained
//           MFMA waits for the one before it, and a wave issues in order).  FP4: MFMA, four of the fold's eight, MFMA,
//           four (NSM_C3C_FP4_SPLIT); an empty asm that names the new accumulator keeps the second MFMA in front of the
//           branch.  So the matrix pipe works under the wave's own epilogue and not only under those of the SIMD's other
//           waves.  OR fold: the units are tile pairs, MFMA, two of the fold's eight, four times (NSM_C3C_OR_SPLIT), and the
//           first chain of the block after is issued without a branch around it (a pair is every other unit; behind a
//           branch no fold stands between its MFMAs), its result dropped where that block does not run.  The pipeline is
//           filled at the start of a run of blocks -- a length class, or what is left of it behind a drain -- and is empty
//           at its end: the block that decides on a drain ends the run, and the next run drains first and loads its words
//           again, so no accumulator, no word, no bias lives across a drain; NSM_C3C_PIPE=0 is the order of before, chain,
//           fold, chain, fold on one accumulator;
//   stack   lanes whose folded result passes push (block's first row, la, tile, lane, rows of the block that exist) on the
//           wave's LDS stack, 8 bytes: one ballot per tile of 1024 pairs and one ds_write where it is not empty, at most 64
//           entries a tile (OR fold: 128 a tile pair: the stack has room for NT x 64 between two checks and one more pair);
//   drain   whenever more than 128 entries are on the stack, checked every NT tiles (in front of a block's last tile, whose
//           entries are still pushed before the drain runs, and at the start of a class), 64 entries at a time (64 of 64
//           lanes busy), an entry handled ONCE for all its rows (nothing goes back on the stack).  A pass has four quarters
//           of 16 entries; in a quarter FOUR lanes have one entry, lane m of them its rows 8 g + 4 (lane >> 5) + m, g = 0 .. 3:
//           the lane reads the right string's 32-bucket histogram and length from the wave's copy in LDS once and runs the
//           exact test, min(la, lb) >= need and L1 <= la + lb - 2 need (8 v_sad_u8 a row, the chain started from the negated
//           budget so that the verdict is its sign), on its four rows, their eight loads issued before the first chain.
//           The four lanes of an entry read four consecutive rows, 128 contiguous bytes of the left histograms, with each
//           load (with an entry per lane and 16 rows each, every lane of every load sat in a cache line of its own and the
//           32-bucket test cost 0.28 ms of the launch instead of 0.04).  The exact test is stricter than the scan's bound
//           (sum of min <= D), so the coarse result is not needed row by row; rows at or past the entry's row count read
//           the block's last row and their verdict is dropped, so no pair shows twice.  The result is a 16-bit mask per
//           lane (bit 4 quarter + g) of the pairs that go on to the bit-parallel LCS on the SCALAR unit (raw_lcs_units in
//           indel_raw.hip), one pair after the other, lane by lane (the lowest lane of a ballot leads) and within a lane from
//           its highest bit down, the pair's entry read again from the stack: the longer string of the pair is the pattern,
//           the shorter one the text, and the chain
//           stops after a word of four text units where LCS so far + text units left < need (99.5 % of these pairs are
//           no hits); the two 64-byte rows of the NEXT surviving pair are requested before the current pair's chain runs
//           (NSM_C3C_LCS_PREFETCH).  Entries carry their row and its length, so the stack outlives the length classes and
//           is emptied once, at the end.
//
// Every test that drops a pair is an upper bound of the LCS: the hits are the one-stage kernel's, the exhaustive kernel's and
// the oracle's.  Measurements: profiles/c3_mfma_ab.txt, profiles/c3_pipe_ab.txt, profiles/c3_codes_ab.txt, profiles/c3_lcs_ab.txt,
// profiles/c3_rows_ab.txt, profiles/c3_fp4_ab.txt and DESIGN 4.3.
#pragma once

namespace nsm {

#ifndef NSM_C3C_CAP
#define NSM_C3C_CAP 3  // i8 scan: code slots per bucket (4: an eighth of the survivors, a third more MFMAs)
#endif
#ifndef NSM_C3C_FP4
#define NSM_C3C_FP4 1  // 1: FP4 codes, four slots per bucket in two MFMAs (CAP is not used); 0: the i8 scan, CAP MFMAs per tile
#endif
#ifndef NSM_C3C_FP4_PERM
#define NSM_C3C_FP4_PERM 1  // 1: the left operand words from a v_perm_b32 byte table; 0: two adds, a shift and three ands each
#endif
#ifndef NSM_C3C_FP4_SPLIT
#define NSM_C3C_FP4_SPLIT 4  // instructions of a tile's fold between the two MFMAs of the next tile's chain (the rest behind them)
#endif
#ifndef NSM_C3C_NT
#define NSM_C3C_NT 4  // right tiles of 32 strings per wave
#endif
#ifndef NSM_C3C_ORFOLD
// 1: the PACKED FP4 scan puts two tiles on an accumulator as fixed-point fields on a bias that holds the lane's needs, and
// folds with OR on the fields' flag bits (NT even); 0, and the unpacked scan always: a tile per accumulator, max fold and a
// compare with the tile's need (the i8 scan's)
#define NSM_C3C_ORFOLD (NSM_C3C_FP4 && NSM_C3C_NT % 2 == 0)
#endif
#ifndef NSM_C3C_CODES2
// 1: the PACKED scan's slots 3 and 4 are value TABLES on both sides (tools/c3_code_search.py), their products multiples of
// 1/4, and the OR fold's fields are 11 bits of 4 D; 0: the indicator and excess codes of the unpacked scan in 9-bit fields
// (the packed kernel of before, instruction for instruction).  The unpacked scan keeps the old codes either way
#define NSM_C3C_CODES2 1
#endif
#ifndef NSM_C3C_PIPE
// 1: two accumulators, a tile's (OR fold: a tile pair's) MFMAs are issued around the fold of the one before; the number of
// tiles (tile pairs) of a wave must be even
#define NSM_C3C_PIPE (NSM_C3C_NT % (NSM_C3C_ORFOLD ? 4 : 2) == 0)
#endif
#ifndef NSM_C3C_OR_SPLIT
#define NSM_C3C_OR_SPLIT 2  // OR fold: instructions of a tile pair's fold behind each of the first three MFMAs of the next chain
#endif
#ifndef NSM_C3C_LCS_PREFETCH
#define NSM_C3C_LCS_PREFETCH 1  // 1: the drain requests the next surviving pair's rows before the current pair's LCS chain
#endif
#ifndef NSM_C3C_EARLY_OUT
#define NSM_C3C_EARLY_OUT 1  // 1: a wave whose right strings fit no length class of its chunk returns before its set-up
#endif
#ifndef NSM_C3C_PERSIST
// 1: the packed scan is a fixed number of waves that pull work items from a list made by the pre-pass (c3p_prepass_kernel);
// 0, the default: one wave per (right tile, left chunk).  Measured at 200k x 200k (profiles/c3_persist_ab.txt, DESIGN 4.3
// step 14): 3.29 ms against 0.896.  The list is in tile-major order, so the waves that run together scan rows from all over
// the left table, where the static grid's (dispatched tile-first) share one chunk of 150 KB in L2.  The hits are the same, and
// NSM_FLAG_ONE_GROUP takes the persistent launch in either build, with one workgroup: the tests keep it honest
#define NSM_C3C_PERSIST 0
#endif
#ifndef NSM_C3P_ITEM_ROWS
#define NSM_C3P_ITEM_ROWS 0  // left rows per work item, a multiple of 32 (A/B runs); 0: what pick_rows_per_chunk gives a chunk
#endif
constexpr int kC3cBlock = 32;                // left rows per block = right strings per tile: the M and N of the MFMA
constexpr int kC3cRights = NSM_C3C_NT * kC3cBlock;  // right strings per wave
// entries per wave; drained when more than kC3cDrainAt are on it.  NT x 64 pushes between two drain checks, and the pipelined scan
// pushes one more tile's before the drain it has decided on runs (the pipeline is emptied first); with the OR fold that is a
// tile PAIR's, 128 entries
constexpr int kC3cPipeExtra = NSM_C3C_PIPE ? (NSM_C3C_ORFOLD ? 2 : 1) : 0;
constexpr int kC3cStack = (NSM_C3C_NT + 2 + kC3cPipeExtra) * kWave;
constexpr int kC3cDrainAt = 2 * kWave;
// a stack entry: one lane of the scan whose folded result passed, that is its 16 left rows (k & 3) + 8 (k >> 2) + 4 (lane >> 5)
// of the block, k = 0 .. 15, against right string tile * 32 + (lane & 31) of the wave.  Low word = the number of rows of the block
// that exist, 1 .. 32 (the drain tests those and no others), high word = (block's first row - chunk start) << 15 | la << 8 |
// tile << 6 | lane (a chunk has at most 2^15 rows: nsm_indel_raw_grid)
static_assert(NSM_C3C_NT >= 1 && NSM_C3C_NT <= 4, "an entry keeps its tile in 2 bits");
// (CAP 2 is the smallest code with an excess slot beside an indicator; beyond 8 the B fragments alone take 128 registers)
static_assert(NSM_C3C_CAP >= 2 && NSM_C3C_CAP <= 8, "code slots per bucket");

// dynamic LDS: [wave][kC3cStack] u64 stack | [wave][8][rights] u32 right histograms | [wave][rights] u8 right lengths
//              | lcsmin bytes
static inline size_t c3c_lds_bytes() {
  return static_cast<size_t>(kWavesPerBlock) * (kC3cStack * 8 + static_cast<size_t>(kC3cRights) * (8 * 4 + 1)) + 136;
}

typedef int c3c_v4i __attribute__((ext_vector_type(4)));
typedef int c3c_v16i __attribute__((ext_vector_type(16)));
typedef int c3c_v8i __attribute__((ext_vector_type(8)));
typedef float c3c_v16f __attribute__((ext_vector_type(16)));

// 64 [c >= k] in each of the four bytes of w (0 <= c <= 64, 1 <= k <= 8: c + 0x40 - k is 56 .. 127, bit 6 where c >= k)
__device__ __forceinline__ uint32_t c3c_ge64(uint32_t w, int k) {
  return (w + static_cast<uint32_t>(0x40 - k) * 0x01010101u) & 0x40404040u;
}

// --- the FP4 codes (NSM_C3C_FP4).  E2M1 nibbles: 0, 0.5, 1, 1.5, 2, 3, 4, 6 for codes 0 .. 7 (bit 3 is the sign: never set).

// the scale exponent k of a right string from its eight histogram words: the smallest k with max(r_b) - 3 <= 12 x 2^k, so
// that its largest excess fits the grid {0, 1, 2, 3, 4, 6, 8, 12} 2^k.  k = 0 exactly where no count has a bit above 15
__device__ __forceinline__ int c3c_fp4_scale(const uint4& f0, const uint4& f1) {
  const uint32_t ws[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
  uint32_t any = 0u;
#pragma unroll
  for (int q = 0; q < 8; ++q) any |= ws[q];
  if ((any & 0xf0f0f0f0u) == 0u) return 0;
  uint32_t top = 0u;
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int b = 0; b < 4; ++b) top = max(top, (ws[q] >> (8 * b)) & 0xffu);
  return top <= 27u ? 1 : top <= 51u ? 2 : 3;
}
// the right operand words of four counts.  m1: 0.5 [r >= 1] in the low nibble of a count's byte, 0.5 [r >= 2] in the high
// one.  m2: 0.5 [r >= 3] in the low nibble; in the high one E, the excess max(r - 3, 0) over 2^k rounded UP to the next of
// 0, 1, 2, 3, 4, 6, 8, 12, as the code of its half (the left indicator is 2.0).
// k = 0 (every count <= 15, nearly every string): both bytes of a count from 8-entry byte tables, v_perm_b32 with the
// count's low three bits as the selector, the table of 0 .. 7 or that of 8 .. 15 by its bit 3 -- ten instructions a word
// where a byte at a time takes forty, and a wave that scans a short chunk pays for its set-up
__device__ __forceinline__ void c3c_fp4_right_k0(uint32_t fw, int& m1, int& m2) {
  const uint32_t sel = fw & 0x07070707u;
  const uint32_t big = ((fw >> 3) & 0x01010101u) * 0xffu;  // 0xff where 8 <= r <= 15
  const uint32_t lo1 = __builtin_amdgcn_perm(0x11111111u, 0x11110100u, sel);
  const uint32_t lo2 = __builtin_amdgcn_perm(0x41312111u, 0x01000000u, sel), hi2 = __builtin_amdgcn_perm(0x71717171u, 0x61615151u, sel);
  m1 = static_cast<int>((big & 0x11111111u) | (~big & lo1));
  m2 = static_cast<int>((big & hi2) | (~big & lo2));
}
// k > 0: byte by byte, E from the table's nibble 4 q for q = 0 .. 12
__device__ __forceinline__ void c3c_fp4_right_scaled(uint32_t fw, int k, int& m1, int& m2) {
  m1 = static_cast<int>((c3c_ge64(fw, 1) >> 6) | (c3c_ge64(fw, 2) >> 2));
  uint32_t w2 = c3c_ge64(fw, 3) >> 6;
  const uint32_t round_up = (1u << k) - 1u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t r = (fw >> (8 * b)) & 0xffu;
    const uint32_t q = (max(r, 3u) - 3u + round_up) >> k;  // 0 .. 12 by the choice of k
    w2 |= (static_cast<uint32_t>(0x7777665543210ull >> (4u * q)) & 0xfu) << (8 * b + 4);
  }
  m2 = static_cast<int>(w2);
}
// the left operand words of four counts: 2.0 [c >= 1] (low nibble) and 2.0 [c >= 2] (high) in m1, 2.0 [c >= 3] and
// 2.0 [c >= 4] in m2.  With the byte table: c + 0x3c is 60 .. 124, so (c + 0x3c) & 0x43 is c where c < 4 and 0x40 or more
// where c >= 4; v_perm_b32 reads selector bytes 0 .. 3 from the table and gives 0xff for 13 and above, which the mask
// turns into "both set"
__device__ __forceinline__ void c3c_fp4_left(uint32_t w, int& m1, int& m2) {
#if NSM_C3C_FP4_PERM
  const uint32_t sel = (w + 0x3c3c3c3cu) & 0x43434343u;
  m1 = static_cast<int>(__builtin_amdgcn_perm(0u, 0x44440400u, sel) & 0x44444444u);
  m2 = static_cast<int>(__builtin_amdgcn_perm(0u, 0x04000000u, sel) & 0x44444444u);
#else
  m1 = static_cast<int>(((c3c_ge64(w, 1) >> 4)) | c3c_ge64(w, 2));
  m2 = static_cast<int>(((c3c_ge64(w, 3) >> 4)) | c3c_ge64(w, 4));
#endif
}
// --- the codes of the packed scan (NSM_C3C_CODES2): slots 1 and 2 as above, slots 3 and 4 value tables by count 0 .. 15, the
// byte of a count = slot 3's E2M1 code in the low nibble, slot 4's in the high one; words = counts 0 - 3, 4 - 7, 8 - 11, 12 - 15.
// The output of tools/c3_code_search.py (SHIPPED there; tests/support/scan_codes2.py restates them):
//   count        0  1  2    3    4    5    6    7    8    9   10   11   12   13   14   15
//   x3 (left)    0  0  0    2    2    2    2    2    2    2    2    3    4    4    4    6
//   x4 (left)    0  0  0    0    1    1  1.5    2    2    2    2    2    2    2    2    2
//   y3 (right)   0  0  0  0.5  0.5  0.5  0.5  0.5  0.5  0.5    1    1    1  1.5  1.5  1.5
//   y4 (right)   0  0  0    0    1    2    2    2    3    3    3    3    3    3    3    3
// x3(a) y3(r) + x4(a) y4(r) >= max(min(a, r) - 2, 0) for all a, r <= 15.  A left count above 15 reads entry 15; a right count
// r >= 3 of a string with scale exponent k reads entry 2 + ceil((r - 2) / 2^k) <= 15 (c3c_fp4_scale's k) and the MFMA scales
// the product by 2^k: 2^k max(min(min(a, 15), entry) - 2, 0) >= min(a, r) - 2.
constexpr uint32_t kC3cLeft2[4] = {0x04000000u, 0x44342424u, 0x45444444u, 0x47464646u};
constexpr uint32_t kC3cRight2[4] = {0x01000000u, 0x41414121u, 0x52525151u, 0x53535352u};
// the table bytes of four counts 0 .. 15: two v_perm_b32 on the counts' low three bits, the one of 0 .. 7 or of 8 .. 15 by bit 3
__device__ __forceinline__ uint32_t c3c_codes2_bytes(uint32_t w, const uint32_t (&t)[4]) {
  const uint32_t sel = w & 0x07070707u;
  const uint32_t big = ((w >> 3) & 0x01010101u) * 0xffu;  // 0xff where 8 <= count <= 15
  return (big & __builtin_amdgcn_perm(t[3], t[2], sel)) | (~big & __builtin_amdgcn_perm(t[1], t[0], sel));
}
// the left words of the pre-pass: m1 as c3c_fp4_left's; m2 from the table, a count above 15 (c + 0x70 has bit 7: a count is
// at most 64, nothing carries) taken as 15
__device__ __forceinline__ void c3c_fp4_left_packed(uint32_t w, int& m1, int& m2) {
#if NSM_C3C_CODES2
  int old2;
  c3c_fp4_left(w, m1, old2);
  const uint32_t over = (((w + 0x70707070u) >> 7) & 0x01010101u) * 0xffu;
  m2 = static_cast<int>(c3c_codes2_bytes((w | over) & 0x0f0f0f0fu, kC3cLeft2));
#else
  c3c_fp4_left(w, m1, m2);
#endif
}
// the right words, k = 0: other constants in c3c_fp4_right_k0's scheme, ten instructions a word
__device__ __forceinline__ void c3c_codes2_right_k0(uint32_t fw, int& m1, int& m2) {
  const uint32_t sel = fw & 0x07070707u;
  const uint32_t big = ((fw >> 3) & 0x01010101u) * 0xffu;
  const uint32_t lo1 = __builtin_amdgcn_perm(0x11111111u, 0x11110100u, sel);
  const uint32_t lo2 = __builtin_amdgcn_perm(kC3cRight2[1], kC3cRight2[0], sel), hi2 = __builtin_amdgcn_perm(kC3cRight2[3], kC3cRight2[2], sel);
  m1 = static_cast<int>((big & 0x11111111u) | (~big & lo1));
  m2 = static_cast<int>((big & hi2) | (~big & lo2));
}
// k > 0: byte by byte, the table's entry 2 + ceil((r - 2) / 2^k) (r < 3: entry 2, which is zero like entries 0 and 1)
__device__ __forceinline__ void c3c_codes2_right_scaled(uint32_t fw, int k, int& m1, int& m2) {
  m1 = static_cast<int>((c3c_ge64(fw, 1) >> 6) | (c3c_ge64(fw, 2) >> 2));
  const unsigned long long lo = (static_cast<unsigned long long>(kC3cRight2[1]) << 32) | kC3cRight2[0];
  const unsigned long long hi = (static_cast<unsigned long long>(kC3cRight2[3]) << 32) | kC3cRight2[2];
  const uint32_t round_up = (1u << k) - 1u;
  uint32_t w2 = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t r = (fw >> (8 * b)) & 0xffu;
    const uint32_t e = min(2u + ((max(r, 2u) - 2u + round_up) >> k), 15u);  // (15 or below by the choice of k: the clamp guards the shift)
    w2 |= (static_cast<uint32_t>((e & 8u ? hi : lo) >> (8u * (e & 7u))) & 0xffu) << (8 * b);
  }
  m2 = static_cast<int>(w2);
}
// slots 1 and 2: the unscaled form (both scale arguments literal 0)
__device__ __forceinline__ c3c_v16f c3c_fp4_mfma1(const c3c_v4i& a, const c3c_v4i& b) {
  const c3c_v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0}, b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};  // (FP4: the upper half is not read)
  const c3c_v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, zero, 4, 4, 0, 0, 0, 0);
}
// slots 3 and 4: A scale 1.0, B scale byte t of `scales` (op_sel has to be a literal)
__device__ __forceinline__ c3c_v16f c3c_fp4_mfma2(const c3c_v4i& a, const c3c_v4i& b, const c3c_v16f& acc, int scales, int t) {
  const c3c_v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0}, b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};
  switch (t) {
    case 0: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 4, 0, 0x7f7f7f7f, 0, scales);
    case 1: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 4, 0, 0x7f7f7f7f, 1, scales);
    case 2: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 4, 0, 0x7f7f7f7f, 2, scales);
    default: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 4, 0, 0x7f7f7f7f, 3, scales);
  }
}

// --- the packed left rows (NSM_C3C_FP4): c3c_fp4_left of a row depends on the row alone, and a row is scanned by every
// right wave whose strings fit its length class.  The pre-pass codes every row ONCE per call; the packed scan
// (indel_raw_coarse_kernel<.., true>) loads the operand words and makes no A fragment.  A packed row is 64 bytes,
// [half 0: m1 words 16 B | m2 words 16 B][half 1: m1 | m2], rows in table order: lane (col, half) of a block reads the 32
// contiguous bytes at row * 64 + half * 32.  tests/support/scan_pack.py restates the layout.
constexpr int kC3cPackedRow = 64;
#ifndef NSM_C3C_PACK_MIN_PAIRS
// the smallest grid (left rows x right rows) that packs by itself.  Measured, forced pack against the parent's kernel
// (profiles/c3_pack_ab.txt): 8k x 8k +0.009 ms, 20k x 20k +0.008, 50k x 50k +0.020, 100k x 100k -0.011, 200k x 200k -0.147.
// The pre-pass, the allocation and the doubled bytes at the start of every length class cost more than the coding saves
// where a wave scans a short chunk; the floor is the smallest measured grid at which every packed run beat every parent run
#define NSM_C3C_PACK_MIN_PAIRS 10000000000ll
#endif
static inline bool c3c_pack_pays(long long pairs) { return pairs >= static_cast<long long>(NSM_C3C_PACK_MIN_PAIRS); }
struct c3c_packed_rows {
  c3c_v4i m1, m2;
};
template <bool PACKED>
struct c3c_rows {
  typedef uint4 type;  // the lane's 16 histogram bytes
};
template <>
struct c3c_rows<true> {
  typedef c3c_packed_rows type;  // the lane's two A fragments
};

// one thread per (row, half) of the whole table: 16 histogram bytes in, 32 operand bytes out
__device__ __forceinline__ void c3c_pack_left_unit(const uint32_t* __restrict__ lhist, c3c_v4i* __restrict__ packed, int n_left,
                                                   int u) {  // u = 2 row + half
  if (u >= 2 * n_left) return;
  const uint4 w = reinterpret_cast<const uint4*>(lhist)[u];
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
  c3c_v4i m1, m2;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int a1, a2;
    c3c_fp4_left_packed(ws[q], a1, a2);
    m1[q] = a1;
    m2[q] = a2;
  }
  packed[2 * static_cast<size_t>(u)] = m1;
  packed[2 * static_cast<size_t>(u) + 1] = m2;
}
__global__ __launch_bounds__(kBlock) void c3c_pack_left_kernel(const uint32_t* __restrict__ lhist, c3c_v4i* __restrict__ packed,
                                                               int n_left) {
  c3c_pack_left_unit(lhist, packed, n_left, blockIdx.x * kBlock + threadIdx.x);
}

// --- the persistent launch of the packed scan (NSM_C3C_PERSIST): a fixed number of waves pull WORK ITEMS from a list that the
// pre-pass makes on the device, every call (nothing is kept from call to call: the library cannot know that a table's
// contents stayed the same).  An item is (right tile of kC3cRights strings, first left row, end row, base row).
//
//   interval  both tables are sorted by length, descending.  The left lengths that fit a right string of lb units are an
//             interval (NSM_C3C_EARLY_OUT above); the host tabulates its ends for every lb from lcsmin, la_lo[lb] and la_hi[lb]
//             (65 and 0: nothing fits), and a tile's left lengths are the HULL of its strings' intervals, lengths
//             rlen[last] .. rlen[first]: rows [lstart[64 - hi], lstart[64 - lo + 1]).  zero_need == 0: every row.  The hull is a
//             superset (a tile of lengths 16 and 64 covers what lies between), and that is all the scan relies on: it keeps its
//             own test per class and lane.
//   items     the interval is cut into WINDOWS of 2^15 rows from its first row, and a window into items of at most item_rows
//             rows (a multiple of 32).  The base of an item is its window's first row: a stack entry keeps its row relative to
//             it in 15 bits (ehi >> 15) and the scan's 32-bit byte offsets count from it, so a wave that goes on with the
//             next item of the same tile and window keeps its stack.
//   list      in tile-major order, queue[1] = the number of items, queue[0] = 0: the head that the waves pull from.
//
// The pre-pass is c3c_pack_left_kernel's grid with ceil(tiles / 256) blocks in front.  Block r lists the items of tiles
// 256 r .. 256 r + 255, one tile a thread: it counts the items of the tiles before its own (a few loads a tile) for its
// place in the list, so no block waits for another.  tests/support/scan_items.py restates the rules.
constexpr int kC3pWindow = 1 << 15;
struct C3pItemParams {
  int n_left, n_right, n_tiles, item_rows, every_row;
  unsigned int cap;            // items the list has room for: tiles x c3p_items_of(n_left), which no table exceeds
  uint8_t la_lo[65], la_hi[65];  // by the right string's length: the smallest and the largest left length that fits
};
// the items of an interval of `rows` rows
__host__ __device__ static inline int c3p_items_of(int rows, int item_rows) {
  const int per_window = (kC3pWindow + item_rows - 1) / item_rows;
  return (rows >> 15) * per_window + ((rows & (kC3pWindow - 1)) + item_rows - 1) / item_rows;
}
// the kept buffer of a persistent call: [item list, BACKWARDS: item k ends 16 k bytes in front of the queue][queue: 64 bytes,
// word 0 the head, word 1 the item count][packed rows]
constexpr int kC3pQueueBytes = 64;
__host__ __device__ static inline unsigned int* c3p_queue(const char* lpacked) {
  return reinterpret_cast<unsigned int*>(const_cast<char*>(lpacked) - kC3pQueueBytes);
}
__host__ __device__ static inline int4* c3p_item(unsigned int* queue, unsigned int k) {
  return reinterpret_cast<int4*>(queue) - 1 - k;
}
__global__ __launch_bounds__(kBlock) void c3p_prepass_kernel(const uint32_t* __restrict__ lhist, c3c_v4i* __restrict__ packed,
                                                             const int32_t* __restrict__ rlen, const int32_t* __restrict__ lstart,
                                                             unsigned int* __restrict__ queue,
                                                             const C3pItemParams ip, int item_blocks) {
  if (static_cast<int>(blockIdx.x) >= item_blocks) {
    c3c_pack_left_unit(lhist, packed, ip.n_left, (static_cast<int>(blockIdx.x) - item_blocks) * kBlock + static_cast<int>(threadIdx.x));
    return;
  }
  __shared__ unsigned long long s_scan[kBlock];
  const int tid = threadIdx.x;
  // the left rows of tile t: first row and number of rows
  auto interval = [&](int t, int& r0) -> int {
    r0 = 0;
    if (ip.every_row) return ip.n_left;
    const int j_a = t * kC3cRights, j_b = min(j_a + kC3cRights, ip.n_right) - 1;
    const int lb_a = min(max(rlen[j_a], 0), 64), lb_b = min(max(rlen[j_b], 0), 64);
    int lo = 65, hi = 0;
    for (int lb = min(lb_a, lb_b); lb <= max(lb_a, lb_b); ++lb) {
      lo = min(lo, static_cast<int>(ip.la_lo[lb]));
      hi = max(hi, static_cast<int>(ip.la_hi[lb]));
    }
    if (hi < lo) return 0;
    r0 = lstart[64 - hi];
    return lstart[64 - lo + 1] - r0;
  };
  unsigned int before = 0u;  // items of the tiles of the blocks in front, this thread's share
  for (int t = tid; t < static_cast<int>(blockIdx.x) * kBlock; t += kBlock) {
    int r0;
    before += static_cast<unsigned int>(c3p_items_of(interval(t, r0), ip.item_rows));
  }
  const int tile = static_cast<int>(blockIdx.x) * kBlock + tid;
  int r0 = 0, rows = 0;
  if (tile < ip.n_tiles) rows = interval(tile, r0);
  const unsigned int own = static_cast<unsigned int>(c3p_items_of(rows, ip.item_rows));
  // one inclusive scan for both: `before` in the upper word, `own` in the lower (the list has fewer than 2^31 items)
  unsigned long long v = (static_cast<unsigned long long>(before) << 32) | own;
  s_scan[tid] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const unsigned long long add = tid >= d ? s_scan[tid - d] : 0ull;
    __syncthreads();
    v += add;
    s_scan[tid] = v;
    __syncthreads();
  }
  const unsigned long long total = s_scan[kBlock - 1];
  const unsigned int carry = static_cast<unsigned int>(total >> 32);
  unsigned int at = carry + static_cast<unsigned int>(v) - own;
  const int per_window = (kC3pWindow + ip.item_rows - 1) / ip.item_rows;
  for (unsigned int k = 0; k < own; ++k, ++at) {
    const int base = r0 + (static_cast<int>(k) / per_window) * kC3pWindow;
    const int first = base + (static_cast<int>(k) % per_window) * ip.item_rows;
    const int end = min(first + ip.item_rows, min(base + kC3pWindow, r0 + rows));
    if (at < ip.cap) *c3p_item(queue, at) = make_int4(tile, first, end, base);
  }
  if (static_cast<int>(blockIdx.x) == item_blocks - 1 && tid == 0) {
    queue[0] = 0u;
    queue[1] = min(carry + static_cast<unsigned int>(total), ip.cap);
  }
}

#ifndef NSM_C3C_OCC
// two waves per SIMD or more: a budget of 256 registers, with which the compiler keeps the accumulators in VGPRs (beyond it
// they go to AGPRs and every result costs a v_accvgpr_read before the fold)
// OR fold: FOUR.  The bias tuple brings the scan to 133 registers under the budget of two waves, which the compiler fills
// with hoisted constants and addresses; told that it has 128, it makes them where they are used: 128, no scratch, no AGPRs
#define NSM_C3C_OCC __attribute__((amdgpu_waves_per_eu((NSM_C3C_ORFOLD && PACKED) ? 4 : 2)))
#endif
// PACKED: the scan reads its A fragments from `lpacked` (c3c_pack_left_kernel's rows of the whole left table); the drain
// reads the raw lhist rows either way.  Without it `lpacked` is not read.
// PERSIST (the packed scan's launch, NSM_C3C_PERSIST): the grid is a fixed number of waves that pull work items from the list
// that c3p_prepass_kernel made, instead of one wave per (right tile, left chunk).  The list and the queue's words stand in
// FRONT of the packed rows, at fixed offsets from `lpacked` (c3p_queue, c3p_item): no argument more, and no pointer more for
// the scan to hold in scalar registers, of which it has none to spare.
template <int NT, int CAP, bool PACKED, bool PERSIST = false>
__global__ __launch_bounds__(kBlock) NSM_C3C_OCC void indel_raw_coarse_kernel(
    const uint8_t* __restrict__ lcodes, const int32_t* __restrict__ llen, const int32_t* __restrict__ lstart,
    const int32_t* __restrict__ lorig, const uint32_t* __restrict__ lhist, const uint8_t* __restrict__ rcodes,
    const int32_t* __restrict__ rlen, const int32_t* __restrict__ rorig, const uint32_t* __restrict__ rhist,
    nsm_hit* __restrict__ hits, unsigned long long* __restrict__ count, const IndelRawParams p,
    const char* __restrict__ lpacked) {
  static_assert(!PACKED || NSM_C3C_FP4, "only the FP4 scan has packed left rows");
  static_assert(!PERSIST || PACKED, "the persistent launch is the packed scan's");
  constexpr int kRights = NT * kC3cBlock;
  // the stack's invariant: a drain check leaves at most kC3cDrainAt entries (above that the drain runs, down to fewer than 64;
  // in the pipelined scan after one more tile's pushes) and at most NT x 64 are pushed before the next check, so no slot past
  // kC3cStack is written; the drain's trigger level must itself be at least 64, so that it only ever runs full passes
  static_assert(kC3cDrainAt >= kWave && kC3cDrainAt + (NT + kC3cPipeExtra) * kWave <= kC3cStack,
                "the drain is triggered above kC3cDrainAt entries and runs full passes");
  // the OR fold is the packed scan's: the grids that do not pack (c3c_pack_pays) are short runs of blocks, where the bias
  // tuple of every class and the longer chain cost more than the fold saves
  constexpr bool kOrFold = NSM_C3C_ORFOLD && PACKED;
  // CODES2: the packed scan's value tables, whose D is a multiple of 1/4: the fields hold 4 D in 11 bits
  constexpr bool kCodes2 = NSM_C3C_CODES2 && PACKED;
  constexpr int kFieldBits = kCodes2 ? 11 : 9, kFieldFrac = kCodes2 ? 2 : 0;  // a field = (D + 256 - need) << kFieldFrac
  constexpr int kFlagLo = 1 << (kFieldBits - 1), kFlagHi = kFlagLo << kFieldBits;  // the top bit of the lower and of the upper field
  static_assert(!kOrFold || (NSM_C3C_FP4 && NT % 2 == 0), "the OR fold puts tiles 2 p and 2 p + 1 of the FP4 scan on one accumulator");
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
  unsigned long long* s_stack = s_mem;
  uint32_t* s_rh = reinterpret_cast<uint32_t*>(s_stack + kWavesPerBlock * kC3cStack);
  uint8_t* s_rl = reinterpret_cast<uint8_t*>(s_rh + kWavesPerBlock * 8 * kRights);
  uint8_t* s_lcsmin = s_rl + kWavesPerBlock * kRights;
  for (int t = threadIdx.x; t < 132; t += kBlock) s_lcsmin[t] = p.lcsmin[t];
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int col = lane & (kC3cBlock - 1);  // the lane's left row of a block (A) and right string of a tile (B, C)
  const int half = lane >> 5;              // ... and its 16 buckets of the 32
  // the wave's first right string.  PERSIST: that of the tile of the item it is scanning (wave-uniform, like all item state)
  int j0 = (blockIdx.x * kWavesPerBlock + wave) * kRights;
  if (!PERSIST && j0 >= p.n_right) return;
  // the lane again, opaque: what is used once per length class or behind a drain (the column, the half) is worked out from it
  // THERE, one instruction, and holds no register across the scan, which has none to spare at four waves per SIMD
  auto lane_again = [&]() -> int {
    int l = lane;
    asm volatile("" : "+v"(l));
    return l;
  };
#if NSM_C3C_EARLY_OUT
  // A wave whose right strings fit no length class of its chunk has nothing to scan: it leaves before it builds its LDS copy
  // and its B fragments.  For a right string of lb > 0 units the left lengths that fit, min(la, lb) >= lcsmin[la + lb], are an
  // interval around lb (a step of la towards lb adds one to min(la, lb) or takes one from la + lb, and lcsmin grows by at
  // most one per unit of la + lb), so the class nearest to lb decides: the chunk's lengths are llen[i1 - 1] .. llen[i0].
  // (Where empty strings score, zero_need == 0, an empty row fits everything: no wave leaves.)
  // (PERSIST: the item list holds no such pair of a tile and rows: the same argument, made once per tile by the pre-pass.)
  if (!PERSIST && p.zero_need != 0) {
    const int ie = blockIdx.y * p.rows_per_chunk;
    const int la_hi = llen[ie], la_lo = llen[min(p.n_left, ie + p.rows_per_chunk) - 1];
    bool fits = false;
#pragma unroll
    for (int k = 0; k < (kRights + kWave - 1) / kWave; ++k) {
      const int j = j0 + k * kWave + lane;
      if (k * kWave + lane < kRights && j < p.n_right) {
        const int lb = rlen[j];
        const int la = min(max(lb, la_lo), la_hi);
        const int nd = (la == 0 || lb == 0) ? p.zero_need : static_cast<int>(s_lcsmin[la + lb]);
        fits = fits || min(la, lb) >= nd;
      }
    }
    if (!__any(fits)) return;
  }
#endif
  unsigned long long* stack = s_stack + wave * kC3cStack;
  uint32_t* rh_lds = s_rh + wave * 8 * kRights;  // [q][right]
  uint8_t* rl_lds = s_rl + wave * kRights;

  // What outlives a work item of the persistent scan stands here, in front of the item loop; without PERSIST the loop's body
  // runs once and is the kernel of before.
  //   valid, bfrag, bscales   the right set-up, made again only where the next item is of another tile (other_tile)
  //   q_cnt                   entries on the stack (wave-uniform)
  //   [ifirst, i1), i0        the rows the wave scans, and the row that stack entries and 32-bit offsets count from: the
  //                           chunk's first row, ifirst == i0; PERSIST: the item's rows and its base, the first row of its window
  //                           of 2^15 rows -- items of one window share it, so the stack outlives them
  //   [it_cur, it_end)        PERSIST: the range of consecutive items that the wave has pulled and not yet scanned
  bool valid[NT];
  c3c_v4i bfrag[NT][NSM_C3C_FP4 ? 2 : CAP];
  uint32_t bscales = 0u;
  int q_cnt = 0;
  int i0 = 0, ifirst = 0, i1 = 0;
  int it_cur = 0, it_end = 0;
  bool other_tile = true;
  // PERSIST: the wave's next work item, at the head of the item loop.  The list is in tile-major order and a pull takes a
  // RANGE of consecutive items with one returning atomic add on the head; the queue's word 1 is the item count.  Guided
  // sizing: half of what a plain read of the head says is left, divided among the waves, at least one -- a stale read only
  // changes the grain, and the range is clipped to the count.  No wave waits for another: a wave whose pull starts at or past
  // the count is done (its stack is empty: the end of the loop's body sees to that), and the result does not depend on how
  // many waves run, or when.  Consecutive items are mostly of one tile and one window, so a wave usually keeps its right
  // set-up and its stack.
  if constexpr (PERSIST) j0 = -1;  // (no tile yet: the first item sets the wave up)
  do {
    if constexpr (PERSIST) {
      unsigned int* queue = c3p_queue(lpacked);
      if (it_cur >= it_end) {
        // (the count is read at a pull, not kept: a pull is rare and the scan has no scalar register to spare)
        const unsigned int n_items = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(queue[1])));
        unsigned int start = 0u, grain = 0u;
        if (lane == 0) {
          const unsigned int seen = *reinterpret_cast<volatile unsigned int*>(queue);
          const unsigned int left = seen < n_items ? n_items - seen : 0u;
          grain = max(1u, left / (2u * gridDim.x * kWavesPerBlock));
          start = atomicAdd(queue, grain);
        }
        // (unsigned: the head runs past the count by a grain per wave that finds the list empty)
        const unsigned int s = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(start)));
        const unsigned int g = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(grain)));
        if (s >= n_items) return;
        it_cur = static_cast<int>(s);
        it_end = static_cast<int>(min(s + g, n_items));
      }
      const int4 it = *c3p_item(queue, static_cast<unsigned int>(it_cur++));
      const int j_it = __builtin_amdgcn_readfirstlane(it.x) * kRights;
      other_tile = j_it != j0;
      j0 = j_it;
      ifirst = __builtin_amdgcn_readfirstlane(it.y);
      i1 = __builtin_amdgcn_readfirstlane(it.z);
      i0 = __builtin_amdgcn_readfirstlane(it.w);
    }
    // the wave's copy of the right fine histograms and lengths (the drain's), two strings per lane
    if (!PERSIST || other_tile) {
      // (PERSIST: the lane, opaque: the addresses of a tile's set-up are worked out here and hold no register across the scan)
      int ln = lane;
      if constexpr (PERSIST) ln = lane_again();
#pragma unroll
      for (int k = 0; k < (kRights + kWave - 1) / kWave; ++k) {
        const int rl = k * kWave + ln;
        if (rl < kRights) {
          const int j = j0 + rl;
          const int jcl = j < p.n_right ? j : p.n_right - 1;
          const uint4* fp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jcl) * 8);
          const uint4 f0 = fp[0], f1 = fp[1];
          uint32_t* dst = rh_lds + rl;
          dst[0 * kRights] = f0.x; dst[1 * kRights] = f0.y; dst[2 * kRights] = f0.z; dst[3 * kRights] = f0.w;
          dst[4 * kRights] = f1.x; dst[5 * kRights] = f1.y; dst[6 * kRights] = f1.z; dst[7 * kRights] = f1.w;
          rl_lds[rl] = static_cast<uint8_t>(j < p.n_right ? rlen[jcl] : 0);
        }
      }
    }
    // the B fragments: lane = right string col of tile t, buckets 16 half .. + 15; rows that do not exist are zero.  They are
    // made from global memory here, beside the loads of the LDS copy, and AGAIN from that copy behind every drain between the
    // tiles: the drain has the loads of eight rows per lane in flight, and 48 registers of fragments alive across it would not
    // leave room for that at four waves per SIMD
#if NSM_C3C_FP4
    // FP4: two fragments a tile, and the tiles' scale bytes (E8M0, 0x7f + k) in one register, tile t in byte t, for op_sel.  A
    // string's scale is that of ALL its 32 buckets, so a lane reads both halves of its string here (one cache line) and both of
    // the string's lanes get the same byte; behind a drain the words come from the LDS copy and the scales are still here
    // OR fold: an even tile's results go to the accumulator's upper field, so its scale bytes are 0x7f + 9 and 0x7f + 9 + k.
    // The slots 1 and 2 then need a scale too, the same in every lane: bscales1, bytes 0x88 and 0x7f in turn
    // CODES2: 4 D in 11-bit fields: 0x7f + 13 and 0x7f + 2
    auto scale_base = [](int t) -> uint32_t {
      return kOrFold ? 0x7fu + static_cast<uint32_t>(kFieldFrac + (t % 2 == 0 ? kFieldBits : 0)) : 0x7fu;
    };
    uint32_t bscales1 = 0u;
    if constexpr (kOrFold) {
#pragma unroll
      for (int t = 0; t < NT; ++t) bscales1 |= scale_base(t) << (8 * t);
      asm volatile("" : "+v"(bscales1));  // (one register for the whole scan: not a v_mov in front of every MFMA)
    }
    // the two fragments of tile t from the lane's four words: one branch a tile, and only a string with a scale takes the
    // byte-by-byte form
    auto code_tile = [&](int t, const uint4& f, int k) __attribute__((always_inline)) {
      const uint32_t ws[4] = {f.x, f.y, f.z, f.w};
      if (k == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int m1, m2;
          if constexpr (kCodes2)
            c3c_codes2_right_k0(ws[q], m1, m2);
          else
            c3c_fp4_right_k0(ws[q], m1, m2);
          bfrag[t][0][q] = m1;
          bfrag[t][1][q] = m2;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int m1, m2;
          if constexpr (kCodes2)
            c3c_codes2_right_scaled(ws[q], k, m1, m2);
          else
            c3c_fp4_right_scaled(ws[q], k, m1, m2);
          bfrag[t][0][q] = m1;
          bfrag[t][1][q] = m2;
        }
      }
    };
    if (!PERSIST || other_tile) {
      bscales = 0u;
      // (PERSIST: the column and the half from the lane, here: what the set-up of a tile needs holds no register across the scan)
      int col_r = col, half_r = half;
      if constexpr (PERSIST) {
        const int l = lane_again();
        col_r = l & (kC3cBlock - 1);
        half_r = l >> 5;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int j = j0 + t * kC3cBlock + col_r;
        valid[t] = j < p.n_right;
        const int jcl = valid[t] ? j : p.n_right - 1;
        const uint4* fp = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jcl) * 8);
        const uint4 f0 = fp[0], f1 = fp[1];
        const int k = c3c_fp4_scale(f0, f1);
        bscales |= (scale_base(t) + static_cast<uint32_t>(k)) << (8 * t);
        uint4 f = half_r ? f1 : f0;
        if (!valid[t]) f = make_uint4(0u, 0u, 0u, 0u);
        code_tile(t, f, k);
      }
    }
    auto make_bfrag = [&]() __attribute__((always_inline)) {
      const int l = lane_again();
      const uint32_t* rp0 = rh_lds + (4 * (l >> 5)) * kRights + (l & (kC3cBlock - 1));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint32_t* rp = rp0 + t * kC3cBlock;
        const int k = static_cast<int>(((bscales >> (8 * t)) & 0xffu) - scale_base(t));
        uint4 f = make_uint4(rp[0], rp[kRights], rp[2 * kRights], rp[3 * kRights]);
        if (!valid[t]) f = make_uint4(0u, 0u, 0u, 0u);
        code_tile(t, f, k);
      }
    };
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#else
    auto code_b = [&](int t, int q, uint32_t fw) {
      const uint32_t full = c3c_ge64(fw, CAP);  // the last slot: 64 [r >= CAP]
#pragma unroll
      for (int s = 0; s < CAP - 1; ++s)  // [r >= s + 1] - [r >= CAP] (the second implies the first: the xor is the difference)
        bfrag[t][s][q] = static_cast<int>((c3c_ge64(fw, s + 1) ^ full) >> 6);
      bfrag[t][CAP - 1][q] = static_cast<int>(full);
    };
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int j = j0 + t * kC3cBlock + col;
      valid[t] = j < p.n_right;
      const int jcl = valid[t] ? j : p.n_right - 1;
      uint4 f = reinterpret_cast<const uint4*>(rhist + static_cast<size_t>(jcl) * 8)[half];
      if (!valid[t]) f = make_uint4(0u, 0u, 0u, 0u);
      code_b(t, 0, f.x); code_b(t, 1, f.y); code_b(t, 2, f.z); code_b(t, 3, f.w);
    }
    auto make_bfrag = [&]() {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint32_t* rp = rh_lds + (4 * half) * kRights + t * kC3cBlock + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) code_b(t, q, valid[t] ? rp[q * kRights] : 0u);
      }
    };
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
    if constexpr (!PERSIST) {
      i0 = ifirst = blockIdx.y * p.rows_per_chunk;
      i1 = min(p.n_left, i0 + p.rows_per_chunk);
    }

    auto need_of = [&](int la, int lb) -> int { return (la == 0 || lb == 0) ? p.zero_need : static_cast<int>(s_lcsmin[la + lb]); };

    // a left row's bytes as a 32-bit offset from the chunk's first row (a chunk has at most 2^15 rows of 32 bytes)
    const char* chunk = reinterpret_cast<const char*>(lhist + static_cast<size_t>(i0) * 8);
    // ... and a packed row's from the chunk's first packed row (the scan's; the drain reads `chunk`)
    const char* pchunk = PACKED ? lpacked + static_cast<size_t>(i0) * kC3cPackedRow : nullptr;

    // pop up to 64 entries and test their rows, a ROW per lane: in quarter s of the pass the four lanes 4 u .. 4 u + 3 have entry
    // 16 s + u, lane 4 u + m its rows 8 g + 4 eh + m, g = 0 .. 3 (eh = the entry's lane half of the scan; the C layout of the
    // 32x32 MFMA).  So the four lanes of an entry read 128 contiguous bytes of lhist with each load -- with an entry per lane
    // (16 rows each) every lane of a load was in a cache line of its own, and the pass was bound by that: DESIGN 4.3 step 10.
    // (always_inline, here and on drain_full: with the FP4 set-up the compiler stopped inlining the drain at its call sites, and
    // a lambda that is called keeps what it captures by reference -- the kernel's parameters among it -- in scratch memory.  The
    // i8 build inlined them by itself: its code, 124 VGPRs and no scratch, is what it was without the attribute)
    auto drain_pass = [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int n = min(q_cnt, kWave);
      const int base = q_cnt - n;
      q_cnt = base;  // (no entry goes back; nothing is pushed before the pass ends, so the slots [base, base + n) stay readable)
#ifdef NSM_C3C_X_NODRAIN  // (timing experiments: the entries are dropped)
      return;
#endif
      const int m = lane & 3;
      // bit 4 s + g of the lane's mask = [row 8 g + 4 eh + m of entry 16 s + (lane >> 2) goes on to the LCS]: the verdicts are
      // shifted in from below, the highest quarter and g = 3 first.  The quarters are turns of a loop that is NOT unrolled, and a
      // quarter without entries is left out (most waves only ever drain a short stack, at their end).  The eight loads of a
      // lane's four rows need the entry alone, so they are issued first, and the right string is read while they are under way:
      // a quarter pays one memory round trip, and 32 registers hold the rows, no more (two quarters in flight: 153 registers)
      uint32_t mask = 0;
#pragma nounroll
      for (int s = (n - 1) >> 4; s >= 0; --s) {
        const int e = 16 * s + (lane >> 2);
        const bool active = e < n;
        const unsigned long long ent = stack[base + (active ? e : 0)];
        const int n_rows = active ? static_cast<int>(static_cast<uint32_t>(ent)) : 0;  // 1 .. 32 rows of the block exist
        const uint32_t ehi = static_cast<uint32_t>(ent >> 32);
        const uint32_t ib_rel = active ? ehi >> 15 : 0u;  // the block's first row, from the chunk's
        // rows at or past the entry's row count read the block's last row, as the scan did, and their verdict is dropped:
        // the repeated row must not be reported again
        const int r0 = 4 * static_cast<int>((ehi >> 5) & 1u) + m;
        const uint32_t last_r = static_cast<uint32_t>(max(n_rows, 1) - 1);
        uint4 w0[4], w1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint4* lp = reinterpret_cast<const uint4*>(chunk + (ib_rel + min(static_cast<uint32_t>(r0 + 8 * g), last_r)) * 32u);
          w0[g] = lp[0];
          w1[g] = lp[1];
        }
        // the right string: its 32-bucket histogram and its length from the wave's copy, once for the lane's four rows
        const int la = static_cast<int>((ehi >> 8) & 127u);
        const int tl = static_cast<int>((ehi >> 6) & 3u) * kC3cBlock + static_cast<int>(ehi & 31u);
        const int lb = rl_lds[tl];
        uint32_t rq[8];
        {
          const uint32_t* rp = rh_lds + tl;
#pragma unroll
          for (int q = 0; q < 8; ++q) rq[q] = rp[q * kRights];
        }
        const int nd = need_of(la, lb);
        // L1 <= la + lb - 2 need as the SIGN of L1 - (la + lb - 2 need) - 1: the v_sad_u8 chain starts from the negated budget
        // (L1 <= 128, the budget is -1 .. 128; -1 where the lengths alone rule the pair out: then the chain starts from 0)
        const int budget = (active && min(la, lb) >= nd) ? la + lb - 2 * nd : -1;
        const uint32_t sad0 = ~static_cast<uint32_t>(budget);
#pragma unroll
        for (int g = 3; g >= 0; --g) {
          uint32_t l1 = sad0;
          l1 = __builtin_amdgcn_sad_u8(w0[g].x, rq[0], l1);
          l1 = __builtin_amdgcn_sad_u8(w0[g].y, rq[1], l1);
          l1 = __builtin_amdgcn_sad_u8(w0[g].z, rq[2], l1);
          l1 = __builtin_amdgcn_sad_u8(w0[g].w, rq[3], l1);
          l1 = __builtin_amdgcn_sad_u8(w1[g].x, rq[4], l1);
          l1 = __builtin_amdgcn_sad_u8(w1[g].y, rq[5], l1);
          l1 = __builtin_amdgcn_sad_u8(w1[g].z, rq[6], l1);
          l1 = __builtin_amdgcn_sad_u8(w1[g].w, rq[7], l1);
          if (r0 + 8 * g >= n_rows) l1 = 0u;
          mask = __builtin_amdgcn_alignbit(mask, l1, 31);
        }
      }
      // the pairs that remain, one after the other on the scalar unit
#ifdef NSM_C3C_X_NOLCS  // (timing experiments)
      mask = 0u;
#endif
#ifdef NSM_C3C_X_FINEONLY  // (timing experiments: the 32-bucket test runs, nobody passes -- not known at compile time)
      mask = p.n_left < 0 ? mask : 0u;
#endif
      // Each pair is two 64-byte loads and the scalar chain of raw_lcs_units, which stops early for most pairs (the pair's need
      // goes with it).  The pairs are walked lane by lane (the lowest lane of the ballot leads), a lane's from its highest bit
      // down: `cur` holds the leader's bits that are left, on the scalar unit, and a pair's entry is read again from the stack
      // (one address for the whole wave).  NSM_C3C_LCS_PREFETCH: the rows of the NEXT surviving pair are requested before the
      // current pair's chain runs, whether that chain stops early or not.
      unsigned long long todo = __ballot(mask != 0u);  // lanes whose pairs have not begun
      uint32_t cur = 0u;
      int leader = 0, row_s = 0, j_n = 0, la_n = 0, lb_n = 0;
      auto next_pair = [&]() -> bool {  // (wave-uniform) the next pair: left row, right row and the two lengths
        if (cur == 0u) {
          if (todo == 0ull) return false;
          leader = __builtin_ctzll(todo);
          todo &= todo - 1ull;
          cur = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mask), leader));
        }
        const int pos = 31 - __builtin_clz(cur);  // bit 4 s + g of lane 4 u + m
        cur &= ~(1u << pos);
        const uint32_t ehi = static_cast<uint32_t>(
            __builtin_amdgcn_readfirstlane(static_cast<int>(stack[base + 16 * (pos >> 2) + (leader >> 2)] >> 32)));
        const int tl = static_cast<int>((ehi >> 6) & 3u) * kC3cBlock + static_cast<int>(ehi & 31u);
        row_s = i0 + static_cast<int>(ehi >> 15) + 8 * (pos & 3) + 4 * static_cast<int>((ehi >> 5) & 1u) + (leader & 3);
        j_n = j0 + tl;
        la_n = static_cast<int>((ehi >> 8) & 127u);
        lb_n = __builtin_amdgcn_readfirstlane(static_cast<int>(rl_lds[tl]));
        return true;
      };
      auto row_units = [&](uint32_t& lc, uint32_t& rc) {
        lc = lcodes[static_cast<size_t>(row_s) * 64 + lane];
        rc = rcodes[static_cast<size_t>(j_n) * 64 + lane];
      };
      uint32_t lc_next = 0, rc_next = 0;
      bool have = next_pair();
      if (NSM_C3C_LCS_PREFETCH && have) row_units(lc_next, rc_next);
      while (have) {
        const int row_c = row_s, j_s = j_n, la_s = la_n, lb_s = lb_n;
        const int need_s = need_of(la_s, lb_s);
        uint32_t lc = lc_next, rc = rc_next;
        if (!NSM_C3C_LCS_PREFETCH) row_units(lc, rc);
        have = next_pair();
        if (NSM_C3C_LCS_PREFETCH && have) row_units(lc_next, rc_next);
        const int lcs = raw_lcs_units(lc, la_s, rc, lb_s, need_s, lane);
#ifdef NSM_C3C_X_COUNTLCS  // (experiments: one record per LCS call)
        if (lane == 0)
#else
        if (lcs >= need_s && lane == 0)
#endif
          emit_hit(hits, p.cap, count, indel_score(la_s, lb_s, lcs), lorig[row_c], rorig[j_s]);
      }
    };
    // the drain between the tiles of the scan: full passes only (the rest waits for more), then the B fragments again
    auto drain_full = [&]() __attribute__((always_inline)) {
      while (q_cnt >= kWave) drain_pass();
      make_bfrag();
    };

    // rows are sorted by length (descending): rows of length 64 - c are [lstart[c], lstart[c + 1])
    const int c_first = 64 - llen[ifirst];
    const int c_last = 64 - llen[i1 - 1];
    uint32_t lane_off = static_cast<uint32_t>(col * 32 + half * 16);
    if constexpr (PERSIST) {
      const int l = lane_again();
      lane_off = static_cast<uint32_t>((l & (kC3cBlock - 1)) * 32 + (l >> 5) * 16);
    }
    for (int c = c_first; c <= c_last; ++c) {
      const int a = max(ifirst, lstart[c]);
      const int b = min(i1, lstart[c + 1]);
      if (a >= b) continue;
      const int la = 64 - c;
      // per tile: the lane's right string can only hit a row of this class if D >= need (kNever: it cannot fit)
      // i8: 64 need - 1, "D' > nm1" is the fold's test.  FP4: the bits of the f32 need - 1/2 (D is a multiple of 1/2, exact in
      // f32, and never negative: its bits compare as integers, and those of -1/2, need = 0, are below them all)
      // OR fold: ONE bias for all the wave's tile pairs, so the lane's need of the upper field is the SMALLEST of its even
      // tiles' and that of the lower field the smallest of its odd tiles'.  A lane whose columns differ in need (the wave's 128
      // right strings straddle a length boundary) pushes a few entries too many, and the drain tests every pair by its own need
      int need2[2] = {static_cast<int>(kNever), static_cast<int>(kNever)};
      int nm1[NT];
      bool some = false;
      const int l_c = lane_again();
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int lb = rl_lds[t * kC3cBlock + (l_c & (kC3cBlock - 1))];  // (from the wave's copy: no register holds it across the classes)
        const int nd = valid[t] ? need_of(la, lb) : static_cast<int>(kNever);
        const bool fits = min(la, lb) >= nd;  // exact length filter: LCS <= min(la, lb)
        some = some || fits;
#if NSM_C3C_FP4
        if constexpr (kOrFold)
          need2[t & 1] = min(need2[t & 1], fits ? nd : static_cast<int>(kNever));  // (fits: nd <= min(la, lb) <= 64)
        else
          // (CODES2: D is a multiple of 1/4, and D >= need is D > need - 1/4)
          nm1[t] = __float_as_int(static_cast<float>(fits ? nd : static_cast<int>(kNever)) - (kCodes2 ? 0.25f : 0.5f));  // (no D reaches kNever: D <= 128; CODES2: 162)
#else
        nm1[t] = 64 * (fits ? nd : static_cast<int>(kNever)) - 1;
#endif
      }
      if (!__any(some)) continue;
      // OR fold: the C operand of a chain's first MFMA: 2^23 + (256 - need_hi) 2^9 + (256 - need_lo) in all 16 registers.  The chain
      // adds 2^9 D_hi + D_lo, D <= 128: an integer in [2^23, 2^24), exact in f32, whose mantissa bits ARE the integer.  Field
      // D + 256 - need <= 384 < 512 does not carry, and its bit 8 is set exactly where D >= need (need = kNever: the field
      // is at most 129; need = 0: always set)
      // (made here and again behind a drain between the tiles, like the B fragments: the drain needs the registers)
      c3c_v16f bias;
      // CODES2: 2^23 + (1024 - 4 need_hi) 2^11 + (1024 - 4 need_lo), the chain adds 2^11 (4 D_hi) + 4 D_lo, D <= 162 a multiple of
      // 1/4: every term an integer, the sum below 2^24, a field 4 D + 1024 - 4 need <= 1672 < 2048, its bit 10 = [D >= need]
      // (need = kNever: at most 4 + 648)
      const float bias1 = __int_as_float(0x4b000000 | (((256 - need2[0]) << kFieldFrac) << kFieldBits) | ((256 - need2[1]) << kFieldFrac));
      auto make_bias = [&]() {
        // (16 registers that stay across the blocks: srcC is a tuple.  The moves are written out: a splat that the compiler
        // sees is made once per class in 16 registers MORE and copied from there behind every drain)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          float x;
          asm volatile("v_mov_b32 %0, %1" : "=v"(x) : "v"(bias1));
          bias[k] = x;
        }
      };

      // the lane's 16 bytes of row i + col (the class's last row again past its end)
      // PACKED: its 32 bytes of packed row i + col, the same clamp in the packed rows' stride (a chunk has at most 2^15 rows
      // of 64 bytes: the offset stays a 32-bit value from the chunk's first packed row)
      typedef typename c3c_rows<PACKED>::type rows_t;
      const uint32_t last_off = static_cast<uint32_t>(b - 1 - i0) * (PACKED ? 64u : 32u) + static_cast<uint32_t>((l_c >> 5) * (PACKED ? 32 : 16));
      auto load_rows = [&](int i) -> rows_t {
        if constexpr (PACKED) {
          const uint32_t off = min(static_cast<uint32_t>(i - i0) * 64u + 2u * lane_off, last_off);
          const c3c_v4i* pp = reinterpret_cast<const c3c_v4i*>(pchunk + off);
          return c3c_packed_rows{pp[0], pp[1]};
        } else {
          const uint32_t off = min(static_cast<uint32_t>(i - i0) * 32u + lane_off, last_off);
          return *reinterpret_cast<const uint4*>(chunk + off);
        }
      };
#if NSM_C3C_FP4
      // the A fragments of a block: two, of two indicator slots each; the loaded words are no operand.  PACKED: the loaded
      // words ARE the two fragments, nothing is made and the chains read the loaded set
      typedef c3c_v16f acc_t;
      c3c_v4i afrag[2];
      auto make_afrag = [&](const rows_t& w) {
        if constexpr (!PACKED) {
          const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            int m1, m2;
            c3c_fp4_left(ws[q], m1, m2);
            afrag[0][q] = m1;
            afrag[1][q] = m2;
          }
        }
      };
      // a unit of the scan is a tile: its two chained MFMAs of the current block, the first in the unscaled form.  OR fold: a
      // tile PAIR, four chained MFMAs against tiles 2 u (scaled by 2^9: the upper field) and 2 u + 1 on the bias, all in the
      // scaled form (the unscaled one cannot carry 2^9)
      constexpr int NU = kOrFold ? NT / 2 : NT;
      auto chain = [&](int u, const rows_t& w) -> acc_t {
        if constexpr (kOrFold) {
          acc_t acc = c3c_fp4_mfma2(w.m1, bfrag[2 * u][0], bias, static_cast<int>(bscales1), 2 * u);
          acc = c3c_fp4_mfma2(w.m2, bfrag[2 * u][1], acc, static_cast<int>(bscales), 2 * u);
          acc = c3c_fp4_mfma2(w.m1, bfrag[2 * u + 1][0], acc, static_cast<int>(bscales1), 2 * u + 1);
          return c3c_fp4_mfma2(w.m2, bfrag[2 * u + 1][1], acc, static_cast<int>(bscales), 2 * u + 1);
        } else if constexpr (PACKED) {
          return c3c_fp4_mfma2(w.m2, bfrag[u][1], c3c_fp4_mfma1(w.m1, bfrag[u][0]), static_cast<int>(bscales), u);
        } else {
          return c3c_fp4_mfma2(afrag[1], bfrag[u][1], c3c_fp4_mfma1(afrag[0], bfrag[u][0]), static_cast<int>(bscales), u);
        }
      };
      // no result is negative, so the f32 bit patterns order as integers do: the fold is the i8 scan's, v_max3_i32 (fmaxf
      // would canonicalise its first two operands, two instructions more).  OR fold: "some row passes" is a flag bit: OR the 16
      // registers (seven v_or3_b32) and mask the two flags (v_bitop3_b32)
      auto fold = [&](const acc_t& acc) -> int {
        const c3c_v16i bits = __builtin_bit_cast(c3c_v16i, acc);
        if constexpr (kOrFold) {
          int top = bits[0] | bits[1] | bits[2];
#pragma unroll
          for (int k = 3; k < 15; k += 2) top = top | bits[k] | bits[k + 1];
          return (top | bits[15]) & (kFlagHi | kFlagLo);
        } else {
          int top = max(max(bits[0], bits[1]), bits[2]);
#pragma unroll
          for (int k = 3; k < 15; k += 2) top = max(max(top, bits[k]), bits[k + 1]);
          return max(top, bits[15]);
        }
      };
#else
      typedef c3c_v16i acc_t;
      constexpr int NU = NT;
      // the A fragments of a block: CAP - 1 indicator slots, two instructions a word; the last slot is the loaded word itself
      c3c_v4i afrag[CAP - 1];
      auto make_afrag = [&](const uint4& w) {
#pragma unroll
        for (int s = 0; s < CAP - 1; ++s) {
          afrag[s].x = static_cast<int>(c3c_ge64(w.x, s + 1)); afrag[s].y = static_cast<int>(c3c_ge64(w.y, s + 1));
          afrag[s].z = static_cast<int>(c3c_ge64(w.z, s + 1)); afrag[s].w = static_cast<int>(c3c_ge64(w.w, s + 1));
        }
      };
      // the CAP chained MFMAs of the current block (its loaded words: w) against tile t
      auto chain = [&](int t, const uint4& w) -> c3c_v16i {
        c3c_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < CAP - 1; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[s], bfrag[t][s], acc, 0, 0, 0);
        const c3c_v4i last = {static_cast<int>(w.x), static_cast<int>(w.y), static_cast<int>(w.z), static_cast<int>(w.w)};
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(last, bfrag[t][CAP - 1], acc, 0, 0, 0);
      };
      auto fold = [&](const c3c_v16i& acc) -> int {
        int top = max(max(acc[0], acc[1]), acc[2]);
#pragma unroll
        for (int k = 3; k < 15; k += 2) top = max(max(top, acc[k]), acc[k + 1]);
        return max(top, acc[15]);
      };
#endif
      // compare and push of tile t of the block at row i: the lanes whose folded result passes push one entry, at most 64 a
      // tile.  Which of a lane's 16 rows passed is not worked out here: the accumulator is dead after the fold, and the drain's
      // exact test decides every row by itself
      auto push = [&](bool ps, unsigned long long m, int t, int i) {
        if (m == 0ull) return;
#ifdef NSM_C3C_X_COUNTPUSH  // (experiments, with NSM_C3C_X_NOLCS: the launch's count is the number of entries pushed)
        if (lane == 0) atomicAdd(count, static_cast<unsigned long long>(__popcll(m)));
#endif
        if (ps) {
          const int slot = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), static_cast<uint32_t>(q_cnt)));
          // (the wave-uniform part first: one v_or at the push instead of a register per tile)
          const uint32_t hi = (static_cast<uint32_t>(i - i0) << 15) | (static_cast<uint32_t>(la) << 8) | (static_cast<uint32_t>(t) << 6);
          uint32_t el = static_cast<uint32_t>(lane);
          asm volatile("" : "+v"(el));  // (opaque: or-ed in here, not kept in a register per tile and class)
          // the rows of the block that exist (wave-uniform): it is short only as the last of its class in the chunk
          const uint32_t n_rows = static_cast<uint32_t>(min(kC3cBlock, b - i));
          stack[slot] = (static_cast<unsigned long long>(hi | el) << 32) | n_rows;
        }
        q_cnt += __popcll(m);
      };
      // OR fold: one branch a tile pair; where it is taken a ballot per flag, bit 17 for tile 2 u and bit 8 for tile 2 u + 1, in
      // the same entry format -- up to 128 entries a pair
      auto finish = [&](int top, int u, int i) {
        if constexpr (kOrFold) {
          if (__ballot(top != 0) == 0ull) return;
          // (a column that does not exist has the flag of the lane's other tile of its parity: with need = 0 that one passes
          // everything, and the drain would take the missing string for an empty one)
          const bool hi = (top & kFlagHi) != 0 && valid[2 * u], lo = (top & kFlagLo) != 0 && valid[2 * u + 1];
          push(hi, __ballot(hi), 2 * u, i);
          push(lo, __ballot(lo), 2 * u + 1, i);
        } else {
          const bool ps = top > nm1[u];
          push(ps, __ballot(ps), u, i);
        }
      };
#if NSM_C3C_PIPE
      // software pipeline over the tiles and the blocks of the class: acc[t & 1] holds tile t, and the chain of the tile after
      // (tile 0 of the next block after a block's last, with that block's A fragments) is issued around the fold and before
      // the branch and the push of tile t, so that the matrix pipe works under the wave's own epilogue.  Filled here, empty
      // again at the end of the class.
      // (units: tiles, or the tile pairs of the OR fold)
      static_assert(NU % 2 == 0, "unit 0 of the next block takes the accumulator of unit NU: NU must be even (or NSM_C3C_PIPE=0)");
      acc_t acc[2];
      // one block at row i.  wc: the block's loaded words, its last A slot, which the chains read until the block's last tile
      // is issued; wn: those of the block after, loaded a block ahead.  The load of the block after that goes to wc, so the
      // two register sets change places from block to block and no word is copied.
      auto block = [&](int i, rows_t& wc, rows_t& wn) __attribute__((always_inline)) -> bool {
        const bool more = i + kC3cBlock < b;
        // the drain check sits in front of a block's LAST unit: at most NT tiles, NT x 64 entries, between two checks.  Where
        // the drain has to run, the pipeline is emptied first (one more unit's entries: kC3cPipeExtra x 64 slots of kC3cStack)
        // and the block returns true: the class loop below drains and starts again behind this block, so that no accumulator,
        // no A fragment, no loaded word and no bias lives across the drain.
        bool flush = false;
#pragma unroll
        for (int t = 0; t < NU; ++t) {
          if (t + 1 < NU) {
            acc[(t + 1) & 1] = chain(t + 1, wc);
          } else {
            flush = q_cnt > kC3cDrainAt;
            // OR fold: the first chain of the block after is issued whether that block exists and runs or not (at the end of a
            // run its result is dropped: the words are the class's last rows again, or this block's).  A pair is every other
            // unit, and behind a branch the chain would stand in a basic block of its own, where no fold goes between its MFMAs
            if (kOrFold || (more && !flush)) {
              make_afrag(wn);
              // (PACKED: the wait for wn, loaded a block ago, stands HERE and not behind the next load, which it would wait for too)
              if constexpr (PACKED) asm volatile("" : "+v"(wn.m1), "+v"(wn.m2));
              if (i + 2 * kC3cBlock < b) wc = load_rows(i + 2 * kC3cBlock);
              acc[0] = chain(0, wn);
            }
          }
          // the fold of tile t goes BETWEEN the MFMAs of the chain (MFMA, 4 VALU, MFMA, 4 VALU, MFMA): a wave issues in order and
          // a chained MFMA waits for the one before it, so a fold behind the whole chain would start 64 cycles later.  The
          // branch ends the scheduling region: the chain cannot sink below it
          const int top = fold(acc[t & 1]);
#if NSM_C3C_FP4
          if constexpr (kOrFold) {
            // (four MFMAs and the fold's eight: NSM_C3C_OR_SPLIT VALU behind each of the first three, the rest behind the last)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, NSM_C3C_OR_SPLIT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, NSM_C3C_OR_SPLIT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, NSM_C3C_OR_SPLIT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8 - 3 * NSM_C3C_OR_SPLIT, 0);
          } else {
            // (two MFMAs: MFMA, NSM_C3C_FP4_SPLIT VALU, MFMA, the rest of the fold's eight behind it)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, NSM_C3C_FP4_SPLIT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8 - NSM_C3C_FP4_SPLIT, 0);
          }
          // (the chain's last MFMA would otherwise be moved behind the branch and the push, in front of its own fold)
          if (t + 1 < NU || kOrFold || (more && !flush)) asm volatile("" : "+v"(acc[(t + 1) & 1]));
#else
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#endif
          finish(top, t, i);
        }
        return flush;
      };
      // a run of blocks from row i on: to the end of the class, or to the block that decides on a drain (the next run drains
      // first; the words that were loaded ahead are loaded again, a drain is rare)
      for (int i = a; i < b;) {
        if (q_cnt > kC3cDrainAt)  // (at the start of a class too: one of a single block has no other check in front of its first units)
          drain_full();
        if constexpr (kOrFold) make_bias();
        rows_t w0 = load_rows(i);
        make_afrag(w0);
        // (once per run, outside the block loop: a run of one block never loads the second set.  PACKED: it does, the
        // class's last row by load_rows' clamp -- nothing waits for the first set before the second load is under way)
        rows_t w1;
        if constexpr (PACKED) {
          w1 = load_rows(i + kC3cBlock);
        } else {
          w1 = w0;
          if (i + kC3cBlock < b) w1 = load_rows(i + kC3cBlock);
        }
        acc[0] = chain(0, w0);
        for (;;) {
          const bool f0 = block(i, w0, w1);
          if ((i += kC3cBlock) >= b || f0) break;
          const bool f1 = block(i, w1, w0);
          if ((i += kC3cBlock) >= b || f1) break;
        }
      }
#else
      if constexpr (kOrFold) make_bias();
      rows_t w_next = load_rows(a);
      for (int i = a; i < b; i += kC3cBlock) {
        const rows_t w = w_next;
        if (i + kC3cBlock < b) w_next = load_rows(i + kC3cBlock);
        // a block pushes up to NT x 64 entries
        if (q_cnt > kC3cDrainAt)
          drain_full();
        make_afrag(w);
#pragma unroll
        for (int t = 0; t < NU; ++t) {
          const acc_t acc = chain(t, w);
          finish(fold(acc), t, i);
        }
      }
#endif
    }
    // PERSIST: the stack's entries count rows from i0 and name strings of j0's tile, so it is emptied here unless the wave's
    // next item is of the same tile and base -- also where the next item is not known yet (the range is used up: a pull
    // comes first, or the end).  Without PERSIST: the end
    bool keep = false;
    if constexpr (PERSIST) {
      if (it_cur < it_end) {
        const int4 nx = *c3p_item(c3p_queue(lpacked), static_cast<unsigned int>(it_cur));
        keep = __builtin_amdgcn_readfirstlane(nx.x) * kRights == j0 && __builtin_amdgcn_readfirstlane(nx.w) == i0;
      }
    }
    if (!keep) {
      while (q_cnt > 0) drain_pass();
    }
  } while (PERSIST);
}

}  // namespace nsm
