// Probe: the operand map, the block scale and the issue rate of the FP4 (E2M1) forms of v_mfma_f32_32x32x64_f8f6f4 on
// gfx950, and the v_perm_b32 byte table of the C3 scan's left operand (csrc/indel_raw_coarse.hpp, NSM_C3C_FP4).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/mfma_fp4_probe.hip -o tools/mfma_fp4_probe && tools/mfma_fp4_probe
// 1. map: A (32 x 64) and B (64 x 32) of exact FP4 values, A != B^T, through the unscaled form (both scale arguments literal
//    0) and through the scaled form with a B scale of 2^1 on ONE column (both of its lanes, byte 2 of the scale register,
//    picked with op_sel), all 1024 results against a host loop.  The map assumed: lane l holds row (column) l & 31 and
//    k = 32 (l >> 5) + j, j = 0 .. 31, element j in nibble j & 1 (0 = low) of byte j >> 1 of its first four registers;
//    C/D: column l & 31, row (i & 3) + 8 (i >> 2) + 4 (l >> 5) in register i.
// 2. perm: the scan's packing of four counts 0 .. 64 into the two left operand words, every count in every byte position.
// 2b. chain4: the OR-fold scan's chain of four MFMAs on one accumulator -- a bias of 2^23 + two need offsets as srcC, one
//    tile through B scales 2^9 and 2^(9 + k), the other through 2^0 and 2^k, k = 0 .. 3 by column -- against a host integer
//    loop, bit for bit.
// 2c. chain4, 11-bit fields: the same chain with the value-table codes of the packed scan (NSM_C3C_CODES2) -- FP4 values on
//    BOTH sides, products multiples of 1/4, B scales 2^13 and 2^(13 + k) for one tile, 2^2 and 2^(2 + k) for the other, a bias
//    of 2^23 + (1024 - 4 need_hi) 2^11 + (1024 - 4 need_lo) -- against a host integer loop in quarters, bit for bit.
// 3. rate: back-to-back chains, one wave per SIMD: ns per MFMA of the i8 32x32x32 form and of the two FP4 forms; and a
//    tile pair as two chains of two (zero C) against one chain of four (bias C), at one and at four waves per SIMD.
// Exit status 0 where 1, 2, 2b and 2c agree with the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static const float kFp4[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};

// a[lane][4], b[lane][4]: the operand registers; sb[lane]: the B scale register; out[kind][lane][16]
__global__ void map_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* sb, float* out) {
  const int l = threadIdx.x;
  const v8i A = {(int)a[4 * l], (int)a[4 * l + 1], (int)a[4 * l + 2], (int)a[4 * l + 3], 0, 0, 0, 0};
  const v8i B = {(int)b[4 * l], (int)b[4 * l + 1], (int)b[4 * l + 2], (int)b[4 * l + 3], 0, 0, 0, 0};
  const v16f z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const v16f plain = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, z, 4, 4, 0, 0, 0, 0);
  const v16f scaled = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, z, 4, 4, 0, 0x7f7f7f7f, 2, (int)sb[l]);
  for (int i = 0; i < 16; ++i) {
    out[l * 16 + i] = plain[i];
    out[1024 + l * 16 + i] = scaled[i];
  }
}

// the left operand words of the scan: low nibble 2.0 [c >= lo], high nibble 2.0 [c >= lo + 1], lo = 1 (m1) and 3 (m2)
__global__ void perm_kernel(const uint32_t* w, uint32_t* m1, uint32_t* m2, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t sel = (w[i] + 0x3c3c3c3cu) & 0x43434343u;
  m1[i] = __builtin_amdgcn_perm(0u, 0x44440400u, sel) & 0x44444444u;
  m2[i] = __builtin_amdgcn_perm(0u, 0x04000000u, sel) & 0x44444444u;
}

// the OR-fold scan's chain of FOUR on one accumulator: bias as srcC of the first, tile `hi` through B scales 2^9 and
// 2^(9 + k_hi), tile `lo` through 2^0 and 2^k_lo.  a[lane][8]: m1 and m2 words of the left rows; bh, bl[lane][8]: those
// of the two right tiles; s1, s2[lane]: the scale registers of the m1 and of the m2 MFMAs, tile hi in byte 0, lo in byte 1
__global__ void chain4_kernel(const uint32_t* a, const uint32_t* bh, const uint32_t* bl, const uint32_t* s1, const uint32_t* s2,
                              const float* bias, float* out) {
  const int l = threadIdx.x;
  const v8i A1 = {(int)a[8 * l], (int)a[8 * l + 1], (int)a[8 * l + 2], (int)a[8 * l + 3], 0, 0, 0, 0};
  const v8i A2 = {(int)a[8 * l + 4], (int)a[8 * l + 5], (int)a[8 * l + 6], (int)a[8 * l + 7], 0, 0, 0, 0};
  const v8i H1 = {(int)bh[8 * l], (int)bh[8 * l + 1], (int)bh[8 * l + 2], (int)bh[8 * l + 3], 0, 0, 0, 0};
  const v8i H2 = {(int)bh[8 * l + 4], (int)bh[8 * l + 5], (int)bh[8 * l + 6], (int)bh[8 * l + 7], 0, 0, 0, 0};
  const v8i L1 = {(int)bl[8 * l], (int)bl[8 * l + 1], (int)bl[8 * l + 2], (int)bl[8 * l + 3], 0, 0, 0, 0};
  const v8i L2 = {(int)bl[8 * l + 4], (int)bl[8 * l + 5], (int)bl[8 * l + 6], (int)bl[8 * l + 7], 0, 0, 0, 0};
  const float bv = bias[l];
  const v16f c = {bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv};
  const int m1 = (int)s1[l], m2 = (int)s2[l];
  v16f acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A1, H1, c, 4, 4, 0, 0x7f7f7f7f, 0, m1);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A2, H2, acc, 4, 4, 0, 0x7f7f7f7f, 0, m2);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A1, L1, acc, 4, 4, 0, 0x7f7f7f7f, 1, m1);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A2, L2, acc, 4, 4, 0, 0x7f7f7f7f, 1, m2);
  for (int i = 0; i < 16; ++i) out[l * 16 + i] = acc[i];
}

template <int KIND>
__global__ __launch_bounds__(256) void rate_kernel(float* out, int iters, int seed) {
  v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v16i acci = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int x = (int)(threadIdx.x * 0x01010101u) & 0x11111111 & seed;
  const v8i A = {x, x, x, x, 0, 0, 0, 0}, B = {x, x ^ 0x10101010, x, x, 0, 0, 0, 0};
  const v4i a4 = {x, x, x, x}, b4 = {x, x, x, x};
  const int sc = 0x7f7f7f7f + (seed & 1);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (KIND == 0) acci = __builtin_amdgcn_mfma_i32_32x32x32_i8(a4, b4, acci, 0, 0, 0);
      if (KIND == 1) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc, 4, 4, 0, 0, 0, 0);
      if (KIND == 2) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc, 4, 4, 0, 0x7f7f7f7f, 1, sc);
    }
  }
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += acc[i] + (float)acci[i];
  if (s == 12345.678f) out[threadIdx.x] = s;  // (keeps the chain)
}

// a tile PAIR: KIND 3 the two chains of two of the max-fold scan (zero C, unscaled then scaled, two accumulators), KIND 4
// the chain of four on one accumulator with the bias as srcC.  The operands are made opaque every turn, so that no MFMA
// leaves the loop; the accumulators are only named (no fold: this is the matrix pipe's time alone)
template <int KIND>
__global__ __launch_bounds__(256) void pair_rate_kernel(float* out, int iters, int seed) {
  int x = (int)(threadIdx.x * 0x01010101u) & 0x11111111 & seed;
  const float bv = 8388608.f + (float)(seed & 0xffff);
  const v16f bias = {bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv, bv};
  const v16f z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int s1 = 0x7f887f88 + (seed & 1), s2 = 0x7f887f88 + (seed & 2);
  v16f acc0 = z, acc1 = z;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      asm volatile("" : "+v"(x));
      const v8i A = {x, x, x, x, 0, 0, 0, 0}, B = {x, x ^ 0x10101010, x, x, 0, 0, 0, 0}, B2 = {x ^ 0x01010101, x, x, x, 0, 0, 0, 0};
      if (KIND == 3) {
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, z, 4, 4, 0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc0, 4, 4, 0, 0x7f7f7f7f, 0, s2);
        acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B2, z, 4, 4, 0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B2, acc1, 4, 4, 0, 0x7f7f7f7f, 1, s2);
        asm volatile("" : "+v"(acc0), "+v"(acc1));
      } else {
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, bias, 4, 4, 0, 0x7f7f7f7f, 0, s1);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc0, 4, 4, 0, 0x7f7f7f7f, 0, s2);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B2, acc0, 4, 4, 0, 0x7f7f7f7f, 1, s1);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B2, acc0, 4, 4, 0, 0x7f7f7f7f, 1, s2);
        asm volatile("" : "+v"(acc0));
      }
    }
  }
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i];
  if (s == 12345.678f) out[threadIdx.x] = s;
}

template <int KIND>
static int pair_rate(const char* name, float* d_out, int cus, int waves) {
  const int iters = 1 << 13;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL(pair_rate_kernel<KIND>, dim3(cus * waves), dim3(256), 0, 0, d_out, 64, 0x11111111);
  CHECK(hipDeviceSynchronize());
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(pair_rate_kernel<KIND>, dim3(cus * waves), dim3(256), 0, 0, d_out, iters, 0x11111111);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  printf("rate %-34s %8.3f ns per tile pair and wave (%d waves per SIMD)\n", name, ms * 1e6 / (iters * 4.0 * waves), waves);
  return 0;
}

template <int KIND>
static int rate(const char* name, float* d_out, int cus) {
  const int iters = 1 << 14;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL(rate_kernel<KIND>, dim3(cus), dim3(256), 0, 0, d_out, 64, 0x11111111);
  CHECK(hipDeviceSynchronize());
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(rate_kernel<KIND>, dim3(cus), dim3(256), 0, 0, d_out, iters, 0x11111111);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  printf("rate %-34s %8.3f ns per MFMA (one wave per SIMD, %d chained)\n", name, ms * 1e6 / (iters * 8.0), iters * 8);
  return 0;
}

int main() {
  // --- 1. the operand map
  // A[i][k] and B[k][j] as FP4 codes 0 .. 7 (no negative values: the scan has none), asymmetric
  static int Ac[32][64], Bc[64][32];
  for (int i = 0; i < 32; ++i)
    for (int k = 0; k < 64; ++k) {
      Ac[i][k] = (i * 5 + k * 3 + (k >> 4)) % 8;
      Bc[k][i] = (i * 3 + k * 7 + (i >> 3) + 1) % 8;
    }
  const int scaled_col = 21;
  std::vector<uint32_t> ha(256, 0), hb(256, 0), hs(64, 0x7f7f7f7fu);
  for (int l = 0; l < 64; ++l) {
    for (int j = 0; j < 32; ++j) {
      const int k = 32 * (l >> 5) + j, sh = 4 * (j & 7);
      ha[4 * l + (j >> 3)] |= (uint32_t)Ac[l & 31][k] << sh;
      hb[4 * l + (j >> 3)] |= (uint32_t)Bc[k][l & 31] << sh;
    }
    // bytes 0, 1, 3 of the scale register hold other scales: op_sel must pick byte 2
    hs[l] = ((l & 31) == scaled_col) ? 0x7d80797eu : 0x7e7f8280u;
  }
  uint32_t *da, *db, *ds;
  float* dout;
  CHECK(hipMalloc(&da, 1024));
  CHECK(hipMalloc(&db, 1024));
  CHECK(hipMalloc(&ds, 256));
  CHECK(hipMalloc(&dout, 2 * 1024 * sizeof(float)));
  CHECK(hipMemcpy(da, ha.data(), 1024, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, hb.data(), 1024, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ds, hs.data(), 256, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(map_kernel, dim3(1), dim3(64), 0, 0, da, db, ds, dout);
  CHECK(hipDeviceSynchronize());
  std::vector<float> hout(2048);
  CHECK(hipMemcpy(hout.data(), dout, 2048 * sizeof(float), hipMemcpyDeviceToHost));
  int bad[2] = {0, 0};
  for (int kind = 0; kind < 2; ++kind)
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 16; ++i) {
        const int col = l & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5);
        float want = 0.f;
        for (int k = 0; k < 64; ++k) want += kFp4[Ac[row][k]] * kFp4[Bc[k][col]];
        if (kind == 1 && col == scaled_col) want *= 2.f;
        const float got = hout[kind * 1024 + l * 16 + i];
        if (got != want && bad[kind]++ < 4) printf("map %s: row %d col %d: %g, host %g\n", kind ? "scaled" : "plain", row, col, got, want);
      }
  printf("map plain:  %d of 1024 differ\nmap scaled: %d of 1024 differ\n", bad[0], bad[1]);

  // --- 2. the byte table
  std::vector<uint32_t> hw;
  for (int c = 0; c <= 64; ++c)
    for (int pos = 0; pos < 4; ++pos)
      for (int nb = 0; nb < 2; ++nb) {
        uint32_t w = nb ? 0x40404040u : 0u;
        w = (w & ~(0xffu << (8 * pos))) | ((uint32_t)c << (8 * pos));
        hw.push_back(w);
      }
  const int n = (int)hw.size();
  uint32_t *dw, *dm1, *dm2;
  CHECK(hipMalloc(&dw, n * 4));
  CHECK(hipMalloc(&dm1, n * 4));
  CHECK(hipMalloc(&dm2, n * 4));
  CHECK(hipMemcpy(dw, hw.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(perm_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dw, dm1, dm2, n);
  CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> hm1(n), hm2(n);
  CHECK(hipMemcpy(hm1.data(), dm1, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hm2.data(), dm2, n * 4, hipMemcpyDeviceToHost));
  int bad_perm = 0;
  for (int i = 0; i < n; ++i) {
    uint32_t w1 = 0, w2 = 0;
    for (int pos = 0; pos < 4; ++pos) {
      const uint32_t c = (hw[i] >> (8 * pos)) & 0xffu;
      w1 |= ((c >= 1 ? 0x04u : 0u) | (c >= 2 ? 0x40u : 0u)) << (8 * pos);
      w2 |= ((c >= 3 ? 0x04u : 0u) | (c >= 4 ? 0x40u : 0u)) << (8 * pos);
    }
    if ((hm1[i] != w1 || hm2[i] != w2) && bad_perm++ < 4) printf("perm: w %08x: %08x %08x, host %08x %08x\n", hw[i], hm1[i], hm2[i], w1, w2);
  }
  printf("perm: %d of %d words differ\n", bad_perm, n);

  // --- 2b. the biased chain of four (the OR-fold scan): left indicators 2.0, right codes 0 .. 7, column c of tile hi with
  // k = c & 3 and of tile lo with k = (c >> 2) & 3, needs per column; every result against a host INTEGER loop, bit for bit
  int bad_chain = 0;
  {
    static int A4[2][32][64], B4[2][2][64][32];  // [m][row][k]; [tile][m][k][col]
    uint32_t rng = 12345u;
    auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int m = 0; m < 2; ++m)
      for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 64; ++k) {
          A4[m][i][k] = (rnd() & 1) ? 4 : 0;
          for (int t = 0; t < 2; ++t) B4[t][m][k][i] = (rnd() & 3) ? 0 : (int)(rnd() & 7);
        }
    std::vector<uint32_t> qa(512, 0), qh(512, 0), ql(512, 0), q1(64), q2(64);
    std::vector<float> qb(64);
    int nh[32], nl[32];
    for (int c = 0; c < 32; ++c) {
      nh[c] = c == 7 ? 255 : (c * 5) % 65;
      nl[c] = c == 9 ? 255 : (c * 11 + 3) % 65;
    }
    for (int l = 0; l < 64; ++l) {
      const int c = l & 31;
      for (int m = 0; m < 2; ++m)
        for (int j = 0; j < 32; ++j) {
          const int k = 32 * (l >> 5) + j, sh = 4 * (j & 7), w = 8 * l + 4 * m + (j >> 3);
          qa[w] |= (uint32_t)A4[m][c][k] << sh;
          qh[w] |= (uint32_t)B4[0][m][k][c] << sh;
          ql[w] |= (uint32_t)B4[1][m][k][c] << sh;
        }
      q1[l] = 0x55aa7f88u;  // (bytes 2 and 3 are not picked)
      q2[l] = 0xaa550000u | (uint32_t)(0x7f + ((c >> 2) & 3)) << 8 | (uint32_t)(0x88 + (c & 3));
      qb[l] = (float)((1 << 23) + (256 - nh[c]) * 512 + (256 - nl[c]));
    }
    uint32_t *ea, *eh, *el, *e1, *e2;
    float *eb, *eo;
    CHECK(hipMalloc(&ea, 2048));
    CHECK(hipMalloc(&eh, 2048));
    CHECK(hipMalloc(&el, 2048));
    CHECK(hipMalloc(&e1, 256));
    CHECK(hipMalloc(&e2, 256));
    CHECK(hipMalloc(&eb, 256));
    CHECK(hipMalloc(&eo, 4096));
    CHECK(hipMemcpy(ea, qa.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(eh, qh.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(el, ql.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(e1, q1.data(), 256, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(e2, q2.data(), 256, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(eb, qb.data(), 256, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chain4_kernel, dim3(1), dim3(64), 0, 0, ea, eh, el, e1, e2, eb, eo);
    CHECK(hipDeviceSynchronize());
    std::vector<float> qo(1024);
    CHECK(hipMemcpy(qo.data(), eo, 4096, hipMemcpyDeviceToHost));
    const int twice[8] = {0, 1, 2, 3, 4, 6, 8, 12};  // 2 x the FP4 value
    int top = 0;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 16; ++i) {
        const int col = l & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5);
        int d[2] = {0, 0};
        for (int t = 0; t < 2; ++t) {
          const int k = t ? (col >> 2) & 3 : col & 3;
          for (int m = 0; m < 2; ++m) {
            int s = 0;  // 2.0 x code / 2 = twice[code] / 2 x [indicator] x 2: an integer
            for (int kk = 0; kk < 64; ++kk) s += A4[m][row][kk] ? twice[B4[t][m][kk][col]] : 0;
            d[t] += m ? s << k : s;
          }
        }
        const int n = (1 << 23) + (256 - nh[col]) * 512 + (256 - nl[col]) + 512 * d[0] + d[1];
        top = n > top ? n : top;
        uint32_t got;
        memcpy(&got, &qo[l * 16 + i], 4);
        if (got != (0x4b000000u | (uint32_t)(n - (1 << 23))) && bad_chain++ < 4)
          printf("chain4: row %d col %d: bits %08x, host N %d (D hi %d lo %d)\n", row, col, got, n, d[0], d[1]);
      }
    if (top >= 1 << 24) { printf("chain4: the host sum leaves [2^23, 2^24)\n"); return 2; }
    printf("chain4 (bias + 2^9 hi + lo, k = 0 .. 3): %d of 1024 differ (largest N - 2^23: %d)\n", bad_chain, top - (1 << 23));
  }

  // --- 2c. the biased chain of four with 11-bit fields of 4 D (the value-table codes): any FP4 code 0 .. 7 on both sides, sparse
  // enough that a field stays below 2^11; the host sums (2 x) (2 y) = 4 x y as integers
  int bad_chain2 = 0;
  {
    static int A4[2][32][64], B4[2][2][64][32];  // [m][row][k]; [tile][m][k][col]
    uint32_t rng = 2468u;
    auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int m = 0; m < 2; ++m)
      for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 64; ++k) {
          A4[m][i][k] = (rnd() & 3) ? 0 : (int)(rnd() & 7);
          for (int t = 0; t < 2; ++t) B4[t][m][k][i] = (rnd() & 7) ? 0 : (int)(rnd() % 6);
        }
    std::vector<uint32_t> qa(512, 0), qh(512, 0), ql(512, 0), q1(64), q2(64);
    std::vector<float> qb(64);
    int nh[32], nl[32];
    for (int c = 0; c < 32; ++c) {
      nh[c] = c == 7 ? 255 : (c * 5) % 65;
      nl[c] = c == 9 ? 255 : (c * 11 + 3) % 65;
    }
    for (int l = 0; l < 64; ++l) {
      const int c = l & 31;
      for (int m = 0; m < 2; ++m)
        for (int j = 0; j < 32; ++j) {
          const int k = 32 * (l >> 5) + j, sh = 4 * (j & 7), w = 8 * l + 4 * m + (j >> 3);
          qa[w] |= (uint32_t)A4[m][c][k] << sh;
          qh[w] |= (uint32_t)B4[0][m][k][c] << sh;
          ql[w] |= (uint32_t)B4[1][m][k][c] << sh;
        }
      q1[l] = 0x55aa0000u | (uint32_t)(0x7f + 2) << 8 | (uint32_t)(0x7f + 13);  // (bytes 2 and 3 are not picked)
      q2[l] = 0xaa550000u | (uint32_t)(0x7f + 2 + ((c >> 2) & 3)) << 8 | (uint32_t)(0x7f + 13 + (c & 3));
      qb[l] = (float)((1 << 23) + (1024 - 4 * nh[c]) * 2048 + (1024 - 4 * nl[c]));
    }
    uint32_t *ea, *eh, *el, *e1, *e2;
    float *eb, *eo;
    CHECK(hipMalloc(&ea, 2048));
    CHECK(hipMalloc(&eh, 2048));
    CHECK(hipMalloc(&el, 2048));
    CHECK(hipMalloc(&e1, 256));
    CHECK(hipMalloc(&e2, 256));
    CHECK(hipMalloc(&eb, 256));
    CHECK(hipMalloc(&eo, 4096));
    CHECK(hipMemcpy(ea, qa.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(eh, qh.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(el, ql.data(), 2048, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(e1, q1.data(), 256, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(e2, q2.data(), 256, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(eb, qb.data(), 256, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chain4_kernel, dim3(1), dim3(64), 0, 0, ea, eh, el, e1, e2, eb, eo);
    CHECK(hipDeviceSynchronize());
    std::vector<float> qo(1024);
    CHECK(hipMemcpy(qo.data(), eo, 4096, hipMemcpyDeviceToHost));
    const int twice[8] = {0, 1, 2, 3, 4, 6, 8, 12};  // 2 x the FP4 value
    long long top = 0;
    int top_field = 0, quarters = 0;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 16; ++i) {
        const int col = l & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5);
        int d[2] = {0, 0};  // 4 D of the two tiles
        for (int t = 0; t < 2; ++t) {
          const int k = t ? (col >> 2) & 3 : col & 3;
          for (int m = 0; m < 2; ++m) {
            int s = 0;
            for (int kk = 0; kk < 64; ++kk) s += twice[A4[m][row][kk]] * twice[B4[t][m][kk][col]];
            d[t] += m ? s << k : s;
          }
        }
        quarters += (d[0] & 3) != 0 || (d[1] & 3) != 0;
        top_field = d[0] > top_field ? d[0] : top_field;
        top_field = d[1] > top_field ? d[1] : top_field;
        const long long n = (1ll << 23) + (1024 - 4 * nh[col]) * 2048ll + (1024 - 4 * nl[col]) + 2048ll * d[0] + d[1];
        top = n > top ? n : top;
        uint32_t got;
        memcpy(&got, &qo[l * 16 + i], 4);
        if (got != (0x4b000000u | (uint32_t)(n - (1 << 23))) && bad_chain2++ < 4)
          printf("chain4 q: row %d col %d: bits %08x, host N %lld (4 D hi %d lo %d)\n", row, col, got, n, d[0], d[1]);
      }
    if (top >= 1 << 24) { printf("chain4 q: the host sum leaves [2^23, 2^24)\n"); return 2; }
    printf("chain4 quarters (bias + 2^11 (4 hi) + 4 lo, k = 0 .. 3): %d of 1024 differ (largest 4 D: %d, results off the integers: %d)\n",
           bad_chain2, top_field, quarters);
  }

  // --- 3. the rate
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  if (rate<0>("v_mfma_i32_32x32x32_i8", dout, prop.multiProcessorCount)) return 2;
  if (rate<1>("v_mfma_f32_32x32x64_f8f6f4 fp4", dout, prop.multiProcessorCount)) return 2;
  if (rate<2>("v_mfma_scale_f32_32x32x64_f8f6f4 fp4", dout, prop.multiProcessorCount)) return 2;
  for (int waves = 1; waves <= 4; waves += 3) {
    if (pair_rate<3>("two chains of two, zero C", dout, prop.multiProcessorCount, waves)) return 2;
    if (pair_rate<4>("one chain of four, bias C", dout, prop.multiProcessorCount, waves)) return 2;
  }
  return (bad[0] || bad[1] || bad_perm || bad_chain || bad_chain2) ? 1 : 0;
}
