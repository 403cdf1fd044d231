// Probe: the operand map, the block scale and the issue rate of the FP4 (E2M1) forms of v_mfma_f32_32x32x64_f8f6f4 on
// gfx950, and the v_perm_b32 byte table of the C3 scan's left operand (csrc/indel_raw_coarse.hpp, NSM_C3C_FP4).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/mfma_fp4_probe.hip -o tools/mfma_fp4_probe && tools/mfma_fp4_probe
// 1. map: A (32 x 64) and B (64 x 32) of exact FP4 values, A != B^T, through the unscaled form (both scale arguments literal
//    0) and through the scaled form with a B scale of 2^1 on ONE column (both of its lanes, byte 2 of the scale register,
//    picked with op_sel), all 1024 results against a host loop.  The map assumed: lane l holds row (column) l & 31 and
//    k = 32 (l >> 5) + j, j = 0 .. 31, element j in nibble j & 1 (0 = low) of byte j >> 1 of its first four registers;
//    C/D: column l & 31, row (i & 3) + 8 (i >> 2) + 4 (l >> 5) in register i.
// 2. perm: the scan's packing of four counts 0 .. 64 into the two left operand words, every count in every byte position.
// 3. rate: back-to-back chains, one wave per SIMD: ns per MFMA of the i8 32x32x32 form and of the two FP4 forms.
// Exit status 0 where 1 and 2 agree with the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
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

  // --- 3. the rate
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  if (rate<0>("v_mfma_i32_32x32x32_i8", dout, prop.multiProcessorCount)) return 2;
  if (rate<1>("v_mfma_f32_32x32x64_f8f6f4 fp4", dout, prop.multiProcessorCount)) return 2;
  if (rate<2>("v_mfma_scale_f32_32x32x64_f8f6f4 fp4", dout, prop.multiProcessorCount)) return 2;
  return (bad[0] || bad[1] || bad_perm) ? 1 : 0;
}
