// Per-row keyed sampling noise: a counter-based source of the prior draws of a sampler whose rows are independent conversations.
// Every draw is a pure function of (the row's 64-bit key, the frame's 64-bit position, the candidate, the channel), so what a
// conversation draws does not depend on the row it sits in, the batch size or what else drew before it, and the state - two words
// per row - can travel with the row. The streaming sessions do not draw from it yet (they use the process generator); this unit is
// the generator and its C entry points. The definition ("Keyed sampling noise"; tests/row_noise_reference.py restates it
// in numpy and the GPU tests hold the kernel to that):
//   o[0..3] = philox4x32_10(counter (c >> 2, lo32(p), hi32(p), k), key (lo32(K), hi32(K)))
//   u_j = (o_j >> 9) * 2^-23 + 2^-24              exact in fp32, in (0, 1), never 0 or 1
//   g0 = sqrt(-2 ln u0) cos(2 pi u1), g1 = sqrt(-2 ln u0) sin(2 pi u1); g2, g3 likewise from (u2, u3)
//   channel c takes g[c & 3]; z = eps * g; |g| <= sqrt(48 ln 2) ~ 5.77
// Accurate libm (logf, sqrtf, sincospif - the angle 2 u1 is exact, so no rounding of 2 pi u enters), no fast intrinsics, no fast-math
// flag on the unit. Plain HBM streaming with 4-byte vector stores (no alignment assumption on `out`); no atomics, no scratch.
#include "lfi_common.h"
#include "lfi_philox.h"

namespace {

// One workgroup per row: every thread reads the row's (key, position) BEFORE the barrier, thread 0 writes the advanced position
// behind it - no other workgroup touches the row's words, so a launch never reads a position it has already moved.
// An item is one Philox call: 4 channels of one (frame i, candidate k).
__global__ __launch_bounds__(256) void row_noise_kernel(unsigned long long* rng, int n, int K, int C, float eps, float* __restrict__ out,
                                                        long stride_frame, long stride_row, long stride_cand, int advance) {
  const int r = blockIdx.x;
  const unsigned long long key = rng[2 * (long)r], pos = rng[2 * (long)r + 1];
  __syncthreads();
  if (advance > 0 && threadIdx.x == 0) rng[2 * (long)r + 1] = pos + (unsigned long long)advance;
  const int Q = (C + 3) >> 2;
  const long items = (long)n * K * Q;
  float* __restrict__ row = out + (long)r * stride_row;
  for (long it = threadIdx.x; it < items; it += 256) {
    const int q = (int)(it % Q);
    const long t = it / Q;
    const int k = (int)(t % K), i = (int)(t / K);
    const unsigned long long p = pos + (unsigned long long)i;
    unsigned o[4];
    philox4x32_10((unsigned)q, (unsigned)p, (unsigned)(p >> 32), (unsigned)k, (unsigned)key, (unsigned)(key >> 32), o);
    float u[4], g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = (float)(o[e] >> 9) * 0x1p-23f + 0x1p-24f;
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const float rad = sqrtf(-2.0f * logf(u[e]));
      float sn, cs;
      sincospif(2.0f * u[e + 1], &sn, &cs);
      g[e] = rad * cs;
      g[e + 1] = rad * sn;
    }
    float* __restrict__ dst = row + (long)i * stride_frame + (long)k * stride_cand + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < C) dst[e] = eps * g[e];
  }
}

__global__ __launch_bounds__(256) void row_rng_advance_kernel(unsigned long long* rng, int B, unsigned long long delta,
                                                              const int* __restrict__ lens) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  unsigned long long d = delta;
  if (lens) d = lens[r] > 0 ? (unsigned long long)lens[r] : 0ull;
  rng[2 * (long)r + 1] += d;
}

}  // namespace

extern "C" int lfi_row_noise(unsigned long long* rng, int B, int n, int ncand, int C, float eps, float* out, long stride_frame,
                             long stride_row, long stride_cand, int advance, void* stream) {
  LFI_REQUIRE(B >= 0 && n >= 0 && ncand >= 0 && C >= 0 && advance >= 0,
              "lfi_row_noise: negative size (B %d, n %d, ncand %d, C %d, advance %d)", B, n, ncand, C, advance);
  LFI_REQUIRE(ncand <= 256, "lfi_row_noise: %d candidates (at most 256)", ncand);
  LFI_REQUIRE(stride_frame >= 0 && stride_row >= 0 && stride_cand >= 0, "lfi_row_noise: negative stride (frame %ld, row %ld, cand %ld)",
              stride_frame, stride_row, stride_cand);
  const bool writes = n > 0 && C > 0;
  if (B == 0 || (!writes && advance == 0)) return LFI_OK;
  LFI_REQUIRE(rng && (reinterpret_cast<uintptr_t>(rng) & 7) == 0, "lfi_row_noise: null / misaligned rng");
  LFI_REQUIRE(!writes || out, "lfi_row_noise: null pointer (out)");
  LFI_REQUIRE(!writes || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "lfi_row_noise: out is not a float address");
  hipLaunchKernelGGL(row_noise_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rng, writes ? n : 0, ncand > 1 ? ncand : 1, C, eps, out,
                     stride_frame, stride_row, stride_cand, advance);
  LFI_LAUNCH_CHECK("lfi_row_noise");
  return LFI_OK;
}

extern "C" int lfi_row_rng_advance(unsigned long long* rng, int B, long delta, const int* lens, void* stream) {
  LFI_REQUIRE(B >= 0 && delta >= 0, "lfi_row_rng_advance: negative size (B %d, delta %ld)", B, delta);
  if (B == 0 || (!lens && delta == 0)) return LFI_OK;
  LFI_REQUIRE(rng && (reinterpret_cast<uintptr_t>(rng) & 7) == 0, "lfi_row_rng_advance: null / misaligned rng");
  hipLaunchKernelGGL(row_rng_advance_kernel, dim3(lfi_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, rng, B, (unsigned long long)delta,
                     lens);
  LFI_LAUNCH_CHECK("lfi_row_rng_advance");
  return LFI_OK;
}
