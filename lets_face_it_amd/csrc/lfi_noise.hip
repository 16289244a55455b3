// Per-row keyed sampling noise: a counter-based source of the prior draws of a sampler whose rows are independent conversations.
// Every draw is a pure function of (the row's 64-bit key, the frame's 64-bit position, the candidate, the channel), so what a
// conversation draws does not depend on the row it sits in, the batch size or what else drew before it, and the state - two words
// per row - can travel with the row. Keyed streaming sessions (open_stream(row_seeds=...)) and inference(row_seeds=...) draw from it;
// this unit is the generator, the row-state moves (seed / save / load of listed rows) and their C entry points. The definition ("Keyed sampling noise"; tests/row_noise_reference.py restates it
// in numpy and the GPU tests hold the kernel to that):
//   o[0..3] = philox4x32_10(counter (c >> 2, lo32(p), hi32(p), k), key (lo32(K), hi32(K)))
//   u_j = (o_j >> 9) * 2^-23 + 2^-24              exact in fp32, in (0, 1), never 0 or 1
//   g0 = sqrt(-2 ln u0) cos(2 pi u1), g1 = sqrt(-2 ln u0) sin(2 pi u1); g2, g3 likewise from (u2, u3)
//   channel c takes g[c & 3]; z = eps * g; |g| <= sqrt(48 ln 2) ~ 5.77
// Accurate libm (logf, sqrtf, sincospif - the angle 2 u1 is exact, so no rounding of 2 pi u enters), no fast intrinsics, no fast-math
// flag on the unit. Plain HBM streaming with 4-byte vector stores (no alignment assumption on `out`); no atomics, no scratch.
#include "lfi_common.h"
#include "lfi_philox.h"

#include <vector>

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

// Row state that moves with the row (seed / save / load of listed rows): the lists travel in the kernel arguments, kRngListRows per
// launch - 2.5 KB of the 4 KB an argument block may hold - so there is no host staging and no host wait. One thread owns one listed
// row (no row is listed twice: checked on the host), plain 8-byte stores.
constexpr int kRngListRows = 128;

struct RngSeedList {
  int rows[kRngListRows];
  unsigned long long keys[kRngListRows];
  unsigned long long pos[kRngListRows];
};

struct RngLoadList {
  int rows[kRngListRows];
  int entries[kRngListRows];
  unsigned long long keys[kRngListRows];
};

struct RngRowList {
  int rows[kRngListRows];
};

__global__ __launch_bounds__(kRngListRows) void row_rng_seed_rows_kernel(unsigned long long* rng, RngSeedList l, int n, int with_keys) {
  const int j = threadIdx.x;
  if (j >= n) return;
  const long r = l.rows[j];
  if (with_keys) rng[2 * r] = l.keys[j];
  rng[2 * r + 1] = l.pos[j];
}

__global__ __launch_bounds__(kRngListRows) void row_rng_save_rows_kernel(const unsigned long long* __restrict__ rng, RngRowList l, int n,
                                                                         unsigned long long* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= n) return;
  const long r = l.rows[j];
  out[2 * j] = rng[2 * r];
  out[2 * j + 1] = rng[2 * r + 1];
}

__global__ __launch_bounds__(kRngListRows) void row_rng_load_rows_kernel(unsigned long long* rng, RngLoadList l, int n,
                                                                         const unsigned long long* __restrict__ saved, int with_keys) {
  const int j = threadIdx.x;
  if (j >= n) return;
  const long r = l.rows[j], e = l.entries[j];
  rng[2 * r] = with_keys ? l.keys[j] : saved[2 * e];
  rng[2 * r + 1] = saved[2 * e + 1];
}

// The checks the three row-list entry points share, before any launch: sizes, the state's address, every listed row inside the batch
// and none twice (rows == nullptr: the identity list, where the entry point allows it).
int row_rng_check_rows(const char* what, const void* rng, int B, int nrows, const int* rows, bool rows_optional) {
  LFI_REQUIRE(B >= 0 && nrows >= 0, "%s: negative size (B %d, nrows %d)", what, B, nrows);
  LFI_REQUIRE(rng && (reinterpret_cast<uintptr_t>(rng) & 7) == 0, "%s: null pointer / misaligned rng", what);
  if (nrows == 0) return LFI_OK;
  LFI_REQUIRE(nrows <= B, "%s: %d rows listed for a batch of %d", what, nrows, B);
  LFI_REQUIRE(rows || rows_optional, "%s: null pointer (rows)", what);
  if (!rows) return LFI_OK;
  std::vector<unsigned char> seen(B, 0);
  for (int j = 0; j < nrows; ++j) {
    LFI_REQUIRE(rows[j] >= 0 && rows[j] < B, "%s: row %d of the list is %d, outside the batch (0 .. %d)", what, j, rows[j], B - 1);
    LFI_REQUIRE(!seen[rows[j]], "%s: row %d is listed twice", what, rows[j]);
    seen[rows[j]] = 1;
  }
  return LFI_OK;
}

}  // namespace

extern "C" int lfi_row_rng_seed_rows(unsigned long long* rng, int B, int nrows, const int* rows, const unsigned long long* keys,
                                     const unsigned long long* positions, void* stream) {
  const char* what = "lfi_row_rng_seed_rows";
  if (int rc = row_rng_check_rows(what, rng, B, nrows, rows, true)) return rc;
  for (int j0 = 0; j0 < nrows; j0 += kRngListRows) {
    const int n = nrows - j0 < kRngListRows ? nrows - j0 : kRngListRows;
    RngSeedList l = {};
    for (int j = 0; j < n; ++j) {
      l.rows[j] = rows ? rows[j0 + j] : j0 + j;
      l.keys[j] = keys ? keys[j0 + j] : 0ull;
      l.pos[j] = positions ? positions[j0 + j] : 0ull;
    }
    hipLaunchKernelGGL(row_rng_seed_rows_kernel, dim3(1), dim3(kRngListRows), 0, (hipStream_t)stream, rng, l, n, keys ? 1 : 0);
    LFI_LAUNCH_CHECK(what);
  }
  return LFI_OK;
}

extern "C" int lfi_row_rng_save_rows(const unsigned long long* rng, int B, int nrows, const int* rows, unsigned long long* out,
                                     void* stream) {
  const char* what = "lfi_row_rng_save_rows";
  if (int rc = row_rng_check_rows(what, rng, B, nrows, rows, false)) return rc;
  if (nrows == 0) return LFI_OK;
  LFI_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: null pointer / misaligned out", what);
  for (int j0 = 0; j0 < nrows; j0 += kRngListRows) {
    const int n = nrows - j0 < kRngListRows ? nrows - j0 : kRngListRows;
    RngRowList l = {};
    for (int j = 0; j < n; ++j) l.rows[j] = rows[j0 + j];
    hipLaunchKernelGGL(row_rng_save_rows_kernel, dim3(1), dim3(kRngListRows), 0, (hipStream_t)stream, rng, l, n, out + 2 * (long)j0);
    LFI_LAUNCH_CHECK(what);
  }
  return LFI_OK;
}

extern "C" int lfi_row_rng_load_rows(unsigned long long* rng, int B, int nrows, const int* rows, const int* entries, int nsaved,
                                     const unsigned long long* saved, const unsigned long long* keys, void* stream) {
  const char* what = "lfi_row_rng_load_rows";
  LFI_REQUIRE(nsaved >= 0, "%s: negative size (nsaved %d)", what, nsaved);
  if (int rc = row_rng_check_rows(what, rng, B, nrows, rows, false)) return rc;
  if (nrows == 0) return LFI_OK;
  LFI_REQUIRE(entries, "%s: null pointer (entries)", what);
  LFI_REQUIRE(saved && (reinterpret_cast<uintptr_t>(saved) & 7) == 0, "%s: null pointer / misaligned saved", what);
  for (int j = 0; j < nrows; ++j)
    LFI_REQUIRE(entries[j] >= 0 && entries[j] < nsaved, "%s: entry %d of the list is %d, outside the saved rows (0 .. %d)", what, j,
                entries[j], nsaved - 1);
  for (int j0 = 0; j0 < nrows; j0 += kRngListRows) {
    const int n = nrows - j0 < kRngListRows ? nrows - j0 : kRngListRows;
    RngLoadList l = {};
    for (int j = 0; j < n; ++j) {
      l.rows[j] = rows[j0 + j];
      l.entries[j] = entries[j0 + j];
      l.keys[j] = keys ? keys[j0 + j] : 0ull;
    }
    hipLaunchKernelGGL(row_rng_load_rows_kernel, dim3(1), dim3(kRngListRows), 0, (hipStream_t)stream, rng, l, n, saved, keys ? 1 : 0);
    LFI_LAUNCH_CHECK(what);
  }
  return LFI_OK;
}

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
