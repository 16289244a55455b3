// Streaming (frame-by-frame) sampling: the per-step state update of a sampling session (engine.py SampleStream).
//
// A session keeps, per conditioning modality with history > 0, the last `hist` frames of every batch row (B x hist x dim), the
// prev_p1_face window of its own output (B x (hist1 + 1) x C), the prior noise of the step and the frame counter. One launch moves
// all of it forward by one frame on the caller's stream; the static part and the reverse chain of the step (a captured graph) then
// read only session-owned, fixed-address memory. What SeqGlow.inference does with whole sequences (glow/models.py:567-596), one
// frame at a time.
#include "lfi_common.h"

namespace {

constexpr int kStreamMaxWins = 8;

struct StreamWins {
  float* win[kStreamMaxWins];        // B x hist x dim, row b at b * hist * dim
  const float* src[kStreamMaxWins];  // B x dim: the new frame; NULL = shift only (the chain writes the last row)
  int hist[kStreamMaxWins];
  int dim[kStreamMaxWins];
  int count;
};

__device__ __forceinline__ unsigned stream_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// Workgroup (i, b): window i of batch row b, or (i = count) the noise row and the frame counter of batch row b. A window is read and
// written by its own workgroup only: every 256-element chunk is read into registers, a barrier, then written. Chunk k reads elements
// [256 k + dim, 256 (k + 1) + dim) and writes [256 k, 256 (k + 1)): nothing a later chunk reads has been written yet, and the barrier
// orders the reads of a chunk before its writes (the trip count is uniform over the workgroup).
__global__ __launch_bounds__(256) void stream_advance_kernel(StreamWins w, const float* __restrict__ noise, float* __restrict__ noise_dst,
                                                            int C, float* __restrict__ frame_nb, unsigned* __restrict__ guard) {
  const int b = blockIdx.y;
  const int i = blockIdx.x;
  unsigned m = 0u;
  if (i < w.count) {
    const int dim = w.dim[i];
    const long n = (long)w.hist[i] * dim;
    const long last = n - dim;                     // first element of the newest row
    float* win = w.win[i] + (long)b * n;
    const float* src = w.src[i];
    const long stop = src ? n : last;              // without a source the newest row stays where it is
    for (long base = 0; base < stop; base += 256) {
      const long j = base + threadIdx.x;
      float v = 0.0f;
      if (j < stop) {
        v = j < last ? win[j + dim] : src[(long)b * dim + (j - last)];
        const unsigned a = stream_abs_bits(v);
        m = a > m ? a : m;
      }
      __syncthreads();
      if (j < stop) win[j] = v;
    }
  } else {
    for (int j = threadIdx.x; j < C; j += 256) {
      const float v = noise[(long)b * C + j];
      noise_dst[(long)b * C + j] = v;
      const unsigned a = stream_abs_bits(v);
      m = a > m ? a : m;
    }
    if (frame_nb && threadIdx.x == 0) frame_nb[b] += 2.0f;   // SeqGlow.inference: ones, + 2 per frame (glow/models.py:572-575)
  }
  if (!guard) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(guard, m);
}

}  // namespace

extern "C" int lfi_stream_advance(int B, int count, float* const* win, const float* const* src, const int* hist, const int* dim,
                                  const float* noise, float* noise_dst, int C, float* frame_nb, unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_advance: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(count >= 0 && count <= kStreamMaxWins, "lfi_stream_advance: %d windows (at most %d)", count, kStreamMaxWins);
  LFI_REQUIRE(count == 0 || (win && src && hist && dim), "lfi_stream_advance: null window table");
  LFI_REQUIRE(noise && noise_dst && C > 0, "lfi_stream_advance: null noise / C = %d", C);
  StreamWins w = {};
  for (int i = 0; i < count; ++i) {
    LFI_REQUIRE(win[i] && hist[i] > 0 && dim[i] > 0, "lfi_stream_advance: window %d: hist %d, dim %d", i, hist[i], dim[i]);
    w.win[i] = win[i]; w.src[i] = src[i]; w.hist[i] = hist[i]; w.dim[i] = dim[i];
  }
  w.count = count;
  hipLaunchKernelGGL(stream_advance_kernel, dim3(count + 1, B), dim3(256), 0, (hipStream_t)stream, w, noise, noise_dst, C, frame_nb,
                     guard_bits);
  LFI_LAUNCH_CHECK("lfi_stream_advance");
  return LFI_OK;
}
