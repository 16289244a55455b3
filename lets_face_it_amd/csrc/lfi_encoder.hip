// Window encoders: the three per-timestep nn.GRU calls of ModalityEncoder.forward (glow/models.py:55-80) for ALL
// (sample, timestep) windows of a training sequence at once, forward and BPTT.
//
// The reference re-encodes an almost identical window from h0 = 0 at every timestep (3 cuDNN GRU launches per
// timestep, each on B rows). Here every window is one row of a (F = N*B) x hid state matrix and the `hist` GRU steps
// advance ALL F windows together:
//   - the input projection x W_ih^T is hoisted out (one GEMM over the B*T distinct frames, shared by every window
//     that covers a frame; the dropout mask is one scalar per (window, step) so it commutes with the projection),
//   - each step is one MFMA GEMM h_{s-1} (F x hid) @ W_hh^T on lfi_gemm_f32 plus one flat, fully coalesced gate
//     kernel that also writes the stash for BPTT,
//   - stashes are step-major ([s][w][...]) so the deferred weight-gradient GEMMs see plain row ranges
//     (dW_hh = dgh[1:]^T hseq[:-1]).
// Backward mirrors it: per step one gate-derivative kernel and one GEMM dgh_s (F x 3hid) @ W_hh accumulated onto the
// carried gradient.
//
// Three translation units: this one (the weight images the fused kernels read, the size queries that belong to neither direction,
// and the elementwise helpers lfi_gather_windows, lfi_fill_frame_nb, lfi_leaky_grad), lfi_encoder_fwd.hip (forward) and
// lfi_encoder_bwd.hip (BPTT, window scatter, bias fold); lfi_encoder_common.h holds what they share.
#include "lfi_encoder_common.h"

namespace {

// element ((((kt*3 + g)*nct + ct)*2 + plane)*64 + lane)*8 + e  (fwd)  /  ((((g*nkt + kt)*nct + ct)*2 + plane)*64 + lane)*8 + e (bwd)
// holds k = kt*16 + 8*(lane>>5) + e, column j = ct*32 + (lane&31) of W_hh^T[k][g*hid + j] (fwd) / W_hh[g*hid + k][j] (bwd)
__global__ __launch_bounds__(256) void enc_frag_weights_kernel(const float* __restrict__ whh, int hid, int Kp, int Jp, int fwd,
                                                               __bf16* __restrict__ dst) {
  const int nkt = Kp >> 4, nct = Jp >> 5;
  const long n = 3L * Kp * Jp * 2;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx & 7), l = (int)((idx >> 3) & 63), plane = (int)((idx >> 9) & 1);
    long q = idx >> 10;
    const int ct = (int)(q % nct); q /= nct;
    int g, kt;
    if (fwd) { g = (int)(q % 3); kt = (int)(q / 3); } else { kt = (int)(q % nkt); g = (int)(q / nkt); }
    const int k = kt * 16 + 8 * (l >> 5) + e, j = ct * 32 + (l & 31);
    float v = 0.0f;
    if (k < hid && j < hid) v = fwd ? whh[((long)g * hid + j) * hid + k] : whh[((long)g * hid + k) * hid + j];
    const __bf16 hi = (__bf16)v;
    dst[idx] = plane ? (__bf16)(v - (float)hi) : hi;
  }
}

// Fragment order of v_mfma_f32_16x16x32_bf16 for the forward recurrence: see enc_chunk16 (lfi_encoder_common.h)
__global__ __launch_bounds__(256) void enc_frag_weights16_kernel(const float* __restrict__ whh, int hid, int Kp, int Jp, __bf16* __restrict__ dst) {
  const int nct = Jp >> 4, nchunk = Kp >> 3;
  const long n = 3L * Kp * Jp * 2;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx & 7), l = (int)((idx >> 3) & 63), plane = (int)((idx >> 9) & 1);
    long q = idx >> 10;
    const int ct = (int)(q % nct); q /= nct;
    const int g = (int)(q % 3), m = (int)(q / 3);
    const int k = 8 * enc_chunk16(m, l >> 4, nchunk) + e, j = ct * 16 + (l & 15);
    float v = 0.0f;
    if (k < hid && j < hid) v = whh[((long)g * hid + j) * hid + k];
    const __bf16 hi = (__bf16)v;
    dst[idx] = plane ? (__bf16)(v - (float)hi) : hi;
  }
}

// fwd = 1: dst[(k*3 + g)*Jp + j] = whh[(g*hid + j)*hid + k] ; fwd = 0: dst[(g*Kp + k)*Jp + j] = whh[(g*hid + k)*hid + j]
__global__ __launch_bounds__(256) void enc_pad_weights_kernel(const float* __restrict__ whh, int hid, int Kp, int Jp, int fwd,
                                                              float* __restrict__ dst) {
  const long n = 3L * Kp * Jp;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int j = (int)(idx % Jp);
    const int q = (int)(idx / Jp);
    const int g = fwd ? q % 3 : q / Kp, k = fwd ? q / 3 : q % Kp;
    float v = 0.0f;
    if (k < hid && j < hid) v = fwd ? whh[((long)g * hid + j) * hid + k] : whh[((long)g * hid + k) * hid + j];
    dst[idx] = v;
  }
}

__global__ __launch_bounds__(256) void gather_windows_kernel(const float* __restrict__ X, int B, int T, int dim, int N, int start,
                                                             int hist, int incl, const float* __restrict__ mask,
                                                             float* __restrict__ cond, int ldcond, int col) {
  const int f = blockIdx.x;  // n*B + b
  const int n = f / B, b = f - n * B;
  const int t0 = start + n - hist + incl;
  const int tot = hist * dim;
  // window rows are consecutive frames of one sample: one contiguous run of hist*dim floats
  const float* src = X + ((long)b * T + t0) * dim;
  float* dst = cond + (long)f * ldcond + col;
  if (mask) {  // dropout multiplier per (window, history step) (glow/models.py:56-58)
    const float* mk = mask + (long)f * hist;
    for (int i = threadIdx.x; i < tot; i += 256) dst[i] = src[i] * mk[i / dim];
  } else {
    for (int i = threadIdx.x; i < tot; i += 256) dst[i] = src[i];
  }
}

// FeatureEncoder's optional frame-counter column (glow/models.py:89,116-117,143-144): frame f = n*B + b gets base[b] + offset + 2n
// (SeqGlow.forward / invert: base = batch["frame_nb"], offset = 2 * start, :539-542,557-558; inference: base = 1, offset 0, :572-575)
__global__ __launch_bounds__(256) void fill_frame_nb_kernel(const float* __restrict__ base, float offset, int B, long F,
                                                            float* __restrict__ cond, int ldcond, int col) {
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < F; f += (long)gridDim.x * 256) {
    const long n = f / B;
    const int b = (int)(f - n * B);
    cond[f * ldcond + col] = (base ? base[b] : 1.0f) + offset + 2.0f * (float)n;
  }
}

__global__ __launch_bounds__(256) void leaky_grad_kernel(float* __restrict__ d, long ldd, const float* __restrict__ y, long ldy, int rows,
                                                         int cols, float slope) {
  const long total = (long)rows * cols;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / cols;
    const int c = (int)(idx - r * cols);
    if (!(y[r * ldy + c] > 0.0f)) d[r * ldd + c] *= slope;
  }
}

}  // namespace

// ---- the recurrent weights as the fused kernels read them, into `work` (enc_build_weights, lfi_encoder_common.h)
extern "C" void lfi_internal_enc_build_weights(int weights, const float* whh, int hid, int Kp, int Jp, int fwd, float* work, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (weights == ENC_W_FRAG16) hipLaunchKernelGGL(enc_frag_weights16_kernel, dim3(lfi_cdiv(6L * Kp * Jp, 256)), dim3(256), 0, st, whh, hid, Kp, Jp,
                                                  reinterpret_cast<__bf16*>(work));
  else if (weights == ENC_W_FRAG) hipLaunchKernelGGL(enc_frag_weights_kernel, dim3(lfi_cdiv(6L * Kp * Jp, 256)), dim3(256), 0, st, whh, hid, Kp, Jp,
                                                     fwd, reinterpret_cast<__bf16*>(work));
  else hipLaunchKernelGGL(enc_pad_weights_kernel, dim3(lfi_cdiv(3L * Kp * Jp, 256)), dim3(256), 0, st, whh, hid, Kp, Jp, fwd, work);
}

// May the gate stash between lfi_encode_windows_fwd and _bwd be fp16 ([hist][F][hid][4] halves instead of [hist][F][4][hid] floats)?
// Only the row-layout fused GRU kernels read / write that form (asked for the masked forward kernel, the larger of the two).
extern "C" int lfi_encode_windows_stash_f16_ok(const lfi_enc_desc* d) {
  return (d && enc_plan_fwd(d, true, true, true).wide_fits && enc_plan_bwd(d, d->ldcond, true).stash_f16_ok) ? 1 : 0;
}

extern "C" long lfi_encode_windows_work_floats(const lfi_enc_desc* d) {
  if (!d) return 0;
  const long unfused = (long)d->N * d->B * (d->lstm ? 4 : 3) * d->hid;  // fwd: gh (F x G); bwd: two (LSTM: four) F x hid buffers
  const long fused = 3L * 256 * 256;                    // fused path: zero-padded weight image
  return unfused > fused ? unfused : fused;
}

extern "C" int lfi_gather_windows(const float* X, int B, int T, int dim, int N, int start, int hist, int incl,
                                  const float* mask, float* cond, int ldcond, int col, void* stream) {
  LFI_REQUIRE(X && cond, "lfi_gather_windows: null pointer");
  LFI_REQUIRE(B > 0 && T > 0 && dim > 0 && N > 0 && hist > 0 && (incl == 0 || incl == 1), "lfi_gather_windows: bad dims");
  LFI_REQUIRE(start - hist + incl >= 0 && start + N - 1 + incl <= T, "lfi_gather_windows: window out of range");
  hipLaunchKernelGGL(gather_windows_kernel, dim3(N * B), dim3(256), 0, (hipStream_t)stream, X, B, T, dim, N, start, hist,
                     incl, mask, cond, ldcond, col);
  LFI_LAUNCH_CHECK("lfi_gather_windows");
  return LFI_OK;
}

extern "C" int lfi_fill_frame_nb(const float* base, float offset, int B, int N, float* cond, int ldcond, int col, void* stream) {
  LFI_REQUIRE(cond && B > 0 && N > 0 && col >= 0 && col < ldcond, "lfi_fill_frame_nb: bad arguments");
  hipLaunchKernelGGL(fill_frame_nb_kernel, dim3(ew_blocks((long)N * B)), dim3(256), 0, (hipStream_t)stream, base, offset, B,
                     (long)N * B, cond, ldcond, col);
  LFI_LAUNCH_CHECK("lfi_fill_frame_nb");
  return LFI_OK;
}

extern "C" int lfi_leaky_grad(float* d, long ldd, const float* y, long ldy, int rows, int cols, float slope, void* stream) {
  LFI_REQUIRE(d && y && rows >= 0 && cols >= 0, "lfi_leaky_grad: bad arguments");
  if (rows == 0 || cols == 0) return LFI_OK;
  hipLaunchKernelGGL(leaky_grad_kernel, dim3(ew_blocks((long)rows * cols)), dim3(256), 0, (hipStream_t)stream, d, ldd, y, ldy,
                     rows, cols, slope);
  LFI_LAUNCH_CHECK("lfi_leaky_grad");
  return LFI_OK;
}
