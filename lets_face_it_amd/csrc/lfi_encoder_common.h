// Window encoders: what more than one of the encoder's translation units uses (lfi_encoder.hip: weight images, size queries and
// the elementwise helpers; lfi_encoder_fwd.hip: the forward kernels and lfi_encode_windows_fwd; lfi_encoder_bwd.hip: BPTT, the
// window scatter, the bias fold and their entry points). Kernel arguments, the fused kernels' geometry, the device helpers of the
// gate epilogues, the switches, the LDS formulas and the shape half of the plans. No kernel lives here: every one is instantiated
// in exactly one unit.
#pragma once
#include "lfi_common.h"
#include <type_traits>

// (LFI_ENC_EXP_M16: timing-only experiment, garbage results - the recurrences' MFMAs as two v_mfma_f32_16x16x32_bf16 on the same
// registers, to see whether the chip holds a higher clock on that shape here as it does in the planes GEMMs)
#ifdef LFI_ENC_EXP_M16
#define ENC_MFMA(a, b, c, x, y, z) enc_mfma16_probe(a, b, c)
#else
#define ENC_MFMA(a, b, c, x, y, z) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, x, y, z)
#endif
namespace {
#ifdef LFI_ENC_EXP_M16
template <typename AV, typename BV>
__device__ __forceinline__ f32x16 enc_mfma16_probe(AV a, BV b, f32x16 c) {
  f32x4 q0 = {c[0], c[1], c[2], c[3]}, q1 = {c[4], c[5], c[6], c[7]};
  q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, q0, 0, 0, 0);
  q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, q1, 0, 0, 0);
  c[0] = q0[0]; c[1] = q0[1]; c[2] = q0[2]; c[3] = q0[3];
  c[4] = q1[0]; c[5] = q1[1]; c[6] = q1[2]; c[7] = q1[3];
  return c;
}
#endif

struct EncArgs {
  int B, T, N, start, hist, hid, ldcond, col, dup;
  int lstm, G;         // LSTM window encoder (gate blocks i, f, g, o); G = (lstm ? 4 : 3) * hid
  int compact;         // fused GRU backward: dgi holds only its n-gate block ([hist][F][hid]); its r and z blocks equal dgh's
  int g16;             // dgi / dgh are bf16 arrays of the same shapes (lfi_enc_desc.bwd_two_products with the wide fused backward)
  int F;
  const float* Xp;     // (B*T) x 3hid
  const float* b_ih;
  const float* b_hh;
  const float* mask;   // F x hist or null
  float* cond;
  float* gates;        // [hist][F][4][hid]
  float* hseq;         // [hist][F][hid]
  const float* dcond; int lddcond;
  float* dgi;          // [hist][F][3hid]
  float* dgh;          // [hist][F][3hid]
  float* bias_part;    // fused backward only: [workgroups * row groups][4][hid] partial sums of dar, dau, dan, dan*r (or null)
  unsigned long long* stamps;  // diagnostics only
};
// phase stamps of the fused forward kernel: compiled in only with -DLFI_ENC_STAMPS (they cost registers: 321 spills)
#ifdef LFI_ENC_STAMPS
#define ENC_STAMP(slot)                                                                                          \
  do {                                                                                                           \
    if (a.stamps && tid == 0 && blockIdx.x == 0 && s >= 4 && s < 12)                                              \
      a.stamps[128 + 8 * (s - 4) + (slot)] = __builtin_amdgcn_s_memtime();                                        \
  } while (0)
#else
#define ENC_STAMP(slot) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------- fused persistent path
// For hid <= 256 the whole window recurrence of a block of windows runs inside ONE workgroup: windows are independent
// of one another, so a workgroup owns R windows, keeps their state h (R x hid) in LDS across all `hist` steps and
// per step does   gh = h_{s-1} W_hh^T  on v_mfma_f32_32x32x2_f32 (A = h from LDS k-major, B = W_hh^T streamed from L2
// straight into the MFMA operand registers, chunk-prefetched) + the gate math on the accumulators. Nothing but the
// stashes the backward pass needs goes to HBM (the unfused path also wrote and re-read gh, F x 3hid, every step, and
// paid one GEMM + one gate launch per step). One launch per modality instead of 2 * hist.
//   workgroup = 4 waves; wave (rg, cg) owns rows [32 rg, 32 rg + 32) x hidden [64 cg, 64 cg + 64) x the 3 gates
//   (6 accumulator tiles); ncg = column groups = next_pow2(ceil(hid / 64)) <= 4, R = 32 * 4 / ncg rows per workgroup;
//   LDS = Kp x (R + 1) floats <= 33 KB and <= 256 VGPRs: two workgroups share a CU and one's epilogue (HBM stores)
//   overlaps the other's MFMAs.
// The weights are re-laid once per call into a zero-padded image (Kp = hid rounded up to 16 rows of k, Jp = 64 ncg
// columns) so the k loop carries no bounds checks: every load in it is unconditional.
#ifndef LFI_ENC_NT
#define LFI_ENC_NT 256   // (512 = one 64-window workgroup per CU: measured slower, 0.90 vs 0.78 ms on the p2_face forward launch - no L1 sharing of the weight stream)
#endif
constexpr int ENC_NT = LFI_ENC_NT;   // threads per workgroup of the fused kernels
constexpr int ENC_NW = ENC_NT / 64;  // waves: ncg column groups x ENC_NW / ncg row groups of 32 windows
constexpr int ENC_KC = 4;  // k-pairs per prefetch chunk (two chunks in flight)
extern __shared__ __attribute__((aligned(16))) float enc_smem[];

struct EncFused {
  int ncg, R, Kp, Jp;
  const float* wpad;   // forward: [Kp][3][Jp] = W_hh^T ; backward: [3][Kp][Jp] = W_hh, zero padded
  const uint4* wfrag;  // bf16x3 mode: the same matrices split into bf16 hi / lo planes in MFMA B-fragment order
};

// bf16x3 variant of the fused path (lfi_enc_desc.precision = 1): the state is split into bf16 hi + lo when it is written
// to LDS (row-major [R][Kp + 8] images, one ds_read_b128 per A fragment) and every 32x32x16 step issues
// lo*hi + hi*lo + hi*hi into the fp32 accumulators (~2^-16 relative per product, 16x the f32-input MFMA rate). The
// weights are split ONCE per call into fragment order: the 8 bf16 a lane feeds to v_mfma_f32_32x32x16_bf16 are 16
// contiguous bytes, a wave's fragment 1 KB: one coalesced global_load_dwordx4 per (k-tile, column tile, plane).
typedef __bf16 ebf16x8 __attribute__((ext_vector_type(8)));
union EncFrag { uint4 u; ebf16x8 v; };
// (hi, lo) bf16 pairs of (a, b), packed low / high half: hi = RNE(v), lo = RNE(v - hi) - as `(__bf16)v` element by element
typedef __bf16 ebf16x2 __attribute__((ext_vector_type(2)));
typedef float efloat2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2(float a, float b, unsigned* hi, unsigned* lo) {
  const ebf16x2 h = __builtin_convertvector((efloat2){a, b}, ebf16x2);
  const unsigned hb = __builtin_bit_cast(unsigned, h);
  const float ha = __builtin_bit_cast(float, hb << 16), hbv = __builtin_bit_cast(float, hb & 0xffff0000u);
  const ebf16x2 l = __builtin_convertvector((efloat2){a - ha, b - hbv}, ebf16x2);
  *hi = hb;
  *lo = __builtin_bit_cast(unsigned, l);
}

// Fragment order of v_mfma_f32_16x16x32_bf16 for the forward recurrence (enc_gru_fwd_r64_kernel<.., M16 = true>; Kp a multiple of 256):
// element ((((m*3 + g)*nct + ct)*2 + plane)*64 + lane)*8 + e holds column j = ct*16 + (lane&15) of W_hh^T[k][g*hid + j] at
// k = 8 enc_chunk16(m, lane>>4, Kp/8) + e: lane group q of MFMA m takes the 16-byte k-chunk 2m + (q>>1) of the first (q even) or
// second (q odd) half of the row - the chunks of the groups that share a ds_read_b128 cycle lie 256 bytes apart in the state
// images, whose rows (Kp + 8 bf16) advance by one 16-byte slot: all 64 banks, no conflict.
__host__ __device__ inline int enc_chunk16(int m, int q, int nchunk) { return 2 * m + (q >> 1) + (nchunk >> 1) * (q & 1); }

__device__ __forceinline__ int enc_rowl(int rg, int r, int half) { return rg * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }

// Raw buffer access for the gate epilogues: a uniform 128-bit resource (base + size) in SGPRs, one 32-bit byte offset per
// lane and a uniform SGPR offset on top. The plain-pointer form cost ~20 VALU instructions of 64-bit address arithmetic
// per access (60 % of the epilogue's instructions; rocprof: these kernels are VALU-issue bound, not HBM or MFMA bound).
// Accesses past `bytes` read 0 / are dropped by the hardware.
typedef __amdgpu_buffer_rsrc_t enc_rsrc;
__device__ __forceinline__ enc_rsrc enc_buf(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0xfffffff0L ? 0xfffffff0L : bytes), 0x00020000);
}
__device__ __forceinline__ float enc_ld(enc_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// read-once stash values in the backward kernel (1.76 GB per p2_face launch): streamed (aux 2 = non-temporal), so that they do
// not sweep the weight fragments every workgroup re-reads each step out of L2
#ifndef LFI_ENC_LDS_AUX
#define LFI_ENC_LDS_AUX 2
#endif
__device__ __forceinline__ float enc_ld_stream(enc_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, LFI_ENC_LDS_AUX));
}
// The stashes are written once and read by a much later kernel (BPTT, the weight-gradient GEMMs): non-temporal (aux 2), so
// 1.5 GB of them per launch do not sweep the weights and the projected inputs out of L2.
#ifndef LFI_ENC_ST_AUX
#define LFI_ENC_ST_AUX 2
#endif
__device__ __forceinline__ void enc_st(float v, enc_rsrc r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, LFI_ENC_ST_AUX);
}

// 16-byte (and 8-byte) forms for the row-layout gate epilogues, where a lane owns 4 consecutive columns
typedef __attribute__((ext_vector_type(4))) unsigned enc_u32x4;
__device__ __forceinline__ f32x4 enc_ld4(enc_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 enc_ld4s(enc_rsrc r, unsigned voff, unsigned soff) {   // read-once stash values: streamed
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 2));
}
__device__ __forceinline__ void enc_st4(f32x4 v, enc_rsrc r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(enc_u32x4, v), r, voff, soff, LFI_ENC_ST_AUX);
}
typedef __attribute__((ext_vector_type(2))) unsigned enc_u32x2;
// four fp32 values rounded to bf16 (round to nearest even, as the GEMMs' operand split rounds the hi part), one 8-byte store
__device__ __forceinline__ void enc_st2h(f32x4 v, enc_rsrc r, unsigned voff, unsigned soff) {
  uint2 h, l;
  split2(v[0], v[1], &h.x, &l.x); split2(v[2], v[3], &h.y, &l.y);
  __builtin_amdgcn_raw_buffer_store_b64((enc_u32x2){h.x, h.y}, r, voff, soff, LFI_ENC_ST_AUX);
}
// fp16 gate stash (lfi_enc_desc.stash_f16): the four values BPTT needs of a hidden unit - r, z, n, W_hn h + b_hn - as four fp16
// side by side (8 bytes per unit instead of 16: r, z, n lie in (-1, 1) and the last one within a few units of 0, so fp16's 11
// bits round them by <= 2^-12 absolute, unbiased - finer than the bf16 rounding the two-product backward products apply to the
// gate DERIVATIVES computed from them). A lane's four consecutive units are 32 contiguous bytes: two 16-byte accesses either way.
typedef _Float16 enc_h16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 enc_pack_gates(float r, float z, float n, float g) {
  const enc_h16x4 h = __builtin_convertvector((f32x4){r, z, n, g}, enc_h16x4);   // round to nearest even
  return __builtin_bit_cast(uint2, h);
}
__device__ __forceinline__ f32x4 enc_unpack_gates(unsigned lo, unsigned hi) {
  const enc_h16x4 h = __builtin_bit_cast(enc_h16x4, (uint2){lo, hi});
  return __builtin_convertvector(h, f32x4);
}
constexpr int ENC_TP = 68;   // floats per row of the transpose tile: 272 B (16-byte aligned rows, 4-bank skew per row)

// Ingredient-removal builds (timing only, results are garbage; tools/enc_probe.py): -DLFI_ENC_EXP_FIXED_W = every k-tile reads the
// weight fragments of k-tile 0 (the L2 -> CU weight stream becomes an L1 hit), -DLFI_ENC_EXP_NO_XP = no projected-input loads
// -DLFI_ENC_EXP_NO_KLOOP = no h W_hh^T product (epilogue + barriers only), -DLFI_ENC_EXP_NO_GATEMATH = sigmoid / tanh replaced by one
// multiply (the epilogue's transcendental VALU work removed, its memory and LDS traffic kept)
#ifdef LFI_ENC_EXP_NO_GATEMATH
#define ENC_SIG(x) (0.25f * (x))
#define ENC_TANH(x) (0.25f * (x))
#else
#define ENC_SIG(x) sigmoidf_(x)
#define ENC_TANH(x) tanhf_(x)
#endif
#ifdef LFI_ENC_EXP_FIXED_W
#define ENC_WKT(kt) 0
#else
#define ENC_WKT(kt) (kt)
#endif

template <typename Kf>
int enc_set_lds(Kf kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return LFI_OK;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    lfi_set_error("window encoder: cannot reserve %zu bytes of LDS: %s", bytes, hipGetErrorString(e));
    return LFI_ERR_LAUNCH;
  }
  return LFI_OK;
}

// shape of the fused path, or 0 when the recurrence is too wide for it
int enc_fused_shape(int hid, EncFused* q) {
  if (hid > 256) return 0;
  int tiles = lfi_cdiv(hid, 64), ncg = 1;
  while (ncg < tiles) ncg <<= 1;
  q->ncg = ncg;
  q->R = 32 * (ENC_NW / ncg);
  q->Kp = (hid + 15) & ~15;
  q->Jp = 64 * ncg;
  return 1;
}

int fill_args(const lfi_enc_desc* d, EncArgs* a, const char* who) {
  LFI_REQUIRE(d, "%s: null descriptor", who);
  LFI_REQUIRE(d->B > 0 && d->T > 0 && d->N > 0 && d->hist > 0 && d->hid > 0, "%s: bad dims", who);
  LFI_REQUIRE(d->start + d->N <= d->T, "%s: start + N > T", who);
  LFI_REQUIRE(d->hist <= d->start + 1, "%s: window longer than start+1", who);
  a->B = d->B; a->T = d->T; a->N = d->N; a->start = d->start; a->hist = d->hist; a->hid = d->hid;
  a->ldcond = d->ldcond; a->col = d->col; a->dup = d->dup;
  a->lstm = d->lstm ? 1 : 0; a->G = (d->lstm ? 4 : 3) * d->hid;
  a->F = d->N * d->B;
  return LFI_OK;
}

int ew_blocks(long total) { return (int)(lfi_cdiv(total, 256) < 4096 ? lfi_cdiv(total, 256) : 4096); }

}  // namespace

// ---- switches: all read at every call (tests and A/B runs flip them inside one process)
static inline bool enc_wide_enabled() { return lfi_env_on("LFI_ENC_WIDE"); }           // the row-layout forward kernels (0: the accumulator-layout kernel)
static inline bool enc_wide_bwd_enabled() { return lfi_env_on("LFI_ENC_WIDE_BWD"); }   // the row-layout backward kernels (0: the exact-f32 accumulator-layout kernel)
static inline bool enc_m16_enabled() { return lfi_env_on("LFI_ENC_M16"); }             // the forward 64-window kernel on v_mfma_f32_16x16x32_bf16
static inline bool enc_r64_enabled() { return lfi_env_on("LFI_ENC_R64"); }             // the two-row-tile kernels, forward and backward
// the forward kernel with the gate epilogue under the matrix phase: LFI_ENC_T16 = 0 never,
// 1 (default) where no stash is written (inference, validation, the sampler's static part: 0.46 against 0.51 ms on the p2_face
// shape), 2 with a stash too (training: measured SLOWER there, 0.545 against 0.532 ms alone and +0.15 ms on the whole step - the
// stash stores share the wave's in-order vmcnt queue with the weight stream)
static inline int enc_t16_mode() {
  const char* e = getenv("LFI_ENC_T16");
  return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : 1;
}

// ---- dynamic LDS of each fused kernel, in bytes: one formula per kernel
// accumulator-layout forward: state images (+ the bf16 hi / lo pair in bf16x3 mode) + per-row offset tables
static inline size_t enc_fwd_fused_lds(const EncFused& q, bool x3) {
  return (size_t)q.Kp * (q.R + 1) * sizeof(float) + (x3 ? (size_t)2 * q.R * (q.Kp + 8) * sizeof(__bf16) : 0) + (size_t)3 * q.R * sizeof(unsigned);
}
// row-layout forward, 32 windows per wave: image pair + transpose tiles + biases + offset tables (+ the mask rows)
static inline size_t enc_fwd_wide_lds(const EncFused& q, int hist, bool masked) {
  return (size_t)2 * q.R * (q.Kp + 8) * sizeof(__bf16) + (size_t)ENC_NW * 32 * ENC_TP * sizeof(float) + (size_t)6 * q.Jp * sizeof(float) +
         (size_t)2 * q.R * sizeof(unsigned) + (masked ? (size_t)q.R * hist * sizeof(float) : 0);
}
static inline size_t enc_fwd_r64_lds(const EncFused& q, int hist, bool masked) {
  const int R2 = 2 * q.R;
  return (size_t)2 * R2 * (q.Kp + 8) * sizeof(__bf16) + (size_t)ENC_NW * 2 * 32 * ENC_TP * sizeof(float) +
         (size_t)6 * q.Jp * sizeof(float) + (size_t)2 * R2 * sizeof(unsigned) + (masked ? (size_t)R2 * hist * sizeof(float) : 0);
}
static inline size_t enc_fwd_t16_lds(int hist, bool masked) {
  return (size_t)4 * 64 * 264 * sizeof(__bf16) + (size_t)6 * 256 * sizeof(float) + (size_t)2 * 64 * sizeof(unsigned) +
         (masked ? (size_t)64 * hist * sizeof(float) : 0);
}
// accumulator-layout backward: state image + per-row offset / liveness tables
static inline size_t enc_bwd_fused_lds(const EncFused& q) { return (size_t)q.Kp * (q.R + 1) * sizeof(float) + (size_t)2 * q.R * sizeof(unsigned); }
// row-layout backward: image pair + the larger of the transpose tiles and one more image pair (in floats) + tables
static inline size_t enc_bwd_wide_lds(const EncFused& q) {
  const long imgf = (long)q.R * (q.Kp + 8);
  return (size_t)2 * q.R * (q.Kp + 8) * sizeof(__bf16) + (size_t)(ENC_NW * 32 * ENC_TP > imgf ? ENC_NW * 32 * ENC_TP : imgf) * sizeof(float) +
         (size_t)2 * q.R * sizeof(unsigned);
}
static inline size_t enc_bwd_r64_lds(const EncFused& q) {
  const int R2 = 2 * q.R;
  const long imgf = (long)R2 * (q.Kp + 8);
  return (size_t)2 * R2 * (q.Kp + 8) * sizeof(__bf16) +
         (size_t)(ENC_NW * 2 * 32 * ENC_TP > imgf ? ENC_NW * 2 * 32 * ENC_TP : imgf) * sizeof(float) + (size_t)2 * R2 * sizeof(unsigned);
}

// ---- which instantiation: the fused kernels all have one signature
typedef void (*EncKernel)(EncArgs, EncFused);

// ---- the recurrent weights as the fused kernels read them, into `work`: the image kernels live in lfi_encoder.hip
enum EncWeights { ENC_W_PAD, ENC_W_FRAG, ENC_W_FRAG16 };   // zero-padded f32 | bf16 hi / lo fragments | the same in 16 x 16 x 32 order (forward only)
static inline void enc_build_weights(EncWeights w, EncFused* q, const float* whh, int hid, int fwd, float* work, hipStream_t st) {
  lfi_internal_enc_build_weights((int)w, whh, hid, q->Kp, q->Jp, fwd, work, st);
  q->wpad = work;
  q->wfrag = reinterpret_cast<const uint4*>(work);
}

// ---- plans: which kernel variant a descriptor takes, and everything sized by that choice. The size queries and the launchers both ask
// here; the launchers then pick the instantiation of that variant in their own unit (enc_fwd_pick, enc_bwd_pick).
// `aligned`: are the buffers the row-layout kernels touch 16-byte aligned? (the queries, which see no pointers, pass true; the
// launchers REQUIRE what the queries promised)
struct EncFwdPlan {
  int variant;       // lfi_encode_windows_fwd_variant's numbering: 0 unfused (hid > 256) or LSTM, 1 accumulator-layout fused, 2 row-layout
                     // (32 windows per wave), 3 two row tiles per wave, 4 the same on 16 x 16 x 32 MFMAs, 5 epilogue under the matrix phase
  EncFused q;
  EncWeights weights;
  size_t lds;
  int grid;
  bool wide_fits;    // the 32-window row-layout kernel takes this shape: the forward half of "may the gate stash be fp16"
};
static inline EncFwdPlan enc_plan_fwd(const lfi_enc_desc* d, bool masked, bool stashed, bool aligned) {
  EncFwdPlan p = {};
  if (d->lstm || !enc_fused_shape(d->hid, &p.q)) return p;
  const EncFused& q = p.q;
  const long F = (long)d->N * d->B;
  const int R2 = 2 * q.R;
  const bool x3 = d->precision == 1;
  // row-layout epilogue (16-byte accesses): needs 4-float granular rows everywhere it vectorises
  const bool wide = enc_wide_enabled() && x3 && d->hid % 4 == 0 && d->ldcond % 4 == 0 && d->col % 4 == 0 && aligned;
  p.wide_fits = wide && enc_fwd_wide_lds(q, d->hist, masked) <= 80 * 1024;
  // two row tiles per wave, one workgroup per CU: half the L2 -> CU weight stream per window; taken when its workgroups still cover
  // the chip (LFI_ENC_R64=0 keeps the 32-window kernel)
  const bool take64 = wide && enc_r64_enabled() && enc_fwd_r64_lds(q, d->hist, masked) <= 160 * 1024 && lfi_cdiv(F, R2) >= 128;
  const bool m16 = take64 && q.Kp == 256 && q.ncg * 64 == q.Jp && enc_m16_enabled();
  const bool t16 = m16 && d->hid == 256 && R2 == 64 && enc_fwd_t16_lds(d->hist, masked) <= 160 * 1024 && enc_t16_mode() >= (stashed ? 2 : 1);
  p.variant = t16 ? 5 : m16 ? 4 : take64 ? 3 : p.wide_fits ? 2 : 1;
  // (the 64-window kernels on the 16 x 16 x 32 shape want their own fragment order)
  p.weights = !x3 ? ENC_W_PAD : (p.variant >= 4 ? ENC_W_FRAG16 : ENC_W_FRAG);
  p.lds = p.variant == 5 ? enc_fwd_t16_lds(d->hist, masked)
        : p.variant >= 3 ? enc_fwd_r64_lds(q, d->hist, masked)
        : p.variant == 2 ? enc_fwd_wide_lds(q, d->hist, masked) : enc_fwd_fused_lds(q, x3);
  p.grid = lfi_cdiv(F, p.variant >= 3 ? R2 : q.R);
  return p;
}

struct EncBwdPlan {
  int variant;         // 0 unfused (hid > 256) or LSTM, 1 accumulator-layout fused (exact f32, whatever the engine's GEMM mode),
                       // 2 row-layout (bf16x3 recurrence), 3 row-layout with two row tiles per wave
  EncFused q;
  EncWeights weights;
  size_t lds;
  int grid;
  int rows_per_wg;     // windows per workgroup: bias_part holds one row per (workgroup, row group)
  bool grads_bf16;     // dgi / dgh are left as bf16 arrays (same shapes, half the bytes): the row-layout kernels in two-product mode. Its
                       // consumers - the dW_hh product (A operand rounded to bf16) and the window scatter - then read bf16
  bool stash_f16_ok;   // a row-layout kernel takes the shape: the backward half of "may the gate stash be fp16"
};
// lddcond: the leading dimension of the d(cond) that is passed in (the queries know d->ldcond only and pass that)
static inline EncBwdPlan enc_plan_bwd(const lfi_enc_desc* d, int lddcond, bool aligned) {
  EncBwdPlan p = {};
  if (d->lstm || !enc_fused_shape(d->hid, &p.q)) return p;
  const EncFused& q = p.q;
  const long F = (long)d->N * d->B;
  // the row-layout kernels (16-byte accesses), but for the leading dimension of d(cond)
  const bool rows_ok = d->precision == 1 && enc_wide_bwd_enabled() && d->hid % 4 == 0 && d->col % 4 == 0 && enc_bwd_wide_lds(q) <= 80 * 1024;
  const bool own_ld = lddcond == d->ldcond;
  p.stash_f16_ok = rows_ok && d->ldcond % 4 == 0;
  p.grads_bf16 = d->bwd_two_products && own_ld && p.stash_f16_ok;
  // bf16x3 recurrence: the row-layout kernels only. What they do not take (LFI_ENC_WIDE_BWD=0, hid not a multiple of 4, unaligned
  // buffers) runs the exact-f32 accumulator-layout kernel, whatever the engine's GEMM mode (see enc_gru_bwd_fused_kernel)
  const bool wide = rows_ok && lddcond % 4 == 0 && aligned;
  // two row tiles per wave, one workgroup per CU: when its workgroups still cover the chip
  const bool r64 = wide && own_ld && enc_r64_enabled() && enc_bwd_r64_lds(q) <= 160 * 1024 && lfi_cdiv(F, 2 * q.R) >= 128;
  p.variant = r64 ? 3 : wide ? 2 : 1;
  p.weights = wide ? ENC_W_FRAG : ENC_W_PAD;
  p.rows_per_wg = r64 ? 2 * q.R : q.R;
  p.lds = r64 ? enc_bwd_r64_lds(q) : wide ? enc_bwd_wide_lds(q) : enc_bwd_fused_lds(q);
  p.grid = lfi_cdiv(F, p.rows_per_wg);
  return p;
}
