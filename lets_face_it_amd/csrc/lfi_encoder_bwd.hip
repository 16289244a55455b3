// Window encoders, backward: the per-step gate-derivative kernels of the unfused GRU / LSTM loops, the three fused BPTT kernels,
// the window scatter, the bias fold and their entry points (see lfi_encoder.hip for the scheme; the forward pass is
// lfi_encoder_fwd.hip).
#include "lfi_encoder_common.h"

namespace {

// Gate derivatives of step s. dh_in: F x hid gradient w.r.t. h_s (null at s = hist-1: taken from dcond, both halves);
// writes dgi[s], dgh[s] and the carried part dh_out = dh * z (the GEMM then adds dgh_s W_hh onto it).
__global__ __launch_bounds__(256) void enc_gate_bwd_kernel(EncArgs a, int s, const float* __restrict__ dh_in,
                                                           float* __restrict__ dh_out) {
  const int hid = a.hid, G3 = 3 * hid;
  const long total = (long)a.F * hid;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int w = (int)(idx / hid), j = (int)(idx - (long)w * hid);
    float dhn;
    if (dh_in) dhn = dh_in[idx];
    else {
      const float* dc = a.dcond + (long)w * a.lddcond + a.col;
      dhn = a.dup ? dc[j] + dc[hid + j] : dc[j];
    }
    const long sw = (long)s * a.F + w;
    const float* gs = a.gates + sw * 4 * hid;
    const float rr = gs[j], uu = gs[hid + j], nn = gs[2 * hid + j], ghn = gs[3 * hid + j];
    const float hp = s > 0 ? a.hseq[((long)(s - 1) * a.F + w) * hid + j] : 0.0f;
    const float du = dhn * (hp - nn);
    const float dn = dhn * (1.0f - uu);
    const float dan = dn * (1.0f - nn * nn);
    const float dau = du * uu * (1.0f - uu);
    const float dar = dan * ghn * rr * (1.0f - rr);
    float* gi = a.dgi + sw * G3;
    gi[j] = dar; gi[hid + j] = dau; gi[2 * hid + j] = dan;
    float* gh = a.dgh + sw * G3;
    gh[j] = dar; gh[hid + j] = dau; gh[2 * hid + j] = dan * rr;
    if (dh_out) dh_out[idx] = dhn * uu;
  }
}

// Gate derivatives of LSTM step s. dh_in / dc_in: F x hid gradients w.r.t. h_s / c_s carried from step s + 1 (null at the last
// step: d h from dcond, d c = 0). Writes dgi[s] = dgh[s] (the pre-activation is a plain sum of both sides), the carried d c
// and zeroes dh_out, onto which the GEMM dgh_s W_hh then accumulates d h_{s-1}.
__global__ __launch_bounds__(256) void enc_lstm_gate_bwd_kernel(EncArgs a, int s, const float* __restrict__ dh_in,
                                                                const float* __restrict__ dc_in, float* __restrict__ dh_out,
                                                                float* __restrict__ dc_out) {
  const int hid = a.hid, G = 4 * hid;
  const long total = (long)a.F * hid;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int w = (int)(idx / hid), j = (int)(idx - (long)w * hid);
    float dhn;
    if (dh_in) dhn = dh_in[idx];
    else {
      const float* dc = a.dcond + (long)w * a.lddcond + a.col;
      dhn = a.dup ? dc[j] + dc[hid + j] : dc[j];
    }
    const long sw = (long)s * a.F + w;
    const float* gs = a.gates + sw * 5 * hid;
    const float ii = gs[j], ff = gs[hid + j], gg = gs[2 * hid + j], oo = gs[3 * hid + j], c = gs[4 * hid + j];
    const float cp = s > 0 ? a.gates[(((long)(s - 1) * a.F + w) * 5 + 4) * hid + j] : 0.0f;
    const float tc = tanhf_(c);
    const float dc = dhn * oo * (1.0f - tc * tc) + (dc_in ? dc_in[idx] : 0.0f);
    const float d0 = dc * gg * ii * (1.0f - ii);
    const float d1 = dc * cp * ff * (1.0f - ff);
    const float d2 = dc * ii * (1.0f - gg * gg);
    const float d3 = dhn * tc * oo * (1.0f - oo);
    float* gi = a.dgi + sw * G;
    float* gh = a.dgh + sw * G;
    gi[j] = d0; gi[hid + j] = d1; gi[2 * hid + j] = d2; gi[3 * hid + j] = d3;
    gh[j] = d0; gh[hid + j] = d1; gh[2 * hid + j] = d2; gh[3 * hid + j] = d3;
    if (dh_out) { dh_out[idx] = 0.0f; dc_out[idx] = dc * ff; }
  }
}

// dXp[b*T + p][c] = sum_{s} mask[w(n,b)][s] * dgi[s][w][c],  n = p - pos0 - s in [0, N)
// One workgroup per frame row; every (step, window) row of dgi is read exactly once over the grid (HBM-bound stream).
// Branch-free: steps whose window falls outside [0, N) read row 0 with weight 0, so eight 16-byte loads per thread are
// in flight at a time.
__global__ __launch_bounds__(256) void enc_scatter_kernel(EncArgs a, float* __restrict__ dXp) {
  const int G3 = a.G;   // 3 * hid (GRU) or 4 * hid (LSTM)
  const int row = blockIdx.x;  // b*T + p
  const int b = row / a.T, p = row - b * a.T;
  const int pos0 = a.start - a.hist + 1;
  const bool vec = (G3 & 3) == 0 && (a.hid & 3) == 0;
  const int nvec = vec ? G3 >> 2 : 0;
  for (int c4 = threadIdx.x; c4 < nvec; c4 += 256) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < a.hist; s0 += 8) {
      f32x4 v[8];
      float wgt[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int s = s0 + u;
        const int n = p - pos0 - s;
        const bool ok = s < a.hist && n >= 0 && n < a.N;
        const long w = ok ? (long)n * a.B + b : 0;
        const int sc = ok ? s : 0;
        wgt[u] = ok ? (a.mask ? a.mask[w * a.hist + sc] : 1.0f) : 0.0f;
        const long r = (long)sc * a.F + w;
        if (a.g16) {   // bf16 stash (compact): 4 values = one 8-byte load
          const __bf16* gh16 = reinterpret_cast<const __bf16*>(a.dgh), *gi16 = reinterpret_cast<const __bf16*>(a.dgi);
          const __bf16* src = 4 * c4 < 2 * a.hid ? gh16 + r * G3 + 4 * c4 : gi16 + r * a.hid + (4 * c4 - 2 * a.hid);
          const uint2 w2 = *reinterpret_cast<const uint2*>(src);
          v[u] = f32x4{__builtin_bit_cast(float, w2.x << 16), __builtin_bit_cast(float, w2.x & 0xffff0000u),
                       __builtin_bit_cast(float, w2.y << 16), __builtin_bit_cast(float, w2.y & 0xffff0000u)};
        } else {
          const float* src = !a.compact ? a.dgi + r * G3 + 4 * c4
                                        : (4 * c4 < 2 * a.hid ? a.dgh + r * G3 + 4 * c4 : a.dgi + r * a.hid + (4 * c4 - 2 * a.hid));
          v[u] = *reinterpret_cast<const f32x4*>(src);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += wgt[u] * v[u];
    }
    *reinterpret_cast<f32x4*>(dXp + (long)row * G3 + 4 * c4) = acc;
  }
  if (!vec)
    for (int c = threadIdx.x; c < G3; c += 256) {
      float acc = 0.0f;
      for (int s = 0; s < a.hist; ++s) {
        const int n = p - pos0 - s;
        if (n < 0 || n >= a.N) continue;
        const long w = (long)n * a.B + b;
        const float mk = a.mask ? a.mask[w * a.hist + s] : 1.0f;
        const long r = (long)s * a.F + w;
        acc += mk * (!a.compact ? a.dgi[r * G3 + c] : (c < 2 * a.hid ? a.dgh[r * G3 + c] : a.dgi[r * a.hid + (c - 2 * a.hid)]));
      }
      dXp[(long)row * G3 + c] = acc;
    }
}

// The same sums for the bf16 compact stash with hid % 8 == 0: 8 values per thread through ONE 16-byte load, and as many frame rows
// per workgroup as 256 threads hold (3 hid / 8 threads per row). Same products, same order over s: bit-identical to the kernel above.
typedef unsigned su32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void enc_scatter16_kernel(EncArgs a, float* __restrict__ dXp, int rows, int cpr, int rpw) {
  const int rl = threadIdx.x / cpr, c = threadIdx.x - rl * cpr;
  const int row = blockIdx.x * rpw + rl;
  if (rl >= rpw || row >= rows) return;
  const int b = row / a.T, p = row - b * a.T;
  const int pos0 = a.start - a.hist + 1;
  const int c8 = 8 * c;
  const bool hh = c8 < 2 * a.hid;
  const __bf16* base = hh ? reinterpret_cast<const __bf16*>(a.dgh) + c8 : reinterpret_cast<const __bf16*>(a.dgi) + (c8 - 2 * a.hid);
  const long ldr = hh ? a.G : a.hid;
  constexpr int UB = 8;   // loads in flight per thread (4 / 8 / 12 and non-temporal loads measured alike: tools/scatter_probe.py)
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < a.hist; s0 += UB) {
    su32x4 v[UB];
    float wgt[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int s = s0 + u;
      const int n = p - pos0 - s;
      const bool ok = s < a.hist && n >= 0 && n < a.N;
      const long w = ok ? (long)n * a.B + b : 0;
      const int sc = ok ? s : 0;
      wgt[u] = ok ? (a.mask ? a.mask[w * a.hist + sc] : 1.0f) : 0.0f;
      const su32x4* src = reinterpret_cast<const su32x4*>(base + ((long)sc * a.F + w) * ldr);
      v[u] = *src;
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const unsigned q[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[2 * e] += wgt[u] * __builtin_bit_cast(float, q[e] << 16);
        acc[2 * e + 1] += wgt[u] * __builtin_bit_cast(float, q[e] & 0xffff0000u);
      }
    }
  }
  float* dst = dXp + (long)row * a.G + c8;
  *reinterpret_cast<f32x4*>(dst) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// BPTT of the same block of windows in one workgroup: dh lives in the accumulator layout of the wave that owns
// (rows, hidden) tile (rg, cg); per step the gate derivatives are taken in registers, written to dgi / dgh (the
// deferred weight-gradient GEMMs read those) and fed gate by gate through LDS as the A operand of
// dh_{s-1} = dgh_s W_hh + dh_s * u   (K = 3 hid, B = W_hh rows streamed from L2).
// Round 6: this kernel is the exact-f32 form only. Its bf16x3 twin (the same layout with three bf16 products per k-step) was the
// fallback behind LFI_ENC_WIDE_BWD=0 and for shapes the row-layout kernels do not take; built with the SLP vectoriser it returned
// different bits on 19 of 19 repeat launches (spill reloads inside its counted-vmcnt product loops, profiles/round5_slp_chase.md;
// the instruction at fault was never found). A kernel that is nondeterministic under a legal compiler flag does not ship: it is
// gone, and those cases run this kernel instead (bit-exact fp32 FMA chains on v_mfma_f32_32x32x2_f32 - slower, never wrong).
// One workgroup per CU's worth of registers (launch bound 1, not 2): at two it fits without the SLP vectoriser (230 VGPRs) but spills
// 26 with it - and the spilling SLP build of THIS form turned out to differ between whole passes as well (p2_face, batch 256:
// profiles/round6_determinism.txt, first run), as its bf16x3 twin had: spill code inside these product loops is what goes wrong, in
// whichever arithmetic. With the whole register file it never spills, in either build.
__global__ __launch_bounds__(ENC_NT, 1) void enc_gru_bwd_fused_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, ldk = q.R + 1, Jp = q.Jp;
  const int jb = cg * 64 + l31;
  const bool jok0 = jb < hid, jok1 = jb + 32 < hid;
  const int wbase = blockIdx.x * q.R;
  float* Dls = enc_smem;  // one gate's derivatives: element (row, k) at Dls[k * ldk + row], rows k >= hid stay zero
  for (int i = tid; i < q.Kp * ldk; i += ENC_NT) Dls[i] = 0.0f;
  // roww[row] = w * hid * 4 (rows past F clamped), live[row] = 1 for real windows (bias sums skip the clamped duplicates)
  unsigned* roww = reinterpret_cast<unsigned*>(enc_smem + q.Kp * ldk);
  float* rlive = reinterpret_cast<float*>(roww + q.R);
  for (int i = tid; i < q.R; i += ENC_NT) {
    roww[i] = (unsigned)min(wbase + i, a.F - 1) * (unsigned)(hid * 4);
    rlive[i] = wbase + i < a.F ? 1.0f : 0.0f;
  }
  const int boff = half * Jp + jb;
  const int aoff = half * ldk + rg * 32 + l31;
  const int nkp = q.Kp >> 1;

  f32x16 dh[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int w = min(wbase + enc_rowl(rg, r, half), a.F - 1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = jb + 32 * t;
      float v = 0.0f;
      if (j < hid) {
        const float* dc = a.dcond + (long)w * a.lddcond + a.col;
        v = a.dup ? dc[j] + dc[hid + j] : dc[j];
      }
      dh[t][r] = v;
    }
  }
  __syncthreads();
  // bias gradients db_ih = sum (dar, dau, dan), db_hh = sum (dar, dau, dan*r) over windows and steps: every lane sums its own
  // column over its rows and all steps in a fixed order; the column sums of the per-(workgroup, row group) partials finish it
  float bsum[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  for (int s = a.hist - 1; s >= 0; --s) {
    float dg[2][2][16];  // gates 1 and 2; gate 0 goes straight into the LDS operand image (free since the last barrier)
    f32x16 acc[2];
    const float hp_on = s > 0 ? 1.0f : 0.0f;
    const int sp = s > 0 ? s - 1 : 0;
    // uniform buffer resources of this step + 32-bit per-lane byte offsets; lane coordinates laundered so that the
    // per-register address arithmetic is not hoisted out of the step loop (see the forward kernel)
    int halfv = half, jv = jb;
    asm volatile("" : "+v"(halfv), "+v"(jv));
    const enc_rsrc bgs = enc_buf(a.gates + (long)s * a.F * 4 * hid, (long)a.F * hid * 16);
    const enc_rsrc bhp = enc_buf(a.hseq + (long)sp * a.F * hid, (long)a.F * hid * 4);
    // d(pre-activation) on the input side differs from the hidden side only in the n gate (dan vs dan * r): dgi keeps that
    // one block ([hist][F][hid]); the scatter and the bias sums take d r, d z from dgh - a third less to write
    const enc_rsrc bgi = enc_buf(a.dgi + (long)s * a.F * hid, (long)a.F * hid * 4);
    const enc_rsrc bgh = enc_buf(a.dgh + (long)s * a.F * G3, (long)a.F * G3 * 4);
    const unsigned h4 = (unsigned)hid * 4u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = jv + 32 * t;
      if (j < hid) {
        const unsigned j4 = (unsigned)j * 4u;
#pragma unroll
        for (int rh = 0; rh < 2; ++rh) {
          float gr[8], gu[8], gn[8], gg[8], hp[8], live[8];
          unsigned wo[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int rl = enc_rowl(rg, rh * 8 + e, halfv);
            wo[e] = roww[rl];
            live[e] = rlive[rl];
            const unsigned go = 4u * wo[e] + j4;
            gr[e] = enc_ld_stream(bgs, go, 0); gu[e] = enc_ld_stream(bgs, go, h4); gn[e] = enc_ld_stream(bgs, go, 2 * h4);
            gg[e] = enc_ld_stream(bgs, go, 3 * h4);
            hp[e] = enc_ld_stream(bhp, wo[e] + j4, 0);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int r = rh * 8 + e;
            const float rr = gr[e], uu = gu[e], nn = gn[e], ghn = gg[e];
            const float dhn = dh[t][r];
            const float du = dhn * (hp[e] * hp_on - nn);
            const float dn = dhn * (1.0f - uu);
            const float dan = dn * (1.0f - nn * nn);
            const float dau = du * uu * (1.0f - uu);
            const float dar = dan * ghn * rr * (1.0f - rr);
            const float danr = dan * rr;
            const unsigned o = 3u * wo[e] + j4;
            enc_st(dan, bgi, wo[e] + j4, 0);
            enc_st(dar, bgh, o, 0); enc_st(dau, bgh, o, h4); enc_st(danr, bgh, o, 2 * h4);
            dg[0][t][r] = dau; dg[1][t][r] = danr;
            if (s > 0) {
              const int rl = enc_rowl(rg, r, halfv);
              Dls[j * ldk + rl] = dar;
            }
            acc[t][r] = dhn * uu;
            bsum[0][t] += live[e] * dar; bsum[1][t] += live[e] * dau; bsum[2][t] += live[e] * dan; bsum[3][t] += live[e] * danr;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { dg[0][t][r] = 0.f; dg[1][t][r] = 0.f; acc[t][r] = 0.f; }
      }
    }
    if (s == 0) break;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      if (g > 0)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = enc_rowl(rg, r, halfv);
        if (jok0) Dls[jv * ldk + rl] = dg[g - 1][0][r];
        if (jok1) Dls[(jv + 32) * ldk + rl] = dg[g - 1][1][r];
      }
      __syncthreads();
      {
        float a0[ENC_KC], a1[ENC_KC], b0[ENC_KC][2], b1[ENC_KC][2];
        const float* __restrict__ wg = q.wpad + (long)g * q.Kp * Jp;
        auto load = [&](int kp0, float (&av)[ENC_KC], float (&bv)[ENC_KC][2]) {
          const float* __restrict__ wk = wg + (long)kp0 * 2 * Jp;  // uniform base, 32-bit per-lane offset: saddr loads
          const float* ak = Dls + kp0 * 2 * ldk;
#pragma unroll
          for (int u = 0; u < ENC_KC; ++u) {
            av[u] = ak[u * 2 * ldk + aoff];
            const float* __restrict__ wu = wk + u * 2 * Jp;  // uniform
            bv[u][0] = wu[(unsigned)boff];
            bv[u][1] = (wu + 32)[(unsigned)boff];
          }
        };
        auto mma = [&](const float (&av)[ENC_KC], const float (&bv)[ENC_KC][2]) {
#pragma unroll
          for (int u = 0; u < ENC_KC; ++u) {
            acc[0] = mfma32(av[u], bv[u][0], acc[0]);
            acc[1] = mfma32(av[u], bv[u][1], acc[1]);
          }
        };
        load(0, a0, b0);
        int kp = 0;
        for (; kp + 2 * ENC_KC < nkp; kp += 2 * ENC_KC) {
          load(kp + ENC_KC, a1, b1);
          __builtin_amdgcn_sched_barrier(0);
          mma(a0, b0);
          load(kp + 2 * ENC_KC, a0, b0);
          __builtin_amdgcn_sched_barrier(0);
          mma(a1, b1);
        }
        load(kp + ENC_KC, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        mma(a1, b1);
      }
      __syncthreads();  // before the next gate overwrites Dls
    }
    dh[0] = acc[0];
    dh[1] = acc[1];
  }
  if (a.bias_part) {
    float* bp = a.bias_part + ((long)blockIdx.x * (ENC_NW / q.ncg) + rg) * 4 * hid;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float v = bsum[qq][t] + __shfl_xor(bsum[qq][t], 32, 64);
        const int j = jb + 32 * t;
        if (half == 0 && j < hid) bp[qq * hid + j] = v;
      }
  }
}

// ---- BPTT with the row-layout epilogue (the counterpart of enc_gru_fwd_wide_kernel; bf16x3 products).
// The accumulator-layout kernel above moves every stash value with its own 4-byte access (gates r, z, n, W_hn h and h_{s-1}
// in; d n, d r, d z, d n * r out: 9 wave instructions per (row, 32 columns) and step) and writes the three gate images for
// the MFMA A operand with 2-byte LDS stores (192 per lane and step). Here d h comes out of the accumulators through the
// wave-private transpose tile, a lane owns 4 consecutive hidden units of 8 windows, everything above is a 16-byte access,
// the images are written 8 bytes at a time, and the tile region doubles as a SECOND image pair while no transpose is in
// flight, so that the r and z gate products run back to back: four workgroup barriers per step instead of six.
// A2 (lfi_enc_desc.bwd_two_products): two bf16 products per k-step instead of three - the A operand, d(gate pre-activations),
// enters rounded to bf16 (its lo image is neither written nor read, the a_lo * w_hi MFMA not issued), as the backward GEMM
// classes do from 8192 frames up (profiles/precision_sweep_b256.md: this recurrence is one of them, class enc_bptt).
template <bool A2, bool S16>
__global__ __launch_bounds__(ENC_NT, 2) void enc_gru_bwd_wide_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, Jp = q.Jp;
  const int wbase = blockIdx.x * q.R;
  const int ldx = q.Kp + 8;
  const int img = q.R * ldx;                                   // bf16 elements of one image
  __bf16* Xhi = reinterpret_cast<__bf16*>(enc_smem);
  __bf16* Xlo = Xhi + img;
  float* Treg = reinterpret_cast<float*>(Xlo + img);           // transpose tiles | second image pair (Yhi, Ylo)
  const int tfloats = max(ENC_NW * 32 * ENC_TP, img);          // (2 * img bf16 = img floats)
  float* T = Treg + wave * (32 * ENC_TP);
  __bf16* Yhi = reinterpret_cast<__bf16*>(Treg);
  __bf16* Ylo = Yhi + img;
  unsigned* roww = reinterpret_cast<unsigned*>(Treg + tfloats);
  float* rlive = reinterpret_cast<float*>(roww + q.R);
  for (int i = tid; i < img; i += ENC_NT) { Xhi[i] = (__bf16)0.0f; Xlo[i] = (__bf16)0.0f; }
  for (int i = tid; i < tfloats; i += ENC_NT) Treg[i] = 0.0f;   // (also the k padding of the second image pair)
  for (int i = tid; i < q.R; i += ENC_NT) {
    roww[i] = (unsigned)min(wbase + i, a.F - 1) * (unsigned)(hid * 4);
    rlive[i] = wbase + i < a.F ? 1.0f : 0.0f;
  }
  const int rsub = lane >> 4, c4 = (lane & 15) * 4;
  const int j0 = cg * 64 + c4;
  const bool jok = j0 < hid;
  const unsigned h4 = (unsigned)hid * 4u;
  const enc_rsrc bdc = enc_buf(a.dcond, ((long)a.F * a.lddcond) * 4);
  f32x4 dhu[8];          // d h_s * z_s: the part of d h_{s-1} that does not go through W_hh (row layout)
  f32x4 bsum[4];         // column sums of d r, d z, d n, d n * r over this lane's rows and all steps
#pragma unroll
  for (int i = 0; i < 8; ++i) dhu[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) bsum[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  __syncthreads();

  for (int s = a.hist - 1; s >= 0; --s) {
    int rsv = rsub, cv = c4, jv = j0;
    asm volatile("" : "+v"(rsv), "+v"(cv), "+v"(jv));
    const unsigned j4 = (unsigned)jv * 4u, oob = jv < hid ? 0u : 0x80000000u;
    float* Trow = T + rsv * ENC_TP + cv;
    float* Tacc = T + (4 * half) * ENC_TP + l31;
    // ---- d h_s in the row layout
    f32x4 dh[8];
    if (s == a.hist - 1) {
      const unsigned cb = (unsigned)a.col * 4u + j4 + oob;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned wrow = (roww[rg * 32 + 4 * i + rsv] / h4) * (unsigned)(a.lddcond * 4);
        dh[i] = enc_ld4(bdc, wrow + cb, 0);
        if (a.dup) dh[i] += enc_ld4(bdc, wrow + cb, h4);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Tacc[((r & 3) + 8 * (r >> 2)) * ENC_TP + 32 * t] = acc[t][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 8; ++i) dh[i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP) + dhu[i];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __syncthreads();   // B0: every wave is done with its transpose tile (the second image pair overlays those) and with the
                       // previous step's n-gate product (which read the first image pair)
    if (q.Kp > hid) {   // the transposes left accumulator bits in the second pair's k padding: NaN patterns x 0 would poison the product
      const int pad = q.Kp - hid;
      for (int i = tid; i < q.R * pad; i += ENC_NT) {
        const int rl = i / pad, c = hid + (i - rl * pad);
        Yhi[rl * ldx + c] = (__bf16)0.0f; Ylo[rl * ldx + c] = (__bf16)0.0f;
      }
    }
    const int sp = s > 0 ? s - 1 : 0;
    const float hp_on = s > 0 ? 1.0f : 0.0f;
    const enc_rsrc bgs = S16 ? enc_buf(reinterpret_cast<const _Float16*>(a.gates) + (long)s * a.F * 4 * hid, (long)a.F * hid * 8)
                             : enc_buf(a.gates + (long)s * a.F * 4 * hid, (long)a.F * hid * 16);
    const enc_rsrc bhp = enc_buf(a.hseq + (long)sp * a.F * hid, (long)a.F * hid * 4);
    // A2: the gradient stash leaves as bf16 (what its consumers - the dW_hh product's rounded A operand, the window scatter in
    // front of dW_ih's - use of it): half the bytes out here and half the bytes into both of them
    const enc_rsrc bgi = A2 ? enc_buf(reinterpret_cast<const __bf16*>(a.dgi) + (long)s * a.F * hid, (long)a.F * hid * 2)
                            : enc_buf(a.dgi + (long)s * a.F * hid, (long)a.F * hid * 4);
    const enc_rsrc bgh = A2 ? enc_buf(reinterpret_cast<const __bf16*>(a.dgh) + (long)s * a.F * G3, (long)a.F * G3 * 2)
                            : enc_buf(a.dgh + (long)s * a.F * G3, (long)a.F * G3 * 4);
    f32x4 danr[8];
#pragma unroll
    for (int ih = 0; ih < 2; ++ih) {
      f32x4 gr[4], gu[4], gn[4], gg[4], hp[4];
      unsigned wo[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rl = rg * 32 + 4 * (4 * ih + u) + rsv;
        wo[u] = roww[rl];
        if (S16) {   // fp16 stash, [window][unit][r, z, n, W_hn h]: two 16-byte loads hold this lane's four units
          const unsigned go = 2u * (wo[u] + j4) + oob;
          const enc_u32x4 p0 = __builtin_amdgcn_raw_buffer_load_b128(bgs, go, 0, 2), p1 = __builtin_amdgcn_raw_buffer_load_b128(bgs, go, 16, 2);
          const f32x4 u0 = enc_unpack_gates(p0[0], p0[1]), u1 = enc_unpack_gates(p0[2], p0[3]);
          const f32x4 u2 = enc_unpack_gates(p1[0], p1[1]), u3 = enc_unpack_gates(p1[2], p1[3]);
          gr[u] = f32x4{u0[0], u1[0], u2[0], u3[0]}; gu[u] = f32x4{u0[1], u1[1], u2[1], u3[1]};
          gn[u] = f32x4{u0[2], u1[2], u2[2], u3[2]}; gg[u] = f32x4{u0[3], u1[3], u2[3], u3[3]};
        } else {
          const unsigned go = 4u * wo[u] + j4 + oob;
          gr[u] = enc_ld4s(bgs, go, 0); gu[u] = enc_ld4s(bgs, go, h4); gn[u] = enc_ld4s(bgs, go, 2 * h4); gg[u] = enc_ld4s(bgs, go, 3 * h4);
        }
        hp[u] = enc_ld4s(bhp, wo[u] + j4 + oob, 0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = 4 * ih + u;
        const int rl = rg * 32 + 4 * i + rsv;
        const float live = rlive[rl];
        f32x4 dan, dau, dar, dnr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float rr = gr[u][e], uu = gu[u][e], nn = gn[u][e], ghn = gg[u][e];
          const float dhn = dh[i][e];
          const float du = dhn * (hp[u][e] * hp_on - nn);
          const float dn = dhn * (1.0f - uu);
          dan[e] = dn * (1.0f - nn * nn);
          dau[e] = du * uu * (1.0f - uu);
          dar[e] = dan[e] * ghn * rr * (1.0f - rr);
          dnr[e] = dan[e] * rr;
          dhu[i][e] = dhn * uu;
        }
        if (A2) {
          const unsigned j2 = j4 >> 1, h2 = h4 >> 1;
          enc_st2h(dan, bgi, (wo[u] >> 1) + j2 + oob, 0);
          const unsigned o = 3u * (wo[u] >> 1) + j2 + oob;
          enc_st2h(dar, bgh, o, 0); enc_st2h(dau, bgh, o, h2); enc_st2h(dnr, bgh, o, 2 * h2);
        } else {
          enc_st4(dan, bgi, wo[u] + j4 + oob, 0);
          const unsigned o = 3u * wo[u] + j4 + oob;
          enc_st4(dar, bgh, o, 0); enc_st4(dau, bgh, o, h4); enc_st4(dnr, bgh, o, 2 * h4);
        }
        bsum[0] += live * dar; bsum[1] += live * dau; bsum[2] += live * dan; bsum[3] += live * dnr;
        danr[i] = dnr;
        if (s > 0 && jok) {   // gate images for the products: d r -> first pair, d z -> second pair
          uint2 h, l;
          split2(dar[0], dar[1], &h.x, &l.x); split2(dar[2], dar[3], &h.y, &l.y);
          *reinterpret_cast<uint2*>(Xhi + rl * ldx + jv) = h;
          if (!A2) *reinterpret_cast<uint2*>(Xlo + rl * ldx + jv) = l;
          split2(dau[0], dau[1], &h.x, &l.x); split2(dau[2], dau[3], &h.y, &l.y);
          *reinterpret_cast<uint2*>(Yhi + rl * ldx + jv) = h;
          if (!A2) *reinterpret_cast<uint2*>(Ylo + rl * ldx + jv) = l;
        }
      }
    }
    if (s == 0) break;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    auto product = [&](int g, const __bf16* Ih, const __bf16* Il) {   // acc += image_g (R x hid) W_hh[g] (hid x hid)
      const int nkt = q.Kp >> 4, nct = Jp >> 5;
      const __bf16* xh = Ih + (rg * 32 + l31) * ldx + 8 * half;
      const __bf16* xl = Il + (rg * 32 + l31) * ldx + 8 * half;
      ebf16x8 ah0, al0, ah1, al1;
      EncFrag f0[2][2], f1[2][2];  // [t][plane]
      auto load = [&](int kt, ebf16x8& ah, ebf16x8& al, EncFrag (&f)[2][2]) {
        ah = *reinterpret_cast<const ebf16x8*>(xh + kt * 16);
        if (!A2) al = *reinterpret_cast<const ebf16x8*>(xl + kt * 16);
        else al = ah;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const uint4* __restrict__ wf = q.wfrag + ((long)((g * nkt + ENC_WKT(kt)) * nct + cg * 2 + t) * 2) * 64;  // uniform
          f[t][0].u = wf[(unsigned)lane];
          f[t][1].u = (wf + 64)[(unsigned)lane];
        }
      };
      auto mma = [&](const ebf16x8& ah, const ebf16x8& al, const EncFrag (&f)[2][2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (!A2) acc[t] = ENC_MFMA(al, f[t][0].v, acc[t], 0, 0, 0);
          acc[t] = ENC_MFMA(ah, f[t][1].v, acc[t], 0, 0, 0);
          acc[t] = ENC_MFMA(ah, f[t][0].v, acc[t], 0, 0, 0);
        }
      };
      load(0, ah0, al0, f0);
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {   // unconditional loads (see the forward kernel)
        load(kt + 1, ah1, al1, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah0, al0, f0);
        load(kt + 2, ah0, al0, f0);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah1, al1, f1);
      }
      if (kt + 1 < nkt) {
        load(kt + 1, ah1, al1, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah0, al0, f0);
        mma(ah1, al1, f1);
      } else {
        mma(ah0, al0, f0);
      }
    };
    __syncthreads();   // B1: both image pairs complete
    product(0, Xhi, Xlo);
    product(1, Yhi, Ylo);
    __syncthreads();   // B2: every wave has read the first pair
    if (jok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl = rg * 32 + 4 * i + rsv;
        uint2 h, l;
        split2(danr[i][0], danr[i][1], &h.x, &l.x); split2(danr[i][2], danr[i][3], &h.y, &l.y);
        *reinterpret_cast<uint2*>(Xhi + rl * ldx + jv) = h;
        if (!A2) *reinterpret_cast<uint2*>(Xlo + rl * ldx + jv) = l;
      }
    }
    __syncthreads();   // B3
    product(2, Xhi, Xlo);
  }
  if (a.bias_part && jok) {
    float* bp = a.bias_part + ((long)blockIdx.x * (ENC_NW / q.ncg) + rg) * 4 * hid;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      f32x4 v = bsum[qq];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] += __shfl_xor(v[e], 16, 64);
        v[e] += __shfl_xor(v[e], 32, 64);
      }
      if (rsub == 0) *reinterpret_cast<f32x4*>(bp + qq * hid + j0) = v;
    }
  }
}

// ---- BPTT with two 32-row tiles per wave (64 windows per row group), one workgroup per CU: the counterpart of
// enc_gru_fwd_r64_kernel (same reasoning: the d gates x W_hh products keep their MFMA work, every weight fragment feeds both row
// tiles). Same phases and barriers as enc_gru_bwd_wide_kernel, every row-layout phase run once per row tile. Measured (p2_face
// shape, two products, fp16 gate stash): 0.57 -> 0.52 ms per launch.
template <bool A2, bool S16>
__global__ __launch_bounds__(ENC_NT, 1) void enc_gru_bwd_r64_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, Jp = q.Jp;
  const int R2 = 2 * q.R;
  const int wbase = blockIdx.x * R2;
  const int ldx = q.Kp + 8;
  const int img = R2 * ldx;                                     // bf16 elements of one image
  __bf16* Xhi = reinterpret_cast<__bf16*>(enc_smem);
  __bf16* Xlo = Xhi + img;
  float* Treg = reinterpret_cast<float*>(Xlo + img);           // transpose tiles | second image pair (Yhi, Ylo)
  const int tfloats = max(ENC_NW * 2 * 32 * ENC_TP, img);      // (2 * img bf16 = img floats)
  float* Tw = Treg + wave * (2 * 32 * ENC_TP);
  __bf16* Yhi = reinterpret_cast<__bf16*>(Treg);
  __bf16* Ylo = Yhi + img;
  // A2 (two products: the hi pieces of the gate derivatives only): the first pair's lo image is never written - its space holds the
  // THIRD gate's image (d n * r), so the three products run back to back: no 64-register copy of d n * r across the first two, no
  // image rewrite between them, three barriers per step instead of four (round 5; same values in the same order)
  __bf16* Zhi = Xlo;
  unsigned* roww = reinterpret_cast<unsigned*>(Treg + tfloats);
  float* rlive = reinterpret_cast<float*>(roww + R2);
  for (int i = tid; i < img; i += ENC_NT) { Xhi[i] = (__bf16)0.0f; Xlo[i] = (__bf16)0.0f; }
  for (int i = tid; i < tfloats; i += ENC_NT) Treg[i] = 0.0f;   // (also the k padding of the second image pair)
  for (int i = tid; i < R2; i += ENC_NT) {
    roww[i] = (unsigned)min(wbase + i, a.F - 1) * (unsigned)(hid * 4);
    rlive[i] = wbase + i < a.F ? 1.0f : 0.0f;
  }
  const int rsub = lane >> 4, c4 = (lane & 15) * 4;
  const int j0 = cg * 64 + c4;
  const bool jok = j0 < hid;
  const unsigned h4 = (unsigned)hid * 4u;
  const enc_rsrc bdc = enc_buf(a.dcond, ((long)a.F * a.lddcond) * 4);
  f32x4 dhu[2][8];       // d h_s * z_s: the part of d h_{s-1} that does not go through W_hh (row layout)
  f32x4 bsum[4];         // column sums of d r, d z, d n, d n * r over this lane's rows and all steps
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int i = 0; i < 8; ++i) dhu[rt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) bsum[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x16 acc[2][2];      // [row tile][column tile]
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][t][r] = 0.0f;
  __syncthreads();
  // PIPE (two products + fp16 gate stash = the training default; round 5): the step's stash comes in four batches of 12 loads
  // (row tile x half, 4 rows each). Round 4 issued a batch and waited for it, four exposed HBM latencies per step; here batch b + 1 is
  // in flight while batch b is worked on. Same values, same order.
#ifdef LFI_ENC_BWD_NOPIPE   // (same-box A/B builds: tools/build_variant.sh; LFI_ENC_BWD_NOZ keeps round 4's two image phases)
  constexpr bool PIPE = false;
#else
  constexpr bool PIPE = A2 && S16;
#endif
#ifdef LFI_ENC_BWD_NOZ
  constexpr bool Z3 = false;
#else
  constexpr bool Z3 = A2;
#endif
  // Two buffers (batch b -> buffer b & 1). Batch 0 of the NEXT step is issued right after this step's last product has issued its
  // last weight load: it travels under the closing barrier, the transposes and B0. Measured (p2_face / p2_speech, ms per launch, same
  // box): round 4's form 0.517 / 0.353; this 0.487 / 0.331. Issued EARLIER - during this step's last batch, in front of the products -
  // it sits in the same in-order queue in front of their weight fragments and gives most of that back (0.516 / 0.358); with a third
  // buffer, one batch earlier still: 20 spilled VGPRs. Neither kept.
  enc_u32x4 rp0[2][4], rp1[2][4];   // [buffer][row of the batch]: the two 16-byte halves of a lane's four units' gates
  f32x4 rhp[2][4];                  // h_{s-1}
  unsigned rwo[2][4];
  constexpr int BUF[4] = {0, 1, 0, 1};
  auto issue = [&](int bi, int sq) {   // batch bi = 2 rt + ih of step sq -> buffer BUF[bi]
    int rsv = rsub, jv = j0;
    asm volatile("" : "+v"(rsv), "+v"(jv));
    const unsigned j4 = (unsigned)jv * 4u, oob = jv < hid ? 0u : 0x80000000u;
    const enc_rsrc gs = enc_buf(reinterpret_cast<const _Float16*>(a.gates) + (long)sq * a.F * 4 * hid, (long)a.F * hid * 8);
    const enc_rsrc hs = enc_buf(a.hseq + (long)(sq > 0 ? sq - 1 : 0) * a.F * hid, (long)a.F * hid * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rl = rg * 64 + (bi >> 1) * 32 + 4 * (4 * (bi & 1) + u) + rsv;
      const unsigned w = roww[rl];
      const unsigned go = 2u * (w + j4) + oob;
      rwo[BUF[bi]][u] = w;
      rp0[BUF[bi]][u] = __builtin_amdgcn_raw_buffer_load_b128(gs, go, 0, 2);
      rp1[BUF[bi]][u] = __builtin_amdgcn_raw_buffer_load_b128(gs, go, 16, 2);
      rhp[BUF[bi]][u] = enc_ld4s(hs, w + j4 + oob, 0);
    }
  };
  if (PIPE) issue(0, a.hist - 1);

  for (int s = a.hist - 1; s >= 0; --s) {
    // ---- d h_s in the row layout
    f32x4 dh[2][8];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int rsv = rsub, cv = c4, jv = j0;
      asm volatile("" : "+v"(rsv), "+v"(cv), "+v"(jv));
      const unsigned j4 = (unsigned)jv * 4u, oob = jv < hid ? 0u : 0x80000000u;
      float* T = Tw + rt * (32 * ENC_TP);
      float* Trow = T + rsv * ENC_TP + cv;
      float* Tacc = T + (4 * half) * ENC_TP + l31;
      if (s == a.hist - 1) {
        const unsigned cb = (unsigned)a.col * 4u + j4 + oob;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const unsigned wrow = (roww[rg * 64 + rt * 32 + 4 * i + rsv] / h4) * (unsigned)(a.lddcond * 4);
          dh[rt][i] = enc_ld4(bdc, wrow + cb, 0);
          if (a.dup) dh[rt][i] += enc_ld4(bdc, wrow + cb, h4);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) Tacc[((r & 3) + 8 * (r >> 2)) * ENC_TP + 32 * t] = acc[rt][t][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 8; ++i) dh[rt][i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP) + dhu[rt][i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();   // B0: every wave is done with its transpose tiles (the second image pair overlays those) and with the
                       // previous step's n-gate product (which read the first image pair)
    if (q.Kp > hid) {   // the transposes left accumulator bits in the second pair's k padding: NaN patterns x 0 would poison the product
      const int pad = q.Kp - hid;
      for (int i = tid; i < R2 * pad; i += ENC_NT) {
        const int rl = i / pad, c = hid + (i - rl * pad);
        Yhi[rl * ldx + c] = (__bf16)0.0f; Ylo[rl * ldx + c] = (__bf16)0.0f;
      }
    }
    const int sp = s > 0 ? s - 1 : 0;
    const float hp_on = s > 0 ? 1.0f : 0.0f;
    const enc_rsrc bgs = S16 ? enc_buf(reinterpret_cast<const _Float16*>(a.gates) + (long)s * a.F * 4 * hid, (long)a.F * hid * 8)
                             : enc_buf(a.gates + (long)s * a.F * 4 * hid, (long)a.F * hid * 16);
    const enc_rsrc bhp = enc_buf(a.hseq + (long)sp * a.F * hid, (long)a.F * hid * 4);
    const enc_rsrc bgi = A2 ? enc_buf(reinterpret_cast<const __bf16*>(a.dgi) + (long)s * a.F * hid, (long)a.F * hid * 2)
                            : enc_buf(a.dgi + (long)s * a.F * hid, (long)a.F * hid * 4);
    const enc_rsrc bgh = A2 ? enc_buf(reinterpret_cast<const __bf16*>(a.dgh) + (long)s * a.F * G3, (long)a.F * G3 * 2)
                            : enc_buf(a.dgh + (long)s * a.F * G3, (long)a.F * G3 * 4);
    f32x4 danr[2][8];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int rsv = rsub, jv = j0;
      asm volatile("" : "+v"(rsv), "+v"(jv));
      const unsigned j4 = (unsigned)jv * 4u, oob = jv < hid ? 0u : 0x80000000u;
#pragma unroll
      for (int ih = 0; ih < 2; ++ih) {
        f32x4 gr[4], gu[4], gn[4], gg[4], hp[4];
        unsigned wo[4];
        if (PIPE) {
          const int bi = 2 * rt + ih;
          if (bi < 3) issue(bi + 1, s);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const enc_u32x4 p0 = rp0[BUF[bi]][u], p1 = rp1[BUF[bi]][u];
            const f32x4 u0 = enc_unpack_gates(p0[0], p0[1]), u1 = enc_unpack_gates(p0[2], p0[3]);
            const f32x4 u2 = enc_unpack_gates(p1[0], p1[1]), u3 = enc_unpack_gates(p1[2], p1[3]);
            gr[u] = f32x4{u0[0], u1[0], u2[0], u3[0]}; gu[u] = f32x4{u0[1], u1[1], u2[1], u3[1]};
            gn[u] = f32x4{u0[2], u1[2], u2[2], u3[2]}; gg[u] = f32x4{u0[3], u1[3], u2[3], u3[3]};
            hp[u] = rhp[BUF[bi]][u];
            wo[u] = rwo[BUF[bi]][u];
          }
        }
#pragma unroll
        for (int u = 0; u < 4 && !PIPE; ++u) {
          const int rl = rg * 64 + rt * 32 + 4 * (4 * ih + u) + rsv;
          wo[u] = roww[rl];
          if (S16) {   // fp16 stash, [window][unit][r, z, n, W_hn h]: two 16-byte loads hold this lane's four units
            const unsigned go = 2u * (wo[u] + j4) + oob;
            const enc_u32x4 p0 = __builtin_amdgcn_raw_buffer_load_b128(bgs, go, 0, 2), p1 = __builtin_amdgcn_raw_buffer_load_b128(bgs, go, 16, 2);
            const f32x4 u0 = enc_unpack_gates(p0[0], p0[1]), u1 = enc_unpack_gates(p0[2], p0[3]);
            const f32x4 u2 = enc_unpack_gates(p1[0], p1[1]), u3 = enc_unpack_gates(p1[2], p1[3]);
            gr[u] = f32x4{u0[0], u1[0], u2[0], u3[0]}; gu[u] = f32x4{u0[1], u1[1], u2[1], u3[1]};
            gn[u] = f32x4{u0[2], u1[2], u2[2], u3[2]}; gg[u] = f32x4{u0[3], u1[3], u2[3], u3[3]};
          } else {
            const unsigned go = 4u * wo[u] + j4 + oob;
            gr[u] = enc_ld4s(bgs, go, 0); gu[u] = enc_ld4s(bgs, go, h4); gn[u] = enc_ld4s(bgs, go, 2 * h4); gg[u] = enc_ld4s(bgs, go, 3 * h4);
          }
          hp[u] = enc_ld4s(bhp, wo[u] + j4 + oob, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 4 * ih + u;
          const int rl = rg * 64 + rt * 32 + 4 * i + rsv;
          const float live = rlive[rl];
          f32x4 dan, dau, dar, dnr;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float rr = gr[u][e], uu = gu[u][e], nn = gn[u][e], ghn = gg[u][e];
            const float dhn = dh[rt][i][e];
            const float du = dhn * (hp[u][e] * hp_on - nn);
            const float dn = dhn * (1.0f - uu);
            dan[e] = dn * (1.0f - nn * nn);
            dau[e] = du * uu * (1.0f - uu);
            dar[e] = dan[e] * ghn * rr * (1.0f - rr);
            dnr[e] = dan[e] * rr;
            dhu[rt][i][e] = dhn * uu;
          }
          if (A2) {
            const unsigned j2 = j4 >> 1, h2 = h4 >> 1;
            enc_st2h(dan, bgi, (wo[u] >> 1) + j2 + oob, 0);
            const unsigned o = 3u * (wo[u] >> 1) + j2 + oob;
            enc_st2h(dar, bgh, o, 0); enc_st2h(dau, bgh, o, h2); enc_st2h(dnr, bgh, o, 2 * h2);
          } else {
            enc_st4(dan, bgi, wo[u] + j4 + oob, 0);
            const unsigned o = 3u * wo[u] + j4 + oob;
            enc_st4(dar, bgh, o, 0); enc_st4(dau, bgh, o, h4); enc_st4(dnr, bgh, o, 2 * h4);
          }
          bsum[0] += live * dar; bsum[1] += live * dau; bsum[2] += live * dan; bsum[3] += live * dnr;
          if (!Z3) danr[rt][i] = dnr;
          if (s > 0 && jok) {   // gate images for the products: d r -> first pair, d z -> second pair (A2: d n * r -> the third image)
            uint2 h, l;
            split2(dar[0], dar[1], &h.x, &l.x); split2(dar[2], dar[3], &h.y, &l.y);
            *reinterpret_cast<uint2*>(Xhi + rl * ldx + jv) = h;
            if (!A2) *reinterpret_cast<uint2*>(Xlo + rl * ldx + jv) = l;
            split2(dau[0], dau[1], &h.x, &l.x); split2(dau[2], dau[3], &h.y, &l.y);
            *reinterpret_cast<uint2*>(Yhi + rl * ldx + jv) = h;
            if (!A2) *reinterpret_cast<uint2*>(Ylo + rl * ldx + jv) = l;
            if (Z3) {
              split2(dnr[0], dnr[1], &h.x, &l.x); split2(dnr[2], dnr[3], &h.y, &l.y);
              *reinterpret_cast<uint2*>(Zhi + rl * ldx + jv) = h;
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (s == 0) break;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][t][r] = 0.0f;
    auto product = [&](int g, const __bf16* Ih, const __bf16* Il) {   // acc += image_g (64 rows x hid) W_hh[g] (hid x hid)
      const int nkt = q.Kp >> 4, nct = Jp >> 5;
      const __bf16* xh = Ih + (rg * 64 + l31) * ldx + 8 * half;
      const __bf16* xl = Il + (rg * 64 + l31) * ldx + 8 * half;
      ebf16x8 ah0[2], al0[2], ah1[2], al1[2];
      EncFrag f0[2][2], f1[2][2];  // [t][plane]
      auto load = [&](int kt, ebf16x8 (&ah)[2], ebf16x8 (&al)[2], EncFrag (&f)[2][2]) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          ah[rt] = *reinterpret_cast<const ebf16x8*>(xh + rt * 32 * ldx + kt * 16);
          if (!A2) al[rt] = *reinterpret_cast<const ebf16x8*>(xl + rt * 32 * ldx + kt * 16);
          else al[rt] = ah[rt];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const uint4* __restrict__ wf = q.wfrag + ((long)((g * nkt + ENC_WKT(kt)) * nct + cg * 2 + t) * 2) * 64;  // uniform
          f[t][0].u = wf[(unsigned)lane];
          f[t][1].u = (wf + 64)[(unsigned)lane];
        }
      };
      auto mma = [&](const ebf16x8 (&ah)[2], const ebf16x8 (&al)[2], const EncFrag (&f)[2][2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            if (!A2) acc[rt][t] = ENC_MFMA(al[rt], f[t][0].v, acc[rt][t], 0, 0, 0);
            acc[rt][t] = ENC_MFMA(ah[rt], f[t][1].v, acc[rt][t], 0, 0, 0);
            acc[rt][t] = ENC_MFMA(ah[rt], f[t][0].v, acc[rt][t], 0, 0, 0);
          }
      };
      load(0, ah0, al0, f0);
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {   // unconditional loads (see the forward kernel)
        load(kt + 1, ah1, al1, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah0, al0, f0);
        load(kt + 2, ah0, al0, f0);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah1, al1, f1);
      }
      if (kt + 1 < nkt) {
        load(kt + 1, ah1, al1, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(ah0, al0, f0);
        mma(ah1, al1, f1);
      } else {
        mma(ah0, al0, f0);
      }
    };
    __syncthreads();   // B1: both image pairs complete
    product(0, Xhi, Xlo);
    product(1, Yhi, Ylo);
    if (Z3) {
      product(2, Zhi, Zhi);
      if (PIPE) issue(0, s - 1);   // (s >= 1 here: the step loop left at s == 0 above)
      __syncthreads();   // B2: every wave has read the second image (the next step's transpose tiles overlay it)
      continue;
    }
    __syncthreads();   // B2: every wave has read the first pair
    if (jok) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rl = rg * 64 + rt * 32 + 4 * i + rsub;
          uint2 h, l;
          split2(danr[rt][i][0], danr[rt][i][1], &h.x, &l.x); split2(danr[rt][i][2], danr[rt][i][3], &h.y, &l.y);
          *reinterpret_cast<uint2*>(Xhi + rl * ldx + j0) = h;
          if (!A2) *reinterpret_cast<uint2*>(Xlo + rl * ldx + j0) = l;
        }
    }
    __syncthreads();   // B3
    product(2, Xhi, Xlo);
    if (PIPE) issue(0, s - 1);
  }
  if (a.bias_part && jok) {
    float* bp = a.bias_part + ((long)blockIdx.x * (ENC_NW / q.ncg) + rg) * 4 * hid;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      f32x4 v = bsum[qq];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] += __shfl_xor(v[e], 16, 64);
        v[e] += __shfl_xor(v[e], 32, 64);
      }
      if (rsub == 0) *reinterpret_cast<f32x4*>(bp + qq * hid + j0) = v;
    }
  }
}

// part [rows][4 * hid] -> column sums; 32 columns per workgroup, 32 row groups (each a strided run of rows, added in order),
// then the 32 partial sums in a fixed order: bit-reproducible. (8 row groups of one 256-thread workgroup took 20 - 28 us per
// modality on 448 rows: a chain of 56 dependent loads per thread.)
// Blocks 0, 1 (d r, d z) go to both bias gradients, block 2 (d n) to db_ih, block 3 (d n * r) to db_hh's n block.
__global__ __launch_bounds__(1024) void enc_bias_fold_kernel(const float* __restrict__ part, long rows, int hid,
                                                            float* __restrict__ db_ih, float* __restrict__ db_hh) {
  __shared__ float red[32][33];
  const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + c, W = 4 * hid;
  float acc = 0.0f;
  if (col < W)
    for (long r = rg; r < rows; r += 32) acc += part[r * W + col];
  red[rg][c] = acc;
  __syncthreads();
  if (rg == 0 && col < W) {
    float v = red[0][c];
#pragma unroll
    for (int i = 1; i < 32; ++i) v += red[i][c];
    const int blk = col / hid, j = col - blk * hid;
    if (blk < 2) { db_ih[col] = v; db_hh[col] = v; }
    else if (blk == 2) db_ih[col] = v;
    else db_hh[2 * hid + j] = v;
  }
}

}  // namespace

// ---- which instantiation: of the variant a finished plan names
template <bool A2, bool H>
static EncKernel enc_bwd_row_kernel_of(bool r64) { return r64 ? enc_gru_bwd_r64_kernel<A2, H> : enc_gru_bwd_wide_kernel<A2, H>; }
static EncKernel enc_bwd_row_pick(bool r64, bool a2, bool f16) {
  if (a2) return f16 ? enc_bwd_row_kernel_of<true, true>(r64) : enc_bwd_row_kernel_of<true, false>(r64);
  return f16 ? enc_bwd_row_kernel_of<false, true>(r64) : enc_bwd_row_kernel_of<false, false>(r64);
}
static EncKernel enc_bwd_pick(const EncBwdPlan& p, const lfi_enc_desc* d) {
  return p.variant >= 2 ? enc_bwd_row_pick(p.variant == 3, p.grads_bf16, d->stash_f16 != 0) : enc_gru_bwd_fused_kernel;
}

// rows of the bias_part buffer lfi_encode_windows_bwd fills (0: the unfused paths leave none)
extern "C" long lfi_encode_windows_bias_rows(const lfi_enc_desc* d) {
  if (!d) return 0;
  const EncBwdPlan p = enc_plan_bwd(d, d->ldcond, true);
  return p.variant ? (long)p.grid * (ENC_NW / p.q.ncg) : 0;
}
// Does lfi_encode_windows_bwd leave dgi / dgh as bf16 arrays? (lfi_gemm_desc.a_bf16; lfi_encode_windows_scatter looks the same answer up itself)
extern "C" int lfi_encode_windows_grad_stash_bf16(const lfi_enc_desc* d) { return (d && enc_plan_bwd(d, d->ldcond, true).grads_bf16) ? 1 : 0; }
// Is dgi left compact ([hist][F][3 hid], with dgh beside it) for lfi_encode_windows_scatter? The fused backward kernels all do.
extern "C" int lfi_encode_windows_compact_dgi(const lfi_enc_desc* d) { return (d && enc_plan_bwd(d, d->ldcond, true).variant != 0) ? 1 : 0; }

extern "C" int lfi_encode_windows_bias_grads(const float* bias_part, long rows, int hid, float* db_ih, float* db_hh,
                                             void* stream) {
  LFI_REQUIRE(bias_part && db_ih && db_hh && rows > 0 && hid > 0, "lfi_encode_windows_bias_grads: bad arguments");
  hipLaunchKernelGGL(enc_bias_fold_kernel, dim3(lfi_cdiv(4 * hid, 32)), dim3(1024), 0, (hipStream_t)stream, bias_part, rows, hid,
                     db_ih, db_hh);
  LFI_LAUNCH_CHECK("lfi_encode_windows_bias_grads");
  return LFI_OK;
}

extern "C" int lfi_encode_windows_bwd(const lfi_enc_desc* d, const float* dcond, int lddcond, const float* whh,
                                      const float* gates, const float* hseq, float* dgi, float* dgh, float* bias_part,
                                      float* work, void* stream) {
  EncArgs a = {};
  int rc = fill_args(d, &a, "lfi_encode_windows_bwd");
  if (rc) return rc;
  LFI_REQUIRE(dcond && whh && gates && hseq && dgi && dgh && work, "lfi_encode_windows_bwd: null pointer");
  a.dcond = dcond; a.lddcond = lddcond; a.gates = (float*)gates; a.hseq = (float*)hseq; a.dgi = dgi; a.dgh = dgh;
  a.bias_part = bias_part;
  hipStream_t st = (hipStream_t)stream;
  const int hid = d->hid, F = a.F;
  LFI_REQUIRE(!d->stash_f16 || lfi_encode_windows_stash_f16_ok(d), "lfi_encode_windows_bwd: lfi_enc_desc.stash_f16 is set for a shape "
              "whose gate stash is fp32 (ask lfi_encode_windows_stash_f16_ok)");
  if (d->lstm) {
    const int blocks = ew_blocks((long)F * hid);
    float* dhb[2] = {work, work + (long)F * hid};
    float* dcb[2] = {work + 2L * F * hid, work + 3L * F * hid};
    const float *dh_in = nullptr, *dc_in = nullptr;
    for (int s = d->hist - 1; s >= 0; --s) {
      float* dh_out = s > 0 ? dhb[s & 1] : nullptr;
      float* dc_out = s > 0 ? dcb[s & 1] : nullptr;
      hipLaunchKernelGGL(enc_lstm_gate_bwd_kernel, dim3(blocks), dim3(256), 0, st, a, s, dh_in, dc_in, dh_out, dc_out);
      if (s > 0) {
        lfi_gemm_desc g = {};
        g.M = F; g.N = hid; g.K = 4 * hid; g.batch = 1;
        g.A = dgh + (long)s * F * 4 * hid; g.lda = 4 * hid; g.a_kcontig = 1;
        g.B = whh; g.ldb = hid; g.b_kcontig = 0;
        g.C = dh_out; g.ldc = hid; g.accumulate = 1; g.precision = d->precision;
        if ((rc = lfi_gemm_f32(&g, stream))) return rc;
      }
      dh_in = dh_out; dc_in = dc_out;
    }
    LFI_LAUNCH_CHECK("lfi_encode_windows_bwd (lstm)");
    return LFI_OK;
  }
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  EncBwdPlan p = enc_plan_bwd(d, lddcond, al16(dcond) && al16(gates) && al16(hseq) && al16(dgi) && al16(dgh) && (!bias_part || al16(bias_part)));
  if (p.variant) {
    LFI_REQUIRE(!p.grads_bf16 || p.variant >= 2, "lfi_encode_windows_bwd: lfi_encode_windows_grad_stash_bf16 promised a bf16 gradient stash but the "
                "buffers are not 16-byte aligned");
    LFI_REQUIRE(!d->stash_f16 || p.variant >= 2, "lfi_encode_windows_bwd: an fp16 gate stash (lfi_enc_desc.stash_f16) needs the row-layout "
                "kernel (lfi_encode_windows_stash_f16_ok) and 16-byte aligned buffers");
    const EncKernel kernel = enc_bwd_pick(p, d);
    enc_build_weights(p.weights, &p.q, whh, hid, 0, work, st);
    if ((rc = enc_set_lds(kernel, p.lds))) return rc;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(ENC_NT), p.lds, st, a, p.q);
    LFI_LAUNCH_CHECK("lfi_encode_windows_bwd (fused)");
    return LFI_OK;
  }
  const int blocks = ew_blocks((long)F * hid);
  float* buf[2] = {work, work + (long)F * hid};
  const float* dh_in = nullptr;
  for (int s = d->hist - 1; s >= 0; --s) {
    float* dh_out = s > 0 ? buf[s & 1] : nullptr;
    hipLaunchKernelGGL(enc_gate_bwd_kernel, dim3(blocks), dim3(256), 0, st, a, s, dh_in, dh_out);
    if (s > 0) {
      lfi_gemm_desc g = {};
      g.M = F; g.N = hid; g.K = 3 * hid; g.batch = 1;
      g.A = dgh + (long)s * F * 3 * hid; g.lda = 3 * hid; g.a_kcontig = 1;
      g.B = whh; g.ldb = hid; g.b_kcontig = 0;  // (dgh W_hh)[w][j] = sum_k dgh[w][k] W_hh[k][j]
      g.C = dh_out; g.ldc = hid; g.accumulate = 1; g.precision = d->precision;
      if ((rc = lfi_gemm_f32(&g, stream))) return rc;
    }
    dh_in = dh_out;
  }
  LFI_LAUNCH_CHECK("lfi_encode_windows_bwd");
  return LFI_OK;
}

extern "C" int lfi_encode_windows_scatter(const lfi_enc_desc* d, const float* dgi, const float* dgh, const float* mask, float* dXp,
                                          void* stream) {
  EncArgs a = {};
  int rc = fill_args(d, &a, "lfi_encode_windows_scatter");
  if (rc) return rc;
  LFI_REQUIRE(dgi && dXp, "lfi_encode_windows_scatter: null pointer");
  a.compact = lfi_encode_windows_compact_dgi(d);
  LFI_REQUIRE(!a.compact || dgh, "lfi_encode_windows_scatter: the compact dgi of the fused backward needs dgh too");
  a.dgi = (float*)dgi; a.dgh = (float*)dgh; a.mask = mask;
  a.g16 = lfi_encode_windows_grad_stash_bf16(d);
  // bf16 compact stash (the training step's): 16-byte loads, several frame rows per workgroup (LFI_ENC_SCATTER16=0: the kernel above)
  const int cpr = 3 * d->hid / 8;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (lfi_env_on("LFI_ENC_SCATTER16") && a.g16 && a.compact && d->hid % 8 == 0 && cpr <= 256 && al16(dgi) && al16(dgh) && al16(dXp)) {
    const int rows = d->B * d->T, rpw = 256 / cpr;
    hipLaunchKernelGGL(enc_scatter16_kernel, dim3(lfi_cdiv(rows, rpw)), dim3(256), 0, (hipStream_t)stream, a, dXp, rows, cpr, rpw);
  } else
    hipLaunchKernelGGL(enc_scatter_kernel, dim3(d->B * d->T), dim3(256), 0, (hipStream_t)stream, a, dXp);
  LFI_LAUNCH_CHECK("lfi_encode_windows_scatter");
  return LFI_OK;
}
