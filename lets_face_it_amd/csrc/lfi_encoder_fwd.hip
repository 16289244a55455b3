// Window encoders, forward: the per-step gate kernels of the unfused GRU / LSTM loops, the four fused forward GRU kernels and
// lfi_encode_windows_fwd (see lfi_encoder.hip for the scheme; BPTT is lfi_encoder_bwd.hip).
#include "lfi_encoder_common.h"

namespace {

// One GRU step for every window. gh: F x 3hid = h_{s-1} W_hh^T (no bias), or null at s = 0 (h = 0).
__global__ __launch_bounds__(256) void enc_gate_fwd_kernel(EncArgs a, int s, const float* __restrict__ gh) {
  const int hid = a.hid, G3 = 3 * hid;
  const long total = (long)a.F * hid;
  const int pos0 = a.start - a.hist + 1;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int w = (int)(idx / hid), j = (int)(idx - (long)w * hid);
    const int n = w / a.B, b = w - n * a.B;
    const float* xp = a.Xp + ((long)b * a.T + (pos0 + n + s)) * G3;
    const float mk = a.mask ? a.mask[(long)w * a.hist + s] : 1.0f;
    float ghr = a.b_hh[j], ghu = a.b_hh[hid + j], ghn = a.b_hh[2 * hid + j];
    float hp = 0.0f;
    if (gh) {
      const float* g = gh + (long)w * G3;
      ghr += g[j]; ghu += g[hid + j]; ghn += g[2 * hid + j];
      hp = a.hseq[((long)(s - 1) * a.F + w) * hid + j];
    }
    const float rr = sigmoidf_(mk * xp[j] + a.b_ih[j] + ghr);
    const float uu = sigmoidf_(mk * xp[hid + j] + a.b_ih[hid + j] + ghu);
    const float nn = tanhf_(mk * xp[2 * hid + j] + a.b_ih[2 * hid + j] + rr * ghn);
    const float hnew = (1.0f - uu) * nn + uu * hp;
    const long sw = (long)s * a.F + w;
    a.hseq[sw * hid + j] = hnew;
    if (a.gates) {
      float* gs = a.gates + sw * 4 * hid;
      gs[j] = rr; gs[hid + j] = uu; gs[2 * hid + j] = nn; gs[3 * hid + j] = ghn;
    }
    if (s == a.hist - 1) {  // cat(seq[:, -1], h_n[0]): the same vector twice (glow/models.py:63-64)
      float* c = a.cond + (long)w * a.ldcond + a.col;
      c[j] = hnew;
      if (a.dup) c[hid + j] = hnew;
    }
  }
}

// ---- "enc: lstm" modality (glow/models.py:27-33,65-69): nn.LSTM from zero (h, c) over the window, gate blocks i, f, g, o
// (torch.nn.LSTM weight layout). Per step one GEMM gh = h_{s-1} W_hh^T (F x 4hid) + this kernel. The stash row of a
// (step, window) is 5 * hid floats: i, f, g, o, c_s.
__global__ __launch_bounds__(256) void enc_lstm_gate_fwd_kernel(EncArgs a, int s, const float* __restrict__ gh) {
  const int hid = a.hid, G = 4 * hid;
  const long total = (long)a.F * hid;
  const int pos0 = a.start - a.hist + 1;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int w = (int)(idx / hid), j = (int)(idx - (long)w * hid);
    const int n = w / a.B, b = w - n * a.B;
    const float* xp = a.Xp + ((long)b * a.T + (pos0 + n + s)) * G;
    const float mk = a.mask ? a.mask[(long)w * a.hist + s] : 1.0f;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pre[q] = mk * xp[q * hid + j] + a.b_ih[q * hid + j] + a.b_hh[q * hid + j];
    float cp = 0.0f;
    if (gh) {
      const float* g = gh + (long)w * G;
#pragma unroll
      for (int q = 0; q < 4; ++q) pre[q] += g[q * hid + j];
      cp = a.gates[(((long)(s - 1) * a.F + w) * 5 + 4) * hid + j];
    }
    const float ii = sigmoidf_(pre[0]), ff = sigmoidf_(pre[1]), gg = tanhf_(pre[2]), oo = sigmoidf_(pre[3]);
    const float c = ff * cp + ii * gg;
    const float hnew = oo * tanhf_(c);
    const long sw = (long)s * a.F + w;
    a.hseq[sw * hid + j] = hnew;
    float* gs = a.gates + sw * 5 * hid;
    gs[j] = ii; gs[hid + j] = ff; gs[2 * hid + j] = gg; gs[3 * hid + j] = oo; gs[4 * hid + j] = c;
    if (s == a.hist - 1) {  // cat(seq[:, -1], h_n[0]): the same vector twice (glow/models.py:68-69)
      float* cc = a.cond + (long)w * a.ldcond + a.col;
      cc[j] = hnew;
      if (a.dup) cc[hid + j] = hnew;
    }
  }
}

template <bool STASH, bool MASK, bool X3>
__global__ __launch_bounds__(ENC_NT, 2) void enc_gru_fwd_fused_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, ldk = q.R + 1, Jp = q.Jp;
  const int jb = cg * 64 + l31;               // hidden index of sub-tile 0; sub-tile 1 is jb + 32
  const int wbase = blockIdx.x * q.R;
  const int pos0 = a.start - a.hist + 1;
  float* Als = enc_smem;  // h_{s-1}: element (row, k) at Als[k * ldk + row], rows k >= hid stay zero
  for (int i = tid; i < q.Kp * ldk; i += ENC_NT) Als[i] = 0.0f;
  // X3: bf16 hi / lo images of the same state, row-major, columns k >= hid stay zero
  const int ldx = q.Kp + 8;
  __bf16* Xhi = reinterpret_cast<__bf16*>(enc_smem + q.Kp * ldk);
  __bf16* Xlo = Xhi + q.R * ldx;
  if (X3)
    for (int i = tid; i < q.R * ldx; i += ENC_NT) { Xhi[i] = (__bf16)0.0f; Xlo[i] = (__bf16)0.0f; }
  // per-row byte offsets (rows past F are clamped to the last window: they recompute and re-store its values):
  // rowx = start of the window's step-0 input projection row in Xp, roww = w * hid * 4
  unsigned* rowx = reinterpret_cast<unsigned*>(X3 ? reinterpret_cast<float*>(Xlo + q.R * ldx) : enc_smem + q.Kp * ldk);
  unsigned* roww = rowx + q.R;
  unsigned* rowm = roww + q.R;   // w * hist * 4 (dropout mask row)
  for (int i = tid; i < q.R; i += ENC_NT) {
    const int w = min(wbase + i, a.F - 1);
    const int n = w / a.B, b = w - n * a.B;
    rowx[i] = (unsigned)(b * a.T + pos0 + n) * (unsigned)(G3 * 4);
    roww[i] = (unsigned)w * (unsigned)(hid * 4);
    rowm[i] = (unsigned)w * (unsigned)(a.hist * 4);
  }

  float bi[2][3], bh[2][3];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int j = jb + 32 * t;
      const bool ok = j < hid;
      bi[t][g] = ok ? a.b_ih[g * hid + j] : 0.0f;
      bh[t][g] = ok ? a.b_hh[g * hid + j] : 0.0f;
    }
  const int boff = half * 3 * Jp + jb;         // per-lane offset into the padded weights (k = 2 kp + half)
  const int aoff = half * ldk + rg * 32 + l31;  // per-lane offset into Als
  const int nkp = q.Kp >> 1;                    // multiple of 2 * ENC_KC
  __syncthreads();

  for (int s = 0; s < a.hist; ++s) {
    ENC_STAMP(0);
    f32x16 acc[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][g][r] = 0.0f;
    if (X3 && s > 0) {
      // per 16-deep k-tile: A hi/lo fragments of this wave's 32 rows, B hi/lo fragments of its 2 x 3 column tiles
      const int nkt = q.Kp >> 4, nct = Jp >> 5;
      const __bf16* xh = Xhi + (rg * 32 + l31) * ldx + 8 * half;
      const __bf16* xl = Xlo + (rg * 32 + l31) * ldx + 8 * half;
      ebf16x8 ah0, al0, ah1, al1;
      EncFrag f0[2][3][2], f1[2][3][2];  // [t][g][plane]
      auto load = [&](int kt, ebf16x8& ah, ebf16x8& al, EncFrag (&f)[2][3][2]) {
        ah = *reinterpret_cast<const ebf16x8*>(xh + kt * 16);
        al = *reinterpret_cast<const ebf16x8*>(xl + kt * 16);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const uint4* __restrict__ wf = q.wfrag + ((long)((kt * 3 + g) * nct + cg * 2 + t) * 2) * 64;  // uniform
            f[t][g][0].u = wf[(unsigned)lane];
            f[t][g][1].u = (wf + 64)[(unsigned)lane];
          }
      };
      auto mma = [&](const ebf16x8& ah, const ebf16x8& al, const EncFrag (&f)[2][3][2]) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            acc[t][g] = ENC_MFMA(al, f[t][g][0].v, acc[t][g], 0, 0, 0);
            acc[t][g] = ENC_MFMA(ah, f[t][g][1].v, acc[t][g], 0, 0, 0);
            acc[t][g] = ENC_MFMA(ah, f[t][g][0].v, acc[t][g], 0, 0, 0);
          }
      };
      // every load in the steady-state loop is unconditional: with a conditional load the compiler cannot count the loads
      // in flight and waits for ALL of them (vmcnt(0)) before the MFMAs, i.e. for the fragments it has just requested
      load(0, ah0, al0, f0);
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {
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
    }
    if (!X3 && s > 0) {
      float a0[ENC_KC], a1[ENC_KC], b0[ENC_KC][6], b1[ENC_KC][6];
      auto load = [&](int kp0, float (&av)[ENC_KC], float (&bv)[ENC_KC][6]) {
        const float* __restrict__ wk = q.wpad + (long)kp0 * 6 * Jp;  // uniform base, 32-bit per-lane offset: saddr loads
        const float* ak = Als + kp0 * 2 * ldk;
#pragma unroll
        for (int u = 0; u < ENC_KC; ++u) {
          av[u] = ak[u * 2 * ldk + aoff];
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            const float* __restrict__ wu = wk + (u * 6 + g) * Jp;  // uniform
            bv[u][g] = wu[(unsigned)boff];
            bv[u][3 + g] = (wu + 32)[(unsigned)boff];
          }
        }
      };
      auto mma = [&](const float (&av)[ENC_KC], const float (&bv)[ENC_KC][6]) {
#pragma unroll
        for (int u = 0; u < ENC_KC; ++u)
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            acc[0][g] = mfma32(av[u], bv[u][g], acc[0][g]);
            acc[1][g] = mfma32(av[u], bv[u][3 + g], acc[1][g]);
          }
      };
      load(0, a0, b0);
      int kp = 0;
      for (; kp + 2 * ENC_KC < nkp; kp += 2 * ENC_KC) {   // unconditional loads (see the bf16x3 loop)
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
    ENC_STAMP(1);
    __syncthreads();  // every wave has finished reading h_{s-1}
    ENC_STAMP(2);
    // gate math on the accumulators in four straight-line groups (one hidden sub-tile x 8 registers each: 40 loads in
    // flight per lane). The lane coordinates are laundered through an empty asm so that the per-register address arithmetic
    // stays inside the step loop instead of being hoisted into ~100 loop-invariant registers (which spilled).
    int halfv = half, jv = jb;
    asm volatile("" : "+v"(halfv), "+v"(jv));
    const enc_rsrc bx = enc_buf(a.Xp, (long)a.B * a.T * G3 * 4);
    const enc_rsrc bhs = enc_buf(STASH ? a.hseq + (long)s * a.F * hid : nullptr, STASH ? (long)a.F * hid * 4 : 0);
    const enc_rsrc bgs = enc_buf(STASH ? a.gates + (long)s * a.F * 4 * hid : nullptr, STASH ? (long)a.F * hid * 16 : 0);
    const enc_rsrc bms = enc_buf(MASK ? a.mask : nullptr, MASK ? (long)a.F * a.hist * 4 : 0);
    const unsigned sx = (unsigned)s * (unsigned)(G3 * 4), h4 = (unsigned)hid * 4u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = jv + 32 * t;
      if (j < hid) {
        const unsigned j4 = (unsigned)j * 4u;
#pragma unroll
        for (int rh = 0; rh < 2; ++rh) {
          float xr[8], xu[8], xn[8], mk[8], hp[8];
          unsigned wo[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int rl = enc_rowl(rg, rh * 8 + e, halfv);
            const unsigned xo = rowx[rl] + j4;
            wo[e] = roww[rl];
            xr[e] = enc_ld(bx, xo, sx); xu[e] = enc_ld(bx, xo, sx + h4); xn[e] = enc_ld(bx, xo, sx + 2 * h4);
            mk[e] = MASK ? enc_ld(bms, rowm[rl], (unsigned)s * 4u) : 1.0f;
            hp[e] = Als[j * ldk + rl];  // zero at s = 0
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int r = rh * 8 + e;
            const int rl = enc_rowl(rg, r, halfv);
            const float ghn = acc[t][2][r] + bh[t][2];
            const float rr = sigmoidf_(mk[e] * xr[e] + bi[t][0] + (acc[t][0][r] + bh[t][0]));
            const float uu = sigmoidf_(mk[e] * xu[e] + bi[t][1] + (acc[t][1][r] + bh[t][1]));
            const float nn = tanhf_(mk[e] * xn[e] + bi[t][2] + rr * ghn);
            const float hnew = (1.0f - uu) * nn + uu * hp[e];
            if (STASH) {
              enc_st(hnew, bhs, wo[e] + j4, 0);
              const unsigned go = 4u * wo[e] + j4;
              enc_st(rr, bgs, go, 0); enc_st(uu, bgs, go, h4); enc_st(nn, bgs, go, 2 * h4); enc_st(ghn, bgs, go, 3 * h4);
            }
            Als[j * ldk + rl] = hnew;
            if (X3) {
              const __bf16 hi = (__bf16)hnew;
              Xhi[rl * ldx + j] = hi;
              Xlo[rl * ldx + j] = (__bf16)(hnew - (float)hi);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          ENC_STAMP(3 + t * 2 + rh);
        }
      }
    }
    __syncthreads();
    ENC_STAMP(7);
  }
  // cat(seq[:, -1], h_n[0]): the final state, once or twice (glow/models.py:63-64), straight from LDS
  for (int idx = tid; idx < q.R * hid; idx += ENC_NT) {
    const int rl = idx / hid, j = idx - rl * hid;
    const int w = wbase + rl;
    if (w < a.F) {
      const float v = Als[j * ldk + rl];
      float* c = a.cond + (long)w * a.ldcond + a.col + j;
      c[0] = v;
      if (a.dup) c[hid] = v;
    }
  }
}

// ---- the same forward recurrence (bf16x3 products) with a ROW-LAYOUT gate epilogue.
// What paced enc_gru_fwd_fused_kernel<.., true> was not HBM, L2 or the matrix pipe but the number of vector-memory
// INSTRUCTIONS: in the accumulator layout a lane holds one column of 16 different rows, so every projected input, mask,
// stash value is its own 4-byte access - 9 wave instructions per (row, 32 columns) and step, 37 k cycles of address
// processing per CU and step next to 25 k for the weight fragments, against 18 k of MFMA issue (round-2 notes in DESIGN.md).
// Here each gate's accumulators go through a wave-private LDS tile (32 rows x 64 columns, written in accumulator order,
// read back row-wise) so that a lane owns 4 CONSECUTIVE columns of 8 rows: projected inputs come in and h, r, z, n, W_hn h
// leave as 16-byte accesses (4.5x fewer instructions), the state images are refreshed with 8-byte LDS stores, and h_{s-1}
// waits in that same tile during the MFMA phase (no k-major fp32 state image: 34 KB of LDS less, two workgroups per CU stay).
template <bool STASH, bool MASK, bool S16>
__global__ __launch_bounds__(ENC_NT, 2) void enc_gru_fwd_wide_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, Jp = q.Jp;
  const int wbase = blockIdx.x * q.R;
  const int pos0 = a.start - a.hist + 1;
  const int ldx = q.Kp + 8;
  // LDS: bf16 hi / lo images of h_{s-1} (row-major [R][Kp + 8]) | per-wave transpose tiles | biases [6][Jp] | per-row tables
  __bf16* Xhi = reinterpret_cast<__bf16*>(enc_smem);
  __bf16* Xlo = Xhi + q.R * ldx;
  float* T = reinterpret_cast<float*>(Xlo + q.R * ldx) + wave * (32 * ENC_TP);
  float* bias = reinterpret_cast<float*>(Xlo + q.R * ldx) + ENC_NW * (32 * ENC_TP);   // [0..2][Jp] = b_ih, [3..5][Jp] = b_hh
  unsigned* rowx = reinterpret_cast<unsigned*>(bias + 6 * Jp);
  unsigned* roww = rowx + q.R;
  float* mk_tab = reinterpret_cast<float*>(roww + q.R);                                 // [R][hist] (MASK only)
  for (int i = tid; i < q.R * ldx; i += ENC_NT) { Xhi[i] = (__bf16)0.0f; Xlo[i] = (__bf16)0.0f; }
  for (int i = tid; i < 6 * Jp; i += ENC_NT) {
    const int g = i / Jp, j = i - g * Jp;
    bias[i] = j < hid ? (g < 3 ? a.b_ih[g * hid + j] : a.b_hh[(g - 3) * hid + j]) : 0.0f;
  }
  for (int i = tid; i < q.R; i += ENC_NT) {
    const int w = min(wbase + i, a.F - 1);   // rows past F recompute and re-store the last window
    const int n = w / a.B, b = w - n * a.B;
    rowx[i] = (unsigned)(b * a.T + pos0 + n) * (unsigned)(G3 * 4);
    roww[i] = (unsigned)w * (unsigned)(hid * 4);
  }
  if (MASK)
    for (int i = tid; i < q.R * a.hist; i += ENC_NT) {
      const int rl = i / a.hist, s = i - rl * a.hist;
      mk_tab[i] = a.mask[(long)min(wbase + rl, a.F - 1) * a.hist + s];
    }
  // row layout of this wave's 32 x 64 tile: lane owns columns c4 .. c4 + 3 of rows 4 i + rsub, i = 0 .. 7
  const int rsub = lane >> 4, c4 = (lane & 15) * 4;
  const int j0 = cg * 64 + c4;            // first hidden index of the lane's four
  const bool jok = j0 < hid;              // hid % 4 == 0: the four are all inside or all outside
  {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(T + (4 * i + rsub) * ENC_TP + c4) = z;   // h_{-1} = 0
  }
  const enc_rsrc bx = enc_buf(a.Xp, (long)a.B * a.T * G3 * 4);
  const unsigned h4 = (unsigned)hid * 4u;
  __syncthreads();

  for (int s = 0; s < a.hist; ++s) {
    ENC_STAMP(0);
    f32x16 acc[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][g][r] = 0.0f;
#ifdef LFI_ENC_EXP_NO_KLOOP
    if (false) {
#else
    if (s > 0) {
#endif
      const int nkt = q.Kp >> 4, nct = Jp >> 5;
      const __bf16* xh = Xhi + (rg * 32 + l31) * ldx + 8 * half;
      const __bf16* xl = Xlo + (rg * 32 + l31) * ldx + 8 * half;
      ebf16x8 ah0, al0, ah1, al1;
      EncFrag f0[2][3][2], f1[2][3][2];  // [t][g][plane]
      auto load = [&](int kt, ebf16x8& ah, ebf16x8& al, EncFrag (&f)[2][3][2]) {
        ah = *reinterpret_cast<const ebf16x8*>(xh + kt * 16);
        al = *reinterpret_cast<const ebf16x8*>(xl + kt * 16);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const uint4* __restrict__ wf = q.wfrag + ((long)((ENC_WKT(kt) * 3 + g) * nct + cg * 2 + t) * 2) * 64;  // uniform
#ifdef LFI_ENC_EXP_NO_WLOADS
            if (kt > 1) continue;
#endif
            f[t][g][0].u = wf[(unsigned)lane];
            f[t][g][1].u = (wf + 64)[(unsigned)lane];
          }
      };
      auto mma = [&](const ebf16x8& ah, const ebf16x8& al, const EncFrag (&f)[2][3][2]) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            acc[t][g] = ENC_MFMA(al, f[t][g][0].v, acc[t][g], 0, 0, 0);
            acc[t][g] = ENC_MFMA(ah, f[t][g][1].v, acc[t][g], 0, 0, 0);
            acc[t][g] = ENC_MFMA(ah, f[t][g][0].v, acc[t][g], 0, 0, 0);
          }
      };
      load(0, ah0, al0, f0);   // every load in the steady-state loop is unconditional (see enc_gru_fwd_fused_kernel)
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {
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
    }
    ENC_STAMP(1);
    // ---- gate epilogue in the row layout
    int rsv = rsub, cv = c4, jv = j0;
    asm volatile("" : "+v"(rsv), "+v"(cv), "+v"(jv));   // keep the per-row address arithmetic inside the step loop (registers)
    const unsigned sx = (unsigned)s * (unsigned)(G3 * 4), j4 = (unsigned)jv * 4u;
    const unsigned oob = jv < hid ? 0u : 0x80000000u;
    const enc_rsrc bhs = enc_buf(STASH ? a.hseq + (long)s * a.F * hid : nullptr, STASH ? (long)a.F * hid * 4 : 0);
    const enc_rsrc bgs = S16 ? enc_buf(STASH ? reinterpret_cast<const _Float16*>(a.gates) + (long)s * a.F * 4 * hid : nullptr,
                                       STASH ? (long)a.F * hid * 8 : 0)
                             : enc_buf(STASH ? a.gates + (long)s * a.F * 4 * hid : nullptr, STASH ? (long)a.F * hid * 16 : 0);
    float* Trow = T + rsv * ENC_TP + cv;                 // + 4 i * ENC_TP per row
    float* Tacc = T + (4 * half) * ENC_TP + l31;         // accumulator (t, r) at + ((r & 3) + 8 (r >> 2)) * ENC_TP + 32 t
    f32x4 hp[8], xin[8];
    unsigned xo[8], wo[8];
    float mk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rl = rg * 32 + 4 * i + rsv;
      xo[i] = rowx[rl] + j4 + oob;   // columns past hid: an offset outside every buffer (loads return 0, stores are dropped)
      wo[i] = roww[rl];
      mk[i] = MASK ? mk_tab[rl * a.hist + s] : 1.0f;
      hp[i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP);   // h_{s-1}, parked here by the previous step
#ifdef LFI_ENC_EXP_NO_XP
      xin[i] = f32x4{0.1f, 0.2f, 0.3f, 0.4f};
#else
      xin[i] = enc_ld4(bx, xo[i], sx);
#endif
    }
    auto transpose = [&](int g, f32x4 (&out)[8]) {   // gate g of this wave's tile: accumulator layout -> row layout
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // earlier reads of the tile are done
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) Tacc[((r & 3) + 8 * (r >> 2)) * ENC_TP + 32 * t] = acc[t][g][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP);
    };
    const f32x4 bir = *reinterpret_cast<const f32x4*>(bias + 0 * Jp + jv), bhr = *reinterpret_cast<const f32x4*>(bias + 3 * Jp + jv);
    const f32x4 biu = *reinterpret_cast<const f32x4*>(bias + 1 * Jp + jv), bhu = *reinterpret_cast<const f32x4*>(bias + 4 * Jp + jv);
    const f32x4 bin = *reinterpret_cast<const f32x4*>(bias + 2 * Jp + jv), bhn = *reinterpret_cast<const f32x4*>(bias + 5 * Jp + jv);
    f32x4 rr[8], uu[8], gh[8];
    transpose(0, gh);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rr[i][e] = ENC_SIG(mk[i] * xin[i][e] + bir[e] + (gh[i][e] + bhr[e]));
      if (STASH && !S16) enc_st4(rr[i], bgs, 4u * wo[i] + j4 + oob, 0);
#ifndef LFI_ENC_EXP_NO_XP
      xin[i] = enc_ld4(bx, xo[i], sx + h4);
#endif
    }
    transpose(1, gh);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) uu[i][e] = ENC_SIG(mk[i] * xin[i][e] + biu[e] + (gh[i][e] + bhu[e]));
      if (STASH && !S16) enc_st4(uu[i], bgs, 4u * wo[i] + j4 + oob, h4);
#ifndef LFI_ENC_EXP_NO_XP
      xin[i] = enc_ld4(bx, xo[i], sx + 2 * h4);
#endif
    }
    transpose(2, gh);
    ENC_STAMP(2);
    __syncthreads();   // every wave has finished the MFMA phase: the state images may be overwritten
    ENC_STAMP(3);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rl = rg * 32 + 4 * i + rsv;
      f32x4 ghn, nn, hn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ghn[e] = gh[i][e] + bhn[e];
        nn[e] = ENC_TANH(mk[i] * xin[i][e] + bin[e] + rr[i][e] * ghn[e]);
        hn[e] = (1.0f - uu[i][e]) * nn[e] + uu[i][e] * hp[i][e];
      }
      if (STASH && S16) {   // [window][unit][r, z, n, W_hn h] fp16: this lane's four units = 32 contiguous bytes
        const uint2 g0 = enc_pack_gates(rr[i][0], uu[i][0], nn[0], ghn[0]), g1 = enc_pack_gates(rr[i][1], uu[i][1], nn[1], ghn[1]);
        const uint2 g2 = enc_pack_gates(rr[i][2], uu[i][2], nn[2], ghn[2]), g3 = enc_pack_gates(rr[i][3], uu[i][3], nn[3], ghn[3]);
        const unsigned go = 2u * (wo[i] + j4) + oob;
        __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g0.x, g0.y, g1.x, g1.y}, bgs, go, 0, LFI_ENC_ST_AUX);
        __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g2.x, g2.y, g3.x, g3.y}, bgs, go, 16, LFI_ENC_ST_AUX);
        enc_st4(hn, bhs, wo[i] + j4 + oob, 0);
        __builtin_amdgcn_sched_barrier(0);   // one row's packing temporaries at a time (register pressure)
      } else if (STASH) {
        enc_st4(nn, bgs, 4u * wo[i] + j4 + oob, 2 * h4);
        enc_st4(ghn, bgs, 4u * wo[i] + j4 + oob, 3 * h4);
        enc_st4(hn, bhs, wo[i] + j4 + oob, 0);
      }
      if (jok) {
        uint2 h, l;
        split2(hn[0], hn[1], &h.x, &l.x);
        split2(hn[2], hn[3], &h.y, &l.y);
        *reinterpret_cast<uint2*>(Xhi + rl * ldx + jv) = h;
        *reinterpret_cast<uint2*>(Xlo + rl * ldx + jv) = l;
      }
      hp[i] = hn;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile's last row-wise reads are done
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(Trow + 4 * i * ENC_TP) = hp[i];   // park h_s for the next step
    if (s == a.hist - 1 && jok) {   // cat(seq[:, -1], h_n[0]): the final state, once or twice (glow/models.py:63-64)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int w = wbase + rg * 32 + 4 * i + rsv;
        if (w < a.F) {
          float* c = a.cond + (long)w * a.ldcond + a.col + jv;
          *reinterpret_cast<f32x4*>(c) = hp[i];
          if (a.dup) *reinterpret_cast<f32x4*>(c + hid) = hp[i];
        }
      }
    }
    ENC_STAMP(4);
    __syncthreads();   // the new state images are complete
    ENC_STAMP(5);
  }
}

// ---- the forward recurrence with TWO 32-row tiles per wave (64 windows per row group) and one workgroup per CU.
// What paces enc_gru_fwd_wide_kernel, from ingredient-removal builds (tools/enc_probe.py + tools/build_variant.sh, p2_face shape, ms per
// launch): 0.66 as shipped; 0.62 without any stash; 0.65 with every k-tile reading the SAME weight fragments (L1 hits instead of the
// L2 stream); 0.64 with no weight loads in the k loop at all; 0.65 with sigmoid / tanh replaced by a multiply; 0.17 without the
// h W_hh^T loop. The k loop costs ~0.46 ms wherever its operands come from: 389 G MFMA-pass-FLOP at ~0.9 PFLOP/s, the rate every
// three-product bf16 stream of this code base settles at on this chip (the planes GEMM: 1.0), and two workgroups per CU meet in the
// matrix phase and in the gate epilogue alike (staggering the second one by 6 k .. 30 k cycles, by any pairing rule, changed nothing).
// This tiling keeps the MFMA work and halves everything around it in the k loop: a wave holds the accumulators of 64 windows (2 row
// tiles x 2 column tiles x 3 gates = 192 of the 512 registers a lone wave per SIMD may use), so a weight fragment and its address
// arithmetic feed six MFMAs instead of three. Measured: forward 0.66 -> 0.61 ms, whole step -0.06 .. -0.08 ms on three boxes. (An
// eight-wave variant - 64 windows x 32 hidden units per wave, two waves per SIMD - measured 0.58 - 0.67 ms by stash variant and
// +0.05 ms on the whole step: removed.) The gate epilogue is the row-layout one of the wide kernel, run once per row tile.
// (Round 5: the second row tile's first projected inputs requested one gate early - 32 more live registers in a kernel that already
// spills 10: 19 spilled, fp16-stash launch 0.544 -> 0.563 ms. Removed.)
// M16 (round 4, Kp a multiple of 256): the same products on v_mfma_f32_16x16x32_bf16 - same FLOP per cycle, but the chip holds a
// higher clock on that shape in three-product streams (timing-only build with the MFMAs swapped: forward 0.614 -> 0.554 ms on the
// p2_face shape; the two-product BPTT kernels gain nothing and keep the 32 x 32 shape). A wave's 64 x 64 x 3 gates are 4 x 4 x 3
// accumulator tiles; per 32-deep MFMA step m the state fragments (4 row tiles x hi / lo, one ds_read_b128 each) are read once and
// serve the three gates, the weight fragments of gate g (4 column tiles x hi / lo, 1 KB each from L2) are reloaded for step m + 1
// as soon as step m's MFMAs on them have issued: three stages of 48 MFMAs in flight between a load and its use.
template <bool STASH, bool MASK, bool S16, bool M16 = false>
__global__ __launch_bounds__(ENC_NT, 1) void enc_gru_fwd_r64_kernel(EncArgs a, EncFused q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int cg = wave % q.ncg, rg = wave / q.ncg;
  const int hid = a.hid, G3 = 3 * hid, Jp = q.Jp;
  const int R2 = 2 * q.R;                        // windows per workgroup
  const int wbase = blockIdx.x * R2;
  const int pos0 = a.start - a.hist + 1;
  const int ldx = q.Kp + 8;
  // LDS: bf16 hi / lo images of h_{s-1} (row-major [R2][Kp + 8]) | per wave two transpose tiles | biases [6][Jp] | per-row tables
  __bf16* Xhi = reinterpret_cast<__bf16*>(enc_smem);
  __bf16* Xlo = Xhi + R2 * ldx;
  float* Tw = reinterpret_cast<float*>(Xlo + R2 * ldx) + wave * (2 * 32 * ENC_TP);
  float* bias = reinterpret_cast<float*>(Xlo + R2 * ldx) + ENC_NW * (2 * 32 * ENC_TP);   // [0..2][Jp] = b_ih, [3..5][Jp] = b_hh
  unsigned* rowx = reinterpret_cast<unsigned*>(bias + 6 * Jp);
  unsigned* roww = rowx + R2;
  float* mk_tab = reinterpret_cast<float*>(roww + R2);                                   // [R2][hist] (MASK only)
  for (int i = tid; i < R2 * ldx; i += ENC_NT) { Xhi[i] = (__bf16)0.0f; Xlo[i] = (__bf16)0.0f; }
  for (int i = tid; i < 6 * Jp; i += ENC_NT) {
    const int g = i / Jp, j = i - g * Jp;
    bias[i] = j < hid ? (g < 3 ? a.b_ih[g * hid + j] : a.b_hh[(g - 3) * hid + j]) : 0.0f;
  }
  for (int i = tid; i < R2; i += ENC_NT) {
    const int w = min(wbase + i, a.F - 1);   // rows past F recompute and re-store the last window
    const int n = w / a.B, b = w - n * a.B;
    rowx[i] = (unsigned)(b * a.T + pos0 + n) * (unsigned)(G3 * 4);
    roww[i] = (unsigned)w * (unsigned)(hid * 4);
  }
  if (MASK)
    for (int i = tid; i < R2 * a.hist; i += ENC_NT) {
      const int rl = i / a.hist, s = i - rl * a.hist;
      mk_tab[i] = a.mask[(long)min(wbase + rl, a.F - 1) * a.hist + s];
    }
  // row layout of a 32 x 64 tile: lane owns columns c4 .. c4 + 3 of rows 4 i + rsub, i = 0 .. 7
  const int rsub = lane >> 4, c4 = (lane & 15) * 4;
  const int j0 = cg * 64 + c4;
  const bool jok = j0 < hid;
  {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(Tw + rt * (32 * ENC_TP) + (4 * i + rsub) * ENC_TP + c4) = z;   // h_{-1} = 0
  }
  const enc_rsrc bx = enc_buf(a.Xp, (long)a.B * a.T * G3 * 4);
  const unsigned h4 = (unsigned)hid * 4u;
  __syncthreads();

  for (int s = 0; s < a.hist; ++s) {
    constexpr int A32 = M16 ? 1 : 2, A16 = M16 ? 4 : 1;
    f32x16 acc[A32][A32][3];   // [row tile][column tile][gate]
    f32x4 acc16[A16][A16][3];  // M16: [16-row tile][16-column tile][gate]
#pragma unroll
    for (int rt = 0; rt < A32; ++rt)
#pragma unroll
      for (int t = 0; t < A32; ++t)
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[rt][t][g][r] = 0.0f;
#pragma unroll
    for (int mi = 0; mi < A16; ++mi)
#pragma unroll
      for (int ni = 0; ni < A16; ++ni)
#pragma unroll
        for (int g = 0; g < 3; ++g) acc16[mi][ni][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (M16) if (s > 0) {
      const int nct = Jp >> 4, nchunk = q.Kp >> 3;
      const int gq = lane >> 4;
      const __bf16* xh = Xhi + (rg * 64 + (lane & 15)) * ldx + 8 * ((gq >> 1) + (nchunk >> 1) * (gq & 1));
      const __bf16* xl = xh + R2 * ldx;
      ebf16x8 ahA[4], alA[4], ahB[4], alB[4];
      EncFrag fb[3][4][2];   // [gate][column tile][plane]
      auto loadA = [&](int m, ebf16x8 (&ah)[4], ebf16x8 (&al)[4]) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          ah[mi] = *reinterpret_cast<const ebf16x8*>(xh + mi * 16 * ldx + m * 16);
          al[mi] = *reinterpret_cast<const ebf16x8*>(xl + mi * 16 * ldx + m * 16);
        }
      };
      // (buffer loads: descriptor + per-lane 16 lane + a scalar fragment offset - 192 per-lane 64-bit addresses would not fit)
      const enc_rsrc bw = enc_buf(q.wfrag, 12L * q.Kp * Jp);
      const unsigned lane16 = (unsigned)lane * 16u;
      auto wload = [&](int m, int g, int ni, int plane) {
        const unsigned so = (unsigned)((((m * 3 + g) * nct + cg * 4 + ni) * 2 + plane) * 1024);
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(bw, lane16, so, 0));
      };
      // one stage: gate G of MFMA step m; its weight fragments are reloaded for step mn column tile by column tile
      auto stage = [&](auto G, const ebf16x8 (&ah)[4], const ebf16x8 (&al)[4], int mn) {
        constexpr int g = decltype(G)::value;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) acc16[mi][ni][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mi], fb[g][ni][0].v, acc16[mi][ni][g], 0, 0, 0);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) acc16[mi][ni][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], fb[g][ni][1].v, acc16[mi][ni][g], 0, 0, 0);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) acc16[mi][ni][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], fb[g][ni][0].v, acc16[mi][ni][g], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          fb[g][ni][0].u = wload(mn, g, ni, 0);
          fb[g][ni][1].u = wload(mn, g, ni, 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      using G0 = std::integral_constant<int, 0>; using G1 = std::integral_constant<int, 1>; using G2 = std::integral_constant<int, 2>;
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          fb[g][ni][0].u = wload(0, g, ni, 0);
          fb[g][ni][1].u = wload(0, g, ni, 1);
        }
      loadA(0, ahA, alA);
#pragma unroll
      for (int m = 0; m < 8; m += 2) {   // (Kp = 256: eight 32-deep steps, straight-line; loads past the end re-read the last step)
        const int m1 = m + 1, m2 = min(m + 2, 7);
        stage(G0{}, ahA, alA, m1);
        loadA(m1, ahB, alB);
        __builtin_amdgcn_sched_barrier(0);
        stage(G1{}, ahA, alA, m1);
        stage(G2{}, ahA, alA, m1);
        stage(G0{}, ahB, alB, m2);
        loadA(m2, ahA, alA);
        __builtin_amdgcn_sched_barrier(0);
        stage(G1{}, ahB, alB, m2);
        stage(G2{}, ahB, alB, m2);
      }
    }
    if constexpr (!M16) if (s > 0) {
      const int nkt = q.Kp >> 4, nct = Jp >> 5;
      const __bf16* xh = Xhi + (rg * 64 + l31) * ldx + 8 * half;
      const __bf16* xl = Xlo + (rg * 64 + l31) * ldx + 8 * half;
      ebf16x8 ah0[2], al0[2], ah1[2], al1[2];
      EncFrag f0[2][3][2], f1[2][3][2];  // [t][g][plane]
      auto load = [&](int kt, ebf16x8 (&ah)[2], ebf16x8 (&al)[2], EncFrag (&f)[2][3][2]) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          ah[rt] = *reinterpret_cast<const ebf16x8*>(xh + rt * 32 * ldx + kt * 16);
          al[rt] = *reinterpret_cast<const ebf16x8*>(xl + rt * 32 * ldx + kt * 16);
        }
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const uint4* __restrict__ wf = q.wfrag + ((long)((ENC_WKT(kt) * 3 + g) * nct + cg * 2 + t) * 2) * 64;  // uniform
            f[t][g][0].u = wf[(unsigned)lane];
            f[t][g][1].u = (wf + 64)[(unsigned)lane];
          }
      };
      auto mma = [&](const ebf16x8 (&ah)[2], const ebf16x8 (&al)[2], const EncFrag (&f)[2][3][2]) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
              acc[rt][t][g] = ENC_MFMA(al[rt], f[t][g][0].v, acc[rt][t][g], 0, 0, 0);
              acc[rt][t][g] = ENC_MFMA(ah[rt], f[t][g][1].v, acc[rt][t][g], 0, 0, 0);
              acc[rt][t][g] = ENC_MFMA(ah[rt], f[t][g][0].v, acc[rt][t][g], 0, 0, 0);
            }
      };
      load(0, ah0, al0, f0);   // every load in the steady-state loop is unconditional (see enc_gru_fwd_fused_kernel)
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {
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
    }
    __syncthreads();   // every wave has finished the MFMA phase: the state images may be overwritten
    // ---- gate epilogue in the row layout, one row tile after the other
    const enc_rsrc bhs = enc_buf(STASH ? a.hseq + (long)s * a.F * hid : nullptr, STASH ? (long)a.F * hid * 4 : 0);
    const enc_rsrc bgs = S16 ? enc_buf(STASH ? reinterpret_cast<const _Float16*>(a.gates) + (long)s * a.F * 4 * hid : nullptr,
                                       STASH ? (long)a.F * hid * 8 : 0)
                             : enc_buf(STASH ? a.gates + (long)s * a.F * 4 * hid : nullptr, STASH ? (long)a.F * hid * 16 : 0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int rsv = rsub, cv = c4, jv = j0;
      asm volatile("" : "+v"(rsv), "+v"(cv), "+v"(jv));   // keep the per-row address arithmetic inside the step loop (registers)
      const unsigned sx = (unsigned)s * (unsigned)(G3 * 4), j4 = (unsigned)jv * 4u;
      const unsigned oob = jv < hid ? 0u : 0x80000000u;
      float* T = Tw + rt * (32 * ENC_TP);
      float* Trow = T + rsv * ENC_TP + cv;                 // + 4 i * ENC_TP per row
      float* Tacc = T + (4 * half) * ENC_TP + l31;         // accumulator (t, r) at + ((r & 3) + 8 (r >> 2)) * ENC_TP + 32 t
      float* Tacc16 = T + (4 * (lane >> 4)) * ENC_TP + (lane & 15);   // M16: tile (mi, ni) register r at + (16 mi + r) * ENC_TP + 16 ni
      const int rbase = rg * 64 + rt * 32;
      f32x4 hp[8], xin[8];
      unsigned xo[8], wo[8];
      float mk[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl = rbase + 4 * i + rsv;
        xo[i] = rowx[rl] + j4 + oob;   // columns past hid: an offset outside every buffer (loads return 0, stores are dropped)
        wo[i] = roww[rl];
        mk[i] = MASK ? mk_tab[rl * a.hist + s] : 1.0f;
        hp[i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP);   // h_{s-1}, parked here by the previous step
        xin[i] = enc_ld4(bx, xo[i], sx);
      }
      auto transpose = [&](int g, f32x4 (&out)[8]) {   // gate g of this tile: accumulator layout -> row layout
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // earlier reads of the tile are done
        if constexpr (M16) {
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
              for (int r = 0; r < 4; ++r) Tacc16[(16 * mi + r) * ENC_TP + 16 * ni] = acc16[2 * rt + mi][ni][g][r];
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) Tacc[((r & 3) + 8 * (r >> 2)) * ENC_TP + 32 * t] = acc[rt][t][g][r];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = *reinterpret_cast<const f32x4*>(Trow + 4 * i * ENC_TP);
      };
      const f32x4 bir = *reinterpret_cast<const f32x4*>(bias + 0 * Jp + jv), bhr = *reinterpret_cast<const f32x4*>(bias + 3 * Jp + jv);
      const f32x4 biu = *reinterpret_cast<const f32x4*>(bias + 1 * Jp + jv), bhu = *reinterpret_cast<const f32x4*>(bias + 4 * Jp + jv);
      const f32x4 bin = *reinterpret_cast<const f32x4*>(bias + 2 * Jp + jv), bhn = *reinterpret_cast<const f32x4*>(bias + 5 * Jp + jv);
      f32x4 rr[8], uu[8], gh[8];
      transpose(0, gh);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rr[i][e] = ENC_SIG(mk[i] * xin[i][e] + bir[e] + (gh[i][e] + bhr[e]));
        if (STASH && !S16) enc_st4(rr[i], bgs, 4u * wo[i] + j4 + oob, 0);
        xin[i] = enc_ld4(bx, xo[i], sx + h4);
      }
      transpose(1, gh);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) uu[i][e] = ENC_SIG(mk[i] * xin[i][e] + biu[e] + (gh[i][e] + bhu[e]));
        if (STASH && !S16) enc_st4(uu[i], bgs, 4u * wo[i] + j4 + oob, h4);
        xin[i] = enc_ld4(bx, xo[i], sx + 2 * h4);
      }
      transpose(2, gh);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl = rbase + 4 * i + rsv;
        f32x4 ghn, nn, hn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ghn[e] = gh[i][e] + bhn[e];
          nn[e] = ENC_TANH(mk[i] * xin[i][e] + bin[e] + rr[i][e] * ghn[e]);
          hn[e] = (1.0f - uu[i][e]) * nn[e] + uu[i][e] * hp[i][e];
        }
        if (STASH && S16) {   // [window][unit][r, z, n, W_hn h] fp16: this lane's four units = 32 contiguous bytes
          const uint2 g0 = enc_pack_gates(rr[i][0], uu[i][0], nn[0], ghn[0]), g1 = enc_pack_gates(rr[i][1], uu[i][1], nn[1], ghn[1]);
          const uint2 g2 = enc_pack_gates(rr[i][2], uu[i][2], nn[2], ghn[2]), g3 = enc_pack_gates(rr[i][3], uu[i][3], nn[3], ghn[3]);
          const unsigned go = 2u * (wo[i] + j4) + oob;
          __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g0.x, g0.y, g1.x, g1.y}, bgs, go, 0, LFI_ENC_ST_AUX);
          __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g2.x, g2.y, g3.x, g3.y}, bgs, go, 16, LFI_ENC_ST_AUX);
          enc_st4(hn, bhs, wo[i] + j4 + oob, 0);
        } else if (STASH) {
          enc_st4(nn, bgs, 4u * wo[i] + j4 + oob, 2 * h4);
          enc_st4(ghn, bgs, 4u * wo[i] + j4 + oob, 3 * h4);
          enc_st4(hn, bhs, wo[i] + j4 + oob, 0);
        }
        if (jok) {
          uint2 h, l;
          split2(hn[0], hn[1], &h.x, &l.x);
          split2(hn[2], hn[3], &h.y, &l.y);
          *reinterpret_cast<uint2*>(Xhi + rl * ldx + jv) = h;
          *reinterpret_cast<uint2*>(Xlo + rl * ldx + jv) = l;
        }
        hp[i] = hn;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile's last row-wise reads are done
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(Trow + 4 * i * ENC_TP) = hp[i];   // park h_s for the next step
      if (s == a.hist - 1 && jok) {   // cat(seq[:, -1], h_n[0]): the final state, once or twice (glow/models.py:63-64)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int w = wbase + rbase + 4 * i + rsv;
          if (w < a.F) {
            float* c = a.cond + (long)w * a.ldcond + a.col + jv;
            *reinterpret_cast<f32x4*>(c) = hp[i];
            if (a.dup) *reinterpret_cast<f32x4*>(c + hid) = hp[i];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // one row tile's epilogue at a time (register pressure)
    }
    __syncthreads();   // the new state images are complete
  }
}

// ---- the forward recurrence with the gate epilogue UNDER the matrix phase (round 5; hid = 256, fragment order of
// enc_frag_weights16_kernel). enc_gru_fwd_r64_kernel runs a step as two serial parts on a lone wave per SIMD: 1152 MFMAs (18.4 k
// cycles of matrix pipe), then ~20 k cycles of transposes through LDS, gate math and stores while the pipe idles (PMC: MFMA busy
// 35 % of the wave's lifetime). Two changes let one wave fill the pipe's shadow with its own VALU work:
//   1. the product is taken TRANSPOSED (weights as the MFMA's A operand, state as B: the same products in the same order, bit for
//      bit): accumulator (mi, ni) register r is window 16 ni + (lane & 15), hidden unit 64 cg + 16 mi + 4 (lane >> 4) + r - four
//      consecutive units of one window per lane, which is the epilogue's own 16-byte layout: no transpose tiles (69 KB of LDS, six
//      write-wait-read round trips per step), and h_{s-1} stays in registers;
//   2. the wave's 64 hidden units are taken as four 16-unit tiles one after the other, each with its whole k sweep (phase p: 8
//      blocks of 36 MFMAs); tile p - 1's epilogue is independent of tile p's MFMAs and is issued between them (sched_group_barrier:
//      one MFMA, then up to LFI_T16_NV VALU). Only the last tile's epilogue is exposed. The state images are double-buffered (step parity)
//      because tile 0's new state is written while other waves still read the old one: one barrier per step.
// Weight fragments: a ring of four blocks, loaded three blocks (~1.7 k cycles) ahead and straight through the step boundary and the
// barrier; every fragment is fetched once per step and wave as before (L2 -> CU stream unchanged), the state fragments are re-read
// from LDS for each of the four tiles. Projected inputs are loaded one phase ahead of their use, three loads per two blocks.
// (timing-only experiment switches, garbage results: -DLFI_T16_NV=n VALU per MFMA in the interleave (0: the compiler's own order),
// -DLFI_T16_NO_XP no projected-input loads, -DLFI_T16_NO_W no weight loads in the loop, -DLFI_T16_NO_MFMA no products,
// -DLFI_T16_NO_EPI no gate math / stores under the products, -DLFI_T16_RING=n blocks of weight prefetch)
#ifndef LFI_T16_NV
#define LFI_T16_NV 2   // (an MFMA of this shape holds the vector issue for 8 of its 16 cycles: two 4-cycle fillers fit; measured level with 3: 0.44 - 0.46 ms)
#endif
#ifndef LFI_T16_RING
#define LFI_T16_RING 12   // weight ring: slots of one (block, gate) = two fragments; a divisor of 96; RING - 1 of them in flight
#endif
template <bool STASH, bool MASK, bool S16>
__global__ __launch_bounds__(ENC_NT, 1) void enc_gru_fwd_t16_kernel(EncArgs a, EncFused q) {
  constexpr int hid = 256, G3 = 768, ldx = 264, R2 = 64, nct = 16, IMG = R2 * ldx;
  constexpr unsigned h4 = hid * 4u;
  const int tid = threadIdx.x, lane = tid & 63, cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wl = lane & 15, jq = lane >> 4;
  const int wbase = blockIdx.x * R2;
  const int pos0 = a.start - a.hist + 1;
  // LDS: state images [step parity][hi, lo][R2][ldx] bf16 | biases [6][256] | per-row tables | masks [R2][hist]
  __bf16* X = reinterpret_cast<__bf16*>(enc_smem);
  float* bias = reinterpret_cast<float*>(X + 4 * IMG);
  unsigned* rowx = reinterpret_cast<unsigned*>(bias + 6 * hid);
  unsigned* roww = rowx + R2;
  float* mk_tab = reinterpret_cast<float*>(roww + R2);
  {
    uint4* z = reinterpret_cast<uint4*>(X);
    for (int i = tid; i < 4 * IMG / 8; i += ENC_NT) z[i] = uint4{0u, 0u, 0u, 0u};   // h_{-1} = 0
  }
  for (int i = tid; i < 6 * hid; i += ENC_NT) bias[i] = i < 3 * hid ? a.b_ih[i] : a.b_hh[i - 3 * hid];
  for (int i = tid; i < R2; i += ENC_NT) {
    const int w = min(wbase + i, a.F - 1);   // rows past F recompute and re-store the last window
    const int n = w / a.B, b = w - n * a.B;
    rowx[i] = (unsigned)(b * a.T + pos0 + n) * (unsigned)(G3 * 4);
    roww[i] = (unsigned)w * h4;
  }
  if (MASK)
    for (int i = tid; i < R2 * a.hist; i += ENC_NT) {
      const int rl = i / a.hist, s = i - rl * a.hist;
      mk_tab[i] = a.mask[(long)min(wbase + rl, a.F - 1) * a.hist + s];
    }
  const enc_rsrc bx = enc_buf(a.Xp, (long)a.B * a.T * G3 * 4);
  const enc_rsrc bw = enc_buf(q.wfrag, 12L * hid * hid);
  const unsigned lane16 = (unsigned)lane * 16u;
  const unsigned jb4 = (unsigned)(cg * 64 + 4 * jq) * 4u;   // byte offset of this lane's units in tile 0 of its wave (+ 64 per tile)
  // element offsets into an image: fragment reads (row wl of window tile ni, k chunk of lane group jq) and state writes
  const int sfr = wl * ldx + 8 * ((jq >> 1) + 16 * (jq & 1));
  const int swr = wl * ldx + cg * 64 + 4 * jq;
  // (the wave's column group goes into the per-lane offset, the plane into the instruction's immediate: what is left for the scalar
  // offset is a compile-time constant per load - 192 runtime scalars lived in VGPR lanes and cost a v_readlane each)
  const unsigned lanecg = lane16 + (unsigned)cg * 8192u;
  auto wload = [&](int m, int g, int mi, int plane) {
    const unsigned so = (unsigned)((((m * 3 + g) * nct + mi) * 2) * 1024);
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(bw, lanecg + (unsigned)plane * 1024u, so, 0));
  };
  constexpr int WR = LFI_T16_RING;
  EncFrag wr[WR][2];             // weight ring [slot = (block, gate) mod WR][plane (hi, lo)]
  ebf16x8 sh[2][4], sl[2][4];    // state fragments [buffer][window tile]
  f32x4 acc[2][4][3];            // [phase parity][window tile][gate]
  f32x4 hprev[4][4];             // h_{s-1} of this lane's units [unit tile][window tile]
  f32x4 xin[4][3];               // projected inputs of the tile whose MFMAs run now [window tile][gate]
  f32x4 rr, uu;                  // between the two halves of an epilogue chunk
  unsigned xo[4], wo[4];
  float mk[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) hprev[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < WR - 1; ++j) {
    wr[j][0].u = wload((j / 3) & 7, j % 3, (j / 3) >> 3, 0);
    wr[j][1].u = wload((j / 3) & 7, j % 3, (j / 3) >> 3, 1);
  }
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    xo[ni] = rowx[16 * ni + wl] + jb4;
    wo[ni] = roww[16 * ni + wl];
    mk[ni] = 1.0f;
  }

  for (int s = 0; s < a.hist; ++s) {
    const __bf16* Xr = X + ((s & 1) ^ 1) * (2 * IMG) + sfr;   // h_{s-1}
    __bf16* Xw = X + (s & 1) * (2 * IMG) + swr;               // h_s
    const unsigned sx = (unsigned)s * (unsigned)(G3 * 4);
    const enc_rsrc bhs = enc_buf(STASH ? a.hseq + (long)s * a.F * hid : nullptr, STASH ? (long)a.F * hid * 4 : 0);
    const enc_rsrc bgs = S16 ? enc_buf(STASH ? reinterpret_cast<const _Float16*>(a.gates) + (long)s * a.F * 4 * hid : nullptr,
                                       STASH ? (long)a.F * hid * 8 : 0)
                             : enc_buf(STASH ? a.gates + (long)s * a.F * 4 * hid : nullptr, STASH ? (long)a.F * hid * 16 : 0);
    if (MASK) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) mk[ni] = mk_tab[(16 * ni + wl) * a.hist + s];
    }
    auto sload = [&](int m, ebf16x8 (&h)[4], ebf16x8 (&l)[4]) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        h[ni] = *reinterpret_cast<const ebf16x8*>(Xr + ni * 16 * ldx + m * 16);
        l[ni] = *reinterpret_cast<const ebf16x8*>(Xr + IMG + ni * 16 * ldx + m * 16);
      }
    };
    sload(0, sh[0], sl[0]);
    f32x4 bir, bhr, biu, bhu, bin, bhn;
    auto load_biases = [&](int qt) {   // biases of unit tile qt
      const float* bb = bias + cg * 64 + 16 * qt + 4 * jq;
      bir = *reinterpret_cast<const f32x4*>(bb); bhr = *reinterpret_cast<const f32x4*>(bb + 3 * hid);
      biu = *reinterpret_cast<const f32x4*>(bb + hid); bhu = *reinterpret_cast<const f32x4*>(bb + 4 * hid);
      bin = *reinterpret_cast<const f32x4*>(bb + 2 * hid); bhn = *reinterpret_cast<const f32x4*>(bb + 5 * hid);
    };
    // projected inputs of (unit tile t, window tile ni): gates r, z in the even block of a pair, n in the odd one
    auto xload = [&](int t, int ni, int odd, f32x4 (&x)[3]) {
      const unsigned t64 = (unsigned)t * 64u;
#ifdef LFI_T16_NO_XP
      if (s == 0 && t == 0) x[0] = x[1] = x[2] = f32x4{0.1f, 0.2f, 0.3f, 0.4f} * (float)(t64 + lane);
#else
      if (!odd) {
        x[0] = enc_ld4(bx, xo[ni], sx + t64);
        x[1] = enc_ld4(bx, xo[ni], sx + h4 + t64);
      } else {
        x[2] = enc_ld4(bx, xo[ni], sx + 2 * h4 + t64);
      }
#endif
    };
    // one half of the epilogue chunk (unit tile qt, window tile ni): r, z (even) | n, h, stash, state images (odd)
    auto epi_half = [&](int qt, int ni, int odd, const f32x4 (&ac)[3], const f32x4 (&x)[3]) {
      const unsigned t64 = (unsigned)qt * 64u;   // byte offset of the tile's units in fp32 rows
      if (!odd) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          rr[e] = ENC_SIG(mk[ni] * x[0][e] + bir[e] + (ac[0][e] + bhr[e]));
          uu[e] = ENC_SIG(mk[ni] * x[1][e] + biu[e] + (ac[1][e] + bhu[e]));
        }
        if (STASH && !S16) {
          enc_st4(rr, bgs, 4u * wo[ni] + jb4, t64);
          enc_st4(uu, bgs, 4u * wo[ni] + jb4, h4 + t64);
        }
      } else {
        f32x4 ghn, nn, hn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ghn[e] = ac[2][e] + bhn[e];
          nn[e] = ENC_TANH(mk[ni] * x[2][e] + bin[e] + rr[e] * ghn[e]);
          hn[e] = (1.0f - uu[e]) * nn[e] + uu[e] * hprev[qt][ni][e];
        }
        if (STASH && S16) {   // [window][unit][r, z, n, W_hn h] fp16: this lane's four units = 32 contiguous bytes
          const uint2 g0 = enc_pack_gates(rr[0], uu[0], nn[0], ghn[0]), g1 = enc_pack_gates(rr[1], uu[1], nn[1], ghn[1]);
          const uint2 g2 = enc_pack_gates(rr[2], uu[2], nn[2], ghn[2]), g3 = enc_pack_gates(rr[3], uu[3], nn[3], ghn[3]);
          const unsigned go = 2u * (wo[ni] + jb4);
          __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g0.x, g0.y, g1.x, g1.y}, bgs, go, 2 * t64, LFI_ENC_ST_AUX);
          __builtin_amdgcn_raw_buffer_store_b128((enc_u32x4){g2.x, g2.y, g3.x, g3.y}, bgs, go, 2 * t64 + 16, LFI_ENC_ST_AUX);
          enc_st4(hn, bhs, wo[ni] + jb4, t64);
        } else if (STASH) {
          enc_st4(nn, bgs, 4u * wo[ni] + jb4, 2 * h4 + t64);
          enc_st4(ghn, bgs, 4u * wo[ni] + jb4, 3 * h4 + t64);
          enc_st4(hn, bhs, wo[ni] + jb4, t64);
        }
        {
          uint2 h, l;
          split2(hn[0], hn[1], &h.x, &l.x);
          split2(hn[2], hn[3], &h.y, &l.y);
          *reinterpret_cast<uint2*>(Xw + ni * 16 * ldx + 16 * qt) = h;
          *reinterpret_cast<uint2*>(Xw + IMG + ni * 16 * ldx + 16 * qt) = l;
        }
        hprev[qt][ni] = hn;
      }
    };
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      if (p > 0) load_biases(p - 1);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int i = p * 8 + m, ni = m >> 1;
        if (p < 4) {
          if (i + 1 < 32) sload((i + 1) & 7, sh[(i + 1) & 1], sl[(i + 1) & 1]);
          const ebf16x8 (&bh)[4] = sh[i & 1];
          const ebf16x8 (&bl)[4] = sl[i & 1];
#ifdef LFI_T16_NO_MFMA
          if (m == 0)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
              for (int n4 = 0; n4 < 4; ++n4) acc[p & 1][n4][g] = f32x4{(float)bh[n4][0], (float)bl[n4][1], (float)wr[(i * 3 + g) % WR][0].v[0], (float)wr[(i * 3 + g) % WR][1].v[1]};
#else
#pragma unroll
          for (int g = 0; g < 3; ++g) {
#ifndef LFI_T16_NO_W
            {
              const int jn = (i * 3 + g + WR - 1) % 96, in = jn / 3;   // (past the last block: the next step's first ones)
              wr[jn % WR][0].u = wload(in & 7, jn % 3, in >> 3, 0);
              wr[jn % WR][1].u = wload(in & 7, jn % 3, in >> 3, 1);
            }
#endif
            const ebf16x8 whi = wr[(i * 3 + g) % WR][0].v, wlo = wr[(i * 3 + g) % WR][1].v;
#pragma unroll
            for (int n4 = 0; n4 < 4; ++n4) {
              const f32x4 c0 = m == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[p & 1][n4][g];
              acc[p & 1][n4][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, bl[n4], c0, 0, 0, 0);
            }
#pragma unroll
            for (int n4 = 0; n4 < 4; ++n4) acc[p & 1][n4][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo, bh[n4], acc[p & 1][n4][g], 0, 0, 0);
#pragma unroll
            for (int n4 = 0; n4 < 4; ++n4) acc[p & 1][n4][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, bh[n4], acc[p & 1][n4][g], 0, 0, 0);
          }
#endif
        }
#ifdef LFI_T16_NO_EPI
        if (p > 0 && m == 7) {
          const int qt = p - 1;
#pragma unroll
          for (int n4 = 0; n4 < 4; ++n4) {
            const f32x4 hn = acc[qt & 1][n4][0] + acc[qt & 1][n4][1] + acc[qt & 1][n4][2] + xin[n4][0] + xin[n4][1] + xin[n4][2];
            uint2 h, l;
            split2(hn[0], hn[1], &h.x, &l.x);
            split2(hn[2], hn[3], &h.y, &l.y);
            *reinterpret_cast<uint2*>(Xw + n4 * 16 * ldx + 16 * qt) = h;
            *reinterpret_cast<uint2*>(Xw + IMG + n4 * 16 * ldx + 16 * qt) = l;
            hprev[qt][n4] = hn;
          }
        }
#else
        // epilogue chunk (unit tile p - 1, window tile ni): first half in the even block, second half in the odd one
        if (p > 0) epi_half(p - 1, ni, m & 1, acc[(p - 1) & 1][ni], xin[ni]);
#endif
        if (p < 4) xload(p, ni, m & 1, xin[ni]);   // projected inputs of tile p, for its epilogue one phase from now
#if LFI_T16_NV > 0
        if (p > 0 && p < 4) {
#pragma unroll
          for (int k = 0; k < 36; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, LFI_T16_NV, 0);
          }
        }
#endif
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();   // h_s is complete in its image, and every wave has read h_{s-1} for the last time
  }
  // cat(seq[:, -1], h_n[0]): the final state, once or twice (glow/models.py:63-64) - outside the step loop, whose body stays one
  // basic block (a branch would cut the scheduling regions the interleave lives in)
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int w = wbase + 16 * ni + wl;
    if (w < a.F) {
      float* c = a.cond + (long)w * a.ldcond + a.col + cg * 64 + 4 * jq;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        *reinterpret_cast<f32x4*>(c + 16 * mi) = hprev[mi][ni];
        if (a.dup) *reinterpret_cast<f32x4*>(c + hid + 16 * mi) = hprev[mi][ni];
      }
    }
  }
}

}  // namespace

// ---- which instantiation: of the variant a finished plan names
template <bool ST, bool MK>
static EncKernel enc_fwd_fused_kernel_of(bool x3) { return x3 ? enc_gru_fwd_fused_kernel<ST, MK, true> : enc_gru_fwd_fused_kernel<ST, MK, false>; }
static EncKernel enc_fwd_fused_pick(bool stash, bool mask, bool x3) {
  if (stash) return mask ? enc_fwd_fused_kernel_of<true, true>(x3) : enc_fwd_fused_kernel_of<true, false>(x3);
  return mask ? enc_fwd_fused_kernel_of<false, true>(x3) : enc_fwd_fused_kernel_of<false, false>(x3);
}
template <bool ST, bool MK, bool H>
static EncKernel enc_fwd_row_kernel_of(int variant) {   // the row-layout forward kernels: variants 2 - 5
  switch (variant) {
    case 5: return enc_gru_fwd_t16_kernel<ST, MK, H>;
    case 4: return enc_gru_fwd_r64_kernel<ST, MK, H, true>;
    case 3: return enc_gru_fwd_r64_kernel<ST, MK, H>;
    default: return enc_gru_fwd_wide_kernel<ST, MK, H>;
  }
}
static EncKernel enc_fwd_row_pick(int variant, bool stash, bool mask, bool f16) {   // (f16: the form of the stash, so only with one)
  if (stash && f16) return mask ? enc_fwd_row_kernel_of<true, true, true>(variant) : enc_fwd_row_kernel_of<true, false, true>(variant);
  if (stash) return mask ? enc_fwd_row_kernel_of<true, true, false>(variant) : enc_fwd_row_kernel_of<true, false, false>(variant);
  return mask ? enc_fwd_row_kernel_of<false, true, false>(variant) : enc_fwd_row_kernel_of<false, false, false>(variant);
}
static EncKernel enc_fwd_pick(const EncFwdPlan& p, const lfi_enc_desc* d, bool masked, bool stashed) {
  return p.variant >= 2 ? enc_fwd_row_pick(p.variant, stashed, masked, stashed && d->stash_f16) : enc_fwd_fused_pick(stashed, masked, d->precision == 1);
}

extern "C" int lfi_encode_windows_fwd_variant(const lfi_enc_desc* d, int masked, int stashed) {
  return d ? enc_plan_fwd(d, masked != 0, stashed != 0, true).variant : 0;
}

extern "C" int lfi_encode_windows_fwd(const lfi_enc_desc* d, const float* Xp, const float* whh, const float* b_ih,
                                      const float* b_hh, const float* mask, float* cond, float* gates, float* hseq,
                                      float* work, void* stream) {
  EncArgs a = {};
  int rc = fill_args(d, &a, "lfi_encode_windows_fwd");
  if (rc) return rc;
  LFI_REQUIRE(Xp && whh && b_ih && b_hh && cond && work, "lfi_encode_windows_fwd: null pointer");
  a.Xp = Xp; a.b_ih = b_ih; a.b_hh = b_hh; a.mask = mask; a.cond = cond; a.gates = gates; a.hseq = hseq;
  a.stamps = g_lfi_stamps;
  hipStream_t st = (hipStream_t)stream;
  const int hid = d->hid, F = a.F;
  LFI_REQUIRE(!d->stash_f16 || lfi_encode_windows_stash_f16_ok(d), "lfi_encode_windows_fwd: lfi_enc_desc.stash_f16 is set for a shape "
              "whose gate stash is fp32 (ask lfi_encode_windows_stash_f16_ok)");
  if (d->lstm) {   // "enc: lstm": one GEMM + one gate kernel per history step (in no shipped hparams file: not fused)
    LFI_REQUIRE(gates && hseq, "lfi_encode_windows_fwd: the LSTM encoder keeps its cell state in the gate stash (5 * hid per row)");
    const int blocks = ew_blocks((long)F * hid);
    for (int s = 0; s < d->hist; ++s) {
      if (s > 0) {
        lfi_gemm_desc g = {};
        g.M = F; g.N = 4 * hid; g.K = hid; g.batch = 1;
        g.A = hseq + (long)(s - 1) * F * hid; g.lda = hid; g.a_kcontig = 1;
        g.B = whh; g.ldb = hid; g.b_kcontig = 1;
        g.C = work; g.ldc = 4 * hid; g.precision = d->precision;
        if ((rc = lfi_gemm_f32(&g, stream))) return rc;
      }
      hipLaunchKernelGGL(enc_lstm_gate_fwd_kernel, dim3(blocks), dim3(256), 0, st, a, s, s > 0 ? work : nullptr);
    }
    LFI_LAUNCH_CHECK("lfi_encode_windows_fwd (lstm)");
    return LFI_OK;
  }
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  EncFwdPlan p = enc_plan_fwd(d, mask != nullptr, gates != nullptr, al16(Xp) && al16(cond) && (!gates || (al16(gates) && al16(hseq))));
  if (p.variant) {
    LFI_REQUIRE(!gates || hseq, "lfi_encode_windows_fwd: the gate stash needs the state stash too");
    // (without a gate stash nothing is kept for a backward pass: hseq is not written either)
    LFI_REQUIRE(p.variant >= 2 || !(gates && d->stash_f16), "lfi_encode_windows_fwd: an fp16 gate stash (lfi_enc_desc.stash_f16) needs the row-layout "
                "kernel (lfi_encode_windows_stash_f16_ok) and 16-byte aligned buffers");
    const EncKernel kernel = enc_fwd_pick(p, d, mask != nullptr, gates != nullptr);
    enc_build_weights(p.weights, &p.q, whh, hid, 1, work, st);
    if ((rc = enc_set_lds(kernel, p.lds))) return rc;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(ENC_NT), p.lds, st, a, p.q);
    LFI_LAUNCH_CHECK(p.variant >= 3 ? "lfi_encode_windows_fwd (fused, two row tiles per wave)"
                     : p.variant == 2 ? "lfi_encode_windows_fwd (fused, row-layout epilogue)" : "lfi_encode_windows_fwd (fused)");
    return LFI_OK;
  }
  LFI_REQUIRE(hseq, "lfi_encode_windows_fwd: hid > 256 needs the state stash hseq");
  const int blocks = ew_blocks((long)F * hid);
  for (int s = 0; s < d->hist; ++s) {
    if (s > 0) {
      lfi_gemm_desc g = {};
      g.M = F; g.N = 3 * hid; g.K = hid; g.batch = 1;
      g.A = hseq + (long)(s - 1) * F * hid; g.lda = hid; g.a_kcontig = 1;
      g.B = whh; g.ldb = hid; g.b_kcontig = 1;  // (h W_hh^T)[w][n] = sum_k h[w][k] W_hh[n][k]
      g.C = work; g.ldc = 3 * hid; g.precision = d->precision;
      if ((rc = lfi_gemm_f32(&g, stream))) return rc;
    }
    hipLaunchKernelGGL(enc_gate_fwd_kernel, dim3(blocks), dim3(256), 0, st, a, s, s > 0 ? work : nullptr);
  }
  LFI_LAUNCH_CHECK("lfi_encode_windows_fwd");
  return LFI_OK;
}
