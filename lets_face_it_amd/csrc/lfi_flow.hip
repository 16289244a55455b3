// The conditional-Glow flow itself: FlowStep.normal_flow / reverse_flow (glow/models.py:311-373), f_seq.forward
// (:204-214), ActNorm2d / InvertibleConv1x1 / LinearZeros (glow/modules.py), SeqGlow.loss (:563-565), and their
// gradients, as one "cell" kernel per (timestep n, flow step k).
//
// Dependency structure. Cell (n, k) needs the flow variable from (n, k-1) and the coupling net's recurrent state from
// (n-1, k) (the GRUCell hidden state is carried over timesteps, glow/models.py:193-214), so the (n, k) grid is walked
// in anti-diagonals: all cells with n + k = d are independent and run in ONE launch (up to min(N, Ks) cells x B/16
// batch tiles of workgroups); N + Ks - 1 launches replace the reference's N * Ks * ~340 ATen calls. Everything that
// does not depend on the recurrence (cond_transform, the W_ih[:, Ch:] c product) is hoisted into big GEMMs by the
// caller (gic), and InvertibleConv1x1's W = P L U is built once per optimiser step (lfi_flow_prep) rather than per
// call (glow/modules.py:163-173).
//
// Cell kernel: 16 samples x all channels per workgroup, 4 waves; the four small GEMMs of a cell
// (a W, [z1|h] [Wz|Whh]^T, h' Wfl^T and their transposes in backward) run on v_mfma_f32_16x16x4_f32 with the A
// operand staged k-major in LDS and the weights streamed from L2 as coalesced row segments; all elementwise math
// (actnorm, gates, LinearZeros scaling, affine coupling, log-det) is fused around them in fp32.
//
// This unit is the TRAINING side: the diagonal and the persistent walks, forward and backward, the NLL, the prep kernels, the invconv
// backward, the ActNorm init and the parameter gradients. The per-frame side - the samplers' and the streaming sessions' cells and
// chains and their entry points - is lfi_flow_chain.hip; what both use (the generic cell bodies among it) is lfi_flow_cells.h.
#include "lfi_flow_cells.h"

namespace {

__global__ __launch_bounds__(NT) void flow_diag_fwd_kernel(FlowK f, int d, int klo) {
  const int k = klo + blockIdx.y, n = d - k;
  const long fr = (long)n * f.B;  // first frame of this timestep
  CellIO io;
  io.k = k; io.rows = f.B;
  if (k == 0) { io.x_in = f.x0 + (long)(f.start + n) * f.C; io.ldx = (long)f.T * f.C; }
  else { io.x_in = f.sX + ((long)(k - 1) * f.F + fr) * f.ldc; io.ldx = f.ldc; }
  io.h_prev = n > 0 ? f.sH + ((long)k * f.F + fr - f.B) * f.H : nullptr;
  io.c_prev = (f.lstm && n > 0) ? f.sC + ((long)k * f.F + fr - f.B) * f.H : nullptr;
  io.c_out = f.lstm ? f.sC + ((long)k * f.F + fr) * f.H : nullptr;
  io.gic = f.gic + ((long)k * f.F + fr) * f.G;
  io.a_out = f.sA + ((long)k * f.F + fr) * f.ldc;
  io.y_out = f.sY + ((long)k * f.F + fr) * f.ldc;
  io.x_out = f.sX + ((long)k * f.F + fr) * f.ldc; io.ldxo = f.ldc;
  io.ld_c = f.ldc; io.ld_o = f.ldo;
  io.h_out = f.sH + ((long)k * f.F + fr) * f.H;
  io.g_out = f.sG + ((long)k * f.F + fr) * 4 * f.H;
  io.o_out = f.sO + ((long)k * f.F + fr) * f.ldo;
  io.l_out = f.sL + (long)k * f.F + fr;
  io.l_accumulate = 0;
  cell_forward(f, io, blockIdx.x * MB);
}

// nll[f] = -(logdet + sum_c -0.5 (z^2 + log 2pi)) / ln 2   (SeqGlow.loss, glow/models.py:563-565)
// 64 frames per workgroup: their z rows (C floats at stride ldc) come in through LDS with coalesced loads (and leave to the
// caller's z the same way); thread i then sums frame i's row in column order - one thread per frame reading its row straight from
// memory took 30 us of the step's critical path between the two walks for 3.7 MB. C > NLL_CMAX: that form (STAGED = false).
template <bool STAGED>
__global__ __launch_bounds__(256) void flow_nll_kernel(FlowK f, float* __restrict__ z, float* __restrict__ nll) {
  extern __shared__ float nll_rows[];   // [NLL_FR][C + 1]
  const int nfr = STAGED ? NLL_FR : 256;
  const long fr0 = (long)blockIdx.x * nfr;
  const float* zbase = f.sX + (long)(f.Ks - 1) * f.F * f.ldc;
  if (STAGED) {
    const long left = f.F - fr0;
    const int tot = (int)(left < NLL_FR ? left : NLL_FR) * f.C;
    for (int e = threadIdx.x; e < tot; e += 256) {
      const int r = e / f.C, c = e - r * f.C;
      const float v = zbase[(fr0 + r) * f.ldc + c];
      nll_rows[r * (f.C + 1) + c] = v;
      if (z) z[fr0 * f.C + e] = v;
    }
    __syncthreads();
  }
  const long fr = fr0 + threadIdx.x;
  if (threadIdx.x >= nfr || fr >= f.F) return;
  float ld = f.ldconst[0];
  for (int k = 0; k < f.Ks; ++k) ld += f.sL[(long)k * f.F + fr];
  const float* zz = STAGED ? nll_rows + threadIdx.x * (f.C + 1) : zbase + fr * f.ldc;
  float lp = 0.0f;
  for (int c = 0; c < f.C; ++c) {
    const float v = zz[c];
    lp += -0.5f * (v * v + LOG2PI_F);
    if (!STAGED && z) z[fr * f.C + c] = v;
  }
  // a persistent walk that gave up (bounded spin timed out, abort word set) must not pass for a result: poison it
  const bool aborted = f.pipe && f.pipe[1] != 0u;
  nll[fr] = aborted ? __builtin_nanf("") : -(ld + lp) / LN2_F;
}

// ------------------------------------------------------------------------------------------- backward cell
struct CarveB {
  int Dl, Gi, Gh, Dy, Cy, Pl, total;
};
__host__ __device__ inline CarveB carve_bwd(int C, int H, int Cout, int G) {
  CarveB c;
  int o = 0;
  c.Dl = o; o += Cout * LT;
  c.Gi = o; o += G * LT;
  c.Gh = o; o += G * LT;
  c.Dy = o; o += C * LT;
  c.Cy = o; o += H * LT;
  c.Pl = o; o += MB * (Cout + 1);
  c.total = o;
  return c;
}

__global__ __launch_bounds__(NT) void flow_diag_bwd_kernel(FlowK f, int d, int klo) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int k = klo + blockIdx.y, n = d - k;
  const int b0 = blockIdx.x * MB;
  const int B = f.B, C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G, I = f.I;
  const long LC = f.ldc, LO = f.ldo;   // stash row strides
  const long fr = (long)n * B;
  const long kf = (long)k * f.F + fr;
  const CarveB cv = carve_bwd(C, H, Cout, G);
  float* Dl = flow_smem + cv.Dl;
  float* Gi = flow_smem + cv.Gi;
  float* Gh = flow_smem + cv.Gh;
  float* Dy = flow_smem + cv.Dy;
  float* Cy = flow_smem + cv.Cy;
  float* Pl = flow_smem + cv.Pl;
  const int ldp = Cout + 1;
  const bool last = k == f.Ks - 1;
  const float gz = f.gscale / LN2_F;   // d loss / d z = z * gz   (prior term)
  const float dl = -f.gscale / LN2_F;  // d loss / d logdet
  const float* dxo = last ? f.sX + kf * LC : f.bDx + ((long)(k + 1) * f.F + fr) * LC;
  const float dxs = last ? gz : 1.0f;

  // Q0: coupling backward + LinearZeros scale
  const float* Y = f.sY + kf * LC;
  const float* O = f.sO + kf * LO;
  const float* lfl = f.p.l_fl + (long)k * Cout;
  for (int idx = tid; idx < MB * C2; idx += NT) {
    const int i = idx / C2, jj = idx - i * C2;
    const int row = b0 + i;
    float dz2 = 0.0f, d0 = 0.0f, d1 = 0.0f, p0 = 0.0f, p1 = 0.0f;
    if (row < B) {
      const float dz2n = dxo[(long)row * LC + Ch + jj] * dxs;
      if (f.affine) {
        const float oe = O[(long)row * LO + 2 * jj], oo = O[(long)row * LO + 2 * jj + 1];
        const float sraw = sigmoidf_(oo + 2.0f);
        const float sc = fmaxf(sraw, f.eps);
        const float z2 = Y[(long)row * LC + Ch + jj];
        dz2 = dz2n * sc;
        const float dsc = dz2n * (z2 + oe) + dl / sc;
        const float dsr = sraw >= f.eps ? dsc : 0.0f;
        d0 = dz2;                             // d o_even (shift)
        d1 = dsr * sraw * (1.0f - sraw);      // d o_odd
        p0 = d0 * oe * 3.0f; p1 = d1 * oo * 3.0f;
      } else {
        const float oe = O[(long)row * LO + jj];
        dz2 = dz2n; d0 = dz2n; p0 = d0 * oe * 3.0f;
      }
    }
    Dy[(Ch + jj) * LT + i] = dz2;
    if (row < B) f.bDy[kf * LC + (long)row * LC + Ch + jj] = dz2;
    if (f.affine) {
      const int c0 = 2 * jj, c1 = 2 * jj + 1;
      const float dl0 = d0 * expf(3.0f * lfl[c0]), dl1 = d1 * expf(3.0f * lfl[c1]);
      Dl[c0 * LT + i] = dl0; Dl[c1 * LT + i] = dl1;
      Pl[i * ldp + c0] = p0; Pl[i * ldp + c1] = p1;
      if (row < B) { f.bDlin[kf * LO + (long)row * LO + c0] = dl0; f.bDlin[kf * LO + (long)row * LO + c1] = dl1; }
    } else {
      const float dl0 = d0 * expf(3.0f * lfl[jj]);
      Dl[jj * LT + i] = dl0;
      Pl[i * ldp + jj] = p0;
      if (row < B) f.bDlin[kf * LO + (long)row * LO + jj] = dl0;
    }
  }
  __syncthreads();
  if (tid < Cout) {
    float s = 0.0f;
    for (int i = 0; i < MB; ++i) s += Pl[i * ldp + tid];
    f.bPlfl[(((long)k * f.N + n) * f.nbt + blockIdx.x) * Cout + tid] = s;
  }

  // Q1: d h' = dlin Wfl + dh from the next timestep; GRU cell backward
  const int nht = (H + 15) >> 4;
  {
    const float* wfl = f.p.w_fl + (long)k * Cout * H;
    const float* dhf = (n < f.N - 1) ? f.bDh + ((long)k * f.F + fr + B) * H : nullptr;
    const float* gs_base = f.sG + kf * 4 * H;
    const float* hp_base = n > 0 ? f.sH + ((long)k * f.F + fr - B) * H : nullptr;
    if (f.lstm) {
      const float* dcf = (n < f.N - 1) ? f.bDc + ((long)k * f.F + fr + B) * H : nullptr;
      const float* cp_base = n > 0 ? f.sC + ((long)k * f.F + fr - B) * H : nullptr;
      const float* c_base = f.sC + kf * H;
      float* dco = f.bDc + kf * H;
      for (int t = wave; t < nht; t += NW) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile16_lds_glb(acc, Dl, LT, wfl + t * 16, H, Cout, min(16, H - t * 16), lane);
        const int j = t * 16 + l15;
        if (j < H) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = lq * 4 + r;
            const int row = b0 + i;
            float dai = 0.f, daf = 0.f, dag = 0.f, dao = 0.f;
            if (row < B) {
              const float dhn = acc[r] + (dhf ? dhf[(long)row * H + j] : 0.0f);
              const float* gs = gs_base + (long)row * 4 * H;
              const f32x4 g4 = *reinterpret_cast<const f32x4*>(gs + 4 * j);
              const float ii = g4[0], ff = g4[1], gg = g4[2], oo = g4[3];
              const float tc = tanhf_(c_base[(long)row * H + j]);
              const float cp = cp_base ? cp_base[(long)row * H + j] : 0.0f;
              const float dc2 = dhn * oo * (1.0f - tc * tc) + (dcf ? dcf[(long)row * H + j] : 0.0f);
              dai = dc2 * gg * ii * (1.0f - ii);
              daf = dc2 * cp * ff * (1.0f - ff);
              dag = dc2 * ii * (1.0f - gg * gg);
              dao = dhn * tc * oo * (1.0f - oo);
              dco[(long)row * H + j] = dc2 * ff;
              float* gi = f.bDgi + kf * G + (long)row * G;
              gi[j] = dai; gi[H + j] = daf; gi[2 * H + j] = dag; gi[3 * H + j] = dao;
              float* gh = f.bDgh + kf * G + (long)row * G;
              gh[j] = dai; gh[H + j] = daf; gh[2 * H + j] = dag; gh[3 * H + j] = dao;
            }
            Gi[j * LT + i] = dai; Gi[(H + j) * LT + i] = daf; Gi[(2 * H + j) * LT + i] = dag; Gi[(3 * H + j) * LT + i] = dao;
            Gh[j * LT + i] = dai; Gh[(H + j) * LT + i] = daf; Gh[(2 * H + j) * LT + i] = dag; Gh[(3 * H + j) * LT + i] = dao;
            Cy[j * LT + i] = 0.0f;
          }
        }
      }
    } else
    for (int t = wave; t < nht; t += NW) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile16_lds_glb(acc, Dl, LT, wfl + t * 16, H, Cout, min(16, H - t * 16), lane);
      const int j = t * 16 + l15;
      if (j < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const int row = b0 + i;
          float dar = 0.f, dau = 0.f, dan = 0.f, danr = 0.f, cy = 0.f;
          if (row < B) {
            const float dhn = acc[r] + (dhf ? dhf[(long)row * H + j] : 0.0f);
            const float* gs = gs_base + (long)row * 4 * H;
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gs + 4 * j);
            const float rr = g4[0], uu = g4[1], nn = g4[2], ghn = g4[3];
            const float hp = hp_base ? hp_base[(long)row * H + j] : 0.0f;
            const float du = dhn * (hp - nn);
            const float dn = dhn * (1.0f - uu);
            cy = dhn * uu;
            dan = dn * (1.0f - nn * nn);
            dau = du * uu * (1.0f - uu);
            dar = dan * ghn * rr * (1.0f - rr);
            danr = dan * rr;
            float* gi = f.bDgi + kf * G + (long)row * G;
            gi[j] = dar; gi[H + j] = dau; gi[2 * H + j] = dan;
            float* gh = f.bDgh + kf * G + (long)row * G;
            gh[j] = dar; gh[H + j] = dau; gh[2 * H + j] = danr;
          }
          Gi[j * LT + i] = dar; Gi[(H + j) * LT + i] = dau; Gi[(2 * H + j) * LT + i] = dan;
          Gh[j * LT + i] = dar; Gh[(H + j) * LT + i] = dau; Gh[(2 * H + j) * LT + i] = danr;
          Cy[j * LT + i] = cy;
        }
      }
    }
  }
  __syncthreads();

  // Q2: d h_prev = dgh Whh + carry (to timestep n-1);  d z1 = dgi W_ih[:, :Ch] + pass-through
  {
    const float* whh = f.p.w_hh + (long)k * G * H;
    if (n > 0) {
      float* dho = f.bDh + kf * H;
      for (int t = wave; t < nht; t += NW) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile16_lds_glb(acc, Gh, LT, whh + t * 16, H, G, min(16, H - t * 16), lane);
        const int j = t * 16 + l15;
        if (j < H) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = lq * 4 + r;
            const int row = b0 + i;
            if (row < B) dho[(long)row * H + j] = acc[r] + Cy[j * LT + i];
          }
        }
      }
    }
    const float* wih = f.p.w_ih + (long)k * G * I;
    const int nzt = (Ch + 15) >> 4;
    for (int t = NW - 1 - wave; t < nzt; t += NW) {  // start from the other end so these tiles land on the less loaded waves
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile16_lds_glb(acc, Gi, LT, wih + t * 16, I, G, min(16, Ch - t * 16), lane);
      const int c = t * 16 + l15;
      if (c < Ch) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const int row = b0 + i;
          float v = 0.0f;
          if (row < B) {
            v = acc[r] + dxo[(long)row * LC + c] * dxs;
            f.bDy[kf * LC + (long)row * LC + c] = v;
          }
          Dy[c * LT + i] = v;
        }
      }
    }
  }
  __syncthreads();

  // Q3: d a = dy W^T ; actnorm backward ; d x_in to flow step k-1
  {
    const float* Wt = f.Wt + (long)k * C * C;
    const float* anl = f.p.an_logs + (long)k * C;
    const float* A = f.sA + kf * LC;
    float* dxi = k > 0 ? f.bDx + kf * LC : nullptr;
    float* pan = f.bPan + (((long)k * f.N + n) * f.nbt + blockIdx.x) * 2 * C;
    const int nt = (C + 15) >> 4;
    for (int t = wave; t < nt; t += NW) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile16_lds_glb(acc, Dy, LT, Wt + t * 16, C, C, min(16, C - t * 16), lane);
      const int c = t * 16 + l15;
      float sl = 0.0f, sb = 0.0f;
      if (c < C) {
        const float es = expf(anl[c]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = b0 + lq * 4 + r;
          if (row < B) {
            const float da = acc[r];
            sl += da * A[(long)row * LC + c];
            sb += da * es;
            if (dxi) dxi[(long)row * LC + c] = da * es;
          }
        }
      }
      sl += __shfl_xor(sl, 16, 64); sl += __shfl_xor(sl, 32, 64);
      sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
      if (lq == 0 && c < C) { pan[c] = sl; pan[C + c] = sb; }
    }
  }
}

template <int NG>
__global__ __launch_bounds__(NT) void flow_diag_fwd_fast_kernel(FlowK f, int d, int klo) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kq = lane >> 4;
  const int ri = tid >> 5, cl = tid & 31;  // elementwise thread map
  int cell, bt;
  flow_cell_of_block(f.nbt, &cell, &bt);
  const int k = klo + cell, n = d - k;
  const int b0 = bt * MB;
  const int B = f.B, C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const long LC = f.ldc, LO = f.ldo;   // stash row strides
  const long fr = (long)n * B;
  const long kf = (long)k * f.F + fr;
  const CarveF cv = carve_fast_fwd(C, C16, H16, Ch16, Cout);
  float* At = flow_smem + cv.At;
  float* Ht = flow_smem + cv.Ht;
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  const int ldy = C + 1, ldo = Cout + 1;
  const int nbC = C16 >> 4, nbZ = Ch16 >> 4, nbH = H16 >> 4;
  LFI_STAMP(0);

  // ---- weights of P1 (this wave's 16 output channels of W) and P2 (its 16 hidden units, NG gates), gic/bias of its rows
  const bool t1 = wave * 16 < C, t2 = wave * 16 < H, t3 = wave * 16 < Cout;
  const int tcol = wave * 16 + l15;
  f32x4 w1[FB_C], wz[NG][FB_Z], wh[NG][FB_H];
  load_frag<FB_C>(w1, f.pW + (long)k * C16 * C16, C16, tcol, kq, nbC, t1);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    load_frag<FB_Z>(wz[g], f.pwz + (long)k * Ch16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbZ, t2);
    load_frag<FB_H>(wh[g], f.pwh + (long)k * H16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbH, t2);
  }
  const int j2 = tcol;                    // hidden unit of this lane in P2
  const bool j2ok = j2 < H;
  float gc[4][NG], bh[NG], cprev[4];
  {
    const float* gicb = f.gic + kf * G;
    const float* bhh = f.p.b_hh + (long)k * G;
    const float* cpb = (NG == 4 && n > 0) ? f.sC + (kf - B) * H : nullptr;
    const int jc = j2ok ? j2 : 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) bh[g] = bhh[g * H + jc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(b0 + kq * 4 + r, B - 1);
#pragma unroll
      for (int g = 0; g < NG; ++g) gc[r][g] = gicb[(long)row * G + g * H + jc];
      cprev[r] = cpb ? cpb[(long)row * H + jc] : 0.0f;
    }
  }
  LFI_STAMP(1);

  // ---- P0: actnorm (glow/modules.py:45-52); stage a, h_prev k-major; zero the k padding
  {
    const int row = b0 + ri;
    const bool rok = row < B;
    const float* xin = (k == 0) ? f.x0 + ((long)row * f.T + f.start + n) * C : f.sX + (kf - f.F + row) * LC;
    const float* anb = f.p.an_bias + (long)k * C;
    const float* anl = f.p.an_logs + (long)k * C;
    for (int c = cl; c < C16; c += 32) {
      float a = 0.0f;
      if (c < C && rok) {
        a = (xin[c] + anb[c]) * expf(anl[c]);
        f.sA[(kf + row) * LC + c] = a;
      }
      At[c * LT + ri] = a;
    }
    const float* hp = n > 0 ? f.sH + (kf - B + row) * H : nullptr;
    for (int j = cl; j < H16; j += 32) {
      Ht[j * LT + ri] = (hp && rok && j < H) ? hp[j] : 0.0f;
      if (j >= H) Hn[j * LT + ri] = 0.0f;
    }
    for (int c = Ch + cl; c < Ch16; c += 32) Zt[c * LT + ri] = 0.0f;
  }
  __syncthreads();
  LFI_STAMP(2);

  // ---- P1: y = a W   (InvertibleConv1x1.forward, glow/modules.py:186)
  if (t1) {
    const f32x4 acc = mma16_reg<FB_C>(At + kq * LT + l15, w1, nbC);
    const int c = tcol;
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        const int row = b0 + i;
        const float v = acc[r];
        Yrm[i * ldy + c] = v;
        if (c < Ch) Zt[c * LT + i] = v;
        if (row < B) f.sY[(kf + row) * LC + c] = v;
      }
    }
  }
  // weights of P3 (this wave's 16 outputs of LinearZeros): in flight under P2
  f32x4 w3[FB_H];
  load_frag<FB_H>(w3, f.pwfl + (long)k * H16 * Co16, Co16, tcol, kq, nbH, t3);
  __syncthreads();
  LFI_STAMP(3);

  // ---- P2: recurrent cell of the coupling net (f_seq.forward, glow/models.py:204-214)
  if (t2) fast_cell_p2<NG>(f, Zt, Ht, Hn, wz, wh, gc, bh, cprev, nbZ, nbH, tcol, kq, l15, b0, B,
                           f.sH + kf * H, NG == 4 ? f.sC + kf * H : nullptr, f.sG + kf * 4 * H);
  __syncthreads();
  LFI_STAMP(4);

  // ---- P3: o = (h' Wfl^T + b) exp(3 logs)   (LinearZeros, glow/modules.py:93-95)
  if (t3) {
    const int cj = tcol < Cout ? tcol : 0;
    fast_cell_p3(f, k, Hn, Orm, w3, nbH, tcol, kq, l15, b0, B, f.sO + kf * LO, LO, f.p.b_fl[(long)k * Cout + cj],
                 expf(3.0f * f.p.l_fl[(long)k * Cout + cj]));
  }
  __syncthreads();
  LFI_STAMP(5);

  // ---- P4: coupling (glow/models.py:330-341), pass-through half, log-det of the coupling (wavefront shuffle sum)
  {
    const int row = b0 + ri;
    const bool rok = row < B;
    float lg = 0.0f;
    if (cl < C2) {
      const float z2 = Yrm[ri * ldy + Ch + cl];
      float z2n;
      if (f.affine) {
        const float shift = Orm[ri * ldo + 2 * cl];
        const float sraw = sigmoidf_(Orm[ri * ldo + 2 * cl + 1] + 2.0f);
        const float sc = fmaxf(sraw, f.eps);
        z2n = (z2 + shift) * sc;
        lg = logf(sc);
      } else {
        z2n = z2 + Orm[ri * ldo + cl];
      }
      if (rok) f.sX[(kf + row) * LC + Ch + cl] = z2n;
    }
    if (cl < Ch && rok) f.sX[(kf + row) * LC + cl] = Yrm[ri * ldy + cl];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) lg += __shfl_xor(lg, o, 64);  // the 32 lanes of one row
    if (cl == 0 && rok) f.sL[kf + row] = lg;
  }
  LFI_STAMP(6);
}

template <int NG, bool X3>
__global__ __launch_bounds__(NT) void flow_pipe_fwd_kernel(FlowK f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15_0 = lane & 15, kq_0 = lane >> 4;
  const int ri_0 = tid >> 5, cl_0 = tid & 31;  // elementwise thread map
  __shared__ int s_id, s_ok, s_rdy;
  if (tid == 0) s_id = (int)atomicAdd(f.pipe, 1u);
  __syncthreads();
  const int id = s_id;
  const int nbt = f.nbt;
  const int k = id / nbt, bt = id - k * nbt;   // tickets in arrival order: (k - 1, bt) always started before (k, bt)
  if (k >= f.Ks) return;
  unsigned* abort_w = f.pipe + 1;
  unsigned* prog = f.pipe + PIPE_WALK_HDR;
  const bool fenced = f.pipe_fence != 0;
  const int b0 = bt * MB;
  const int B = f.B, C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const long LC = f.ldc, LO = f.ldo;
  const CarveF cv = carve_fast_fwd(C, C16, H16, Ch16, Cout);
  float* At = flow_smem + cv.At;
  float* Ht = flow_smem + cv.Ht;   // h of the previous timestep
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;   // h of this timestep (the two swap every iteration)
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  const int ldy = C + 1, ldo = Cout + 1;
  const int nbC = C16 >> 4, nbZ = Ch16 >> 4, nbH = H16 >> 4;

  // ---- this workgroup's weights, once: P1 (16 output channels of W), P2 (16 hidden units, NG gates), P3 (16 outputs)
  const bool t1 = wave * 16 < C, t2 = wave * 16 < H, t3 = wave * 16 < Cout;
  const int tcol_0 = wave * 16 + l15_0;
  f32x4 wz[X3 ? 1 : NG][FB_Z], wh[X3 ? 1 : NG][FB_H];          // exact f32 form
  X3Frag wzx[X3 ? NG : 1][FB_Z / 2], whx[X3 ? NG : 1][FB_H / 2];  // bf16 x 3 form: the same fragments, split once
  {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      f32x4 tz[FB_Z], th[FB_H];
#pragma unroll
      for (int b = 0; b < FB_Z; ++b) tz[b] = zero4;
#pragma unroll
      for (int b = 0; b < FB_H; ++b) th[b] = zero4;
      load_frag<FB_Z>(tz, f.pwz + (long)k * Ch16 * NG * H16, NG * H16, g * H16 + tcol_0, kq_0, nbZ, t2);
      load_frag<FB_H>(th, f.pwh + (long)k * H16 * NG * H16, NG * H16, g * H16 + tcol_0, kq_0, nbH, t2);
      if (X3) {
#pragma unroll
        for (int b = 0; b < FB_Z / 2; ++b) wzx[g][b] = x3_pack(tz[2 * b], tz[2 * b + 1]);
#pragma unroll
        for (int b = 0; b < FB_H / 2; ++b) whx[g][b] = x3_pack(th[2 * b], th[2 * b + 1]);
      } else {
#pragma unroll
        for (int b = 0; b < FB_Z; ++b) wz[X3 ? 0 : g][b] = tz[b];
#pragma unroll
        for (int b = 0; b < FB_H; ++b) wh[X3 ? 0 : g][b] = th[b];
      }
    }
  }
  // P1 / P3 weights: each owning wave parks its fragments in LDS (its own region, its own lanes: no barrier needed)
  f32x4* w1s = reinterpret_cast<f32x4*>(flow_smem + ((cv.total + 3) & ~3)) + wave * nbC * 64 + lane;
  f32x4* w3s = reinterpret_cast<f32x4*>(flow_smem + ((cv.total + 3) & ~3)) + nbC * nbC * 64 + wave * nbH * 64 + lane;
  if (t1) {
    const f32x4* p = reinterpret_cast<const f32x4*>(f.pW + (long)k * C16 * C16) + (long)kq_0 * C16 + tcol_0;
    for (int b = 0; b < nbC; ++b) w1s[b * 64] = p[(long)b * 4 * C16];
  }
  if (t3) {
    const f32x4* p = reinterpret_cast<const f32x4*>(f.pwfl + (long)k * H16 * Co16) + (long)kq_0 * Co16 + tcol_0;
    for (int b = 0; b < nbH; ++b) w3s[b * 64] = p[(long)b * 4 * Co16];
  }
  // bf16 x 3: operand images of the recurrent cell (fast_cell_p2_x3_img)
  const int ldxi = Ch16 + H16 + 8;
  __bf16* imgb = reinterpret_cast<__bf16*>(flow_smem + pipe_fwd_img_offset(C, C16, H16, Ch16, Cout, Co16));
  __bf16* ich = imgb;                       // current buffer: z1 of this timestep | h of the previous one (hi; lo at + MB * ldxi)
  __bf16* inh = imgb + 2 * MB * ldxi;       // next buffer: receives h of this timestep
  if (X3)
    for (int q = tid; q < 4 * MB * ldxi; q += NT) imgb[q] = (__bf16)0.0f;
  const int j2 = tcol_0;
  const int jc = j2 < H ? j2 : 0;
  float bh[NG], cprev[4] = {0.f, 0.f, 0.f, 0.f};
  {
    const float* bhh = f.p.b_hh + (long)k * G;
#pragma unroll
    for (int g = 0; g < NG; ++g) bh[g] = bhh[g * H + jc];
  }
  const float flb = tcol_0 < Cout ? f.p.b_fl[(long)k * Cout + tcol_0] : 0.0f;              // LinearZeros bias and scale
  const float fls = tcol_0 < Cout ? expf(3.0f * f.p.l_fl[(long)k * Cout + tcol_0]) : 0.0f;
  // actnorm of this flow step for the (at most two) channels this thread handles in P0
  float anb[2], ans[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = cl_0 + 32 * u;
    anb[u] = c < C ? f.p.an_bias[(long)k * C + c] : 0.0f;
    ans[u] = c < C ? expf(f.p.an_logs[(long)k * C + c]) : 0.0f;
  }
  // zero state and the k padding of the LDS operands (never written again)
  for (int j = cl_0; j < H16; j += 32) {
    Ht[j * LT + ri_0] = 0.0f;
    Hn[j * LT + ri_0] = 0.0f;
  }
  for (int c = Ch + cl_0; c < Ch16; c += 32) Zt[c * LT + ri_0] = 0.0f;
  __syncthreads();

  const int row = b0 + ri_0;          // elementwise phases: this thread's sample
  const bool rok = row < B;
  // Look-ahead acquire. Every cell paid two dependent L2 round trips at its top - the poll of the predecessor's progress
  // word, then (behind a barrier) the sc1 loads of the tile: 3.6 k of a 20 k-cycle timestep (stamps: 0.5 k in step 0, which
  // has no predecessor, 4.1 k in step 1). Now thread 0 peeks at the word for cell n + 1 at the start of P4 of cell n (the
  // load returns under P4 and the store drain); if that cell is already published, every thread fetches its elements of
  // the tile right behind the publish barrier (poll -> barrier -> sc1 loads, the order of the blocking form) and the next
  // iteration starts with them in flight instead of polling. A step settles ~0.15 cell + one hand-off behind its
  // predecessor, where the peek succeeds every time; a miss just takes the blocking path.
  bool have_next = false;
  float xnext[2] = {0.0f, 0.0f};
  // conditioning part of the gates (written by the GEMM before this launch): cell 0's here, cell n + 1's behind P2 of cell n,
  // into the registers P2 has just finished with (at the top of the cell these loads sat in front of the tile's in the
  // in-order vmcnt queue: -2 % on the walk)
  float gc[4][NG];
  {
    const float* gicb = f.gic + (long)k * f.F * G;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rw = min(b0 + kq_0 * 4 + r, B - 1);
#pragma unroll
      for (int g = 0; g < NG; ++g) gc[r][g] = gicb[(long)rw * G + g * H + jc];
    }
  }
  for (int n = 0; n < f.N; ++n) {
    // lane coordinates laundered per iteration: otherwise every per-lane stash address (a dozen arrays x 4 rows, 64-bit) is
    // hoisted out of the timestep loop and the kernel spills ~150 VGPRs
    int l15 = l15_0, kq = kq_0, ri = ri_0, cl = cl_0, tcol = tcol_0;
    asm volatile("" : "+v"(l15), "+v"(kq), "+v"(ri), "+v"(cl), "+v"(tcol));

    const long fr = (long)n * B;
    const long kf = (long)k * f.F + fr;
    PIPE_STAMP(0, 0);
    if (k > 0 && !have_next && !pipe_acquire(prog + ((k - 1) * nbt + bt) * PIPE_STRIDE, (unsigned)n + 1u, abort_w, tid, &s_ok, fenced)) break;

    PIPE_STAMP(0, 1);
    // ---- P0: actnorm (glow/modules.py:45-52); stage a k-major
    {
      const float* xin = (k == 0) ? f.x0 + ((long)row * f.T + f.start + n) * C : f.sX + (kf - f.F + row) * LC;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = cl + 32 * u;
        if (c < C16) {
          float a = 0.0f;
          if (c < C && rok) a = ((k == 0 ? xin[c] : (have_next ? xnext[u] : ld_tile(xin + c, fenced))) + anb[u]) * ans[u];
          At[c * LT + ri] = a;
        }
      }
    }
    __syncthreads();
    PIPE_STAMP(0, 2);

    // ---- P1: y = a W   (InvertibleConv1x1.forward, glow/modules.py:186)
    if (t1) {
      const f32x4 acc = mma16_lds(At + kq * LT + l15, w1s, nbC);
      const int c = tcol;
      if (c < C) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = kq * 4 + r;
          const float v = acc[r];
          Yrm[i * ldy + c] = v;
          if (c < Ch) {
            Zt[c * LT + i] = v;
            if (X3) x3_put(ich, ich + MB * ldxi, i * ldxi + x3_pos(c), v);
          }
        }
      }
    }
    __syncthreads();
    PIPE_STAMP(0, 3);

    // ---- P2: recurrent cell of the coupling net (f_seq.forward, glow/models.py:204-214); state stays in LDS / registers
    if (t2) {
      float cnew[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (X3)
        fast_cell_p2_x3_img<NG>(f, ich, ich + MB * ldxi, ldxi, Ch16, Ht, Hn, wzx, whx, gc, bh, cprev, (nbZ + 1) >> 1, (nbH + 1) >> 1,
                                tcol, kq, l15, b0, B, nullptr, NG == 4 ? f.sC + kf * H : nullptr, f.sG + kf * 4 * H, cnew,
                                inh, inh + MB * ldxi);
      else
        fast_cell_p2<NG>(f, Zt, Ht, Hn, wz, wh, gc, bh, cprev, nbZ, nbH, tcol, kq, l15, b0, B, nullptr,
                         NG == 4 ? f.sC + kf * H : nullptr, f.sG + kf * 4 * H, cnew);
#pragma unroll
      for (int r = 0; r < 4; ++r) cprev[r] = cnew[r];
    }
    if (n + 1 < f.N) {
      const float* gicb = f.gic + (kf + B) * G;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rw = min(b0 + kq * 4 + r, B - 1);
#pragma unroll
        for (int g = 0; g < NG; ++g) gc[r][g] = gicb[(long)rw * G + g * H + jc];
      }
    }
    __syncthreads();
    PIPE_STAMP(0, 4);

    // ---- P3: o = (h' Wfl^T + b) exp(3 logs)   (LinearZeros, glow/modules.py:93-95)
    if (t3) {
      // (exact f32 MFMA in every mode: o sets the coupling's scale and shift directly, and the inverse pass - sampling, invert -
      // computes it in exact f32; with three bf16 products here decode(encode(x)) at 96 flow steps went from 7e-4 to 3e-3 of x
      // for 20 us of a 500 us walk)
      const f32x4 acc = mma16_lds(Hn + kq * LT + l15, w3s, nbH);
      if (tcol < Cout) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = kq * 4 + r;
          const float o = (acc[r] + flb) * fls;
          Orm[i * ldo + tcol] = o;
        }
      }
    }
    __syncthreads();
    PIPE_STAMP(0, 5);

    // ---- P4: coupling (glow/models.py:330-341), pass-through half, log-det; the output tile is the hand-off payload
    const bool peek = k > 0 && !fenced && n + 1 < f.N;
    unsigned pk = 0u;
    if (peek && tid == 0) pk = ld_agent(prog + ((k - 1) * nbt + bt) * PIPE_STRIDE);
    // the cell's stash rows a, y, h', o leave from their LDS tiles here, 16 bytes per thread and array (thread (row ri, columns
    // 4 cl .. 4 cl + 3)): one store instruction each instead of the 2 / 4 / 4 / 4 dword stores per lane that P0 .. P3 issued from the
    // MFMA accumulator layout (the walk is bound by vector-memory instruction issue; round 3: 20 % faster without its stash stores)
    if (rok) {
      const int c0 = 4 * cl;
      if (c0 < C) {   // (LC, LO are multiples of 4 floats: the last vector's tail lies in the row padding)
        f32x4 va, vy;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          va[e] = c0 + e < C ? At[(c0 + e) * LT + ri] : 0.0f;
          vy[e] = c0 + e < C ? Yrm[ri * ldy + c0 + e] : 0.0f;
        }
        *reinterpret_cast<f32x4*>(f.sA + (kf + row) * LC + c0) = va;
        *reinterpret_cast<f32x4*>(f.sY + (kf + row) * LC + c0) = vy;
      }
      if (c0 < Cout) {
        f32x4 vo;
#pragma unroll
        for (int e = 0; e < 4; ++e) vo[e] = c0 + e < Cout ? Orm[ri * ldo + c0 + e] : 0.0f;
        *reinterpret_cast<f32x4*>(f.sO + (kf + row) * LO + c0) = vo;
      }
      for (int h0 = c0; h0 < H; h0 += 128) {   // (H <= 128 on this path: one trip)
        f32x4 vh;
#pragma unroll
        for (int e = 0; e < 4; ++e) vh[e] = h0 + e < H ? Hn[(h0 + e) * LT + ri] : 0.0f;
        if (h0 + 3 < H && (H & 3) == 0) *reinterpret_cast<f32x4*>(f.sH + (kf + row) * H + h0) = vh;
        else
          for (int e = 0; e < 4; ++e)
            if (h0 + e < H) f.sH[(kf + row) * H + h0 + e] = vh[e];
      }
    }
    {
      float lg = 0.0f;
      if (cl < C2) {
        const float z2 = Yrm[ri * ldy + Ch + cl];
        float z2n;
        if (f.affine) {
          const float shift = Orm[ri * ldo + 2 * cl];
          const float sraw = sigmoidf_(Orm[ri * ldo + 2 * cl + 1] + 2.0f);
          const float sc = fmaxf(sraw, f.eps);
          z2n = (z2 + shift) * sc;
          lg = logf(sc);
        } else {
          z2n = z2 + Orm[ri * ldo + cl];
        }
        if (rok) st_sc1(f.sX + (kf + row) * LC + Ch + cl, z2n);
      }
      if (cl < Ch && rok) st_sc1(f.sX + (kf + row) * LC + cl, Yrm[ri * ldy + cl]);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) lg += __shfl_xor(lg, o, 64);  // the 32 lanes of one row
      if (cl == 0 && rok) f.sL[kf + row] = lg;
    }
    PIPE_STAMP(0, 6);
    // (pipe_publish, with the outcome of the peek riding on its barrier)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (peek && tid == 0) s_rdy = pk >= (unsigned)n + 2u ? 1 : 0;
    __syncthreads();
    if (k + 1 < f.Ks && tid == 0) st_agent(prog + (k * nbt + bt) * PIPE_STRIDE, (unsigned)n + 1u);
    have_next = peek && s_rdy != 0;
    if (have_next) {
      const float* xn = f.sX + (kf + B - f.F + row) * LC;   // cell n + 1 of step k - 1
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = cl + 32 * u;
        xnext[u] = (c < C && rok) ? ld_tile(xn + c, false) : 0.0f;
      }
    }
    PIPE_STAMP(0, 7);
    float* t = Ht; Ht = Hn; Hn = t;
    __bf16* ti = ich; ich = inh; inh = ti;
  }
}

struct CarveFB {
  int Dl, Gi, Dy, Cy, Pl, total;
};
__host__ __device__ inline CarveFB carve_fast_bwd(int C16, int H16, int Co16, int Cout, int NG) {
  CarveFB c;
  int o = 0;
  c.Dl = o; o += Co16 * LT;
  c.Gi = o; o += 2 * NG * H16 * LT;   // Gi then Gh, each [NG][H16][LT]
  c.Dy = o; o += C16 * LT;
  c.Cy = o; o += H16 * LT;
  c.Pl = o; o += MB * (Cout + 1);
  c.total = o;
  return c;
}

// acc + sum over NG gate blocks (each nb blocks of 16 k; a_lane advances by blk floats per gate)
template <int NG, int MAXB>
__device__ __forceinline__ f32x4 mma16_reg_gates(const float* a_lane, int blk, const f32x4 (&w)[NG][MAXB], int nb) {
  f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int b = 0; b < MAXB; ++b)
      if (b < nb) {
        const float* ab = a_lane + g * blk + b * 16 * LT;
        const float a0 = ab[0], a1 = ab[4 * LT], a2 = ab[8 * LT], a3 = ab[12 * LT];
        e = mfma16(a0, w[g][b][0], e);
        o = mfma16(a1, w[g][b][1], o);
        e = mfma16(a2, w[g][b][2], e);
        o = mfma16(a3, w[g][b][3], o);
      }
  return e + o;
}

template <int NG>
__global__ __launch_bounds__(NT) void flow_diag_bwd_fast_kernel(FlowK f, int d, int klo) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kq = lane >> 4;
  const int ri = tid >> 5, cl = tid & 31;
  int cell, bt;
  flow_cell_of_block(f.nbt, &cell, &bt);
  const int k = klo + cell, n = d - k;
  const int b0 = bt * MB;
  const int B = f.B, C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const long LC = f.ldc, LO = f.ldo;   // stash row strides
  const long fr = (long)n * B;
  const long kf = (long)k * f.F + fr;
  const CarveFB cv = carve_fast_bwd(C16, H16, Co16, Cout, NG);
  float* Dl = flow_smem + cv.Dl;
  float* Gi = flow_smem + cv.Gi;
  float* Gh = Gi + NG * H16 * LT;
  float* Dy = flow_smem + cv.Dy;
  float* Cy = flow_smem + cv.Cy;
  float* Pl = flow_smem + cv.Pl;
  const int ldp = Cout + 1;
  const int nbC = C16 >> 4, nbH = H16 >> 4, nbO = Co16 >> 4;
  const bool last = k == f.Ks - 1;
  const float gz = f.gscale / LN2_F;   // d loss / d z = z * gz   (prior term)
  const float dl = -f.gscale / LN2_F;  // d loss / d logdet
  const float* dxo = last ? f.sX + kf * LC : f.bDx + (kf + f.F) * LC;
  const float dxs = last ? gz : 1.0f;

  // which tiles this wave owns: hidden tile `wave` (Q1, Q2), z tile `wave` (Q2, waves < Ch16/16), channel tile `wave` (Q3)
  const bool th = wave * 16 < H, tz = wave * 16 < Ch, tc = wave * 16 < C;
  const int tcol = wave * 16 + l15;
  // ---- weights of Q1 (dlin Wfl: K = Cout) for this wave's hidden tile
  f32x4 wq1[FB_O];
  load_frag<FB_O>(wq1, f.bwfl + (long)k * Co16 * H16, H16, tcol, kq, nbO, th);
  // the z-tile waves stream W_ih[:, :Ch] first (they run dz1 before the barrier), the others W_hh
  f32x4 wq2[NG][FB_H];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (tz) load_frag<FB_H>(wq2[g], f.bwz + ((long)k * NG + g) * H16 * Ch16, Ch16, tcol, kq, nbH, true);
    else load_frag<FB_H>(wq2[g], f.bwh + ((long)k * NG + g) * H16 * H16, H16, tcol, kq, nbH, th);
  }

  // ---- every stash operand of Q1 / Q2 / Q3 (none depends on this cell's arithmetic) is requested now: issued inside
  //      their phases, each of these HBM round trips (~2 us) was exposed behind a barrier
  float sg[4][4], shp[4], sdhf[4], sc2[4], scp[4], sdcf[4], sdxo[4], sa[4];
  {
    const int j = tcol < H ? tcol : 0, cz = tcol < Ch ? tcol : 0, cc = tcol < C ? tcol : 0;
    const bool hasn = n < f.N - 1, hasp = n > 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = min(b0 + kq * 4 + r, B - 1);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(f.sG + (kf + row) * 4 * H + 4 * j);
      sg[r][0] = g4[0]; sg[r][1] = g4[1]; sg[r][2] = g4[2]; sg[r][3] = g4[3];
      shp[r] = hasp ? f.sH[(kf - B + row) * H + j] : 0.0f;
      sdhf[r] = hasn ? f.bDh[(kf + B + row) * H + j] : 0.0f;
      if (NG == 4) {
        sc2[r] = f.sC[(kf + row) * H + j];
        scp[r] = hasp ? f.sC[(kf - B + row) * H + j] : 0.0f;
        sdcf[r] = hasn ? f.bDc[(kf + B + row) * H + j] : 0.0f;
      }
      sdxo[r] = dxo[row * LC + cz] * dxs;
      sa[r] = f.sA[(kf + row) * LC + cc];
    }
  }

  // ---- Q0: coupling backward + LinearZeros scale; zero the k padding of the LDS operands
  {
    const int row = b0 + ri;
    const bool rok = row < B;
    const float* lfl = f.p.l_fl + (long)k * Cout;
    float dz2 = 0.0f, dl0 = 0.0f, dl1 = 0.0f, p0 = 0.0f, p1 = 0.0f;
    if (cl < C2) {
      if (rok) {
        const float dz2n = dxo[(long)row * LC + Ch + cl] * dxs;
        const float* O = f.sO + (kf + row) * LO;
        if (f.affine) {
          const float oe = O[2 * cl], oo = O[2 * cl + 1];
          const float sraw = sigmoidf_(oo + 2.0f);
          const float sc = fmaxf(sraw, f.eps);
          const float z2 = f.sY[(kf + row) * LC + Ch + cl];
          dz2 = dz2n * sc;
          const float dsc = dz2n * (z2 + oe) + dl / sc;
          const float dsr = sraw >= f.eps ? dsc : 0.0f;
          const float d0 = dz2;                             // d o_even (shift)
          const float d1 = dsr * sraw * (1.0f - sraw);      // d o_odd
          p0 = d0 * oe * 3.0f; p1 = d1 * oo * 3.0f;
          dl0 = d0 * expf(3.0f * lfl[2 * cl]); dl1 = d1 * expf(3.0f * lfl[2 * cl + 1]);
          f.bDlin[(kf + row) * LO + 2 * cl] = dl0; f.bDlin[(kf + row) * LO + 2 * cl + 1] = dl1;
        } else {
          const float oe = O[cl];
          dz2 = dz2n; p0 = dz2n * oe * 3.0f;
          dl0 = dz2n * expf(3.0f * lfl[cl]);
          f.bDlin[(kf + row) * LO + cl] = dl0;
        }
        f.bDy[(kf + row) * LC + Ch + cl] = dz2;
      }
      Dy[(Ch + cl) * LT + ri] = dz2;
      if (f.affine) {
        Dl[(2 * cl) * LT + ri] = dl0; Dl[(2 * cl + 1) * LT + ri] = dl1;
        Pl[ri * ldp + 2 * cl] = p0; Pl[ri * ldp + 2 * cl + 1] = p1;
      } else {
        Dl[cl * LT + ri] = dl0;
        Pl[ri * ldp + cl] = p0;
      }
    }
    for (int c = Cout + cl; c < Co16; c += 32) Dl[c * LT + ri] = 0.0f;
    for (int c = C + cl; c < C16; c += 32) Dy[c * LT + ri] = 0.0f;
    for (int j = H + cl; j < H16; j += 32) {
#pragma unroll
      for (int g = 0; g < NG; ++g) { Gi[(g * H16 + j) * LT + ri] = 0.0f; Gh[(g * H16 + j) * LT + ri] = 0.0f; }
    }
  }
  __syncthreads();
  if (tid < Cout) {
    float sum = 0.0f;
    for (int i = 0; i < MB; ++i) sum += Pl[i * ldp + tid];
    f.bPlfl[(((long)k * f.N + n) * f.nbt + bt) * Cout + tid] = sum;
  }

  // ---- Q1: d h' = dlin Wfl + dh carried from timestep n + 1; recurrent cell backward
  if (th) {
    const f32x4 acc = mma16_reg<FB_O>(Dl + kq * LT + l15, wq1, nbO);
    const int j = tcol;
    if (j < H) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        const int row = b0 + i;
        float gi_[4] = {0.f, 0.f, 0.f, 0.f}, gh_[4] = {0.f, 0.f, 0.f, 0.f}, cy = 0.0f;
        if (row < B) {
          const float dhn = acc[r] + sdhf[r];
          const float g0 = sg[r][0], g1 = sg[r][1], g2 = sg[r][2], g3 = sg[r][3];
          if (NG == 3) {
            const float rr = g0, uu = g1, nn = g2, ghn = g3;
            const float hp = shp[r];
            const float du = dhn * (hp - nn);
            const float dn = dhn * (1.0f - uu);
            cy = dhn * uu;
            const float dan = dn * (1.0f - nn * nn);
            const float dau = du * uu * (1.0f - uu);
            const float dar = dan * ghn * rr * (1.0f - rr);
            gi_[0] = dar; gi_[1] = dau; gi_[2] = dan;
            gh_[0] = dar; gh_[1] = dau; gh_[2] = dan * rr;
          } else {
            const float ii = g0, ff = g1, gg = g2, oo = g3;
            const float tcv = tanhf_(sc2[r]);
            const float cp = scp[r];
            const float dcf = sdcf[r];
            const float dc2 = dhn * oo * (1.0f - tcv * tcv) + dcf;
            gi_[0] = dc2 * gg * ii * (1.0f - ii);
            gi_[1] = dc2 * cp * ff * (1.0f - ff);
            gi_[2] = dc2 * ii * (1.0f - gg * gg);
            gi_[NG - 1] = dhn * tcv * oo * (1.0f - oo);
#pragma unroll
            for (int g = 0; g < NG; ++g) gh_[g] = gi_[g];
            f.bDc[(kf + row) * H + j] = dc2 * ff;
          }
          float* go = f.bDgi + (kf + row) * G + j;
          float* ho = f.bDgh + (kf + row) * G + j;
#pragma unroll
          for (int g = 0; g < NG; ++g) { go[g * H] = gi_[g]; ho[g * H] = gh_[g]; }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) { Gi[(g * H16 + j) * LT + i] = gi_[g]; Gh[(g * H16 + j) * LT + i] = gh_[g]; }
        Cy[j * LT + i] = cy;
      }
    }
  }
  // weights of Q3 (dy W^T) for this wave's channel tile: in flight under Q2
  f32x4 wq3[FB_C];
  load_frag<FB_C>(wq3, f.pWt + (long)k * C16 * C16, C16, tcol, kq, nbC, tc);
  __syncthreads();

  // ---- Q2: d z1 = dgi W_ih[:, :Ch] + pass-through (z-tile waves, before the barrier: Q3 needs it);
  //          d h_prev = dgh W_hh + carry (to timestep n - 1; not needed inside this cell)
  auto dh_prev_tile = [&](const f32x4 (&w)[NG][FB_H]) {
    if (n > 0 && th) {
      const f32x4 acc = mma16_reg_gates<NG, FB_H>(Gh + kq * LT + l15, H16 * LT, w, nbH);
      const int j = tcol;
      if (j < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = kq * 4 + r;
          const int row = b0 + i;
          if (row < B) f.bDh[(kf + row) * H + j] = acc[r] + Cy[j * LT + i];
        }
      }
    }
  };
  if (tz) {
    const f32x4 acc = mma16_reg_gates<NG, FB_H>(Gi + kq * LT + l15, H16 * LT, wq2, nbH);
    const int c = tcol;
    if (c < Ch) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        const int row = b0 + i;
        float v = 0.0f;
        if (row < B) {
          v = acc[r] + sdxo[r];
          f.bDy[(kf + row) * LC + c] = v;
        }
        Dy[c * LT + i] = v;
      }
    }
    // now fetch this wave's W_hh slice for its d h_prev tile (runs after Q3)
#pragma unroll
    for (int g = 0; g < NG; ++g) load_frag<FB_H>(wq2[g], f.bwh + ((long)k * NG + g) * H16 * H16, H16, tcol, kq, nbH, n > 0 && th);
  } else {
    dh_prev_tile(wq2);
  }
  __syncthreads();

  // ---- Q3: d a = dy W^T ; actnorm backward ; d x_in to flow step k - 1
  if (tc) {
    const f32x4 acc = mma16_reg<FB_C>(Dy + kq * LT + l15, wq3, nbC);
    const int c = tcol;
    float sl = 0.0f, sb = 0.0f;
    if (c < C) {
      const float es = expf(f.p.an_logs[(long)k * C + c]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + kq * 4 + r;
        if (row < B) {
          const float da = acc[r];
          sl += da * sa[r];
          sb += da * es;
          if (k > 0) f.bDx[(kf + row) * LC + c] = da * es;
        }
      }
    }
    sl += __shfl_xor(sl, 16, 64); sl += __shfl_xor(sl, 32, 64);
    sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
    if (kq == 0 && c < C) {
      float* pan = f.bPan + (((long)k * f.N + n) * f.nbt + bt) * 2 * C;
      pan[c] = sl; pan[C + c] = sb;
    }
  }
  if (tz) dh_prev_tile(wq2);
}

// Backward twin of flow_pipe_fwd_kernel: workgroup (k, bt) keeps flow step k's backward weights, walks n = N-1 .. 0, carries
// d h (and the LSTM's d c) from timestep n + 1 in registers and receives d x of flow step k + 1 through the same write-through
// hand-off (bDx tile + progress counter). The z-tile waves need two weight slices (W_ih[:, :Ch] and W_hh): the second one is
// re-read from L2 every timestep, requested before the wait.
template <int NG, bool X3>
__global__ __launch_bounds__(NT) void flow_pipe_bwd_kernel(FlowK f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15_0 = lane & 15, kq_0 = lane >> 4;
  const int ri_0 = tid >> 5, cl_0 = tid & 31;
  __shared__ int s_id, s_ok, s_rdy;
  if (tid == 0) s_id = (int)atomicAdd(f.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int kk = s_id / nbt, bt = s_id - kk * nbt;
  if (kk >= f.Ks) return;
  const int k = f.Ks - 1 - kk;   // tickets in arrival order: (k + 1, bt) always started before (k, bt)
  unsigned* abort_w = f.pipe + 1;
  unsigned* prog = f.pipe + PIPE_WALK_HDR;
  const bool fenced = f.pipe_fence != 0;
  const int b0 = bt * MB;
  const int B = f.B, C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const long LC = f.ldc, LO = f.ldo;   // stash row strides
  const CarveFB cv = carve_fast_bwd(C16, H16, Co16, Cout, NG);
  float* Dl = flow_smem + cv.Dl;
  float* Gi = flow_smem + cv.Gi;
  float* Gh = Gi + NG * H16 * LT;
  // bf16 x 3: the Gi / Gh regions hold bf16 hi + lo images instead ([16][ldx], see x3_put); 64 (NG H16 + 8) <= 68 NG H16 bytes
  const int ldx = NG * H16 + 8;
  __bf16* GiH = reinterpret_cast<__bf16*>(Gi);
  __bf16* GiL = GiH + MB * ldx;
  __bf16* GhH = reinterpret_cast<__bf16*>(Gh);
  __bf16* GhL = GhH + MB * ldx;
  float* Dy = flow_smem + cv.Dy;
  float* Cy = flow_smem + cv.Cy;
  float* Pl = flow_smem + cv.Pl;
  const int ldp = Cout + 1;
  const int nbC = C16 >> 4, nbH = H16 >> 4, nbO = Co16 >> 4;
  const bool last = k == f.Ks - 1;
  const float gz = f.gscale / LN2_F;   // d loss / d z = z * gz   (prior term)
  const float dl = -f.gscale / LN2_F;  // d loss / d logdet
  const float dxs = last ? gz : 1.0f;

  // which tiles this wave owns: hidden tile `wave` (Q1, Q2), z tile `wave` (Q2, waves < Ch16/16), channel tile `wave` (Q3)
  const bool th = wave * 16 < H, tz = wave * 16 < Ch, tc = wave * 16 < C;
  const int tcol_0 = wave * 16 + l15_0;
  // ---- weights of Q1 (dlin Wfl: K = Cout) for this wave's hidden tile
  f32x4 wq1[FB_O];
  {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < FB_O; ++b) wq1[b] = zero4;
  }
  load_frag<FB_O>(wq1, f.bwfl + (long)k * Co16 * H16, H16, tcol_0, kq_0, nbO, th);
  // bf16 x 3: Q1's product too (dlin Wfl, K = Cout): the fragments packed into 32-k blocks, the A operand d lin as a bf16
  // hi / lo image [16][ldxd] that Q0 writes (x3_put, slot order x3_pos) behind the regions of the exact path
  X3Frag wq1x[FB_O / 2];
  const int nbO2 = (nbO + 1) >> 1, ldxd = 32 * nbO2 + 8;
  __bf16* DlH = reinterpret_cast<__bf16*>(flow_smem + ((cv.total + 3) & ~3));
  __bf16* DlL = DlH + MB * ldxd;
  if constexpr (X3) {
#pragma unroll
    for (int b2 = 0; b2 < FB_O / 2; ++b2) wq1x[b2] = x3_pack(wq1[2 * b2], wq1[2 * b2 + 1]);
    for (int q = tid; q < 2 * MB * ldxd; q += NT) DlH[q] = (__bf16)0.0f;
  }
  // W_hh slice of this wave's hidden tile: resident, except in the z-tile waves, which need two slices (W_ih[:, :Ch] for
  // d z1, then W_hh) and stream both through the same registers every timestep, as the per-diagonal kernel does
  f32x4 wq2[X3 ? 1 : NG][X3 ? 1 : FB_H];      // exact f32 form
  X3Frag wq2x[X3 ? NG : 1][FB_H / 2];         // bf16 x 3 form: pre-split 32-k fragments (flow_prep_x3_kernel)
  const int nB = H16 >> 5, nbH2 = (nbH + 1) >> 1;
  const long perH = (long)NG * nB * H16 * 4, perZ = (long)NG * nB * Ch16 * 4;   // uint4 entries per plane and flow step
  const uint4* xh = f.xbwh + (long)k * 2 * perH;
  const uint4* xz = f.xbwz + (long)k * 2 * perZ;
  if (!tz) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if constexpr (X3) x3_load<FB_H / 2>(wq2x[g], xh, perH, g, nB, H16, tcol_0, kq_0, nbH2, th);
      else load_frag<FB_H>(wq2[g], f.bwh + ((long)k * NG + g) * H16 * H16, H16, tcol_0, kq_0, nbH, th);
    }
  }
  // weights of Q3 (dy W^T) for this wave's channel tile
  f32x4 wq3[FB_C];
  load_frag<FB_C>(wq3, f.pWt + (long)k * C16 * C16, C16, tcol_0, kq_0, nbC, tc);
  const float es_an = tcol_0 < C ? expf(f.p.an_logs[(long)k * C + tcol_0]) : 0.0f;
  float dhc[4] = {0.f, 0.f, 0.f, 0.f}, dcc[4] = {0.f, 0.f, 0.f, 0.f};   // d h / d c carried from timestep n + 1 (registers)

  if constexpr (X3) {   // padding columns (hidden units >= H) are never written: zero the images once
    for (int q = tid; q < 2 * MB * ldx; q += NT) { GiH[q] = (__bf16)0.0f; GhH[q] = (__bf16)0.0f; }
    __syncthreads();
  }
  // b_ih / b_hh gradients = column sums of dgi / dgh over all frames: every thread of the Q1 tile sums its own hidden unit
  // over its 4 rows and all timesteps here (fixed order), instead of two 350 MB passes over the stash afterwards
  float bsi[NG], bsh[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) { bsi[g] = 0.0f; bsh[g] = 0.0f; }
  // look-ahead acquire, as in the forward walk: thread 0 peeks at flow step k + 1's progress word for cell n - 1 at the start
  // of Q3 of cell n; if it is published, every thread fetches its elements of that d x tile behind the publish barrier
  bool have_next = false;
  float nx_dxo[4] = {0.f, 0.f, 0.f, 0.f}, nx_dz2 = 0.0f;
  for (int n = f.N - 1; n >= 0; --n) {
    // lane coordinates laundered per iteration: otherwise every per-lane stash address (a dozen arrays x 4 rows, 64-bit) is
    // hoisted out of the timestep loop and the kernel spills ~150 VGPRs
    int l15 = l15_0, kq = kq_0, ri = ri_0, cl = cl_0, tcol = tcol_0;
    asm volatile("" : "+v"(l15), "+v"(kq), "+v"(ri), "+v"(cl), "+v"(tcol));

  const long fr = (long)n * B;
  const long kf = (long)k * f.F + fr;
  const float* dxo = last ? f.sX + kf * LC : f.bDx + (kf + f.F) * LC;
  PIPE_STAMP(1, 0);
  // ---- forward-stash operands of Q1 / Q2 / Q3 (written before this launch): in flight under the wait for flow step k + 1
  float sg[4][4], shp[4], sdhf[4], sc2[4], scp[4], sdcf[4], sdxo[4], sa[4];
  {
    const int j = tcol < H ? tcol : 0, cc = tcol < C ? tcol : 0;
    const bool hasp = n > 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = min(b0 + kq * 4 + r, B - 1);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(f.sG + (kf + row) * 4 * H + 4 * j);
      sg[r][0] = g4[0]; sg[r][1] = g4[1]; sg[r][2] = g4[2]; sg[r][3] = g4[3];
      shp[r] = hasp ? f.sH[(kf - B + row) * H + j] : 0.0f;
      sdhf[r] = dhc[r];
      if (NG == 4) {
        sc2[r] = f.sC[(kf + row) * H + j];
        scp[r] = hasp ? f.sC[(kf - B + row) * H + j] : 0.0f;
        sdcf[r] = dcc[r];
      }
      sa[r] = f.sA[(kf + row) * LC + cc];
    }
  }
  if (tz) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if constexpr (X3) x3_load<FB_H / 2>(wq2x[g], xz, perZ, g, nB, Ch16, tcol, kq, nbH2, true);
      else load_frag<FB_H>(wq2[g], f.bwz + ((long)k * NG + g) * H16 * Ch16, Ch16, tcol, kq, nbH, true);
    }
  }
  // Q0's forward-stash operands (o of the coupling net, z2) for this thread's element
  float q_oe = 0.0f, q_oo = 0.0f, q_z2 = 0.0f;
  if (cl < C2 && b0 + ri < B) {
    const float* O = f.sO + (kf + b0 + ri) * LO;
    if (f.affine) {
      q_oe = O[2 * cl]; q_oo = O[2 * cl + 1];
      q_z2 = f.sY[(kf + b0 + ri) * LC + Ch + cl];
    } else {
      q_oe = O[cl];
    }
  }
  if (!last && !have_next && !pipe_acquire(prog + ((k + 1) * nbt + bt) * PIPE_STRIDE, (unsigned)(f.N - n), abort_w, tid, &s_ok, fenced)) break;
  {
    const int cz = tcol < Ch ? tcol : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = min(b0 + kq * 4 + r, B - 1);
      sdxo[r] = (last ? dxo[row * LC + cz] : (have_next ? nx_dxo[r] : ld_tile(dxo + row * LC + cz, fenced))) * dxs;
    }
  }

  PIPE_STAMP(1, 1);
  // ---- Q0: coupling backward + LinearZeros scale; zero the k padding of the LDS operands
  {
    const int row = b0 + ri;
    const bool rok = row < B;
    const float* lfl = f.p.l_fl + (long)k * Cout;
    float dz2 = 0.0f, dl0 = 0.0f, dl1 = 0.0f, p0 = 0.0f, p1 = 0.0f;
    if (cl < C2) {
      if (rok) {
        const float dz2n = (last ? dxo[(long)row * LC + Ch + cl]
                                 : (have_next ? nx_dz2 : ld_tile(dxo + (long)row * LC + Ch + cl, fenced))) * dxs;
        if (f.affine) {
          const float oe = q_oe, oo = q_oo;
          const float sraw = sigmoidf_(oo + 2.0f);
          const float sc = fmaxf(sraw, f.eps);
          const float z2 = q_z2;
          dz2 = dz2n * sc;
          const float dsc = dz2n * (z2 + oe) + dl / sc;
          const float dsr = sraw >= f.eps ? dsc : 0.0f;
          const float d0 = dz2;                             // d o_even (shift)
          const float d1 = dsr * sraw * (1.0f - sraw);      // d o_odd
          p0 = d0 * oe * 3.0f; p1 = d1 * oo * 3.0f;
          dl0 = d0 * expf(3.0f * lfl[2 * cl]); dl1 = d1 * expf(3.0f * lfl[2 * cl + 1]);
          f.bDlin[(kf + row) * LO + 2 * cl] = dl0; f.bDlin[(kf + row) * LO + 2 * cl + 1] = dl1;
        } else {
          const float oe = q_oe;
          dz2 = dz2n; p0 = dz2n * oe * 3.0f;
          dl0 = dz2n * expf(3.0f * lfl[cl]);
          f.bDlin[(kf + row) * LO + cl] = dl0;
        }
        f.bDy[(kf + row) * LC + Ch + cl] = dz2;
      }
      Dy[(Ch + cl) * LT + ri] = dz2;
      if (f.affine) {
        if constexpr (X3) {
          x3_put(DlH, DlL, ri * ldxd + x3_pos(2 * cl), dl0);
          x3_put(DlH, DlL, ri * ldxd + x3_pos(2 * cl + 1), dl1);
        } else {
          Dl[(2 * cl) * LT + ri] = dl0; Dl[(2 * cl + 1) * LT + ri] = dl1;
        }
        Pl[ri * ldp + 2 * cl] = p0; Pl[ri * ldp + 2 * cl + 1] = p1;
      } else {
        if constexpr (X3) x3_put(DlH, DlL, ri * ldxd + x3_pos(cl), dl0);
        else Dl[cl * LT + ri] = dl0;
        Pl[ri * ldp + cl] = p0;
      }
    }
    if (!X3) for (int c = Cout + cl; c < Co16; c += 32) Dl[c * LT + ri] = 0.0f;
    for (int c = C + cl; c < C16; c += 32) Dy[c * LT + ri] = 0.0f;
    for (int j = H + cl; j < H16; j += 32) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (!X3) { Gi[(g * H16 + j) * LT + ri] = 0.0f; Gh[(g * H16 + j) * LT + ri] = 0.0f; }
    }
  }
  __syncthreads();
  PIPE_STAMP(1, 2);
  if (tid < Cout) {
    float sum = 0.0f;
    for (int i = 0; i < MB; ++i) sum += Pl[i * ldp + tid];
    f.bPlfl[(((long)k * f.N + n) * f.nbt + bt) * Cout + tid] = sum;
  }

  // ---- Q1: d h' = dlin Wfl + dh carried from timestep n + 1; recurrent cell backward
  if (th) {
    f32x4 acc;
    if constexpr (X3) {
      const __bf16* rh = DlH + l15 * ldxd + 8 * kq;
      const __bf16* rl = DlL + l15 * ldxd + 8 * kq;
      f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int b2 = 0; b2 < FB_O / 2; ++b2)
        if (b2 < nbO2) {
          X3Frag av;
          av.hi = *reinterpret_cast<const fbf16x8*>(rh + b2 * 32);
          av.lo = *reinterpret_cast<const fbf16x8*>(rl + b2 * 32);
          if (b2 & 1) o = x3_mma(av, wq1x[b2], o);
          else e = x3_mma(av, wq1x[b2], e);
        }
      acc = e + o;
    } else {
      acc = mma16_reg<FB_O>(Dl + kq * LT + l15, wq1, nbO);
    }
    const int j = tcol;
    if (j < H) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        const int row = b0 + i;
        float gi_[4] = {0.f, 0.f, 0.f, 0.f}, gh_[4] = {0.f, 0.f, 0.f, 0.f}, cy = 0.0f;
        if (row < B) {
          const float dhn = acc[r] + sdhf[r];
          const float g0 = sg[r][0], g1 = sg[r][1], g2 = sg[r][2], g3 = sg[r][3];
          if (NG == 3) {
            const float rr = g0, uu = g1, nn = g2, ghn = g3;
            const float hp = shp[r];
            const float du = dhn * (hp - nn);
            const float dn = dhn * (1.0f - uu);
            cy = dhn * uu;
            const float dan = dn * (1.0f - nn * nn);
            const float dau = du * uu * (1.0f - uu);
            const float dar = dan * ghn * rr * (1.0f - rr);
            gi_[0] = dar; gi_[1] = dau; gi_[2] = dan;
            gh_[0] = dar; gh_[1] = dau; gh_[2] = dan * rr;
          } else {
            const float ii = g0, ff = g1, gg = g2, oo = g3;
            const float tcv = tanhf_(sc2[r]);
            const float cp = scp[r];
            const float dcf = sdcf[r];
            const float dc2 = dhn * oo * (1.0f - tcv * tcv) + dcf;
            gi_[0] = dc2 * gg * ii * (1.0f - ii);
            gi_[1] = dc2 * cp * ff * (1.0f - ff);
            gi_[2] = dc2 * ii * (1.0f - gg * gg);
            gi_[NG - 1] = dhn * tcv * oo * (1.0f - oo);
#pragma unroll
            for (int g = 0; g < NG; ++g) gh_[g] = gi_[g];
            dcc[r] = dc2 * ff;
          }
          float* go = f.bDgi + (kf + row) * G + j;
          float* ho = f.bDgh + (kf + row) * G + j;
#pragma unroll
          // (GRU: d r, d z on the hidden side equal the input side's. Storing only the n block of dgh and taking the other two
          // rows of the W_hh gradient from dgi was measured in round 4: 8 of 24 dword stores per lane and cell less, but the
          // gradient then needs two products over the frames instead of one - whole step 7.73 / 7.69 ms against 7.67 / 7.64: removed)
          for (int g = 0; g < NG; ++g) {
            if (X3 && f.g16) {   // (rounded as the products' operand split rounds its hi part: to nearest even)
              reinterpret_cast<__bf16*>(f.bDgi)[(kf + row) * G + j + g * H] = (__bf16)gi_[g];
              reinterpret_cast<__bf16*>(f.bDgh)[(kf + row) * G + j + g * H] = (__bf16)gh_[g];
            } else {
              go[g * H] = gi_[g]; ho[g * H] = gh_[g];
            }
            bsi[g] += gi_[g]; bsh[g] += gh_[g];
          }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if constexpr (X3) {
            const int at = i * ldx + g * H16 + j;   // natural column order (weights: flow_prep_x3_kernel)
            x3_put(GiH, GiL, at, gi_[g]);
            x3_put(GhH, GhL, at, gh_[g]);
          } else {
            Gi[(g * H16 + j) * LT + i] = gi_[g]; Gh[(g * H16 + j) * LT + i] = gh_[g];
          }
        }
        Cy[j * LT + i] = cy;
      }
    }
  }
  __syncthreads();
  PIPE_STAMP(1, 3);

  // ---- Q2: d z1 = dgi W_ih[:, :Ch] + pass-through (z-tile waves, before the barrier: Q3 needs it);
  //          d h_prev = dgh W_hh + carry (to timestep n - 1; not needed inside this cell)
  auto dh_prev_tile = [&]() {
    if (n > 0 && th) {
      f32x4 acc;
      if constexpr (X3) acc = x3_mma_gates_img<NG, FB_H / 2>(GhH + l15 * ldx + 8 * kq, GhL + l15 * ldx + 8 * kq, H16, wq2x, nbH2);
      else acc = mma16_reg_gates<NG, FB_H>(Gh + kq * LT + l15, H16 * LT, wq2, nbH);
      const int j = tcol;
      if (j < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = kq * 4 + r;
          const int row = b0 + i;
          (void)row;
          dhc[r] = acc[r] + Cy[j * LT + i];
        }
      }
    }
  };
  if (tz) {
    f32x4 acc;
    if constexpr (X3) acc = x3_mma_gates_img<NG, FB_H / 2>(GiH + l15 * ldx + 8 * kq, GiL + l15 * ldx + 8 * kq, H16, wq2x, nbH2);
    else acc = mma16_reg_gates<NG, FB_H>(Gi + kq * LT + l15, H16 * LT, wq2, nbH);
    const int c = tcol;
    if (c < Ch) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        const int row = b0 + i;
        float v = 0.0f;
        if (row < B) {
          v = acc[r] + sdxo[r];
          f.bDy[(kf + row) * LC + c] = v;
        }
        Dy[c * LT + i] = v;
      }
    }
    // now fetch this wave's W_hh slice for its d h_prev tile (runs after Q3)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if constexpr (X3) x3_load<FB_H / 2>(wq2x[g], xh, perH, g, nB, H16, tcol, kq, nbH2, n > 0 && th);
      else load_frag<FB_H>(wq2[g], f.bwh + ((long)k * NG + g) * H16 * H16, H16, tcol, kq, nbH, n > 0 && th);
    }
  } else {
    dh_prev_tile();
  }
  __syncthreads();
  PIPE_STAMP(1, 4);

  // ---- Q3: d a = dy W^T ; actnorm backward ; d x_in to flow step k - 1
  const bool peek = !last && !fenced && n > 0;
  unsigned pk = 0u;
  if (peek && tid == 0) pk = ld_agent(prog + ((k + 1) * nbt + bt) * PIPE_STRIDE);
  if constexpr (X3) {
    // dgi of this cell as operand planes (include/lfi.h) for the two products that consume it - dpre = dgi W_c sums over gate
    // columns, dW_c = dgi^T c over frames: one set of planes serves both - straight from the bf16 hi / lo LDS images Q1 left: one
    // 16-byte LDS read and one 16-byte store per 8 values and plane, by the waves that own no channel tile and idle through Q3
    if (f.bDgiR && !tc) {
      const int ntc = (C + 15) >> 4;                 // channel-tile waves are waves 0 .. ntc - 1
      const int ne = NT - ntc * 64, et = tid - ntc * 64;
      const long gr0 = kf + b0;                      // row of the (Ks F x G) matrix: flow step k, frame n B + b0 (+ i)
      const int nktG = G >> 4;
      char* rbase = reinterpret_cast<char*>(f.bDgiR) + ((gr0 >> 5) * nktG * 2) * 1024;
      const int r0 = (int)(gr0 & 16);                // this tile's 16 rows inside the 32-row plane tile
      // u = 32 ct + 2 i + hp: the chunk that lies hp-th in row r0 + i of block (row tile, ct): consecutive threads write consecutive
      // 16 bytes, 32 threads the 512 contiguous bytes this tile owns of a block (a row's two chunks in one store instruction:
      // the per-half mapping left every store at a 32-byte stride and the backward walk 0.11 ms longer)
      for (int u = et; u < 2 * G; u += ne) {
        const int hp = u & 1, i = (u >> 1) & 15, ct = u >> 5;
        const int h = hp ^ (((r0 + i) >> 3) & 1);    // which 8 columns lie there (lfi_u_plane_offset)
        const int so = i * ldx + ct * 16 + h * 8;
        char* dst = rbase + (long)ct * 2048 + (r0 + i) * 32 + hp * 16;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(GiH + so);
        if (!f.dgi_hi_only) *reinterpret_cast<uint4*>(dst + 1024) = *reinterpret_cast<const uint4*>(GiL + so);
      }
    }
  }
  if (tc) {
    const f32x4 acc = mma16_reg<FB_C>(Dy + kq * LT + l15, wq3, nbC);
    const int c = tcol;
    float sl = 0.0f, sb = 0.0f;
    if (c < C) {
      const float es = es_an;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + kq * 4 + r;
        if (row < B) {
          const float da = acc[r];
          sl += da * sa[r];
          sb += da * es;
          if (k > 0) st_sc1(f.bDx + (kf + row) * LC + c, da * es);
        }
      }
    }
    sl += __shfl_xor(sl, 16, 64); sl += __shfl_xor(sl, 32, 64);
    sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
    if (kq == 0 && c < C) {
      float* pan = f.bPan + (((long)k * f.N + n) * f.nbt + bt) * 2 * C;
      pan[c] = sl; pan[C + c] = sb;
    }
  }
  PIPE_STAMP(1, 5);
  // (pipe_publish, with the outcome of the peek riding on its barrier)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (peek && tid == 0) s_rdy = pk >= (unsigned)(f.N - n) + 1u ? 1 : 0;
  __syncthreads();
  if (k > 0 && tid == 0) st_agent(prog + (k * nbt + bt) * PIPE_STRIDE, (unsigned)(f.N - n));
  have_next = peek && s_rdy != 0;
  if (have_next) {
    const float* dxn = f.bDx + (kf - B + f.F) * LC;   // cell n - 1 of flow step k + 1
    const int cz = tcol < Ch ? tcol : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) nx_dxo[r] = ld_tile(dxn + (long)min(b0 + kq * 4 + r, B - 1) * LC + cz, false);
    nx_dz2 = (cl < C2 && b0 + ri < B) ? ld_tile(dxn + (long)(b0 + ri) * LC + Ch + cl, false) : 0.0f;
  }
  PIPE_STAMP(1, 6);
  // the z-tile waves' own d h_prev tile is only needed by the next timestep of THIS workgroup: after the hand-off, off the
  // pipeline's latency path (it reads Gh / Cy, which the next timestep rewrites only behind its first barrier)
  if (tz) dh_prev_tile();
  PIPE_STAMP(1, 7);
  }  // timestep loop
  if (th) {   // (an abandoned walk leaves these incomplete: flow_pipe_poison_kernel overwrites them with NaN)
    float* pb = f.bPbias + ((long)k * nbt + bt) * 2 * G;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float vi = bsi[g], vh = bsh[g];
      vi += __shfl_xor(vi, 16, 64); vi += __shfl_xor(vi, 32, 64);
      vh += __shfl_xor(vh, 16, 64); vh += __shfl_xor(vh, 32, 64);
      if ((lane >> 4) == 0 && tcol_0 < H) { pb[g * H + tcol_0] = vi; pb[G + g * H + tcol_0] = vh; }
    }
  }
}

// A backward walk that gave up must not pass for a result: NaN into one frame of every flow step's stashed gradients, which
// every parameter gradient (and, through dgi, the encoder gradients) sums over.
__global__ __launch_bounds__(64) void flow_pipe_poison_kernel(FlowK f) {
  if (f.pipe[1] == 0u) return;
  const float nan = __builtin_nanf("");
  for (long i = threadIdx.x; i < (long)f.Ks * 2 * f.G; i += 64) f.bPbias[(i / (2 * f.G)) * f.nbt * 2 * f.G + i % (2 * f.G)] = nan;
  for (int k = threadIdx.x; k < f.Ks; k += 64) {
    for (long fr = 0; fr < f.F; fr += (f.F > 1 ? f.F - 1 : 1)) {   // first and last frame (the W_hh gradient skips timestep 0)
      f.bDlin[((long)k * f.F + fr) * f.ldo] = nan;
      if (f.g16) {   // the dgi | dgh rows are bf16 arrays of the same shapes (an fp32 store here landed on two bf16
                     // elements of another flow step's frame, or past the bf16 region)
        reinterpret_cast<__bf16*>(f.bDgi)[((long)k * f.F + fr) * f.G] = (__bf16)nan;
        reinterpret_cast<__bf16*>(f.bDgh)[((long)k * f.F + fr) * f.G] = (__bf16)nan;
      } else {
        f.bDgi[((long)k * f.F + fr) * f.G] = nan;
        f.bDgh[((long)k * f.F + fr) * f.G] = nan;
      }
      f.bDy[((long)k * f.F + fr) * f.ldc] = nan;
    }
    // dgi as operand planes (the dgi^T c and dpre products read these, not the rows): element (row k F, column 0) of the hi plane
    if (f.bDgiR && f.F % 32 == 0) f.bDgiR[(((long)k * f.F / 32) * (f.G / 16) * 2) * 512] = (__bf16)nan;
  }
}

// Zero-padded fragment-order weight images for the register-resident cells (layout: flow_img_index).
// which: 0 pW (k = input channel, col = output channel of W), 1 pWt, 2 pwz (k = z channel, col = g*H16 + hidden),
// 3 pwh (k = hidden in), 4 pwfl (k = hidden, col = output), 5 bwfl (k = output, col = hidden),
// 6 bwh [g] (k = hidden of gate g, col = hidden), 7 bwz [g] (k = hidden of gate g, col = z channel)
__global__ __launch_bounds__(256) void flow_prep_pad_kernel(FlowK f, float* pW, float* pWt, float* pwz, float* pwh, float* pwfl,
                                                            float* bwfl, float* bwh, float* bwz, float* pWinv) {
  const int k = blockIdx.y, which = blockIdx.z;
  const int C = f.C, H = f.H, Ch = f.Ch, Cout = f.Cout, I = f.I, NG = f.NG;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const float* W = f.W + (long)k * C * C;
  const float* wih = f.p.w_ih + (long)k * f.G * I;
  const float* whh = f.p.w_hh + (long)k * f.G * H;
  const float* wfl = f.p.w_fl + (long)k * Cout * H;
  int K, J, nimg = 1;   // rows (padded), columns (padded), images per flow step
  float* dst;
  switch (which) {
    case 0: K = C16; J = C16; dst = pW; break;
    case 1: K = C16; J = C16; dst = pWt; break;
    case 2: K = Ch16; J = NG * H16; dst = pwz; break;
    case 3: K = H16; J = NG * H16; dst = pwh; break;
    case 4: K = H16; J = Co16; dst = pwfl; break;
    case 5: K = Co16; J = H16; dst = bwfl; break;
    case 6: K = H16; J = H16; nimg = NG; dst = bwh; break;
    case 7: K = H16; J = Ch16; nimg = NG; dst = bwz; break;
    default: K = C16; J = C16; dst = pWinv; break;   // 8: reverse weight (only when lfi_flow_prep built it)
  }
  if (which == 8 && !pWinv) return;
  const long per = (long)K * J;
  dst += (long)k * nimg * per;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < nimg * per; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx / per);
    const long q = idx - g * per;
    const int kk = (int)(q / J), col = (int)(q - (long)kk * J);
    float v = 0.0f;
    switch (which) {
      case 0: if (kk < C && col < C) v = W[kk * C + col]; break;
      case 1: if (kk < C && col < C) v = W[col * C + kk]; break;
      case 2: { const int gg = col / H16, j = col - gg * H16; if (kk < Ch && j < H) v = wih[((long)gg * H + j) * I + kk]; } break;
      case 3: { const int gg = col / H16, j = col - gg * H16; if (kk < H && j < H) v = whh[((long)gg * H + j) * H + kk]; } break;
      case 4: if (kk < H && col < Cout) v = wfl[(long)col * H + kk]; break;
      case 5: if (kk < Cout && col < H) v = wfl[(long)kk * H + col]; break;
      case 6: if (kk < H && col < H) v = whh[((long)g * H + kk) * H + col]; break;
      case 7: if (kk < H && col < Ch) v = wih[((long)g * H + kk) * I + col]; break;
      default: if (kk < C && col < C) v = f.Winv[(long)k * C * C + kk * C + col]; break;
    }
    dst[g * per + flow_img_index(kk, col, J)] = v;
  }
}

// bf16 hi / lo fragment images of the backward recurrent weights for the bf16 x 3 walk. which 0: bwh (k = hidden of gate g,
// col = hidden: W_hh[g*H + k][col]); 1: bwz (col = z channel: W_ih[g*H + k][col]). Entry (g, B, col, kq) holds the eight k of
// k = 32 B + 8 kq + i, the natural operand order of v_mfma_f32_16x16x32_bf16: the backward walk's d(gate) LDS images are then
// plain row-major [16 rows][gate columns] and double as the source of the dgi operand planes it emits (lfi_flow_seq_bwd_planes).
__global__ __launch_bounds__(256) void flow_prep_x3_kernel(FlowK f, uint4* xbwh, uint4* xbwz) {
  const int k = blockIdx.y, which = blockIdx.z;
  const int H = f.H, Ch = f.Ch, I = f.I, NG = f.NG, H16 = f.H16;
  const int J = which ? f.Ch16 : H16, nB = H16 >> 5;
  const float* whh = f.p.w_hh + (long)k * f.G * H;
  const float* wih = f.p.w_ih + (long)k * f.G * I;
  const long per = (long)NG * nB * J * 4;              // uint4 entries per flow step and plane
  uint4* hi = (which ? xbwz : xbwh) + (long)k * 2 * per;
  uint4* lo = hi + per;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < per; idx += (long)gridDim.x * 256) {
    const int kq = (int)(idx & 3);
    long r = idx >> 2;
    const int col = (int)(r % J); r /= J;
    const int B = (int)(r % nB), g = (int)(r / nB);
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = 32 * B + 8 * kq + i;
      float x = 0.0f;
      if (kk < H) {
        if (which == 0) { if (col < H) x = whh[((long)g * H + kk) * H + col]; }
        else if (col < Ch) x = wih[((long)g * H + kk) * I + col];
      }
      v[i] = x;
    }
    uint4 h, l;
    x3_split2(v[0], v[1], &h.x, &l.x);
    x3_split2(v[2], v[3], &h.y, &l.y);
    x3_split2(v[4], v[5], &h.z, &l.z);
    x3_split2(v[6], v[7], &h.w, &l.w);
    hi[idx] = h;
    lo[idx] = l;
  }
}

// fp16 hi / lo fragment images of the reverse cell's weights (three fp16 products, x3h_*): image `which` 0: pwz (K = Ch16,
// J = NG H16), 1: pwh (H16, NG H16), 2: pwfl (H16, Co16), 3: pWinv (C16, C16) of flow step blockIdx.y. Entry (b, kq, col) is
// x3h_pack of the padded f32 image's entries (2b, kq, col) and (2b + 1, kq, col) - exactly what rev_fast_cell made of them in
// registers in every workgroup of every generated frame (672 conversions per lane in front of a cell's first product).
__global__ __launch_bounds__(256) void flow_prep_x3h_kernel(FlowK f, uint4* hwz, uint4* hwh, uint4* hwfl, uint4* hWinv) {
  const int k = blockIdx.y, which = blockIdx.z;
  const int K16 = which == 0 ? f.Ch16 : (which == 3 ? f.C16 : f.H16);
  const int J = which < 2 ? f.NG * f.H16 : (which == 2 ? f.Co16 : f.C16);
  const float* src = which == 0 ? f.pwz : (which == 1 ? f.pwh : (which == 2 ? f.pwfl : f.pWinv));
  uint4* dst = which == 0 ? hwz : (which == 1 ? hwh : (which == 2 ? hwfl : hWinv));
  const long per = (long)(K16 >> 5) * 4 * J;            // uint4 entries per flow step and plane
  const f32x4* img = reinterpret_cast<const f32x4*>(src + (long)k * K16 * J);
  uint4* hi = dst + (long)k * 2 * per;
  uint4* lo = hi + per;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < per; idx += (long)gridDim.x * 256) {
    const int col = (int)(idx % J);
    const long r = idx / J;
    const int kq = (int)(r & 3), b = (int)(r >> 2);
    const X3FragH w = x3h_pack(img[((long)(2 * b) * 4 + kq) * J + col], img[((long)(2 * b + 1) * 4 + kq) * J + col]);
    hi[idx] = __builtin_bit_cast(uint4, w.hi);
    lo[idx] = __builtin_bit_cast(uint4, w.lo);
  }
}

// ActNorm2d.forward as a stand-alone module call (glow/modules.py:45-80): out = (x + bias) exp(logs), or its inverse
// x exp(-logs) - bias; dlogdet[0] = +-C * sum(logs) (the x C factor of modules.py:62)
__global__ __launch_bounds__(256) void actnorm_module_kernel(const float* __restrict__ x, long rows, int C, const float* __restrict__ bias,
                                                             const float* __restrict__ logs, int reverse, float* __restrict__ out,
                                                             float* __restrict__ dlogdet) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    out[i] = reverse ? x[i] * expf(-logs[c]) - bias[c] : (x[i] + bias[c]) * expf(logs[c]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && dlogdet) {
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += logs[c];
    dlogdet[0] = (reverse ? -(float)C : (float)C) * s;
  }
}

// ------------------------------------------------------------------------------------------- prep
// One workgroup per flow step: W = P (L*mask + I)(U*mask^T + diag(sign exp(log_s)))  (glow/modules.py:167-173),
// its transpose, and (optionally) the reverse weight U^-1 L^-1 P^-1 with fp64 triangular inverses (:175-177).
__global__ __launch_bounds__(256) void flow_prep_invconv_kernel(FlowK f, float* __restrict__ W, float* __restrict__ Wt,
                                                                float* __restrict__ Winv, double* __restrict__ dscratch,
                                                                float* __restrict__ ldpart) {
  __shared__ int piv;
  __shared__ double logabs;
  const int k = blockIdx.x, C = f.C, tid = threadIdx.x;
  float* Lm = flow_smem;            // C*C
  float* Um = Lm + C * C;           // C*C
  float* Tm = Um + C * C;           // C*C
  const long kc = (long)k * C * C;
  float* Wk = W + kc;
  float* Wtk = Wt + kc;
  if (f.p.inv_w) {
    for (int idx = tid; idx < C * C; idx += 256) {
      const int i = idx / C, j = idx - i * C;
      const float v = f.p.inv_w[kc + idx];
      Wk[idx] = v;
      Wtk[(long)j * C + i] = v;
    }
    // log|det| and inverse by Gauss-Jordan with partial pivoting in fp64 (torch.slogdet / torch.inverse(double))
    double* M = dscratch + (long)k * 2 * C * C;  // C x 2C augmented
    for (int idx = tid; idx < C * C; idx += 256) {
      const int i = idx / C, j = idx - i * C;
      M[(long)i * 2 * C + j] = (double)f.p.inv_w[kc + idx];
      M[(long)i * 2 * C + C + j] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) logabs = 0.0;
    __syncthreads();
    for (int col = 0; col < C; ++col) {
      if (tid == 0) {
        int best = col;
        double bv = fabs(M[(long)col * 2 * C + col]);
        for (int r = col + 1; r < C; ++r) {
          const double v = fabs(M[(long)r * 2 * C + col]);
          if (v > bv) { bv = v; best = r; }
        }
        piv = best;
        logabs += log(bv);
      }
      __syncthreads();
      const int pr = piv;
      if (pr != col)
        for (int j = tid; j < 2 * C; j += 256) {
          const double t0 = M[(long)col * 2 * C + j];
          M[(long)col * 2 * C + j] = M[(long)pr * 2 * C + j];
          M[(long)pr * 2 * C + j] = t0;
        }
      __syncthreads();
      const double pv = M[(long)col * 2 * C + col];
      __syncthreads();
      for (int j = tid; j < 2 * C; j += 256) M[(long)col * 2 * C + j] /= pv;
      __syncthreads();
      // two-pass elimination: every row's factor M[r][col] is read before any row is updated
      double* fac = dscratch + (long)f.Ks * 2 * C * C + (long)k * C;
      for (int r = tid; r < C; r += 256) fac[r] = (r == col) ? 0.0 : M[(long)r * 2 * C + col];
      __syncthreads();
      for (int idx = tid; idx < C * 2 * C; idx += 256) {
        const int r = idx / (2 * C), j = idx - r * 2 * C;
        M[(long)r * 2 * C + j] -= fac[r] * M[(long)col * 2 * C + j];
      }
      __syncthreads();
    }
    if (Winv)
      for (int idx = tid; idx < C * C; idx += 256) {
        const int i = idx / C, j = idx - i * C;
        Winv[kc + idx] = (float)M[(long)i * 2 * C + C + j];
      }
    if (tid == 0) {
      // (in fp64: the sum is scaled by C - the log-det is counted C times - and its rounding with it)
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += (double)f.p.an_logs[(long)k * C + c];
      ldpart[k] = (float)((double)C * (s + logabs));
    }
    return;
  }
  const float* l = f.p.inv_l + kc;
  const float* u = f.p.inv_u + kc;
  const float* P = f.p.inv_p + kc;
  const float* sg = f.p.inv_sign + (long)k * C;
  const float* ls = f.p.inv_logs + (long)k * C;
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    Lm[idx] = i > j ? l[idx] : (i == j ? 1.0f : 0.0f);
    Um[idx] = i < j ? u[idx] : (i == j ? sg[i] * expf(ls[i]) : 0.0f);
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += 256) {  // T = Lm Um
    const int i = idx / C, j = idx - i * C;
    float s = 0.0f;
    for (int q = 0; q < C; ++q) s += Lm[i * C + q] * Um[q * C + j];
    Tm[idx] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += 256) {  // W = P T
    const int i = idx / C, j = idx - i * C;
    float s = 0.0f;
    for (int q = 0; q < C; ++q) s += P[i * C + q] * Tm[q * C + j];
    Wk[idx] = s;
    Wtk[(long)j * C + i] = s;
  }
  if (tid == 0) {
    // in fp64: the log|s| of a well-conditioned W are of size 1 and cancel to a small sum, which is then scaled by C (the log-det
    // is counted C times) - a serial fp32 sum left 1e-6 of the per-frame NLL here, the same offset in every frame
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)f.p.an_logs[(long)k * C + c] + (double)ls[c];
    ldpart[k] = (float)((double)C * s);
  }
  if (!Winv) return;
  // fp64 triangular inverses by substitution, one column per thread
  double* Li = dscratch + (long)k * 2 * C * C;
  double* Ui = Li + C * C;
  __syncthreads();
  for (int j = tid; j < C; j += 256) {
    // Lm unit lower: solve Lm x = e_j
    for (int i = 0; i < C; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int q = j; q < i; ++q) s -= (double)Lm[i * C + q] * Li[(long)q * C + j];
      Li[(long)i * C + j] = i < j ? 0.0 : s;  // diagonal is 1
    }
    // Um upper: solve Um x = e_j
    for (int i = C - 1; i >= 0; --i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int q = i + 1; q <= j; ++q) s -= (double)Um[i * C + q] * Ui[(long)q * C + j];
      Ui[(long)i * C + j] = i > j ? 0.0 : s / (double)Um[i * C + i];
    }
  }
  __syncthreads();
  // reference order (fp32): w = u^-1 (l^-1 p^-1), p^-1 = p^T for a permutation
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    float s = 0.0f;
    for (int q = 0; q < C; ++q) s += (float)Li[(long)i * C + q] * P[j * C + q];
    Tm[idx] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    float s = 0.0f;
    for (int q = 0; q < C; ++q) s += (float)Ui[(long)i * C + q] * Tm[q * C + j];
    Winv[kc + idx] = s;
  }
}

__global__ __launch_bounds__(256) void flow_prep_transpose_kernel(FlowK f, float* __restrict__ wz_t, float* __restrict__ whh_t,
                                                                  float* __restrict__ wfl_t, float* __restrict__ wc,
                                                                  const float* __restrict__ ldpart, float* __restrict__ ldconst) {
  const int k = blockIdx.y;
  const int G = f.G, H = f.H, Ch = f.Ch, Cout = f.Cout, I = f.I, D = f.D;
  const long n1 = (long)Ch * G, n2 = (long)H * G, n3 = (long)H * Cout, n4 = (long)G * D;
  // wc[k][g][d] = w_ih[k][g][Ch + d]: the conditioning half of W_ih as its own 16-byte aligned matrix
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n4; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx / D), dd = (int)(idx - (long)g * D);
    wc[(long)k * n4 + idx] = f.p.w_ih[((long)k * G + g) * I + Ch + dd];
  }
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n1 + n2 + n3; idx += (long)gridDim.x * 256) {
    if (idx < n1) {
      const int c = (int)(idx / G), g = (int)(idx - (long)c * G);
      wz_t[(long)k * n1 + idx] = f.p.w_ih[((long)k * G + g) * I + c];
    } else if (idx < n1 + n2) {
      const long q = idx - n1;
      const int h = (int)(q / G), g = (int)(q - (long)h * G);
      whh_t[(long)k * n2 + q] = f.p.w_hh[((long)k * G + g) * H + h];
    } else {
      const long q = idx - n1 - n2;
      const int h = (int)(q / Cout), col = (int)(q - (long)h * Cout);
      wfl_t[(long)k * n3 + q] = f.p.w_fl[((long)k * Cout + col) * H + h];
    }
  }
  if (k == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.0f;
    for (int q = 0; q < f.Ks; ++q) s += ldpart[q];
    ldconst[0] = s;
  }
}

// Gradients of the LU parameters from dW (glow/modules.py:167-173 differentiated), one workgroup per flow step.
__global__ __launch_bounds__(256) void flow_invconv_bwd_kernel(FlowK f, const float* __restrict__ dW, lfi_flow_grads g,
                                                               float cconst, int accumulate, int stage) {
  const int k = blockIdx.x, C = f.C, tid = threadIdx.x;
  const long kc = (long)k * C * C;
  float* Lm = flow_smem;
  float* Um = Lm + C * C;
  float* Q = Um + C * C;  // P^T dW
  if (f.p.inv_w) {
    // dense: d weight = dW + cconst * W^-T   (d log|det W| / dW = W^-T)
    for (int idx = tid; idx < C * C; idx += 256) {
      const int i = idx / C, j = idx - i * C;
      const float v = dW[kc + idx] + cconst * f.Winv[kc + (long)j * C + i];
      g.inv_w[kc + idx] = accumulate ? g.inv_w[kc + idx] + v : v;
    }
    return;
  }
  const float* l = f.p.inv_l + kc;
  const float* u = f.p.inv_u + kc;
  const float* P = f.p.inv_p + kc;
  const float* sg = f.p.inv_sign + (long)k * C;
  const float* ls = f.p.inv_logs + (long)k * C;
  // (P and dW through LDS first: read from global inside the inner product - 100 dependent L2 round trips per thread - this
  // 16-workgroup kernel took 88 us alone and 260 us next to the HBM streams it shares its stream slot with)
  // (stage = 0, C > 90: five C x C images do not fit 160 KB of LDS - P and dW are then read where they lie, as before round 4)
  float* Pl = Q + C * C;
  float* Dl = Pl + C * C;
  const float* Pm = stage ? Pl : P;
  const float* Dm = stage ? Dl : dW + kc;
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    Lm[idx] = i > j ? l[idx] : (i == j ? 1.0f : 0.0f);
    Um[idx] = i < j ? u[idx] : (i == j ? sg[i] * expf(ls[i]) : 0.0f);
    if (stage) {
      Pl[idx] = P[idx];
      Dl[idx] = dW[kc + idx];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    float s = 0.0f;
    for (int q = 0; q < C; ++q) s += Pm[q * C + i] * Dm[q * C + j];
    Q[idx] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += 256) {
    const int i = idx / C, j = idx - i * C;
    if (i > j) {  // dL = Q Um^T, strictly lower
      float s = 0.0f;
      for (int q = 0; q < C; ++q) s += Q[i * C + q] * Um[j * C + q];
      g.inv_l[kc + idx] = accumulate ? g.inv_l[kc + idx] + s : s;
      if (!accumulate) g.inv_u[kc + idx] = 0.0f;
    } else {      // dU = Lm^T Q, upper incl. diagonal
      float s = 0.0f;
      for (int q = 0; q < C; ++q) s += Lm[q * C + i] * Q[q * C + j];
      if (i < j) {
        g.inv_u[kc + idx] = accumulate ? g.inv_u[kc + idx] + s : s;
        if (!accumulate) g.inv_l[kc + idx] = 0.0f;
      } else {
        const float v = s * sg[i] * expf(ls[i]) + cconst;
        const long o = (long)k * C + i;
        g.inv_logs[o] = accumulate ? g.inv_logs[o] + v : v;
        if (!accumulate) { g.inv_l[kc + idx] = 0.0f; g.inv_u[kc + idx] = 0.0f; }
      }
    }
  }
}

__global__ __launch_bounds__(256) void add_const_kernel(float* __restrict__ x, long n, float v) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] += v;
}

// ------------------------------------------------------------------------------------------- actnorm init
__global__ __launch_bounds__(256) void actnorm_stats_kernel(const float* __restrict__ x, int rows, int C, double* __restrict__ sums) {
  // one block; column c handled by threads c, c+256...; fixed-order fp64 sums
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0, s2 = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double v = (double)x[(long)r * C + c];
      s += v; s2 += v * v;
    }
    sums[c] = s; sums[C + c] = s2;
  }
}
__global__ __launch_bounds__(256) void actnorm_apply_kernel(const double* __restrict__ sums, double count, int C, float scale,
                                                            float* __restrict__ bias, float* __restrict__ logs) {
  for (int c = threadIdx.x; c < C; c += 256) {
    const double mean = sums[c] / count;
    double var = sums[C + c] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    bias[c] = (float)(-mean);
    logs[c] = (float)log((double)scale / (sqrt(var) + 1e-6));
  }
}

// ------------------------------------------------------------------------------------------- host helpers
long stash_offsets(const FlowK& f, long* off) {
  const long KF = (long)f.Ks * f.F;
  long o = 0;
  off[0] = o; o += KF * f.ldc;       // a      (rows of ldc = C rounded up to 4 floats)
  off[1] = o; o += KF * f.ldc;       // y
  off[2] = o; o += KF * f.ldc;       // x_out
  off[3] = o; o += KF * f.H;         // h
  o = (o + 3) & ~3L;
  off[4] = o; o += KF * 4 * f.H;     // gates: [frame][hidden unit][4], read and written 16 bytes at a time
  off[5] = o; o += KF * f.ldo;       // o      (rows of ldo = Cout rounded up to 4 floats)
  off[6] = o; o += KF;               // coupling log-det
  off[7] = o; o += f.lstm ? KF * f.H : 0;  // LSTM cell state
  return o;
}
long bstash_offsets(const FlowK& f, long* off) {
  const long KF = (long)f.Ks * f.F;
  long o = 0;
  off[0] = o; o += KF * f.ldo;       // dlin
  off[1] = o; o += KF * f.G;         // dgi
  off[2] = o; o += KF * f.G;         // dgh
  off[3] = o; o += KF * f.ldc;       // dy
  off[4] = o; o += KF * f.ldc;       // dx
  off[5] = o; o += KF * f.H;         // dh
  off[6] = o; o += (long)f.Ks * f.N * f.nbt * f.Cout;   // partial sums for l_fl
  off[7] = o; o += (long)f.Ks * f.N * f.nbt * 2 * f.C;  // partial sums for actnorm logs | bias
  off[8] = o; o += f.lstm ? KF * f.H : 0;               // carried d cell state (LSTM)
  off[9] = o; o += (long)f.Ks * f.nbt * 2 * f.G;        // partial sums for b_ih | b_hh (persistent walk)
  return o;
}
// persistent-pipeline state appended to either stash: header + one progress word per (flow step, batch tile), padded to 16 bytes
long pipe_words(const FlowK& f) { return ((long)PIPE_WALK_HDR + (long)f.Ks * f.nbt * PIPE_STRIDE + 3) & ~3L; }
long align4(long x) { return (x + 3) & ~3L; }
void bind_stash(FlowK* f, float* stash) {
  long off[8];
  stash_offsets(*f, off);
  f->sA = stash + off[0]; f->sY = stash + off[1]; f->sX = stash + off[2]; f->sH = stash + off[3];
  f->sG = stash + off[4]; f->sO = stash + off[5]; f->sL = stash + off[6]; f->sC = stash + off[7];
}
void bind_bstash(FlowK* f, float* b) {
  long off[10];
  bstash_offsets(*f, off);
  f->bDlin = b + off[0]; f->bDgi = b + off[1]; f->bDgh = b + off[2]; f->bDy = b + off[3];
  f->bDx = b + off[4]; f->bDh = b + off[5]; f->bPlfl = b + off[6]; f->bPan = b + off[7]; f->bDc = b + off[8];
  f->bPbias = b + off[9];
}

// ---- which instantiation runs: one picker per kernel family; set_flow_lds and the launch take the pointer
typedef void (*FlowDiagKernel)(FlowK, int, int);
typedef void (*FlowPipeKernel)(FlowK);

FlowDiagKernel flow_diag_fwd_pick(bool fast, bool lstm) {
  if (!fast) return flow_diag_fwd_kernel;
  return lstm ? flow_diag_fwd_fast_kernel<4> : flow_diag_fwd_fast_kernel<3>;
}
FlowDiagKernel flow_diag_bwd_pick(bool fast, bool lstm) {
  if (!fast) return flow_diag_bwd_kernel;
  return lstm ? flow_diag_bwd_fast_kernel<4> : flow_diag_bwd_fast_kernel<3>;
}
FlowPipeKernel flow_pipe_fwd_pick(bool lstm, bool x3) {
  if (lstm) return flow_pipe_fwd_kernel<4, false>;
  return x3 ? flow_pipe_fwd_kernel<3, true> : flow_pipe_fwd_kernel<3, false>;
}
FlowPipeKernel flow_pipe_bwd_pick(bool lstm, bool x3) {
  if (lstm) return flow_pipe_bwd_kernel<4, false>;
  return x3 ? flow_pipe_bwd_kernel<3, true> : flow_pipe_bwd_kernel<3, false>;
}

// ---- which walk a call takes (lfi_flow_walk_variant's codes): the ONE place the three entry points and the query decide it.
// 0 generic diagonal cells, 1 register-resident diagonal cells, 2 persistent walk with exact f32 recurrent products, 3 persistent
// walk with bf16x3 recurrent products. backward: the backward walk's rule (flow_x3_bwd_walk) instead of the forward walk's.
int flow_walk_code(const lfi_flow_dims* d, const FlowK& f, bool backward) {
  if (!flow_fast_ok(f.C, f.H, f.Cout) || flow_force_generic()) return 0;
  if (!flow_pipe_enabled()) return 1;
  return (backward ? flow_x3_bwd_walk(d, f) : flow_x3_fwd_walk(d, f)) ? 3 : 2;
}
// LFI_FLOW_WGRAD_FUSED=0: the thin weight-gradient products as four batched split-K launches + a column-sum pass (rounds 2 - 5)
bool flow_wgrad_fused_enabled() { return lfi_env_on("LFI_FLOW_WGRAD_FUSED"); }
// the thin products of lfi_flow_param_grads in one pass (lfi_wgrad.hip): bf16 gradient rows, GRU, the shapes that file is built for
bool flow_wgrad_one_pass(const lfi_flow_dims* d, const FlowK& f) {
  return ((d->gemm_precision >> 16) & 1) && !f.lstm && flow_wgrad_fused_enabled() &&
         lfi_internal_flow_wgrad_ok(f.B, f.N, f.C, f.Ch, f.Cout, f.H, f.G, f.ldc, f.ldo) != 0;
}

// start state of a persistent walk: header and progress words cleared (LFI_PIPE_FORCE_ABORT=1: the abort word already set)
int flow_pipe_reset(const FlowK& f, hipStream_t st, const char* who) {
  hipError_t me = hipMemsetAsync(f.pipe, 0, (size_t)pipe_words(f) * sizeof(unsigned), st);
  LFI_REQUIRE(me == hipSuccess, "%s: hipMemsetAsync: %s", who, hipGetErrorString(me));
  if (flow_pipe_force_abort()) (void)hipMemsetAsync(f.pipe + 1, 1, sizeof(unsigned), st);
  return LFI_OK;
}

}  // namespace

// =================================================================================================== C ABI
// Diagnostics: device buffer of >= 16 * Ks 64-bit slots that the register-resident forward cells stamp with s_memtime at
// their phase boundaries (workgroup column 0 only); NULL switches it off. Process-global, not for production use.
extern "C" int lfi_debug_set_stamps(void* device_buffer) {
  g_lfi_stamps = (unsigned long long*)device_buffer;
  return LFI_OK;
}

extern "C" long lfi_flow_prep_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  // published layout, scratch (per-step log-det parts, fp64 workspace for the inverses), zero-padded cell images
  return prep_scratch_end(d) + prep_padded_floats(d) + 16;
}

extern "C" int lfi_flow_prep(const lfi_flow_dims* d, const lfi_flow_params* p, float* prep, int with_inverse, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_prep");
  if (rc) return rc;
  LFI_REQUIRE(prep, "lfi_flow_prep: null prep buffer");
  LFI_REQUIRE((p->inv_w != nullptr) || (p->inv_l && p->inv_u && p->inv_logs && p->inv_p && p->inv_sign),
              "lfi_flow_prep: invconv parameters missing");
  hipStream_t st = (hipStream_t)stream;
  float* ldconst = (float*)f.ldconst;
  float* ldpart = ldconst + 4;
  // 8-byte aligned fp64 scratch after the float part
  uintptr_t dp = (uintptr_t)(ldpart + d->Ks + 4);
  dp = (dp + 7) & ~(uintptr_t)7;
  double* dscratch = (double*)dp;
  const size_t lds = (size_t)3 * d->C * d->C * sizeof(float);
  rc = set_flow_lds(flow_prep_invconv_kernel, lds, "lfi_flow_prep");
  if (rc) return rc;
  hipLaunchKernelGGL(flow_prep_invconv_kernel, dim3(d->Ks), dim3(256), lds, st, f, (float*)f.W, (float*)f.Wt,
                     (with_inverse || p->inv_w) ? (float*)f.Winv : nullptr, dscratch, ldpart);
  LFI_LAUNCH_CHECK("lfi_flow_prep invconv");
  hipLaunchKernelGGL(flow_prep_transpose_kernel, dim3(64, d->Ks), dim3(256), 0, st, f, (float*)f.wz_t, (float*)f.whh_t,
                     (float*)f.wfl_t, (float*)f.wc, ldpart, ldconst);
  LFI_LAUNCH_CHECK("lfi_flow_prep transpose");
  if (flow_fast_ok(f.C, f.H, f.Cout)) {
    hipLaunchKernelGGL(flow_prep_pad_kernel, dim3(8, d->Ks, 9), dim3(256), 0, st, f, (float*)f.pW, (float*)f.pWt, (float*)f.pwz,
                       (float*)f.pwh, (float*)f.pwfl, (float*)f.bwfl, (float*)f.bwh, (float*)f.bwz,
                       (with_inverse || p->inv_w) ? (float*)f.pWinv : nullptr);
    LFI_LAUNCH_CHECK("lfi_flow_prep pad");
    if (flow_x3_prep_images(d, f)) {
      hipLaunchKernelGGL(flow_prep_x3_kernel, dim3(16, d->Ks, 2), dim3(256), 0, st, f, const_cast<uint4*>(f.xbwh),
                         const_cast<uint4*>(f.xbwz));
      LFI_LAUNCH_CHECK("lfi_flow_prep x3");
    }
    if ((with_inverse || p->inv_w) && flow_x3h_images_ok(f)) {   // (whatever the precision of this call: the sampler picks its own)
      hipLaunchKernelGGL(flow_prep_x3h_kernel, dim3(8, d->Ks, 4), dim3(256), 0, st, f, const_cast<uint4*>(f.hwz),
                         const_cast<uint4*>(f.hwh), const_cast<uint4*>(f.hwfl), const_cast<uint4*>(f.hWinv));
      LFI_LAUNCH_CHECK("lfi_flow_prep x3h");
    }
  }
  return LFI_OK;
}

extern "C" long lfi_flow_stash_floats(const lfi_flow_dims* d) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (fill_flow(d, &p, nullptr, &f, "lfi_flow_stash_floats")) return -1;
  long off[8];
  return align4(stash_offsets(f, off)) + pipe_words(f);
}
extern "C" long lfi_flow_bstash_floats(const lfi_flow_dims* d) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (fill_flow(d, &p, nullptr, &f, "lfi_flow_bstash_floats")) return -1;
  long off[10];
  return align4(bstash_offsets(f, off)) + pipe_words(f);
}
extern "C" float* lfi_flow_stash_ptr(const lfi_flow_dims* d, float* stash, int which) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (which < 0 || which > 8 || fill_flow(d, &p, nullptr, &f, "lfi_flow_stash_ptr")) return nullptr;
  long off[8];
  const long end = stash_offsets(f, off);
  if (which == 8) return stash + align4(end);
  return stash + off[which];
}
extern "C" float* lfi_flow_bstash_ptr(const lfi_flow_dims* d, float* bstash, int which) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (which < 0 || which > 9 || fill_flow(d, &p, nullptr, &f, "lfi_flow_bstash_ptr")) return nullptr;
  long off[10];
  const long end = bstash_offsets(f, off);
  if (which == 9) return bstash + align4(end);
  return bstash + off[which];
}

extern "C" int lfi_flow_seq_fwd(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* x0, int T,
                                int start, const float* gic, float* stash, float* z, float* nll, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_seq_fwd");
  if (rc) return rc;
  LFI_REQUIRE(prep && x0 && gic && stash && nll, "lfi_flow_seq_fwd: null pointer");
  LFI_REQUIRE(start >= 0 && start + d->N <= T, "lfi_flow_seq_fwd: start %d + N %d > T %d", start, d->N, T);
  bind_stash(&f, stash);
  f.x0 = x0; f.T = T; f.start = start; f.gic = gic;
  hipStream_t st = (hipStream_t)stream;
  const int variant = flow_walk_code(d, f, false);
  const bool fast = variant >= 1;
  const Carve cv = carve_fwd(f.C, f.H, f.Ch, f.C2, f.Cout);
  const CarveF cf = carve_fast_fwd(f.C, f.C16, f.H16, f.Ch16, f.Cout);
  const size_t lds = (size_t)(fast ? cf.total : cv.total) * sizeof(float);
  const FlowDiagKernel diag = flow_diag_fwd_pick(fast, f.lstm);
  if ((rc = set_flow_lds(diag, lds, "lfi_flow_seq_fwd"))) return rc;
  const bool pipe = variant >= 2;
  if (pipe) {
    long off[8];
    f.pipe = reinterpret_cast<unsigned*>(stash + align4(stash_offsets(f, off)));
    f.pipe_fence = flow_pipe_fence();
    const size_t plds = (size_t)pipe_fwd_lds_floats(f.C, f.C16, f.H16, f.Ch16, f.Cout, f.Co16) * sizeof(float);
    const FlowPipeKernel walk = flow_pipe_fwd_pick(f.lstm, variant == 3);
    if ((rc = set_flow_lds(walk, plds, "lfi_flow_seq_fwd"))) return rc;
    if ((rc = flow_pipe_reset(f, st, "lfi_flow_seq_fwd"))) return rc;
    hipLaunchKernelGGL(walk, dim3(f.Ks * f.nbt), dim3(NT), plds, st, f);
  }
  for (int dg = 0; !pipe && dg < f.N + f.Ks - 1; ++dg) {
    const int klo = dg - (f.N - 1) > 0 ? dg - (f.N - 1) : 0;
    const int khi = dg < f.Ks - 1 ? dg : f.Ks - 1;
    const dim3 grid(f.nbt, khi - klo + 1);
    hipLaunchKernelGGL(diag, grid, dim3(NT), lds, st, f, dg, klo);
  }
  LFI_LAUNCH_CHECK("lfi_flow_seq_fwd");
  if (f.C <= NLL_CMAX)
    hipLaunchKernelGGL(flow_nll_kernel<true>, dim3(lfi_cdiv(f.F, NLL_FR)), dim3(256), (size_t)NLL_FR * (f.C + 1) * sizeof(float), st, f, z, nll);
  else
    hipLaunchKernelGGL(flow_nll_kernel<false>, dim3(lfi_cdiv(f.F, 256)), dim3(256), 0, st, f, z, nll);
  LFI_LAUNCH_CHECK("lfi_flow_seq_fwd nll");
  return LFI_OK;
}

// Can the backward walk of these dims leave dgi as operand planes? It takes the persistent walk with bf16x3 recurrent products
// (whose d(gate) LDS images are the source), gate columns that are the stash's (H a multiple of 32: no padding columns) and
// batch tiles that pair up into whole 32-row plane tiles (B a multiple of 32).
static bool flow_bwd_planes_ok(const lfi_flow_dims* d) {
  if (!d || !flow_x3_bwd_planes(d) || d->B % 32 != 0) return false;
  FlowK f = {};
  lfi_flow_params p = {};
  return fill_flow(d, &p, nullptr, &f, "lfi_flow_bwd_emits_planes") == LFI_OK && flow_walk_code(d, f, true) == 3;
}
extern "C" int lfi_flow_bwd_emits_planes(const lfi_flow_dims* d) { return flow_bwd_planes_ok(d) ? 1 : 0; }

extern "C" int lfi_flow_walk_variant(const lfi_flow_dims* d, int which) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (which < 0 || which > 2 || fill_flow(d, &p, nullptr, &f, "lfi_flow_walk_variant")) return -1;
  if (which == 2) return flow_wgrad_one_pass(d, f) ? 1 : 0;
  return flow_walk_code(d, f, which == 1);
}

extern "C" int lfi_flow_seq_bwd(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* stash,
                                float gscale, float* bstash, void* stream) {
  return lfi_flow_seq_bwd_planes(d, p, prep, stash, gscale, bstash, nullptr, 0, stream);
}

extern "C" int lfi_flow_seq_bwd_planes(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* stash,
                                       float gscale, float* bstash, void* dgi_rows, int hi_only, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_seq_bwd");
  if (rc) return rc;
  LFI_REQUIRE(prep && stash && bstash, "lfi_flow_seq_bwd: null pointer");
  LFI_REQUIRE(!dgi_rows || flow_bwd_planes_ok(d), "lfi_flow_seq_bwd_planes: these dims / switches cannot emit planes "
              "(lfi_flow_bwd_emits_planes returns 0)");
  LFI_REQUIRE((reinterpret_cast<uintptr_t>(dgi_rows) & 15) == 0, "lfi_flow_seq_bwd_planes: planes must be 16-byte aligned");
  bind_stash(&f, (float*)stash);
  bind_bstash(&f, bstash);
  f.bDgiR = reinterpret_cast<__bf16*>(dgi_rows);
  f.dgi_hi_only = hi_only ? 1 : 0;
  f.g16 = (dgi_rows && ((d->gemm_precision >> 16) & 1)) ? 1 : 0;
  f.gscale = gscale;
  hipStream_t st = (hipStream_t)stream;
  const int variant = flow_walk_code(d, f, true);
  const bool fast = variant >= 1;
  const CarveB cv = carve_bwd(f.C, f.H, f.Cout, f.G);
  const CarveFB cf = carve_fast_bwd(f.C16, f.H16, f.Co16, f.Cout, f.NG);
  const size_t lds = (size_t)(fast ? cf.total : cv.total) * sizeof(float);
  const FlowDiagKernel diag = flow_diag_bwd_pick(fast, f.lstm);
  if ((rc = set_flow_lds(diag, lds, "lfi_flow_seq_bwd"))) return rc;
  const bool pipe = variant >= 2;
  if (pipe) {
    long off[10];
    f.pipe = reinterpret_cast<unsigned*>(bstash + align4(bstash_offsets(f, off)));
    f.pipe_fence = flow_pipe_fence();
    const bool x3 = variant == 3;
    // + the bf16 hi / lo image of d lin (Q1's bf16 x 3 operand): 2 x MB rows of 32 ceil(Co16 / 32) + 8 bf16
    const size_t plds = x3 ? (((size_t)cf.total + 3) & ~(size_t)3) * sizeof(float) + (size_t)2 * MB * (32 * ((f.Co16 + 31) / 32) + 8) * 2 : lds;
    const FlowPipeKernel walk = flow_pipe_bwd_pick(f.lstm, x3);
    if ((rc = set_flow_lds(walk, plds, "lfi_flow_seq_bwd"))) return rc;
    if ((rc = flow_pipe_reset(f, st, "lfi_flow_seq_bwd"))) return rc;
    hipLaunchKernelGGL(walk, dim3(f.Ks * f.nbt), dim3(NT), plds, st, f);
    hipLaunchKernelGGL(flow_pipe_poison_kernel, dim3(1), dim3(64), 0, st, f);
  }
  for (int dg = f.N + f.Ks - 2; !pipe && dg >= 0; --dg) {
    const int klo = dg - (f.N - 1) > 0 ? dg - (f.N - 1) : 0;
    const int khi = dg < f.Ks - 1 ? dg : f.Ks - 1;
    const dim3 grid(f.nbt, khi - klo + 1);
    hipLaunchKernelGGL(diag, grid, dim3(NT), lds, st, f, dg, klo);
  }
  LFI_LAUNCH_CHECK("lfi_flow_seq_bwd");
  return LFI_OK;
}

extern "C" long lfi_flow_param_grads_work_floats(const lfi_flow_dims* d) {
  FlowK f = {};
  lfi_flow_params p = {};
  if (fill_flow(d, &p, nullptr, &f, "lfi_flow_param_grads_work_floats")) return -1;
  const int splitk = 16;
  long gemm_ws = (long)f.Ks * splitk * ((long)f.G * f.I > (long)f.C * f.C ? (long)f.G * f.I : (long)f.C * f.C);
  long cs = lfi_colsum_work_floats(f.F > f.N * f.nbt ? f.F : f.N * f.nbt, f.G > 2 * f.C ? f.G : 2 * f.C, f.Ks);
  // + a second split-K workspace for the products that run on bias_stream
  // + the per-workgroup partials of the one-pass form of the thin products (lfi_wgrad.hip)
  long fused = 0;
  if (lfi_internal_flow_wgrad_ok(f.B, f.N, f.C, f.Ch, f.Cout, f.H, f.G, f.ldc, f.ldo))
    fused = lfi_internal_flow_wgrad_work_floats(f.B, f.N, f.Ks, 0) + lfi_internal_flow_wgrad_work_floats(f.B, f.N, f.Ks, 1) + 32;
  return (long)f.Ks * f.C * f.C + gemm_ws + cs + 16 + gemm_ws + 16 + fused;
}

extern "C" int lfi_flow_param_grads(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* stash,
                                    const float* bstash, const float* c, long ldc, float gscale, const lfi_flow_grads* g,
                                    int accumulate, float* work, void* stream, void* bias_stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_param_grads");
  if (rc) return rc;
  LFI_REQUIRE(prep && stash && bstash && g && work, "lfi_flow_param_grads: null pointer");
  bind_stash(&f, (float*)stash);
  bind_bstash(&f, (float*)bstash);
  const int Ks = f.Ks, F = f.F, B = f.B, C = f.C, H = f.H, G = f.G, I = f.I, Cout = f.Cout, Ch = f.Ch, D = f.D;
  float* dW = work;                       // [Ks][C][C]
  float* gws = dW + (long)Ks * C * C;     // split-k workspace
  const int splitk = 16;
  const long gws_floats = (long)Ks * splitk * ((long)G * I > (long)C * C ? (long)G * I : (long)C * C);
  float* cws = gws + gws_floats;          // colsum workspace
  const long cws_floats = lfi_colsum_work_floats(F > f.N * f.nbt ? F : f.N * f.nbt, G > 2 * C ? G : 2 * C, Ks);
  float* gws2 = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(cws + cws_floats) + 63) & ~(uintptr_t)63);  // dW split-K partials
  void* bs = bias_stream ? bias_stream : stream;

  // gemm_precision bit 16 (with the walk's planes mode): dgi | dgh rows are bf16 (FlowK.g16) - the two products that read them take
  // them as an operand that arrives rounded (lfi_gemm_desc.a_bf16: two-product mode, i.e. skip bit 0 set by the caller)
  const bool g16 = ((d->gemm_precision >> 16) & 1) != 0;
  LFI_REQUIRE(!g16 || (flow_bwd_planes_ok(d) && !c && (d->gemm_precision & 0x100) && !(d->gemm_precision & 0x200)),
              "lfi_flow_param_grads: bf16 gradient rows (gemm_precision bit 16) need the walk's planes mode and two-product thin products");
  lfi_gemm_desc q = {};
  q.batch = Ks; q.accumulate = accumulate; q.splitk = splitk; q.work = gws; q.precision = d->gemm_precision & 0xffff;
  q.a_kcontig = 0; q.b_kcontig = 0; q.K = F;
  // K split (<= 16, what the workspace holds) of a K = F product with Ks x few 128 x 128 output tiles: the one that best
  // fills whole rounds of the 512 co-resident workgroups, less 3 % per extra partial for the reduce pass
  auto fill_split = [&](int M, int N, int K) {
    const double tiles = (double)lfi_cdiv(M, 128) * lfi_cdiv(N, 128) * Ks;
    int best = 1;
    double best_score = -1.0;
    for (int sk = 1; sk <= splitk && K / sk >= 512; ++sk) {
      const double wg = tiles * sk, rounds = (double)(long)((wg + 511.0) / 512.0);
      const double score = wg / (rounds * 512.0) * (1.0 - 0.03 * (sk - 1));
      if (score > best_score + 1e-9) { best_score = score; best = sk; }
    }
    return best;
  };
  // w_ih[k][:, Ch:] (G x D) = dgi[k]^T c[:, kD:(k+1)D]: the one MFMA-bound product (it reads c: before the caller's dpre
  // product overwrites it)
  // (c == NULL: the caller runs this product on operand planes itself - lfi_gemm_planes on the walk's dgi planes and c's)
  if (c) {
    q.M = G; q.N = D; q.splitk = fill_split(G, D, F); q.A = f.bDgi; q.lda = G; q.strideA = (long)F * G; q.B = c; q.ldb = ldc; q.strideB = D;
    q.C = g->w_ih + Ch; q.ldc = I; q.strideC = (long)G * I;
    if ((rc = lfi_gemm_f32(&q, stream))) return rc;
  }
  // Round 6: ONE pass over the backward stash for all of the thin products below, b_fl's column sums included (lfi_wgrad.hip) -
  // when the walk left dgi | dgh as bf16 rows (two-product mode) and the shapes are the register-resident cell's. Two roles:
  // w_hh | w_fl | b_fl in line on `stream` (its workgroups hold a CU each: beside the caller's MFMA-bound dgi^T c product on the
  // other stream both ran at half speed, profiles/round6_thin_products_ab.md), w_ih[:, :Ch] | dW (two workgroups per CU) on
  // bias_stream, where dW's reader, the LU-gradient kernel, follows (LFI_FLOW_WGRAD_IH=main: in line as well).
  const bool fused = flow_wgrad_one_pass(d, f);
  if (fused) {
    float* part0 = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(gws2 + gws_floats) + 63) & ~(uintptr_t)63);
    float* part1 = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(part0 + lfi_internal_flow_wgrad_work_floats(B, f.N, Ks, 0)) + 63) & ~(uintptr_t)63);
    const char* ws = getenv("LFI_FLOW_WGRAD_IH");
    void* s1 = (ws && ws[0] == 'm') ? stream : bs;   // default: side (same-box A/B 6.44 against 6.48 ms per step in line)
    if ((rc = lfi_internal_flow_wgrad(1, B, f.N, Ks, C, Ch, Cout, I, f.ldc, f.ldo, f.bDgh, f.bDgi, f.sH, f.bDlin, f.sY, f.sA, f.bDy, part1,
                                      g->w_hh, g->w_ih, g->w_fl, g->b_fl, dW, accumulate, s1)))
      return rc;
    if (s1 != bs) {   // the LU-gradient kernel below reads dW on bias_stream
      hipEvent_t ev;
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { lfi_set_error("lfi_flow_param_grads: hipEventCreate failed"); return LFI_ERR_LAUNCH; }
      (void)hipEventRecord(ev, (hipStream_t)s1);
      (void)hipStreamWaitEvent((hipStream_t)bs, ev, 0);
      (void)hipEventDestroy(ev);
    }
    if ((rc = lfi_internal_flow_wgrad(0, B, f.N, Ks, C, Ch, Cout, I, f.ldc, f.ldo, f.bDgh, f.bDgi, f.sH, f.bDlin, f.sY, f.sA, f.bDy, part0,
                                      g->w_hh, g->w_ih, g->w_fl, g->b_fl, dW, accumulate, stream)))
      return rc;
  } else {
  // The other products are thin (K = F frames, a few output tiles per step), HBM-bound at 3 - 4 TB/s. (Moving them to
  // bias_stream as well, next to the caller's MFMA-bound products, was measured no better than leaving them here: same-box
  // A/B 0.18 ms per step gained with them there, 0.21 ms without; round 4, any one or two of them: 6.86 - 6.91 ms per step
  // whichever way.)
  // w_fl[k] (Cout x H) = dlin[k]^T h[k]
  q.M = Cout; q.N = H; q.splitk = fill_split(Cout, H, F); q.A = f.bDlin; q.lda = f.ldo; q.strideA = (long)F * f.ldo; q.B = f.sH; q.ldb = H; q.strideB = (long)F * H;
  q.C = g->w_fl; q.ldc = H; q.strideC = (long)Cout * H;
  if ((rc = lfi_gemm_f32(&q, stream))) return rc;
  // w_hh[k] (G x H) = dgh[k][n >= 1]^T h[k][n - 1]
  if (f.N > 1) {
    q.K = F - B; q.M = G; q.N = H; q.splitk = fill_split(G, H, F - B); q.A = f.bDgh + (long)B * G; q.lda = G; q.strideA = (long)F * G; q.B = f.sH; q.ldb = H;
    q.strideB = (long)F * H; q.C = g->w_hh; q.ldc = H; q.strideC = (long)G * H;
    if (g16) { q.a_bf16 = 1; q.A = reinterpret_cast<const float*>(reinterpret_cast<const __bf16*>(f.bDgh) + (long)B * G); }
    if ((rc = lfi_gemm_f32(&q, stream))) return rc;
    q.a_bf16 = 0;
  } else if (!accumulate) {
    (void)hipMemsetAsync(g->w_hh, 0, sizeof(float) * (size_t)Ks * G * H, (hipStream_t)stream);
  }
  q.K = F;
  // w_ih[k][:, :Ch] (G x Ch) = dgi[k]^T z1[k]
  if (Ch > 0) {
    q.M = G; q.N = Ch; q.splitk = fill_split(G, Ch, F); q.A = f.bDgi; q.lda = G; q.strideA = (long)F * G; q.B = f.sY; q.ldb = f.ldc; q.strideB = (long)F * f.ldc;
    q.C = g->w_ih; q.ldc = I; q.strideC = (long)G * I;
    q.a_bf16 = g16 ? 1 : 0;
    if ((rc = lfi_gemm_f32(&q, stream))) return rc;
    q.a_bf16 = 0;
  }
  // dW[k] (C x C) = a[k]^T dy[k]  -> LU parameter gradients, then a 16-workgroup kernel: on bias_stream (with a split-K
  // workspace of their own) they run next to the products above instead of holding the chip for 0.14 ms
  q.accumulate = 0; q.work = gws2;
  q.M = C; q.N = C; q.splitk = fill_split(C, C, F); q.A = f.sA; q.lda = f.ldc; q.strideA = (long)F * f.ldc; q.B = f.bDy; q.ldb = f.ldc; q.strideB = (long)F * f.ldc;
  q.C = dW; q.ldc = C; q.strideC = (long)C * C;
  if ((rc = lfi_gemm_f32(&q, bs))) return rc;
  }
  // constant log-det terms: nll has -(C sum(logs))/ln2 per frame -> d/dlogs = -C/ln2 * gscale * F
  const float cconst = -(float)((double)gscale * (double)F * (double)C / 0.6931471805599453);
  {
    const int stage = (size_t)5 * C * C * sizeof(float) <= 160 * 1024 ? 1 : 0;
    const size_t lds = (size_t)(stage ? 5 : 3) * C * C * sizeof(float);
    rc = set_flow_lds(flow_invconv_bwd_kernel, lds, "lfi_flow_param_grads");
    if (rc) return rc;
    hipLaunchKernelGGL(flow_invconv_bwd_kernel, dim3(Ks), dim3(256), lds, (hipStream_t)bs, f, dW, *g, cconst, accumulate, stage);
    LFI_LAUNCH_CHECK("lfi_flow_param_grads invconv");
  }
  // biases and the per-tile partial sums: column sums over the backward stash only (HBM streams), independent of the
  // products above - on bias_stream when the caller has forked one after the backward walk
  if (!fused && (rc = lfi_colsum_f32(f.bDlin, f.ldo, (long)F * f.ldo, F, Cout, Ks, g->b_fl, Cout, 1.0f, accumulate, cws, bs))) return rc;
  if (flow_walk_code(d, f, true) >= 2) {
    // the persistent backward walk left per-workgroup sums of dgi | dgh: [Ks][nbt][2][G]
    if ((rc = lfi_colsum_f32(f.bPbias, 2 * G, (long)f.nbt * 2 * G, f.nbt, G, Ks, g->b_ih, G, 1.0f, accumulate, cws, bs))) return rc;
    if ((rc = lfi_colsum_f32(f.bPbias + G, 2 * G, (long)f.nbt * 2 * G, f.nbt, G, Ks, g->b_hh, G, 1.0f, accumulate, cws, bs))) return rc;
  } else {
    if ((rc = lfi_colsum_f32(f.bDgh, G, (long)F * G, F, G, Ks, g->b_hh, G, 1.0f, accumulate, cws, bs))) return rc;
    if ((rc = lfi_colsum_f32(f.bDgi, G, (long)F * G, F, G, Ks, g->b_ih, G, 1.0f, accumulate, cws, bs))) return rc;
  }
  const int prow = f.N * f.nbt;
  if ((rc = lfi_colsum_f32(f.bPlfl, Cout, (long)prow * Cout, prow, Cout, Ks, g->l_fl, Cout, 1.0f, accumulate, cws, bs))) return rc;
  if ((rc = lfi_colsum_f32(f.bPan, 2 * C, (long)prow * 2 * C, prow, C, Ks, g->an_logs, C, 1.0f, accumulate, cws, bs))) return rc;
  if ((rc = lfi_colsum_f32(f.bPan + C, 2 * C, (long)prow * 2 * C, prow, C, Ks, g->an_bias, C, 1.0f, accumulate, cws, bs))) return rc;
  hipLaunchKernelGGL(add_const_kernel, dim3(lfi_cdiv((long)Ks * C, 256)), dim3(256), 0, (hipStream_t)bs, g->an_logs, (long)Ks * C, cconst);
  LFI_LAUNCH_CHECK("lfi_flow_param_grads const");
  return LFI_OK;
}

extern "C" int lfi_actnorm_init_stats(const float* x, int rows, int C, double* sums, void* stream) {
  LFI_REQUIRE(x && sums && rows > 0 && C > 0, "lfi_actnorm_init_stats: bad arguments");
  hipLaunchKernelGGL(actnorm_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, rows, C, sums);
  LFI_LAUNCH_CHECK("lfi_actnorm_init_stats");
  return LFI_OK;
}
extern "C" int lfi_actnorm_init_apply(const double* sums, double count, int C, float scale, float* bias, float* logs,
                                      void* stream) {
  LFI_REQUIRE(sums && bias && logs && count > 0 && C > 0, "lfi_actnorm_init_apply: bad arguments");
  hipLaunchKernelGGL(actnorm_apply_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, count, C, scale, bias, logs);
  LFI_LAUNCH_CHECK("lfi_actnorm_init_apply");
  return LFI_OK;
}

// ---------------------------------------------------------------------------------------------- stand-alone module calls
// What the reference's test_modules.py:9-29 pokes directly: ActNorm2d and InvertibleConv1x1 outside any flow.
extern "C" int lfi_actnorm_forward(const float* x, int rows, int C, const float* bias, const float* logs, int reverse, float* out,
                                   float* dlogdet, void* stream) {
  LFI_REQUIRE(x && bias && logs && out && rows > 0 && C > 0, "lfi_actnorm_forward: bad arguments");
  const long total = (long)rows * C;
  const int blocks = (int)(lfi_cdiv(total, 256) < 2048 ? lfi_cdiv(total, 256) : 2048);
  hipLaunchKernelGGL(actnorm_module_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (long)rows, C, bias, logs, reverse, out,
                     dlogdet);
  LFI_LAUNCH_CHECK("lfi_actnorm_forward");
  return LFI_OK;
}

extern "C" long lfi_invconv_work_floats(int C) {
  if (C <= 0) return 0;
  return 2L * (2L * C * C + C) + (long)C * C + C + 16;   // fp64 scratch (as floats), W^T, a zero ActNorm row
}

extern "C" int lfi_invconv_weights(int C, const float* inv_l, const float* inv_u, const float* inv_logs, const float* inv_p,
                                   const float* inv_sign, const float* inv_w, int with_inverse, float* W, float* Winv,
                                   float* dlogdet, float* work, void* stream) {
  LFI_REQUIRE(C >= 2 && W && dlogdet && work, "lfi_invconv_weights: bad arguments");
  LFI_REQUIRE(inv_w || (inv_l && inv_u && inv_logs && inv_p && inv_sign), "lfi_invconv_weights: invconv parameters missing");
  LFI_REQUIRE(!with_inverse || Winv, "lfi_invconv_weights: with_inverse needs Winv");
  LFI_REQUIRE(((uintptr_t)work & 7) == 0, "lfi_invconv_weights: work must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* dscratch = reinterpret_cast<double*>(work);
  float* Wt = work + 2L * (2L * C * C + C);
  float* zeros = Wt + (long)C * C;
  hipError_t me = hipMemsetAsync(zeros, 0, sizeof(float) * (size_t)C, st);
  LFI_REQUIRE(me == hipSuccess, "lfi_invconv_weights: hipMemsetAsync: %s", hipGetErrorString(me));
  FlowK f = {};
  f.C = C; f.Ks = 1;
  f.p.inv_l = inv_l; f.p.inv_u = inv_u; f.p.inv_logs = inv_logs; f.p.inv_p = inv_p; f.p.inv_sign = inv_sign; f.p.inv_w = inv_w;
  f.p.an_logs = zeros;   // the kernel adds the ActNorm part of the constant log-det: none here
  const size_t lds = (size_t)3 * C * C * sizeof(float);
  int rc = set_flow_lds(flow_prep_invconv_kernel, lds, "lfi_invconv_weights");
  if (rc) return rc;
  hipLaunchKernelGGL(flow_prep_invconv_kernel, dim3(1), dim3(256), lds, st, f, W, Wt, (with_inverse || inv_w) ? Winv : nullptr, dscratch,
                     dlogdet);
  LFI_LAUNCH_CHECK("lfi_invconv_weights");
  return LFI_OK;
}
