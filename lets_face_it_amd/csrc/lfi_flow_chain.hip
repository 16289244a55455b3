// The per-frame side of the flow: one frame's Ks cells with the recurrent state carried by the caller. The reverse cell of the
// samplers and of SeqGlow.invert (rev_fast_cell), the forward cell of a teacher-forced frame (fwd_chain_cell), the one-launch chains
// over them (reverse, forward, both at once row by row, and the reverse chain over N candidates per row), the persistent reverse walk, and every entry point a sampler or a
// streaming session calls. Nothing here is reached by the training step: that side is lfi_flow.hip, and what the two share - the
// cell's structs and carves, the generic cell bodies, the register-resident cell's phases, the hand-off primitives, fill_flow and
// the switch readers - is lfi_flow_cells.h.
#include "lfi_flow_cells.h"

namespace {

template <bool REVERSE>
__global__ __launch_bounds__(NT) void flow_step_kernel(FlowK f, CellIO io) {
  if (REVERSE) cell_reverse(f, io, blockIdx.x * MB);
  else cell_forward(f, io, blockIdx.x * MB);
}

// FlowStep.reverse_flow (glow/models.py:345-373) with explicit state, register-resident weights: the sampler's and
// SeqGlow.invert's cell. coupling^-1 -> invconv^-1 (W^-1 image) -> actnorm^-1.
// wait_flag / pub_flag: hand-off words of the per-frame reverse chain (flow_rev_chain_kernel), or null for a stand-alone launch:
// the input tile is then read with sc1 loads after the producer's progress word is seen, and the output tile is stored sc1,
// drained and published (the hand-off of the persistent walks).
// need / pub_value: the progress value waited for / published (1 for the one-frame chain; timestep + 1 in the persistent reverse
// walk). false = the wait was abandoned (abort word set): nothing was computed.
// XW (with X3): the weights come as the fp16 fragment images lfi_flow_prep left (FlowK.hwz ..): no f32 fragments, no split here.
// NLL (the chain of a sampler that reports its frames' likelihood): the rows' running log-density log p(z) - sum of the reverse
// coupling log-dets so far travels with the tile. q_in: one float per row from step k + 1, handed over as the tile is (null: this
// cell starts it from the prior term of the noise tile it stages); q_out: where this cell leaves it - sc1 stores in front of the
// publish - or, q_last, the finished -(q + logdet_const) / ln 2 of the frame in bits. One writer per word, k descending: a fixed
// summation order. Not NLL: none of it is compiled.
// RM (flow_rows_chain_kernel): a row-masked cell. Everything it leaves in memory - h_out / c_out, its output tile or the frame row, the
// hand-over q or the NLL word - is stored only for the tile's rows whose role word (io.role) is io.role_want; the other rows still
// pass through the products (see that kernel) and are dropped. Not RM: none of it is compiled.
// CD (flow_cand_chain_kernel): a candidate cell. io.rows counts VIRTUAL rows, `ncand` per session row; virtual row v reads h_prev,
// c_prev and gic from row v / ncand of the session's arrays (io.h_prev / io.c_prev / io.gic are the parents') and stores everything
// at row v of its own. The division is made once per thread where those loads are requested, in front of the wait. Not CD: none of
// it is compiled.
template <int NG, bool X3 = false, bool XW = false, bool NLL = false, bool RM = false, bool CD = false>
__device__ __forceinline__ bool rev_fast_cell(const FlowK& f, const CellIO& io, int b0, const unsigned* wait_flag,
                                              unsigned* abort_w, unsigned* pub_flag, int* s_ok, unsigned need = 1u,
                                              unsigned pub_value = 1u, const float* q_in = nullptr, float* q_out = nullptr,
                                              bool q_last = false, int ncand = 1) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kq = lane >> 4;
  const int ri = tid >> 5, cl = tid & 31;
  const int k = io.k, rows = io.rows;
  const int C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const CarveF cv = carve_fast_fwd(C, C16, H16, Ch16, Cout);
  float* Yt = flow_smem + cv.At;   // y = [z1 | z2] k-major for the W^-1 product
  float* Ht = flow_smem + cv.Ht;
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  const int ldy = C + 1, ldo = Cout + 1;
  const int nbC = C16 >> 4, nbZ = Ch16 >> 4, nbH = H16 >> 4;
  const bool t1 = wave * 16 < C, t2 = wave * 16 < H, t3 = wave * 16 < Cout;
  const int tcol = wave * 16 + l15;
  unsigned live = 0u;
  if constexpr (RM) live = tile_live_rows(io.role, io.role_want, b0, rows);
  // phase stamps of the stamping workgroup (flow step LFI_STAMP_K, tile 0): s_memtime at the phase boundaries (tools/rev_stamps.py)
#define REV_STAMP(slot)                                                                                                  \
  do {                                                                                                                   \
    if (f.stamps && io.stamp_base > 0 && tid == 0 && b0 == 0 && k == f.stamp_k)                                           \
      f.stamps[io.stamp_base - 1 + (slot)] = __builtin_amdgcn_s_memtime();                                               \
  } while (0)
  REV_STAMP(0);
  static_assert(!XW || X3, "pre-split weight images are the X3 cell's");
  f32x4 wz[XW ? 1 : NG][XW ? 1 : FB_Z], wh[XW ? 1 : NG][XW ? 1 : FB_H], w3[XW ? 1 : FB_H];
  X3FragH wzx[X3 ? NG : 1][FB_Z / 2];            // three fp16 products (fp32-grade, x3h_*): the z1-side fragments
  X3FragH whx[XW ? NG : 1][XW ? FB_H / 2 : 1];   // XW: the h-side fragments too (otherwise split where they are used)
  X3FragH w3x[X3 ? FB_H / 2 : 1], w1x[X3 ? FB_C / 2 : 1];
  // this lane's entries of a pre-split image of flow step k: nb2 32-k blocks of the 16-column tile at `col` (row pitch J entries)
  auto load_x3h = [&](X3FragH* w, int maxb2, const uint4* img, int K16, int J, int col, int nb2, bool on) {
    const long per = (long)(K16 >> 5) * 4 * J;
    const uint4* p = img + (long)k * 2 * per + (long)kq * J + col;
#pragma unroll
    for (int b = 0; b < maxb2; ++b)
      if (on && b < nb2) {
        w[b].hi = __builtin_bit_cast(fh16x8, p[(long)b * 4 * J]);
        w[b].lo = __builtin_bit_cast(fh16x8, p[(long)b * 4 * J + per]);
      } else {
        w[b].hi = (fh16x8)(_Float16)0.0f;
        w[b].lo = (fh16x8)(_Float16)0.0f;
      }
  };
  float hv[XW ? FB_H / 2 : 1];   // XW: this thread's elements of h_prev (row ri, columns cl + 32 q), staged to LDS further down
  if constexpr (XW) {
    // Vector-memory results come back in issue order: what the work in front of the wait needs first is issued first - h_prev
    // (its LDS image gates the barrier), then the h-side fragments of the product that runs before the wait; the fragments of the
    // phases behind the wait follow and arrive under that product.
    const int row = b0 + ri;
    const int hrow = CD ? row / ncand : row;
#pragma unroll
    for (int q = 0; q < FB_H / 2; ++q) {
      const int j = cl + 32 * q;
      hv[q] = (io.h_prev && row < rows && j < H) ? ld_tile(io.h_prev + (long)hrow * H + j, io.state_l2 == 0) : 0.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) load_x3h(whx[g], FB_H / 2, f.hwh, H16, NG * H16, g * H16 + tcol, nbH >> 1, t2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) load_x3h(wzx[g], FB_Z / 2, f.hwz, Ch16, NG * H16, g * H16 + tcol, nbZ >> 1, t2);
    load_x3h(w3x, FB_H / 2, f.hwfl, H16, Co16, tcol, nbH >> 1, t3);
  } else {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int b = 0; b < FB_Z; ++b) wz[g][b] = zero4;
#pragma unroll
      for (int b = 0; b < FB_H; ++b) wh[g][b] = zero4;
      load_frag<FB_Z>(wz[g], f.pwz + (long)k * Ch16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbZ, t2);
      load_frag<FB_H>(wh[g], f.pwh + (long)k * H16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbH, t2);
    }
    load_frag<FB_H>(w3, f.pwfl + (long)k * H16 * Co16, Co16, tcol, kq, nbH, t3);
  }
  float gc[4][NG], bh[NG], cprev[4];
  {
    const float* bhh = f.p.b_hh + (long)k * G;
    const int jc = tcol < H ? tcol : 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) bh[g] = bhh[g * H + jc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vrow = min(b0 + kq * 4 + r, rows - 1);
      const int row = CD ? vrow / ncand : vrow;
#pragma unroll
      for (int g = 0; g < NG; ++g) gc[r][g] = io.gic[(long)row * G + g * H + jc];
      cprev[r] = (NG == 4 && io.c_prev) ? ld_tile(io.c_prev + (long)row * H + jc, io.state_l2 == 0) : 0.0f;
    }
  }
  // ---- everything that does not depend on the incoming tile runs BEFORE the wait for it (a chain of Ks dependent cells pays
  // whatever follows the wait Ks times per frame; stamps of round 4: staging h_prev, splitting the weight fragments into fp16
  // pieces and the h_prev W_hh half of the recurrent product - 4 of its 5 k-blocks - were 10 k of a cell's 20 k dependent cycles)
  if constexpr (XW) {
#pragma unroll
    for (int q = 0; q < FB_H / 2; ++q) {
      const int j = cl + 32 * q;
      if (j < H16) {
        Ht[j * LT + ri] = hv[q];
        if (j >= H) Hn[j * LT + ri] = 0.0f;
      }
    }
    for (int c = Ch + cl; c < Ch16; c += 32) Zt[c * LT + ri] = 0.0f;
  } else {
    const int row = b0 + ri;
    const int hrow = CD ? row / ncand : row;
    const bool rok = row < rows;
    for (int j = cl; j < H16; j += 32) {
      Ht[j * LT + ri] = (io.h_prev && rok && j < H) ? ld_tile(io.h_prev + (long)hrow * H + j, io.state_l2 == 0) : 0.0f;
      if (j >= H) Hn[j * LT + ri] = 0.0f;
    }
    for (int c = Ch + cl; c < Ch16; c += 32) Zt[c * LT + ri] = 0.0f;
  }
  // W^-1 slice of this wave's 16 output channels: in flight under the coupling net
  f32x4 w1[XW ? 1 : FB_C];
  if constexpr (XW) load_x3h(w1x, FB_C / 2, f.hWinv, C16, C16, tcol, nbC >> 1, t1);
  else load_frag<FB_C>(w1, f.pWinv + (long)k * C16 * C16, C16, tcol, kq, nbC, t1);
  // per-column constants of the phases after the wait (LinearZeros bias / scale, ActNorm^-1 scale / bias): loaded here, not between
  // the barriers of the dependent phases (two L2 round trips per cell each)
  const float flb = tcol < Cout ? f.p.b_fl[(long)k * Cout + tcol] : 0.0f;
  const float fls = tcol < Cout ? expf(3.0f * f.p.l_fl[(long)k * Cout + tcol]) : 0.0f;
  const float an_es = tcol < C ? expf(-f.p.an_logs[(long)k * C + tcol]) : 0.0f;
  const float an_bb = tcol < C ? f.p.an_bias[(long)k * C + tcol] : 0.0f;
  // X3: LinearZeros and W^-1 as three fp16 products too (K = H and K = C: 32 and 16 dependent f32-input MFMAs of 32 cycles
  // otherwise, per cell, after the wait); their weight fragments are split here, before it. Whole pairs of 16-k blocks only.
  // (X3 is only instantiated for shapes with whole pairs everywhere: the launcher checks H16, Ch16 and C16)
  if constexpr (X3 && !XW) {
#pragma unroll
    for (int b = 0; b < FB_H / 2; ++b)
      if (b < (nbH >> 1)) w3x[b] = x3h_pack(w3[2 * b], w3[2 * b + 1]);
#pragma unroll
    for (int b = 0; b < FB_C / 2; ++b)
      if (b < (nbC >> 1)) w1x[b] = x3h_pack(w1[2 * b], w1[2 * b + 1]);
  }
  __syncthreads();
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (t2) {
    const float* hl = Ht + kq * LT + l15;
    if constexpr (XW) {
#pragma unroll
      for (int b = 0; b < FB_H / 2; ++b)
        if (b < ((nbH + 1) >> 1)) {
          const X3FragH a = x3h_a(hl + b * 32 * LT);
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = x3h_mma(a, whx[g][b], ah[g]);
        }
    } else if constexpr (X3) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int b = 0; b < FB_Z / 2; ++b) wzx[g][b] = x3h_pack(wz[g][2 * b], wz[g][2 * b + 1]);
#pragma unroll
      for (int b = 0; b < FB_H / 2; ++b)
        if (b < ((nbH + 1) >> 1)) {
          const X3FragH a = x3h_a(hl + b * 32 * LT);
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = x3h_mma(a, x3h_pack(wh[g][2 * b], wh[g][2 * b + 1]), ah[g]);
        }
    } else {
#pragma unroll
      for (int b = 0; b < FB_H; ++b)
        if (b < nbH) {
          const float* ab = hl + b * 16 * LT;
          const float a0 = ab[0], a1 = ab[4 * LT], a2 = ab[8 * LT], a3 = ab[12 * LT];
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = mfma16(a0, wh[g][b][0], ah[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = mfma16(a1, wh[g][b][1], ah[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = mfma16(a2, wh[g][b][2], ah[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) ah[g] = mfma16(a3, wh[g][b][3], ah[g]);
        }
    }
  }
  if constexpr (XW) {
    // the fragments of the phases AFTER the wait are plain loads now: pin them in front of it (the compiler sinks a load towards its
    // use - behind the wait, where a chain of Ks cells pays its L2 round trip Ks times per frame)
    auto pin = [](X3FragH& w) { asm volatile("" : "+v"(w.hi), "+v"(w.lo)); };
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int b = 0; b < FB_Z / 2; ++b) pin(wzx[g][b]);
#pragma unroll
    for (int b = 0; b < FB_H / 2; ++b) pin(w3x[b]);
#pragma unroll
    for (int b = 0; b < FB_C / 2; ++b) pin(w1x[b]);
  }
  REV_STAMP(1);
  if (wait_flag && !pipe_acquire(wait_flag, need, abort_w, tid, s_ok, false)) return false;
  REV_STAMP(2);
  // ---- R0: stage the tile [z1 | z2']
  float q = 0.0f;   // NLL: lane cl == 0 carries its row's running log-density; the first cell's lanes their parts of sum z^2
  {
    const int row = b0 + ri;
    const bool rok = row < rows;
    if constexpr (NLL) {
      if (q_in && cl == 0 && rok) q = ld_tile(q_in + row, false);   // (in flight under the cell: needed in R3)
    }
    for (int c = cl; c < C16; c += 32) {
      const float v = (c < C && rok) ? ld_tile(io.x_in + (long)row * io.ldx + c, wait_flag == nullptr) : 0.0f;
      if constexpr (NLL) {
        if (!q_in) q += v * v;
      }
      if (c < C) Yrm[ri * ldy + c] = v;
      if (c < Ch) Zt[c * LT + ri] = v;
      if (c < Ch || c >= C) Yt[c * LT + ri] = v;   // z1 rows and the zero k padding; z2 rows come from R3
    }
  }
  __syncthreads();
  REV_STAMP(3);
  if (t2) {   // the z1 half of the product (one k-block at C <= 64), then the gate math
    const float* zl = Zt + kq * LT + l15;
    if constexpr (X3) {
#pragma unroll
      for (int b = 0; b < FB_Z / 2; ++b)
        if (b < ((nbZ + 1) >> 1)) {
          const X3FragH a = x3h_a(zl + b * 32 * LT);
#pragma unroll
          for (int g = 0; g < NG; ++g) az[g] = x3h_mma(a, wzx[g][b], az[g]);
        }
    } else {
#pragma unroll
      for (int b = 0; b < FB_Z; ++b)
        if (b < nbZ) {
          const float* ab = zl + b * 16 * LT;
          const float a0 = ab[0], a1 = ab[4 * LT], a2 = ab[8 * LT], a3 = ab[12 * LT];
#pragma unroll
          for (int g = 0; g < NG; ++g) az[g] = mfma16(a0, wz[g][b][0], az[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) az[g] = mfma16(a1, wz[g][b][1], az[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) az[g] = mfma16(a2, wz[g][b][2], az[g]);
#pragma unroll
          for (int g = 0; g < NG; ++g) az[g] = mfma16(a3, wz[g][b][3], az[g]);
        }
    }
    fast_cell_p2_gates<NG, RM>(f, Ht, Hn, az, ah, gc, bh, cprev, tcol, kq, b0, rows, io.h_out, io.c_out, nullptr, nullptr, nullptr, nullptr,
                               0, 0, live);
  }
  __syncthreads();
  REV_STAMP(4);
  if (t3) {
    if constexpr (X3) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* hl = Hn + kq * LT + l15;
#pragma unroll
      for (int b = 0; b < FB_H / 2; ++b)
        if (b < (nbH >> 1)) acc = x3h_mma(x3h_a(hl + b * 32 * LT), w3x[b], acc);
      if (tcol < Cout) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Orm[(kq * 4 + r) * ldo + tcol] = (acc[r] + flb) * fls;
      }
    } else {
      fast_cell_p3(f, k, Hn, Orm, w3, nbH, tcol, kq, l15, b0, rows, nullptr, 0, flb, fls);
    }
  }
  __syncthreads();
  REV_STAMP(5);
  // ---- R3: coupling inverse (glow/models.py:356-365)
  {
    const int row = b0 + ri;
    const bool rs = RM ? ((live >> ri) & 1u) != 0u : row < rows;
    float lg = 0.0f;
    if (cl < C2) {
      const float z2n = Yrm[ri * ldy + Ch + cl];
      float z2;
      if (f.affine) {
        const float shift = Orm[ri * ldo + 2 * cl];
        const float sraw = sigmoidf_(Orm[ri * ldo + 2 * cl + 1] + 2.0f);
        const float sc = fmaxf(sraw, f.eps);
        z2 = z2n / sc;
        z2 = z2 - shift;
        lg = -logf(sc);
      } else {
        z2 = z2n - Orm[ri * ldo + cl];
      }
      Yt[(Ch + cl) * LT + ri] = z2;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) lg += __shfl_xor(lg, o, 64);
    if (cl == 0 && rs && io.l_out) {
      if (io.l_accumulate) io.l_out[row] += lg; else io.l_out[row] = lg;
    }
    if constexpr (NLL) {
      if (!q_in) {   // log p(z) of the prior draw: sum_c -0.5 (z_c^2 + log 2 pi)
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        q = -0.5f * (q + (float)C * LOG2PI_F);
      }
      if (cl == 0 && rs) {
        q -= lg;   // forward log-det of this step's coupling = -lg
        if (q_last) q_out[row] = -(q + f.ldconst[0]) / LN2_F;
        else st_sc1(q_out + row, q);
      }
    }
  }
  __syncthreads();
  REV_STAMP(6);
  // ---- R4: x = (y W^-1) exp(-logs) - bias   (scale then center, glow/modules.py:76-79)
  if (t1) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (X3) {
      const float* yl = Yt + kq * LT + l15;
#pragma unroll
      for (int b = 0; b < FB_C / 2; ++b)
        if (b < (nbC >> 1)) acc = x3h_mma(x3h_a(yl + b * 32 * LT), w1x[b], acc);
    } else {
      acc = mma16_reg<FB_C>(Yt + kq * LT + l15, w1, nbC);
    }
    const int c = tcol;
    if (c < C) {
      const float es = an_es, bb = an_bb;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + kq * 4 + r;
        if (RM ? ((live >> (kq * 4 + r)) & 1u) != 0u : row < rows) {
          if (pub_flag) st_sc1(io.x_out + (long)row * io.ldxo + c, acc[r] * es - bb);
          else io.x_out[(long)row * io.ldxo + c] = acc[r] * es - bb;
        }
      }
    }
  }
  REV_STAMP(7);
  if (pub_flag) pipe_publish(pub_flag, pub_value, tid, true);
  REV_STAMP(8);
#undef REV_STAMP
  return true;
}

template <int NG>
__global__ __launch_bounds__(NT) void flow_step_rev_fast_kernel(FlowK f, CellIO io) {
  rev_fast_cell<NG>(f, io, blockIdx.x * MB, nullptr, nullptr, nullptr, nullptr);
}

// One generated frame of the sampler: all Ks reverse flow steps of all batch tiles in ONE launch instead of Ks launches of
// B / 16 workgroups each (64 of 256 CUs at batch 1024, 270 KB of weights fetched behind every launch boundary). Workgroup
// (k, tile) - ids by ticket, k descending, so a workgroup only waits on one that already runs - requests its weights, its
// part of gic and its recurrent state, then waits for the tile of step k + 1 (the prior noise for k = Ks - 1), runs the
// cell and hands its tile to step k - 1 (step 0 writes the frame). Tiles of one sample block chain strictly, so the two
// ping-pong tile buffers of the per-step launches still do.
struct RevChain {
  const float* noise;     // B x C prior draws of this frame
  float *xa, *xb;         // B x C tile buffers: step k writes (k & 1) ? xa : xb
  float* frame; long ld_frame;   // output rows of this frame in faces (row stride seq_len * C)
  const float* gic;       // [Ks][B][G]
  float *h, *cstate;      // [Ks][B][H] recurrent state, updated in place
  int has_prev;           // 0 at the first generated frame (zero state)
  int frame_no;           // index of the generated frame (diagnostic phase stamps of frames < 128 only)
  unsigned* pipe;         // ticket, abort, progress words (zeroed before every launch)
  // round 5: step 0's workgroups also leave the NEXT frame's window as the fp16 fragments the fused conditioning kernel reads
  // (lfi_sample.hip, sc_xfrag_kernel's format: tile bt, step m, plane: lane l, element e = window[16 bt + (l & 15)][32 m + 8 (l >> 4) + e])
  // - one launch per generated frame less; null: the conditioning call makes them itself
  _Float16* xf;
  const float* faces;     // row 0 of the frames buffer (row pitch ld_frame)
  long xf_off;            // first window column of the next frame in a row: (t + 1 - hist1) * C
  int K1, NM1;
  // NLL instantiations only: the rows' running log-density crosses the chain beside the tile (rev_fast_cell)
  float *qa, *qb;         // B floats each: step k writes (k & 1) ? qa : qb, as the tiles ping-pong
  float* nll;             // B floats: this frame's NLL in bits, written by step 0
};
template <int NG, bool X3, bool XW = false, bool NLL = false>
__global__ __launch_bounds__(NT) void flow_rev_chain_kernel(FlowK f, RevChain rc) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(rc.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int kk = s_id / nbt, bt = s_id - kk * nbt;
  if (kk >= f.Ks) return;
  const int k = f.Ks - 1 - kk;
  unsigned* prog = rc.pipe + PIPE_HDR;
  CellIO io = {};
  io.k = k; io.rows = f.B;
  if (k == f.Ks - 1) { io.x_in = rc.noise; io.ldx = f.C; }
  else { io.x_in = ((k + 1) & 1) ? rc.xa : rc.xb; io.ldx = f.C; }
  if (k == 0) { io.x_out = rc.frame; io.ldxo = rc.ld_frame; }
  else { io.x_out = (k & 1) ? rc.xa : rc.xb; io.ldxo = f.C; }
  io.h_prev = rc.has_prev ? rc.h + (long)k * f.B * f.H : nullptr;
  io.h_out = rc.h + (long)k * f.B * f.H;
  if (NG == 4) { io.c_prev = rc.has_prev ? rc.cstate + (long)k * f.B * f.H : nullptr; io.c_out = rc.cstate + (long)k * f.B * f.H; }
  io.gic = rc.gic + (long)k * f.B * f.G;
  io.stamp_base = rc.frame_no < 128 ? 1024 + 16 * rc.frame_no + 1 : 0;
  if constexpr (NLL)
    rev_fast_cell<NG, X3, XW, true>(f, io, bt * MB, k + 1 < f.Ks ? prog + (k + 1) * nbt + bt : nullptr, rc.pipe + 1,
                                    k > 0 ? prog + k * nbt + bt : nullptr, &s_ok, 1u, 1u,
                                    k + 1 < f.Ks ? (((k + 1) & 1) ? rc.qa : rc.qb) : nullptr,
                                    k == 0 ? rc.nll : ((k & 1) ? rc.qa : rc.qb), k == 0);
  else
  rev_fast_cell<NG, X3, XW>(f, io, bt * MB, k + 1 < f.Ks ? prog + (k + 1) * nbt + bt : nullptr, rc.pipe + 1,
                    k > 0 ? prog + k * nbt + bt : nullptr, &s_ok);
  if (k == 0 && ld_agent(rc.pipe + 1) != 0u) {   // an abandoned chain must not pass for a frame
    const int row = bt * MB + (int)(threadIdx.x >> 5);
    if (row < f.B)
      for (int c = threadIdx.x & 31; c < f.C; c += 32) rc.frame[(long)row * rc.ld_frame + c] = __builtin_nanf("");
    if constexpr (NLL) {   // (the thread that wrote the row's word in R3, if the cell got that far)
      if (row < f.B && (threadIdx.x & 31) == 0) rc.nll[row] = __builtin_nanf("");
    }
  }
  if (k == 0 && rc.xf) {
    // the frame's rows of this tile are on their way to memory: drain, meet, then read the window back past the L1 (agent scope)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    typedef _Float16 xh8 __attribute__((ext_vector_type(8)));
    for (int it = threadIdx.x; it < rc.NM1 * 64; it += NT) {
      const int l = it & 63, m = it >> 6;
      const int row = bt * MB + (l & 15), kk0 = 32 * m + 8 * (l >> 4);
      xh8 hi, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = 0.0f;
        if (row < f.B && kk0 + e < rc.K1) v = ld_tile(rc.faces + (long)row * rc.ld_frame + rc.xf_off + kk0 + e, false);
        const _Float16 h = (_Float16)v;
        hi[e] = h;
        lo[e] = (_Float16)(v - (float)h);
      }
      _Float16* dst = rc.xf + ((long)(bt * rc.NM1 + m) * 2) * 512 + l * 8;
      *reinterpret_cast<xh8*>(dst) = hi;
      *reinterpret_cast<xh8*>(dst + 512) = lo;
    }
  }
}

// N CANDIDATES of one generated frame per session row (SampleStream.step_candidates): flow_rev_chain_kernel over V = B * ncand virtual
// rows, always with the NLL hand-over. Virtual row v is candidate v % ncand of session row v / ncand: it takes its own prior draw
// (noise, V x C) and reads gic and the incoming h / c of its PARENT row in place (the CD cell) - within one frame the candidates of a
// row share their conditioning and their recurrent state, so nothing of the session's is copied V-fold and nothing of it is written.
// What a candidate leaves goes to areas of its own: its frame to `frames` (V x C), its NLL word to nll[v], its new state to
// ch / cc ([Ks][V][H]); lfi_stream_commit_cand installs the chosen one. Ks * ceil(V / 16) workgroups, ids by ticket, k descending; the
// ticket and progress words are sized for V. Rows of one tile may belong to different parents - rows never mix inside a cell.
struct CandChain {
  const float* noise;     // V x C prior draws
  float *xa, *xb;         // V x C tile buffers: step k writes (k & 1) ? xa : xb
  float* frames;          // V x C: the candidates' frames
  const float* gic;       // [Ks][B][G], the parents'
  const float *h, *cstate;   // [Ks][B][H], the parents' state: read only
  float *ch, *cc;         // [Ks][V][H]: the candidates' new state
  int has_prev;           // 0 at the first frame of a session (zero state: h / cstate are not read)
  int V, ncand, nbt;      // nbt = ceil(V / 16)
  unsigned* pipe;         // ticket, abort, progress words (zeroed before every launch)
  float *qa, *qb;         // V floats each: the log-density hand-over
  float* nll;             // V floats
};
template <int NG, bool X3, bool XW>
__global__ __launch_bounds__(NT) void flow_cand_chain_kernel(FlowK f, CandChain rc) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(rc.pipe, 1u);
  __syncthreads();
  const int nbt = rc.nbt, V = rc.V;
  const int kk = s_id / nbt, bt = s_id - kk * nbt;
  if (kk >= f.Ks) return;
  const int k = f.Ks - 1 - kk;
  unsigned* prog = rc.pipe + PIPE_HDR;
  CellIO io = {};
  io.k = k; io.rows = V; io.ldx = f.C; io.ldxo = f.C;
  io.x_in = (k == f.Ks - 1) ? rc.noise : (((k + 1) & 1) ? rc.xa : rc.xb);
  io.x_out = (k == 0) ? rc.frames : ((k & 1) ? rc.xa : rc.xb);
  io.h_prev = rc.has_prev ? rc.h + (long)k * f.B * f.H : nullptr;
  io.h_out = rc.ch + (long)k * V * f.H;
  if (NG == 4) { io.c_prev = rc.has_prev ? rc.cstate + (long)k * f.B * f.H : nullptr; io.c_out = rc.cc + (long)k * V * f.H; }
  io.gic = rc.gic + (long)k * f.B * f.G;
  rev_fast_cell<NG, X3, XW, true, false, true>(f, io, bt * MB, k + 1 < f.Ks ? prog + (k + 1) * nbt + bt : nullptr, rc.pipe + 1,
                                               k > 0 ? prog + k * nbt + bt : nullptr, &s_ok, 1u, 1u,
                                               k + 1 < f.Ks ? (((k + 1) & 1) ? rc.qa : rc.qb) : nullptr,
                                               k == 0 ? rc.nll : ((k & 1) ? rc.qa : rc.qb), k == 0, rc.ncand);
  if (k == 0 && ld_agent(rc.pipe + 1) != 0u) {   // an abandoned chain must not pass for candidates
    const int row = bt * MB + (int)(threadIdx.x >> 5);
    if (row < V) {
      for (int c = threadIdx.x & 31; c < f.C; c += 32) rc.frames[(long)row * f.C + c] = __builtin_nanf("");
      if ((threadIdx.x & 31) == 0) rc.nll[row] = __builtin_nanf("");
    }
  }
}

// The candidates on the per-step launches (shapes outside the register-resident cells, LFI_SAMPLE_CHAIN=0, LFI_FLOW_GENERIC=1): the
// parents' gic and incoming state broadcast to V rows, which the existing cells then advance in place. Workgroup (v, k).
__global__ __launch_bounds__(256) void cand_gather_kernel(const float* __restrict__ gic, const float* __restrict__ h,
                                                          const float* __restrict__ cstate, int B, int V, int ncand, int G, int H,
                                                          int has_prev, float* __restrict__ gicv, float* __restrict__ ch,
                                                          float* __restrict__ cc) {
  const int v = blockIdx.x, k = blockIdx.y;
  const long b = v / ncand;
  const float* g = gic + ((long)k * B + b) * G;
  float* gv = gicv + ((long)k * V + v) * G;
  for (int j = threadIdx.x; j < G; j += 256) gv[j] = g[j];
  if (!has_prev) return;
  const long src = ((long)k * B + b) * H, dst = ((long)k * V + v) * H;
  for (int j = threadIdx.x; j < H; j += 256) {
    ch[dst + j] = h[src + j];
    if (cstate) cc[dst + j] = cstate[src + j];
  }
}

// ------------------------------------------------------------------------------------------- forward chain (teacher-forced frame)
// (the cell itself, fwd_chain_cell, is in lfi_flow_cells.h: lfi_flow_chunk.hip runs it too)
// One OBSERVED frame of a streaming session (SampleStream.observe): all Ks forward flow steps of all batch tiles in ONE launch, the
// forward twin of flow_rev_chain_kernel. Workgroup (k, tile) - ids by ticket, k ASCENDING, so a workgroup only waits on one that
// already runs - requests its weights, its part of gic and its recurrent state, then waits for the tile of step k - 1 (the observed
// frame itself for k = 0), runs the cell and hands its tile and the rows' running log-det to step k + 1; step Ks - 1 writes z (if
// wanted) and the frame's NLL. Tiles of one sample block chain strictly, so two ping-pong buffers do.
struct FwdChain {
  const float* frame; long ld_frame;   // the observed frame's rows in faces (row stride seq_len * C)
  float *xa, *xb;         // B x C tile buffers: step k writes (k & 1) ? xa : xb
  const float* gic;       // [Ks][B][G]
  float *h, *cstate;      // [Ks][B][H] recurrent state, updated in place
  int has_prev;           // 0 at the first frame of a sequence (zero state)
  unsigned* pipe;         // ticket, abort, progress words (zeroed before every launch)
  float *qa, *qb;         // B floats each: step k writes (k & 1) ? qa : qb, as the tiles ping-pong
  float* z;               // B x C: the frame's latent, or null
  float* nll;             // B floats: the frame's NLL in bits, written by step Ks - 1
};
template <int NG, bool X3>
__global__ __launch_bounds__(NT) void flow_fwd_chain_kernel(FlowK f, FwdChain fc) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(fc.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int k = s_id / nbt, bt = s_id - k * nbt;
  if (k >= f.Ks) return;
  const bool last = k == f.Ks - 1;
  unsigned* prog = fc.pipe + PIPE_HDR;
  CellIO io = {};
  io.k = k; io.rows = f.B;
  if (k == 0) { io.x_in = fc.frame; io.ldx = fc.ld_frame; }
  else { io.x_in = ((k - 1) & 1) ? fc.xa : fc.xb; io.ldx = f.C; }
  io.x_out = last ? fc.z : ((k & 1) ? fc.xa : fc.xb); io.ldxo = f.C;
  io.h_prev = fc.has_prev ? fc.h + (long)k * f.B * f.H : nullptr;
  io.h_out = fc.h + (long)k * f.B * f.H;
  if (NG == 4) { io.c_prev = fc.has_prev ? fc.cstate + (long)k * f.B * f.H : nullptr; io.c_out = fc.cstate + (long)k * f.B * f.H; }
  io.gic = fc.gic + (long)k * f.B * f.G;
  fwd_chain_cell<NG, X3>(f, io, bt * MB, k > 0 ? prog + (k - 1) * nbt + bt : nullptr, fc.pipe + 1, last ? nullptr : prog + k * nbt + bt,
                         &s_ok, k > 0 ? (((k - 1) & 1) ? fc.qa : fc.qb) : nullptr, (k & 1) ? fc.qa : fc.qb, last ? fc.nll : nullptr);
  if (last && ld_agent(fc.pipe + 1) != 0u) {   // an abandoned chain must not pass for a likelihood
    const int row = bt * MB + (int)(threadIdx.x >> 5);
    if (row < f.B) {
      if (fc.z)
        for (int c = threadIdx.x & 31; c < f.C; c += 32) fc.z[(long)row * f.C + c] = __builtin_nanf("");
      if ((threadIdx.x & 31) == 0) fc.nll[row] = __builtin_nanf("");   // (the thread that wrote the row's word in F4, if the cell got that far)
    }
  }
}

// One frame of a streaming session in which every batch row either GENERATES or OBSERVES (SampleStream.step_rows): both chains above in
// ONE launch of 2 Ks nbt workgroups, ids by ticket. Tickets [0, Ks nbt) are flow_rev_chain_kernel's roles (k descending, the NLL
// hand-over), tickets [Ks nbt, 2 Ks nbt) flow_fwd_chain_kernel's (k ascending). A workgroup waits only on one of its OWN direction with
// a lower ticket - there is no wait across the directions - so, as in both chains, it only waits on a workgroup that already runs and
// any number of resident workgroups makes progress. Each direction has its own ping-pong tiles, log-density hand-over and progress
// words (the reverse's at pipe[PIPE_HDR ..], the forward's Ks nbt words behind them); the ticket and the abort word are shared.
//
// role: one word per batch row, != 0 = the row observes (its frame is in `faces` already), 0 = it generates (from its noise row). Both
// directions run the cell on whole 16-row tiles with row-masked stores (RM): a tile's rows of the other role still flow through its
// MFMAs, but row i of the A operand only ever reaches row i of D, every reduction of the cells is along one row, and the elementwise
// phases are per element - so what such a row holds, NaN included, stays in its row and is never stored. One consequence: a forward
// workgroup may read h_prev / c_prev or the frame slot of a GENERATING row while the reverse workgroup of that tile writes it (and a
// reverse workgroup the state of an observing row while the forward one writes it): that value feeds only the row that is dropped.
// Rows of its own role a workgroup reads are written by nobody else in this launch.
//
// A workgroup whose tile has no row of its direction leaves at once, before it requests any weights: all Ks workgroups of that
// (direction, tile) read the same 16 role words and decide alike, so nobody waits on one that left. A caller that keeps generating and
// observing rows in separate tiles pays for each tile once.
struct RowsChain {
  RevChain rev;       // the generating rows' chain (xf = null: the conditioning makes the next window's fragments itself); rev.pipe: the shared words
  FwdChain fwd;       // the observing rows' chain (z = null)
  const int* role;    // B words
};
template <int NG, bool X3R, bool XW, bool X3F>
__global__ __launch_bounds__(NT) void flow_rows_chain_kernel(FlowK f, RowsChain rc) {
  __shared__ int s_id, s_ok;
  unsigned* pipe = rc.rev.pipe;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt, per = f.Ks * nbt;
  const int dir = s_id / per;
  if (dir >= 2) return;
  const int id = s_id - dir * per;
  const int kk = id / nbt, bt = id - kk * nbt;
  if (tile_live_rows(rc.role, dir, bt * MB, f.B) == 0u) return;   // (uniform: no row of this direction in the tile)
  unsigned* prog = pipe + PIPE_HDR + dir * per;
  const int row = bt * MB + (int)(threadIdx.x >> 5);
  CellIO io = {};
  io.rows = f.B; io.role = rc.role; io.role_want = dir;
  if (dir == 0) {
    const RevChain& r = rc.rev;
    const int k = f.Ks - 1 - kk;
    io.k = k;
    if (k == f.Ks - 1) { io.x_in = r.noise; io.ldx = f.C; }
    else { io.x_in = ((k + 1) & 1) ? r.xa : r.xb; io.ldx = f.C; }
    if (k == 0) { io.x_out = r.frame; io.ldxo = r.ld_frame; }
    else { io.x_out = (k & 1) ? r.xa : r.xb; io.ldxo = f.C; }
    io.h_prev = r.has_prev ? r.h + (long)k * f.B * f.H : nullptr;
    io.h_out = r.h + (long)k * f.B * f.H;
    if (NG == 4) { io.c_prev = r.has_prev ? r.cstate + (long)k * f.B * f.H : nullptr; io.c_out = r.cstate + (long)k * f.B * f.H; }
    io.gic = r.gic + (long)k * f.B * f.G;
    rev_fast_cell<NG, X3R, XW, true, true>(f, io, bt * MB, k + 1 < f.Ks ? prog + (k + 1) * nbt + bt : nullptr, pipe + 1,
                                           k > 0 ? prog + k * nbt + bt : nullptr, &s_ok, 1u, 1u,
                                           k + 1 < f.Ks ? (((k + 1) & 1) ? r.qa : r.qb) : nullptr,
                                           k == 0 ? r.nll : ((k & 1) ? r.qa : r.qb), k == 0);
    if (k == 0 && ld_agent(pipe + 1) != 0u) {   // an abandoned chain must not pass for a frame
      if (row < f.B && rc.role[row] == 0) {
        for (int c = threadIdx.x & 31; c < f.C; c += 32) r.frame[(long)row * r.ld_frame + c] = __builtin_nanf("");
        if ((threadIdx.x & 31) == 0) r.nll[row] = __builtin_nanf("");
      }
    }
  } else {
    const FwdChain& w = rc.fwd;
    const int k = kk;
    const bool last = k == f.Ks - 1;
    io.k = k;
    if (k == 0) { io.x_in = w.frame; io.ldx = w.ld_frame; }
    else { io.x_in = ((k - 1) & 1) ? w.xa : w.xb; io.ldx = f.C; }
    io.x_out = last ? nullptr : ((k & 1) ? w.xa : w.xb); io.ldxo = f.C;
    io.h_prev = w.has_prev ? w.h + (long)k * f.B * f.H : nullptr;
    io.h_out = w.h + (long)k * f.B * f.H;
    if (NG == 4) { io.c_prev = w.has_prev ? w.cstate + (long)k * f.B * f.H : nullptr; io.c_out = w.cstate + (long)k * f.B * f.H; }
    io.gic = w.gic + (long)k * f.B * f.G;
    fwd_chain_cell<NG, X3F, true>(f, io, bt * MB, k > 0 ? prog + (k - 1) * nbt + bt : nullptr, pipe + 1, last ? nullptr : prog + k * nbt + bt,
                                  &s_ok, k > 0 ? (((k - 1) & 1) ? w.qa : w.qb) : nullptr, (k & 1) ? w.qa : w.qb, last ? w.nll : nullptr);
    if (last && ld_agent(pipe + 1) != 0u) {   // an abandoned chain must not pass for a likelihood
      if (row < f.B && rc.role[row] != 0 && (threadIdx.x & 31) == 0) w.nll[row] = __builtin_nanf("");
    }
  }
}

// SeqGlow.invert (glow/models.py:617-645): the teacher-forced reverse pass over ALL timesteps in ONE launch - the reverse twin of the
// persistent forward walk. Workgroup (k, tile), ids by ticket with k descending, walks n = 0 .. N-1: it waits for step k + 1's tile
// of timestep n (the latent z_n for k = Ks - 1), runs the reverse cell with its recurrent state carried in h / cstate (its own
// rows, updated in place) and hands its tile to step k - 1 (step 0 writes x_n). Every (n, k) tile has its own slot in `tiles`, so a
// fast producer never overwrites what its consumer has not read and more workgroups than CUs just run as successive groups. The
// coupling log-det of every (k, n, row) goes to its own word of `ldk` (workgroups on different CUs must not read-modify-write one
// accumulator between kernel boundaries); the host call sums them over k.
struct RevWalk {
  const float* z;       // [N][B][C]
  float* tiles;         // [Ks][N * B][C]
  float* out;           // [N][B][C]
  const float* gic;     // [Ks][N * B][G]
  float *h, *cstate;    // [Ks][B][H]
  float* ldk;           // [Ks][N * B]
  unsigned* pipe;       // ticket, abort, 2 reserved, then one progress word per (k, tile): timesteps published
};
template <int NG>
__global__ __launch_bounds__(NT) void flow_rev_walk_kernel(FlowK f, RevWalk rw) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(rw.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int kk = s_id / nbt, bt = s_id - kk * nbt;
  if (kk >= f.Ks) return;
  const int k = f.Ks - 1 - kk;
  unsigned* prog = rw.pipe + PIPE_HDR;
  const long F = f.F, B = f.B;
  bool ok = true;
  for (int n = 0; n < f.N && ok; ++n) {
    CellIO io = {};
    io.k = k; io.rows = f.B; io.ldx = f.C; io.ldxo = f.C;
    io.x_in = (k == f.Ks - 1) ? rw.z + (long)n * B * f.C : rw.tiles + ((long)(k + 1) * F + (long)n * B) * f.C;
    io.x_out = (k == 0) ? rw.out + (long)n * B * f.C : rw.tiles + ((long)k * F + (long)n * B) * f.C;
    io.h_prev = n > 0 ? rw.h + (long)k * B * f.H : nullptr;
    io.h_out = rw.h + (long)k * B * f.H;
    if (NG == 4) { io.c_prev = n > 0 ? rw.cstate + (long)k * B * f.H : nullptr; io.c_out = rw.cstate + (long)k * B * f.H; }
    io.gic = rw.gic + ((long)k * F + (long)n * B) * f.G;
    io.l_out = rw.ldk + (long)k * F + (long)n * B; io.l_accumulate = 0;
    io.state_l2 = 1;
    io.stamp_base = n < 128 ? 1024 + 16 * n + 1 : 0;
    ok = rev_fast_cell<NG, false>(f, io, bt * MB, k + 1 < f.Ks ? prog + (k + 1) * nbt + bt : nullptr, rw.pipe + 1,
                                  k > 0 ? prog + k * nbt + bt : nullptr, &s_ok, (unsigned)n + 1u, (unsigned)n + 1u);
    __syncthreads();   // the cell's last reads of the LDS operands are done before the next timestep stages its own
  }
  if (k == 0 && ld_agent(rw.pipe + 1) != 0u) {   // an abandoned walk must not pass for a reconstruction
    const int row = bt * MB + (int)(threadIdx.x >> 5);
    if (row < f.B)
      for (int n = 0; n < f.N; ++n)
        for (int c = threadIdx.x & 31; c < f.C; c += 32) rw.out[((long)n * B + row) * f.C + c] = __builtin_nanf("");
  }
}

// ---- which instantiation runs: one picker per kernel family; set_flow_lds and the launch take the pointer
typedef void (*FlowStepKernel)(FlowK, CellIO);
typedef void (*FlowRevWalkKernel)(FlowK, RevWalk);
typedef void (*FlowRevChainKernel)(FlowK, RevChain);
typedef void (*FlowFwdChainKernel)(FlowK, FwdChain);
typedef void (*FlowRowsChainKernel)(FlowK, RowsChain);
typedef void (*FlowCandChainKernel)(FlowK, CandChain);

FlowStepKernel flow_step_rev_pick(bool fast, bool lstm) {
  if (!fast) return flow_step_kernel<true>;
  return lstm ? flow_step_rev_fast_kernel<4> : flow_step_rev_fast_kernel<3>;
}
FlowRevWalkKernel flow_rev_walk_pick(bool lstm) { return lstm ? flow_rev_walk_kernel<4> : flow_rev_walk_kernel<3>; }
// (the chains' forms by the frame plan's bits, FramePlan in lfi_flow_cells.h: x3 / xw the reverse cells', x3f the forward cells'; the
// LSTM cell exact in all)
template <bool NLL>
FlowRevChainKernel flow_rev_chain_pick_(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_rev_chain_kernel<4, false, false, NLL>;
  if (pl.xw) return flow_rev_chain_kernel<3, true, true, NLL>;
  return pl.x3 ? flow_rev_chain_kernel<3, true, false, NLL> : flow_rev_chain_kernel<3, false, false, NLL>;
}
FlowRevChainKernel flow_rev_chain_pick(const FramePlan& pl, bool lstm, bool nll) {
  return nll ? flow_rev_chain_pick_<true>(pl, lstm) : flow_rev_chain_pick_<false>(pl, lstm);
}
FlowCandChainKernel flow_cand_chain_pick(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_cand_chain_kernel<4, false, false>;
  if (pl.xw) return flow_cand_chain_kernel<3, true, true>;
  return pl.x3 ? flow_cand_chain_kernel<3, true, false> : flow_cand_chain_kernel<3, false, false>;
}
FlowFwdChainKernel flow_fwd_chain_pick(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_fwd_chain_kernel<4, false>;
  return pl.x3f ? flow_fwd_chain_kernel<3, true> : flow_fwd_chain_kernel<3, false>;
}
FlowRowsChainKernel flow_rows_chain_pick(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_rows_chain_kernel<4, false, false, false>;
  if (!pl.x3) return flow_rows_chain_kernel<3, false, false, false>;
  if (pl.xw) return pl.x3f ? flow_rows_chain_kernel<3, true, true, true> : flow_rows_chain_kernel<3, true, true, false>;
  return pl.x3f ? flow_rows_chain_kernel<3, true, false, true> : flow_rows_chain_kernel<3, true, false, false>;
}

}  // namespace

// =================================================================================================== C ABI
extern "C" int lfi_flow_step(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, int k, int rows,
                             const float* x_in, long ldx, const float* h_prev, const float* c_prev, const float* gic_k,
                             float* x_out, long ldxo, float* h_out, float* c_out, float* ldc_acc, int reverse, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_step");
  if (rc) return rc;
  LFI_REQUIRE(prep && x_in && gic_k && x_out && h_out, "lfi_flow_step: null pointer");
  LFI_REQUIRE(k >= 0 && k < d->Ks && rows > 0, "lfi_flow_step: bad k/rows");
  LFI_REQUIRE(!d->lstm || c_out, "lfi_flow_step: the LSTM cell needs c_out");
  CellIO io = {};
  io.k = k; io.rows = rows; io.x_in = x_in; io.ldx = ldx; io.h_prev = h_prev; io.gic = gic_k;
  io.c_prev = d->lstm ? c_prev : nullptr; io.c_out = d->lstm ? c_out : nullptr;
  io.x_out = x_out; io.ldxo = ldxo; io.h_out = h_out; io.l_out = ldc_acc; io.l_accumulate = 1;
  const bool fast = reverse && flow_fast_ok(f.C, f.H, f.Cout) && !flow_force_generic();   // (the forward cell has the streaming form only)
  const size_t lds = (size_t)(fast ? carve_fast_fwd(f.C, f.C16, f.H16, f.Ch16, f.Cout).total : carve_fwd(f.C, f.H, f.Ch, f.C2, f.Cout).total) *
                     sizeof(float);
  const FlowStepKernel cell = reverse ? flow_step_rev_pick(fast, f.lstm) : flow_step_kernel<false>;
  if ((rc = set_flow_lds(cell, lds, "lfi_flow_step"))) return rc;
  hipLaunchKernelGGL(cell, dim3(lfi_cdiv(rows, MB)), dim3(NT), lds, (hipStream_t)stream, f, io);
  LFI_LAUNCH_CHECK("lfi_flow_step");
  return LFI_OK;
}

// SeqGlow.invert (glow/models.py:617-645) as ONE persistent launch (flow_rev_walk_kernel) + the sum of the per-step log-dets.
extern "C" int lfi_flow_seq_rev_ok(const lfi_flow_dims* d) {
  if (!d) return 0;
  const int Cout = d->affine ? 2 * (d->C - d->C / 2) : d->C - d->C / 2;
  return (flow_fast_ok(d->C, d->H, Cout) && !flow_force_generic() && lfi_env_on("LFI_INVERT_WALK")) ? 1 : 0;
}

extern "C" long lfi_flow_seq_rev_work_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  const long F = (long)d->N * d->B, tiles = (d->B + MB - 1) / MB;
  return (long)d->Ks * F * d->C + (long)d->Ks * F + lfi_colsum_work_floats(d->Ks, (int)F, 1) +
         (((long)PIPE_HDR + d->Ks * tiles + 3) & ~3L) + 16;
}

extern "C" int lfi_flow_seq_rev(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* z,
                                const float* gic, float* x_out, float* logdet, float* h, float* cstate, float* work,
                                void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_seq_rev");
  if (rc) return rc;
  LFI_REQUIRE(prep && z && gic && x_out && logdet && h && work, "lfi_flow_seq_rev: null pointer");
  LFI_REQUIRE(!d->lstm || cstate, "lfi_flow_seq_rev: the LSTM cell needs cstate");
  LFI_REQUIRE(lfi_flow_seq_rev_ok(d), "lfi_flow_seq_rev: C <= 64, hidden_channels <= 128 only (lfi_flow_seq_rev_ok); wider flows "
              "walk cell by cell with lfi_flow_step");
  LFI_REQUIRE((long)f.N * f.B < (1L << 31), "lfi_flow_seq_rev: too many frames");
  hipStream_t st = (hipStream_t)stream;
  const long F = f.F;
  RevWalk rw = {};
  rw.z = z; rw.gic = gic; rw.out = x_out; rw.h = h; rw.cstate = cstate;
  rw.tiles = work;
  rw.ldk = rw.tiles + (long)f.Ks * F * f.C;
  float* cws = rw.ldk + (long)f.Ks * F;
  rw.pipe = reinterpret_cast<unsigned*>((reinterpret_cast<uintptr_t>(cws + lfi_colsum_work_floats(f.Ks, (int)F, 1)) + 15) & ~(uintptr_t)15);
  const size_t words = (size_t)(((long)PIPE_HDR + (long)f.Ks * f.nbt + 3) & ~3L);
  hipError_t me = hipMemsetAsync(rw.pipe, 0, words * sizeof(unsigned), st);
  LFI_REQUIRE(me == hipSuccess, "lfi_flow_seq_rev: hipMemsetAsync: %s", hipGetErrorString(me));
  const size_t lds = (size_t)carve_fast_fwd(f.C, f.C16, f.H16, f.Ch16, f.Cout).total * sizeof(float);
  const FlowRevWalkKernel walk = flow_rev_walk_pick(f.lstm);
  if ((rc = set_flow_lds(walk, lds, "lfi_flow_seq_rev"))) return rc;
  hipLaunchKernelGGL(walk, dim3(f.Ks * f.nbt), dim3(NT), lds, st, f, rw);
  LFI_LAUNCH_CHECK("lfi_flow_seq_rev");
  // logdet[n][b] = sum over the flow steps of the coupling log-dets (the constant ActNorm / invconv part is the caller's)
  return lfi_colsum_f32(rw.ldk, F, 0, f.Ks, (int)F, 1, logdet, 0, 1.0f, 0, cws, stream);
}

// SeqGlow.inference (glow/models.py:567-596): everything that does not depend on generated frames was hoisted by the
// caller into pre_static; per frame two small GEMMs (window part of cond_transform, then W_ih[:, Ch:] c) and Ks
// reverse cells. The growing torch.cat history of the reference (:591, O(T^2) copies) is a preallocated buffer here.
extern "C" long lfi_flow_sample_p1_work_floats(const lfi_flow_dims* d, const lfi_p1enc* e, int hist1) {
  if (!d || !e || e->kind == 0) return 0;
  const long hid4 = (e->hid + 3) & ~3;
  long n = (long)d->B * hid4 + 16;
  if (e->kind == 2 || e->kind == 3) {
    const int ng = e->kind == 3 ? 4 : 3;
    lfi_enc_desc ed = {};
    ed.B = d->B; ed.T = hist1; ed.N = 1; ed.start = hist1 - 1; ed.hist = hist1; ed.hid = e->hid; ed.lstm = e->kind == 3;
    n += (long)d->B * hist1 * ng * e->hid + lfi_encode_windows_work_floats(&ed) + (long)hist1 * d->B * e->hid;
    if (e->kind == 3) n += (long)hist1 * d->B * 5 * e->hid;   // the LSTM encoder keeps its cell state in the gate stash
  }
  return n;
}

extern "C" long lfi_flow_sample_work_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  const int G = (d->lstm ? 4 : 3) * d->H;
  const long tiles = (d->B + MB - 1) / MB;
  return (long)d->B * d->Ks * d->D + (long)d->Ks * d->B * G + 2L * d->B * d->C + 16
         + (((long)PIPE_HDR + d->Ks * tiles + 3) & ~3L) + 4    // + the hand-off words of the per-frame reverse chain
         + (long)d->B * 64 * ((d->C + 3) & ~3) + 4             // + the aligned copy of the raw prev_p1_face window (hist1 <= 64)
         + lfi_internal_sample_cond_bytes(d->B, d->Ks, G, 512) / 4 + 64;   // + the fused conditioning's fragments (window <= 512 floats)
}

extern "C" int lfi_flow_sample_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct,
                                   long E, int hist1, float* pre_static, const float* noise, float* faces, int seq_len,
                                   int start, int nframes, float* h, float* cstate, const lfi_p1enc* p1, float* p1work,
                                   float* work, void* stream) {
  return lfi_flow_sample_seq_from(d, p, prep, wct, E, hist1, pre_static, noise, faces, seq_len, start, nframes, 0, h, cstate, p1,
                                  p1work, work, stream);
}

// A run of `nframes` generated frames that is NOT the first of its sequence: first_frame = how many frames of the sequence earlier
// calls generated (> 0: the recurrent state in h / cstate is theirs and carries on; pre_static / noise / start are this run's own).
// The engine samples a long sequence as a few such runs so that the static part of run i + 1 (window encoders, the
// non-autoregressive cond_transform columns) can be computed on a second stream under the latency-bound chain of run i.
extern "C" int lfi_flow_sample_seq_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct,
                                        long E, int hist1, float* pre_static, const float* noise, float* faces, int seq_len,
                                        int start, int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1,
                                        float* p1work, float* work, void* stream) {
  return lfi_flow_sample_seq_nll(d, p, prep, wct, E, hist1, pre_static, noise, faces, seq_len, start, nframes, first_frame, h, cstate,
                                 p1, p1work, work, nullptr, nullptr, stream);
}

// The per-frame conditioning front end of the sampler (lfi_flow_sample_seq_nll) and of the teacher-forced scorer
// (lfi_flow_score_seq_from): the carve of `work`, which form the window part of cond_transform + gic takes, and its launches for one
// frame. Both callers run the same launches of the same kernels for a frame.
namespace {
struct SampleFront {
  const lfi_flow_dims* d; const lfi_flow_params* p; const FlowK* f;
  const float* wct; long E; int hist1; float* faces; int seq_len;
  const lfi_p1enc* p1; float* p1work; int p1kind, p1col;
  float *gic, *xa, *xb, *wstage;   // [Ks][B][G]; the chain's B x C ping / pong tiles; the aligned copy of the raw window
  unsigned* chain_state; size_t chain_words;
  int ldw, K1;
  bool stage_win, fused, chain;
  void* cfrags;
};
// `chain`: a one-launch chain follows every frame's conditioning (the fused kernel then clears its ticket / progress words)
// pipe / pipe_words: those words, when they are not the carve's own
int sample_front_setup(SampleFront* s, const lfi_flow_dims* d, const lfi_flow_params* p, const FlowK* f, const float* wct, long E, int hist1,
                       const float* pre_static, float* faces, int seq_len, const lfi_p1enc* p1, float* p1work, float* work, bool chain,
                       int nframes, void* stream, const char* who, unsigned* pipe = nullptr, size_t pipe_words = 0) {
  s->d = d; s->p = p; s->f = f; s->wct = wct; s->E = E; s->hist1 = hist1; s->faces = faces; s->seq_len = seq_len;
  s->p1 = p1; s->p1work = p1work; s->chain = chain;
  s->p1kind = p1 ? p1->kind : 0;
  LFI_REQUIRE(s->p1kind >= 0 && s->p1kind <= 3, "%s: bad p1_face encoder kind %d", who, s->p1kind);
  LFI_REQUIRE(s->p1kind == 0 || (p1work && p1->hid > 0), "%s: encoded p1_face window needs p1work", who);
  s->p1col = p1 ? p1->col : 0;
  const int B = f->B, C = f->C, D = f->D, Ks = f->Ks, G = f->G;
  s->gic = work + (long)B * Ks * D;        // [Ks][B][G]   (the first B x Ks*D floats: round 2's copy of c, unused now)
  s->xa = s->gic + (long)Ks * B * G;       // B x C ping
  s->xb = s->xa + (long)B * C;             // B x C pong
  s->chain_state = reinterpret_cast<unsigned*>((reinterpret_cast<uintptr_t>(s->xb + (long)B * C) + 15) & ~(uintptr_t)15);
  s->chain_words = (size_t)(((long)PIPE_HDR + (long)Ks * f->nbt + 3) & ~3L);
  // raw prev_p1_face windows start (t - hist1) * C floats into a row: 16-byte aligned only on every other frame at C = 50,
  // which sent half of the window products to the exact-f32 kernel (91 vs 35 us). A gather into an aligned buffer first.
  s->wstage = reinterpret_cast<float*>(s->chain_state + s->chain_words);
  // pipe: a chain with more hand-off words than one direction's (flow_rows_chain_kernel) brings its own, and the fused conditioning
  // kernel clears those; everything else of the carve stays where every other caller has it
  if (pipe) { s->chain_state = pipe; s->chain_words = pipe_words; }
  s->ldw = (hist1 * C + 3) & ~3;
  s->stage_win = s->p1kind == 0 && hist1 <= 64;
  // raw window + fp16 pieces (precision 9) + final widths: cond_transform's window part and the coupling cell's input projection
  // as ONE launch per frame, c never written (lfi_sample.hip); the weights' fragments are made here, once per call
  s->K1 = hist1 * C;
  s->fused = s->stage_win && (d->gemm_precision & 0xff) == 9 && lfi_internal_sample_cond_ok(D, G, s->K1) &&
             (reinterpret_cast<uintptr_t>(pre_static) & 15) == 0;
  s->cfrags = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(s->wstage + (long)B * 64 * ((C + 3) & ~3)) + 255) & ~(uintptr_t)255);
  if (s->fused && nframes > 0) return lfi_internal_sample_cond_prepare(wct, E, s->p1col, s->K1, f->wc, Ks, G, s->cfrags, stream);
  return LFI_OK;
}
// The front end's products for M rows of windows - M = B: one frame; M = nframes * B, frame-major: a chunk of frames known up front.
// win: row m's raw prev_p1_face window (hist1 * C floats, row pitch ldwin); cfr: the rows' pre_static (M x Ks D, overwritten with c);
// gic: [Ks][M][G]; p1work: lfi_flow_sample_p1_work_floats for M rows (encoded kinds).
// d, p, p1, wct, E, hist1: the sampler's; wc: the coupling cells' W_ih[:, Ch:] of all steps (FlowK.wc).
}  // namespace
extern "C" int lfi_internal_sample_front_rows(const lfi_flow_dims* d, const lfi_flow_params* p, const lfi_p1enc* p1, const float* wct, long E,
                                              int hist1, const float* wc, int M, const float* win, long ldwin, float* cfr, float* gic,
                                              float* p1work, void* stream) {
  const int C = d->C, D = d->D, Ks = d->Ks, G = (d->lstm ? 4 : 3) * d->H;
  const int p1kind = p1 ? p1->kind : 0, p1col = p1 ? p1->col : 0;
  int rc;
  // c = LeakyReLU(pre_static[n] + window @ Wct[:, :hist1*C]^T), IN PLACE: frame n's rows of pre_static are read by this product
  // alone, so they are its pre-activation addend and its output at once (a 32 MB copy per frame into a separate c otherwise)
  lfi_gemm_desc q = {};
  q.batch = 1; q.M = M; q.N = Ks * D; q.K = hist1 * C;
  q.A = win; q.lda = ldwin; q.a_kcontig = 1;
  q.B = wct + p1col; q.ldb = E; q.b_kcontig = 1;
  q.C = cfr; q.ldc = (long)Ks * D; q.accumulate = 2; q.act = 1; q.slope = 0.01f; q.precision = d->gemm_precision;
  if (p1kind != 0) {
    // features of the window first: e (M x hid4), then c = LeakyReLU(pre_static + e Wct[:, col : col + hid]^T)
    const int hid = p1->hid, hid4 = (hid + 3) & ~3;
    float* ebuf = p1work;                         // M x hid4
    if (p1kind == 1) {
      lfi_gemm_desc m = {};
      m.batch = 1; m.M = M; m.N = hid; m.K = hist1 * C;
      m.A = q.A; m.lda = q.lda; m.a_kcontig = 1;
      m.B = p1->w1; m.ldb = (long)hist1 * C; m.b_kcontig = 1;
      m.C = ebuf; m.ldc = hid4; m.bias = p1->b1; m.act = 1; m.slope = 0.01f; m.precision = d->gemm_precision;
      if ((rc = lfi_gemm_f32(&m, stream))) return rc;
    } else {
      // GRU / LSTM over the window: input projections of its hist1 frames (batched over the step), then the recurrence
      const int ng = p1kind == 3 ? 4 : 3;
      float* xp = ebuf + (long)M * hid4;          // [M][hist1][ng * hid]
      float* ework = xp + (long)M * hist1 * ng * hid;
      lfi_gemm_desc m = {};
      m.batch = hist1; m.M = M; m.N = ng * hid; m.K = C;
      m.A = q.A; m.lda = q.lda; m.a_kcontig = 1; m.strideA = C;
      m.B = p1->w_ih; m.ldb = C; m.b_kcontig = 1;
      m.C = xp; m.ldc = (long)hist1 * ng * hid; m.strideC = ng * hid; m.precision = d->gemm_precision;
      if ((rc = lfi_gemm_f32(&m, stream))) return rc;
      lfi_enc_desc ed = {};
      ed.B = M; ed.T = hist1; ed.N = 1; ed.start = hist1 - 1; ed.hist = hist1; ed.hid = hid;
      ed.ldcond = hid4; ed.col = 0; ed.precision = d->gemm_precision; ed.dup = 0; ed.lstm = p1kind == 3;
      float* hs = ework + lfi_encode_windows_work_floats(&ed);   // unfused path / LSTM: state sequence
      float* gst = p1kind == 3 ? hs + (long)hist1 * M * hid : nullptr;   // LSTM: gate + cell stash, 5 * hid per (step, row)
      if ((rc = lfi_encode_windows_fwd(&ed, xp, p1->w_hh, p1->b_ih, p1->b_hh, nullptr, ebuf, gst, hs, ework, stream)))
        return rc;
    }
    q.K = hid; q.A = ebuf; q.lda = hid4;
  }
  if ((rc = lfi_gemm_f32(&q, stream))) return rc;
  // gic[k] = c[:, kD:(k+1)D] @ W_ih[k][:, Ch:]^T + b_ih[k]
  lfi_gemm_desc r = {};
  r.batch = Ks; r.M = M; r.N = G; r.K = D;
  r.A = cfr; r.lda = (long)Ks * D; r.a_kcontig = 1; r.strideA = D;
  r.B = wc; r.ldb = D; r.b_kcontig = 1; r.strideB = (long)G * D;
  r.C = gic; r.ldc = G; r.strideC = (long)M * G;
  r.bias = p->b_ih; r.strideBias = G; r.precision = d->gemm_precision;
  return lfi_gemm_f32(&r, stream);
}
namespace {
// frame t of the sequence in `faces`: gic of all flow steps from the frame's rows `cfr` of pre_static (B x Ks D, overwritten) and the
// window faces[:, t - hist1 : t]. have_xfrag: the window's fp16 fragments are already in cfrags (the previous frame's reverse chain)
// ncand >= 2 (lfi_flow_sample_cand_seq, the fused kernel only): cfr holds B / ncand parent rows, row r reads row r / ncand of it
int sample_front_frame(const SampleFront& s, int t, float* cfr, int have_xfrag, void* stream, int ncand = 0) {
  const int B = s.f->B, C = s.f->C, Ks = s.f->Ks, G = s.f->G, hist1 = s.hist1, seq_len = s.seq_len;
  if (s.fused) {
    // (its first workgroup also clears the chain's ticket / progress words for the launch that follows: no memset node per frame)
    return lfi_internal_sample_cond(s.faces, (long)seq_len * C, (long)(t - hist1) * C, s.K1, B, Ks, G, cfr, s.p->b_ih, s.cfrags, s.gic, 0.01f,
                                    (long)B * seq_len * C, s.chain ? s.chain_state : nullptr, (int)s.chain_words, have_xfrag, ncand, stream);
  }
  const float* win = s.faces + (long)(t - hist1) * C;
  long ldwin = (long)seq_len * C;
  if (s.stage_win) {
    int rc;
    if ((rc = lfi_gather_windows(s.faces, B, seq_len, C, 1, t, hist1, 0, nullptr, s.wstage, s.ldw, 0, stream))) return rc;
    win = s.wstage; ldwin = s.ldw;
  }
  return lfi_internal_sample_front_rows(s.d, s.p, s.p1, s.wct, s.E, hist1, s.f->wc, B, win, ldwin, cfr, s.gic, s.p1work, stream);
}
// the chain's ticket / progress words before a frame's launch, unless the fused conditioning kernel has cleared them
int sample_front_clear_chain(const SampleFront& s, hipStream_t st, const char* who) {
  if (s.fused) return LFI_OK;
  hipError_t me = hipMemsetAsync(s.chain_state, 0, s.chain_words * sizeof(unsigned), st);
  LFI_REQUIRE(me == hipSuccess, "%s: hipMemsetAsync: %s", who, hipGetErrorString(me));
  return LFI_OK;
}

// ---- one frame as Ks launches of one cell each (LFI_SAMPLE_CHAIN=0 and the generic cell): what the chain kernels do in one launch.
// h / cstate: the [Ks][B][H] state the frame advances in place (has_prev = 0: from zeros); xa / xb: the B x C tiles between the
// steps, step k writing (k & 1) ? xa : xb; xin / ldx: the rows the first cell reads; l_out: B floats, the rows' sum of the coupling
// log-dets (launch after launch: no two workgroups at one word at a time). The caller's finish and merge launches follow.
// Reverse, z -> x through steps Ks-1 .. 0; step 0 writes `out` (row pitch ld_out). l_out may be null: no log-dets.
void launch_rev_steps(const FlowK& f, FlowStepKernel cell, size_t lds, hipStream_t st, const float* gic, float* h, float* cstate,
                      int has_prev, float* xa, float* xb, const float* xin, long ldx, float* out, long ld_out, float* l_out) {
  const int B = f.B, C = f.C, H = f.H, Ks = f.Ks, G = f.G;
  for (int k = Ks - 1; k >= 0; --k) {
    CellIO io = {};
    io.k = k; io.rows = B; io.x_in = xin; io.ldx = ldx;
    io.h_prev = has_prev ? h + (long)k * B * H : nullptr;
    io.gic = gic + (long)k * B * G;
    io.h_out = h + (long)k * B * H;
    if (f.lstm) { io.c_prev = has_prev ? cstate + (long)k * B * H : nullptr; io.c_out = cstate + (long)k * B * H; }
    if (k == 0) { io.x_out = out; io.ldxo = ld_out; }
    else { io.x_out = (k & 1) ? xa : xb; io.ldxo = C; }
    if (l_out) { io.l_out = l_out; io.l_accumulate = k + 1 < Ks; }
    hipLaunchKernelGGL(cell, dim3(f.nbt), dim3(NT), lds, st, f, io);
    xin = io.x_out; ldx = io.ldxo;
  }
}
// Forward, x -> z through steps 0 .. Ks-1; returns the last step's tile (B x C).
const float* launch_fwd_steps(const FlowK& f, FlowStepKernel cell, size_t lds, hipStream_t st, const float* gic, float* h, float* cstate,
                              int has_prev, float* xa, float* xb, const float* xin, long ldx, float* l_out) {
  const int B = f.B, C = f.C, H = f.H, Ks = f.Ks, G = f.G;
  for (int k = 0; k < Ks; ++k) {
    CellIO io = {};
    io.k = k; io.rows = B; io.x_in = xin; io.ldx = ldx;
    io.h_prev = has_prev ? h + (long)k * B * H : nullptr;
    io.gic = gic + (long)k * B * G;
    io.h_out = h + (long)k * B * H;
    if (f.lstm) { io.c_prev = has_prev ? cstate + (long)k * B * H : nullptr; io.c_out = cstate + (long)k * B * H; }
    io.x_out = (k & 1) ? xa : xb; io.ldxo = C;
    io.l_out = l_out; io.l_accumulate = k > 0;
    hipLaunchKernelGGL(cell, dim3(f.nbt), dim3(NT), lds, st, f, io);
    xin = io.x_out; ldx = C;
  }
  return xin;
}
}  // namespace

// The per-step launches' finish of a frame's NLL (LFI_SAMPLE_CHAIN=0 and the generic cell; the chain kernel does this in its cells):
// acc[b] = sum over the flow steps of the reverse coupling log-dets, left there by the cells' l_out.
__global__ __launch_bounds__(256) void sample_nll_finish_kernel(const float* __restrict__ noise, const float* __restrict__ acc,
                                                                const float* __restrict__ ldconst, int B, int C,
                                                                float* __restrict__ nll) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float lp = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float v = noise[(long)b * C + c];
    lp += -0.5f * (v * v + LOG2PI_F);
  }
  nll[b] = -(ldconst[0] - acc[b] + lp) / LN2_F;
}

extern "C" long lfi_flow_sample_nll_work_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  return 2L * d->B + 8;   // the two ping-pong hand-over arrays of the chain (the first is the per-step launches' accumulator)
}

extern "C" int lfi_flow_frame_plan(const lfi_flow_dims* d) { return d ? flow_frame_plan(d).bits() : 0; }

// A frame's rows of pre_static for the candidates of lfi_flow_sample_cand_seq, where the front end overwrites what it reads (every
// path but the fused kernel): workgroup v copies parent row v / ncand (KD floats) to row v of a one-frame scratch. 16-byte words
// where both sides allow it.
__global__ __launch_bounds__(256) void cand_pre_bcast_kernel(const float* __restrict__ src, float* __restrict__ dst, int ncand, long KD,
                                                            int vec) {
  const long v = blockIdx.x;
  const float* from = src + (v / ncand) * KD;
  float* to = dst + v * KD;
  if (vec) {
    for (long j = threadIdx.x; j < KD / 4; j += 256) reinterpret_cast<float4*>(to)[j] = reinterpret_cast<const float4*>(from)[j];
  } else {
    for (long j = threadIdx.x; j < KD; j += 256) to[j] = from[j];
  }
}

namespace {
constexpr long kCandMaxRows = 1L << 22;   // virtual rows of one lfi_flow_sample_cand_from / lfi_flow_sample_cand_seq call
// launch_rev_steps from the prior draws `noise` (f.B x C), then the finish of the frame's NLL from the cells' accumulator (nll null: neither)
void launch_rev_frame(const FlowK& f, FlowStepKernel cell, size_t lds, hipStream_t st, const float* gic, float* h, float* cstate, int has_prev,
                      float* xa, float* xb, const float* noise, float* out, long ld_out, float* acc, float* nll) {
  launch_rev_steps(f, cell, lds, st, gic, h, cstate, has_prev, xa, xb, noise, f.C, out, ld_out, nll ? acc : nullptr);
  if (nll) hipLaunchKernelGGL(sample_nll_finish_kernel, dim3(lfi_cdiv(f.B, 256)), dim3(256), 0, st, noise, acc, f.ldconst, f.B, f.C, nll);
}
// where the one-frame scratch of lfi_flow_sample_cand_seq lies in its work area: behind the sampler's own carve, 16-byte aligned
inline long cand_seq_scratch_offset(const lfi_flow_dims* dv) { return (lfi_flow_sample_work_floats(dv) + 3) & ~3L; }

// The body of lfi_flow_sample_seq_nll (ncand = 0, names as they always were) and of lfi_flow_sample_cand_seq (ncand >= 1: the d->B
// rows are ncand candidates of each of d->B / ncand parent rows; pre_static has the PARENTS' rows, nframes * (d->B / ncand), and
// virtual row v of frame n reads row n * (d->B / ncand) + v / ncand). Everything else is per row in both.
int sample_seq_run(const char* who, const char* who_from, const char* who_nll, const lfi_flow_dims* d, const lfi_flow_params* p,
                   const float* prep, const float* wct, long E, int hist1, float* pre_static, const float* noise, float* faces,
                   int seq_len, int start, int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1, float* p1work,
                   float* work, float* nll, float* nll_work, void* stream, int ncand) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, who);
  if (rc) return rc;
  if ((rc = frame_args_check(who, who_from, d, prep && wct && pre_static && noise && faces && h && work,
                             E, hist1, start, nframes, seq_len, cstate, first_frame, p1))) return rc;
  LFI_REQUIRE(!nll || nll_work, "%s: nll needs nll_work (lfi_flow_sample_nll_work_floats)", who_nll);
  if (ncand) {
    LFI_REQUIRE(ncand >= 1 && d->B % ncand == 0 && (long)d->B <= kCandMaxRows,
                "%s: %d candidates per row do not divide the %d virtual rows (at most %ld)", who, ncand, d->B, kCandMaxRows);
    LFI_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "%s: work is not 16-byte aligned", who);
  }
  const int B = f.B, C = f.C, D = f.D, Ks = f.Ks;
  const int Bp = ncand ? B / ncand : B;          // rows of pre_static per frame
  hipStream_t st = (hipStream_t)stream;
  const FramePlan pl = flow_frame_plan(d);
  const bool chain = pl.chain;
  const size_t lds = pl.fast ? pl.lds_fast : pl.lds_gen;
  const FlowStepKernel cell = flow_step_rev_pick(pl.fast, f.lstm);
  if ((rc = set_flow_lds(cell, lds, "lfi_flow_sample_seq"))) return rc;
  // the per-frame conditioning (sample_front_*): the carve of `work`, the fused kernel's weight fragments once per call
  SampleFront sf = {};
  if ((rc = sample_front_setup(&sf, d, p, &f, wct, E, hist1, pre_static, faces, seq_len, p1, p1work, work, chain, nframes, stream,
                               who))) return rc;
  const int K1 = sf.K1;
  // candidates: the fused kernel reads the parents' rows in place (it never writes them); every other front end overwrites its rows
  // of pre_static with c, so each frame's parent rows are first copied to B rows of a one-frame scratch behind the sampler's carve
  // (ncand = 1: a plain copy, then the same launches on the same shapes)
  float* scratch = (ncand && !sf.fused) ? work + cand_seq_scratch_offset(d) : nullptr;
  const long KD = (long)Ks * D;
  // (diagnostics, tools/stream_latency.py, the candidates' entry point only: LFI_CHUNK_ONLY=front launches every frame's front end and
  // no chain, so that events around the call time the front end alone. Results are not meaningful.)
  const char* only = ncand ? getenv("LFI_CHUNK_ONLY") : nullptr;
  const bool run_chain = !(only && only[0] == 'f');
  // LFI_SAMPLE_XF_CHAIN=0 keeps the window-fragment kernel in front of every frame's conditioning
  const bool xf_chain = sf.fused && chain && lfi_env_on("LFI_SAMPLE_XF_CHAIN");
  // one launch for the whole chain of a frame; with nll the cells also pass the rows' running log-density down the chain
  const FlowRevChainKernel chain_kernel = flow_rev_chain_pick(pl, f.lstm, nll != nullptr);
  if (chain && (rc = set_flow_lds(chain_kernel, lds, nll ? who_nll : who))) return rc;
  for (int n = 0; n < nframes; ++n) {
    const int t = start + n;
    float* cfr = pre_static + (long)n * Bp * KD;
    if (scratch) {
      const int vec = KD % 4 == 0 && (reinterpret_cast<uintptr_t>(cfr) & 15) == 0 ? 1 : 0;
      hipLaunchKernelGGL(cand_pre_bcast_kernel, dim3(B), dim3(256), 0, st, cfr, scratch, ncand, KD, vec);
      cfr = scratch;
    }
    // (from the run's second frame on the window's fragments are already there: the previous frame's chain left them)
    if ((rc = sample_front_frame(sf, t, cfr, (xf_chain && n > 0) ? 1 : 0, stream, scratch ? 0 : ncand))) return rc;
    if (!run_chain) continue;
    // reverse flow: z -> x through steps Ks-1 .. 0
    if (chain) {   // one launch for the whole chain of this frame
      RevChain rcn = {};
      rcn.noise = noise + (long)n * B * C; rcn.xa = sf.xa; rcn.xb = sf.xb;
      rcn.frame = faces + (long)t * C; rcn.ld_frame = (long)seq_len * C;
      rcn.gic = sf.gic; rcn.h = h; rcn.cstate = cstate; rcn.has_prev = first_frame + n > 0 ? 1 : 0; rcn.frame_no = first_frame + n; rcn.pipe = sf.chain_state;
      if (xf_chain && n + 1 < nframes) {
        rcn.xf = reinterpret_cast<_Float16*>(lfi_internal_sample_cond_xfrag_ptr(sf.cfrags, Ks, f.G, K1));
        rcn.faces = faces; rcn.xf_off = (long)(t + 1 - hist1) * C; rcn.K1 = K1; rcn.NM1 = (K1 + 31) / 32;
      }
      if ((rc = sample_front_clear_chain(sf, st, who))) return rc;
      if (nll) { rcn.qa = nll_work; rcn.qb = nll_work + B; rcn.nll = nll + (long)n * B; }
      hipLaunchKernelGGL(chain_kernel, dim3(Ks * f.nbt), dim3(NT), lds, st, f, rcn);
      continue;
    }
    launch_rev_frame(f, cell, lds, st, sf.gic, h, cstate, first_frame + n > 0 ? 1 : 0, sf.xa, sf.xb, noise + (long)n * B * C,
                     faces + (long)t * C, (long)seq_len * C, nll_work, nll ? nll + (long)n * B : nullptr);
  }
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}
}  // namespace

// lfi_flow_sample_seq_from that also leaves the per-frame NLL (bits) of every frame it generates in nll (nframes x B); nll == NULL:
// lfi_flow_sample_seq_from itself - the same launches of the same kernels.
extern "C" int lfi_flow_sample_seq_nll(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct,
                                       long E, int hist1, float* pre_static, const float* noise, float* faces, int seq_len,
                                       int start, int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1,
                                       float* p1work, float* work, float* nll, float* nll_work, void* stream) {
  return sample_seq_run("lfi_flow_sample_seq", "lfi_flow_sample_seq_from", "lfi_flow_sample_seq_nll", d, p, prep, wct, E, hist1, pre_static,
                        noise, faces, seq_len, start, nframes, first_frame, h, cstate, p1, p1work, work, nll, nll_work, stream, 0);
}

// ---- N candidate ROLLOUTS of nframes frames per session row (SampleStream.rollout_candidates): the sampler over V = B * ncand virtual
// rows whose static conditioning is their parent row's, read in place
extern "C" long lfi_flow_sample_cand_seq_work_floats(const lfi_flow_dims* d, int ncand) {
  if (!d || ncand < 1 || d->B < 1 || (long)d->B * ncand > kCandMaxRows) return 0;
  lfi_flow_dims dv = *d;
  dv.B = d->B * ncand;
  return cand_seq_scratch_offset(&dv) + (long)dv.B * dv.Ks * dv.D + 8;
}

extern "C" int lfi_flow_sample_cand_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct,
                                        long E, int hist1, float* pre_static, const float* noise, float* faces, int seq_len,
                                        int start, int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1,
                                        float* p1work, float* work, float* nll, float* nll_work, int ncand, void* stream) {
  const char* who = "lfi_flow_sample_cand_seq";
  LFI_REQUIRE(d && p, "%s: null pointer (dims / params)", who);
  LFI_REQUIRE(ncand >= 1, "%s: %d candidates per row (at least 1)", who, ncand);
  return sample_seq_run(who, who, who, d, p, prep, wct, E, hist1, pre_static, noise, faces, seq_len, start, nframes, first_frame, h, cstate,
                        p1, p1work, work, nll, nll_work, stream, ncand);
}

// ---- N candidates of one frame per session row (SampleStream.step_candidates)
namespace {
// the carve of lfi_flow_sample_cand_from's candidate work area
struct CandWork {
  unsigned* pipe; long pipe_words;
  float *xa, *xb;     // V x C ping / pong tiles
  float *qa, *qb;     // V floats each: the log-density hand-over (qa: the per-step launches' accumulator)
  float* gicv;        // per-step launches only: [Ks][V][G], the parents' gic broadcast
  long total;
};
CandWork cand_work_carve(float* base, long V, long C, long G, long Ks) {
  CandWork w = {};
  const long tiles = (V + MB - 1) / MB;
  long o = 0;
  w.pipe = reinterpret_cast<unsigned*>(base); w.pipe_words = ((long)PIPE_HDR + Ks * tiles + 3) & ~3L; o += w.pipe_words;
  w.xa = base + o; o += V * C;
  w.xb = base + o; o += V * C;
  w.qa = base + o; o += V;
  w.qb = base + o; o += V;
  w.gicv = base + o; o += Ks * V * G;
  w.total = o + 8;
  return w;
}
}  // namespace

extern "C" long lfi_flow_sample_cand_work_floats(const lfi_flow_dims* d, int ncand) {
  if (!d || ncand < 1 || d->B < 1 || (long)d->B * ncand > kCandMaxRows) return 0;
  return cand_work_carve(nullptr, (long)d->B * ncand, d->C, (long)(d->lstm ? 4 : 3) * d->H, d->Ks).total;
}

extern "C" int lfi_flow_sample_cand_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct,
                                         long E, int hist1, float* pre_static, const float* noise, float* faces, int seq_len,
                                         int start, int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1,
                                         float* p1work, float* work, float* nll, float* nll_work, int ncand, float* cand_frames,
                                         float* cand_nll, float* cand_h, float* cand_c, float* cand_work, void* stream) {
  const char* who = "lfi_flow_sample_cand_from";
  (void)nll; (void)nll_work;
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, who);
  if (rc) return rc;
  if ((rc = frame_args_check(who, who, d, prep && wct && pre_static && noise && faces && h && work && cand_frames && cand_nll && cand_h && cand_work,
                             E, hist1, start, nframes, seq_len, cstate, first_frame, p1))) return rc;
  LFI_REQUIRE(nframes == 1, "%s: %d frames (one frame per call)", who, nframes);
  LFI_REQUIRE(ncand >= 1 && (long)d->B * ncand <= kCandMaxRows, "%s: %d candidates per row (1 .. %ld at batch %d)", who, ncand,
              kCandMaxRows / d->B, d->B);
  LFI_REQUIRE(!d->lstm || cand_c, "%s: the LSTM cell needs cand_c", who);
  LFI_REQUIRE((reinterpret_cast<uintptr_t>(cand_work) & 3) == 0, "%s: cand_work is not 4-byte aligned", who);
  const int B = f.B, C = f.C, H = f.H, Ks = f.Ks, G = f.G;
  const int V = B * ncand, nbtv = lfi_cdiv(V, MB);
  hipStream_t st = (hipStream_t)stream;
  const FramePlan pl = flow_frame_plan(d);
  const bool chain = pl.chain;
  const size_t lds = pl.fast ? pl.lds_fast : pl.lds_gen;
  const FlowCandChainKernel chain_kernel = flow_cand_chain_pick(pl, f.lstm);
  const FlowStepKernel cell = flow_step_rev_pick(pl.fast, f.lstm);
  if ((rc = chain ? set_flow_lds(chain_kernel, lds, who) : set_flow_lds(cell, lds, who))) return rc;
  const CandWork cw = cand_work_carve(cand_work, V, C, G, Ks);
  // the front end for the session's B rows, unchanged; the chain's words are the candidate area's (sized for V)
  SampleFront sf = {};
  if ((rc = sample_front_setup(&sf, d, p, &f, wct, E, hist1, pre_static, faces, seq_len, p1, p1work, work, chain, 1, stream, who,
                               chain ? cw.pipe : nullptr, (size_t)cw.pipe_words))) return rc;
  if ((rc = sample_front_frame(sf, start, pre_static, 0, stream))) return rc;
  const int has_prev = first_frame > 0 ? 1 : 0;
  if (chain) {
    CandChain cc = {};
    cc.noise = noise; cc.xa = cw.xa; cc.xb = cw.xb; cc.frames = cand_frames; cc.gic = sf.gic; cc.h = h; cc.cstate = cstate;
    cc.ch = cand_h; cc.cc = cand_c; cc.has_prev = has_prev; cc.V = V; cc.ncand = ncand; cc.nbt = nbtv; cc.pipe = cw.pipe;
    cc.qa = cw.qa; cc.qb = cw.qb; cc.nll = cand_nll;
    if ((rc = sample_front_clear_chain(sf, st, who))) return rc;   // (sf's chain words are cw.pipe here)
    hipLaunchKernelGGL(chain_kernel, dim3(Ks * nbtv), dim3(NT), lds, st, f, cc);
  } else {
    hipLaunchKernelGGL(cand_gather_kernel, dim3(V, Ks), dim3(256), 0, st, sf.gic, h, f.lstm ? cstate : nullptr, B, V, ncand, G, H, has_prev,
                       cw.gicv, cand_h, cand_c);
    FlowK fv = f;   // the cells over V rows
    fv.B = V; fv.F = V; fv.nbt = nbtv;
    launch_rev_frame(fv, cell, lds, st, cw.gicv, cand_h, cand_c, has_prev, cw.xa, cw.xb, noise, cand_frames, C, cw.qa, cand_nll);
  }
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}

// ---- teacher-forced frames of a sequence whose state is carried (SampleStream.observe): the sampler's front end, then the FORWARD chain
// The per-step launches' finish of an observed frame (LFI_SAMPLE_CHAIN=0 and the generic cell; the forward chain does this in its
// last cell): acc[b] = sum over the flow steps of the forward coupling log-dets (the cells' l_out), zlast = the last step's tile.
__global__ __launch_bounds__(256) void score_finish_kernel(const float* __restrict__ zlast, const float* __restrict__ acc,
                                                           const float* __restrict__ ldconst, int B, int C, float* __restrict__ z,
                                                           float* __restrict__ nll) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float lp = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float v = zlast[(long)b * C + c];
    lp += -0.5f * (v * v + LOG2PI_F);
    if (z) z[(long)b * C + c] = v;
  }
  nll[b] = -(ldconst[0] + acc[b] + lp) / LN2_F;
}

namespace {
// launch_fwd_steps of the streaming forward cell on the frame at `frame`, then the finish: the frame's NLL, its latent where z is not null
void launch_fwd_frame(const FlowK& f, size_t lds, hipStream_t st, const float* gic, float* h, float* cstate, int has_prev, float* xa,
                      float* xb, const float* frame, long ld_frame, float* acc, float* z, float* nll) {
  const float* zlast = launch_fwd_steps(f, flow_step_kernel<false>, lds, st, gic, h, cstate, has_prev, xa, xb, frame, ld_frame, acc);
  hipLaunchKernelGGL(score_finish_kernel, dim3(lfi_cdiv(f.B, 256)), dim3(256), 0, st, zlast, acc, f.ldconst, f.B, f.C, z, nll);
}
}  // namespace

extern "C" long lfi_flow_score_work_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  return 2L * d->B + 8;   // the two ping-pong log-det hand-over arrays of the forward chain (the first: the per-step launches' accumulator)
}

extern "C" int lfi_flow_score_seq_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                                       int hist1, float* pre_static, float* faces, int seq_len, int start, int nframes, int first_frame,
                                       float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work, float* score_work,
                                       float* z, float* nll, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, "lfi_flow_score_seq_from");
  if (rc) return rc;
  const char* who = "lfi_flow_score_seq_from";
  if ((rc = frame_args_check(who, who, d, prep && wct && pre_static && faces && h && work && score_work && nll, E, hist1, start, nframes,
                             seq_len, cstate, first_frame, p1))) return rc;
  LFI_REQUIRE(nframes >= 0, "%s: bad frame range", who);
  const int B = f.B, C = f.C, D = f.D, Ks = f.Ks;
  hipStream_t st = (hipStream_t)stream;
  // the register-resident chain for the shapes the sampler's chain takes; otherwise (and with LFI_SAMPLE_CHAIN=0) Ks launches of the
  // streaming forward cell + the finish
  const FramePlan pl = flow_frame_plan(d);
  const bool chain = pl.chain;
  const size_t lds = chain ? pl.lds_fast : pl.lds_gen;
  const FlowFwdChainKernel chain_kernel = flow_fwd_chain_pick(pl, f.lstm);
  if ((rc = chain ? set_flow_lds(chain_kernel, lds, "lfi_flow_score_seq_from") : set_flow_lds(flow_step_kernel<false>, lds, "lfi_flow_score_seq_from")))
    return rc;
  SampleFront sf = {};
  if ((rc = sample_front_setup(&sf, d, p, &f, wct, E, hist1, pre_static, faces, seq_len, p1, p1work, work, chain, nframes, stream,
                               "lfi_flow_score_seq_from"))) return rc;
  float *qa = score_work, *qb = score_work + B;
  for (int n = 0; n < nframes; ++n) {
    const int t = start + n;
    if ((rc = sample_front_frame(sf, t, pre_static + (long)n * B * Ks * D, 0, stream))) return rc;
    float* zn = z ? z + (long)n * B * C : nullptr;
    const int has_prev = first_frame + n > 0 ? 1 : 0;
    if (chain) {
      FwdChain fc = {};
      fc.frame = faces + (long)t * C; fc.ld_frame = (long)seq_len * C;
      fc.xa = sf.xa; fc.xb = sf.xb; fc.gic = sf.gic; fc.h = h; fc.cstate = cstate; fc.has_prev = has_prev; fc.pipe = sf.chain_state;
      fc.qa = qa; fc.qb = qb; fc.z = zn; fc.nll = nll + (long)n * B;
      if ((rc = sample_front_clear_chain(sf, st, who))) return rc;
      hipLaunchKernelGGL(chain_kernel, dim3(Ks * f.nbt), dim3(NT), lds, st, f, fc);
      continue;
    }
    launch_fwd_frame(f, lds, st, sf.gic, h, cstate, has_prev, sf.xa, sf.xb, faces + (long)t * C, (long)seq_len * C, qa, zn, nll + (long)n * B);
  }
  LFI_LAUNCH_CHECK("lfi_flow_score_seq_from");
  return LFI_OK;
}

// ---- one frame of a session whose rows generate or observe, row by row (SampleStream.step_rows)
namespace {
// words of flow_rows_chain_kernel's state: ticket, abort, 2 reserved, then Ks * tiles progress words per direction
inline long rows_pipe_words(long Ks, long tiles) { return ((long)PIPE_HDR + 2 * Ks * tiles + 3) & ~3L; }

// the carve of lfi_flow_step_rows_from's second work area
struct RowsWork {
  unsigned* pipe; long pipe_words;
  float *xa, *xb;     // the forward direction's B x C ping / pong tiles
  float *qa, *qb;     // its log-det hand-over (the per-step launches' accumulator)
  float *hs, *cs;     // per-step launches only: [Ks][B][H] copies of h / cstate the forward direction advances
  float *gframe;      // ... B x C: the frame the reverse direction generates
  float *fnll;        // ... B: the forward direction's NLL
  long total;
};
RowsWork rows_work_carve(float* base, long B, long C, long H, long Ks) {
  RowsWork w = {};
  const long tiles = (B + MB - 1) / MB;
  long o = 0;
  w.pipe = reinterpret_cast<unsigned*>(base); w.pipe_words = rows_pipe_words(Ks, tiles); o += w.pipe_words;
  w.xa = base + o; o += B * C;
  w.xb = base + o; o += B * C;
  w.qa = base + o; o += B;
  w.qb = base + o; o += B;
  w.hs = base + o; o += Ks * B * H;
  w.cs = base + o; o += Ks * B * H;
  w.gframe = base + o; o += B * C;
  w.fnll = base + o; o += B;
  w.total = o + 8;
  return w;
}

// The per-step launches' last launch of a mixed frame: the reverse direction has advanced h / cstate of EVERY row and left its frame in
// gframe and its NLL in nll; the forward direction has advanced the copies hs / cs from the frame in `faces` and left its NLL in fnll.
// Observing rows take the forward direction's state and NLL (their frame is in place), generating rows their generated frame.
// Thread (row, element) over Ks * H state elements and C frame elements of every row.
__global__ __launch_bounds__(256) void rows_merge_kernel(const int* __restrict__ role, int B, int C, int H, int Ks, float* __restrict__ h,
                                                         float* __restrict__ cstate, const float* __restrict__ hs,
                                                         const float* __restrict__ cs, float* __restrict__ frame, long ld_frame,
                                                         const float* __restrict__ gframe, float* __restrict__ nll,
                                                         const float* __restrict__ fnll) {
  const int b = blockIdx.x;
  const bool observes = role[b] != 0;
  if (observes) {
    for (int e = threadIdx.x; e < Ks * H; e += 256) {
      const long o = ((long)(e / H) * B + b) * H + e % H;
      h[o] = hs[o];
      if (cstate) cstate[o] = cs[o];
    }
    if (threadIdx.x == 0) nll[b] = fnll[b];
  } else {
    for (int c = threadIdx.x; c < C; c += 256) frame[(long)b * ld_frame + c] = gframe[(long)b * C + c];
  }
}
}  // namespace

extern "C" long lfi_flow_step_rows_work_floats(const lfi_flow_dims* d) {
  if (!d) return 0;
  return rows_work_carve(nullptr, d->B, d->C, d->H, d->Ks).total;
}

// nframes >= 1 frames in which row b observes frame n where observed[n * B + b] != 0 - that frame is in faces[:, start + n] already - and
// generates it from noise[n][b] otherwise: the one body of lfi_flow_step_rows_from (nframes = 1) and lfi_flow_step_rows_seq. Per frame:
// the conditioning front end, the chain-state clear, then flow_rows_chain_kernel with that frame's role, noise and nll rows; shapes and
// switches outside the chain: the forward direction's per-step launches on copies of h / cstate, the reverse direction's on the state
// itself with its frame aside, one merge launch. The work areas are one frame's, reused from frame to frame: the stream orders them,
// as in lfi_flow_sample_seq_nll's loop. have_xfrag stays 0: the reverse chain's window-fragment hand-over has no forward-direction
// counterpart, and a frame a row observed never passes through the chain that would leave its fragments.
namespace {
int step_rows_frames(const char* who, const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                     int hist1, float* pre_static, const float* noise, float* faces, int seq_len, int start, int nframes,
                     int first_frame, float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work, float* nll,
                     float* nll_work, const int* observed, float* rows_work, void* stream) {
  FlowK f = {};
  int rc = fill_flow(d, p, prep, &f, who);
  if (rc) return rc;
  if ((rc = frame_args_check(who, who, d, prep && wct && pre_static && noise && faces && h && work && nll && nll_work && observed && rows_work,
                             E, hist1, start, nframes, seq_len, cstate, first_frame, p1))) return rc;
  LFI_REQUIRE(nframes >= 1, "%s: %d frames (at least one)", who, nframes);
  LFI_REQUIRE((reinterpret_cast<uintptr_t>(rows_work) & 3) == 0, "%s: rows_work is not 4-byte aligned", who);
  const int B = f.B, C = f.C, D = f.D, H = f.H, Ks = f.Ks;
  hipStream_t st = (hipStream_t)stream;
  const FramePlan pl = flow_frame_plan(d);
  const bool fast = pl.fast, chain = pl.chain;
  const size_t lds_fast = pl.lds_fast, lds_gen = pl.lds_gen;
  const FlowRowsChainKernel chain_kernel = flow_rows_chain_pick(pl, f.lstm);   // (each direction's own form)
  const FlowStepKernel rev_cell = flow_step_rev_pick(fast, f.lstm);
  if (chain) {
    if ((rc = set_flow_lds(chain_kernel, lds_fast, who))) return rc;
  } else {
    if ((rc = set_flow_lds(rev_cell, fast ? lds_fast : lds_gen, who))) return rc;
    if ((rc = set_flow_lds(flow_step_kernel<false>, lds_gen, who))) return rc;
  }
  const RowsWork rw = rows_work_carve(rows_work, B, C, H, Ks);
  SampleFront sf = {};
  if ((rc = sample_front_setup(&sf, d, p, &f, wct, E, hist1, pre_static, faces, seq_len, p1, p1work, work, chain, nframes, stream,
                               who, chain ? rw.pipe : nullptr, (size_t)rw.pipe_words))) return rc;
  const long ld_frame = (long)seq_len * C;
  const size_t state_bytes = (size_t)Ks * B * H * sizeof(float);
  for (int n = 0; n < nframes; ++n) {
    const int t = start + n;
    const int has_prev = first_frame + n > 0 ? 1 : 0;
    const int* role = observed + (long)n * B;
    const float* noise_n = noise + (long)n * B * C;
    float* nll_n = nll + (long)n * B;
    if ((rc = sample_front_frame(sf, t, pre_static + (long)n * B * Ks * D, 0, stream))) return rc;
    float* frame = faces + (long)t * C;
    if (chain) {
      RowsChain rcn = {};
      rcn.role = role;
      rcn.rev.noise = noise_n; rcn.rev.xa = sf.xa; rcn.rev.xb = sf.xb; rcn.rev.frame = frame; rcn.rev.ld_frame = ld_frame;
      rcn.rev.gic = sf.gic; rcn.rev.h = h; rcn.rev.cstate = cstate; rcn.rev.has_prev = has_prev; rcn.rev.frame_no = first_frame + n;
      rcn.rev.pipe = rw.pipe; rcn.rev.qa = nll_work; rcn.rev.qb = nll_work + B; rcn.rev.nll = nll_n;
      rcn.fwd.frame = frame; rcn.fwd.ld_frame = ld_frame; rcn.fwd.xa = rw.xa; rcn.fwd.xb = rw.xb; rcn.fwd.gic = sf.gic;
      rcn.fwd.h = h; rcn.fwd.cstate = cstate; rcn.fwd.has_prev = has_prev; rcn.fwd.pipe = rw.pipe;
      rcn.fwd.qa = rw.qa; rcn.fwd.qb = rw.qb; rcn.fwd.nll = nll_n;
      if ((rc = sample_front_clear_chain(sf, st, who))) return rc;   // (sf's chain words are rw.pipe here)
      hipLaunchKernelGGL(chain_kernel, dim3(2 * Ks * f.nbt), dim3(NT), lds_fast, st, f, rcn);
      continue;
    }
    // ---- per-step launches. The forward direction first: it reads the observed frame and the state of the frame before
    if (has_prev) {
      hipError_t me = hipMemcpyAsync(rw.hs, h, state_bytes, hipMemcpyDeviceToDevice, st);
      if (me == hipSuccess && f.lstm) me = hipMemcpyAsync(rw.cs, cstate, state_bytes, hipMemcpyDeviceToDevice, st);
      LFI_REQUIRE(me == hipSuccess, "%s: hipMemcpyAsync: %s", who, hipGetErrorString(me));
    }
    launch_fwd_frame(f, lds_gen, st, sf.gic, rw.hs, rw.cs, has_prev, rw.xa, rw.xb, frame, ld_frame, rw.qa, nullptr, rw.fnll);
    // ---- the reverse direction on the state itself, its frame aside (the observing rows' frame stays in `faces`)
    launch_rev_frame(f, rev_cell, fast ? lds_fast : lds_gen, st, sf.gic, h, cstate, has_prev, sf.xa, sf.xb, noise_n, rw.gframe, C, nll_work, nll_n);
    hipLaunchKernelGGL(rows_merge_kernel, dim3(B), dim3(256), 0, st, role, B, C, H, Ks, h, cstate, rw.hs, rw.cs, frame, ld_frame,
                       rw.gframe, nll_n, rw.fnll);
  }
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}
}  // namespace

// One frame (nframes = 1) in which row b observes where observed[b] != 0 - its frame is in faces[:, start] already - and generates from
// noise[b] otherwise: lfi_flow_sample_seq_nll's arguments, the role words and a second work area (lfi_flow_step_rows_work_floats).
// Every row's h / cstate, frame and nll (B, required) are what lfi_flow_score_seq_from or lfi_flow_sample_seq_nll alone leaves for it.
// The one-frame call of step_rows_frames: the conditioning front end once, then flow_rows_chain_kernel (or the per-step launches).
extern "C" int lfi_flow_step_rows_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                                       int hist1, float* pre_static, const float* noise, float* faces, int seq_len, int start,
                                       int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1, float* p1work,
                                       float* work, float* nll, float* nll_work, const int* observed, float* rows_work, void* stream) {
  const char* who = "lfi_flow_step_rows_from";
  LFI_REQUIRE(nframes == 1, "%s: %d frames (one frame per call)", who, nframes);
  return step_rows_frames(who, d, p, prep, wct, E, hist1, pre_static, noise, faces, seq_len, start, nframes, first_frame, h, cstate, p1,
                          p1work, work, nll, nll_work, observed, rows_work, stream);
}

// A run of nframes >= 1 frames of a chunk whose rows take their roles frame by frame (SampleStream.step_rows_many): what a host loop
// of nframes lfi_flow_step_rows_from calls launches, in one call with one argument check, one kernel pick and - for the fused
// conditioning kernel - one preparation of the weight fragments. lfi_flow_step_rows_from's arguments; pre_static has nframes * B rows,
// noise is nframes x B x C, nll nframes x B and observed nframes x B ints, all frame-major. Frame n runs at t = start + n with
// has_prev = first_frame + n > 0 and frame_no = first_frame + n; the work areas are one frame's.
extern "C" int lfi_flow_step_rows_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                                      int hist1, float* pre_static, const float* noise, float* faces, int seq_len, int start,
                                      int nframes, int first_frame, float* h, float* cstate, const lfi_p1enc* p1, float* p1work,
                                      float* work, float* nll, float* nll_work, const int* observed, float* rows_work, void* stream) {
  return step_rows_frames("lfi_flow_step_rows_seq", d, p, prep, wct, E, hist1, pre_static, noise, faces, seq_len, start, nframes,
                          first_frame, h, cstate, p1, p1work, work, nll, nll_work, observed, rows_work, stream);
}
