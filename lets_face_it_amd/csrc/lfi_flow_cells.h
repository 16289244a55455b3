// What the two flow units share: lfi_flow.hip (the training walks, the prep kernels, the parameter gradients) and
// lfi_flow_chain.hip (the per-frame cells and chains of the samplers and the streaming sessions). The cell's argument structs and
// constants, the LDS carves, the generic forward / reverse cell bodies, the register-resident cell's phases and MFMA helpers, the
// hand-off primitives of the persistent kernels, and the host helpers both sides call. Everything here is inline or has internal
// linkage; no __global__ function lives here - each kernel is defined and instantiated in exactly one of the two units.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "lfi_common.h"

namespace {

constexpr int MB = 16;        // samples per workgroup
constexpr int NT = 512;       // threads per workgroup (8 waves: one 16-wide hidden tile each at H = 128)
constexpr int NW = NT / 64;
constexpr int LT = MB + 1;    // k-major LDS leading dimension. (ds_read_b32 / ds_write_b32 bank = dword address mod 32, 32 lanes per LDS cycle:
                              // with a pitch of 17 a column-of-k store (one row, 32 consecutive k) is conflict-free and the MFMA A-operand read
                              // of two consecutive k rows x 16 lanes puts ONE lane of the second row on the first row's bank 0 - the extra cycle
                              // SQ_LDS_BANK_CONFLICT counts on nearly every such read (36 - 40 % of the walks' LDS cycles). Round 4 tried a
                              // pitch of 16 with 2 floats after every fourth row (reads conflict-free, stores 2 - 4-way): the counter stayed at
                              // 36 - 40 % - it is not these reads that it counts - and the backward cell's Q3 went from 2.5 k to 5.4 k cycles:
                              // reverted, profiles/round4_walk_ab.md.)
constexpr float LOG2PI_F = 1.8378770664093453f;
constexpr float LN2_F = 0.6931471805599453f;

struct FlowK {
  // dims
  int B, N, C, H, D, Ks, affine, lstm;
  float eps;
  int Ch, C2, Cout, G, I, F, nbt;
  int ldc, ldo;   // row strides of the (rows x C) and (rows x Cout) stash arrays: C and Cout rounded up to 4 floats, so that the
                  // deferred weight-gradient products over them read 16-byte aligned rows (bf16x3 / vector-load paths)
  // params
  lfi_flow_params p;
  // prep
  const float *W, *Wt, *Winv, *wz_t, *whh_t, *wfl_t, *wc, *ldconst;
  // prep, zero-padded images for the register-resident cell kernels (k rows padded to 4, columns to 16)
  const float *pW, *pWt, *pwz, *pwh, *pwfl, *bwfl, *bwh, *bwz, *pWinv;
  // backward recurrent weights pre-split into bf16 hi / lo 32-k fragments (bf16 x 3 walk): [Ks][NG][H16/32][J][4 lane groups],
  // one uint4 per entry and plane; the lo plane follows the hi plane of an image
  const uint4 *xbwh, *xbwz;
  // reverse (sampling) cell weights pre-split into fp16 hi / lo 32-k fragments (flow_prep_x3h_kernel): images of pwz, pwh, pwfl and
  // pWinv, entry (32-k block b, lane group kq, column) = x3h_pack of the two f32x4 entries the cell used to load and split itself;
  // one uint4 per entry and plane, the lo plane follows the hi plane of a flow step's image. Null unless lfi_flow_prep made them.
  const uint4 *hwz, *hwh, *hwfl, *hWinv;
  int dgi_hi_only;         // the dgi planes' hi halves only (their consumers take them as a rounded A operand: two products)
  int g16;                 // backward walk (planes mode): the dgi | dgh ROWS of the backward stash are bf16 arrays of the same shapes -
                           // their readers, the thin weight-gradient products, round that operand to bf16 anyway (two products):
                           // lfi_flow_dims.gemm_precision bit 16, honoured by lfi_flow_seq_bwd_planes and lfi_flow_param_grads alike
  __bf16* bDgiR;           // backward walk (bf16x3): dgi also as operand planes of the (Ks F x G) matrix (lfi_flow_seq_bwd_planes)
  int C16, Ch16, H16, Co16, NG;
  // forward stash
  float *sA, *sY, *sX, *sH, *sG, *sO, *sL, *sC;   // sC: LSTM cell state (lstm only)
  // backward stash
  float *bDlin, *bDgi, *bDgh, *bDy, *bDx, *bDh, *bPlfl, *bPan, *bDc;   // bDc: carried d cell state (lstm only)
  float* bPbias;   // [Ks][nbt][2][G]: per-workgroup sums over timesteps and the tile's rows of dgi | dgh (persistent walk only)
  // sequence inputs
  const float* x0; int T, start;
  const float* gic;
  float gscale;
  unsigned long long* stamps;  // diagnostics only (lfi_debug_set_stamps): s_memtime at phase boundaries, else null
  int stamp_k;                 // flow step whose workgroup (tile 0) stamps (LFI_STAMP_K, default Ks / 2)
  int pipe_fence;              // 1: consumers run an agent-scope acquire after the poll and read the tile with plain loads
                               // 0: no fence, every load of a handed-off tile is an sc1 load (L1 bypass)
  unsigned* pipe;              // persistent-pipeline state (flow_pipe_*_kernel): [0] ticket, [1] abort, [4 + k * nbt + bt] progress
};

// Everything one forward cell touches, resolved to pointers for its (k, frame block).
struct CellIO {
  int k, rows;            // flow step, valid rows in this call (<= B)
  const float* x_in; long ldx;   // rows x C
  const float* h_prev;    // rows x H or null (zeros)
  const float* c_prev;    // LSTM cell state, rows x H or null (zeros); unused for GRU
  float* c_out;           // LSTM: new cell state (required when lstm)
  const float* gic;       // rows x G
  float *a_out, *y_out, *x_out, *h_out, *g_out, *o_out, *l_out;  // nullable stashes; x_out/h_out required
  long ldxo;              // leading dimension of x_out
  long ld_c, ld_o;        // leading dimensions of a_out / y_out and of o_out
  int l_accumulate;       // l_out += instead of =
  int stamp_base;         // diagnostics (lfi_debug_set_stamps): slot of this cell's first phase stamp + 1, 0 = none (rev_fast_cell)
  int state_l2;           // reverse cell: read h_prev / c_prev with L1-bypassing (sc1) loads - the persistent reverse walk re-reads
                          // the state its own workgroup stored one timestep earlier, with no kernel boundary in between
  const int* role;        // row-masked cells (flow_rows_chain_kernel) only: one word per batch row, != 0 = the row observes
  int role_want;          // ... and the role this cell stores for (0: generating rows, 1: observing rows); other rows are never stored
};

extern __shared__ __attribute__((aligned(16))) float flow_smem[];

__device__ __forceinline__ int rup16(int x) { return (x + 15) & ~15; }

// The rows of the 16-row tile at b0 that a row-masked cell stores: bit i = row b0 + i is inside the batch and has the role `want`.
// The same for every thread of the workgroup (a uniform read of the tile's 16 role words).
__device__ __forceinline__ unsigned tile_live_rows(const int* role, int want, int b0, int rows) {
  unsigned m = 0u;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int row = b0 + i;
    if (row < rows && (role[row] != 0) == (want != 0)) m |= 1u << i;
  }
  return m;
}

// ---- shared phase: coupling net given z1 (Zt) and h_prev (Ht) in LDS -> new hidden (Hn, LDS) and o (Orm, LDS)
__device__ __forceinline__ void coupling_net_phase(const FlowK& f, const CellIO& io, int b0, const float* Zt, const float* Ht,
                                                   float* Hn, float* Orm, int tid) {
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int k = io.k, H = f.H, G = f.G, Ch = f.Ch, Cout = f.Cout;
  const float* wz = f.wz_t + (long)k * Ch * G;
  const float* wh = f.whh_t + (long)k * H * G;
  const float* bhh = f.p.b_hh + (long)k * G;
  const int nht = (H + 15) >> 4;
  if (f.lstm) {
    // torch.nn.LSTMCell (gate order i, f, g, o) from zero (h, c) at the first modelled frame (glow/models.py:181-185,
    // 209-213; the reference's own call crashes there, SURVEY.md finding 2: semantics = zero initial state)
    for (int t = wave; t < nht; t += NW) {
      const int j = t * 16 + l15;
      const bool jok = j < H;
      f32x4 gz[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      mma16_pf<4>(gz, Zt, LT, wz + t * 16, G, H, Ch, jok, lane);
      f32x4 gh[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      mma16_pf<4>(gh, Ht, LT, wh + t * 16, G, H, H, jok, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lq * 4 + r;
        const int row = b0 + i;
        float hnew = 0.0f;
        if (row < io.rows && jok) {
          const float* gc = io.gic + (long)row * G;
          const float ii = sigmoidf_(gz[0][r] + gh[0][r] + gc[j] + bhh[j]);
          const float ff = sigmoidf_(gz[1][r] + gh[1][r] + gc[H + j] + bhh[H + j]);
          const float gg = tanhf_(gz[2][r] + gh[2][r] + gc[2 * H + j] + bhh[2 * H + j]);
          const float oo = sigmoidf_(gz[3][r] + gh[3][r] + gc[3 * H + j] + bhh[3 * H + j]);
          const float cp = io.c_prev ? io.c_prev[(long)row * H + j] : 0.0f;
          const float c2 = ff * cp + ii * gg;
          hnew = oo * tanhf_(c2);
          io.h_out[(long)row * H + j] = hnew;
          io.c_out[(long)row * H + j] = c2;
          if (io.g_out) {
            float* gs = io.g_out + (long)row * 4 * H;
            *reinterpret_cast<f32x4*>(gs + 4 * j) = (f32x4){ii, ff, gg, oo};   // gate-interleaved stash: one 16-byte store
          }
        }
        if (jok) Hn[j * LT + i] = hnew;
      }
    }
  } else
  for (int t = wave; t < nht; t += NW) {
    const int j = t * 16 + l15;
    const bool jok = j < H;
    // input side (z1 part; the conditioning part was hoisted into gic): r, z, n chains share the A operand
    f32x4 gz[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    mma16_pf<3>(gz, Zt, LT, wz + t * 16, G, H, Ch, jok, lane);
    // hidden side
    f32x4 gh[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    mma16_pf<3>(gh, Ht, LT, wh + t * 16, G, H, H, jok, lane);
    const f32x4 ar = gz[0] + gh[0], au = gz[1] + gh[1], ain = gz[2], ahn = gh[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = lq * 4 + r;
      const int row = b0 + i;
      float hnew = 0.0f;
      if (row < io.rows && jok) {
        const float* gc = io.gic + (long)row * G;
        const float rr = sigmoidf_(ar[r] + gc[j] + bhh[j]);
        const float uu = sigmoidf_(au[r] + gc[H + j] + bhh[H + j]);
        const float ghn = ahn[r] + bhh[2 * H + j];
        const float nn = tanhf_(ain[r] + gc[2 * H + j] + rr * ghn);
        const float hp = Ht[j * LT + i];
        hnew = (1.0f - uu) * nn + uu * hp;
        io.h_out[(long)row * H + j] = hnew;
        if (io.g_out) {
          float* gs = io.g_out + (long)row * 4 * H;
          *reinterpret_cast<f32x4*>(gs + 4 * j) = (f32x4){rr, uu, nn, ghn};
        }
      }
      if (jok) Hn[j * LT + i] = hnew;
    }
  }
  __syncthreads();
  // o = (h' Wfl^T + b) * exp(3 logs)    (LinearZeros, glow/modules.py:93-95)
  const float* wf = f.wfl_t + (long)k * H * Cout;
  const float* bfl = f.p.b_fl + (long)k * Cout;
  const float* lfl = f.p.l_fl + (long)k * Cout;
  const int not_ = (Cout + 15) >> 4;
  const int ldo = Cout + 1;
  for (int t = wave; t < not_; t += NW) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = tile16_lds_glb(acc, Hn, LT, wf + t * 16, Cout, H, min(16, Cout - t * 16), lane);
    const int col = t * 16 + l15;
    if (col < Cout) {
      const float bb = bfl[col], sc = expf(3.0f * lfl[col]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lq * 4 + r;
        const int row = b0 + i;
        const float o = (acc[r] + bb) * sc;
        Orm[i * ldo + col] = o;
        if (io.o_out && row < io.rows) io.o_out[(long)row * io.ld_o + col] = o;
      }
    }
  }
  __syncthreads();
}

// LDS carve for the cell kernels (floats). Every k-major block is [dim][LT].
struct Carve {
  int At, Ht, Zt, Hn, Yrm, Orm, Lg, total;
};
__host__ __device__ inline Carve carve_fwd(int C, int H, int Ch, int C2, int Cout) {
  Carve c;
  int o = 0;
  c.At = o; o += C * LT;
  c.Ht = o; o += H * LT;
  c.Zt = o; o += (Ch > 0 ? Ch : 1) * LT;
  c.Hn = o; o += H * LT;
  c.Yrm = o; o += MB * (C + 1);
  c.Orm = o; o += MB * (Cout + 1);
  c.Lg = o; o += MB * (C2 + 1);
  c.total = o;
  return c;
}

// ------------------------------------------------------------------------------------------- forward cell
__device__ void cell_forward(const FlowK& f, const CellIO& io, int b0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, k = io.k;
  const Carve cv = carve_fwd(C, H, Ch, C2, Cout);
  float* At = flow_smem + cv.At;
  float* Ht = flow_smem + cv.Ht;
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  float* Lg = flow_smem + cv.Lg;
  const int ldy = C + 1, ldo = Cout + 1, ldl = C2 + 1;

  // P0: actnorm (glow/modules.py:45-52), stage a and h_prev k-major
  const float* anb = f.p.an_bias + (long)k * C;
  const float* anl = f.p.an_logs + (long)k * C;
  for (int idx = tid; idx < MB * C; idx += NT) {
    const int i = idx / C, c = idx - i * C;
    const int row = b0 + i;
    float a = 0.0f;
    if (row < io.rows) {
      a = (io.x_in[(long)row * io.ldx + c] + anb[c]) * expf(anl[c]);
      if (io.a_out) io.a_out[(long)row * io.ld_c + c] = a;
    }
    At[c * LT + i] = a;
  }
  for (int idx = tid; idx < MB * H; idx += NT) {
    const int i = idx / H, j = idx - i * H;
    const int row = b0 + i;
    Ht[j * LT + i] = (io.h_prev && row < io.rows) ? io.h_prev[(long)row * H + j] : 0.0f;
  }
  __syncthreads();

  // P1: y = a W   (InvertibleConv1x1.forward, glow/modules.py:186; row-vector convention)
  {
    const float* W = f.W + (long)k * C * C;
    const int nt = (C + 15) >> 4;
    for (int t = wave; t < nt; t += NW) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile16_lds_glb(acc, At, LT, W + t * 16, C, C, min(16, C - t * 16), lane);
      const int c = t * 16 + l15;
      if (c < C) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const int row = b0 + i;
          const float v = acc[r];
          Yrm[i * ldy + c] = v;
          if (c < Ch) Zt[c * LT + i] = v;
          if (io.y_out && row < io.rows) io.y_out[(long)row * io.ld_c + c] = v;
        }
      }
    }
  }
  __syncthreads();

  // P2 + P3: coupling net
  coupling_net_phase(f, io, b0, Zt, Ht, Hn, Orm, tid);

  // P4: coupling (glow/models.py:330-341) and pass-through half
  for (int idx = tid; idx < MB * C2; idx += NT) {
    const int i = idx / C2, jj = idx - i * C2;
    const int row = b0 + i;
    const float z2 = Yrm[i * ldy + Ch + jj];
    float z2n, lg = 0.0f;
    if (f.affine) {
      const float shift = Orm[i * ldo + 2 * jj];
      const float sraw = sigmoidf_(Orm[i * ldo + 2 * jj + 1] + 2.0f);
      const float sc = fmaxf(sraw, f.eps);
      z2n = (z2 + shift) * sc;
      lg = logf(sc);
    } else {
      z2n = z2 + Orm[i * ldo + jj];
    }
    Lg[i * ldl + jj] = lg;
    if (row < io.rows) io.x_out[(long)row * io.ldxo + Ch + jj] = z2n;
  }
  for (int idx = tid; idx < MB * Ch; idx += NT) {
    const int i = idx / Ch, c = idx - i * Ch;
    const int row = b0 + i;
    if (row < io.rows) io.x_out[(long)row * io.ldxo + c] = Yrm[i * ldy + c];
  }
  __syncthreads();
  if (tid < MB && io.l_out) {
    const int row = b0 + tid;
    if (row < io.rows) {
      float s = 0.0f;
      for (int jj = 0; jj < C2; ++jj) s += Lg[tid * ldl + jj];
      if (io.l_accumulate) io.l_out[row] += s; else io.l_out[row] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------- reverse cell
// FlowStep.reverse_flow (glow/models.py:345-373): coupling^-1 -> invconv^-1 -> actnorm^-1.
__device__ void cell_reverse(const FlowK& f, const CellIO& io, int b0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, k = io.k;
  const Carve cv = carve_fwd(C, H, Ch, C2, Cout);
  float* Yt = flow_smem + cv.At;   // y = [z1 | z2] k-major for the W^-1 product
  float* Ht = flow_smem + cv.Ht;
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  float* Lg = flow_smem + cv.Lg;
  const int ldy = C + 1, ldo = Cout + 1, ldl = C2 + 1;

  for (int idx = tid; idx < MB * C; idx += NT) {
    const int i = idx / C, c = idx - i * C;
    const int row = b0 + i;
    const float v = row < io.rows ? io.x_in[(long)row * io.ldx + c] : 0.0f;
    Yrm[i * ldy + c] = v;
    if (c < Ch) { Zt[c * LT + i] = v; Yt[c * LT + i] = v; }
  }
  for (int idx = tid; idx < MB * H; idx += NT) {
    const int i = idx / H, j = idx - i * H;
    const int row = b0 + i;
    Ht[j * LT + i] = (io.h_prev && row < io.rows) ? io.h_prev[(long)row * H + j] : 0.0f;
  }
  __syncthreads();
  coupling_net_phase(f, io, b0, Zt, Ht, Hn, Orm, tid);
  for (int idx = tid; idx < MB * C2; idx += NT) {
    const int i = idx / C2, jj = idx - i * C2;
    const float z2n = Yrm[i * ldy + Ch + jj];
    float z2, lg = 0.0f;
    if (f.affine) {
      const float shift = Orm[i * ldo + 2 * jj];
      const float sraw = sigmoidf_(Orm[i * ldo + 2 * jj + 1] + 2.0f);
      const float sc = fmaxf(sraw, f.eps);
      z2 = z2n / sc;
      z2 = z2 - shift;
      lg = -logf(sc);
    } else {
      z2 = z2n - Orm[i * ldo + jj];
    }
    Lg[i * ldl + jj] = lg;
    Yt[(Ch + jj) * LT + i] = z2;
  }
  __syncthreads();
  {
    const float* Wi = f.Winv + (long)k * C * C;
    const float* anb = f.p.an_bias + (long)k * C;
    const float* anl = f.p.an_logs + (long)k * C;
    const int nt = (C + 15) >> 4;
    for (int t = wave; t < nt; t += NW) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile16_lds_glb(acc, Yt, LT, Wi + t * 16, C, C, min(16, C - t * 16), lane);
      const int c = t * 16 + l15;
      if (c < C) {
        const float es = expf(-anl[c]), bb = anb[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = b0 + lq * 4 + r;
          if (row < io.rows) io.x_out[(long)row * io.ldxo + c] = acc[r] * es - bb;  // scale then center (modules.py:76-79)
        }
      }
    }
  }
  if (tid < MB && io.l_out) {
    const int row = b0 + tid;
    if (row < io.rows) {
      float s = 0.0f;
      for (int jj = 0; jj < C2; ++jj) s += Lg[tid * ldl + jj];
      if (io.l_accumulate) io.l_out[row] += s; else io.l_out[row] = s;
    }
  }
}

// flow_nll_kernel's tile (lfi_flow.hip): frames per workgroup, and the widest row it stages through LDS
constexpr int NLL_FR = 64, NLL_CMAX = 128;

// ------------------------------------------------------------------------------------------- register-resident cells
// Same cells for the common sizes (C <= 64, H <= 128): the generic kernels above stream every weight chunk from L2 inside
// the dependent MFMA chains (4 phases x ~10 chunk round trips per cell: ~54 % of a wave's life is s_waitcnt, rocprof
// PMC). Weights do not depend on the data, so here each wave issues the loads of ITS slice of a phase's weights one phase
// ahead, into registers (<= 136 VGPRs), from zero-padded images made by lfi_flow_prep, and the k loops run MFMA-paced
// from registers + LDS. Image layout = MFMA B-fragment order in blocks of 16 k: element (k, column) of a K x J operand
// sits at (((k / 16) * 4 + k % 4) * J16 + column) * 4 + (k / 4) % 4, so the four k-steps of a block are ONE 16-byte load
// per lane and a wave-load is four 256-byte segments (dword-per-lane loads spent 12k cycles per cell in issue alone,
// s_memtime stamps). K and J are padded to 16 with zeros: no bounds checks. Elementwise phases use a fixed
// (row = tid / 32, column = tid % 32 [+ 32]) thread map: no integer divisions, 128-byte row segments.
#define LFI_STAMP(slot)                                                                                  \
  do {                                                                                                   \
    if (f.stamps && tid == 0 && bt == 0) f.stamps[cell * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

constexpr int FB_C = 4;   // blocks of 16 k over C    <= 64
constexpr int FB_Z = 2;   //                 over Ch   <= 32
constexpr int FB_H = 8;   //                 over H    <= 128
constexpr int FB_O = 4;   //                 over Cout <= 64

__host__ __device__ inline bool flow_fast_ok(int C, int H, int Cout) { return C <= 64 && H <= 128 && Cout <= 64; }
__host__ __device__ inline long flow_img_index(int k, int col, int J) {
  return ((long)((k >> 4) * 4 + (k & 3)) * J + col) * 4 + ((k >> 2) & 3);
}

// Workgroup -> (cell, batch tile). Workgroups are dealt round-robin over the 8 XCDs (block b and b + 8 share one), and every
// cell of a diagonal needs its own 270 KB of weights: give each XCD a contiguous run of (cell, tile) pairs so that a cell's
// 16 batch tiles (and the same flow step on the next diagonal) hit the same 4 MB L2 instead of all 8 L2s holding all 16
// steps' weights (4.3 MB: thrashing). Bijective for any grid size; speed only, never correctness.
__device__ __forceinline__ void flow_cell_of_block(int nbt, int* cell, int* bt) {
  const int total = gridDim.x * gridDim.y;
  int bid = blockIdx.x + gridDim.x * blockIdx.y;
  const int q = total >> 3, r = total & 7, xcd = bid & 7, idx = bid >> 3;
  bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  *cell = bid / nbt;
  *bt = bid - *cell * nbt;
}

struct CarveF {
  int At, Ht, Zt, Hn, Yrm, Orm, total;
};
__host__ __device__ inline CarveF carve_fast_fwd(int C, int C16, int H16, int Ch16, int Cout) {
  CarveF c;
  int o = 0;
  c.At = o; o += C16 * LT;
  c.Ht = o; o += H16 * LT;
  c.Zt = o; o += Ch16 * LT;
  c.Hn = o; o += H16 * LT;
  c.Yrm = o; o += MB * (C + 1);
  c.Orm = o; o += MB * (Cout + 1);
  c.total = o;
  return c;
}

// sum over nb blocks of 16 k: A(16 x 16 nb) from LDS (k-major: a_lane = a_lds + kq * LT + l15, element k at + k * LT) times
// the register-resident B slice w[b] (components e: k = 16 b + 4 e + kq). Two interleaved chains (40-cycle dependent latency
// against a 32-cycle issue).
template <int MAXB>
__device__ __forceinline__ f32x4 mma16_reg(const float* a_lane, const f32x4 (&w)[MAXB], int nb) {
  f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < MAXB; ++b)
    if (b < nb) {
      const float* ab = a_lane + b * 16 * LT;
      const float a0 = ab[0], a1 = ab[4 * LT], a2 = ab[8 * LT], a3 = ab[12 * LT];
      e = mfma16(a0, w[b][0], e);
      o = mfma16(a1, w[b][1], o);
      e = mfma16(a2, w[b][2], e);
      o = mfma16(a3, w[b][3], o);
    }
  return e + o;
}

// this lane's slice of one 16-column tile of an image: nb float4 (k blocks), image row pitch J (columns, multiple of 16)
template <int MAXB>
__device__ __forceinline__ void load_frag(f32x4 (&w)[MAXB], const float* __restrict__ img, int J, int col, int kq, int nb,
                                          bool on) {
  const f32x4* p = reinterpret_cast<const f32x4*>(img) + (long)kq * J + col;
#pragma unroll
  for (int b = 0; b < MAXB; ++b)
    if (on && b < nb) w[b] = p[(long)b * 4 * J];
}

// ---- bf16 x 3 form of the recurrent products (persistent walk, engine_precision bf16x3). The f32-input MFMA the cells use
// everywhere else runs at 1/16 of the bf16 rate, and with flow step k's weights resident the recurrent cell's
// (z1, h) x (W_ih[:, :Ch], W_hh) product is what a pipeline step waits for (46 % of a forward step, tools/pipe_stamps.py).
// Same split as the GEMMs: x = hi + lo in bf16, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 into fp32 accumulators.
// No new weight images: two consecutive 16-k blocks of the f32 fragment registers (components e: k = 16 b + 4 e + kq) are
// split in registers once per launch into one 32-k bf16 fragment, slot i of lane group kq standing for
// k = 32 B + 16 (i >> 2) + 4 (i & 3) + kq - any bijection does as long as the A operand uses the same one, and this one
// makes the A side exactly the LDS reads the f32 path already does.
typedef __bf16 fbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 fbf16x2 __attribute__((ext_vector_type(2)));
typedef float ffloat2 __attribute__((ext_vector_type(2)));
struct X3Frag { fbf16x8 hi, lo; };
__device__ __forceinline__ void x3_split2(float a, float b, unsigned* hi, unsigned* lo) {
  const fbf16x2 h = __builtin_convertvector((ffloat2){a, b}, fbf16x2);
  const unsigned hb = __builtin_bit_cast(unsigned, h);
  const float ha = __builtin_bit_cast(float, hb << 16), hbv = __builtin_bit_cast(float, hb & 0xffff0000u);
  const fbf16x2 l = __builtin_convertvector((ffloat2){a - ha, b - hbv}, fbf16x2);
  *hi = hb;
  *lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ X3Frag x3_pack(const f32x4& b0, const f32x4& b1) {
  uint4 h, l;
  x3_split2(b0[0], b0[1], &h.x, &l.x);
  x3_split2(b0[2], b0[3], &h.y, &l.y);
  x3_split2(b1[0], b1[1], &h.z, &l.z);
  x3_split2(b1[2], b1[3], &h.w, &l.w);
  X3Frag r;
  r.hi = __builtin_bit_cast(fbf16x8, h);
  r.lo = __builtin_bit_cast(fbf16x8, l);
  return r;
}
// A fragment of 32 k from a k-major LDS operand: the eight reads of two f32 blocks
__device__ __forceinline__ X3Frag x3_a(const float* ab) {
  f32x4 b0 = {ab[0], ab[4 * LT], ab[8 * LT], ab[12 * LT]};
  const float* a1 = ab + 16 * LT;
  f32x4 b1 = {a1[0], a1[4 * LT], a1[8 * LT], a1[12 * LT]};
  return x3_pack(b0, b1);
}
__device__ __forceinline__ f32x4 x3_mma(const X3Frag& a, const X3Frag& w, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, w.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, w.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, w.hi, acc, 0, 0, 0);
  return acc;
}

// ---- the same with fp16 pieces (11 + 11 mantissa bits: 2^-22 relative, fp32-grade) for the SAMPLER's reverse cells. Their
// operands - h in (-1, 1), flow activations, trained weights - sit far inside fp16's range (a value beyond 65504 turns into
// inf - inf = NaN: loud, as the exact path is at 3e38; tiny values lose nothing that matters: fp16's subnormal spacing, 6e-8,
// is the absolute error of an fp32 near 1). Gradients do not qualify (1e-10 underflows), so every backward product and the
// training walks keep bf16 pieces. Same MFMA rate, same register footprint as bf16 x 3.
typedef _Float16 fh16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 fh16x2 __attribute__((ext_vector_type(2)));
struct X3FragH { fh16x8 hi, lo; };
__device__ __forceinline__ void x3h_split2(float a, float b, unsigned* hi, unsigned* lo) {
  const fh16x2 h = __builtin_convertvector((ffloat2){a, b}, fh16x2);
  const ffloat2 hf = __builtin_convertvector(h, ffloat2);
  const fh16x2 l = __builtin_convertvector((ffloat2){a - hf[0], b - hf[1]}, fh16x2);
  *hi = __builtin_bit_cast(unsigned, h);
  *lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ X3FragH x3h_pack(const f32x4& b0, const f32x4& b1) {
  uint4 h, l;
  x3h_split2(b0[0], b0[1], &h.x, &l.x);
  x3h_split2(b0[2], b0[3], &h.y, &l.y);
  x3h_split2(b1[0], b1[1], &h.z, &l.z);
  x3h_split2(b1[2], b1[3], &h.w, &l.w);
  X3FragH r;
  r.hi = __builtin_bit_cast(fh16x8, h);
  r.lo = __builtin_bit_cast(fh16x8, l);
  return r;
}
__device__ __forceinline__ X3FragH x3h_a(const float* ab) {
  f32x4 b0 = {ab[0], ab[4 * LT], ab[8 * LT], ab[12 * LT]};
  const float* a1 = ab + 16 * LT;
  f32x4 b1 = {a1[0], a1[4 * LT], a1[8 * LT], a1[12 * LT]};
  return x3h_pack(b0, b1);
}
__device__ __forceinline__ f32x4 x3h_mma(const X3FragH& a, const X3FragH& w, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, w.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, w.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, w.hi, acc, 0, 0, 0);
  return acc;
}

// this lane's fragments of one 16-column tile of a pre-split backward image: nb2 32-k blocks of gate g
template <int MAXB2>
__device__ __forceinline__ void x3_load(X3Frag (&w)[MAXB2], const uint4* __restrict__ img, long per, int g, int nB, int J, int col,
                                        int kq, int nb2, bool on) {
  const uint4* p = img + (((long)g * nB) * J + col) * 4 + kq;
#pragma unroll
  for (int b = 0; b < MAXB2; ++b)
    if (on && b < nb2) {
      w[b].hi = __builtin_bit_cast(fbf16x8, p[(long)b * J * 4]);
      w[b].lo = __builtin_bit_cast(fbf16x8, p[(long)b * J * 4 + per]);
    }
}
// sum over NG gate blocks of nb2 32-k blocks each (A: k-major LDS operand, gate stride blk floats)
template <int NG, int MAXB2>
__device__ __forceinline__ f32x4 x3_mma_gates(const float* a_lane, int blk, const X3Frag (&w)[NG][MAXB2], int nb2) {
  f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int b = 0; b < MAXB2; ++b)
      if (b < nb2) {
        const X3Frag a = x3_a(a_lane + g * blk + b * 32 * LT);
        if ((g * MAXB2 + b) & 1) o = x3_mma(a, w[g][b], o);
        else e = x3_mma(a, w[g][b], e);
      }
  return e + o;
}

// The backward cell's MFMA operands d(gate pre-activations) are needed by all eight waves: instead of every wave splitting the
// same fp32 LDS values again (24 blocks x ~30 VALU per wave and timestep - it bound Q2 once the MFMAs were bf16), the wave
// that computes a value stores its bf16 hi and lo ONCE, row-major [16 rows][NG * H16 + 8], the column of hidden unit j of
// gate g at g * H16 + x3_pos(j): within a 32-k block the slot order of x3_a, so a lane's 8 k are one 16-byte read.
__device__ __forceinline__ int x3_pos(int j) { return (j & ~31) | ((j & 3) << 3) | ((j >> 2) & 7); }
__device__ __forceinline__ void x3_put(__bf16* hi_img, __bf16* lo_img, int idx, float v) {
  const __bf16 h = (__bf16)v;
  hi_img[idx] = h;
  lo_img[idx] = (__bf16)(v - (float)h);
}
template <int NG, int MAXB2>
__device__ __forceinline__ f32x4 x3_mma_gates_img(const __bf16* hi_row, const __bf16* lo_row, int H16, const X3Frag (&w)[NG][MAXB2],
                                                  int nb2) {
  f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int b = 0; b < MAXB2; ++b)
      if (b < nb2) {
        X3Frag a;
        a.hi = *reinterpret_cast<const fbf16x8*>(hi_row + g * H16 + b * 32);
        a.lo = *reinterpret_cast<const fbf16x8*>(lo_row + g * H16 + b * 32);
        if ((g * MAXB2 + b) & 1) o = x3_mma(a, w[g][b], o);
        else e = x3_mma(a, w[g][b], e);
      }
  return e + o;
}

// P2 of a register-resident cell: the coupling net's recurrent cell on this wave's 16 hidden units. Zt / Ht: z1 and
// h_prev in LDS (k-major), Hn: new state (LDS), h_out / c_out / g_out: row-0 pointers of the (rows x H) / (rows x 4H) outputs
// (g_out may be null).
// gate math + stores of P2 on this wave's 16 hidden units, given the two accumulated products (az: z1 side, ah: h side)
// RM (row-masked cells): h_out / c_out are stored for the rows of `live` only (tile_live_rows), not for every row inside the batch.
// CST = false (the frame loop of fwd_chain_cell): c_out is not stored here - the caller keeps the cell state in cnew and stores it itself.
template <int NG, bool RM = false, bool CST = true>
__device__ __forceinline__ void fast_cell_p2_gates(const FlowK& f, const float* Ht, float* Hn, const f32x4 (&az)[NG],
                                                   const f32x4 (&ah)[NG], const float (&gc)[4][NG], const float (&bh)[NG],
                                                   const float (&cprev)[4], int j2, int kq, int b0, int rows, float* h_out,
                                                   float* c_out, float* g_out, float* cnew, __bf16* img_hi = nullptr,
                                                   __bf16* img_lo = nullptr, int img_ld = 0, int img_col = 0, unsigned live = 0u) {
  const int H = f.H;
  if (j2 < H) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = kq * 4 + r;
      const int row = b0 + i;
      const bool rs = RM ? ((live >> i) & 1u) != 0u : row < rows;   // this row's results go to memory
      float hnew;
      float gs0, gs1, gs2, gs3;
      if (NG == 3) {  // torch.nn.GRUCell, gate order r, z, n
        const float rr = sigmoidf_(az[0][r] + ah[0][r] + gc[r][0] + bh[0]);
        const float uu = sigmoidf_(az[1][r] + ah[1][r] + gc[r][1] + bh[1]);
        const float ghn = ah[2][r] + bh[2];
        // (explicit fused forms: left to -ffp-contract, "(1 - z) n + z h" fuses either product, and which one depended on the
        // kernel this function was inlined into - the persistent walk and the diagonal walk then differed by an ulp)
        const float nn = tanhf_(__builtin_fmaf(rr, ghn, az[2][r] + gc[r][2]));
        const float hp = Ht[j2 * LT + i];
        hnew = __builtin_fmaf(uu, hp, (1.0f - uu) * nn);
        gs0 = rr; gs1 = uu; gs2 = nn; gs3 = ghn;
      } else {        // torch.nn.LSTMCell, gate order i, f, g, o; zero (h, c) at the first modelled frame
        const float ii = sigmoidf_(az[0][r] + ah[0][r] + gc[r][0] + bh[0]);
        const float ff = sigmoidf_(az[1][r] + ah[1][r] + gc[r][1] + bh[1]);
        const float gg = tanhf_(az[2][r] + ah[2][r] + gc[r][2] + bh[2]);
        const float oo = sigmoidf_(az[NG - 1][r] + ah[NG - 1][r] + gc[r][NG - 1] + bh[NG - 1]);
        const float c2 = __builtin_fmaf(ff, cprev[r], ii * gg);
        hnew = oo * tanhf_(c2);
        if (CST && rs) c_out[(long)row * H + j2] = c2;
        if (cnew) cnew[r] = c2;
        gs0 = ii; gs1 = ff; gs2 = gg; gs3 = oo;
      }
      Hn[j2 * LT + i] = hnew;
      if (img_hi) x3_put(img_hi, img_lo, i * img_ld + img_col + x3_pos(j2), hnew);   // bf16 hi / lo image for the next cell's product
      if (rs) {
        if (h_out) h_out[(long)row * H + j2] = hnew;   // (null: the caller stores the tile's rows itself, 16 bytes at a time)
        if (g_out) {
          // the four stashed gate values of (row, hidden unit) lie together: ONE 16-byte store here and one 16-byte load in the
          // backward cell instead of four dword accesses each (the walks are bound by vector-memory instruction issue:
          // without the P2 stash stores the forward walk ran 11 % faster)
          *reinterpret_cast<f32x4*>(g_out + (long)row * 4 * H + 4 * j2) = (f32x4){gs0, gs1, gs2, gs3};
        }
      }
    }
  }
}

template <int NG>
__device__ __forceinline__ void fast_cell_p2(const FlowK& f, const float* Zt, const float* Ht, float* Hn,
                                             const f32x4 (&wz)[NG][FB_Z], const f32x4 (&wh)[NG][FB_H], const float (&gc)[4][NG],
                                             const float (&bh)[NG], const float (&cprev)[4], int nbZ, int nbH, int j2, int kq,
                                             int l15, int b0, int rows, float* h_out, float* c_out, float* g_out,
                                             float* cnew = nullptr) {
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float* zl = Zt + kq * LT + l15;
  const float* hl = Ht + kq * LT + l15;
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
  fast_cell_p2_gates<NG>(f, Ht, Hn, az, ah, gc, bh, cprev, j2, kq, b0, rows, h_out, c_out, g_out, cnew);
}

// The same cell with its A operand (z1 | h_{t-1}) read from bf16 hi / lo LDS images the PRODUCERS wrote (P1 for z1, the previous
// timestep's gate epilogue for h: x3_put, slot order x3_pos): one 16-byte read per 32-k block and plane instead of eight
// 4-byte reads of the k-major fp32 images plus a split redone by all eight waves (stamps: 2.8 k of the 5.8 k cycles of P2).
template <int NG>
__device__ __forceinline__ void fast_cell_p2_x3_img(const FlowK& f, const __bf16* ih, const __bf16* il, int ldx, int Ch16,
                                                    const float* Ht, float* Hn, const X3Frag (&wz)[NG][FB_Z / 2],
                                                    const X3Frag (&wh)[NG][FB_H / 2], const float (&gc)[4][NG],
                                                    const float (&bh)[NG], const float (&cprev)[4], int nbZ2, int nbH2, int j2,
                                                    int kq, int l15, int b0, int rows, float* h_out, float* c_out, float* g_out,
                                                    float* cnew, __bf16* ihn, __bf16* iln) {
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const __bf16* rh = ih + l15 * ldx + 8 * kq;
  const __bf16* rl = il + l15 * ldx + 8 * kq;
#pragma unroll
  for (int b = 0; b < FB_Z / 2; ++b)
    if (b < nbZ2) {
      X3Frag a;
      a.hi = *reinterpret_cast<const fbf16x8*>(rh + b * 32);
      a.lo = *reinterpret_cast<const fbf16x8*>(rl + b * 32);
#pragma unroll
      for (int g = 0; g < NG; ++g) az[g] = x3_mma(a, wz[g][b], az[g]);
    }
#pragma unroll
  for (int b = 0; b < FB_H / 2; ++b)
    if (b < nbH2) {
      X3Frag a;
      a.hi = *reinterpret_cast<const fbf16x8*>(rh + Ch16 + b * 32);
      a.lo = *reinterpret_cast<const fbf16x8*>(rl + Ch16 + b * 32);
#pragma unroll
      for (int g = 0; g < NG; ++g) ah[g] = x3_mma(a, wh[g][b], ah[g]);
    }
  fast_cell_p2_gates<NG>(f, Ht, Hn, az, ah, gc, bh, cprev, j2, kq, b0, rows, h_out, c_out, g_out, cnew, ihn, iln, ldx, Ch16);
}

// bf16 x 3 form: weights as packed 32-k fragments (x3_pack), nbZ2 / nbH2 = number of 32-k blocks
template <int NG>
__device__ __forceinline__ void fast_cell_p2_x3(const FlowK& f, const float* Zt, const float* Ht, float* Hn,
                                                const X3Frag (&wz)[NG][FB_Z / 2], const X3Frag (&wh)[NG][FB_H / 2],
                                                const float (&gc)[4][NG], const float (&bh)[NG], const float (&cprev)[4], int nbZ2,
                                                int nbH2, int j2, int kq, int l15, int b0, int rows, float* h_out, float* c_out,
                                                float* g_out, float* cnew) {
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float* zl = Zt + kq * LT + l15;
  const float* hl = Ht + kq * LT + l15;
#pragma unroll
  for (int b = 0; b < FB_Z / 2; ++b)
    if (b < nbZ2) {
      const X3Frag a = x3_a(zl + b * 32 * LT);
#pragma unroll
      for (int g = 0; g < NG; ++g) az[g] = x3_mma(a, wz[g][b], az[g]);
    }
#pragma unroll
  for (int b = 0; b < FB_H / 2; ++b)
    if (b < nbH2) {
      const X3Frag a = x3_a(hl + b * 32 * LT);
#pragma unroll
      for (int g = 0; g < NG; ++g) ah[g] = x3_mma(a, wh[g][b], ah[g]);
    }
  fast_cell_p2_gates<NG>(f, Ht, Hn, az, ah, gc, bh, cprev, j2, kq, b0, rows, h_out, c_out, g_out, cnew);
}

// fp16 x 3 form (x3h_*): the sampler's reverse cells
template <int NG>
__device__ __forceinline__ void fast_cell_p2_x3h(const FlowK& f, const float* Zt, const float* Ht, float* Hn,
                                                 const X3FragH (&wz)[NG][FB_Z / 2], const X3FragH (&wh)[NG][FB_H / 2],
                                                 const float (&gc)[4][NG], const float (&bh)[NG], const float (&cprev)[4], int nbZ2,
                                                 int nbH2, int j2, int kq, int l15, int b0, int rows, float* h_out, float* c_out,
                                                 float* g_out, float* cnew) {
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float* zl = Zt + kq * LT + l15;
  const float* hl = Ht + kq * LT + l15;
#pragma unroll
  for (int b = 0; b < FB_Z / 2; ++b)
    if (b < nbZ2) {
      const X3FragH a = x3h_a(zl + b * 32 * LT);
#pragma unroll
      for (int g = 0; g < NG; ++g) az[g] = x3h_mma(a, wz[g][b], az[g]);
    }
#pragma unroll
  for (int b = 0; b < FB_H / 2; ++b)
    if (b < nbH2) {
      const X3FragH a = x3h_a(hl + b * 32 * LT);
#pragma unroll
      for (int g = 0; g < NG; ++g) ah[g] = x3h_mma(a, wh[g][b], ah[g]);
    }
  fast_cell_p2_gates<NG>(f, Ht, Hn, az, ah, gc, bh, cprev, j2, kq, b0, rows, h_out, c_out, g_out, cnew);
}

// P3: o = (h' Wfl^T + b) exp(3 logs) on this wave's 16 outputs   (LinearZeros, glow/modules.py:93-95); o_out may be null
// (bb, sc: LinearZeros bias and exp(3 logs) of this lane's output column, loaded by the caller OUTSIDE its dependent phases)
__device__ __forceinline__ void fast_cell_p3(const FlowK& f, int k, const float* Hn, float* Orm, const f32x4 (&w3)[FB_H], int nbH,
                                             int col, int kq, int l15, int b0, int rows, float* o_out, long ld_out, float bb, float sc) {
  const int Cout = f.Cout, ldo = Cout + 1;
  const f32x4 acc = mma16_reg<FB_H>(Hn + kq * LT + l15, w3, nbH);
  if (col < Cout) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = kq * 4 + r;
      const int row = b0 + i;
      const float o = (acc[r] + bb) * sc;
      Orm[i * ldo + col] = o;
      if (o_out && row < rows) o_out[(long)row * ld_out + col] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------- persistent pipeline
// The diagonal walk (lfi_flow.hip) pays one launch + one reload of 270 KB of weights per workgroup for every one of the N + Ks - 1
// diagonals, although a workgroup's weights never change: cell (n, k) of batch tile bt always needs flow step k's. Here
// workgroup (k, bt) is PERSISTENT: it loads step k's weights into registers once, then walks n = 0 .. N-1 for its 16
// samples; the recurrent state h (and the LSTM cell state) never leaves the workgroup (LDS / registers), and the only
// inter-workgroup traffic is the 16 x C output tile handed from (k, bt) to (k + 1, bt): a systolic pipeline over the flow
// steps, N + Ks - 1 cell times end to end, one launch. Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility, form R1):
// the producer stores the tile write-through (sc1), every wave drains its stores, workgroup barrier, ONE lane publishes
// the progress counter with an agent-scope atomic store; the consumer polls that one word relaxed, ONE agent-scope acquire,
// barrier, then plain loads. Deadlock-free for ANY grid size and dispatch order: logical (k, bt) ids are dealt by an atomic
// ticket in arrival order and a workgroup only ever waits on a smaller ticket, i.e. on a workgroup that is already
// running (more workgroups than CUs simply run as successive groups of flow steps). Every spin is bounded: on timeout
// the abort word is set, every workgroup leaves its loop, and the host reports LFI_ERR_LAUNCH.
constexpr unsigned PIPE_HDR = 4;                 // ticket, abort, 2 reserved words
#ifndef LFI_PIPE_STRIDE
#define LFI_PIPE_STRIDE 32
#endif
constexpr unsigned PIPE_STRIDE = LFI_PIPE_STRIDE;   // words between two progress words of the persistent walks: one 128-byte line each (the polls of 256 workgroups
                                                    // on eight shared lines queued at one memory channel)
constexpr unsigned PIPE_WALK_HDR = PIPE_STRIDE > PIPE_HDR ? PIPE_STRIDE : PIPE_HDR;
constexpr unsigned PIPE_SPIN_LIMIT = 1u << 23;   // polls (each >= ~0.5 us) before giving up

__device__ __forceinline__ unsigned ld_agent(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned* p, unsigned v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// write-through (sc1) store of one payload element
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// load of one handed-off payload element: L1-bypassing (sc1) when the consumer did not fence
__device__ __forceinline__ float ld_tile(const float* p, bool fenced) {
  return fenced ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ONE lane: wait until *flag >= need. false = aborted (timeout here or in another workgroup).
__device__ __forceinline__ bool pipe_wait(const unsigned* flag, unsigned need, unsigned* abort_w) {
  unsigned spins = 0;
  while (ld_agent(flag) < need) {
    if ((++spins & 31u) == 0u) {
      if (ld_agent(abort_w) != 0u) return false;
      if (spins > PIPE_SPIN_LIMIT) {
        st_agent(abort_w, 1u);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(4);
  }
  return true;
}
// consumer side of a hand-off, all threads: thread 0 polls + acquires, the rest learn the outcome through LDS
__device__ __forceinline__ bool pipe_acquire(const unsigned* flag, unsigned need, unsigned* abort_w, int tid, int* s_ok,
                                             bool fence) {
  if (tid == 0) {
    const bool ok = pipe_wait(flag, need, abort_w);
    if (ok && fence) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  return *s_ok != 0;
}
// producer side, all threads: drain this wave's stores, barrier, one lane publishes
__device__ __forceinline__ void pipe_publish(unsigned* flag, unsigned value, int tid, bool signal) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (signal && tid == 0) st_agent(flag, value);
}

// as mma16_reg with the B fragments of this wave in LDS: wl[b * 64] is this lane's float4 of k block b (consecutive lanes
// read consecutive 16 bytes: conflict-free ds_read_b128)
__device__ __forceinline__ f32x4 mma16_lds(const float* a_lane, const f32x4* wl, int nb) {
  f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < nb; ++b) {
    const float* ab = a_lane + b * 16 * LT;
    const f32x4 w = wl[b * 64];
    const float a0 = ab[0], a1 = ab[4 * LT], a2 = ab[8 * LT], a3 = ab[12 * LT];
    e = mfma16(a0, w[0], e);
    o = mfma16(a1, w[1], o);
    e = mfma16(a2, w[2], e);
    o = mfma16(a3, w[3], o);
  }
  return e + o;
}
// LDS floats of the pipeline kernel: the cell's operands, then the W fragments of the C16/16 P1 waves and the Wfl fragments
// of the Co16/16 P3 waves (the recurrent weights W_ih[:, :Ch] and W_hh stay in registers: 120 VGPRs at H = 128)
__host__ __device__ inline int pipe_fwd_img_offset(int C, int C16, int H16, int Ch16, int Cout, int Co16) {
  const int base = (carve_fast_fwd(C, C16, H16, Ch16, Cout).total + 3) & ~3;
  return base + (C16 >> 4) * (C16 >> 4) * 256 + (Co16 >> 4) * (H16 >> 4) * 256;
}
// + the bf16 x 3 cell's operand images: two buffers (h of the previous / of this timestep) x {hi, lo} x MB rows of
// Ch16 + H16 + 8 bf16 (2 MB ldx floats)
__host__ __device__ inline int pipe_fwd_lds_floats(int C, int C16, int H16, int Ch16, int Cout, int Co16) {
  return pipe_fwd_img_offset(C, C16, H16, Ch16, Cout, Co16) + 2 * MB * (Ch16 + H16 + 8);
}

// diagnostics (lfi_debug_set_stamps): s_memtime of workgroup (Ks / 2, tile 0) at the phase boundaries of every timestep, in
// slots [4096 + 2048 * backward + 16 * n + phase] of the stamp buffer
#define PIPE_STAMP(dir, slot)                                                                                              \
  do {                                                                                                                     \
    if (f.stamps && tid == 0 && bt == 0 && k == f.stamp_k && n < 128)                                                       \
      f.stamps[4096 + 2048 * (dir) + 16 * n + (slot)] = __builtin_amdgcn_s_memtime();                                      \
  } while (0)

// ------------------------------------------------------------------------------------------- host helpers
// floats of the prep buffer up to the end of the scratch area (published layout + log-det parts + fp64 workspace)
inline long prep_scratch_end(const lfi_flow_dims* d) {
  const int Ch = d->C / 2, C2 = d->C - Ch, Cout = d->affine ? 2 * C2 : C2, G = (d->lstm ? 4 : 3) * d->H;
  const long cc = (long)d->Ks * d->C * d->C;
  long n = 3 * cc + (long)d->Ks * Ch * G + (long)d->Ks * d->H * G + (long)d->Ks * d->H * Cout + (long)d->Ks * G * d->D + 4;
  n += d->Ks + 4;
  n += 2 * ((long)d->Ks * 2 * d->C * d->C + (long)d->Ks * d->C) + 8;  // doubles, counted as 2 floats each
  return (n + 3) & ~3L;  // 16-byte aligned: the images behind it are read with dwordx4 loads
}
inline long prep_padded_floats(const lfi_flow_dims* d) {
  const int Ch = d->C / 2, C2 = d->C - Ch, Cout = d->affine ? 2 * C2 : C2, NG = d->lstm ? 4 : 3;
  auto r16 = [](int x) { return (long)((x + 15) & ~15); };
  const long C16 = r16(d->C), Ch16 = Ch ? r16(Ch) : 16, H16 = r16(d->H), Co16 = r16(Cout);
  return d->Ks * (3 * C16 * C16 + Ch16 * NG * H16 + H16 * NG * H16 + 2 * H16 * Co16 + NG * H16 * H16 + NG * H16 * Ch16)
         + d->Ks * (NG * H16 * H16 + NG * H16 * Ch16) + 8    // + the bf16 hi/lo fragment images of bwh / bwz (same byte counts)
         + d->Ks * (Ch16 * NG * H16 + H16 * NG * H16 + H16 * Co16 + C16 * C16) + 8;   // + the fp16 hi/lo images of pwz / pwh / pwfl / pWinv
}

// the sizes and widths that follow from dims alone (fill_flow; the host-only queries and flow_frame_plan, which have no params)
inline void flow_widths(const lfi_flow_dims* d, FlowK* f) {
  f->B = d->B; f->N = d->N; f->C = d->C; f->H = d->H; f->D = d->D; f->Ks = d->Ks;
  f->affine = d->affine; f->lstm = d->lstm; f->eps = d->scale_eps;
  f->Ch = d->C / 2; f->C2 = d->C - f->Ch; f->Cout = d->affine ? 2 * f->C2 : f->C2;
  f->G = (d->lstm ? 4 : 3) * d->H; f->I = f->Ch + d->D; f->F = d->N * d->B; f->nbt = lfi_cdiv(d->B, MB);
  f->NG = d->lstm ? 4 : 3;
  f->ldc = (f->C + 3) & ~3; f->ldo = (f->Cout + 3) & ~3;
  f->C16 = (f->C + 15) & ~15; f->Ch16 = (f->Ch + 15) & ~15; f->H16 = (f->H + 15) & ~15; f->Co16 = (f->Cout + 15) & ~15;
  if (f->Ch16 == 0) f->Ch16 = 16;
}

inline int fill_flow(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, FlowK* f, const char* who) {
  LFI_REQUIRE(d && p, "%s: null dims/params", who);
  LFI_REQUIRE(d->B > 0 && d->N > 0 && d->C >= 2 && d->H > 0 && d->D > 0 && d->Ks > 0, "%s: bad dims", who);
  flow_widths(d, f);
  f->p = *p;
  f->stamps = g_lfi_stamps;
  {
    const char* e = getenv("LFI_STAMP_K");
    f->stamp_k = e ? atoi(e) : f->Ks / 2;
  }
  if (prep) {
    const long cc = (long)d->Ks * d->C * d->C;
    const float* q = prep;
    f->W = q; q += cc;
    f->Wt = q; q += cc;
    f->Winv = q; q += cc;
    f->wz_t = q; q += (long)d->Ks * f->Ch * f->G;
    f->whh_t = q; q += (long)d->Ks * d->H * f->G;
    f->wfl_t = q; q += (long)d->Ks * d->H * f->Cout;
    f->wc = q; q += (long)d->Ks * f->G * d->D;
    f->ldconst = q;
    // scratch (log-det parts, fp64 inverse workspace), then the zero-padded images of the register-resident cells
    q = prep + prep_scratch_end(d);
    const long Ks = d->Ks;
    f->pW = q; q += Ks * f->C16 * f->C16;
    f->pWt = q; q += Ks * f->C16 * f->C16;
    f->pwz = q; q += Ks * f->Ch16 * f->NG * f->H16;
    f->pwh = q; q += Ks * f->H16 * f->NG * f->H16;
    f->pwfl = q; q += Ks * f->H16 * f->Co16;
    f->bwfl = q; q += Ks * f->Co16 * f->H16;
    f->bwh = q; q += Ks * f->NG * f->H16 * f->H16;
    f->bwz = q; q += Ks * f->NG * f->H16 * f->Ch16;
    f->pWinv = q; q += Ks * f->C16 * f->C16;
    q = reinterpret_cast<const float*>((reinterpret_cast<uintptr_t>(q) + 15) & ~(uintptr_t)15);
    f->xbwh = reinterpret_cast<const uint4*>(q); q += Ks * f->NG * f->H16 * f->H16;
    f->xbwz = reinterpret_cast<const uint4*>(q); q += Ks * f->NG * f->H16 * f->Ch16;
    q = reinterpret_cast<const float*>((reinterpret_cast<uintptr_t>(q) + 15) & ~(uintptr_t)15);
    f->hwz = reinterpret_cast<const uint4*>(q); q += Ks * f->Ch16 * f->NG * f->H16;
    f->hwh = reinterpret_cast<const uint4*>(q); q += Ks * f->H16 * f->NG * f->H16;
    f->hwfl = reinterpret_cast<const uint4*>(q); q += Ks * f->H16 * f->Co16;
    f->hWinv = reinterpret_cast<const uint4*>(q); q += Ks * f->C16 * f->C16;
  }
  return LFI_OK;
}

// LFI_FLOW_GENERIC=1 keeps the streaming cell kernels (tests cover both paths at sizes where either applies)
inline bool flow_force_generic() { return lfi_env_set("LFI_FLOW_GENERIC"); }

// LFI_FLOW_PIPE=0 keeps one launch per anti-diagonal instead of the persistent pipeline (tests cover both)
inline bool flow_pipe_enabled() { return lfi_env_on("LFI_FLOW_PIPE"); }
// LFI_PIPE_FENCE=1: consumers of a hand-off run an agent-scope acquire and read the tile with plain loads, instead of the
// fence-free form (every store and load of the tile sc1; MI355X_MICROARCH.md, hand-offs measured without the acquire, row 1)
// LFI_PIPE_X3=0: keep the exact f32 MFMA for the recurrent products of the persistent walk in bf16x3 mode too
inline bool flow_pipe_x3_enabled() { return lfi_env_on("LFI_PIPE_X3"); }
// shapes for which lfi_flow_prep leaves the reverse cell's fp16 fragment images (whole 32-k blocks everywhere: the X3 reverse cell's condition)
inline bool flow_x3h_images_ok(const FlowK& f) { return !f.lstm && f.H16 % 32 == 0 && f.Ch16 % 32 == 0 && f.C16 % 32 == 0; }
// LFI_SAMPLE_WFRAG16=0: the sampler's reverse cells load the f32 images and split them in registers, as before round 5
inline bool flow_sample_wfrag16_enabled() { return lfi_env_on("LFI_SAMPLE_WFRAG16"); }
// LFI_PIPE_FORCE_ABORT=1 (tests): start the walk with the abort word already set, as if a spin had timed out
inline bool flow_pipe_force_abort() { return lfi_env_set("LFI_PIPE_FORCE_ABORT"); }
inline int flow_pipe_fence() { return lfi_env_set("LFI_PIPE_FENCE") ? 1 : 0; }

template <typename Kf>
int set_flow_lds(Kf kernel, size_t bytes, const char* who) {
  if (bytes > 160 * 1024) {
    lfi_set_error("%s: needs %zu bytes of LDS (C/H too large)", who, bytes);
    return LFI_ERR_UNSUPPORTED;
  }
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
      lfi_set_error("%s: hipFuncSetAttribute(%zu): %s", who, bytes, hipGetErrorString(e));
      return LFI_ERR_LAUNCH;
    }
  }
  return LFI_OK;
}

// ---- bf16x3 / fp16x3 recurrent products: who takes them. One predicate per consumer; all want bf16x3 GEMM mode (gemm_precision bit 0)
// and GRU cells. The tails differ on purpose, with what each kernel contracts over (a contraction runs in whole 32-k blocks).
inline bool flow_x3_base(const lfi_flow_dims* d) { return (d->gemm_precision & 1) && !d->lstm; }
// lfi_flow_prep's bf16 hi / lo fragment images of bwh / bwz (flow_prep_x3_kernel), the backward walk's weights: k runs over the hidden
// units of a gate in both (Ch16 is a column count there). No switch and no size floor: the images are made for every shape that
// flow_x3_bwd_walk can take, whatever the switches say when the walk runs.
inline bool flow_x3_prep_images(const lfi_flow_dims* d, const FlowK& f) { return flow_x3_base(d) && f.H16 % 32 == 0; }
// forward walk: its products contract over h (H16) and over z1 (Ch16): both 16-k paddings must be whole 32-k blocks
inline bool flow_x3_fwd_walk(const lfi_flow_dims* d, const FlowK& f) {
  return flow_x3_base(d) && f.H16 % 32 == 0 && f.Ch16 % 32 == 0 && flow_pipe_x3_enabled();
}
// backward walk: contracts over the hidden units only (the images above: no Ch16 term), and its bf16 operand images, 64 (NG H16 + 8)
// bytes each, must fit the fp32 regions they replace (NG * H16 >= 128)
inline bool flow_x3_bwd_walk(const lfi_flow_dims* d, const FlowK& f) {
  return flow_x3_base(d) && f.H16 % 32 == 0 && f.NG * f.H16 >= 128 && flow_pipe_x3_enabled();
}
// backward planes: the walk above leaves its d(gate) images as the stash's operand planes, so the gate columns must be the stash's
// own: H itself, not its padding H16, a multiple of 32 (no padding columns), which makes 3 * H the walk's NG * H16
inline bool flow_x3_bwd_planes(const lfi_flow_dims* d) {
  return flow_x3_base(d) && d->H % 32 == 0 && 3 * d->H >= 128 && flow_pipe_x3_enabled();
}
// reverse cell (the samplers' chain; three fp16 products - fp32-grade - in both bf16 modes of the per-frame GEMMs): it contracts over
// z1, h and, for the inverse 1x1 convolution, the channels, so C16 joins the 32-k conditions - the shapes of flow_x3h_images_ok
inline bool flow_x3_rev_cell(const lfi_flow_dims* d, const FlowK& f) {
  return (d->gemm_precision & 1) && flow_x3h_images_ok(f) && flow_pipe_x3_enabled();
}

// ---- what a per-frame driver of a streaming session or a sampler decides from dims and the switches of the moment (nothing cached):
// sample_seq_run, lfi_flow_sample_cand_from, lfi_flow_score_seq_from, step_rows_frames (lfi_flow_chain.hip) and the two chunk drivers
// take every answer from here, and so do their *_pick functions. What depends on pointers or on the call - the fused front end, the
// staged window, the window-fragment hand-over, the nll form of the chain - stays with SampleFront and the drivers.
struct FramePlan {
  bool fast;    // the register-resident cells (flow_fast_ok); LFI_FLOW_GENERIC=1 keeps the streaming cells
  bool chain;   // one launch for a frame's whole chain; LFI_SAMPLE_CHAIN=0 (and the streaming cells) keep one launch per flow step
  bool x3;      // reverse cells: three fp16 products of two-piece operands, at per-frame arithmetic 9 and 5 (flow_x3_rev_cell)
  bool xw;      // ... their weights from the fp16 fragment images lfi_flow_prep left, no split in every workgroup (LFI_SAMPLE_WFRAG16=0: split)
  bool x3f;     // forward cells: three fp16 products for per-frame arithmetic 9 ONLY. The reverse cells keep them at 5 as well - their
                // operands are bounded (the prior draw, h in (-1, 1)) - but the forward chain's first operand is actnorm of a frame the
                // CALLER supplies: a value beyond fp16's range would turn into inf - inf = NaN in the split and stay in h / c. 5 is the
                // arithmetic a session falls back to when its range guard trips and must have no range caveat: it takes the exact-f32
                // cell (as 0 and the LSTM cell do), which is at least as accurate as six bf16 products.
  size_t lds_fast, lds_gen;   // dynamic LDS of the register-resident cells' carve and of the streaming cells'
  // lfi_flow_frame_plan's answer (include/lfi.h)
  int bits() const { return (fast ? 1 : 0) | (chain ? 2 : 0) | (x3 ? 4 : 0) | (xw ? 8 : 0) | (x3f ? 16 : 0); }
};
inline FramePlan flow_frame_plan(const lfi_flow_dims* d) {
  FlowK f = {};
  flow_widths(d, &f);
  FramePlan pl = {};
  pl.fast = flow_fast_ok(f.C, f.H, f.Cout) && !flow_force_generic();
  pl.chain = pl.fast && lfi_env_on("LFI_SAMPLE_CHAIN");
  pl.x3 = flow_x3_rev_cell(d, f);
  pl.xw = pl.x3 && pl.chain && flow_sample_wfrag16_enabled();
  pl.x3f = pl.x3 && (d->gemm_precision & 0xff) == 9;
  pl.lds_fast = (size_t)carve_fast_fwd(f.C, f.C16, f.H16, f.Ch16, f.Cout).total * sizeof(float);
  pl.lds_gen = (size_t)carve_fwd(f.C, f.H, f.Ch, f.C2, f.Cout).total * sizeof(float);
  return pl;
}

// What lfi_flow_sample_seq_nll, lfi_flow_score_seq_from and lfi_flow_step_rows_from (and lfi_flow_score_seq_chunk, lfi_flow_chunk.hip) ask of the arguments they share, in one order.
// who_from: the name first_frame is reported under (the sampler's is its _from entry point); ptrs_ok: the caller's own list of
// pointers that must not be null. A rule on the frame count itself is the caller's and follows this check.
// What has to fit into the E columns of wct is what the window product reads of them: hist1 * C columns from p1->col for a raw
// window, p1->hid for an encoded one (its features, not its frames - a feature vector may well be narrower than the window).
inline int frame_args_check(const char* who, const char* who_from, const lfi_flow_dims* d, bool ptrs_ok, long E, int hist1, int start,
                     int nframes, int seq_len, const float* cstate, int first_frame, const lfi_p1enc* p1) {
  LFI_REQUIRE(first_frame >= 0, "%s: negative first_frame", who_from);
  LFI_REQUIRE(ptrs_ok, "%s: null pointer", who);
  LFI_REQUIRE(hist1 >= 0 && hist1 <= start && start + nframes <= seq_len, "%s: bad frame range", who);
  const long p1cols = p1 && p1->kind != 0 ? (long)p1->hid : (long)hist1 * d->C, p1col = p1 ? p1->col : 0;
  LFI_REQUIRE(p1col >= 0 && p1col + p1cols <= E, "%s: window wider than the feature vector", who);
  LFI_REQUIRE(!d->lstm || cstate, "%s: the LSTM cell needs cstate", who);
  return LFI_OK;
}


// ---- the forward chain's cell (lfi_flow_chain.hip: one frame per launch; lfi_flow_chunk.hip: the frames of a chunk in one launch)
// FlowStep.normal_flow (glow/models.py:311-341) of ONE observed frame with the recurrent state carried in place: the forward twin of
// rev_fast_cell for a streaming session's observe() step. Same thread maps, same LDS carve, same place of the wait: the weights, gic,
// h_prev and the h_prev W_hh half of the recurrent product run before it; behind it actnorm, y = a W, the z1 half + the gates,
// LinearZeros and the coupling. The recurrent cell sees what the reverse cell of the same frame sees - z1 and the conditioning - so
// the h / c it leaves is the state a sampler continues from. No stash of any kind.
// X3: every product as three fp16 products of two-piece operands (x3h_*, fp32-grade: 2^-22 relative), the f32 fragment images split
// in registers before the wait; otherwise the exact f32 MFMA. (The training walks' three bf16 products - 2^-16 pieces - are not used
// here: the state must match the reverse cell's to the sampler's own tolerance.)
// q_in: the rows' running coupling log-det from step k - 1 (null: this cell starts it); q_out: where it goes on to step k + 1, sc1
// stores in front of the publish. nll_out (the last step): the cell adds the prior term of its z, sum_c -0.5 (z_c^2 + log 2 pi), and
// logdet_const and writes -(logdet + log p(z)) / ln 2 in bits. One writer per word, k ascending: a fixed summation order.
// io.x_out may be null (the last step of a caller that does not want z).
// RM (flow_rows_chain_kernel): a row-masked cell, as rev_fast_cell's - h_out / c_out, the output tile, the hand-over q and the NLL word
// are stored for the rows of role io.role_want only.
// SEQ (flow_fwd_seq_chain_kernel): the cell runs the sq->frames frames of a launch one after another. What does not depend on the frame
// is requested once where the register file allows - the GRU cell's W_hh and W_ih[:, :Ch], the per-column constants, h_prev / c_prev
// of the first frame; W and LinearZeros (and, for the LSTM cell, whose four gate blocks of W_hh alone are 128 VGPRs, every weight)
// are asked for again in every frame, from the L2 and in front of where they are needed. The recurrent state stays
// on chip: Hn of frame n is Ht of frame n + 1 (the two LDS images swap), the LSTM cell state crosses in registers; h_out and c_out are stored at
// the last frame only. Per frame: gic, the wait for frame n of step k - 1 (progress word >= n + 1), the cell, the hand-over slot of
// (k, n), progress word = n + 1. io / q_in / q_out / nll_out point at frame 0; sq holds the strides. A wait that gives up leaves NaN in
// the nll / z of the frames the last step has not finished.
// RAG (flow_fwd_seq_rows_chain_kernel, lfi_flow_chunk_rows.hip; with SEQ): a ragged chunk - batch row r takes the first sq->lengths[r]
// frames only. sq->frames is the TILE's longest row (the same in every step k of the tile, so the progress words agree); per frame
// two uniform masks of the tile's 16 rows (tile_row_lengths once, tile_row_frames per frame: scalar registers): h_out / c_out are
// stored for the rows whose last frame this is - the masked stores of the RM cells - and the output tile, the hand-over q and the
// NLL word for the rows that have the frame. A row behind its length goes on through the arithmetic (rows never mix inside a cell)
// and reaches nothing stored.
struct FwdSeq {
  int frames;
  long x_in_step, x_out_step;   // floats between two frames' rows of x_in / x_out
  long gic_step, row_step;      // B * G; B (q_in, q_out, nll_out)
  const int* lengths;           // RAG only: one word per batch row
};
// RAG: the lengths of the tile's 16 rows, read once in front of the frame loop, clamped from above to `frames`; 0 for a row outside the
// batch. A length below 0 acts as 0. (Uniform values, and through readfirstlane the compiler knows it: behind the kernel's first
// stores it reads them with vector loads, and sixteen VGPRs across the frame loop are more than the SEQ cell has to spare.)
__device__ __forceinline__ void tile_row_lengths(const int* lengths, int b0, int rows, int frames, int (&len)[MB]) {
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int row = b0 + i;
    len[i] = row < rows ? min(__builtin_amdgcn_readfirstlane(lengths[row]), frames) : 0;
  }
}
// RAG: the tile's rows at frame n - bit i of *has: row b0 + i has the frame (length > n), of *ends: it is the row's last (length == n + 1)
__device__ __forceinline__ void tile_row_frames(const int (&len)[MB], int n, unsigned* has, unsigned* ends) {
  unsigned a = 0u, e = 0u;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (len[i] > n) a |= 1u << i;
    if (len[i] == n + 1) e |= 1u << i;
  }
  *has = a; *ends = e;
}
// RAG: the longest row of the tile at b0, lengths clamped to [0, nframes] (0: the tile has nothing to do)
__device__ __forceinline__ int tile_max_frames(const int* lengths, int b0, int rows, int nframes) {
  int m = 0;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int row = b0 + i;
    if (row < rows) m = max(m, min(lengths[row], nframes));
  }
  return m;
}
template <int NG, bool X3, bool RM = false, bool SEQ = false, bool RAG = false>
__device__ __forceinline__ bool fwd_chain_cell(const FlowK& f, const CellIO& io, int b0, const unsigned* wait_flag, unsigned* abort_w,
                                               unsigned* pub_flag, int* s_ok, const float* q_in, float* q_out, float* nll_out,
                                               const FwdSeq* sq = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int l15 = lane & 15, kq = lane >> 4;   // (not const: SEQ, at the head of the frame loop)
  int ri = tid >> 5, cl = tid & 31;
  const int k = io.k, rows = io.rows;
  const int C = f.C, H = f.H, Ch = f.Ch, C2 = f.C2, Cout = f.Cout, G = f.G;
  const int C16 = f.C16, Ch16 = f.Ch16, H16 = f.H16, Co16 = f.Co16;
  const CarveF cv = carve_fast_fwd(C, C16, H16, Ch16, Cout);
  float* At = flow_smem + cv.At;
  float* Ht = flow_smem + cv.Ht;
  float* Zt = flow_smem + cv.Zt;
  float* Hn = flow_smem + cv.Hn;
  float* Yrm = flow_smem + cv.Yrm;
  float* Orm = flow_smem + cv.Orm;
  const int ldy = C + 1, ldo = Cout + 1;
  const int nbC = C16 >> 4, nbZ = Ch16 >> 4, nbH = H16 >> 4;
  const bool t1 = wave * 16 < C, t2 = wave * 16 < H, t3 = wave * 16 < Cout;
  int tcol = wave * 16 + l15;
  unsigned live = 0u;
  if constexpr (RM) live = tile_live_rows(io.role, io.role_want, b0, rows);
  // ---- requests in the order their results are needed: h_prev (its LDS image gates the first barrier), the recurrent weights, then
  // the weights of the phases behind the wait
  const int hrow = b0 + ri;
  float hv[FB_H / 2];
#pragma unroll
  for (int q = 0; q < FB_H / 2; ++q) {
    const int j = cl + 32 * q;
    hv[q] = (io.h_prev && hrow < rows && j < H) ? io.h_prev[(long)hrow * H + j] : 0.0f;
  }
  f32x4 wz[NG][FB_Z], wh[NG][FB_H], w3[FB_H], w1[FB_C];
  // SEQ: what a frame asks for again, whole (zero padding included, so that nothing of it lives across the frames): W behind the
  // h-side product and LinearZeros behind F1; for the LSTM cell also W_hh in front of the h-side product and W_ih[:, :Ch] behind it.
  // W_hh and W_ih[:, :Ch] of the GRU cell (120 VGPRs at H = 128) are what the register file holds across the frames beside the
  // cell's own values. (The image pointer goes through an empty asm statement in every frame: the compiler would otherwise hoist
  // these loop-invariant loads out of the frame loop and keep their 48 - 208 VGPRs alive across it - in scratch.)
  constexpr bool WH_PER_FRAME = SEQ && NG == 4;
  auto per_frame = [](const float* img) {
    asm volatile("" : "+s"(img));
    return img;
  };
  [[maybe_unused]] auto load_wh = [&](const float* img) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int b = 0; b < FB_H; ++b) wh[g][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
      load_frag<FB_H>(wh[g], img + (long)k * H16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbH, t2);
    }
  };
  [[maybe_unused]] auto load_w1 = [&]() {
#pragma unroll
    for (int b = 0; b < FB_C; ++b) w1[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    load_frag<FB_C>(w1, per_frame(f.pW) + (long)k * C16 * C16, C16, tcol, kq, nbC, t1);
  };
  [[maybe_unused]] auto load_w3 = [&]() {
#pragma unroll
    for (int b = 0; b < FB_H; ++b) w3[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    load_frag<FB_H>(w3, per_frame(f.pwfl) + (long)k * H16 * Co16, Co16, tcol, kq, nbH, t3);
  };
  [[maybe_unused]] auto load_wz = [&](const float* img) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int b = 0; b < FB_Z; ++b) wz[g][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
      load_frag<FB_Z>(wz[g], img + (long)k * Ch16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbZ, t2);
    }
  };
  if constexpr (SEQ) {
    if constexpr (!WH_PER_FRAME) {
      load_wh(f.pwh);
      load_wz(f.pwz);
    }
  } else {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int b = 0; b < FB_Z; ++b) wz[g][b] = zero4;
#pragma unroll
      for (int b = 0; b < FB_H; ++b) wh[g][b] = zero4;
      load_frag<FB_H>(wh[g], f.pwh + (long)k * H16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbH, t2);
      load_frag<FB_Z>(wz[g], f.pwz + (long)k * Ch16 * NG * H16, NG * H16, g * H16 + tcol, kq, nbZ, t2);
    }
#pragma unroll
    for (int b = 0; b < FB_H; ++b) w3[b] = zero4;
#pragma unroll
    for (int b = 0; b < FB_C; ++b) w1[b] = zero4;
    // (the LSTM cell's four gate blocks of W_hh fill the register file: its W and LinearZeros fragments are requested once the h-side
    // product has let those go - still in front of the wait; 24 VGPRs in scratch otherwise)
    if constexpr (NG != 4) {
      load_frag<FB_C>(w1, f.pW + (long)k * C16 * C16, C16, tcol, kq, nbC, t1);
      load_frag<FB_H>(w3, f.pwfl + (long)k * H16 * Co16, Co16, tcol, kq, nbH, t3);
    }
  }
  float gc[4][NG], bh[NG], cprev[4];
  [[maybe_unused]] float cnew[4];
  auto load_gic = [&](const float* gic, bool first) {   // first: + the constants and the state that arrive once
    const float* bhh = f.p.b_hh + (long)k * G;
    const int jc = tcol < H ? tcol : 0;
    if (first) {
#pragma unroll
      for (int g = 0; g < NG; ++g) bh[g] = bhh[g * H + jc];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(b0 + kq * 4 + r, rows - 1);
#pragma unroll
      for (int g = 0; g < NG; ++g) gc[r][g] = gic[(long)row * G + g * H + jc];
      if (first) cprev[r] = (NG == 4 && io.c_prev) ? io.c_prev[(long)row * H + jc] : 0.0f;
    }
  };
  if constexpr (NG != 4) load_gic(io.gic, true);
  // per-column constants of the phases behind the wait: ActNorm of this thread's two channels (cl, cl + 32), LinearZeros of its column
  float an_b[2], an_s[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = cl + 32 * q;
    an_b[q] = c < C ? f.p.an_bias[(long)k * C + c] : 0.0f;
    an_s[q] = c < C ? expf(f.p.an_logs[(long)k * C + c]) : 0.0f;
  }
  const float flb = tcol < Cout ? f.p.b_fl[(long)k * Cout + tcol] : 0.0f;
  const float fls = tcol < Cout ? expf(3.0f * f.p.l_fl[(long)k * Cout + tcol]) : 0.0f;
  // ---- before the wait: h_prev and the zero k padding into LDS, the fragment split, the h_prev W_hh half of the recurrent product
#pragma unroll
  for (int q = 0; q < FB_H / 2; ++q) {
    const int j = cl + 32 * q;
    if (j < H16) {
      Ht[j * LT + ri] = hv[q];
      if (j >= H) Hn[j * LT + ri] = 0.0f;
    }
  }
  for (int c = Ch + cl; c < Ch16; c += 32) Zt[c * LT + ri] = 0.0f;
  X3FragH wzx[X3 ? NG : 1][FB_Z / 2], w3x[X3 ? FB_H / 2 : 1], w1x[X3 ? FB_C / 2 : 1];
  if constexpr (X3) {   // (instantiated for shapes with whole 32-k blocks everywhere: flow_x3h_images_ok)
    if constexpr (!SEQ) {
#pragma unroll
    for (int b = 0; b < FB_H / 2; ++b) w3x[b] = x3h_pack(w3[2 * b], w3[2 * b + 1]);
#pragma unroll
    for (int b = 0; b < FB_C / 2; ++b) w1x[b] = x3h_pack(w1[2 * b], w1[2 * b + 1]);
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int b = 0; b < FB_Z / 2; ++b) wzx[g][b] = WH_PER_FRAME ? X3FragH{} : x3h_pack(wz[g][2 * b], wz[g][2 * b + 1]);
  }
  __syncthreads();
  const int frames = SEQ ? sq->frames : 1;
  [[maybe_unused]] unsigned rag_has = 0u, rag_ends = 0u;
  [[maybe_unused]] int rag_len[RAG ? MB : 1];
  if constexpr (RAG) tile_row_lengths(sq->lengths, b0, rows, frames, rag_len);
  for (int n = 0; n < frames; ++n) {
  if constexpr (RAG) tile_row_frames(rag_len, n, &rag_has, &rag_ends);
  if constexpr (SEQ) {
    // (the thread's coordinates pass through an empty asm statement: everything addressed from them is then worked out again in
    // every frame - a few VALU instructions - instead of being hoisted out of the loop, where some twenty such addresses and
    // predicates sat in registers across all phases and pushed the kernel into scratch)
    asm volatile("" : "+v"(l15), "+v"(kq), "+v"(ri), "+v"(cl), "+v"(tcol));
    if constexpr (WH_PER_FRAME) load_wh(per_frame(f.pwh));
    if (NG != 4 && n > 0) load_gic(io.gic + n * sq->gic_step, false);
  }
  f32x4 az[NG], ah[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    az[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (t2) {
    const float* hl = Ht + kq * LT + l15;
    if constexpr (X3) {
#pragma unroll
      for (int b = 0; b < FB_H / 2; ++b)
        if (b < (nbH >> 1)) {
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
  if constexpr (SEQ) {
    __builtin_amdgcn_sched_barrier(0);
    load_w1();   // (W now, LinearZeros once F1 has let W go: in flight under the recurrent product of F2)
    if constexpr (WH_PER_FRAME) load_wz(per_frame(f.pwz));
    if constexpr (NG == 4) load_gic(io.gic + n * sq->gic_step, n == 0);
    if constexpr (X3) {
#pragma unroll
      for (int b = 0; b < FB_C / 2; ++b) w1x[b] = x3h_pack(w1[2 * b], w1[2 * b + 1]);
    }
  } else if constexpr (NG == 4) {
    __builtin_amdgcn_sched_barrier(0);
    load_frag<FB_C>(w1, f.pW + (long)k * C16 * C16, C16, tcol, kq, nbC, t1);
    load_frag<FB_H>(w3, f.pwfl + (long)k * H16 * Co16, Co16, tcol, kq, nbH, t3);
    load_gic(io.gic, true);
  }
  if (wait_flag && !pipe_acquire(wait_flag, SEQ ? (unsigned)(n + 1) : 1u, abort_w, tid, s_ok, false)) {
    if constexpr (SEQ) {
      const int row = b0 + ri;
      int mend = frames;
      if constexpr (RAG) mend = row < rows ? min(sq->lengths[row], frames) : 0;   // (the row's own frames only)
      if (nll_out && row < rows)
        for (int m = n; m < mend; ++m) {
          if (io.x_out)
            for (int c = cl; c < C; c += 32) io.x_out[m * sq->x_out_step + (long)row * io.ldxo + c] = __builtin_nanf("");
          if (cl == 0) nll_out[m * sq->row_step + row] = __builtin_nanf("");
        }
    }
    return false;
  }
  const float* x_in = SEQ ? io.x_in + n * sq->x_in_step : io.x_in;
  float* x_out = (SEQ && io.x_out) ? io.x_out + n * sq->x_out_step : io.x_out;
  const long rstep = SEQ ? n * sq->row_step : 0;
  // ---- F0: actnorm of the incoming tile (glow/modules.py:45-52), k-major with zero k padding
  float q = 0.0f;   // lane cl == 0 carries its row's running coupling log-det
  {
    const int row = b0 + ri;
    const bool rok = row < rows;
    if (q_in && cl == 0 && rok) q = ld_tile(q_in + rstep + row, false);   // (in flight under the cell: needed in F4)
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      const int c = cl + 32 * qq;
      if (c < C16) {
        const float v = (c < C && rok) ? ld_tile(x_in + (long)row * io.ldx + c, wait_flag == nullptr) : 0.0f;
        At[c * LT + ri] = c < C ? (v + an_b[qq]) * an_s[qq] : 0.0f;
      }
    }
  }
  __syncthreads();
  // ---- F1: y = a W   (InvertibleConv1x1.forward, glow/modules.py:186); z1 = y[:, :Ch] is the recurrent cell's input
  if (t1) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (X3) {
      const float* al = At + kq * LT + l15;
#pragma unroll
      for (int b = 0; b < FB_C / 2; ++b)
        if (b < (nbC >> 1)) acc = x3h_mma(x3h_a(al + b * 32 * LT), w1x[b], acc);
    } else {
      acc = mma16_reg<FB_C>(At + kq * LT + l15, w1, nbC);
    }
    if (tcol < C) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kq * 4 + r;
        Yrm[i * ldy + tcol] = acc[r];
        if (tcol < Ch) Zt[tcol * LT + i] = acc[r];
      }
    }
  }
  if constexpr (SEQ) {
    __builtin_amdgcn_sched_barrier(0);
    load_w3();
  }
  __syncthreads();
  // ---- F2: the z1 half of the recurrent product, then the gate math (h / c updated in place)
  if (t2) {
    const float* zl = Zt + kq * LT + l15;
    if constexpr (X3) {
#pragma unroll
      for (int b = 0; b < FB_Z / 2; ++b)
        if (b < (nbZ >> 1)) {
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
    if constexpr (RAG) {   // the state leaves at each row's own last frame
      fast_cell_p2_gates<NG, true, false>(f, Ht, Hn, az, ah, gc, bh, cprev, tcol, kq, b0, rows, io.h_out, nullptr, nullptr,
                                          NG == 4 ? cnew : nullptr, nullptr, nullptr, 0, 0, rag_ends);
      if (NG == 4 && tcol < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = kq * 4 + r;
          if ((rag_ends >> i) & 1u) io.c_out[(long)(b0 + i) * H + tcol] = cnew[r];
        }
      }
    } else if constexpr (SEQ) {
      fast_cell_p2_gates<NG, RM, false>(f, Ht, Hn, az, ah, gc, bh, cprev, tcol, kq, b0, rows, n == frames - 1 ? io.h_out : nullptr, nullptr,
                                        nullptr, NG == 4 ? cnew : nullptr, nullptr, nullptr, 0, 0, live);
      if (NG == 4 && n == frames - 1 && tcol < H) {   // the cell state crossed the frames in registers: stored once, as h
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = b0 + kq * 4 + r;
          if (row < rows) io.c_out[(long)row * H + tcol] = cnew[r];
        }
      }
    } else
    fast_cell_p2_gates<NG, RM>(f, Ht, Hn, az, ah, gc, bh, cprev, tcol, kq, b0, rows, io.h_out, io.c_out, nullptr, nullptr, nullptr, nullptr,
                               0, 0, live);
  }
  __syncthreads();
  // ---- F3: o = (h' Wfl^T + b) exp(3 logs)   (LinearZeros, glow/modules.py:93-95)
  if constexpr (SEQ && X3) {
#pragma unroll
    for (int b = 0; b < FB_H / 2; ++b) w3x[b] = x3h_pack(w3[2 * b], w3[2 * b + 1]);
  }
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
  // ---- F4: coupling (glow/models.py:330-341), the pass-through half, the row's log-det; the last step: the prior term and the NLL
  {
    const int row = b0 + ri;
    bool rok = RM ? ((live >> ri) & 1u) != 0u : row < rows;
    if constexpr (RAG) rok = ((rag_has >> ri) & 1u) != 0u;
    float lg = 0.0f, zz = 0.0f;
    auto put = [&](int c, float v) {
      if (!x_out || !rok) return;
      if (pub_flag) st_sc1(x_out + (long)row * io.ldxo + c, v);
      else x_out[(long)row * io.ldxo + c] = v;
    };
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
      put(Ch + cl, z2n);
      zz = z2n * z2n;
    }
    if (cl < Ch) {
      const float z1 = Yrm[ri * ldy + cl];
      put(cl, z1);
      zz = __builtin_fmaf(z1, z1, zz);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) lg += __shfl_xor(lg, o, 64);   // the 32 lanes of one row
    if (nll_out) {
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) zz += __shfl_xor(zz, o, 64);
    }
    if (cl == 0 && rok) {
      q += lg;
      if (nll_out) nll_out[rstep + row] = -(q + f.ldconst[0] + -0.5f * (zz + (float)C * LOG2PI_F)) / LN2_F;
      else st_sc1(q_out + rstep + row, q);
    }
  }
  if (pub_flag) pipe_publish(pub_flag, SEQ ? (unsigned)(n + 1) : 1u, tid, true);
  if constexpr (SEQ) {   // this frame's new state is the next frame's previous one
    float* t = Ht; Ht = Hn; Hn = t;
    if constexpr (NG == 4) {
#pragma unroll
      for (int r = 0; r < 4; ++r) cprev[r] = cnew[r];
    }
  }
  }
  return true;
}

// ---- the carve of a chunk work area (lfi_flow_score_seq_chunk and its ragged form) for F = nframes * B rows, in floats from its
// 16-byte aligned start
struct ChunkCarve {
  long p1work, wstage, gic, tiles, q, pipe, pipe_words, total;
  int ldw;
};
inline ChunkCarve chunk_carve(const lfi_flow_dims* d, const lfi_p1enc* p1, int hist1, int nframes) {
  const long F = (long)nframes * d->B, G = (long)(d->lstm ? 4 : 3) * d->H, nbt = (d->B + MB - 1) / MB;
  auto up4 = [](long v) { return (v + 3) & ~3L; };
  lfi_flow_dims dm = *d;
  dm.B = (int)F;
  ChunkCarve c = {};
  c.ldw = (int)up4((long)hist1 * d->C);
  long o = 0;
  c.p1work = o; o += up4(lfi_flow_sample_p1_work_floats(&dm, p1, hist1));
  c.wstage = o; o += F * c.ldw;
  c.gic = o; o += up4((long)d->Ks * F * G);
  c.tiles = o; o += up4((long)(d->Ks - 1) * F * d->C);
  c.q = o; o += up4((long)(d->Ks - 1) * F);
  c.pipe = o; c.pipe_words = up4((long)PIPE_HDR + (long)d->Ks * nbt); o += c.pipe_words;
  c.total = o;
  return c;
}

// What lfi_flow_score_seq_chunk and its ragged form do between fill_flow and the launch of their chain, once for both: the checks
// (ptrs_ok: the caller's own list), the carve, the unit's kernel (`pick`, of the plan's bits) and its LDS, the front end ONCE - the
// windows of all frames (row n * B + b: frames [start + n - hist1, start + n) of sample b), then the products - and the chain-state
// clear. Leaves the fields the two kernel-argument structs share in *sc, the kernel and its LDS in *kernel / *lds; *kernel stays null
// where the caller has no chain to launch:
// (diagnostics, tools/stream_latency.py: LFI_CHUNK_ONLY=front / chain launches one of the two parts alone, so that events around the
// call time it - the chain then reads the gic an earlier whole call left in the work area. Results are not meaningful.)
template <typename SC, typename Kf>
int chunk_front(const char* who, const lfi_flow_dims* d, const lfi_flow_params* p, const FlowK& f, bool ptrs_ok, const float* wct, long E,
                int hist1, float* pre_static, float* faces, int seq_len, int start, int nframes, int first_frame, float* h, float* cstate,
                const lfi_p1enc* p1, float* chunk_work, float* z, float* nll, void* stream, Kf (*pick)(const FramePlan&, bool), SC* sc,
                Kf* kernel, size_t* lds) {
  int rc;
  if ((rc = frame_args_check(who, who, d, ptrs_ok, E, hist1, start, nframes, seq_len, cstate, first_frame, p1))) return rc;
  LFI_REQUIRE(nframes >= 1 && nframes <= d->N, "%s: %d frames, the work area holds d->N = %d", who, nframes, d->N);
  LFI_REQUIRE(hist1 >= 1, "%s: bad frame range (hist1 %d)", who, hist1);
  LFI_REQUIRE((long)nframes * f.B < (1L << 24), "%s: %d frames x batch %d: too many rows for one launch", who, nframes, f.B);
  const FramePlan pl = flow_frame_plan(d);
  LFI_REQUIRE(pl.chain, "%s: C, Cout <= 64 and hidden_channels <= 128 only, LFI_SAMPLE_CHAIN not 0 "
              "(lfi_flow_score_chunk_ok); otherwise lfi_flow_score_seq_from", who);
  const int B = f.B, C = f.C;
  const int p1kind = p1 ? p1->kind : 0;
  LFI_REQUIRE(p1kind >= 0 && p1kind <= 3, "%s: bad p1_face encoder kind %d", who, p1kind);
  LFI_REQUIRE(p1kind == 0 || p1->hid > 0, "%s: encoded p1_face window with hid %d", who, p1->hid);
  const ChunkCarve cv = chunk_carve(d, p1, hist1, nframes);
  float* base = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(chunk_work) + 15) & ~(uintptr_t)15);
  unsigned* pipe = reinterpret_cast<unsigned*>(base + cv.pipe);
  const Kf chain_kernel = pick(pl, f.lstm);
  if ((rc = set_flow_lds(chain_kernel, pl.lds_fast, who))) return rc;
  const char* only = getenv("LFI_CHUNK_ONLY");
  const bool run_front = !(only && only[0] == 'c'), run_chain = !(only && only[0] == 'f');
  if (run_front) {
    if ((rc = lfi_gather_windows(faces, B, seq_len, C, nframes, start, hist1, 0, nullptr, base + cv.wstage, cv.ldw, 0, stream))) return rc;
    if ((rc = lfi_internal_sample_front_rows(d, p, p1, wct, E, hist1, f.wc, nframes * B, base + cv.wstage, cv.ldw, pre_static, base + cv.gic,
                                             base + cv.p1work, stream))) return rc;
  }
  if (!run_chain) return LFI_OK;
  hipError_t me = hipMemsetAsync(pipe, 0, (size_t)cv.pipe_words * sizeof(unsigned), (hipStream_t)stream);
  LFI_REQUIRE(me == hipSuccess, "%s: hipMemsetAsync: %s", who, hipGetErrorString(me));
  sc->frame0 = faces + (long)start * C; sc->ld_frame = (long)seq_len * C; sc->nframes = nframes;
  sc->tiles = base + cv.tiles; sc->q = base + cv.q; sc->gic = base + cv.gic;
  sc->h = h; sc->cstate = cstate; sc->has_prev = first_frame > 0 ? 1 : 0; sc->pipe = pipe; sc->z = z; sc->nll = nll;
  *kernel = chain_kernel; *lds = pl.lds_fast;
  return LFI_OK;
}

}  // namespace
