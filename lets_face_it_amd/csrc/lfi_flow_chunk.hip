// A chunk of teacher-forced frames of a streaming session per call (SampleStream.observe_many): the forward chain's cell
// (fwd_chain_cell, lfi_flow_cells.h) with the loop over the frames inside the chain, and its entry points. A unit of its own: the
// reverse chains and the reverse walk of lfi_flow_chain.hip compile to the instructions they had without it (in one unit with
// them, these kernels changed the inliner's choices inside the LSTM cells there).
#include "lfi_flow_cells.h"

namespace {

// A CHUNK of observed frames of a streaming session (SampleStream.observe_many): flow_fwd_chain_kernel with the loop over the frames
// INSIDE the chain - the systolic schedule of the training walk (nframes + Ks - 1 cell times end to end, where one launch per frame
// runs nframes * Ks) on the streaming cell, from a carried state and with no stash. Workgroup (k, tile), ids by ticket, k ascending,
// runs fwd_chain_cell<.., SEQ> over all frames of its tile. It waits only on (k - 1, tile), a lower ticket, and the hand-over slots
// are per (step boundary, frame), never reused inside a launch: there is no back-pressure, so no wait on a higher ticket, and any
// number of resident workgroups makes progress. The caller bounds the slots by the frames it gives one launch.
struct FwdSeqChain {
  const float* frame0; long ld_frame;   // the chunk's first frame in the faces sequence (row stride seq_len * C); frame n: + n * C
  int nframes;
  float* tiles;           // [Ks - 1][nframes][B][C]: what step k hands to step k + 1
  float* q;               // [Ks - 1][nframes][B]: the rows' running log-det beside it
  const float* gic;       // [Ks][nframes][B][G]
  float *h, *cstate;      // [Ks][B][H] recurrent state: read at the first frame, written at the last
  int has_prev;           // 0: the chunk starts a sequence (zero state)
  unsigned* pipe;         // ticket, abort, progress words (frames published per (k, tile)); zeroed before the launch
  float* z;               // [nframes][B][C] or null
  float* nll;             // [nframes][B]
};
template <int NG, bool X3>
__global__ __launch_bounds__(NT) void flow_fwd_seq_chain_kernel(FlowK f, FwdSeqChain sc) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(sc.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int k = s_id / nbt, bt = s_id - k * nbt;
  if (k >= f.Ks) return;
  const bool last = k == f.Ks - 1;
  const long FB = (long)sc.nframes * f.B;
  unsigned* prog = sc.pipe + PIPE_HDR;
  CellIO io = {};
  FwdSeq sq = {};
  sq.frames = sc.nframes; sq.gic_step = (long)f.B * f.G; sq.row_step = f.B; sq.x_out_step = (long)f.B * f.C;
  io.k = k; io.rows = f.B;
  if (k == 0) { io.x_in = sc.frame0; io.ldx = sc.ld_frame; sq.x_in_step = f.C; }
  else { io.x_in = sc.tiles + (long)(k - 1) * FB * f.C; io.ldx = f.C; sq.x_in_step = (long)f.B * f.C; }
  io.x_out = last ? sc.z : sc.tiles + (long)k * FB * f.C; io.ldxo = f.C;
  io.h_prev = sc.has_prev ? sc.h + (long)k * f.B * f.H : nullptr;
  io.h_out = sc.h + (long)k * f.B * f.H;
  if (NG == 4) { io.c_prev = sc.has_prev ? sc.cstate + (long)k * f.B * f.H : nullptr; io.c_out = sc.cstate + (long)k * f.B * f.H; }
  io.gic = sc.gic + (long)k * FB * f.G;
  fwd_chain_cell<NG, X3, false, true>(f, io, bt * MB, k > 0 ? prog + (k - 1) * nbt + bt : nullptr, sc.pipe + 1,
                                      last ? nullptr : prog + k * nbt + bt, &s_ok, k > 0 ? sc.q + (long)(k - 1) * FB : nullptr,
                                      last ? nullptr : sc.q + (long)k * FB, last ? sc.nll : nullptr, &sq);
}

typedef void (*FlowFwdSeqChainKernel)(FlowK, FwdSeqChain);
FlowFwdSeqChainKernel flow_fwd_seq_chain_pick(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_fwd_seq_chain_kernel<4, false>;
  return pl.x3f ? flow_fwd_seq_chain_kernel<3, true> : flow_fwd_seq_chain_kernel<3, false>;
}

}  // namespace

// ---- a chunk of teacher-forced frames known up front (SampleStream.observe_many): the front end once, the chain as ONE launch
// (the carve of the chunk work area: chunk_carve, lfi_flow_cells.h - shared with the ragged chunk of lfi_flow_chunk_rows.hip)

extern "C" int lfi_flow_score_chunk_ok(const lfi_flow_dims* d) { return d && flow_frame_plan(d).chain ? 1 : 0; }

extern "C" long lfi_flow_score_chunk_work_floats(const lfi_flow_dims* d, const lfi_p1enc* p1, int hist1) {
  if (!d || d->B <= 0 || d->N <= 0 || d->Ks <= 0 || hist1 < 0) return 0;
  return chunk_carve(d, p1, hist1, d->N).total + 4;   // (+ the slack of the 16-byte alignment)
}

extern "C" int lfi_flow_score_seq_chunk(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                                        int hist1, float* pre_static, float* faces, int seq_len, int start, int nframes, int first_frame,
                                        float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work, float* chunk_work,
                                        float* z, float* nll, void* stream) {
  FlowK f = {};
  const char* who = "lfi_flow_score_seq_chunk";
  int rc = fill_flow(d, p, prep, &f, who);
  if (rc) return rc;
  FwdSeqChain sc = {};
  FlowFwdSeqChainKernel chain_kernel = nullptr;
  size_t lds = 0;
  // (the checks, the front end and the chain-state clear: chunk_front, lfi_flow_cells.h; no kernel: LFI_CHUNK_ONLY=front)
  if ((rc = chunk_front(who, d, p, f, prep && wct && pre_static && faces && h && chunk_work && nll, wct, E, hist1, pre_static, faces, seq_len,
                        start, nframes, first_frame, h, cstate, p1, chunk_work, z, nll, stream, flow_fwd_seq_chain_pick, &sc, &chain_kernel,
                        &lds)) || !chain_kernel) return rc;
  hipLaunchKernelGGL(chain_kernel, dim3(f.Ks * f.nbt), dim3(NT), lds, (hipStream_t)stream, f, sc);
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}
