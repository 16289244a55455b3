// A RAGGED chunk of teacher-forced frames of a streaming session per call (SampleStream.observe_many with lengths): the chunk chain
// of lfi_flow_chunk.hip with a length per batch row, and its entry point. A unit of its own for the reason that one is: a further
// chain kernel beside flow_fwd_seq_chain_kernel changes the inliner's choices there, and the dense chunk must stay what it is.
#include "lfi_flow_cells.h"

namespace {

// flow_fwd_seq_chain_kernel (lfi_flow_chunk.hip) in which batch row r takes the first lengths[r] frames only: the same workgroup map,
// tickets, hand-over slots (strides by the chunk's nframes) and waits. Workgroup (k, tile) loops to the tile's longest row - the same
// bound in every step k, so what (k, tile) publishes is what (k + 1, tile) waits for - and a tile whose rows all have length 0
// leaves before it asks for a weight. The cell (fwd_chain_cell<.., SEQ, RAG>) stores h / c at each row's own last frame and z / nll
// for the frames a row has; lengths outside [0, nframes] are clamped.
struct FwdSeqRowsChain {
  const float* frame0; long ld_frame;   // the chunk's first frame in the faces sequence (row stride seq_len * C); frame n: + n * C
  int nframes;
  float* tiles;           // [Ks - 1][nframes][B][C]: what step k hands to step k + 1
  float* q;               // [Ks - 1][nframes][B]: the rows' running log-det beside it
  const float* gic;       // [Ks][nframes][B][G]
  float *h, *cstate;      // [Ks][B][H] recurrent state: read at the first frame, row r written at its frame lengths[r] - 1
  int has_prev;           // 0: the chunk starts a sequence (zero state)
  unsigned* pipe;         // ticket, abort, progress words (frames published per (k, tile)); zeroed before the launch
  float* z;               // [nframes][B][C] or null; frames behind a row's length are not written
  float* nll;             // [nframes][B]; likewise
  const int* lengths;     // [B]
};
template <int NG, bool X3>
__global__ __launch_bounds__(NT) void flow_fwd_seq_rows_chain_kernel(FlowK f, FwdSeqRowsChain sc) {
  __shared__ int s_id, s_ok;
  if (threadIdx.x == 0) s_id = (int)atomicAdd(sc.pipe, 1u);
  __syncthreads();
  const int nbt = f.nbt;
  const int id = __builtin_amdgcn_readfirstlane(s_id);   // (what an LDS read gives is uniform here: the tile's lengths are then scalar loads)
  const int k = id / nbt, bt = id - k * nbt;
  if (k >= f.Ks) return;
  const int longest = tile_max_frames(sc.lengths, bt * MB, f.B, sc.nframes);
  if (longest == 0) return;   // (uniform; nobody waits for this tile: step k + 1 of it leaves here too)
  const bool last = k == f.Ks - 1;
  const long FB = (long)sc.nframes * f.B;
  unsigned* prog = sc.pipe + PIPE_HDR;
  CellIO io = {};
  FwdSeq sq = {};
  sq.frames = longest; sq.gic_step = (long)f.B * f.G; sq.row_step = f.B; sq.x_out_step = (long)f.B * f.C; sq.lengths = sc.lengths;
  io.k = k; io.rows = f.B;
  if (k == 0) { io.x_in = sc.frame0; io.ldx = sc.ld_frame; sq.x_in_step = f.C; }
  else { io.x_in = sc.tiles + (long)(k - 1) * FB * f.C; io.ldx = f.C; sq.x_in_step = (long)f.B * f.C; }
  io.x_out = last ? sc.z : sc.tiles + (long)k * FB * f.C; io.ldxo = f.C;
  io.h_prev = sc.has_prev ? sc.h + (long)k * f.B * f.H : nullptr;
  io.h_out = sc.h + (long)k * f.B * f.H;
  if (NG == 4) { io.c_prev = sc.has_prev ? sc.cstate + (long)k * f.B * f.H : nullptr; io.c_out = sc.cstate + (long)k * f.B * f.H; }
  io.gic = sc.gic + (long)k * FB * f.G;
  fwd_chain_cell<NG, X3, false, true, true>(f, io, bt * MB, k > 0 ? prog + (k - 1) * nbt + bt : nullptr, sc.pipe + 1,
                                            last ? nullptr : prog + k * nbt + bt, &s_ok, k > 0 ? sc.q + (long)(k - 1) * FB : nullptr,
                                            last ? nullptr : sc.q + (long)k * FB, last ? sc.nll : nullptr, &sq);
}

typedef void (*FlowFwdSeqRowsChainKernel)(FlowK, FwdSeqRowsChain);
FlowFwdSeqRowsChainKernel flow_fwd_seq_rows_chain_pick(const FramePlan& pl, bool lstm) {
  if (lstm) return flow_fwd_seq_rows_chain_kernel<4, false>;
  return pl.x3f ? flow_fwd_seq_rows_chain_kernel<3, true> : flow_fwd_seq_rows_chain_kernel<3, false>;
}

}  // namespace

// ---- lfi_flow_score_seq_chunk with a length per batch row: the same checks, work area and front end (dense over nframes * B windows)
extern "C" int lfi_flow_score_seq_chunk_rows(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E,
                                             int hist1, float* pre_static, float* faces, int seq_len, int start, int nframes,
                                             int first_frame, float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                                             float* chunk_work, float* z, float* nll, const int* lengths, void* stream) {
  FlowK f = {};
  const char* who = "lfi_flow_score_seq_chunk_rows";
  int rc = fill_flow(d, p, prep, &f, who);
  if (rc) return rc;
  FwdSeqRowsChain sc = {};
  FlowFwdSeqRowsChainKernel chain_kernel = nullptr;
  size_t lds = 0;
  // (chunk_front, lfi_flow_cells.h: as lfi_flow_score_seq_chunk; no kernel: LFI_CHUNK_ONLY=front)
  if ((rc = chunk_front(who, d, p, f, prep && wct && pre_static && faces && h && chunk_work && nll && lengths, wct, E, hist1, pre_static, faces,
                        seq_len, start, nframes, first_frame, h, cstate, p1, chunk_work, z, nll, stream, flow_fwd_seq_rows_chain_pick, &sc,
                        &chain_kernel, &lds)) || !chain_kernel) return rc;
  sc.lengths = lengths;
  hipLaunchKernelGGL(chain_kernel, dim3(f.Ks * f.nbt), dim3(NT), lds, (hipStream_t)stream, f, sc);
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}
