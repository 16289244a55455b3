// Streaming (frame-by-frame) sampling: the per-step state update of a sampling session (stream.py SampleStream).
//
// A session keeps, per conditioning modality with history > 0, the last `hist` frames of every batch row (B x hist x dim), the
// prev_p1_face window of its own output (B x (hist1 + 1) x C), the prior noise of the step and the frame counter. One launch moves
// all of it forward by one frame on the caller's stream; the static part and the reverse chain of the step (a captured graph) then
// read only session-owned, fixed-address memory. What SeqGlow.inference does with whole sequences (glow/models.py:567-596), one
// frame at a time. A second entry point puts listed batch rows back to the state of the open (SampleStream.reset_rows), between
// steps, leaving the other rows alone: conversations join and leave one batched session independently. Two more copy listed rows'
// live state out of a session into plain fp32 records and back into any session of the same model (SampleStream.save_rows /
// load_rows): conversations move between sessions, pause on the host, branch and roll back. One more installs the chosen one of every
// row's candidates for a frame (SampleStream.commit, after step_candidates). Two more stand around N candidate rollouts over a chunk of
// frames (SampleStream.rollout_candidates / commit): each row's faces sequence and state broadcast to its candidates, and the chosen
// candidate's frames, window and state installed.
#include "lfi_common.h"

#include <vector>

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

// The guard folds, one of which every kernel here ends with: max |v| (as bits) of what a thread moved goes into the session's guard
// word (NULL = no guard), which only grows between the session's clears. Per wave: one atomic from every wave that saw a value.
__device__ __forceinline__ void stream_guard_fold(unsigned m, unsigned* __restrict__ guard) {
  if (!guard) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(guard, m);
}

// Per workgroup of 256 (every thread calls it): one atomic, and none when the word already holds as much - the clears are
// stream-ordered before the launch, so a read of at least m means the result is at least m. Atomics on the one word serialise (~10 ns
// each on this chip): one per wave was most of a 64-row reset launch.
__device__ __forceinline__ void stream_guard_fold_block(unsigned m, unsigned* __restrict__ guard) {
  if (!guard) return;
  __shared__ unsigned wmax[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = wmax[0];
    for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
    if (m > __atomic_load_n(guard, __ATOMIC_RELAXED)) atomicMax(guard, m);
  }
}

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
  stream_guard_fold(m, guard);
}

// stream_advance_kernel for a step whose rows observe or generate one by one (SampleStream.step_rows): the same workgroup map and chunk
// order. Window face_win takes its source row only where the row observes (a generating row shifts only: the chain writes its newest
// row, and its row of the source is never read); the noise row is copied for every row and folded into the guard only where the row
// generates; workgroup (count, b) also leaves the row's role as one int for the chain.
__global__ __launch_bounds__(256) void stream_advance_rows_kernel(StreamWins w, int face_win, const float* __restrict__ noise,
                                                                 float* __restrict__ noise_dst, int C, float* __restrict__ frame_nb,
                                                                 const unsigned char* __restrict__ observed, int* __restrict__ role,
                                                                 unsigned* __restrict__ guard) {
  const int b = blockIdx.y;
  const int i = blockIdx.x;
  const bool observes = observed[b] != 0;
  unsigned m = 0u;
  if (i < w.count) {
    const int dim = w.dim[i];
    const long n = (long)w.hist[i] * dim;
    const long last = n - dim;                     // first element of the newest row
    float* win = w.win[i] + (long)b * n;
    const float* src = (i != face_win || observes) ? w.src[i] : nullptr;
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
      const unsigned a = observes ? 0u : stream_abs_bits(v);
      m = a > m ? a : m;
    }
    if (threadIdx.x == 0) {
      role[b] = observes ? 1 : 0;
      if (frame_nb) frame_nb[b] += 2.0f;
    }
  }
  stream_guard_fold(m, guard);
}

// ---- a chunk of n frames per call (SampleStream.observe_many / step_many / step_rows_many): the windows as sequences, and back.
// One kernel each way; what the calls differ in are nullable arguments (gen_win: -1 = none), and every branch on them is uniform over
// a workgroup.
struct StreamChunk {
  float* win[kStreamMaxWins];        // B x hist x dim, row b at b * hist * dim
  const float* src[kStreamMaxWins];  // B x n x dim: the chunk's frames (in only; NULL for a gen_win without roles)
  float* seq[kStreamMaxWins];        // B x (start + n) x dim
  int hist[kStreamMaxWins];
  int dim[kStreamMaxWins];
  int lead[kStreamMaxWins];
  int count;
};

// In: workgroup (i, b) lays window i of batch row b out as the sequence the sequence mode of the feature builder and the chains take,
// seq[i] (B x (start + n) x dim): the window's live frames (all hist of a conditioning window; rows 1 .. hist - 1 of the prev_p1_face
// window, lead = 1) end at frame start - 1, the chunk's n frames follow from frame `start`. Frames in front of the window are never
// read by anybody and never written here. max |v| of the NEW values that are used goes into the guard word, as
// stream_advance_kernel's.
//   i != gen_win: the row's first len frames of src, len = n or (lengths, a ragged chunk) the clamped lengths[b]; zeros behind len,
//     where the source is not read. (A row of length 0 still gets its live frames: the dense front end reads every row.)
//   i == gen_win (dim == C), the window a chain writes: the live frames only, and row b of the n noise frames (n x B x C, frame-major,
//     read where the caller keeps them) is folded into the guard word instead. With roles (n x B ints, frame-major; what n
//     stream_advance_rows_kernel launches move, in one): where roles[f * B + b] != 0 the row's given frame f of src enters the
//     sequence and the guard word, elsewhere the slot is left alone - the rows chain writes it - the given frame is not read and the
//     row's noise of that frame is folded.
__global__ __launch_bounds__(256) void stream_chunk_in_kernel(StreamChunk w, int n, int start, const int* __restrict__ lengths,
                                                              int gen_win, int B, const float* __restrict__ noise,
                                                              const int* __restrict__ roles, unsigned* __restrict__ guard) {
  const int b = blockIdx.y;
  const int i = blockIdx.x;
  const int dim = w.dim[i];
  const long live = (long)(w.hist[i] - w.lead[i]) * dim, fresh = (long)n * dim;
  const float* win = w.win[i] + ((long)b * w.hist[i] + w.lead[i]) * dim;
  float* seq = w.seq[i] + (long)b * (start + n) * dim + (long)start * dim;
  for (long j = threadIdx.x; j < live; j += 256) seq[j - live] = win[j];
  unsigned m = 0u;
  if (i != gen_win) {
    const float* src = w.src[i] + (long)b * fresh;
    const long mine = lengths ? (long)min(max(lengths[b], 0), n) * dim : fresh;
    for (long j = threadIdx.x; j < mine; j += 256) {
      const float v = src[j];
      seq[j] = v;
      const unsigned a = stream_abs_bits(v);
      m = a > m ? a : m;
    }
    for (long j = mine + threadIdx.x; j < fresh; j += 256) seq[j] = 0.0f;
  } else {
    for (int f = 0; f < n; ++f) {
      const bool observes = roles && roles[(long)f * B + b] != 0;
      const float* row = observes ? w.src[i] + (long)b * fresh + (long)f * dim : noise + ((long)f * B + b) * dim;
      for (int j = threadIdx.x; j < dim; j += 256) {
        const float v = row[j];
        if (observes) seq[(long)f * dim + j] = v;
        const unsigned a = stream_abs_bits(v);
        m = a > m ? a : m;
      }
    }
  }
  stream_guard_fold(m, guard);
}

// Out: workgroup (i, b) takes the last hist frames that end at frame start + len of seq[i] back into window i of batch row b - right
// for len below, at and above hist; len as above. The prev_p1_face window's hist counts its leading row, which so receives the frame
// in front of the last hist - 1: what len one-frame advances leave there. A ragged row of length 0 is not touched at all (its window
// is what it was; with hist - lead == start the leading row would be read from in front of the sequence). Workgroup (count, b): the
// row's frame counter += 2 len. With out, workgroup (gen_win, b) also hands the n fresh frames of row b to the caller (out + b *
// ld_out, n x C) and folds them into the guard word: what the next one-frame advance does with a frame step() generated.
__global__ __launch_bounds__(256) void stream_chunk_out_kernel(StreamChunk w, int n, int start, const int* __restrict__ lengths,
                                                               int gen_win, float* __restrict__ out, long ld_out,
                                                               float* __restrict__ frame_nb, unsigned* __restrict__ guard) {
  const int b = blockIdx.y;
  const int i = blockIdx.x;
  const int len = lengths ? min(max(lengths[b], 0), n) : n;
  if (len == 0) return;
  if (i == w.count) {
    if (frame_nb && threadIdx.x == 0) frame_nb[b] += 2.0f * (float)len;
    return;
  }
  const int dim = w.dim[i];
  const long tot = (long)w.hist[i] * dim;
  float* win = w.win[i] + (long)b * tot;
  const float* gen = w.seq[i] + ((long)b * (start + n) + start) * dim;      // the row's first fresh frame
  const float* seq = gen + (long)len * dim - tot;
  for (long j = threadIdx.x; j < tot; j += 256) win[j] = seq[j];
  if (i != gen_win || !out) return;
  const long fresh = (long)n * dim;
  float* dst = out + (long)b * ld_out;
  unsigned m = 0u;
  for (long j = threadIdx.x; j < fresh; j += 256) {
    const float v = gen[j];
    dst[j] = v;
    const unsigned a = stream_abs_bits(v);
    m = a > m ? a : m;
  }
  stream_guard_fold(m, guard);
}

// ---- per-row reseed (SampleStream.reset_rows): the state open_stream / reset() give a row, for a listed subset of rows
//
// Rows are passed by value in the kernel argument block (StreamReset.rows), at most kResetMaxRows per launch: no staging copy and no
// host wait; the host entry point splits a longer list into launches of its own.
constexpr int kResetMaxRows = 256;

struct StreamReset {
  float* win[kStreamMaxWins];         // B x hist x dim, row b at b * hist * dim
  const float* seed[kStreamMaxWins];  // list entry j's first copied frame at seed[i] + j * seed_ld[i]
  long seed_ld[kStreamMaxWins];
  int hist[kStreamMaxWins];
  int dim[kStreamMaxWins];
  int lead[kStreamMaxWins];           // 1: the window's frame 0 is zeroed and the seed fills frames 1.. (the prev_p1_face window)
  int count;
  int rows[kResetMaxRows];
};

// Workgroup (i, j): window i of session row rows[j], or (i = count) that row's coupling state h / c (all Ks flow steps) and its frame
// counter. Only the listed rows are written; max |v| of every seed value copied is folded into the guard word (never cleared here).
__global__ __launch_bounds__(256) void stream_reset_rows_kernel(StreamReset r, float* __restrict__ h, float* __restrict__ cstate, int B,
                                                                int Ks, int H, float* __restrict__ frame_nb, unsigned* __restrict__ guard) {
  const int j = blockIdx.y;
  const int i = blockIdx.x;
  const long b = r.rows[j];
  unsigned m = 0u;
  if (i < r.count) {
    const int dim = r.dim[i];
    const long n = (long)r.hist[i] * dim;
    const long lead = r.lead[i] ? dim : 0;
    float* win = r.win[i] + b * n;
    const float* src = r.seed[i] + (long)j * r.seed_ld[i];
    for (long e = threadIdx.x; e < n; e += 256) {
      float v = 0.0f;
      if (e >= lead) {
        v = src[e - lead];
        const unsigned a = stream_abs_bits(v);
        m = a > m ? a : m;
      }
      win[e] = v;
    }
  } else {
    // h / c: [Ks][B][H]. A zero row is what a null h_prev / c_prev gives the reverse cells (first_frame = 0)
    for (int k = 0; k < Ks; ++k) {
      const long o = ((long)k * B + b) * H;
      for (int c = threadIdx.x; c < H; c += 256) {
        h[o + c] = 0.0f;
        if (cstate) cstate[o + c] = 0.0f;
      }
    }
    if (frame_nb && threadIdx.x == 0) frame_nb[b] = -1.0f;   // the next advance's + 2 makes it inference's 1
  }
  stream_guard_fold_block(m, guard);
}

// ---- live rows out of and into a session (SampleStream.save_rows / load_rows): a conversation's whole state as one record
//
// A row's record is plain fp32, in this order: every window (count of them, the prev_p1_face window last, hist[i] x dim[i] each), h
// (Ks x H), c (Ks x H, LSTM only), the frame counter (one float, only with a counter). stream_record() is the one definition of that
// layout: lfi_stream_row_floats returns its R and both kernels take their offsets from it.
struct StreamRecord {
  long win[kStreamMaxWins];   // first float of window i
  long h, c, nb;              // first float of h / c / the counter (c, nb: -1 = not in the record)
  long R;
};

StreamRecord stream_record(int count, const int* hist, const int* dim, int Ks, int H, int lstm, int has_frame_nb) {
  StreamRecord t = {};
  long o = 0;
  for (int i = 0; i < count; ++i) { t.win[i] = o; o += (long)hist[i] * dim[i]; }
  t.h = o; o += (long)Ks * H;
  t.c = lstm ? o : -1; o += lstm ? (long)Ks * H : 0;
  t.nb = has_frame_nb ? o : -1; o += has_frame_nb ? 1 : 0;
  t.R = o;
  return t;
}

struct StreamMove {
  float* win[kStreamMaxWins];         // B x hist x dim, row b at b * hist * dim
  int hist[kStreamMaxWins];
  int dim[kStreamMaxWins];
  StreamRecord rec;
  int count;
  int rows[kResetMaxRows];            // session row of list position j
  int entries[kResetMaxRows];         // record of list position j (save: j itself, counted over the whole list)
};

// Workgroup (i, j): window i of session row rows[j], or (i = count) that row's coupling state h / c (all Ks flow steps) and its frame
// counter, between the session's buffers and record entries[j] of `data` (row stride ld). LOAD = false: session -> record, nothing
// of the session is written; zero_state writes zeros for h / c (a session that has not stepped: its first launch ignores what the
// buffers hold). LOAD = true: record -> session, only the listed rows are written, and max |v| of the windows and of c is folded
// into the guard word as stream_reset_rows_kernel does (|h| < 1; the counter is a frame number, which lfi_stream_advance does not
// fold either).
template <bool LOAD>
__global__ __launch_bounds__(256) void stream_move_rows_kernel(StreamMove r, float* __restrict__ h, float* __restrict__ cstate, int B,
                                                               int Ks, int H, float* __restrict__ frame_nb, int zero_state,
                                                               float* __restrict__ data, long ld, unsigned* __restrict__ guard) {
  const int j = blockIdx.y;
  const int i = blockIdx.x;
  const long b = r.rows[j];
  float* rec = data + (long)r.entries[j] * ld;
  unsigned m = 0u;
  if (i < r.count) {
    const long n = (long)r.hist[i] * r.dim[i];
    float* win = r.win[i] + b * n;
    float* rw = rec + r.rec.win[i];
    for (long e = threadIdx.x; e < n; e += 256) {
      if (LOAD) {
        const float v = rw[e];
        const unsigned a = stream_abs_bits(v);
        m = a > m ? a : m;
        win[e] = v;
      } else {
        rw[e] = win[e];
      }
    }
  } else {
    // h / c: [Ks][B][H] in the session, [Ks][H] in the record
    for (int k = 0; k < Ks; ++k) {
      const long o = ((long)k * B + b) * H;
      const long q = (long)k * H;
      for (int c = threadIdx.x; c < H; c += 256) {
        if (LOAD) {
          h[o + c] = rec[r.rec.h + q + c];
          if (cstate) {
            const float v = rec[r.rec.c + q + c];
            const unsigned a = stream_abs_bits(v);
            m = a > m ? a : m;
            cstate[o + c] = v;
          }
        } else {
          rec[r.rec.h + q + c] = zero_state ? 0.0f : h[o + c];
          if (cstate) rec[r.rec.c + q + c] = zero_state ? 0.0f : cstate[o + c];
        }
      }
    }
    if (frame_nb && threadIdx.x == 0) {
      if (LOAD) frame_nb[b] = rec[r.rec.nb];
      else rec[r.rec.nb] = frame_nb[b];
    }
  }
  if (LOAD) stream_guard_fold_block(m, guard);
}

// The argument checks save and load share (everything but the record side); fills r and the layout table.
int stream_move_args(const char* what, int B, int nrows, const int* rows, int count, float* const* win, const int* hist, const int* dim,
                     const float* h, const float* cstate, int Ks, int H, const float* frame_nb, StreamMove* r) {
  LFI_REQUIRE(B > 0 && B <= 65535, "%s: batch %d (1 .. 65535)", what, B);
  LFI_REQUIRE(nrows >= 1 && nrows <= B, "%s: %d rows (1 .. batch %d)", what, nrows, B);
  LFI_REQUIRE(rows, "%s: null row list", what);
  LFI_REQUIRE(count >= 0 && count <= kStreamMaxWins, "%s: %d windows (at most %d)", what, count, kStreamMaxWins);
  LFI_REQUIRE(count == 0 || (win && hist && dim), "%s: null window table", what);
  LFI_REQUIRE(h && Ks > 0 && H > 0, "%s: null h / Ks = %d, H = %d", what, Ks, H);
  for (int i = 0; i < count; ++i) {
    LFI_REQUIRE(win[i] && hist[i] > 0 && dim[i] > 0, "%s: window %d: hist %d, dim %d", what, i, hist[i], dim[i]);
    r->win[i] = win[i]; r->hist[i] = hist[i]; r->dim[i] = dim[i];
  }
  r->count = count;
  r->rec = stream_record(count, hist, dim, Ks, H, cstate != nullptr, frame_nb != nullptr);
  std::vector<unsigned char> seen(B, 0);
  for (int j = 0; j < nrows; ++j) {
    LFI_REQUIRE(rows[j] >= 0 && rows[j] < B, "%s: row %d of the list is %d, outside the batch (0 .. %d)", what, j, rows[j], B - 1);
    LFI_REQUIRE(!seen[rows[j]], "%s: row %d is listed twice", what, rows[j]);
    seen[rows[j]] = 1;
  }
  return LFI_OK;
}

// What a chunk window launch takes beyond the window tables. An entry point names what it has (`kind`: those pointers are required)
// and leaves the rest as it is here, which the kernels take as "not there".
enum : unsigned { kChunkIn = 1u, kChunkRagged = 2u, kChunkGen = 4u, kChunkRoles = 8u };

struct StreamChunkOpts {
  const float* const* src = nullptr;   // kChunkIn: the chunk's frames per window
  const int* lengths = nullptr;        // kChunkRagged
  int gen_win = -1;                    // kChunkGen ...
  const float* noise = nullptr;        // ... in
  int C = 0;
  float* out = nullptr;                // ... out
  long ld_out = 0;
  const int* roles = nullptr;          // kChunkRoles (in, with kChunkGen): the generated window's source is then required too
};

// The argument checks of the seven chunk entry points, before any launch; fills w.
int stream_chunk_args(const char* what, unsigned kind, int B, int n, int start, int count, float* const* win, float* const* seq,
                      const int* hist, const int* dim, const int* lead, const StreamChunkOpts& o, StreamChunk* w) {
  const bool in = kind & kChunkIn, gen = kind & kChunkGen, roles = kind & kChunkRoles;
  LFI_REQUIRE(B > 0 && B <= 65535, "%s: batch %d (1 .. 65535)", what, B);
  LFI_REQUIRE(n >= 1 && start >= 0 && (long)start + n < (1L << 30), "%s: %d frames from frame %d", what, n, start);
  LFI_REQUIRE(count >= 1 && count <= kStreamMaxWins, "%s: %d windows (1 .. %d)", what, count, kStreamMaxWins);
  LFI_REQUIRE(win && seq && hist && dim && lead, "%s: null pointer (window table)", what);
  // (hist - lead <= start and a written row's len >= 1: the last hist frames of a sequence lie inside what in and the chain wrote)
  for (int i = 0; i < count; ++i) {
    LFI_REQUIRE(win[i] && seq[i], "%s: null pointer (window %d)", what, i);
    LFI_REQUIRE(hist[i] > 0 && dim[i] > 0 && (lead[i] == 0 || lead[i] == 1) && hist[i] - lead[i] <= start,
                "%s: window %d: hist %d, dim %d, lead %d, start %d", what, i, hist[i], dim[i], lead[i], start);
    w->win[i] = win[i]; w->seq[i] = seq[i]; w->hist[i] = hist[i]; w->dim[i] = dim[i]; w->lead[i] = lead[i];
  }
  w->count = count;
  if (in) LFI_REQUIRE(o.src && (!gen || o.noise), "%s: null pointer (source table%s)", what, gen ? " / noise" : "");
  if (kind & kChunkRagged) LFI_REQUIRE(o.lengths, "%s: null pointer (lengths)", what);
  if (roles) LFI_REQUIRE(o.roles, "%s: null pointer (roles)", what);
  if (gen && !in) LFI_REQUIRE(o.out, "%s: null pointer (out)", what);
  if (gen) LFI_REQUIRE(o.gen_win >= 0 && o.gen_win < count, "%s: generated window %d of %d", what, o.gen_win, count);
  if (gen && in)
    LFI_REQUIRE(o.C > 0 && dim[o.gen_win] == o.C, "%s: generated window %d has dim %d, the noise C = %d", what, o.gen_win,
                dim[o.gen_win], o.C);
  if (gen && !in)
    LFI_REQUIRE(o.ld_out >= (long)n * dim[o.gen_win], "%s: out row pitch %ld below the %d frames' %ld floats", what, o.ld_out, n,
                (long)n * dim[o.gen_win]);
  for (int i = 0; in && i < count; ++i) {
    // (the generated window has no source - the chain writes its frames - but with roles: the given frames of the rows that observe)
    const bool none = gen && !roles && i == o.gen_win;
    LFI_REQUIRE(none || o.src[i], "%s: null pointer (source %d)", what, i);
    w->src[i] = none ? nullptr : o.src[i];
  }
  return LFI_OK;
}

// ---- best-of-N (SampleStream.step_candidates / commit): one of a row's candidates becomes the row's frame
//
// Workgroup r: session row r. Thread 0 picks j - the clamped choice[r], or (choice == NULL) the arg-min of the row's ncand NLL words:
// ties go to the lowest index, NaN counts as larger than any number, all NaN picks 0 - then the workgroup copies candidate (r, j): its
// frame into the newest slot of the row's faces window and into out_frame, its h / c of every flow step into the session's, its NLL
// word and j into out_nll / out_choice. Every word has one writer; the frame is folded into the guard word as a window value is.
__global__ __launch_bounds__(256) void stream_commit_cand_kernel(int B, int ncand, int C, int Ks, int H, const int* __restrict__ choice,
                                                                const float* __restrict__ cand_frames,
                                                                const float* __restrict__ cand_nll, const float* __restrict__ cand_h,
                                                                const float* __restrict__ cand_c, float* __restrict__ face_win,
                                                                int hist, float* __restrict__ h, float* __restrict__ cstate,
                                                                float* __restrict__ out_frame, float* __restrict__ out_nll,
                                                                int* __restrict__ out_choice, unsigned* __restrict__ guard) {
  __shared__ int s_j;
  const long r = blockIdx.x;
  if (threadIdx.x == 0) {
    int j = 0;
    if (choice) {
      j = min(max(choice[r], 0), ncand - 1);
    } else {
      float best = cand_nll[r * ncand];
      for (int i = 1; i < ncand; ++i) {
        const float v = cand_nll[r * ncand + i];
        if (v < best || (best != best && v == v)) { best = v; j = i; }
      }
    }
    s_j = j;
    out_choice[r] = j;
    out_nll[r] = cand_nll[r * ncand + j];
  }
  __syncthreads();
  const long v = r * ncand + s_j, V = (long)B * ncand;
  unsigned m = 0u;
  float* slot = face_win + (r * hist + (hist - 1)) * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float x = cand_frames[v * C + c];
    slot[c] = x;
    out_frame[r * C + c] = x;
    const unsigned a = stream_abs_bits(x);
    m = a > m ? a : m;
  }
  for (int e = threadIdx.x; e < Ks * H; e += 256) {
    const int k = e / H, c = e - k * H;
    const long src = ((long)k * V + v) * H + c, dst = ((long)k * B + r) * H + c;
    h[dst] = cand_h[src];
    if (cstate) cstate[dst] = cand_c[src];
  }
  stream_guard_fold_block(m, guard);
}

// ---- N candidate rollouts of n frames per row (SampleStream.rollout_candidates / commit / discard). V = B * ncand virtual rows, row
// v = b * ncand + j: candidate j of session row b. Nothing the session owns is written before the commit.
//
// In: workgroup (v, part). Part 0: the first `start` frames of the parent's faces sequence (parent_seq, B x (start + n) x C, as
// stream_chunk_in_kernel left it) go to the candidate's own sequence (cand_seq, V x (start + n) x C), whose frames start .. are the
// chain's to write. Part 1 (has_prev): the parent's h / c of every flow step go to the candidate's state ([Ks][V][H]). Part 2: the
// candidate's n noise rows (n x V x C, frame-major, read where the caller keeps them) are folded into the guard word.
__global__ __launch_bounds__(256) void stream_cand_seq_in_kernel(int B, int ncand, int n, int start, int C, int Ks, int H,
                                                                const float* __restrict__ parent_seq, float* __restrict__ cand_seq,
                                                                const float* __restrict__ h, const float* __restrict__ cstate,
                                                                float* __restrict__ cand_h, float* __restrict__ cand_c, int has_prev,
                                                                const float* __restrict__ noise, unsigned* __restrict__ guard) {
  const long v = blockIdx.x, V = (long)B * ncand, b = v / ncand;
  const int part = blockIdx.y;
  unsigned m = 0u;
  if (part == 0) {
    const long T = (long)start + n, live = (long)start * C;
    const float* src = parent_seq + b * T * C;
    float* dst = cand_seq + v * T * C;
    for (long j = threadIdx.x; j < live; j += 256) dst[j] = src[j];
  } else if (part == 1) {
    if (has_prev) {
      for (int e = threadIdx.x; e < Ks * H; e += 256) {
        const int k = e / H, c = e - k * H;
        const long src = ((long)k * B + b) * H + c, dst = ((long)k * V + v) * H + c;
        cand_h[dst] = h[src];
        if (cstate) cand_c[dst] = cstate[src];
      }
    }
  } else {
    for (int f = 0; f < n; ++f) {
      const float* row = noise + ((long)f * V + v) * C;
      for (int j = threadIdx.x; j < C; j += 256) {
        const unsigned a = stream_abs_bits(row[j]);
        m = a > m ? a : m;
      }
    }
  }
  stream_guard_fold_block(m, guard);
}

// Of two (summed NLL, index) pairs the one a commit prefers: the smaller sum; a NaN sum loses to any number; equal sums and two NaNs
// go to the lower index.
__device__ __forceinline__ bool stream_cand_better(float a, int ia, float b, int ib) {
  if (a < b || (b != b && a == a)) return true;
  if (b < a || (a != a && b == b)) return false;
  return ia < ib;
}

// Commit: workgroup r, session row r. j = the clamped choice[r], or (choice == NULL) the candidate of least summed NLL - every sum
// runs over the frames in ascending order in fp32 (one thread per candidate, no reassociation), ties to the lowest index, a NaN sum
// never wins unless all are NaN, then 0. Then candidate (r, j)'s n frames go to out (B x n x C) and into the guard word, the last
// hist frames of its sequence (they end at frame start + n; hist <= start + n) into the row's faces window, its h / c of every flow
// step into the session's, its n NLL words to out_nll (n x B), j to out_choice, and the row's frame counter moves by 2 n. Every word
// has one writer.
__global__ __launch_bounds__(256) void stream_commit_cand_seq_kernel(int B, int ncand, int n, int start, int C, int Ks, int H,
                                                                    const int* __restrict__ choice, const float* __restrict__ cand_seq,
                                                                    const float* __restrict__ cand_nll, const float* __restrict__ cand_h,
                                                                    const float* __restrict__ cand_c, float* __restrict__ face_win,
                                                                    int hist, float* __restrict__ h, float* __restrict__ cstate,
                                                                    float* __restrict__ frame_nb, float* __restrict__ out,
                                                                    float* __restrict__ out_nll, int* __restrict__ out_choice,
                                                                    unsigned* __restrict__ guard) {
  __shared__ float s_sum[256];
  __shared__ int s_idx[256];
  __shared__ int s_j;
  const long r = blockIdx.x, V = (long)B * ncand;
  const int tid = threadIdx.x;
  if (choice) {
    if (tid == 0) s_j = min(max(choice[r], 0), ncand - 1);
  } else {
    float best = 0.0f;
    int bi = -1;                                   // (no candidate of this thread's yet)
    for (int i = tid; i < ncand; i += 256) {
      float sum = 0.0f;
      for (int f = 0; f < n; ++f) sum = __fadd_rn(sum, cand_nll[(long)f * V + r * ncand + i]);
      if (bi < 0 || stream_cand_better(sum, i, best, bi)) { best = sum; bi = i; }
    }
    s_sum[tid] = best; s_idx[tid] = bi;
    __syncthreads();
    if (tid == 0) {
      for (int t = 1; t < 256 && t < ncand; ++t)
        if (stream_cand_better(s_sum[t], s_idx[t], best, bi)) { best = s_sum[t]; bi = s_idx[t]; }
      s_j = bi;
    }
  }
  __syncthreads();
  const int j = s_j;
  const long v = r * ncand + j, T = (long)start + n;
  const float* seq = cand_seq + v * T * C;
  if (tid == 0) {
    out_choice[r] = j;
    if (frame_nb) frame_nb[r] += 2.0f * (float)n;
  }
  for (int f = tid; f < n; f += 256) out_nll[(long)f * B + r] = cand_nll[(long)f * V + v];
  unsigned m = 0u;
  const float* gen = seq + (long)start * C;
  float* dst = out + r * (long)n * C;
  for (long e = tid; e < (long)n * C; e += 256) {
    const float x = gen[e];
    dst[e] = x;
    const unsigned a = stream_abs_bits(x);
    m = a > m ? a : m;
  }
  const long tot = (long)hist * C;
  const float* tail = seq + T * C - tot;
  float* win = face_win + r * tot;
  for (long e = tid; e < tot; e += 256) win[e] = tail[e];
  for (int e = tid; e < Ks * H; e += 256) {
    const int k = e / H, c = e - k * H;
    const long src = ((long)k * V + v) * H + c, to = ((long)k * B + r) * H + c;
    h[to] = cand_h[src];
    if (cstate) cstate[to] = cand_c[src];
  }
  stream_guard_fold_block(m, guard);
}

// The checks and the launch of a chunk entry point: windows in (kChunkIn) or out.
int stream_chunk_launch(const char* what, unsigned kind, int B, int n, int start, int count, float* const* win, float* const* seq,
                        const int* hist, const int* dim, const int* lead, const StreamChunkOpts& o, float* frame_nb, unsigned* guard,
                        void* stream) {
  StreamChunk w = {};
  const int rc = stream_chunk_args(what, kind, B, n, start, count, win, seq, hist, dim, lead, o, &w);
  if (rc != LFI_OK) return rc;
  if (kind & kChunkIn)
    hipLaunchKernelGGL(stream_chunk_in_kernel, dim3(count, B), dim3(256), 0, (hipStream_t)stream, w, n, start, o.lengths, o.gen_win, B,
                       o.noise, o.roles, guard);
  else
    hipLaunchKernelGGL(stream_chunk_out_kernel, dim3(count + 1, B), dim3(256), 0, (hipStream_t)stream, w, n, start, o.lengths, o.gen_win,
                       o.out, o.ld_out, frame_nb, guard);
  LFI_LAUNCH_CHECK(what);
  return LFI_OK;
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

extern "C" int lfi_stream_advance_rows(int B, int count, float* const* win, const float* const* src, const int* hist, const int* dim,
                                       int face_win, const float* noise, float* noise_dst, int C, float* frame_nb,
                                       const unsigned char* observed, int* role, unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_advance_rows: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(count >= 1 && count <= kStreamMaxWins, "lfi_stream_advance_rows: %d windows (1 .. %d)", count, kStreamMaxWins);
  LFI_REQUIRE(win && src && hist && dim, "lfi_stream_advance_rows: null window table");
  LFI_REQUIRE(noise && noise_dst && C > 0, "lfi_stream_advance_rows: null noise / C = %d", C);
  LFI_REQUIRE(observed && role, "lfi_stream_advance_rows: null observed / role");
  LFI_REQUIRE(face_win >= 0 && face_win < count && src[face_win], "lfi_stream_advance_rows: face window %d of %d, or its source is null",
              face_win, count);
  StreamWins w = {};
  for (int i = 0; i < count; ++i) {
    LFI_REQUIRE(win[i] && hist[i] > 0 && dim[i] > 0, "lfi_stream_advance_rows: window %d: hist %d, dim %d", i, hist[i], dim[i]);
    w.win[i] = win[i]; w.src[i] = src[i]; w.hist[i] = hist[i]; w.dim[i] = dim[i];
  }
  w.count = count;
  hipLaunchKernelGGL(stream_advance_rows_kernel, dim3(count + 1, B), dim3(256), 0, (hipStream_t)stream, w, face_win, noise, noise_dst, C,
                     frame_nb, observed, role, guard_bits);
  LFI_LAUNCH_CHECK("lfi_stream_advance_rows");
  return LFI_OK;
}

extern "C" int lfi_stream_reset_rows(int B, int nrows, const int* rows, int count, float* const* win, const float* const* seed,
                                     const long* seed_ld, const int* hist, const int* dim, const int* lead_zero, float* h, float* cstate,
                                     int Ks, int H, float* frame_nb, unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_reset_rows: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(nrows >= 1 && nrows <= B, "lfi_stream_reset_rows: %d rows (1 .. batch %d)", nrows, B);
  LFI_REQUIRE(rows, "lfi_stream_reset_rows: null row list");
  LFI_REQUIRE(count >= 0 && count <= kStreamMaxWins, "lfi_stream_reset_rows: %d windows (at most %d)", count, kStreamMaxWins);
  LFI_REQUIRE(count == 0 || (win && seed && seed_ld && hist && dim && lead_zero), "lfi_stream_reset_rows: null window table");
  LFI_REQUIRE(h && Ks > 0 && H > 0, "lfi_stream_reset_rows: null h / Ks = %d, H = %d", Ks, H);
  StreamReset r = {};
  for (int i = 0; i < count; ++i) {
    LFI_REQUIRE(win[i] && hist[i] > 0 && dim[i] > 0 && (lead_zero[i] == 0 || lead_zero[i] == 1),
                "lfi_stream_reset_rows: window %d: hist %d, dim %d, lead_zero %d", i, hist[i], dim[i], lead_zero[i]);
    const long frames = hist[i] - lead_zero[i];
    LFI_REQUIRE(frames == 0 || (seed[i] && seed_ld[i] >= frames * dim[i]),
                "lfi_stream_reset_rows: window %d: null seed or seed row stride %ld < %ld", i, seed_ld[i], frames * dim[i]);
    r.win[i] = win[i]; r.seed[i] = frames ? seed[i] : nullptr; r.seed_ld[i] = seed_ld[i];
    r.hist[i] = hist[i]; r.dim[i] = dim[i]; r.lead[i] = lead_zero[i];
  }
  r.count = count;
  std::vector<unsigned char> seen(B, 0);
  for (int j = 0; j < nrows; ++j) {
    LFI_REQUIRE(rows[j] >= 0 && rows[j] < B, "lfi_stream_reset_rows: row %d of the list is %d, outside the batch (0 .. %d)", j, rows[j],
                B - 1);
    LFI_REQUIRE(!seen[rows[j]], "lfi_stream_reset_rows: row %d is listed twice", rows[j]);
    seen[rows[j]] = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < nrows; j0 += kResetMaxRows) {
    const int n = nrows - j0 < kResetMaxRows ? nrows - j0 : kResetMaxRows;
    for (int i = 0; i < count; ++i) r.seed[i] = r.seed[i] ? seed[i] + (long)j0 * seed_ld[i] : nullptr;
    for (int j = 0; j < n; ++j) r.rows[j] = rows[j0 + j];
    hipLaunchKernelGGL(stream_reset_rows_kernel, dim3(count + 1, n), dim3(256), 0, st, r, h, cstate, B, Ks, H, frame_nb, guard_bits);
    LFI_LAUNCH_CHECK("lfi_stream_reset_rows");
  }
  return LFI_OK;
}

extern "C" long lfi_stream_row_floats(int count, const int* hist, const int* dim, int Ks, int H, int lstm, int has_frame_nb) {
  LFI_REQUIRE(count >= 0 && count <= kStreamMaxWins, "lfi_stream_row_floats: %d windows (at most %d)", count, kStreamMaxWins);
  LFI_REQUIRE(count == 0 || (hist && dim), "lfi_stream_row_floats: null window table");
  LFI_REQUIRE(Ks > 0 && H > 0, "lfi_stream_row_floats: Ks = %d, H = %d", Ks, H);
  for (int i = 0; i < count; ++i)
    LFI_REQUIRE(hist[i] > 0 && dim[i] > 0, "lfi_stream_row_floats: window %d: hist %d, dim %d", i, hist[i], dim[i]);
  return stream_record(count, hist, dim, Ks, H, lstm != 0, has_frame_nb != 0).R;
}

extern "C" int lfi_stream_save_rows(int B, int nrows, const int* rows, int count, const float* const* win, const int* hist,
                                    const int* dim, const float* h, const float* cstate, int Ks, int H, const float* frame_nb,
                                    int zero_state, float* out, long ld_out, void* stream) {
  StreamMove r = {};
  // (the save kernel only reads the session's buffers: one kernel body serves both directions, hence the casts)
  const int rc = stream_move_args("lfi_stream_save_rows", B, nrows, rows, count, const_cast<float* const*>(win), hist, dim, h, cstate, Ks,
                                  H, frame_nb, &r);
  if (rc != LFI_OK) return rc;
  LFI_REQUIRE(out, "lfi_stream_save_rows: null out");
  LFI_REQUIRE(ld_out >= r.rec.R, "lfi_stream_save_rows: record stride %ld below the record's %ld floats", ld_out, r.rec.R);
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < nrows; j0 += kResetMaxRows) {
    const int n = nrows - j0 < kResetMaxRows ? nrows - j0 : kResetMaxRows;
    for (int j = 0; j < n; ++j) { r.rows[j] = rows[j0 + j]; r.entries[j] = j0 + j; }
    hipLaunchKernelGGL(stream_move_rows_kernel<false>, dim3(count + 1, n), dim3(256), 0, st, r, const_cast<float*>(h),
                       const_cast<float*>(cstate), B, Ks, H, const_cast<float*>(frame_nb), zero_state ? 1 : 0, out, ld_out,
                       (unsigned*)nullptr);
    LFI_LAUNCH_CHECK("lfi_stream_save_rows");
  }
  return LFI_OK;
}

extern "C" int lfi_stream_load_rows(int B, int nrows, const int* rows, const int* entries, int nentries, int count, float* const* win,
                                    const int* hist, const int* dim, float* h, float* cstate, int Ks, int H, float* frame_nb,
                                    const float* in, long ld_in, unsigned* guard_bits, void* stream) {
  StreamMove r = {};
  const int rc = stream_move_args("lfi_stream_load_rows", B, nrows, rows, count, win, hist, dim, h, cstate, Ks, H, frame_nb, &r);
  if (rc != LFI_OK) return rc;
  LFI_REQUIRE(in, "lfi_stream_load_rows: null in");
  LFI_REQUIRE(nentries >= 1, "lfi_stream_load_rows: %d saved entries (at least 1)", nentries);
  LFI_REQUIRE(entries, "lfi_stream_load_rows: null entry list");
  for (int j = 0; j < nrows; ++j)
    LFI_REQUIRE(entries[j] >= 0 && entries[j] < nentries, "lfi_stream_load_rows: entry %d of the list is %d, outside the saved entries (0 .. %d)",
                j, entries[j], nentries - 1);
  LFI_REQUIRE(ld_in >= r.rec.R, "lfi_stream_load_rows: record stride %ld below the record's %ld floats", ld_in, r.rec.R);
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < nrows; j0 += kResetMaxRows) {
    const int n = nrows - j0 < kResetMaxRows ? nrows - j0 : kResetMaxRows;
    for (int j = 0; j < n; ++j) { r.rows[j] = rows[j0 + j]; r.entries[j] = entries[j0 + j]; }
    hipLaunchKernelGGL(stream_move_rows_kernel<true>, dim3(count + 1, n), dim3(256), 0, st, r, h, cstate, B, Ks, H, frame_nb, 0,
                       const_cast<float*>(in), ld_in, guard_bits);
    LFI_LAUNCH_CHECK("lfi_stream_load_rows");
  }
  return LFI_OK;
}

extern "C" int lfi_stream_chunk_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                                   const int* hist, const int* dim, const int* lead, unsigned* guard_bits, void* stream) {
  StreamChunkOpts o;
  o.src = src;
  return stream_chunk_launch("lfi_stream_chunk_in", kChunkIn, B, n, start, count, win, seq, hist, dim, lead, o, nullptr, guard_bits, stream);
}

extern "C" int lfi_stream_chunk_out(int B, int n, int start, int count, float* const* win, float* const* seq, const int* hist,
                                    const int* dim, const int* lead, float* frame_nb, void* stream) {
  return stream_chunk_launch("lfi_stream_chunk_out", 0u, B, n, start, count, win, seq, hist, dim, lead, StreamChunkOpts(), frame_nb, nullptr,
                             stream);
}

extern "C" int lfi_stream_chunk_in_rows(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                                        const int* hist, const int* dim, const int* lead, unsigned* guard_bits, const int* lengths,
                                        void* stream) {
  StreamChunkOpts o;
  o.src = src; o.lengths = lengths;
  return stream_chunk_launch("lfi_stream_chunk_in_rows", kChunkIn | kChunkRagged, B, n, start, count, win, seq, hist, dim, lead, o, nullptr,
                             guard_bits, stream);
}

extern "C" int lfi_stream_chunk_out_rows(int B, int n, int start, int count, float* const* win, float* const* seq, const int* hist,
                                         const int* dim, const int* lead, float* frame_nb, const int* lengths, void* stream) {
  StreamChunkOpts o;
  o.lengths = lengths;
  return stream_chunk_launch("lfi_stream_chunk_out_rows", kChunkRagged, B, n, start, count, win, seq, hist, dim, lead, o, frame_nb, nullptr,
                             stream);
}

extern "C" int lfi_stream_chunk_gen_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                                       const int* hist, const int* dim, const int* lead, int gen_win, const float* noise, int C,
                                       unsigned* guard_bits, void* stream) {
  StreamChunkOpts o;
  o.src = src; o.gen_win = gen_win; o.noise = noise; o.C = C;
  return stream_chunk_launch("lfi_stream_chunk_gen_in", kChunkIn | kChunkGen, B, n, start, count, win, seq, hist, dim, lead, o, nullptr,
                             guard_bits, stream);
}

extern "C" int lfi_stream_chunk_roles_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                                         const int* hist, const int* dim, const int* lead, int gen_win, const float* noise, int C,
                                         const int* roles, unsigned* guard_bits, void* stream) {
  StreamChunkOpts o;
  o.src = src; o.gen_win = gen_win; o.noise = noise; o.C = C; o.roles = roles;
  return stream_chunk_launch("lfi_stream_chunk_roles_in", kChunkIn | kChunkGen | kChunkRoles, B, n, start, count, win, seq, hist, dim, lead,
                             o, nullptr, guard_bits, stream);
}

extern "C" int lfi_stream_chunk_gen_out(int B, int n, int start, int count, float* const* win, float* const* seq, const int* hist,
                                        const int* dim, const int* lead, int gen_win, float* out, long ld_out, float* frame_nb,
                                        unsigned* guard_bits, void* stream) {
  StreamChunkOpts o;
  o.gen_win = gen_win; o.out = out; o.ld_out = ld_out;
  return stream_chunk_launch("lfi_stream_chunk_gen_out", kChunkGen, B, n, start, count, win, seq, hist, dim, lead, o, frame_nb, guard_bits,
                             stream);
}

extern "C" int lfi_stream_commit_cand(int B, int ncand, int C, int Ks, int H, const int* choice, const float* cand_frames,
                                      const float* cand_nll, const float* cand_h, const float* cand_c, float* face_win, int hist,
                                      float* h, float* cstate, float* out_frame, float* out_nll, int* out_choice,
                                      unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_commit_cand: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(ncand >= 1 && (long)B * ncand <= (1L << 22), "lfi_stream_commit_cand: %d candidates per row at batch %d", ncand, B);
  LFI_REQUIRE(C > 0 && Ks > 0 && H > 0 && hist >= 1, "lfi_stream_commit_cand: C = %d, Ks = %d, H = %d, hist = %d", C, Ks, H, hist);
  LFI_REQUIRE(cand_frames && cand_nll && cand_h && face_win && h && out_frame && out_nll && out_choice,
              "lfi_stream_commit_cand: null pointer");
  LFI_REQUIRE(!cstate || cand_c, "lfi_stream_commit_cand: cstate without cand_c");
  hipLaunchKernelGGL(stream_commit_cand_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, B, ncand, C, Ks, H, choice, cand_frames, cand_nll,
                     cand_h, cand_c, face_win, hist, h, cstate, out_frame, out_nll, out_choice, guard_bits);
  LFI_LAUNCH_CHECK("lfi_stream_commit_cand");
  return LFI_OK;
}

extern "C" int lfi_stream_cand_seq_in(int B, int ncand, int n, int start, int C, int Ks, int H, const float* parent_seq, float* cand_seq,
                                      const float* h, const float* cstate, float* cand_h, float* cand_c, int first_frame,
                                      const float* noise, unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_cand_seq_in: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(ncand >= 1 && (long)B * ncand <= (1L << 22), "lfi_stream_cand_seq_in: %d candidates per row at batch %d", ncand, B);
  LFI_REQUIRE(n >= 1 && start >= 0 && (long)start + n < (1L << 30), "lfi_stream_cand_seq_in: %d frames from frame %d", n, start);
  LFI_REQUIRE(C > 0 && Ks > 0 && H > 0 && first_frame >= 0, "lfi_stream_cand_seq_in: C = %d, Ks = %d, H = %d, first_frame = %d", C, Ks, H,
              first_frame);
  LFI_REQUIRE(parent_seq && cand_seq && h && cand_h && noise, "lfi_stream_cand_seq_in: null pointer");
  LFI_REQUIRE(!cstate || cand_c, "lfi_stream_cand_seq_in: cstate without cand_c");
  hipLaunchKernelGGL(stream_cand_seq_in_kernel, dim3(B * ncand, 3), dim3(256), 0, (hipStream_t)stream, B, ncand, n, start, C, Ks, H, parent_seq,
                     cand_seq, h, cstate, cand_h, cand_c, first_frame > 0 ? 1 : 0, noise, guard_bits);
  LFI_LAUNCH_CHECK("lfi_stream_cand_seq_in");
  return LFI_OK;
}

extern "C" int lfi_stream_commit_cand_seq(int B, int ncand, int n, int start, int C, int Ks, int H, const int* choice,
                                          const float* cand_seq, const float* cand_nll, const float* cand_h, const float* cand_c,
                                          float* face_win, int hist, float* h, float* cstate, float* frame_nb, float* out, float* out_nll,
                                          int* out_choice, unsigned* guard_bits, void* stream) {
  LFI_REQUIRE(B > 0 && B <= 65535, "lfi_stream_commit_cand_seq: batch %d (1 .. 65535)", B);
  LFI_REQUIRE(ncand >= 1 && (long)B * ncand <= (1L << 22), "lfi_stream_commit_cand_seq: %d candidates per row at batch %d", ncand, B);
  LFI_REQUIRE(n >= 1 && start >= 0 && (long)start + n < (1L << 30), "lfi_stream_commit_cand_seq: %d frames from frame %d", n, start);
  LFI_REQUIRE(C > 0 && Ks > 0 && H > 0 && hist >= 1 && hist <= start + n,
              "lfi_stream_commit_cand_seq: C = %d, Ks = %d, H = %d, hist = %d (1 .. start + n = %d)", C, Ks, H, hist, start + n);
  LFI_REQUIRE(cand_seq && cand_nll && cand_h && face_win && h && out && out_nll && out_choice, "lfi_stream_commit_cand_seq: null pointer");
  LFI_REQUIRE(!cstate || cand_c, "lfi_stream_commit_cand_seq: cstate without cand_c");
  hipLaunchKernelGGL(stream_commit_cand_seq_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, B, ncand, n, start, C, Ks, H, choice, cand_seq,
                     cand_nll, cand_h, cand_c, face_win, hist, h, cstate, frame_nb, out, out_nll, out_choice, guard_bits);
  LFI_LAUNCH_CHECK("lfi_stream_commit_cand_seq");
  return LFI_OK;
}
