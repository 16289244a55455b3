/*
 * lfi.h — C ABI of liblfi_hip.so: the MI355X (gfx950) kernels behind the conditional-Glow hot path of
 * jonepatr/lets_face_it.
 *
 * The reference has no FFI of its own for this path (it is pure PyTorch: SURVEY.md §8b); the Python object
 * surface it exposes (SeqGlow.forward / inference / invert, LetsFaceItGlow.training_step /
 * configure_optimizers) is mirrored by lets_face_it_amd/glow/, and THIS header is what that host code binds
 * with ctypes. Each entry point names the reference code it replaces (paths relative to
 * /root/reference/code/glow_pytorch/).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; every pointer is a DEVICE pointer to fp32 unless noted.
 *  - The caller owns every buffer; the library allocates nothing and keeps no global mutable state in normal operation (per
 *    thread: the last error message; process-wide and null unless a diagnostic tool sets it: lfi_debug_set_stamps's pointer).
 *  - `stream` is a hipStream_t passed as void* (torch's current stream); all work is enqueued on it, no host
 *    synchronisation, so every call is hipGraph-capturable.
 *  - Return value: 0 = ok, < 0 = error; the message is in lfi_last_error() (thread-local).
 *  - Frames are time-major: frame f = n * B + b for timestep n (0 .. N-1) and sample b.
 */
#ifndef LFI_H
#define LFI_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFI_OK 0
#define LFI_ERR_ARG (-1)
#define LFI_ERR_LAUNCH (-2)
#define LFI_ERR_UNSUPPORTED (-3)

const char* lfi_last_error(void);
int lfi_version(void);

/* ---------------------------------------------------------------- generic fp32 GEMM on MFMA
 * C[b] (+)= act( opA(A[b]) * opB(B[b]) + bias[b] ) ,  b = 0 .. batch-1
 *   a_kcontig = 1: A element (m,k) at A[m*lda + k];  0: at A[k*lda + m]
 *   b_kcontig = 1: B element (k,n) at B[n*ldb + k];  0: at B[k*ldb + n]
 * act: 0 none | 1 leaky_relu(slope) | 2 multiply by leaky_relu'(G) (G same shape/ld as C: G > 0 ? 1 : slope)
 * splitk > 1 needs `work` of lfi_gemm_work_floats() floats; partial sums are reduced deterministically.
 * Replaces the aten::addmm / aten::mm calls of nn.Linear / nn.GRU input projections and their autograd
 * (glow/models.py:63,187-190; glow/modules.py:93-95,186).
 */
typedef struct {
  int M, N, K;
  const float* A; long lda; int a_kcontig;
  const float* B; long ldb; int b_kcontig;
  float* C; long ldc;
  const float* bias;          /* per column n, or NULL */
  const float* G; long ldg;   /* act == 2 only */
  int batch; long strideA, strideB, strideC, strideBias, strideG;
  int accumulate;             /* 1: C = act(..) + C ; 2: C = act(.. + C) (pre-activation add) */
  int act; float slope;
  int splitk; float* work;    /* splitk 0 = let the library pick the split (needs work of lfi_gemm_work_floats floats; a NULL
                                 work then means no split) */
  int precision;              /* 0: exact fp32 (f32-input MFMA). 1: bf16x3 — operands split into bf16 hi + lo on the fly,
                                 three bf16 MFMAs per step into fp32 accumulators (~2^-16 relative); needs 16-byte aligned
                                 operands, otherwise the exact kernel runs. Tests may OR in 0x10 (force the 256 x 256 tile
                                 kernel) or 0x20 (force 128 x 128) instead of the library's own choice. Bit 2 (1 | 4 = 5): SIX bf16
                                 products of three-piece operands (x = p0 + p1 + p2, 24 mantissa bits; what is dropped is 2^-24 relative:
                                 fp32-grade results at 6/16 of the f32-input MFMA's cost; 128 x 128 tiles; the sampler's per-frame
                                 products). Bit 3 (1 | 8 = 9): three products of FP16 pieces (11 + 11 mantissa bits, 2^-22 relative: fp32-grade at the
                                 three-product cost) - for operands inside fp16's range only (a value beyond 65504 turns into NaN):
                                 activations and weights, never gradients; 128 x 128 tiles. Bits 8 / 9 (0x100 / 0x200) DROP the
                                 a_lo * b_hi / a_hi * b_lo product of the bf16x3 kernels (a measurement switch: what each GEMM
                                 class loses with one or two bf16 passes, tools/precision_sweep.py -> profiles/precision_sweep.md;
                                 never set by the engine's default configuration) */
  int a_bf16;                 /* 1: A points at bf16 values (same lda / strides, in elements) that stand for an operand already rounded
                                 to bf16 - the encoders' bf16 gradient stash. Needs precision bit 8 (two products: a_lo is never
                                 used), a_kcontig = b_kcontig = 0 and 8-byte aligned rows; runs the 256 x 256 bf16x3 kernel */
  float* colsum_part; long ld_part;  /* optional: the epilogue also leaves column sums of the STORED result over each block of
                                 rows it handles, row r of a (lfi_gemm_colpart_rows(d) x ld_part) matrix, columns as in C (batch
                                 entries side by side: strideC * batch <= ldc). Summing its rows (lfi_colsum_f32) gives the bias
                                 gradient of a Linear without a second pass over C (autograd of nn.Linear.bias,
                                 glow/models.py:187-190). NULL: off. lfi_gemm_colpart_rows returns 0 when the product would not
                                 run on a kernel that can do it (then leave colsum_part NULL) */
} lfi_gemm_desc;

long lfi_gemm_work_floats(const lfi_gemm_desc* d);
long lfi_gemm_colpart_rows(const lfi_gemm_desc* d);
int lfi_gemm_f32(const lfi_gemm_desc* d, void* stream);

/* ---- bf16x3 GEMM on PRE-SPLIT operands. lfi_gemm_f32's bf16x3 kernels split every fp32 operand element into bf16 hi + lo
 * inside every workgroup that touches it; for the big products of the step (cond_transform of all flow steps and its
 * autograd, glow/models.py:187-190; the hoisted W_ih[:, Ch:] c product of the coupling cell and its autograd, :176-179,
 * 206-208) the split is done ONCE instead - by lfi_planes_from_f32 for operands that exist as fp32, by the producing kernel's
 * epilogue (or the backward walk) for operands that are themselves results - into "planes" of the fp32 matrix X (rows x cols):
 * per 32-row tile rt and 16-column tile ct two 1-KB blocks (hi, lo), block ((rt * nct + ct) * 2 + plane) * 512 bf16, 16-byte
 * aligned, rows zero padded to whole 256-row panels and columns to whole tiles (lfi_planes_elems(rows, cols) bf16 elements),
 * which the kernel moves global -> LDS by LDS-DMA (block layout and both reads: lets_face_it_amd/csrc/lfi_pgemm.hip).
 * An operand takes the planes of X in one of two uses:
 *   use 0, row use: the operand is X (mn x k), k = X's columns: an nn.Linear input or weight in its forward product;
 *   use 1, transposed use: the operand is X^T, k = X's ROWS: the same matrices in the autograd products that sum over frames or
 *     over output units. The operand pointer must then address a whole 32-row tile (and a column tile that is a multiple of 2).
 * C[b] (+)= act(A[b] B[b]^T + bias[b]) with A: M x K, B: N x K. a_nkt / b_nkt = column tiles per row tile (nct) of the plane
 * buffers. Same products and accumulation order as lfi_gemm_f32's bf16x3 kernels (results bit-identical). A workgroup reads
 * whole 128- / 256-wide mn panels from a batch entry's first tile: when batch entries start inside one buffer, keep that
 * buffer one panel (256 rows) longer than lfi_planes_elems says (what is read there only feeds rows / columns past M / N,
 * which are never stored). */
long lfi_planes_elems(long rows, int cols);
int lfi_planes_from_f32(const float* X, long ldx, long rows, int cols, void* planes, void* stream);
typedef struct {
  int M, N, K;
  const void* Ap; int a_nkt; long a_stride;   /* planes of A; k-tiles per mn tile in that buffer; bf16 elements between batch
                                                 entries (a batch entry may be a k-tile range of one buffer: stride kt0 * 1024) */
  const void* Bp; int b_nkt; long b_stride;
  float* C; long ldc;
  const float* bias; const float* G; long ldg;   /* as lfi_gemm_desc */
  int batch; long strideC, strideBias, strideG;
  int accumulate, act; float slope;
  int skip;                                      /* bit 0 drops a_lo * b_hi, bit 1 a_hi * b_lo (as lfi_gemm_desc.precision bits 8 / 9) */
  int a_fmt, b_fmt;                              /* use of either operand's planes: 0 row use, 1 transposed use */
  int splitk; float* work;                       /* K split over grid.z with a deterministic reduce, as lfi_gemm_desc (0 / 1: none);
                                                    work: lfi_gemm_planes_work_floats floats */
  int store_f32;                                 /* 1: the result goes to C as fp32 rows; 0: plane outputs only (C may be NULL) */
  /* The result as operand planes of the products that consume it, in either use (splitk <= 1; batch entries side by side in C's
   * columns): planes of the matrix whose rows are C's rows and whose columns are cr_col0 + b * strideC + C's columns (cr_nkt column
   * tiles per row tile in that buffer). Rows >= M and columns >= N are written as zeros. NULL: off. */
  void* Cr; int cr_nkt; long cr_col0;
  /* act == 2 (multiply by leaky_relu'(G)): G may be given as the planes another lfi_gemm_planes call emitted (only the sign of
   * the hi plane is used), same indexing as Cr. NULL: the fp32 G above. */
  const void* Gr; int gr_nkt; long gr_col0;
  float* colsum_part; long ld_part;              /* as lfi_gemm_desc: lfi_gemm_planes_colpart_rows(d) rows of per-pass column sums */
  int out_hi_only;                               /* plane outputs: write the hi planes only - enough for a consumer that takes them
                                                    as its A operand with skip bit 0 (two products, A rounded to bf16), which never
                                                    fetches A's lo planes */
  int tile;                                      /* 0: the library picks 128 x 256 or 256 x 128 tiles by N; 1 / 2 pin them (tests) */
  /* Sign words of the Cr matrix (format below; lfi_planes_sign_words(M, 16 cr_nkt) words, indexed like Cr: cr_col0, strideC).
   * sign_out: the product also writes them, bit = (hi plane value > 0). sign_in: act == 2 takes its mask from them instead of G / Gr
   * (the in-place masked product: Cr is then also where the mask's matrix lay). Only where lfi_gemm_planes_signs_ok says so;
   * lfi_gemm_planes rejects them anywhere else. NULL: off. */
  void* sign_out; const void* sign_in;
} lfi_pgemm_desc;
long lfi_gemm_planes_work_floats(const lfi_pgemm_desc* d);
long lfi_gemm_planes_colpart_rows(const lfi_pgemm_desc* d);
/* ---- sign words of a planes matrix: ONE BIT per element, (the hi plane's bf16 value, as a float, > 0) - all that the act == 2 mask of
 * a later product uses of it. Defined in element coordinates of the rows x cols matrix (rows and cols padded to 64), whoever writes
 * them; element (row, col):
 *   64 x 64 patch (row >> 6, col >> 6), patches row-major, 64 words of 64 bits per patch;
 *   word = lane (row & 15) + 16 * ((col >> 2) & 3) of the patch;
 *   bit  = 16 * ((row >> 4) & 3) + 4 * ((col >> 4) & 3) + (col & 3) of that word.
 * (What one lane of a wave holds of its 64 x 64 patch in the kernels' direct plane epilogue: a wave moves one contiguous 512-byte run
 * per patch.) Bits of elements outside the matrix inside an existing patch are 0. Buffer: lfi_planes_sign_words(rows, cols) 8-byte
 * words, 8-byte aligned.
 * lfi_gemm_planes_signs_ok(d): 1 when the product d describes (sign_out and / or sign_in set to the buffer it would get) takes the sign
 * path - the direct plane epilogue is chosen on 128 x 256 tiles, cr_nkt is a multiple of 4, cr_col0 and (batch > 1) strideC are multiples of 64,
 * splitk <= 1 - and 0 otherwise, or with LFI_PGEMM_SIGNS=0 (read per call). */
long lfi_planes_sign_words(long rows, long cols);
int lfi_gemm_planes_signs_ok(const lfi_pgemm_desc* d);
/* Workgroups of the persistent launch the product d describes gets (the in-place masked product with LFI_PGEMM_PERSIST=1:
 * min(tiles x batch, 2 x CUs), capped by the test hook LFI_PGEMM_PERSIST_WGS), 0 when it is launched one workgroup per tile. Read per call. */
long lfi_gemm_planes_persist_grid(const lfi_pgemm_desc* d);
int lfi_gemm_planes(const lfi_pgemm_desc* d, void* stream);

/* out[c] (+)= scale * sum_r X[r*ldx + c]  for r < rows, c < cols; batched. Deterministic two-stage reduction.
 * (bias gradients: autograd of the nn.Linear / GRU biases.) work: lfi_colsum_work_floats floats. */
long lfi_colsum_work_floats(int rows, int cols, int batch);
int lfi_colsum_f32(const float* X, long ldx, long strideX, int rows, int cols, int batch,
                   float* out, long strideOut, float scale, int accumulate, float* work, void* stream);

/* Column folding. The reference's GRU encoders emit cat(seq[:, -1], h_n[0]) — the same vector twice (glow/models.py:63-64)
 * — so cond_transform multiplies two weight column blocks by identical inputs. The engine stores each block once and
 * folds the weights instead: dst[r][j] = src[r][a[j]] (+ src[r][b[j]] if b[j] >= 0), j < ncols. With b = NULL the same
 * call is a plain column gather, which is how the folded weight gradient is expanded back (both copies get it). */
int lfi_cols_fold(const float* src, long lds, long rows, const int* a, const int* b, int ncols, float* dst, long ldd,
                  void* stream);

/* ---------------------------------------------------------------- window encoders (ModalityEncoder, glow/models.py:55-80)
 * One modality: single-layer GRU from h0 = 0 over a `hist`-frame window ending at frame t (inclusive) for every
 * (sample, timestep) pair; output cat(seq[:, -1], h_n[0]) written into columns [col, col + 2*hid) of the
 * feature matrix `cond` (F x ldcond). Window w = n*B + b covers rows b*T + (start + n - hist + 1 + s), s < hist,
 * of the pre-projected input Xp = X @ W_ih^T (B*T x 3*hid, no bias; made with lfi_gemm_f32).
 * mask: optional (F x hist) dropout multipliers (glow/models.py:56-58); NULL in eval mode.
 * gates ([hist][F][4*hid]: r, z, n, W_hn h + b_hn; NULL to skip) and hseq ([hist][F][hid], required: it is the
 * recurrent state) are step-major stashes for the backward pass. work: lfi_encode_windows_work_floats floats.
 */
typedef struct {
  int B, T, N, start;   /* batch, sequence length, timesteps (T - start), first modelled frame */
  int hist, hid;        /* window length, hidden size */
  int ldcond, col;      /* leading dimension of cond and first output column */
  int precision;        /* lfi_gemm_desc.precision of the per-step recurrent GEMMs */
  int dup;              /* 1: write the state twice, columns [col, col+hid) and [col+hid, col+2*hid) as the reference's
                           cat(seq[:, -1], h_n[0]) does; 0: once (folded feature layout, see lfi_cols_fold) */
  int lstm;             /* 1: "enc: lstm" (nn.LSTM from zero (h, c), gate blocks i, f, g, o; glow/models.py:27-33,65-69): every
                           "3*hid" below reads 4*hid, the gate stash row is 5*hid (i, f, g, o, c) and is required, dgi = dgh */
  int bwd_two_products; /* lfi_encode_windows_bwd, bf16x3 fused GRU path: 1 = two bf16 products per k-step in the d gates x W_hh
                           recurrence (d gates rounded to bf16), as lfi_gemm_desc.precision bit 8 does for a GEMM; 0 = three */
  int stash_f16;        /* 1: `gates` is an fp16 array, [hist][F][hid][4] halves (r, z, n, W_hn h + b_hn of a hidden unit side by
                           side; half the bytes of the fp32 form) - written by lfi_encode_windows_fwd, read by _bwd; only where
                           lfi_encode_windows_stash_f16_ok(d) (the row-layout fused GRU kernels), both calls with the same value.
                           The state stash hseq stays fp32: it is a GEMM operand of dW_hh (glow/models.py:63, nn.GRU's BPTT) */
} lfi_enc_desc;

long lfi_encode_windows_work_floats(const lfi_enc_desc* d);
int lfi_encode_windows_fwd(const lfi_enc_desc* d, const float* Xp, const float* whh /* 3hid x hid */,
                           const float* b_ih, const float* b_hh, const float* mask,
                           float* cond, float* gates, float* hseq, float* work, void* stream);
/* BPTT of the above. dcond (F x lddcond): gradient of the feature matrix; the two output halves are summed.
 * Writes dgi ([hist][F][3*hid], or compact - see lfi_encode_windows_scatter: grads of the pre-activations on the input side,
 * before the dropout mask) and
 * dgh ([hist][F][3*hid]: on the hidden side). Weight gradients follow from those with lfi_gemm_f32/lfi_colsum:
 * dW_hh = dgh[1:]^T hseq[:-1], db_hh = colsum(dgh), db_ih = colsum(dgi), dW_ih = scatter(dgi)^T X. */
int lfi_encode_windows_bwd(const lfi_enc_desc* d, const float* dcond, int lddcond, const float* whh /* 3hid x hid */,
                           const float* gates, const float* hseq, float* dgi, float* dgh,
                           float* bias_part /* [lfi_encode_windows_bias_rows][4][hid] or NULL */, float* work, void* stream);
/* The fused backward (hid <= 256) also leaves per-workgroup partial sums over windows and steps of the four distinct
 * pre-activation gradients (d r, d z, d n, d n * r) in bias_part: db_ih = colsum of blocks {0, 1, 2}, db_hh = colsum of
 * blocks {0, 1, 3} - no second pass over dgi / dgh. Returns the number of partial rows, 0 when the unfused path runs
 * (then bias_part is not written and the biases follow from lfi_colsum_f32 over dgi / dgh). */
long lfi_encode_windows_bias_rows(const lfi_enc_desc* d);
/* Folds bias_part ([rows][4][hid]) into both bias gradients in one launch: db_ih ([3hid]) = column sums of blocks {0, 1, 2},
 * db_hh ([3hid]) = those of blocks {0, 1, 3}; rows are added in a fixed order (bit-reproducible). */
int lfi_encode_windows_bias_grads(const float* bias_part, long rows, int hid, float* db_ih, float* db_hh, void* stream);
/* dXp[b*T + p] = sum over the windows (n, s) that read row p of mask * dgi[(n*B+b)*hist + s]   (B*T x 3*hid)
 * Compact dgi: the input-side and hidden-side gate derivatives of a GRU differ only in the n block (d n vs d n * r), so the
 * fused backward (lfi_encode_windows_compact_dgi(d) == 1: hid <= 256, not lstm) writes dgi as that block alone,
 * [hist][F][hid], and the scatter takes the r and z blocks from dgh (then required; db_ih comes from bias_part). */
int lfi_encode_windows_compact_dgi(const lfi_enc_desc* d);
/* 1 when lfi_encode_windows_bwd (d->bwd_two_products set, fused GRU path, d->ldcond = lddcond) writes dgi / dgh as bf16 arrays of
 * the same shapes: the dW_hh product then takes dgh with lfi_gemm_desc.a_bf16 and lfi_encode_windows_scatter reads bf16. */
int lfi_encode_windows_grad_stash_bf16(const lfi_enc_desc* d);
/* 1 when the shape runs on the row-layout fused GRU kernels in both directions, i.e. lfi_enc_desc.stash_f16 may be set. */
int lfi_encode_windows_stash_f16_ok(const lfi_enc_desc* d);
/* Which forward kernel lfi_encode_windows_fwd takes for this descriptor with 16-byte aligned buffers (tests and the bench's kernel
 * name; shape and environment switches only): 0 = one GEMM + gate kernel per history step, 1 = fused accumulator-layout kernel,
 * 2 = 32-window row-layout kernel, 3 = 64-window kernel (32 x 32 x 16), 4 = 64-window kernel (16 x 16 x 32), 5 = 64-window
 * kernel with the gate epilogue under the matrix phase (transposed product, hid = 256). (glow/models.py:55-80) */
int lfi_encode_windows_fwd_variant(const lfi_enc_desc* d, int masked, int stashed);
int lfi_encode_windows_scatter(const lfi_enc_desc* d, const float* dgi, const float* dgh, const float* mask, float* dXp,
                               void* stream);
/* "enc: none" modality (glow/models.py:76-77), the flattened p1_face history (glow/models.py:601-603) and the input of an
 * "enc: mlp" modality (glow/models.py:70-71):
 * cond[f, col + s*dim + c] = mask[f, s] * X[b, start + n - hist + s + incl, c]   (incl = 0 for prev_p1_face, 1 otherwise;
 * mask (F x hist) = the dropout multipliers of glow/models.py:56-58, or NULL) */
int lfi_gather_windows(const float* X, int B, int T, int dim, int N, int start, int hist, int incl, const float* mask,
                       float* cond, int ldcond, int col, void* stream);
/* Zero-padded copy of a (rows x cols) matrix with row pitch lds into row pitch ldd >= cols (the padding columns are written as
 * zeros): the engine's 4-float granular copies of 50-d face / 27-d speech inputs and of W_ih, so that x W_ih^T (nn.GRU's input
 * projection, glow/models.py:63) and its weight gradient take the vector-load GEMM kernels. */
int lfi_pad_rows(const float* src, long rows, int cols, long lds, float* dst, long ldd, void* stream);
/* Dropout multipliers of ModalityEncoder.forward (glow/models.py:56-58: nn.Dropout(p) on ones(B, hist), one scalar per (sample,
 * history step) and timestep): out[i] = 1 / keep with probability keep, else 0, for up to 4 modalities in one launch. Philox4x32-10
 * keyed on (seed, offset): reproducible from those two numbers; same law as the reference's, another stream (tests inject
 * masks for parity). */
int lfi_dropout_masks(int count, float* const* out, const long* n, const float* keep, unsigned long long seed,
                      unsigned long long offset, void* stream);
/* Conditioning.use_frame_nb (glow/models.py:89,116-117,143-144): one extra feature column holding a frame counter,
 * cond[n*B + b, col] = base[b] + offset + 2n. SeqGlow.forward / invert pass base = batch["frame_nb"] (B floats) and
 * offset = 2 * start (glow/models.py:539-542,557-558,623-625); SeqGlow.inference starts from ones: base = NULL (:572-575). */
int lfi_fill_frame_nb(const float* base, float offset, int B, int N, float* cond, int ldcond, int col, void* stream);
/* d[r, c] *= (y[r, c] > 0 ? 1 : slope): backward of the LeakyReLU of an "enc: mlp" modality, in place on the feature
 * gradient block (its weight / bias gradients then follow from lfi_gemm_f32 / lfi_colsum_f32). */
int lfi_leaky_grad(float* d, long ldd, const float* y, long ldy, int rows, int cols, float slope, void* stream);

/* ---------------------------------------------------------------- flow (FlowStep / FlowNet / Glow, glow/models.py:217-521)
 * Parameters of the Ks = K*L flow steps are struct-of-arrays, step-major: e.g. whh is [Ks][3H][H].
 */
typedef struct {
  int B, N, C, H, D, Ks;     /* batch, timesteps, channels, hidden_channels, cond_dim, flow steps */
  int affine;                /* 1 affine coupling, 0 additive (glow/models.py:330-341) */
  int lstm;                  /* 0 GRUCell, 1 LSTMCell coupling net (glow/models.py:176-185); the LSTM starts from zero
                                (h, c) at the first modelled frame (the reference's own call, models.py:209-213, crashes) */
  float scale_eps;           /* Glow.scale_eps */
  int gemm_precision;        /* lfi_gemm_desc.precision of the GEMMs issued by lfi_flow_param_grads / lfi_flow_sample_seq (bits 0..15).
                                Bit 16 (round 5; the same value in lfi_flow_seq_bwd_planes and lfi_flow_param_grads, planes mode and
                                two-product thin products only - skip bit 0x100 set): the backward stash's dgi | dgh ROWS are bf16
                                arrays of the same shapes instead of fp32 - their only readers round that operand to bf16 anyway
                                (glow/models.py:204-214 backward: the GRUCell's weight gradients) */
} lfi_flow_dims;
/* derived: Ch = C/2, C2 = C - Ch, Cout = affine ? 2*C2 : C2, G = lstm ? 4H : 3H, I = Ch + D */

typedef struct {
  const float *an_bias, *an_logs;          /* [Ks][C]   ActNorm2d (glow/modules.py:10-80) */
  const float *inv_l, *inv_u, *inv_logs;   /* [Ks][C][C], [Ks][C][C], [Ks][C]  InvertibleConv1x1 LU params */
  const float *inv_p, *inv_sign;           /* [Ks][C][C], [Ks][C]  buffers (glow/modules.py:139-145) */
  const float *inv_w;                      /* [Ks][C][C] dense weight (LU_decomposed: false), else NULL */
  const float *w_ih, *w_hh, *b_ih, *b_hh;  /* [Ks][G][I], [Ks][G][H], [Ks][G], [Ks][G]  f.rnn */
  const float *w_fl, *b_fl, *l_fl;         /* [Ks][Cout][H], [Ks][Cout], [Ks][Cout]  f.final_linear (LinearZeros) */
} lfi_flow_params;

/* Derived weights, rebuilt once per optimiser step instead of once per (timestep, flow step) as
 * InvertibleConv1x1.get_weight does (glow/modules.py:147-178). Layout of `prep` (floats), step-major blocks:
 *   W [Ks][C][C], Wt [Ks][C][C], Winv [Ks][C][C] (reverse weight, fp64 inverse cast to fp32),
 *   wz_t [Ks][Ch][G], whh_t [Ks][H][G], wfl_t [Ks][H][Cout], wc [Ks][G][D] (= W_ih[:, Ch:], 16-byte aligned copy),
 *   logdet_const [1] = C * sum(an_logs + inv_logs)
 * followed by private images of the same weights in the layouts the cell kernels load (zero-padded f32 fragments; bf16 hi / lo
 * fragments of the backward recurrent weights; with_inverse: fp16 hi / lo fragments of the reverse cell's weights, which the
 * sampler's cells load instead of splitting f32 fragments in every workgroup of every generated frame). */
long lfi_flow_prep_floats(const lfi_flow_dims* d);
int lfi_flow_prep(const lfi_flow_dims* d, const lfi_flow_params* p, float* prep, int with_inverse, void* stream);

/* Teacher-forced pass over all N timesteps and Ks flow steps (SeqGlow.forward's loop, glow/models.py:546-559,
 * FlowNet.encode :444-451, FlowStep.normal_flow :311-342, f_seq.forward :204-214), walked as anti-diagonals of
 * the (n, k) grid. x0: p1_face (B x T x C, batch-first), first frame `start`. gic: [Ks][F][G] = hoisted
 * W_ih[:, Ch:] c + b_ih. stash: lfi_flow_stash_floats floats (activations for the backward pass; also holds z).
 * nll (F): per-frame NLL in bits (SeqGlow.loss :563-565); z (F x C). */
long lfi_flow_stash_floats(const lfi_flow_dims* d);
int lfi_flow_seq_fwd(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                     const float* x0, int T, int start, const float* gic,
                     float* stash, float* z, float* nll, void* stream);
/* Backward of the above for loss = gscale * sum_f nll[f]. bstash: lfi_flow_bstash_floats floats; afterwards
 * it holds dlin [Ks][F][Cout], dgi [Ks][F][G], dgh [Ks][F][G], dy [Ks][F][C] and the per-tile partial sums that
 * lfi_flow_param_grads turns into parameter gradients. dgi doubles as the gradient of gic. */
long lfi_flow_bstash_floats(const lfi_flow_dims* d);
int lfi_flow_seq_bwd(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                     const float* stash, float gscale, float* bstash, void* stream);

/* The same walk, also leaving dgi - the gradient of the hoisted W_ih[:, Ch:] c + b_ih product, (Ks F x G), flow step k in rows
 * [k F, (k + 1) F) - as operand planes (lfi_planes_elems(Ks F, G) bf16) for the two products that consume it (lfi_gemm_planes):
 * d pre-activation of cond_transform = dgi W_c sums over gate columns (row use), dW_c = dgi^T c sums over frames (transposed
 * use). Written by the walk from its bf16 hi / lo LDS images instead of by a conversion pass over the fp32 dgi (which is still
 * written: the thin dW_ih[:, :Ch] product reads it). lfi_flow_bwd_emits_planes(d) = 1 when the dims allow it (bf16x3 persistent
 * walk, H and B multiples of 32). */
int lfi_flow_bwd_emits_planes(const lfi_flow_dims* d);
/* Which kernels a call with these dims takes under the environment switches as they stand (host only, no device call; the
 * launchers decide through the same function). which 0: lfi_flow_seq_fwd, 1: lfi_flow_seq_bwd / _bwd_planes -> 0 = generic
 * diagonal cells, 1 = register-resident diagonal cells, 2 = persistent walk with exact f32 recurrent products, 3 = persistent walk
 * with bf16x3 recurrent products. which 2: the thin products of lfi_flow_param_grads -> 0 = four split-K products, 1 = one pass
 * over the backward stash (gemm_precision bit 16 set, as that call is given it). Bad dims or `which`: -1.
 * (FlowStep.normal_flow and its autograd, glow/models.py:311-342) */
int lfi_flow_walk_variant(const lfi_flow_dims* d, int which);
int lfi_flow_seq_bwd_planes(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* stash, float gscale, float* bstash, void* dgi_planes,
                            int hi_only /* 1: the hi planes only (lfi_pgemm_desc.out_hi_only) */, void* stream);

typedef struct {
  float *an_bias, *an_logs, *inv_l, *inv_u, *inv_logs, *inv_w;
  float *w_ih, *w_hh, *b_ih, *b_hh, *w_fl, *b_fl, *l_fl;
} lfi_flow_grads;
/* Parameter gradients of the flow from the two stashes. c: (F x ldc) LeakyReLU(cond_transform) outputs, step k in
 * columns [k*D, (k+1)*D), or NULL when the caller computes dW_ih[:, Ch:] = dgi^T c itself (on operand planes). Overwrites (accumulate = 0) or adds to (1) the gradient arrays. work: floats from
 * lfi_flow_param_grads_work_floats. */
long lfi_flow_param_grads_work_floats(const lfi_flow_dims* d);
int lfi_flow_param_grads(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                         const float* stash, const float* bstash, const float* c, long ldc, float gscale,
                         const lfi_flow_grads* g, int accumulate, float* work, void* stream,
                         void* bias_stream /* NULL = stream. Otherwise the bias / ActNorm column sums (streams over the
                                              backward stash, independent of the weight-gradient products) are enqueued
                                              there: the caller orders it after lfi_flow_seq_bwd and joins it */);

/* Pointers into the stashes (host-side address arithmetic only). which: 0 a, 1 y, 2 x_out, 3 h, 4 gates, 5 o, 6 ldc,
 * 7 LSTM cell state (empty for GRU), 8 pipeline state for the forward stash; 0 dlin, 1 dgi, 2 dgh, 3 dy, 4 dx, 5 dh,
 * 6/7 per-tile partial sums, 8 carried d cell state (LSTM), 9 pipeline state for the backward stash.
 * Pipeline state = 32-bit words of the persistent walk (lfi_flow_seq_fwd / _bwd zero it before every launch): word 1 is
 * non-zero afterwards iff a bounded spin timed out and the walk was abandoned - the results are then invalid; callers
 * check it at their next synchronisation point. */
float* lfi_flow_stash_ptr(const lfi_flow_dims* d, float* stash, int which);
float* lfi_flow_bstash_ptr(const lfi_flow_dims* d, float* bstash, int which);

/* ActNorm data-dependent initialisation for flow step k from the first timestep (glow/modules.py:32-43):
 * stats: accumulates per-channel sum and sum of squares of the step's input over the local batch into
 * sums[2*C] (fp64 on device, so ranks can all-reduce them); apply: bias = -mean, logs = log(scale/(sqrt(var)+1e-6)). */
int lfi_actnorm_init_stats(const float* x, int rows, int C, double* sums, void* stream);
int lfi_actnorm_init_apply(const double* sums, double count, int C, float scale, float* bias, float* logs, void* stream);
/* One flow step on a (rows x C) batch with explicit state; used by the init walk, by module-level
 * FlowStep.forward and by the sampler. h_prev/h_out: (rows x H) (NULL h_prev = zeros); c_prev/c_out: the LSTM cell
 * state, same shape (lstm = 1 only; c_out required then, ignored for GRU). reverse = 1 runs
 * FlowStep.reverse_flow (glow/models.py:345-373). gic_k: (rows x G). ldc_acc (rows): log-det accumulator (+=). */
int lfi_flow_step(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, int k, int rows,
                  const float* x_in, long ldx, const float* h_prev, const float* c_prev, const float* gic_k,
                  float* x_out, long ldxo, float* h_out, float* c_out, float* ldc_acc, int reverse, void* stream);
/* SeqGlow.invert (glow/models.py:617-645), the teacher-forced reverse pass of a whole sequence in ONE persistent launch (the
 * reverse twin of lfi_flow_seq_fwd's walk; replaces N * Ks lfi_flow_step(reverse = 1) calls): z (N x B x C latents) ->
 * x_out (N x B x C), logdet (N x B) = the sum over the flow steps of the coupling log-dets, negated as FlowStep.reverse_flow
 * returns them (the constant ActNorm / invconv term is the caller's: lfi_flow_prep's constant). gic: [Ks][N*B][G] as for
 * lfi_flow_seq_fwd. h / cstate: [Ks][B][H] scratch for the recurrent state (zero state at the first timestep, as
 * init_rnn_hidden, glow/models.py:619). Only where lfi_flow_seq_rev_ok(d) (C <= 64, hidden_channels <= 128); prep must hold
 * the inverse weights (lfi_flow_prep with_inverse = 1). */
int lfi_flow_seq_rev_ok(const lfi_flow_dims* d);
long lfi_flow_seq_rev_work_floats(const lfi_flow_dims* d);
int lfi_flow_seq_rev(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* z, const float* gic,
                     float* x_out, float* logdet, float* h, float* cstate, float* work, void* stream);

/* Stand-alone module calls (what code/glow_pytorch/test_modules.py:9-29 exercises outside any flow).
 * lfi_actnorm_forward: ActNorm2d.forward (glow/modules.py:45-80) on a (rows x C) batch: out = (x + bias) exp(logs), or with
 * reverse = 1 x exp(-logs) - bias; dlogdet[0] (nullable) = +-C * sum(logs).
 * lfi_invconv_weights: InvertibleConv1x1.get_weight (glow/modules.py:147-178): W (C x C) from the LU parameters or the dense
 * weight inv_w, optionally the reverse weight Winv (fp64 inverses cast to fp32; required when with_inverse, and written
 * whenever inv_w is given), dlogdet[0] = C * sum(inv_logs) resp. C * log|det inv_w|. z = x W is then one lfi_gemm_f32.
 * work: lfi_invconv_work_floats(C) floats, 8-byte aligned. */
int lfi_actnorm_forward(const float* x, int rows, int C, const float* bias, const float* logs, int reverse, float* out,
                        float* dlogdet, void* stream);
long lfi_invconv_work_floats(int C);
int lfi_invconv_weights(int C, const float* inv_l, const float* inv_u, const float* inv_logs, const float* inv_p,
                        const float* inv_sign, const float* inv_w, int with_inverse, float* W, float* Winv, float* dlogdet,
                        float* work, void* stream);

/* ---------------------------------------------------------------- autoregressive sampling (SeqGlow.inference, glow/models.py:567-596)
 * Whole sequence in one call. faces (B x seq_len x C, batch-first) holds the `start` seed frames and receives the
 * generated ones. Per frame t: c = LeakyReLU(pre_static[n] + faces[:, t-hist1:t] Wct[:, :hist1*C]^T) for all Ks steps
 * (pre_static = everything of cond_transform that does not depend on generated frames, bias included:
 * (nframes*B) x (Ks*D), frame-major; CONSUMED: c of frame n is written over its rows), gic = c W_ih[:, Ch:]^T + b_ih, then the Ks reverse flow steps from the
 * injected prior noise (nframes x B x C, already scaled by eps_std). h: [Ks][B][H] recurrent state, zero on entry.
 * Only "enc: none" for p1_face (all shipped hparams). work: lfi_flow_sample_work_floats floats. */
/* The autoregressive prev_p1_face window may itself go through a ModalityEncoder (the reference's hparam search draws
 * p1_face "enc" from {rnn, mlp, none}, hparam_tuning_configs/large_hparam_search.py:45-62): then its features are
 * recomputed for every generated frame. kind 0: "none" (raw window); 1: "mlp" = LeakyReLU(window W1^T + b1);
 * 2: "rnn" = GRU from h0 = 0 over the window (output folded: the hidden state once); 3: "lstm" = nn.LSTM likewise
 * (glow/models.py:27-33,65-69; four gate blocks in w_ih / w_hh / b_ih / b_hh). `col` = first column of the
 * p1_face block in the (folded) feature layout / in wct; eval mode (no dropout), as SeqGlow.inference runs.
 * Arithmetic of the in-sampler encoder by d->gemm_precision, which the drivers hand on unchanged: the mlp's product, the recurrent
 * kinds' input projection and e wct[:, col : col + hid]^T are lfi_gemm_f32 products at that precision; it is also the
 * lfi_enc_desc.precision of the recurrence, where 1 -> bf16x3 recurrence; any other value -> exact f32 recurrence; loops take the GEMM
 * mode as given (the fused GRU kernels, hid <= 256, know only "== 1"; the unfused GRU loop, hid > 256, and the LSTM loop pass the
 * value to their per-step lfi_gemm_f32, where 5 and 9 mean what they mean there). The features lie in p1work with row pitch
 * (hid + 3) & ~3; the padding columns are never read. */
typedef struct {
  int kind, hid;
  const float *w1, *b1;                        /* mlp: [hid][hist1*C], [hid] */
  const float *w_ih, *w_hh, *b_ih, *b_hh;      /* rnn: [3hid][C], [3hid][hid], [3hid], [3hid]; lstm: 4hid */
  int col;
} lfi_p1enc;

long lfi_flow_sample_work_floats(const lfi_flow_dims* d);
long lfi_flow_sample_p1_work_floats(const lfi_flow_dims* d, const lfi_p1enc* e, int hist1);
int lfi_flow_sample_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                        const float* wct /* [Ks*D][E] */, long E, int hist1,
                        float* pre_static, const float* noise,
                        float* faces, int seq_len, int start, int nframes,
                        float* h, float* cstate /* [Ks][B][H] LSTM cell state, zero on entry; NULL for GRU */,
                        const lfi_p1enc* p1 /* NULL = "none" */, float* p1work /* lfi_flow_sample_p1_work_floats */,
                        float* work, void* stream);
/* The same for a run of frames that continues a sequence: first_frame = number of frames earlier calls generated (the state in
 * h / cstate carries on when > 0); pre_static, noise and start are this run's own. Lets the caller compute the static part of
 * the next run on another stream while this run's chain of dependent cells executes. */
/* Range guard of the sampler's fp16-piece arithmetic: out_bits[0] = bit pattern of max |v| over `count` (<= 8) fp32 arrays, one
 * launch (finite |v| order like their bit patterns; an inf reads back as inf, a NaN as NaN). Replaces one blocking
 * `tensor.abs().max()` per input of SeqGlow.inference (glow/models.py:567-596 has no such guard: its arithmetic is plain fp32). */
int lfi_absmax_f32(int count, const float* const* ptrs, const long* n, unsigned* out_bits, void* stream);
/* A HIP stream that owns `cus_per_xcd` CUs of every XCD (1 .. 32 on MI355X) and leaves the rest of the chip to the streams beside
 * it: the sampler's static part (window encoders, static cond_transform columns of the NEXT run of frames) runs on one while the
 * per-frame chain keeps the other CUs - on an ordinary second stream the two only take turns. Not a reference
 * interface: SeqGlow.inference (glow/models.py:567-596) is one PyTorch stream. Destroy with lfi_stream_destroy. The CU-mask bit
 * layout is known (probed) for the 256-CU / 8-XCD part only: any other device gets LFI_ERR_ARG and the caller stays on an ordinary
 * second stream. */
int lfi_stream_create_partial(int cus_per_xcd, void** stream);
int lfi_stream_destroy(void* stream);
int lfi_flow_sample_seq_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                             const float* wct, long E, int hist1, float* pre_static, const float* noise,
                             float* faces, int seq_len, int start, int nframes, int first_frame,
                             float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work, void* stream);
/* lfi_flow_sample_seq_from that also leaves nll (nframes x B, frame-major): the per-frame NLL in bits of every frame it generates,
 * -(logdet_fwd(x) + sum_c -0.5 (z_c^2 + log 2 pi)) / ln 2 at the z it was given in `noise` - the value lfi_flow_seq_fwd's nll holds
 * for that frame when the generated sequence is fed back teacher-forced (SeqGlow.loss, glow/models.py:563-565). The model's own
 * density (temperature 1) of the frame, not a density of the tempered sampling distribution. The reverse cells already form every
 * coupling log-det: on the one-launch-per-frame chain the rows' running sum crosses the chain beside the tile, with no launch and no
 * pass added. nll_work: lfi_flow_sample_nll_work_floats(d) floats (the hand-over words). nll == NULL: lfi_flow_sample_seq_from. */
long lfi_flow_sample_nll_work_floats(const lfi_flow_dims* d);
int lfi_flow_sample_seq_nll(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static, const float* noise,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* nll, float* nll_work, void* stream);
/* Teacher-forced frames of a sequence whose recurrent state is carried (SampleStream.observe; SeqGlow.forward, glow/models.py:524-561,
 * one frame at a time): lfi_flow_sample_seq_nll's arguments without `noise`. Per frame n the sampler's conditioning front end (the
 * window part of cond_transform + gic, every lfi_p1enc kind), then ALL Ks forward flow steps of the OBSERVED frame faces[:, start + n]
 * in one launch: h / cstate are read and updated in place exactly as the sampler's reverse cells update them (the recurrent cell sees
 * the pass-through half and the conditioning, the same in both directions), so observed and generated frames alternate freely.
 * nll (nframes x B): the frame's NLL in bits, -(logdet_fwd + sum_c -0.5 (z_c^2 + log 2 pi)) / ln 2; z (nframes x B x C, NULL = not
 * wanted): its latent. Arithmetic of the cells by d->gemm_precision: 9 = three fp16 products of two-piece operands (range: the
 * caller's guard), 5 and 0 = the exact f32 MFMA (no range caveat: the observed frame is caller data; 5 is the range guard's fallback). Shapes outside the register-resident
 * cells (and LFI_SAMPLE_CHAIN=0): Ks launches of the streaming forward cell + a finish. score_work: lfi_flow_score_work_floats(d)
 * floats; work / p1work: the sampler's. Allocation-free, capturable; every argument is checked before the first launch. */
long lfi_flow_score_work_floats(const lfi_flow_dims* d);
int lfi_flow_score_seq_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* score_work, float* z, float* nll, void* stream);
/* lfi_flow_score_seq_from for a CHUNK of frames known up front (SampleStream.observe_many): the same arguments with a chunk work area
 * where that has score_work, and the same contract - it leaves in h / cstate, z and nll what lfi_flow_score_seq_from leaves for
 * them. The front end runs ONCE for all nframes (the prev_p1_face windows gathered, the encoded kinds over nframes * B windows,
 * c = LeakyReLU(pre_static + window part) in place, gic as [Ks][nframes * B][G]) at d->gemm_precision, and the chain is ONE launch of
 * Ks ceil(B / 16) workgroups: workgroup (k, tile) loops over the frames with its recurrent state on chip, waits for frame n of
 * (k - 1, tile) and hands its own on through a slot per (step boundary, frame) - nframes + Ks - 1 cell times end to end where one
 * launch per frame takes nframes * Ks. A workgroup waits only on a lower ticket and no slot is reused inside a launch, so any number
 * of resident workgroups makes progress; spins are bounded, and an abandoned launch leaves NaN in every nll / z it did not finish.
 * The cells' arithmetic by d->gemm_precision as lfi_flow_score_seq_from's. chunk_work: lfi_flow_score_chunk_work_floats(d, p1, hist1)
 * floats, d->N = the frames per call (the caller bounds it by splitting a long chunk: state carries through h / cstate and
 * first_frame); p1work / work are not used. lfi_flow_score_chunk_ok: 1 where this chain runs (C, Cout <= 64, H <= 128,
 * LFI_SAMPLE_CHAIN not 0, LFI_FLOW_GENERIC not 1); elsewhere call lfi_flow_score_seq_from. hist1 >= 1 is required (a window of no
 * frames has no front end to batch: lfi_flow_score_seq_from takes that case too). LFI_CHUNK_ONLY=front / chain, for
 * tools/stream_latency.py alone: only that part of the call is launched, to be timed; the results are not meaningful.
 * Allocation-free; every argument is checked before the first launch. */
long lfi_flow_score_chunk_work_floats(const lfi_flow_dims* d, const lfi_p1enc* p1, int hist1);
int lfi_flow_score_chunk_ok(const lfi_flow_dims* d);
/* Host-only query (no GPU touched; d == NULL: 0): what the per-frame drivers above and below - lfi_flow_sample_seq{,_from,_nll},
 * lfi_flow_sample_cand_from / _cand_seq, lfi_flow_score_seq_from / _chunk / _chunk_rows, lfi_flow_step_rows_from / _seq - decide from d
 * and the switches read at the call, as bits: 1 = the register-resident cells (C, Cout <= 64, H <= 128; LFI_FLOW_GENERIC not 1),
 * 2 = one launch per frame's chain (bit 1 and LFI_SAMPLE_CHAIN not 0; lfi_flow_score_chunk_ok is this bit), 4 = reverse cells with
 * three fp16 products (gemm_precision bit 0, GRU, whole 32-k blocks, LFI_PIPE_X3 not 0), 8 = their weights read as the fp16 fragment
 * images of lfi_flow_prep (bits 2 and 4, LFI_SAMPLE_WFRAG16 not 0), 16 = forward cells with three fp16 products (bit 4 and
 * (gemm_precision & 0xff) == 9 only: the observed frame is caller data, see lfi_flow_score_seq_from). Bits 4 .. 16 are used where
 * bit 2 is set. */
int lfi_flow_frame_plan(const lfi_flow_dims* d);
int lfi_flow_score_seq_chunk(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                             const float* wct, long E, int hist1, float* pre_static,
                             float* faces, int seq_len, int start, int nframes, int first_frame,
                             float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                             float* chunk_work, float* z, float* nll, void* stream);
/* lfi_flow_score_seq_chunk for a RAGGED chunk (SampleStream.observe_many with lengths): lengths, B ints on the device - batch row b
 * takes the first lengths[b] of the nframes frames (values outside 0 .. nframes are clamped by the kernel). h / cstate of row b are
 * what lfi_flow_score_seq_chunk leaves after lengths[b] frames (a row of length 0 is not written at all), z and nll are written for
 * frames n < lengths[b] only - the caller zeroes them first - and with the dense call's arithmetic, instruction for instruction. The
 * front end stays dense over nframes * B windows (behind a row's length `faces` and pre_static must hold finite values; their results
 * reach nothing stored); in the chain a 16-row tile loops to its longest row, and a tile of length 0 leaves at once. The work area,
 * lfi_flow_score_chunk_ok, LFI_CHUNK_ONLY and every other rule are lfi_flow_score_seq_chunk's. */
int lfi_flow_score_seq_chunk_rows(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                             const float* wct, long E, int hist1, float* pre_static,
                             float* faces, int seq_len, int start, int nframes, int first_frame,
                             float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                             float* chunk_work, float* z, float* nll, const int* lengths, void* stream);
/* ONE frame of a session in which every batch row either observes or generates (SampleStream.step_rows): lfi_flow_sample_seq_nll's
 * arguments (nframes must be 1; nll, B floats, and nll_work are required), then observed (B ints on the device: != 0 = the row's
 * frame is GIVEN - it is in faces[:, start] already - and 0 = the row generates from its noise row) and a second work area, rows_work
 * (lfi_flow_step_rows_work_floats(d) floats). Every row's h / cstate, frame in `faces` and nll are what lfi_flow_score_seq_from
 * (observing rows) or lfi_flow_sample_seq_nll (generating rows) alone leaves for it; noise rows of observing rows and frame slots of
 * generating rows are read but never reach anything stored. The conditioning front end once, then both chains in one launch of
 * 2 Ks ceil(B / 16) workgroups with row-masked stores; a 16-row tile whose rows all have one role costs one chain, not two. Each
 * direction keeps its own arithmetic rule by d->gemm_precision. Shapes outside the register-resident cells (and LFI_SAMPLE_CHAIN=0):
 * the two directions' per-step launches and a merge launch. Allocation-free, capturable; every argument is checked before the
 * first launch. */
long lfi_flow_step_rows_work_floats(const lfi_flow_dims* d);
int lfi_flow_step_rows_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static, const float* noise,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* nll, float* nll_work, const int* observed, float* rows_work, void* stream);
/* N CANDIDATES of ONE frame per batch row (SampleStream.step_candidates, best-of-N): lfi_flow_sample_seq_nll's arguments (nframes must
 * be 1; nll and nll_work are not used and may be NULL), then ncand >= 1, the candidates' outputs and a work area, cand_work
 * (lfi_flow_sample_cand_work_floats(d, ncand) floats). noise is B x ncand x C (already * eps): virtual row v = b * ncand + j is
 * candidate j of batch row b. The conditioning front end runs once for the B rows; the reverse chain runs over V = B * ncand virtual
 * rows that read gic and the incoming h / cstate of their PARENT row in place - one launch of Ks ceil(V / 16) workgroups, nothing of
 * the session copied V-fold. faces, h and cstate are READ ONLY here: candidate v's frame goes to cand_frames (V x C), its NLL in bits
 * to cand_nll (V), its new state to cand_h / cand_c ([Ks][V][H]; cand_c NULL for GRU), each what lfi_flow_sample_seq_nll leaves for
 * a row with that state, conditioning and prior draw - bit for bit on the one-launch chain. lfi_stream_commit_cand installs the
 * chosen candidates. Shapes outside the register-resident cells, LFI_SAMPLE_CHAIN=0, LFI_FLOW_GENERIC=1: a gather launch broadcasts
 * gic / h / c to V rows, then the per-step launches and the NLL finish over V rows. Allocation-free, capturable; every argument is
 * checked before the first launch. */
long lfi_flow_sample_cand_work_floats(const lfi_flow_dims* d, int ncand);
int lfi_flow_sample_cand_from(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static, const float* noise,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* nll, float* nll_work, int ncand, float* cand_frames, float* cand_nll, float* cand_h,
                            float* cand_c, float* cand_work, void* stream);
/* N candidate ROLLOUTS of nframes >= 1 frames per batch row (SampleStream.rollout_candidates): lfi_flow_sample_seq_nll's arguments with
 * d->B = V = B * ncand VIRTUAL rows, then ncand >= 1 (it must divide d->B; V <= 2^22). Virtual row v = b * ncand + j is candidate j
 * of batch row b. From the second frame on the candidates of a row differ in their faces windows and their h / c, so faces
 * (V x seq_len x C), noise (nframes x V x C), nll (nframes x V), h / cstate ([Ks][V][H]), p1work and nll_work are the candidates'
 * own, sized for V rows and updated in place exactly as lfi_flow_sample_seq_nll updates them for V rows. What they share is the static
 * conditioning: pre_static has the PARENTS' rows only, nframes * (V / ncand) of them, frame-major, and virtual row v of frame i reads
 * row i * (V / ncand) + v / ncand. Where the fused front end runs (lfi_flow_sample_seq_nll's rule) it reads the parent's row in place -
 * a compile-time parent mode of the same kernel, the row index of its one pre_static load divided by ncand - and pre_static is not
 * written: a parent's Ks * D floats come out of L2 ncand times and are never copied V-fold. Every other front end overwrites the rows
 * it reads, so there a small launch per frame first copies the frame's parent rows to V rows of a ONE-frame scratch inside `work`,
 * which the front end then consumes in place (pre_static itself stays as it was). work: lfi_flow_sample_cand_seq_work_floats(d, ncand)
 * floats, 16-byte aligned, where d is the PARENTS' dims (d->B = V / ncand): lfi_flow_sample_work_floats for V rows and that scratch;
 * 0 for a NULL d, ncand < 1 or V beyond the limit. The reverse chain, the step-0 window-fragment hand-over and the NLL hand-over are
 * lfi_flow_sample_seq_nll's for V rows, kernel for kernel: rows never mix in the fused kernel or in a cell, so on that path candidate
 * (b, j) is bit for bit the row a B-row call generates from the same state, conditioning and draws; ncand = 1 runs the same launches
 * on the same shapes on every path (the copy aside). LFI_CHUNK_ONLY=front, for tools/stream_latency.py alone: every frame's front
 * end and no chain is launched, to be timed; the results are not meaningful. Allocation-free; every argument is checked before the
 * first launch. */
long lfi_flow_sample_cand_seq_work_floats(const lfi_flow_dims* d, int ncand);
int lfi_flow_sample_cand_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static, const float* noise,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* nll, float* nll_work, int ncand, void* stream);
/* A run of nframes >= 1 frames of a chunk in which every batch row takes its role FRAME BY FRAME (SampleStream.step_rows_many): it
 * replaces a host loop of nframes lfi_flow_step_rows_from calls - the same launches, from one call with one argument check, one kernel
 * pick and one preparation of the fused conditioning kernel's weight fragments. lfi_flow_step_rows_from's arguments, frame-major:
 * pre_static has nframes * B rows, noise is nframes x B x C, nll nframes x B, observed nframes x B ints (!= 0 = row b's frame n is
 * GIVEN, in faces[:, start + n] already). Per frame n: the conditioning front end at t = start + n on that frame's rows of pre_static,
 * the chain-state clear, one flow_rows_chain_kernel launch with that frame's role, noise and nll rows, has_prev = first_frame + n > 0
 * and frame_no = first_frame + n; LFI_SAMPLE_CHAIN=0 and the generic cell: the per-step launches and the merge launch, per frame.
 * The work areas are ONE frame's (lfi_flow_step_rows_work_floats, lfi_flow_sample_nll_work_floats, lfi_flow_sample_work_floats),
 * reused from frame to frame; the stream orders them. The window-fragment hand-over of the reverse chain is not used (a frame may
 * have been observed). lfi_flow_step_rows_from is the nframes = 1 call of the same body. Allocation-free; every argument is checked
 * before the first launch. */
int lfi_flow_step_rows_seq(const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep,
                            const float* wct, long E, int hist1, float* pre_static, const float* noise,
                            float* faces, int seq_len, int start, int nframes, int first_frame,
                            float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work,
                            float* nll, float* nll_work, const int* observed, float* rows_work, void* stream);
/* One frame forward of a streaming sampling session (SeqGlow.open_stream; glow/models.py:567-596 one frame at a time), in ONE launch:
 * every window i (B x hist[i] x dim[i], rows per batch entry) moves up by one frame in place, and its last row receives src[i] (B x
 * dim[i]), or - src[i] == NULL, the prev_p1_face window of the session's own output - keeps the frame the last step generated there;
 * noise (B x C, already * eps) is copied into noise_dst; frame_nb (B floats, NULL = no counter) += 2; max |v| of every value read
 * is folded into *guard_bits (atomic max of the bit pattern, as lfi_absmax_f32; never cleared here, NULL = no guard). count <= 8.
 * Allocation-free, capturable; the host never waits on guard_bits. */
int lfi_stream_advance(int B, int count, float* const* win, const float* const* src, const int* hist, const int* dim,
                       const float* noise, float* noise_dst, int C, float* frame_nb, unsigned* guard_bits, void* stream);
/* lfi_stream_advance for a step in which every batch row either observes or generates (SampleStream.step_rows). observed: B bytes on
 * the device (a bool mask), != 0 = the row observes; role (B ints, the session's own) receives 0 / 1 per row - what
 * lfi_flow_step_rows_from reads. Window face_win (0 <= face_win < count, src[face_win] required: the observed frames, B x
 * dim[face_win]) receives its source only in observing rows; generating rows shift only, and the chain writes their newest row.
 * Into *guard_bits go only values that are used: the windows' (the face only of observing rows) and the noise of generating rows;
 * the face of a generating row is never read. Everything else as lfi_stream_advance. */
int lfi_stream_advance_rows(int B, int count, float* const* win, const float* const* src, const int* hist, const int* dim,
                            int face_win, const float* noise, float* noise_dst, int C, float* frame_nb,
                            const unsigned char* observed, int* role, unsigned* guard_bits, void* stream);
/* A chunk of n >= 1 observed frames of a streaming session per call (SampleStream.observe_many), two launches around the chunk's static
 * part and chain. The window tables are lfi_stream_reset_rows' (count <= 8, the prev_p1_face window last with lead[i] = 1: its hist[i]
 * counts the leading row). seq[i]: the session's sequence buffer of window i, B x (start + n) x dim[i], the shape the sequence mode
 * of the feature builder and lfi_flow_score_seq_chunk take; hist[i] - lead[i] <= start.
 * in: the window's live frames go to frames start - (hist[i] - lead[i]) .. start - 1 of seq[i], src[i] (B x n x dim[i], the
 * caller's frames t .. t + n - 1; the observed faces for the prev_p1_face window) to frames start .. start + n - 1. Frames in front
 * of a window are neither read nor written (zero them once). max |v| of every NEW value is folded into *guard_bits as
 * lfi_stream_advance does (NULL = no guard).
 * out: every window takes the last hist[i] frames of seq[i] - right for n below, at and above hist[i] (the prev_p1_face window's
 * leading row so holds what n one-frame advances leave in it); frame_nb (B floats, NULL = no counter) += 2 n.
 * Allocation-free; every argument is checked before the launch. */
int lfi_stream_chunk_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                        const int* hist, const int* dim, const int* lead, unsigned* guard_bits, void* stream);
int lfi_stream_chunk_out(int B, int n, int start, int count, float* const* win, float* const* seq, const int* hist,
                         const int* dim, const int* lead, float* frame_nb, void* stream);
/* The two window launches around a RAGGED chunk (SampleStream.observe_many with lengths; lfi_flow_score_seq_chunk_rows): the dense
 * ones' arguments and lengths, B ints on the device (values outside 0 .. n are clamped), required.
 * in_rows: the window's live frames as lfi_stream_chunk_in, then the first lengths[b] frames of row b's source, then zeros up to
 * frame start + n - 1. What a source holds behind a row's length is not read: it reaches neither seq[i] nor *guard_bits.
 * out_rows: row b takes the hist[i] frames of seq[i] that end at frame start + lengths[b], and frame_nb[b] += 2 lengths[b]; a row
 * of length 0 is skipped entirely (its windows and counter are not written).
 * Allocation-free; every argument is checked before the launch. */
int lfi_stream_chunk_in_rows(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                        const int* hist, const int* dim, const int* lead, unsigned* guard_bits, const int* lengths, void* stream);
int lfi_stream_chunk_out_rows(int B, int n, int start, int count, float* const* win, float* const* seq, const int* hist,
                         const int* dim, const int* lead, float* frame_nb, const int* lengths, void* stream);
/* The two window launches for a chunk of n >= 1 GENERATED frames per call (SampleStream.step_many), around the chunk's static part
 * and lfi_flow_sample_seq_nll with nframes = n on seq[gen_win]: lfi_stream_chunk_in / lfi_stream_chunk_out with the same tables,
 * for a session whose prev_p1_face window gen_win (0 <= gen_win < count, dim[gen_win] == C) has no source - the chain writes its
 * frames start .. start + n - 1.
 * gen_in: every window but gen_win as lfi_stream_chunk_in. Of gen_win only the live frames go into seq[gen_win]; src[gen_win] is not
 * read and may be NULL (the table itself may not); its frames start .. start + n - 1 are left alone. noise (n x B x C, frame-major,
 * already * eps: lfi_flow_sample_seq_nll's) is read once and folded into *guard_bits beside the new conditioning values; it is not
 * copied - the chain reads the caller's tensor in place.
 * gen_out: lfi_stream_chunk_out, and the n generated frames of every batch row b go from seq[gen_win] to out + b * ld_out (n x C
 * each; ld_out >= n * C floats, so a (B, N, C) result takes a run of its frames in place) and are folded into *guard_bits: a
 * generated value beyond the fp16 pieces' range reaches the guard as it does through the lfi_stream_advance after a one-frame step.
 * guard_bits NULL = no guard. One launch each, allocation-free; every argument is checked before the launch. */
int lfi_stream_chunk_gen_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                            const int* hist, const int* dim, const int* lead, int gen_win,
                            const float* noise /* n x B x C, frame-major, already * eps */, int C,
                            unsigned* guard_bits, void* stream);
int lfi_stream_chunk_gen_out(int B, int n, int start, int count, float* const* win, float* const* seq,
                             const int* hist, const int* dim, const int* lead, int gen_win,
                             float* out /* B x n x C, row pitch ld_out floats */, long ld_out,
                             float* frame_nb, unsigned* guard_bits, void* stream);
/* The window launch INTO a chunk of n >= 1 frames whose rows observe or generate frame by frame (SampleStream.step_rows_many): it
 * replaces n lfi_stream_advance_rows launches. lfi_stream_chunk_gen_in's arguments and roles (n x B ints on the device, frame-major,
 * != 0 = the row observes that frame), required; unlike gen_in, src[gen_win] (the given faces, B x n x C) is required too. Every
 * conditioning window is laid out as in gen_in. Of gen_win the live frames go into seq[gen_win]; then, frame by frame: where
 * roles[f * B + b] != 0 the given frame goes to frame start + f of the sequence and is folded into *guard_bits; elsewhere the slot is
 * left alone - lfi_flow_step_rows_seq writes it - the given frame is not read, and the row's noise of that frame is folded instead.
 * Only values that are used reach the guard word. The way out is lfi_stream_chunk_gen_out as it is (all n frames of the faces
 * sequence go to `out` and are folded; a given frame folded twice changes nothing in a maximum). One launch, allocation-free; every
 * argument is checked before the launch. */
int lfi_stream_chunk_roles_in(int B, int n, int start, int count, float* const* win, const float* const* src, float* const* seq,
                            const int* hist, const int* dim, const int* lead, int gen_win,
                            const float* noise /* n x B x C, frame-major, already * eps */, int C,
                            const int* roles, unsigned* guard_bits, void* stream);
/* Reseed listed batch rows of a streaming sampling session (SampleStream.reset_rows; the start of glow/models.py:567-596 for those
 * rows alone) between steps: each session row rows[j] (0 <= rows[j] < B, none twice, nrows >= 1) gets the state open_stream gives
 * a row, from entry j of the caller's seed, and no other row is written. Per window i (count <= 8; the layout of lfi_stream_advance):
 * the row's hist[i] frames are copied from seed[i] + j * seed_ld[i] (the caller's (n, T, dim) tensor read in place: seed[i] points at
 * frame start - hist of entry 0, seed_ld[i] = T * dim), or - lead_zero[i] = 1, the prev_p1_face window - frame 0 of the row is zeroed
 * and frames 1 .. hist[i] - 1 come from the seed. h / cstate ([Ks][B][H] each; cstate NULL = GRU): the row is zeroed in every flow
 * step, which is what the reverse cells load for a null h_prev (first_frame = 0). frame_nb (NULL = no counter): the row is set to
 * -1 (the next advance's + 2 gives inference's 1). max |v| of every seed value copied is folded into *guard_bits as lfi_stream_advance
 * does; the guard is never cleared here (other rows' values live in it). Rows travel in the kernel arguments, 256 per launch (a
 * longer list is several launches): allocation-free, no host staging and no host wait, capturable. Every argument, every row
 * included, is checked before the first launch. */
int lfi_stream_reset_rows(int B, int nrows, const int* rows, int count, float* const* win, const float* const* seed,
                          const long* seed_ld, const int* hist, const int* dim, const int* lead_zero, float* h, float* cstate,
                          int Ks, int H, float* frame_nb, unsigned* guard_bits, void* stream);
/* Live rows out of and into a streaming sampling session (SampleStream.save_rows / load_rows), between steps. The reference keeps
 * this state as plain attributes (the coupling cells' f_seq.hidden, glow/models.py:193-194, and inference()'s local windows); here it
 * lives in session-owned buffers, and these two copy listed rows of it to and from plain fp32 records. A row's record, in order:
 * every window i (count <= 8, the layout of lfi_stream_advance with the prev_p1_face window last; hist[i] x dim[i] floats each), h
 * (Ks x H), c (Ks x H; only with cstate, LSTM), the frame counter (one float; only with frame_nb). lfi_stream_row_floats returns
 * the record's length R (host arithmetic only; -1 on a bad argument) and is the single definition of that layout: both kernels take
 * their offsets from the same table. A record does not depend on B or on the session's per-frame arithmetic.
 * save: record j of `out` (row stride ld_out >= R floats, nrows records) receives the state of session row rows[j]; nothing of the
 * session is written. zero_state != 0 writes zeros for h / c: a session that has not stepped since its open / reset ignores what
 * those buffers hold (first_frame = 0), and zeros are what that means.
 * load: session row rows[j] receives record entries[j] of `in` (nentries records, row stride ld_in >= R); an entry may be listed
 * more than once (a branch), a row may not. Only the listed rows are written. max |v| of the windows and of c is folded into
 * *guard_bits as lfi_stream_reset_rows does (never cleared; |h| < 1, and the counter is a frame number, not a model input).
 * Both: rows (and entries) travel in the kernel arguments, 256 per launch - allocation-free, no host staging, no host wait,
 * capturable; every argument, every row and entry included, is checked before the first launch. */
long lfi_stream_row_floats(int count, const int* hist, const int* dim, int Ks, int H, int lstm, int has_frame_nb);
int lfi_stream_save_rows(int B, int nrows, const int* rows, int count, const float* const* win, const int* hist, const int* dim,
                         const float* h, const float* cstate, int Ks, int H, const float* frame_nb, int zero_state, float* out,
                         long ld_out, void* stream);
int lfi_stream_load_rows(int B, int nrows, const int* rows, const int* entries, int nentries, int count, float* const* win,
                         const int* hist, const int* dim, float* h, float* cstate, int Ks, int H, float* frame_nb, const float* in,
                         long ld_in, unsigned* guard_bits, void* stream);
/* One of every row's candidates becomes the row's frame (SampleStream.commit), in ONE launch: for session row r, j = choice[r]
 * (B ints on the device, clamped into 0 .. ncand - 1 by the kernel) or - choice == NULL - the arg-min of cand_nll[r, :] (ties to the
 * lowest index; NaN counts as larger than any number; all NaN: 0). cand_frames[r, j] (lfi_flow_sample_cand_from's outputs) goes into
 * the newest slot of the row's faces window (face_win, B x hist x C) and to out_frame (B x C); cand_h[k][r * ncand + j] to h[k][r]
 * for every flow step k, and cand_c to cstate likewise when cstate is non-NULL; cand_nll[r, j] to out_nll[r], j to out_choice[r].
 * The frame is folded into *guard_bits as a window value (NULL = no guard). Allocation-free, no host wait, capturable. */
int lfi_stream_commit_cand(int B, int ncand, int C, int Ks, int H, const int* choice, const float* cand_frames,
                           const float* cand_nll, const float* cand_h, const float* cand_c, float* face_win, int hist,
                           float* h, float* cstate, float* out_frame, float* out_nll, int* out_choice,
                           unsigned* guard_bits, void* stream);
/* The two launches around lfi_flow_sample_cand_seq (SampleStream.rollout_candidates / commit), V = B * ncand virtual rows, row
 * v = b * ncand + j. Neither writes a conditioning window; the session's own state is written by the commit alone.
 * cand_seq_in, after lfi_stream_chunk_gen_in has laid the windows out as sequences: the first `start` frames of batch row b's faces
 * sequence (parent_seq, B x (start + n) x C) go to every candidate's own sequence (cand_seq, V x (start + n) x C), whose frames
 * start .. start + n - 1 are the chain's to write; with first_frame > 0 the row's h / cstate ([Ks][B][H]) go to the candidates'
 * ([Ks][V][H]; first_frame = 0: the chain ignores what they hold); the candidates' noise (n x V x C, frame-major, already * eps) is
 * read once and folded into *guard_bits (NULL = no guard) - it is not copied. ncand = 1: a copy.
 * commit_cand_seq: for session row r, j = choice[r] (B ints on the device, clamped into 0 .. ncand - 1 by the kernel) or - choice ==
 * NULL - the candidate of least summed NLL: sum over f = 0 .. n - 1 in that order, in fp32, of cand_nll[f, r, j] (n x V); ties to the
 * lowest index; a NaN sum counts as larger than any number; all NaN: 0. Of candidate (r, j): frames start .. start + n - 1 of its
 * sequence go to out (B x n x C) and are folded into *guard_bits; the last hist frames of its sequence (1 <= hist <= start + n; they
 * end at frame start + n, so a short rollout keeps old frames) become the row's faces window (face_win, B x hist x C); cand_h / cand_c
 * of every flow step become h / cstate of the row (cstate NULL = GRU); its NLL words go to out_nll (n x B), j to out_choice[r], and
 * frame_nb[r] += 2 n (NULL = no counter). The conditioning windows come back with lfi_stream_chunk_out over those windows alone.
 * One launch each, allocation-free, no host wait; every argument is checked before the launch. */
int lfi_stream_cand_seq_in(int B, int ncand, int n, int start, int C, int Ks, int H, const float* parent_seq, float* cand_seq,
                           const float* h, const float* cstate, float* cand_h, float* cand_c, int first_frame,
                           const float* noise, unsigned* guard_bits, void* stream);
int lfi_stream_commit_cand_seq(int B, int ncand, int n, int start, int C, int Ks, int H, const int* choice,
                               const float* cand_seq, const float* cand_nll, const float* cand_h, const float* cand_c,
                               float* face_win, int hist, float* h, float* cstate, float* frame_nb, float* out, float* out_nll,
                               int* out_choice, unsigned* guard_bits, void* stream);

/* ---------------------------------------------------------------- optimiser (configure_optimizers, glow/lets_face_it_glow.py:61-72)
 * Flat-buffer Adam with global-norm gradient clipping (Trainer gradient_clip_val, hparams/final_model.yaml:126):
 * norm: sumsq[0] = sum g^2 (fp64, deterministic). step: coef = min(1, clip/(sqrt(sumsq)+1e-6)) (clip <= 0: 1),
 * g *= coef * gmul; Adam (weight decay / amsgrad: lfi_adam_clip_step_ex below). step_count is 1-based. */
int lfi_grad_sumsq(const float* g, long n, double* sumsq, double* work /* 1024 doubles */, void* stream);
int lfi_adam_clip_step(float* p, const float* g, float* m, float* v, long n, const double* sumsq,
                       float clip, float gmul, float lr, float beta1, float beta2, float eps, int step_count,
                       void* stream);

/* torch.optim.Adam's remaining constructor arguments, which the reference forwards verbatim from the YAML
 * (glow/lets_face_it_glow.py:61-70: `Adam(params, lr=lr, **Optim["args"]["adam"])`): weight_decay (L2 term `wd * p` added to the
 * clipped gradient before the moments) and amsgrad (vmax = running maximum of the second moment, used in the denominator; NULL =
 * off). hyper: NULL, or the device block of a captured step (as lfi_adam_clip_step_dev; lr / step_count are then not read). */
int lfi_adam_clip_step_ex(float* p, const float* g, float* m, float* v, float* vmax, long n, const double* sumsq, float clip,
                          float gmul, float lr, float beta1, float beta2, float eps, float weight_decay, int step_count,
                          const float* hyper, void* stream);

/* The other two optimisers configure_optimizers can build (glow/lets_face_it_glow.py:61-72: `{"adam", "sgd", "rmsprop"}[name](params,
 * lr=hparams.lr, **hparams.Optim["args"][name])`; hparam_tuning_configs/large_hparam_search.py:9-11 draws all three), on the same
 * flat buffers with the same global-norm clip in front: torch.optim.SGD (momentum, dampening, weight_decay, nesterov; final_model.yaml:
 * momentum 0.9; buf = the momentum buffer, may be NULL when momentum == 0; step_count 1-based: the first step sets buf = g) and
 * torch.optim.RMSprop (alpha, eps, weight_decay, momentum, centered: sq = the square average, buf = the momentum buffer or NULL,
 * gavg = the centered variant's gradient average or NULL; final_model.yaml: eps 1e-8, torch defaults otherwise). */
int lfi_sgd_clip_step(float* p, const float* g, float* buf, long n, const double* sumsq, float clip, float gmul, float lr,
                      float momentum, float dampening, float weight_decay, int nesterov, int step_count, void* stream);
int lfi_rmsprop_clip_step(float* p, const float* g, float* sq, float* buf, float* gavg, long n, const double* sumsq, float clip,
                          float gmul, float lr, float alpha, float eps, float weight_decay, float momentum, void* stream);

/* Running average of the flat parameter buffer (Polyak / EMA), one launch behind whichever optimiser step ran, eager or inside a
 * captured step: ema[i] += a * (p[i] - ema[i]) in fp32 with a = (float)(1.0 - (double)decay), the lerp of
 * torch.optim.swa_utils.get_ema_multi_avg_fn(decay). 0 <= decay < 1 (NaN refused); the two ranges must not overlap; either pointer may
 * sit at any 4-byte offset (16-byte loads and stores when both are 16-byte aligned); n == 0 succeeds without a launch. The first
 * average is a copy of the parameters and is the caller's to make (GlowEngine.ema_update). */
int lfi_ema_update(float* ema, const float* p, long n, float decay, void* stream);

/* The training step as a captured hipGraph (lets_face_it_amd/glow/lets_face_it_glow.py, fused_training_step): what changes from
 * one optimiser step to the next - the dropout-mask key, Adam's bias-corrected step size - lives in a 32-byte device block
 * (u64 seed, u64 mask offset, f32 step_size = lr / (1 - beta1^t), f32 1 / sqrt(1 - beta2^t)) that lfi_set_step_params fills with
 * an ordinary launch before every replay; the _dev variants of the two kernels read it instead of taking the values as
 * arguments. The host computes the two floats exactly as lfi_adam_clip_step does (bit-identical parameters, tested). */
int lfi_set_step_params(void* params, unsigned long long seed, unsigned long long offset, float step_size, float inv_sqrt_bc2,
                        void* stream);
int lfi_dropout_masks_dev(int count, float* const* out, const long* n, const float* keep, const unsigned long long* seed_offset,
                          void* stream);
int lfi_adam_clip_step_dev(float* p, const float* g, float* m, float* v, long n, const double* sumsq, float clip, float gmul,
                           float beta1, float beta2, float eps, const float* hyper /* = params + 16 bytes */, void* stream);

/* ---------------------------------------------------------------- non-finite step guard
 * A step whose flat gradient (after the all-reduce, after gmul) holds a NaN or an Inf is not taken: parameters, optimiser state and
 * the running average keep their bits, Adam's t does not advance, a momentum buffer / average that did not exist still does not.
 * This is torch.optim + clip_grad_norm_ + the EMA lerp with optimizer.step() and the EMA update not called on that step. The decision
 * is taken on the device from the fp64 sum of squares (fp64 cannot overflow on 2^63 squares of fp32 values: the sum is finite exactly
 * when every element is; gradients of +-3e38 are legal) and lives, with everything that depends on it, in a guard record of
 * LFI_GUARD_SLOTS 8-byte slots that the caller allocates (8-byte aligned) and seeds:
 *   SKIPPED, CONSECUTIVE, APPLIED  u64 counters (steps skipped / skipped in a row / taken);
 *   LAST_NORM   fp64 sqrt(sumsq) * |gmul| of the last decide, before the clip (NaN / Inf on a skipped step);
 *   MAX_NORM    fp64, the largest finite norm seen;
 *   APPLY       u64, 1 = take this step, 0 = skip it;
 *   STEP_FLOATS two fp32: step_size = lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) for t = APPLIED, what the guarded Adam reads;
 *   MOMENTUM_LIVE, AVERAGE_LIVE  u64: bit 0 = the momentum buffer / the average held a value BEFORE this step (what this step's
 *               kernels read: 0 makes SGD set buf = g and the averaging copy), bit 1 = it holds one after it. Seed with 0 or 3.
 * lfi_grad_guard = lfi_grad_sumsq (same stage 1, a second stage with the same adds in the same order: sumsq[0] has the same bits)
 * whose last workgroup moves the record. flags: bit 0 = the optimiser behind it keeps a momentum buffer that a taken step
 * initialises (SGD with momentum), bit 1 = an averaging update follows. step_size / inv_sqrt_bc2 are the host's floats for ITS step
 * count t_host (1-based), computed as lfi_adam_clip_step computes them: they are taken as they are while APPLIED + 1 == t_host - every
 * step until one has been skipped and the host has not yet read the record - and otherwise re-based on the device in fp64 to
 * t = APPLIED + 1: step_size * (1 - beta1^t_host) / (1 - beta1^t), 1 / sqrt(1 - beta2^t). Optimisers without bias correction pass 0 / 0.
 * The _dev form reads the two floats and t_host from a step-params block (lfi_set_step_params_t): a captured step.
 * The _guard optimisers and lfi_ema_update_guard are lfi_adam_clip_step_ex (vmax NULL and weight_decay 0: lfi_adam_clip_step) /
 * lfi_sgd_clip_step / lfi_rmsprop_clip_step / lfi_ema_update - same arithmetic, same bits - that return before their first load when
 * APPLY == 0 and take the step floats, "first step" and copy-versus-lerp from the record. Refused calls launch nothing. */
#define LFI_GUARD_SKIPPED 0
#define LFI_GUARD_CONSECUTIVE 1
#define LFI_GUARD_APPLIED 2
#define LFI_GUARD_LAST_NORM 3
#define LFI_GUARD_MAX_NORM 4
#define LFI_GUARD_APPLY 5
#define LFI_GUARD_STEP_FLOATS 6
#define LFI_GUARD_MOMENTUM_LIVE 7
#define LFI_GUARD_AVERAGE_LIVE 8
#define LFI_GUARD_SLOTS 9
int lfi_grad_guard(const float* g, long n, double* sumsq, double* work /* 1024 doubles */, void* rec, float gmul, int flags,
                   float beta1, float beta2, float step_size, float inv_sqrt_bc2, unsigned long long t_host, void* stream);
int lfi_grad_guard_dev(const float* g, long n, double* sumsq, double* work /* 1024 doubles */, void* rec, float gmul, int flags,
                       float beta1, float beta2, const void* step_params, void* stream);
int lfi_adam_clip_step_guard(float* p, const float* g, float* m, float* v, float* vmax, long n, const double* sumsq, float clip,
                             float gmul, float beta1, float beta2, float eps, float weight_decay, const void* rec, void* stream);
int lfi_sgd_clip_step_guard(float* p, const float* g, float* buf, long n, const double* sumsq, float clip, float gmul, float lr,
                            float momentum, float dampening, float weight_decay, int nesterov, const void* rec, void* stream);
int lfi_rmsprop_clip_step_guard(float* p, const float* g, float* sq, float* buf, float* gavg, long n, const double* sumsq, float clip,
                                float gmul, float lr, float alpha, float eps, float weight_decay, float momentum, const void* rec,
                                void* stream);
int lfi_ema_update_guard(float* ema, const float* p, long n, float decay, const void* rec, void* stream);
/* lfi_set_step_params plus the step number the two floats belong to, in the block's last 8 bytes (u64 t_host, 1-based). */
int lfi_set_step_params_t(void* params, unsigned long long seed, unsigned long long offset, float step_size, float inv_sqrt_bc2,
                          unsigned long long t_host, void* stream);

/* ---------------------------------------------------------------- per-array statistics, and the blame record of a skipped step
 * lfi_segment_stats looks once at many fp32 arrays: the nseg segments (offset, length: int64 pairs in DEVICE memory, in floats,
 * disjoint, inside [0, n), any 4-byte position, gaps allowed and never read) of the flat buffer `flat` of n floats, then nextra
 * (<= 8) further arrays given as host lists of pointers and lengths (passed by value, as lfi_absmax_f32's). Array i of the
 * nseg + nextra fills record i of `out`, LFI_SEG_SLOTS 8-byte slots:
 *   SUMSQ  fp64 sum of squares of its FINITE elements;   NAN / INF  u64 counts of NaNs / of +-Inf;
 *   FIRST  u64 index within the array of its first non-finite element, all ones when it has none.
 * A zero-length array yields zeros and FIRST = all ones. Three launches for any number of arrays: arrays are cut into chunks of
 * lfi_segment_stats_chunk() floats, one workgroup per chunk leaves its partials in `work` (lfi_segment_stats_work_floats floats,
 * 8-byte aligned), one workgroup sums each array's partials in chunk order. No atomics: the same input gives the same bits on every
 * run and from either entry point. Null pointers, nseg < 0, nextra > 8, negative lengths and misaligned records / work buffers are
 * refused before any launch; an empty call succeeds.
 * lfi_segment_stats_guard is the same work behind the step guard: `rec` is the guard record (read only), `blame` a record of
 * LFI_BLAME_HEAD + LFI_SEG_SLOTS * (nseg + nextra) slots: FILLED (u64 0 / 1), STEP (u64, 1-based number of the step the table
 * belongs to: APPLIED + SKIPPED as the decide kernel left them), then the table above. While rec's APPLY is 1, or FILLED is 1, every
 * workgroup of every launch returns before its first load of data and nothing is written (the FIRST skipped step since the host
 * cleared the header is the one kept). Otherwise the table is filled, then STEP, then FILLED: the call's last store. */
#define LFI_SEG_SUMSQ 0
#define LFI_SEG_NAN 1
#define LFI_SEG_INF 2
#define LFI_SEG_FIRST 3
#define LFI_SEG_SLOTS 4
#define LFI_BLAME_FILLED 0
#define LFI_BLAME_STEP 1
#define LFI_BLAME_HEAD 2
long lfi_segment_stats_chunk(void);
long lfi_segment_stats_work_floats(long n, int nseg, int nextra, const long* xlen);
int lfi_segment_stats(const float* flat, long n, const long* segs, int nseg, int nextra, const float* const* xptrs, const long* xlen,
                      void* out, void* work, void* stream);
int lfi_segment_stats_guard(const float* flat, long n, const long* segs, int nseg, int nextra, const float* const* xptrs,
                            const long* xlen, const void* rec, void* blame, void* work, void* stream);

/* ---------------------------------------------------------------- per-row keyed sampling noise (a counter-based prior for samplers)
 * rng: DEVICE memory, B x 2 64-bit words, (key, position) per row. For row r with key K, the frame at position p, candidate k
 * (0 for a plain step) and channel c:
 *   o[0..3] = Philox4x32-10 with key words (lo32(K), hi32(K)) and counter words (c >> 2, lo32(p), hi32(p), k)
 *   u_j = (o_j >> 9) * 2^-23 + 2^-24                       exact in fp32, inside (0, 1), never 0 or 1
 *   g0 = sqrt(-2 ln u0) cos(2 pi u1), g1 = sqrt(-2 ln u0) sin(2 pi u1); g2, g3 likewise from (u2, u3); channel c takes g[c & 3]
 *   z = eps * g, |g| <= sqrt(48 ln 2) ~ 5.77               accurate logf / sqrtf / sincospif, fp32 throughout
 * lfi_row_noise: out[i * stride_frame + r * stride_row + k * stride_cand + c] = eps * g(key_r, pos_r + i, k, c) for i < n, r < B,
 * k < max(ncand, 1), c < C (strides in floats): (B, C), (B, ncand, C), (n, B, C) and (n, B, ncand, C) are all one call, padded
 * layouts too. `out` may sit at any 4-byte address; nothing but the addressed elements is written. With advance > 0 the SAME
 * launch then sets pos_r += advance (every read of a row's position precedes its write: one workgroup per row, a barrier between);
 * n == 0 with advance > 0 only advances. One launch, deterministic, no atomics, capturable. Null pointers, negative sizes or
 * strides and ncand > 256 are refused before the launch; B == 0, and nothing to write with advance == 0, succeed without one.
 * lfi_row_rng_advance: pos_r += lens ? max(lens[r], 0) : delta (lens: B ints on the device) - for frames a row takes without a
 * draw (observed frames, a caller's own noise). */
int lfi_row_noise(unsigned long long* rng /* device, B x 2: (key, pos) */, int B, int n, int ncand, int C, float eps, float* out,
                  long stride_frame, long stride_row, long stride_cand, int advance, void* stream);
int lfi_row_rng_advance(unsigned long long* rng, int B, long delta, const int* lens /* device int32 B, or null */, void* stream);
/* The row state moves with the row (SampleStream open / reset / reset_rows / save_rows / load_rows of a keyed session). rows,
 * entries, keys and positions are HOST lists that travel in the kernel arguments, 128 rows per launch (a longer list is several
 * launches): allocation-free, no host staging, no host wait. Only the listed rows are written; one thread owns one listed row,
 * plain 8-byte stores. Every argument, every row and entry included, is checked before the first launch: null pointers, negative
 * sizes, a row outside 0 .. B - 1 or listed twice, an entry outside 0 .. nsaved - 1 are argument errors; nrows == 0 succeeds
 * without a launch.
 * seed: rng[rows[j]] = (keys[j], positions ? positions[j] : 0); rows == NULL lists rows 0 .. nrows - 1; keys == NULL keeps every
 * listed row's key and sets only its position.
 * save: out[j] = rng[rows[j]], out nrows x 2 64-bit words on the device; rng is not written.
 * load: rng[rows[j]] = saved[entries[j]] (saved: nsaved x 2 words on the device; an entry may repeat - a branch); with keys (host)
 * the row takes keys[j] and the saved entry's position - a branch that draws differently from its sibling. */
int lfi_row_rng_seed_rows(unsigned long long* rng, int B, int nrows, const int* rows, const unsigned long long* keys,
                          const unsigned long long* positions, void* stream);
int lfi_row_rng_save_rows(const unsigned long long* rng, int B, int nrows, const int* rows, unsigned long long* out, void* stream);
int lfi_row_rng_load_rows(unsigned long long* rng, int B, int nrows, const int* rows, const int* entries, int nsaved,
                          const unsigned long long* saved, const unsigned long long* keys, void* stream);

/* ---------------------------------------------------------------- callers either side of the flow (SURVEY.md par. 8f)
 * Window sampler, replaces MimicryDataset.__getitem__ + DataLoader collation (code/glow_pytorch/mimicry_data_module.py:45-78):
 * one modality of a split lives in HBM as ONE (rows x dim) matrix, the recording bins back to back; a training window is T
 * consecutive rows of one bin. dst[b, t, :] = src[starts[b] + t, :] for b < B (starts: B row indices, int64, on the device;
 * the host-side index table guarantees starts[b] + T does not cross a bin boundary). dst: (B x T x dim), batch-first. */
int lfi_gather_sequences(const float* src, long rows, int dim, const long* starts, int B, int T, float* dst, void* stream);
/* calc_jerk (code/glow_pytorch/glow/utils.py:53-58; MimicryLogger, mimicry_logger.py:187-196): out[0] = mean over (B, T-3, C)
 * of |third difference along time| of x (B x T x C, batch-first, fp32 differences as the reference). work: 1024 doubles. */
int lfi_jerk_mean(const float* x, int B, int T, int C, float* out, double* work /* 1024 doubles */, void* stream);

/* ---------------------------------------------------------------- diagnostics */
/* Timing probe of the register-resident forward cells: a device buffer of >= 16 * Ks 64-bit slots stamped with s_memtime
 * (100 MHz) at the phase boundaries of the cells in workgroup column 0; NULL switches it off. Process-global - the ONE piece of
 * global mutable state in this library, null in normal operation (a per-thread pointer was tried in round 5: PyTorch runs the
 * backward pass on its autograd thread, so the walks' backward stamps never saw it). Set it only around a single-engine
 * diagnostic run (tools/pipe_stamps.py, tools/rev_stamps.py). */
int lfi_debug_set_stamps(void* device_buffer);
/* Checks the MFMA operand/accumulator lane maps the kernels rely on; out[0] = number of mismatches. */
int lfi_selftest_mfma(int* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LFI_H */
