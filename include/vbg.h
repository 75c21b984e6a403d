/* libvbg — C-ABI of the MI355X-native ViBERTgrid hot path (gfx950 only).
 *
 * The reference (ZeningLin/ViBERTgrid-PyTorch) is 100 % Python: it has no FFI, so there is no
 * existing binding to mirror.  Each entry point below replaces the third-party library call the
 * reference makes at the cited file:line (paths relative to the reference root); the Python side
 * that binds them with ctypes is vibertgrid-pytorch_amd/vbg/lib.py, and INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named `h_*`;
 *   - activations are NHWC / row-major [rows, channels] fp32; index tensors are int32 unless noted;
 *   - `stream` is a hipStream_t; nothing uses the default stream, nothing synchronises the device;
 *   - the caller owns every buffer including workspaces; the library keeps no mutable global state;
 *   - return value: 0 ok, negative = argument error (VBG_EARG = -1), positive = hipError_t;
 *   - re-entrant: may be called concurrently from autograd worker threads on different streams.
 */
#ifndef VBG_H
#define VBG_H

#ifdef __cplusplus
extern "C" {
#endif

#define VBG_VERSION 100

int vbg_version(void);

/* ------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM convolution (fp32 MFMA).  C[M,N] (+)= opA[M,K] * opB[K,N].
 * Replaces: torch.nn.Linear / Conv2d forward+backward inside transformers.BertModel
 * (model/BERTgrid_generator.py:134), model/ResNetFPN_ViBERTgrid.py:478-508 & 612-648,
 * model/semantic_segmentation_head.py:66-78, model/field_type_classification_head.py:64-75,
 * 181-188, 564-575, and torch.cat + conv1x1 / Linear fusions at ResNetFPN_ViBERTgrid.py:317-318,
 * 505-506, field_type_classification_head.py:185-188 (K segments read in place: no concat).
 * ------------------------------------------------------------------------------------------ */
enum {
    VBG_OP_DENSE_K = 0, /* elem(row,k) = p[row*ld + k]      (k contiguous; A may have K segments)  */
    VBG_OP_DENSE_R = 1, /* elem(row,k) = p[k*ld + row]      (row contiguous)                        */
    VBG_OP_CONV_K = 2,  /* A only: row = output pixel, k = (tap, channel) gathered from NHWC source */
    VBG_OP_CONV_R = 3,  /* B only: k = output pixel, col = (tap, ci) gathered from NHWC source      */
    VBG_OP_WT_R = 4     /* B only: conv weight [Cout][taps][Cin] read as k = (tap, co), col = ci    */
};
enum { VBG_EPI_NONE = 0, VBG_EPI_RELU = 1, VBG_EPI_GELU_DUAL = 2 /* C = x, C2 = gelu_erf(x) */,
       VBG_EPI_MUL_GELU_GRAD = 3 /* vbg_plane_gemm only: C = x * gelu_erf'(C2), C2 = h is an INPUT (GELU backward in the data-gradient product) */ };

typedef struct vbg_conv_geo {
    int Hs, Ws, Cs;      /* gather-source tensor [*, Hs, Ws, Cs] (X for fwd/wgrad, dY for dgrad)   */
    int Hr, Wr;          /* spatial dims of the row space (output pixels; dX pixels for dgrad)      */
    int kh, kw, stride, pad;
    int dgrad;           /* 0: src = row*stride - pad + tap;  1: src = (row + pad - tap) / stride   */
} vbg_conv_geo;

/* Frozen BatchNorm (torch.nn.BatchNorm2d in eval mode behind a bias-free convolution, model/ResNetFPN_ViBERTgrid.py:116-123) as the
 * EPILOGUE of the convolution that feeds it: with v the finished accumulator of output channel c,
 *   v = (v - mean[c]) * invstd[c] * gamma[c] + beta[c];  v += res[row][c] (res != NULL);  v = max(v, 0) (relu != 0);  store v
 * -- the expression and order of vbg_bn_apply, so conv + vbg_bn_apply and the fused launch agree to the compiler's contraction of the
 * same expression.  amax (optional): an amax slot (VBG_AMAX_WORDS words, zeroed by the caller) that receives the bit pattern of the
 * launch's max |v|, as vbg_bn_apply's y_amax.  mean, invstd, gamma, beta: [N] fp32; res: the output's shape and row stride, 16-byte
 * aligned, not the output itself.  No float atomics: legal in deterministic mode. */
typedef struct vbg_bn_epilogue {
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    const float* res;
    int relu;
    unsigned* amax;
} vbg_bn_epilogue;

typedef struct vbg_gemm_desc {
    int M, N, K;
    const float* A; long long lda; int a_kind; int a_vec;   /* a_vec: 16-byte vector loads legal   */
    /* DENSE_K A may be split along K into up to 4 segments, each its own tensor read in place;     */
    /* shift>0: the segment lives at 1/2^shift resolution (nearest-upsampled on the fly), rows are  */
    /* pixels of an [*, a_H, a_W] map.                                                               */
    int a_nseg; const float* a_seg_ptr[4]; int a_seg_kend[4]; long long a_seg_ld[4]; int a_seg_shift[4];
    int a_H, a_W;
    int a_prologue; float a_scale;                          /* 1: a = max(a,0)*a_scale              */
    const float* B; long long ldb; int b_kind; int b_vec;
    vbg_conv_geo geo;
    float* C; long long ldc; float* C2; const float* bias;  /* bias[N] or NULL                      */
    int epi; float alpha; int accumulate;                   /* C += result (atomic only if splitk>1)*/
    int splitk;                                             /* >1 requires accumulate; 1 = never split; 0 = the library may zero C and
                                                               split a long reduction with few output tiles (linear epilogues only;
                                                               atomic order is not reproducible run to run)                         */
    int tile;                                               /* 0 auto, BM*1000+BN: 128128/128064/64064 */
    /* grouped problems: grp[g*8 + {0..6}] = M, N, K, offA, offB, offC, offBias (elements; offsets */
    /* are relative to A/B/C/bias and may be negative); NULL = single problem                       */
    const long long* grp; int ngroups; int grp_maxM, grp_maxN;
    int bk;                                                 /* k-tile depth: 0 auto, 16 or 32       */
    /* optional BatchNorm statistics of the OUTPUT, fused into the epilogue (the conv in front of a training-mode BatchNorm,
       model/ResNetFPN_ViBERTgrid.py:116-123): per column sum and sum of squares of the stored values are added (fp64 atomics) into
       slot row (row-tile index % stats_slots) of stats[stats_slots][2*N]; needs splitk == 1, no accumulate, ldc % 4 == 0, C 16-B aligned.
       The statistics are added on the LDS-staged store path: a tile / bk request that names an instance without one (fp32 form, 128-row
       tile, 16-deep k-tiles) runs the 64 x 64 tile of the same depth instead */
    double* stats; int stats_slots;
    /* arithmetic form of the products.
       0: v_mfma_f32_32x32x2_f32, exact fp32 products.
       1: amp -- operands stay fp32 in memory, are rounded to bf16 (nearest even) inside the kernel and multiplied with
          v_mfma_f32_32x32x16_bf16, fp32 accumulation; replaces torch.cuda.amp.autocast of pipeline/train_val_utils.py:264 for
          these ops.
       3: fp32-grade on the bf16 matrix cores -- every operand element is split exactly into three bf16 pieces inside the kernel and
          each product is the fp32 sum of the six piece products of order <= 2^-16 (error <= 2^-23 of the product).
       2 (round 6): fp32-grade on the fp16 matrix cores for operands INSIDE fp16's range -- two pieces per element (hi = fp16(x), lo' =
          fp16((x - hi) 2^11), round to nearest), three piece products: half the matrix-core work of form 3, the same measured error
          against fp64; |x| >= 65520 becomes inf, never a clipped value.  The FORWARD kinds only (A DENSE_K / CONV_K, B DENSE_K: activations
          and weights) where they run 64 x 64 tiles; any other kind or tile given form 2 runs form 3 (on the 128 x 128 tiles it measured slower).
       Forms 1 and 3 need 16-byte aligned operands (a_vec, b_vec); form 3 is not available for row-contiguous A (the library uses
       form 0 there), and products whose geometry forces 16-deep k-tiles run as form 0.  Results of all forms agree to fp32
       rounding for 0 / 3 and to bf16 operand rounding for 1. */
    int bf16;
    /* round 6, optional: DETERMINISTIC split of the reduction.  splitk > 1 with slab_stride > 0 (elements): split s of the k range STORES its
       partial product at C + s * slab_stride (plain stores, no atomics; no bias / epilogue / accumulate / groups / statistics), and
       vbg_slab_reduce adds the slabs in split order, with the bias and an optional ReLU.  For products with a handful of output tiles and a
       very long reduction: the first layer of the field-type classifier on ONE document is 128 x 1024 outputs over k = 13 312
       (model/field_type_classification_head.py:78-110) -- 32 tiles of 416 k-tiles otherwise. */
    long long slab_stride;
    /* optional: frozen-BatchNorm epilogue (below); bn.mean == NULL (a zeroed value): none.  The row stride of bn.res is ldc.  An argument
       error together with stats, accumulate, splitk != 1, slab_stride, groups, C2, epi != NONE, bias, N % 4 != 0, ldc % 4 != 0, a C or
       bn.res that is not 16-byte aligned, or bn.res == C. */
    vbg_bn_epilogue bn;
} vbg_gemm_desc;

int vbg_gemm(const vbg_gemm_desc* desc, void* stream);
/* Which kernel instance vbg_gemm would run for this descriptor, decided by the function vbg_gemm itself launches from: host only (no
 * device call, no pointer of the descriptor is dereferenced, the automatic split zeroes nothing), the return codes of vbg_gemm.
 *   out = { BM, BN, BK, vec (1: 16-byte loads, 0: the scalar-load path), prec (the arithmetic form that RUNS: 0 / 1 / 2 / 3 as
 *           vbg_gemm_desc.bf16), splitk in effect (the automatic split's choice for splitk = 0), 1: the tile leaves through the LDS-staged
 *           float4 store path / 0: per-lane stores or atomics, accumulate in effect (1 as well where the automatic split adds into a
 *           zeroed C) }
 * An empty problem (M, N or the group count 0) launches nothing: VBG_OK with out all zero. */
int vbg_gemm_variant(const vbg_gemm_desc* desc, int out[8]);
/* Measurement hooks (bench.py `roofline`; no reference counterpart): the same launch with the dispatch's own begin / end
 * timestamps delivered to two events (hipExtLaunchKernel start / stop events: no barrier packets around the kernel, the figure
 * rocprofv3's kernel trace reports), plus create / destroy / elapsed for those events (hipEvent_t passed as void*). */
int vbg_gemm_timed(const vbg_gemm_desc* desc, void* stream, void* start_event, void* stop_event);
/* out[m][n] = (relu ? max(., 0) : .)(sum_{s < nslabs, in order} slabs[s * slab_stride + m * lds + n] + bias[n])  (bias may be NULL; N % 4 == 0) */
int vbg_slab_reduce(const float* slabs, int nslabs, long long slab_stride, int M, int N, long long lds, const float* bias, int relu,
                    float* out, long long ldc, void* stream);
int vbg_timer_create(void** event);
int vbg_timer_destroy(void* event);
int vbg_timer_elapsed_ms(void* start_event, void* stop_event, float* ms);

/* ------------------------------------------------------------------------------------------
 * Plane GEMM: the same fp32-grade NT product as vbg_gemm form 3, from operands that were split into bf16 planes ONCE
 * (by vbg_split_planes / vbg_split_planes_t or by a producing epilogue) instead of inside every block of every product.
 * A plane operand is [3][rows][ld] bf16 (hi, mid, lo: x = hi + mid + lo exactly), K-contiguous, ld a multiple of 8 and
 * >= K, K a multiple of 32 (the split kernels zero-pad).  C[M,N] (+)= alpha * A[M,K] * B[N,K]^T (+ bias[N]).
 * Replaces: torch.nn.functional.linear inside transformers BertModel (model/BERTgrid_generator.py:134) and its autograd
 * products (dgrad with the transposed weight planes, wgrad with transposed activation planes), the MLP heads
 * (model/field_type_classification_head.py:78-110).
 * ------------------------------------------------------------------------------------------ */
#define VBG_PLANE_MAX_GROUPS 4
typedef struct vbg_plane_group {                                  /* one problem of a grouped plane GEMM launch */
    const unsigned short* A; const unsigned short* B; float* C;
    long long a_plane, lda, b_plane, ldb, ldc;
    int M, N;
    int tiles_m, tiles_n;                                         /* filled by the library */
    const unsigned* a_amax;                                       /* form 1: amax slot whose power of two A was scaled by, or NULL */
} vbg_plane_group;
typedef struct vbg_plane_gemm_desc {
    int M, N, K;
    const unsigned short* A; long long a_plane; long long lda;   /* plane stride / row stride in elements */
    const unsigned short* B; long long b_plane; long long ldb;
    float* C; long long ldc; float* C2; const float* bias;       /* C may be NULL when only Cp is wanted   */
    /* optional: the stored value (after bias / ReLU / GELU) split into planes [3][M][ldp] -- the A operand of the next product */
    unsigned short* Cp; long long c_plane; long long ldp;
    int epi; float alpha; int accumulate;                         /* C += result (atomics only if splitk > 1) */
    int splitk;                                                   /* >1 requires accumulate */
    int tile;                                                     /* 0 auto; 256256 / 256128 / 128128 / 128129 / 128130 / 128064 / 64064;
                                                                     64004: 64 x 64 with four LDS stages (forms 1, 2: cold weights, few tiles) */
    /* trans != 0 ("TN"): C[M,N] (+)= alpha * sum_k A[k,M] * B[k,N] -- the reduction index is the operands' ROW index: A planes
       [3][K][lda], B planes [3][K][ldb], lda / ldb multiples of 32 (zero padded), K any length.  The weight gradient dW = dY^T X
       straight from the planes of dY and X that the data-gradient / forward products already use (LDS transpose reads). */
    int trans;
    /* ngroups > 0: a grouped launch -- grp[0..ngroups) are independent problems of ONE reduction length K (and one `trans`,
       `accumulate`, `alpha`) that share the grid, so their partial rounds of output tiles fill the chip together (the four weight
       gradients of an encoder layer: 432 tiles in 2 rounds instead of 4 launches of <= 144 tiles on 256 CUs).  No bias / epilogue. */
    int ngroups;
    vbg_plane_group grp[VBG_PLANE_MAX_GROUPS];
    /* optional: colsum[n] += sum_m (stored value)[m][n] (atomics, one per column and row tile): the bias gradient of the layer whose
       output gradient this product produces (NT, no split-K / groups / accumulate / GELU-dual / 256256 tile) */
    float* colsum;
    /* form 1 (NT, tiles 128129 / 128130 / 256128, no split-K / groups): A and B are TWO fp16 planes [2][rows][ld] written by
       vbg_split_planes_pair, a producer's pair output or Cq below: hi = fp16(x), lo' = fp16((x - hi) 2^11), round to nearest; three
       piece products (hi hi, and lo' hi + hi lo' scaled by 2^-11 in the epilogue).  Half the matrix-core work and 4 instead of 6
       operand bytes per element for operands inside fp16's range (the forward products: LayerNorm / GELU outputs and weights);
       |x| >= 65520 becomes inf.  form 0: three bf16 planes, six piece products.
       form 2 (`amp`: the reference's autocast linears, pipeline/train_val_utils.py:264): the same fp16-pair operands, ONE product on their hi
       planes (x rounded to fp16; a_amax as in form 1), fp32 accumulation; tiles 128129 / 256128, NT and the weight-gradient products. */
    int form;
    /* optional: the stored value (after bias / GELU) also as fp16-pair planes [2][M][ldq] (plane stride q_plane elements) */
    unsigned short* Cq; long long q_plane; long long ldq;
    /* form 1, optional: the A planes hold x * 2^e, e = the power of two that brings the value of this amax slot to [2^13, 2^14)
       (vbg_split_planes_pair with the same slot): the product is scaled back by 2^-e -- a GRADIENT as the A operand.  With trans != 0
       form 1 also covers the weight-gradient products (single and grouped: vbg_plane_group.a_amax per problem). */
    const unsigned* a_amax;
    /* optional (NT): amax slot that receives max |stored value| of this launch (zeroed by the caller) */
    unsigned* c_amax;
    /* optional (NT 8-wave tiles, with Cq; round 4): the Cq planes hold (stored value) * 2^e where e comes from a rigorous BOUND of the
       stored values instead of their measured maximum -- a GRADIENT leaves the epilogue as pair planes without a split pass of its own:
       bound = value(cq_ref_in: an amax slot holding max |A operand|, unscaled) * value(*cq_l1_in: float bits of max_j sum_k |B[j][k]|, the
       largest row L1 norm of the NT B operand; NULL: 1) * cq_mul (the epilogue's Lipschitz constant, e.g. 1.13 for the GELU gradient, and
       the rounding margin); |sum_k a_k b_jk| <= max |a| * sum_k |b_jk| holds for every element.  The bound's bit pattern is written to
       word 0 of the zeroed amax slot cq_ref_out: consumers pass that slot as a_amax.  The two-piece form keeps 22 bits over ~30 binades,
       so a bound 2^5 ... 2^10 above the true maximum costs no precision. */
    const unsigned* cq_ref_in; const unsigned* cq_l1_in; float cq_mul; unsigned* cq_ref_out;
} vbg_plane_gemm_desc;
/* out[i] = max(out[i], bits of max_c sum_r |w_i[r][c]|) for n matrices (w_i [rows_i][cols_i], row stride ld_i): the largest column L1
 * norm -- with w = the nn.Linear weight [out, in] of a layer, the bound factor of the data gradient dY W (a cq_l1_in word).  One launch
 * for a table of matrices (device memory; max_cols = the largest cols_i); `out` words are maxed into: zero them first. */
typedef struct vbg_l1_entry { const float* w; long long ld; int rows, cols; } vbg_l1_entry;
int vbg_col_l1_max(const vbg_l1_entry* table_dev, int n, int max_cols, unsigned* out, void* stream);
int vbg_plane_gemm(const vbg_plane_gemm_desc* desc, void* stream);
int vbg_plane_gemm_timed(const vbg_plane_gemm_desc* desc, void* stream, void* start_event, void* stop_event);
/* x [rows][cols] fp32 (row stride ldx) -> planes [3][rows][ldp] (plane stride `plane` elements), columns cols..ldp-1 zero;
 * relu != 0: the pieces of max(x, 0); colsum_accum != NULL: colsum_accum[c] += sum_r x[r][c] in the same pass (the bias gradient
 * of a linear layer: torch's autograd `grad_output.sum(0)` for F.linear) */
int vbg_split_planes(const float* x, long long ldx, int rows, int cols, unsigned short* out, int ldp, long long plane, int relu,
                     float* colsum_accum, void* stream);
/* x [rows][cols] fp32 -> TRANSPOSED planes [3][cols][ldp], ldp >= rows (multiple of 32), entries rows..ldp-1 zero */
int vbg_split_planes_t(const float* x, long long ldx, int rows, int cols, unsigned short* out, int ldp, long long plane,
                       void* stream);
/* x [rows][cols] fp32 -> fp16-pair planes [2][rows][ldp] (hi, lo' as above; columns cols..ldp-1 zero): operands of form-1 products */
int vbg_split_planes_pair(const float* x, long long ldx, int rows, int cols, unsigned short* out, int ldp, long long plane,
                          const unsigned* amax, float* colsum_accum, void* stream);
/* amax (optional): x is multiplied by the power of two that brings the slot's value to [2^13, 2^14) first (gradient operands);
 * colsum_accum (optional): colsum_accum[c] += sum_r x[r][c] of the unscaled values, as in vbg_split_planes */
/* many matrices of one fp32 buffer in one launch: tbl_dev = device int64 [njobs][6] = {source offset (elements), rows, cols,
 * destination offset (elements), ldp (multiple of 32, >= rows), index of the job's first 64 x 64 tile}; job j writes the planes of
 * its matrix TRANSPOSED ([3][cols][ldp]) at dst + offset, plane stride `plane` for all jobs.  (The W^T planes of every weight of a
 * flat parameter buffer, refreshed once per optimizer step.) */
int vbg_split_planes_t_batched(const float* src, unsigned short* dst, const long long* tbl_dev, int njobs, int total_tiles,
                               long long plane, void* stream);
/* the same as fp16-pair planes [2][cols][ldp] per job (the W^T operands of the form-1 data-gradient products) */
int vbg_split_planes_pair_t_batched(const float* src, unsigned short* dst, const long long* tbl_dev, int njobs, int total_tiles,
                                    long long plane, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused self-attention on packed variable-length sequences (head width 64), fp32-grade on the bf16 matrix cores; no [L, L]
 * score / probability block is ever written.  Replaces transformers' BertSelfAttention inside BertModel
 * (model/BERTgrid_generator.py:134): softmax(Q K^T * scale) -> dropout -> P V, and its autograd.
 * Q, K, V are columns [0, hid), [hid, 2 hid), [2 hid, 3 hid) (hid = heads * 64) of the plane tensor `qkv` [3][ntok][qkv_ld]
 * (vbg_plane_gemm's Cp output); dO (backward) is a plane tensor [3][ntok][do_ld].  Sequence s owns token rows
 * [seq_row0[s], seq_row0[s] + seq_len[s]); tasks = int32 [ntasks][2] = (sequence, 128-row block) pairs; grid = ntasks x heads.
 *   mode FWD: out = O [ntok][ldo] (columns head * 64 ..); lse [2][heads][ntok_pad]: [0][head][pad_off[s] + row] = maximum m of the scaled
 *             scores of the row, [1][..] = 1 / sum exp(x - m) (the two numbers the row was normalised with; the backward modes read them);
 *   mode DQ : out = dqkv [ntok][ldo]: columns [0, hid) <- dQ; forms delta = rowsum(dO o O) from the dO planes and `o`, WRITES the rows' own
 *             sum_k P_k dP_k into `delta` (zero in the padding rows on entry) and corrects dQ for the difference with kbar;
 *   mode DKV: columns [hid, 3 hid) <- dK, dV; run it after DQ.
 * delta: fp32 [heads][ntok_pad]; pad_off[s] a multiple of 32 with room for roundup(seq_len, 32) rows, rows past a
 * sequence's length ZERO.  Dropout: mask_q / mask_k from vbg_attn_mask (NULL = none), keep_scale =
 * 65536 / (65536 - vbg_attn_drop_thr16(p)); mask_off[s] = first word of sequence s (heads * roundup(len,32) * ceil(len/32) words). */
enum { VBG_ATTN_FWD = 0, VBG_ATTN_DQ = 1, VBG_ATTN_DKV = 2 };
typedef struct vbg_attn_desc {
    int mode, heads, ntasks, max_len;                 /* max_len: longest sequence (<= 512: BERT windows) */
    const int* tasks; const int* seq_len; const int* seq_row0; const int* pad_off; long long ntok_pad;
    const unsigned short* qkv; long long qkv_plane, qkv_ld;
    const unsigned short* dO; long long do_plane, do_ld;
    float* out; long long ldo;
    float* lse; float* delta;
    unsigned short* out_planes; long long op_plane, op_ld;   /* FWD, optional: the three bf16 planes [3][ntok][op_ld] of O */
    float* kbar; long long ldk;     /* [ntok][ldk]: FWD writes sum_k P_k K_k (bf16 precision; NULL = skip), DQ reads it */
    const float* o;                 /* DQ: the forward's O as fp32 [ntok][ldk] (delta = rowsum(dO o O) is formed in the kernel) */
    const unsigned* mask_q; const unsigned* mask_k; const long long* mask_off;
    float scale, keep_scale;
    unsigned* out_amax;             /* DQ / DKV, optional: amax slot (zeroed by the caller) that receives max |value written to out| */
    unsigned short* out_pair; long long oq_plane, oq_ld;     /* FWD, optional (round 4): O also as fp16-pair planes [2][ntok][oq_ld] -- the B operand
                                                                of the output projection's weight gradient, saved for backward instead of split there */
    int form;                       /* round 5.  0: qkv / dO are three bf16 planes, six piece products per product (above);
                                       1: qkv / dO are fp16-pair planes [2][ntok][ld] (hi, (x - hi) 2^11; vbg_plane_gemm's Cq output), three fp16 piece
                                          products per product into one accumulator set (one operand of each cross product carries the 2^-11);
                                       2: the hi planes of the same tensors alone, one product (`amp`: what fp16 autocast multiplies) */
    const unsigned* do_amax;        /* forms 1 / 2, DQ / DKV: the amax slot dO's planes were scaled with (their producer's bound; NULL: unscaled) */
} vbg_attn_desc;
int vbg_attn(const vbg_attn_desc* desc, void* stream);
/* dropout keeps of one layer and step, both orientations (torch.nn.Dropout(attention_probs_dropout_prob) on the probabilities):
 * keep <=> a 16-bit slice of the counter hash >= thr16 = round(p * 65536), i.e. drop rate thr16 / 65536 */
unsigned vbg_attn_drop_thr16(float drop_p);
int vbg_attn_mask(const int* seq_len, const long long* mask_off, int nseq, int heads, int maxlen, float drop_p,
                  unsigned long long seed, unsigned long long stream_id, unsigned* mask_q, unsigned* mask_k, void* stream);
/* the same for `nlayers` encoder layers of one step in ONE launch (transformers BertSelfAttention.dropout of every layer of
 * model/BERTgrid_generator.py:134's encoder): layer l draws from stream id stream_id0 + l * stream_id_stride and owns the words
 * [l * layer_words, (l + 1) * layer_words) of mask_q / mask_k; bit-identical to nlayers calls of vbg_attn_mask */
int vbg_attn_mask_layers(const int* seq_len, const long long* mask_off, int nseq, int heads, int maxlen, float drop_p,
                         unsigned long long seed, unsigned long long stream_id0, unsigned long long stream_id_stride, int nlayers,
                         long long layer_words, unsigned* mask_q, unsigned* mask_k, void* stream);

/* column sums: out[n] (+)= sum_m x[m*ld + n]   (bias gradients) */
int vbg_colsum(const float* x, long long ld, int M, int N, float* out, int accumulate, void* stream);
/* the same with every partial sum in fp64 (ws: N doubles of caller scratch, overwritten): bias gradients of the 1x1 segmentation
 * classifiers (model/semantic_segmentation_head.py:66-78: torch's pairwise sum over ~1e6 pixel terms that cancel to 1e-3 of their
 * running magnitude) and every other bias gradient that does not ride on a split pass */
int vbg_colsum_f64(const float* x, long long ld, int M, int N, float* out, int accumulate, double* ws, void* stream);

/* 3x3 / stride 1 / pad 1 convolution, NHWC, fp32-grade split form, activation rows reused across the three horizontal taps
 * (csrc/conv3.hip): y[B,H,W,N] (+)= conv(x[B,H,W,Cs], w[N,3,3,Cs]) (+ bias); stats: BatchNorm slot workspace [slots][2][N] fp64 that
 * receives the per-channel sum / sum of squares of y (not with accumulate).  Replaces torch.nn.Conv2d(k=3, s=1, p=1) forward
 * (model/ResNetFPN_ViBERTgrid.py:478-508, 612-648; model/semantic_segmentation_head.py) and, with the filter written by
 * vbg_conv3x3_wflip, its input gradient.  Requires W a power of two >= 16, H*W % 64 == 0, Cs % 16 == 0, N % 4 == 0 -- or H = W = 7:
 * the [B,7,7,C] region-of-interest maps of the field-type head (model/field_type_classification_head.py:64-75), stored compactly, two
 * images per 128-row tile.  Filter counts that are odd multiples of 64 run 64-filter tiles.
 * nsplit > 1 (vbg_conv3x3_split(...) says how many: the late trunk stages with 64-128 tiles of 2304-4608 long reductions): nsplit
 * workgroups share a tile, each reducing one filter row (nsplit % 3 == 0) and / or one channel group; they meet through split_slab
 * ([tiles][nsplit][128*128] floats of caller scratch) and split_tickets ([tiles] words, zero on entry and left zero), the last
 * arriver adding the partial tiles in a fixed order (deterministic).  nsplit = 1: both may be NULL. */
int vbg_conv3x3_split(int B, int H, int W, int Cs, int N);
int vbg_conv3x3(const float* x, const float* w, const float* bias, float* y, double* stats, int stats_slots, int B, int H, int W,
                int Cs, int N, int accumulate, int form, const unsigned* x_amax, float* split_slab, unsigned* split_tickets,
                int nsplit, void* stream);
/* form 0: three bf16 pieces per operand, six piece products (any operands); form 1: two fp16 pieces (round to nearest), three piece
 * products -- same measured accuracy against fp64 and half the matrix-core work, for operands inside fp16's range; a magnitude of
 * 65520 or more becomes inf, never a silently clipped value.  x_amax (form 1, optional): amax slot (below) holding the bit pattern of
 * max |x| (vbg_amax, or the amax output of vbg_bn_bwd_apply): x is multiplied by the power of two that brings that maximum to
 * [2^13, 2^14) on its way into the kernel and the result by its inverse (exact), which puts a GRADIENT operand inside fp16's range:
 * the input gradient of the convolution in form 1. */
/* An "amax slot" is VBG_AMAX_WORDS = 64 device words VBG_AMAX_STRIDE = 32 words (128 bytes, one L2 line) apart -- 8 KB in all; its
 * value -- the bit pattern of a tensor's largest magnitude (non-negative floats order like their bit patterns) -- is the max over the
 * words.  Producers max INTO a slot (their blocks spread over the words: atomics on one L2 line serialise at ~10 ns each), the caller
 * zeroes it; consumers reduce the 64 words with one wave.  vbg_amax: slot = max(slot, max |x[i]|). */
#define VBG_AMAX_WORDS 64
#define VBG_AMAX_STRIDE 32
int vbg_amax(const float* x, long long n, unsigned* amax, void* stream);
/* out[ci][2-kh][2-kw][co] = w[co][kh][kw][ci]: the filter with which the input gradient of a 3x3 / s1 / p1 convolution is the
 * same convolution of dy */
int vbg_conv3x3_wflip(const float* w, int Cout, int Cin, float* out, void* stream);

/* The same convolution in form 1 with the FILTER PRE-SPLIT (round 4): `w_planes` = the fp16-pair image of the filter that
 * vbg_conv3x3_wprep wrote (flip = 0: the forward of torch.nn.Conv2d(k=3, s=1, p=1); flip = 1: the filter of the input gradient, i.e.
 * vbg_conv3x3_wflip + split in one pass).  The kernel streams the filter through LDS-DMA in 128-byte lines and spends no VALU on it;
 * results equal vbg_conv3x3(form 1) bit for bit (same pieces, same products, same order).  Needs 128-pixel tiles (the shapes for which
 * vbg_conv3x3 picks them, incl. every nsplit > 1 and the 7x7 region maps); other shapes are argument errors.
 * vbg_conv3x3_wprep: ONE launch for a table of filters (the caller keeps the table in device AND host memory; entries must stay valid
 * until the launch has run): entry = {w [Cout,3,3,Cin] fp32, out, Cout, Cin, flip, bn}; `out` receives vbg_conv3x3_wprep_bytes(Cout,
 * Cin, flip) bytes; bn = rows per filter tile = 64 when the image's row count (flip ? Cin : Cout) is an odd multiple of 64, else 128.
 * The reduction width (flip ? Cout : Cin) must be a multiple of 16. */
typedef struct vbg_conv3_wprep_entry {
    const float* w;
    void* out;
    int Cout, Cin, flip, bn;
} vbg_conv3_wprep_entry;
long long vbg_conv3x3_wprep_bytes(int Cout, int Cin, int flip, int bn);
int vbg_conv3x3_wprep(const vbg_conv3_wprep_entry* table_dev, const vbg_conv3_wprep_entry* table_host, int n, void* stream);
int vbg_conv3x3_pw(const float* x, const void* w_planes, const float* bias, float* y, double* stats, int stats_slots, int B, int H, int W,
                   int Cs, int N, int accumulate, const unsigned* x_amax, float* split_slab, unsigned* split_tickets, int nsplit,
                   int bn, void* stream);
/* `amp` form of vbg_conv3x3_pw (the reference's `amp: True`, pipeline/train_val_utils.py:264: autocast convolutions): ONE product on the
 * hi pieces -- x (scaled into range by x_amax as above) and the filter rounded to fp16, fp32 accumulation; the lo planes of the image are
 * not loaded at 128 filters per tile.  Same arguments, same image. */
int vbg_conv3x3_pw_amp(const float* x, const void* w_planes, const float* bias, float* y, double* stats, int stats_slots, int B, int H, int W,
                       int Cs, int N, int accumulate, const unsigned* x_amax, float* split_slab, unsigned* split_tickets, int nsplit,
                       int bn, void* stream);
/* The same convolution with a frozen-BatchNorm epilogue (vbg_bn_epilogue above; bn->mean must be set): y = relu?(bn(conv(x, w)) + res) from
 * ONE launch, in the split form applied by the tile's finishing workgroup after it has added the slabs in block order.  Exactly one of
 * `w` (fp32 filter [N,3,3,Cs]: form 0 or 1 as vbg_conv3x3) and `w_planes` (the plane image: form 1 = vbg_conv3x3_pw, 2 = vbg_conv3x3_pw_amp;
 * `bn_tile` = their `bn`, 0 with `w`) is given; no bias, statistics or accumulate (a BatchNorm's convolution has none).  res and y are
 * [B,H,W,N] (compact rows for the 7 x 7 region maps), 16-byte aligned, res != y. */
int vbg_conv3x3_bn(const float* x, const float* w, const void* w_planes, float* y, int B, int H, int W, int Cs, int N, int form,
                   const unsigned* x_amax, float* split_slab, unsigned* split_tickets, int nsplit, int bn_tile,
                   const vbg_bn_epilogue* bn, void* stream);
/* bn (vbg_conv3x3_pw / vbg_conv3x3_wprep_bytes): filters per tile the image was written for -- 0: the library's rule above; 64 / 128: the
 * caller's choice (64-filter tiles double the tile count of a launch: the late trunk stages, whose 128-filter tiles do not fill the chip);
 * the launch then runs 128-pixel tiles whatever the tile count, and nsplit > 1 needs N % bn == 0 (slabs of 128 * bn floats). */

/* weight gradient of that convolution: dw[Cout,3,3,Cs] += sum over pixels dy[B,H,W,Cout]^T * shifted x[B,H,W,Cs] (csrc/conv3.hip:
 * operands stay [pixel][channel] in LDS, fragments through transposing LDS reads, one load + split of x serves all nine taps).
 * The pixel range is cut into vbg_conv3x3_wgrad_strips(...) strips; slab = [strips][Cout,3,3,Cs] scratch -> each strip stores its
 * partial result plainly and a second launch adds them into dw in a fixed order (deterministic); slab = NULL -> float atomics.
 * Replaces the weight gradient autograd forms for torch.nn.Conv2d(k=3, s=1, p=1).  Requires W % 16 == 0, Cs % 32 == 0 and
 * Cout % 128 == 0 (or Cout % 64 == 0 and Cs % 64 == 0); or H = W = 7 (region maps, Cout % 128 == 0): a k-tile is then two rows of the
 * image's 8 x 8 slot grid. */
int vbg_conv3x3_wgrad_strips(int B, int H, int W, int Cs, int Cout);
int vbg_conv3x3_wgrad(const float* dy, const float* x, float* dw, float* slab, int B, int H, int W, int Cs, int Cout, int form,
                      const unsigned* dy_amax, const unsigned* x_amax, void* stream);
/* form 0: three bf16 pieces per operand, six piece products; form 1: two fp16 pieces, three piece products, both operands scaled by
 * the powers of two that bring max |dy| and max |x| (bit patterns in the device words dy_amax / x_amax: vbg_amax, or the amax outputs
 * of vbg_bn_bwd_apply / vbg_bn_apply) to [2^13, 2^14), the result scaled back: exact scaling, half the matrix-core work */

/* stem im2col: NHWC [B,H,W,C] -> [B*Ho*Wo, Kpad] with k = (dy*kw+dx)*C + c, zero padded to Kpad */
int vbg_im2col(const float* x, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad,
               float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * a1. input transform  (pipeline/transform.py:104-171, 225-271)
 * ------------------------------------------------------------------------------------------ */
/* one image CHW [3,h,w] -> normalised, bilinearly resized (align_corners=False, torch
 * recompute_scale_factor semantics: src = (dst+0.5)*(in/out)-0.5) into batch slot b of an NHWC
 * [B,H,W,3] buffer that the caller zero-filled (padding).  oh==h && ow==w is an exact copy. */
int vbg_normalize_resize(const float* img, int h, int w, int oh, int ow, const float* h_mean3, const float* h_std3,
                         float* batch_nhwc, int b, int H, int W, void* stream);
/* boxes int64 [S,4] -> int32 [S,4]: cols 0,2 *= ratio_h, cols 1,3 *= ratio_w in fp32, truncate */
int vbg_rescale_boxes(const long long* in, int S, float ratio_h, float ratio_w, int* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole of a1 for a batch (csrc/convaux.hip).  Replaces the per-image loop of pipeline/transform.py:104-171, 225-271 --
 * normalise, resize_image, resize_boxes, batch_images' zero padding -- and the packing of the boxes that the grid scatter and
 * RoIAlign read: ONE launch per VBG_TRANSFORM_MAX_IMAGES images.  `h_images` is HOST memory (B descriptors), copied into the kernel
 * arguments as vbg_field_decode's row ranges are -- no device copy, no sync; a larger batch takes several launches.
 *   formats   VBG_IMAGE_F32_CHW  fp32 [3,h,w], contiguous: the sample vbg_normalize_resize reads;
 *             VBG_IMAGE_U8_CHW   uint8 [3,h,w], contiguous;
 *             VBG_IMAGE_U8_HWC   uint8 [h,w,3], dense, a pixel's three bytes adjacent (a decoded image as it lies in memory);
 *             a byte u is the sample (float)u / 255.0f, by DIVISION, correctly rounded: the value torch's CPU
 *             `uint8 -> float32 -> .div(255)` (ToTensor) gives for all 256 bytes.  A multiplication by 1/255 differs in 126 of them.
 *             image_mean / image_std stay on the 0..1 scale for every format.
 *   image     slot i of the NHWC fp32 [B,H,W,3] batch: rows < oh and columns < ow with vbg_normalize_resize's arithmetic (the two
 *             kernels share one device function: same bits), the right and bottom padding as +0.0.  Every element of the slot is
 *             written exactly once: the caller needs no fill.
 *   boxes     int64 [S,4] (NULL with S == 0) -> rows box_row .. box_row + S of boxes_out int32 [N,4] with vbg_rescale_boxes's
 *             arithmetic and the ratios (float)((double)oh / h), (float)((double)ow / w): columns 0, 2 take the HEIGHT ratio as the
 *             reference does (:167-168).  box_doc[row] = i for those rows; box_off[i] = box_row, box_off[B] = the last image's
 *             box_row + S (box_off int32 [B + 1], may be NULL).  box_row must be the running sum of S: box_row[i + 1] = box_row[i] + S[i].
 * 64-bit indexing; bytes are read one at a time, nothing outside the 3 * h * w samples of an image is touched and no alignment is
 * assumed.  No atomics: deterministic.  Argument errors, before any launch: h, w, oh or ow < 1, oh > H, ow > W, an unknown format,
 * S < 0, rows outside [0, N), box_row not the running sum, B < 0, a NULL operand that is needed.  B == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
#define VBG_TRANSFORM_MAX_IMAGES 64
#define VBG_IMAGE_F32_CHW 0
#define VBG_IMAGE_U8_CHW 1
#define VBG_IMAGE_U8_HWC 2
typedef struct vbg_transform_image {                              /* 48 bytes */
    const void* img;
    const long long* boxes;
    int format, h, w, oh, ow;
    int S, box_row;
} vbg_transform_image;
int vbg_transform_max_images(void);
int vbg_transform_batch(const vbg_transform_image* h_images, int B, const float* h_mean3, const float* h_std3, float* batch_nhwc,
                        int H, int W, int* boxes_out, int* box_doc, int* box_off, long long N, void* stream);

/* ------------------------------------------------------------------------------------------
 * a3. BERT encoder pieces (transformers BertModel; model/BERTgrid_generator.py:134)
 * ------------------------------------------------------------------------------------------ */
/* out[t] = dropout(LN(word[ids[t]] + pos[pos_ids[t]] + type[0])) ; saves xhat/rstd for backward */
int vbg_embed_ln_fwd(const int* ids, const int* pos_ids, int ntok, int hidden, const float* word, const float* pos,
                     const float* type0, const float* gamma, const float* beta, float eps, float drop_p,
                     unsigned long long seed, unsigned long long stream_id, float* out, float* xhat, float* rstd,
                     void* stream);
int vbg_embed_ln_bwd(const float* dout, const float* xhat, const float* rstd, const int* ids, const int* pos_ids,
                     int ntok, int hidden, const float* gamma, float drop_p, unsigned long long seed,
                     unsigned long long stream_id, float* dword, float* dpos, float* dtype0, float* dgamma,
                     float* dbeta, void* stream);
/* y = LN(dropout(x) + res) * gamma + beta ; x already holds the dense output + bias */
int vbg_dropout_add_ln_fwd(const float* x, const float* res, int rows, int hidden, const float* gamma,
                           const float* beta, float eps, float drop_p, unsigned long long seed,
                           unsigned long long stream_id, float* y, float* xhat, float* rstd, void* stream);
/* the same, and y's three bf16 planes [3][rows][ldp] (plane stride `plane`; ldp == hidden leaves no padding columns to zero, a wider
 * ldp expects them zero already) -- the A operand of the plane GEMM that consumes y: saves the separate split pass */
int vbg_dropout_add_ln_fwd_planes(const float* x, const float* res, int rows, int hidden, const float* gamma,
                                  const float* beta, float eps, float drop_p, unsigned long long seed,
                                  unsigned long long stream_id, float* y, float* xhat, float* rstd, unsigned short* y_planes, int ldp,
                                  long long plane, unsigned short* y_pair, int ldq, long long qplane, void* stream);
/* (y_pair, optional: y also as fp16-pair planes [2][rows][ldq] -- the A operand of the form-1 forward products) */
/* dx (to the dense output), dres, dgamma/dbeta +=.  `slots_ws` (optional): fp32 workspace [vbg_ln_bwd_ws_rows(rows)][2][hidden]; it
 * need not be initialised and holds nothing afterwards.  With it every block of the kernel stores its column sums as one plain row and a
 * second small launch adds the rows in a fixed order (deterministic; round 5: the 516 x 2304 float atomics of the earlier slot scheme
 * were a ~9 us tail at the L2's atomic rate); without it (few rows) the sums go straight into dgamma / dbeta as atomics */
int vbg_ln_bwd_ws_rows(int rows);
int vbg_dropout_add_ln_bwd(const float* dy, const float* xhat, const float* rstd, int rows, int hidden,
                           const float* gamma, float drop_p, unsigned long long seed, unsigned long long stream_id,
                           float* dx, float* dres, float* dgamma, float* dbeta, float* slots_ws, unsigned* dx_amax, void* stream);
/* dx_amax (optional): amax slot (zeroed by the caller) that receives max |dx| -- the scale of dx as an fp16-pair operand */
/* the same with dx delivered as bf16 planes [3][rows][ldp] (not as fp32) and its column sums added into dbias_accum[hidden]: dx is the
 * gradient of the dense output in front of the LayerNorm, which is only ever a plane operand of that layer's gradient products, and
 * its column sums are that layer's bias gradient.  slots3_ws: fp32 [vbg_ln_bwd_ws_rows(rows)][3][hidden], as above (mandatory). */
int vbg_dropout_add_ln_bwd_planes(const float* dy, const float* xhat, const float* rstd, int rows, int hidden,
                                  const float* gamma, float drop_p, unsigned long long seed, unsigned long long stream_id,
                                  unsigned short* dx_planes, int ldp, long long plane, float* dres, float* dgamma, float* dbeta,
                                  float* dbias_accum, float* slots3_ws, void* stream);
/* the same with dx delivered as fp16-pair planes [2][rows][ldp] scaled by the power of two of a rigorous bound of |dx| (round 4: no split
 * pass for this gradient): bound = max |dy| (amax slot dy_amax) * max |gamma| * max rstd * (2 + sqrt(hidden)) / keep * 1.01; its bit
 * pattern goes to word 0 of the zeroed slot dx_bound (the consumers' a_amax), max |dx| itself into the zeroed slot dx_amax (optional) */
int vbg_dropout_add_ln_bwd_pair(const float* dy, const float* xhat, const float* rstd, int rows, int hidden,
                                const float* gamma, float drop_p, unsigned long long seed, unsigned long long stream_id,
                                unsigned short* dx_pair, int ldp, long long plane, float* dres, float* dgamma, float* dbeta,
                                float* dbias_accum, float* slots3_ws, const unsigned* dy_amax, unsigned* dx_amax, unsigned* dx_bound,
                                void* stream);
/* attention probabilities, in place on the grouped score buffer: for group g (= seq*heads + head)
 * rows L=len[g/heads], row stride ldp[g/heads], block offset off[g]; P = softmax(S*scale);
 * dropped entries are stored NEGATED (sign bit = dropped), kept entries unscaled; pad columns = 0.
 * maxlen <= 1024 (an argument error beyond). */
int vbg_softmax_fwd(float* s, const long long* off, const int* len, const int* ldp, int ngroups, int heads,
                    int maxlen, float scale, float drop_p, unsigned long long seed, unsigned long long stream_id,
                    void* stream);
/* dS (in place on dp) from sign-encoded P and dP_drop: dS = scale * P * (keep*dP/(1-p) - sum_j P_drop*dP_drop) */
int vbg_softmax_bwd(const float* p, float* dp, const long long* off, const int* len, const int* ldp, int ngroups,
                    int heads, int maxlen, float scale, float drop_p, void* stream);
/* y[r,:] = softmax(x[r,:]) for the returned class probabilities (field_type_classification_head.py:587) */
int vbg_row_softmax(const float* x, int rows, int cols, float* y, void* stream);
int vbg_gelu_bwd(const float* h, float* dg_inout, long long n, void* stream);      /* dh = dg * gelu'(h) */
int vbg_relu_bwd(const float* y, float* dy_inout, long long n, void* stream);      /* dx = dy * (y > 0)  */

/* ------------------------------------------------------------------------------------------
 * One encoder layer forward in ONE call (round 6; csrc/encoder.hip).  Replaces one transformers BertLayer.forward inside BertModel
 * (model/BERTgrid_generator.py:134: BertSelfAttention, BertSelfOutput, BertIntermediate, BertOutput) = the seven launches
 *   vbg_plane_gemm (stacked Q/K/V projection -> planes) -> vbg_attn(FWD) -> vbg_plane_gemm (output projection) ->
 *   vbg_dropout_add_ln_fwd_planes -> vbg_plane_gemm (FFN1, GELU) -> vbg_plane_gemm (FFN2) -> vbg_dropout_add_ln_fwd_planes
 * with exactly the descriptors the caller would have passed one by one (bit-identical results); what it saves is host time per launch.
 * A vbg_planes_ref names a plane tensor (buf NULL = absent): three bf16 planes for a form-0 product, fp16-pair planes for forms 1 / 2.
 *   form_qkv / form_ao / form_ffn: arithmetic form of the products (vbg_plane_gemm_desc.form); form_attn: of the attention (vbg_attn_desc.form;
 *   != 0: pqkv receives fp16-pair planes, else three bf16 planes).
 *   xa = planes of x in the form of form_qkv; wqkv [3 hidden][hidden], wo, wi, wo2 = weight planes in the form of their product.
 *   form_ao != 0 reads pctxq (the attention writes it), else pctx; form_ffn != 0 reads px1q / pgq, else px1 / pg; every present output
 *   plane tensor is written (the caller keeps them for backward / hands py / pyq to the next layer).
 *   Dropout streams: stream_id0 + 1 (first LayerNorm), + 2 (second); attention keeps from mask_q / mask_k (vbg_attn_mask; NULL = none). */
typedef struct vbg_planes_ref { unsigned short* buf; long long plane, ld; } vbg_planes_ref;
typedef struct vbg_bert_layer_fwd_desc {
    int ntok, hidden, inter, heads;
    float eps, drop_p; unsigned long long seed, stream_id0;
    int form_qkv, form_attn, form_ao, form_ffn;
    int tile_qkv, tile_ao, tile_ffn1, tile_ffn2;
    /* packed sequences: the fields of vbg_attn_desc */
    int ntasks, max_len; const int* tasks; const int* seq_len; const int* seq_row0; const int* pad_off; long long ntok_pad;
    const unsigned* mask_q; const unsigned* mask_k; const long long* mask_off; float attn_scale, keep_scale;
    /* inputs */
    const float* x; vbg_planes_ref xa;
    vbg_planes_ref wqkv, wo, wi, wo2;
    const float* bqkv; const float* bo; const float* bi; const float* bo2; const float* g1; const float* b1; const float* g2; const float* b2;
    /* outputs (fp32 [ntok][hidden] unless noted) */
    vbg_planes_ref pqkv;                                     /* [ntok][3 hidden] planes of q, k, v */
    float* ctx; float* lse; float* kbar; vbg_planes_ref pctx, pctxq;      /* attention output, its row statistics [2][heads][ntok_pad], kbar (optional) */
    float* ao; float* x1; float* xhat1; float* rstd1; vbg_planes_ref px1, px1q;
    float* h; vbg_planes_ref pg, pgq;                        /* h [ntok][inter] fp32; gelu(h) as planes only */
    float* fo; float* y; float* xhat2; float* rstd2; vbg_planes_ref py, pyq;
} vbg_bert_layer_fwd_desc;
int vbg_bert_layer_fwd(const vbg_bert_layer_fwd_desc* desc, void* stream);

/* The backward of that layer in ONE call (csrc/encoder.hip): the all-pair backward (every product on fp16-pair planes, forms 1 / 2) on
 * the bound route -- hidden % 256 == 0, the Q/K/V weights, biases and their gradients stacked back to back, every parameter gradient
 * accumulated straight into its destination.  Replaces the autograd of one transformers BertLayer (model/BERTgrid_generator.py:134) = the
 * ten launches
 *   vbg_dropout_add_ln_bwd_pair (LayerNorm 2: dy -> qdfo, dx1, dg2 / db2, dbo2) ->
 *   vbg_plane_gemm (qdfo Wo2^T o gelu'(h) -> qdh by the bound cq_mul_dh, column sums -> dbi) -> vbg_plane_gemm (dx1 += qdh Wi^T) ->
 *   vbg_dropout_add_ln_bwd_pair (LayerNorm 1: dx1 -> qdao, dx, dg1 / db1, dbo) -> vbg_plane_gemm (qdao Wo^T -> pdctx by the bound cq_mul_dctx) ->
 *   vbg_attn (DQ) -> vbg_attn (DKV) -> vbg_split_planes_pair (dqkv -> qdqkv, column sums -> dbqkv) -> vbg_plane_gemm (dx += qdqkv Wqkv^T) ->
 *   grouped TN vbg_plane_gemm (dwo2 += qdfo^T qg, dwi += qdh^T qx1, dwo += qdao^T qctx, dwqkv += qdqkv^T qx)
 * with exactly the descriptors the caller would have passed one by one (bit-identical results); what it saves is host time per launch.
 *   form: of the products (1, or 2 inside an autocast region); form_attn: of the two attention passes (1 or 2).
 *   Every vbg_planes_ref is fp16-pair planes [2][rows][ld].  w*_t: planes of the TRANSPOSED weights (wqkv_t [hidden][3 hidden], wo_t
 *   [hidden][hidden], wi_t [hidden][inter], wo2_t [inter][hidden]); l1_wo2 / l1_wo: their vbg_col_l1_max words.
 *   s_dy: the amax slot of dy (input).  The nine slots behind it are zeroed by the caller and distinct: s_dfo / s_dao receive max |dfo| /
 *   max |dao|, s_dfo_ref / s_dao_ref / s_dh / s_dctx the bounds their planes were scaled with, s_dx1 / s_dqkv / s_dx the maxima of those tensors.
 *   ln_ws: fp32 [vbg_ln_bwd_ws_rows(ntok)][3][hidden].  delta: fp32 [heads][ntok_pad], zero in the padding rows (vbg_attn).
 *   deterministic != 0: no float atomics -- the column sums of launch 2 are taken from its stored fp32 output det_scratch
 *   [ntok][roundup(inter, 4)] by vbg_colsum_det behind the product, those of dqkv by vbg_colsum_det in front of the split; det_ws:
 *   max(vbg_colsum_det_ws_elems(ntok, inter), vbg_colsum_det_ws_elems(ntok, 3 hidden)) doubles; the flag without both is an argument error.
 *   Dropout streams: stream_id0 + 2 (LayerNorm 2), + 1 (LayerNorm 1); attention keeps from mask_q / mask_k (NULL = none).
 *   Gradient destinations are accumulated into (+=); dx1, dqkv and the five q* / pdctx plane tensors are caller scratch that is written. */
typedef struct vbg_bert_layer_bwd_desc {
    int ntok, hidden, inter, heads;
    float drop_p; unsigned long long seed, stream_id0;
    int form, form_attn, deterministic;
    int tile_dh, tile_dx1, tile_dctx, tile_dx, tile_wgrad;   /* launches 2, 3, 5, 9, 10 */
    float cq_mul_dh, cq_mul_dctx;                            /* vbg_plane_gemm_desc.cq_mul of launches 2 and 5 */
    /* packed sequences: the fields of vbg_attn_desc */
    int ntasks, max_len; const int* tasks; const int* seq_len; const int* seq_row0; const int* pad_off; long long ntok_pad;
    const unsigned* mask_q; const unsigned* mask_k; const long long* mask_off; float attn_scale, keep_scale;
    /* inputs: the output gradient, what the forward saved, the weights */
    const float* dy; const unsigned* s_dy;
    const float* xhat2; const float* rstd2; const float* g2; const float* xhat1; const float* rstd1; const float* g1;
    const float* h; const float* ctx; float* kbar; float* lse;
    vbg_planes_ref pqkv, qx, qctx, qx1, qg;                  /* planes of q / k / v, x, the attention output, x1, gelu(h) */
    vbg_planes_ref wqkv_t, wo_t, wi_t, wo2_t;
    const unsigned* l1_wo2; const unsigned* l1_wo;
    /* amax slots (zero on entry) */
    unsigned* s_dfo; unsigned* s_dfo_ref; unsigned* s_dh; unsigned* s_dx1; unsigned* s_dao; unsigned* s_dao_ref; unsigned* s_dctx;
    unsigned* s_dqkv; unsigned* s_dx;
    /* workspaces and intermediates */
    float* ln_ws; float* delta; float* det_scratch; double* det_ws;
    vbg_planes_ref qdfo, qdh, qdao, pdctx, qdqkv;
    float* dx1; float* dqkv;                                 /* [ntok][hidden], [ntok][3 hidden] */
    /* gradients: dx [ntok][hidden] is written, the rest accumulated into */
    float* dx;
    float* dg2; float* db2; float* dbo2; float* dbi; float* dg1; float* db1; float* dbo; float* dbqkv;
    float* dwo2; float* dwi; float* dwo; float* dwqkv;       /* [hidden][inter], [inter][hidden], [hidden][hidden], [3 hidden][hidden] */
} vbg_bert_layer_bwd_desc;
int vbg_bert_layer_bwd(const vbg_bert_layer_bwd_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * a4. token -> segment aggregation  (model/BERTgrid_generator.py:148-191)
 * ------------------------------------------------------------------------------------------ */
/* tok_row[i] = row of the i-th token (mask==1 order) in `tok`; runs: start[s], len[s] in token order.
 * mode 0 mean = sequential sum in token order then / n (bit-exact vs the reference), 1 = first. */
int vbg_seg_reduce_fwd(const float* tok, const int* tok_row, const int* run_start, const int* run_len, int nseg,
                       int hidden, int mode, float* out, void* stream);
int vbg_seg_reduce_bwd(const float* dout, const int* tok_row, const int* run_start, const int* run_len, int nseg,
                       int hidden, int mode, float* dtok_accum, void* stream);

/* ------------------------------------------------------------------------------------------
 * a5 / a9. bbox -> owner map, grid scatter, label raster  (model/BERTgrid_generator.py:193-245,
 *          model/semantic_segmentation_head.py:314-341).  Bit-exact.
 * ------------------------------------------------------------------------------------------ */
/* boxes int32 [nbox,4] (x1,y1,x2,y2) for all docs, doc b owns boxes [box_off[b], box_off[b+1]).
 * owner[b,y,x] = GLOBAL index of the last box of doc b whose rectangle
 * rows int(y1/stride):int(y2/stride), cols int(x1/stride):int(x2/stride) (python slice clipping,
 * truncating division) covers the cell, else -1. */
int vbg_owner_map(const int* boxes, const int* box_off, int B, int gh, int gw, int stride, int* owner, void* stream);
/* grid[b,y,x,:] = emb[owner] or 0.  layout 0: NHWC [B,gh,gw,C]; 1: NCHW [B,C,gh,gw] (reference layout) */
int vbg_grid_scatter_fwd(const float* emb, const int* owner, int B, int gh, int gw, int C, int layout, float* grid,
                         void* stream);
/* demb[s,:] (+)= sum over cells owned by s of dgrid (CopySlices semantics); dgrid NHWC */
int vbg_grid_scatter_bwd(const float* dgrid, const int* owner, const int* boxes, const int* box_doc, int nbox, int gh,
                         int gw, int stride, int C, float* demb_accum, void* stream);
/* full-resolution labels from the stride-1 owner map: pos_neg (0 bg / 1 class>0 / 2 class==0), cls */
int vbg_label_raster(const int* owner, const int* seg_class, long long ncell, int* pos_neg, int* cls, void* stream);

/* ------------------------------------------------------------------------------------------
 * a6-a9, a11. convolution trunk helpers (NHWC): BatchNorm (Sync-able), max-pool, FPN resampling
 * ------------------------------------------------------------------------------------------ */
/* The two reductions below spread their fp64 partial sums over vbg_bn_slots() SLOT ROWS of 2*C doubles (same-address
 * atomics serialise; consumers fold the slots): `slots_accum` is [vbg_bn_slots()][2*C], zero on entry.  The folding entry
 * points take `clear_slots`: non-zero = zero the slot rows behind the read, so one persistent workspace serves every layer
 * without fill launches. */
int vbg_bn_slots(void);
/* per-channel sum / sum of squares over rows of x[M,C] (torch.nn.BatchNorm2d training statistics,
 * model/ResNetFPN_ViBERTgrid.py:116-123): slot[s][0..C) += sum, slot[s][C..2C) += sumsq */
int vbg_bn_stats(const float* x, long long M, int C, double* slots_accum, void* stream);
/* from sums over `count` rows held in `nslots` slot rows (nslots = 1: already folded, e.g. after a SyncBN all-reduce;
 * count_dev, if non-NULL, is a device scalar that overrides `count`: the all-reduced row count): mean, invstd;
 * running <- (1-mom)*running + mom*{mean, unbiased var} */
int vbg_bn_finalize(double* stats, int nslots, int clear_slots, double count, const double* count_dev, int C, float eps, float momentum,
                    float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
/* y = relu?( (x-mean)*invstd*gamma + beta (+ res) ) */
int vbg_bn_apply(const float* x, const float* res, long long M, int C, const float* mean, const float* invstd,
                 const float* gamma, const float* beta, int relu, float* y, unsigned* y_amax, void* stream);
/* y_amax (optional): amax slot (VBG_AMAX_WORDS words, zeroed by the caller) that receives the bit pattern of max |y|: the scale of y as an operand of
 * fp16-form products */
/* backward reductions: slot[s][0..C) += sum(g), slot[s][C..2C) += sum(g*xhat), g = dy*(y>0 if relu) */
int vbg_bn_bwd_reduce(const float* dy, const float* y, const float* x, long long M, int C, const float* mean,
                      const float* invstd, int relu, double* slots_accum, void* stream);
/* dx = gamma*invstd*(g - sum_g/count - xhat*sum_gx/count) from FOLDED sums[2*C]; dres = g (optional);
 * dgamma += sum_gx, dbeta += sum_g (optional) */
int vbg_bn_bwd_apply(const float* dy, const float* y, const float* x, long long M, int C, const float* mean,
                     const float* invstd, const float* gamma, const double* sums, double count, const double* count_dev,
                     int relu, float* dx,
                     float* dres, float* dgamma_accum, float* dbeta_accum, unsigned* dx_amax, void* stream);
/* dx_amax (optional): amax slot (VBG_AMAX_WORDS words, zeroed by the caller) that receives the bit pattern of max |dx| -- the scale of the fp16-form
 * products that consume dx */
/* vbg_bn_finalize + vbg_bn_apply, and vbg_bn_param_grad + vbg_bn_bwd_apply, as ONE launch each (round 5; torch.nn.BatchNorm2d training
 * forward / backward of model/ResNetFPN_ViBERTgrid.py:116-123 on one rank): every block folds the `nslots` slot rows of its 64 channels in
 * its prologue (fold order of the separate entry points: the same bits), the block of the first row chunk publishes mean / invstd / the
 * running statistics (forward) or adds the affine gradients (backward: dbeta += sum_g, dgamma += sum_gx).  C % 64 == 0.  The slot rows are
 * NOT cleared: hand in zeroed rows per use. */
int vbg_bn_apply_fold(const float* x, const float* res, long long M, int C, double* slots, int nslots, double count,
                      const double* count_dev, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                      float* running_var, const float* gamma, const float* beta, int relu, float* y, unsigned* y_amax, void* stream);
/* (count_dev, optional: a device scalar that overrides `count` -- SyncBatchNorm hands in the all-reduced [sum, sumsq, count] buffer as
 * slots with nslots = 1 and its last element as count_dev)
 * vbg_bn_fold_count: fold the slot rows into folded[0..2C) and put `count` (this rank's row count) into folded[2C]: the buffer of
 * torch.nn.SyncBatchNorm's forward all-reduce, from one launch */
int vbg_bn_fold_count(double* slots, int nslots, int clear_slots, int C, double* folded, double count, void* stream);
int vbg_bn_bwd_apply_fold(const float* dy, const float* y, const float* x, long long M, int C, const float* mean,
                          const float* invstd, const float* gamma, double* slots, int nslots, double count, int relu, float* dx,
                          float* dres, float* dgamma_accum, float* dbeta_accum, unsigned* dx_amax, void* stream);
/* fold `nslots` slot rows: folded[0..2C) = sum over slots (optional output), and (optional) the BatchNorm affine
   gradients from these LOCAL sums: dbeta += (float)folded[0..C), dgamma += (float)folded[C..2C)  (call before a SyncBN
   all-reduce of `folded`; torch.nn.SyncBatchNorm leaves weight/bias gradients per-rank for DDP to average,
   model/ResNetFPN_ViBERTgrid.py:196-206 `norm_layer`) */
int vbg_bn_param_grad(double* slots, int nslots, int clear_slots, int C, double* folded, float* dgamma_accum, float* dbeta_accum,
                      void* stream);
int vbg_maxpool3x3s2_fwd(const float* x, int B, int H, int W, int C, float* y, int* argmax, void* stream);
/* bwd: every dx element is WRITTEN (gather over the <= 4 windows that contain it; no atomics, no zero fill needed) */
int vbg_maxpool3x3s2_bwd(const float* dy, const int* argmax, int B, int Ho, int Wo, int C, int H, int W,
                         float* dx, void* stream);
/* nn.AvgPool2d(2, 2) of the ResNet-D projection shortcut (model/ResNetFPN_ViBERTgrid.py:222-236): x [B,H,W,C] ->
 * y [B,H/2,W/2,C] (floor); bwd: dx [B,H,W,C] = dy/4 over each 2x2 window, 0 on a dropped trailing row / column */
int vbg_avgpool2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream);
int vbg_avgpool2_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream);
/* y[b,y,x,:] = lo[b,y/2,x/2,:] + skip[b,y,x,:]   (nearest x2 upsample + add) */
int vbg_upsample2_add(const float* lo, const float* skip, int B, int H, int W, int C, float* y, void* stream);
/* lo[b,y,x,:] (+)= sum of the f x f block of hi   (backward of nearest upsampling by f) */
int vbg_sumpool(const float* hi, int B, int H, int W, int C, int f, float* lo, int accumulate, void* stream);
/* layout changes: [B,C,HW] <-> [B,HW,C] */
int vbg_nchw_to_nhwc(const float* x, int B, int C, int HW, float* y, void* stream);
int vbg_nhwc_to_nchw(const float* x, int B, int C, int HW, float* y, void* stream);
/* nearest-upsample a [B,h,w,C] NHWC map by f into NCHW [B,C,h*f,w*f] (eval-mode seg logits) */
int vbg_upsample_nhwc_to_nchw(const float* x, int B, int h, int w, int C, int f, float* y, void* stream);
int vbg_add_inplace(float* a, const float* b, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * a10. RoIAlign  (torchvision.ops.RoIAlign(7 or (h, w), 1/4, sampling_ratio=-1, aligned=False);
 *      model/grid_roi_align.py:37-41, 81).  feat NHWC [B,H,W,C]; boxes int32 image coords.
 * ------------------------------------------------------------------------------------------ */
int vbg_roi_align_fwd(const float* feat, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi,
                      int out, float scale, float* y /* [nroi,out,out,C] */, void* stream);
int vbg_roi_align_bwd(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi,
                      int out, float scale, float* dfeat_accum, void* stream);
/* rectangular bins: torchvision.ops.RoIAlign(output_size=(out_h, out_w)) -- upstream model/grid_roi_align.py:10-19 takes
 * output_size as an int or (H, W).  y [nroi,out_h,out_w,C].  The int entries above are these with out_h = out_w = out.  Backward:
 * separable form for out_h * out_w <= 64, out_h <= 8, out_w <= 32 (H, W <= 256), the per-tap atomic kernel otherwise. */
int vbg_roi_align_hw_fwd(const float* feat, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi,
                         int out_h, int out_w, float scale, float* y, void* stream);
int vbg_roi_align_hw_bwd(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi,
                         int out_h, int out_w, float scale, float* dfeat_accum, void* stream);

/* ------------------------------------------------------------------------------------------
 * a13. losses  (pipeline/custom_loss.py:35-101, 127-201)
 * ------------------------------------------------------------------------------------------ */
/* per-element CE.  Element i of the list is pixel/row e = elem ? elem[i] : i; its label is labels[e];
 * its logits row is e itself (H <= 0) or, for logits kept at 1/2^up_shift resolution of an
 * [*, H, W] label map, the low-resolution pixel under e (nearest upsampling folded into the index).
 * loss[i] = -w[t] * log_softmax(x)[t]. */
int vbg_ce_fwd(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n,
               const float* weight, int up_shift, int H, int W, float* loss, void* stream);
/* dlogits[row(e)] += g * w[t] * (softmax(x) - onehot(t)),  g = gmul * (gscale_dev ? *gscale_dev : 1) (atomic) */
int vbg_ce_bwd(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n,
               const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W,
               float* dlogits_accum, void* stream);
/* the same two with the element count in device memory: the first min(*n_dev, n_cap) elements of a list of capacity n_cap (the grid
 * is sized by n_cap); nothing at or beyond the count is read or written.  (The lists of vbg_sample_select / vbg_ohem_topk.) */
int vbg_ce_fwd_dyn(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n_cap,
                   const int* n_dev, const float* weight, int up_shift, int H, int W, float* loss, void* stream);
int vbg_ce_bwd_dyn(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n_cap,
                   const int* n_dev, const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W,
                   float* dlogits_accum, void* stream);
/* order-preserving compaction: out_idx = ascending i with (labels[i] == value) == eq; *out_count_dev = how many */
long long vbg_compact_ws_bytes(long long n);
int vbg_compact(const int* labels, long long n, int value, int eq, int* out_idx, int* out_count_dev, void* ws,
                long long ws_bytes, void* stream);
/* STABLE descending sort (LSD radix): keys_out sorted, idx_out[r] = original position of rank r */
long long vbg_sort_ws_bytes(long long n);
int vbg_sort_desc(const float* keys, long long n, float* keys_out, int* idx_out, void* ws, long long ws_bytes,
                  void* stream);
int vbg_gather_f32(const float* src, const int* idx, long long n, float* out, void* stream);
int vbg_gather_i32(const int* src, const int* idx, long long n, int* out, void* stream);
int vbg_sum_f32(const float* x, long long n, float* out_accum, void* stream);

/* ------------------------------------------------------------------------------------------
 * a12 (classifier_mode full / crf). row subsets and the linear-chain CRF
 * ------------------------------------------------------------------------------------------ */
/* dst[r,:] = src[idx[r],:]  /  dst[idx[r],:] += src[r,:]  : `fuse_embeddings[pred_pos_neg_mask]` and its backward
 * (model/field_type_classification_head.py:371, 389-395) */
int vbg_gather_rows(const float* src, const int* idx, long long n, int C, float* dst, void* stream);
int vbg_scatter_rows_add(const float* src, const int* idx, long long n, int C, float* dst_accum, void* stream);
/* CRF over `ndoc` documents whose segments are the row ranges doc_off[d]..doc_off[d+1] of emissions [N, ntag] (ntag <= 64,
 * trans[i*ntag + j] = score of j -> i, model/crf.py:33-46).  fwd: forward algorithm (:48-79) and gold path score (:81-97):
 * nll[d] = (log Z_d - score_d) / n_d (:147-151); alpha [N, ntag] and logz [ndoc] are kept for bwd, which writes
 * demissions [N, ntag] and accumulates dtrans [ntag, ntag], both scaled by gout[d].  viterbi (:99-145): best tag per row,
 * path score per document; backptr [N, ntag] is workspace. */
int vbg_crf_nll_fwd(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                    int start_tag, int stop_tag, float* alpha, float* logz, float* nll, void* stream);
int vbg_crf_nll_bwd(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                    int start_tag, int stop_tag, const float* alpha, const float* logz, const float* gout, float* demissions,
                    float* dtrans_accum, void* stream);
int vbg_crf_viterbi(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                    int stop_tag, int* backptr, int* path, float* score, void* stream);
/* Posterior of the same CRF, for the prediction path of the crf mode (reference model/field_type_classification_head.py:690-716
 * returns the Viterbi tags and no score): ONE launch gives, for all documents,
 *   path int32 [N], score [ndoc]   vbg_crf_viterbi's, bit for bit (the same additions, the same first maximum);
 *   logz [ndoc]                    log Z of model/crf.py:48-79;
 *   marginals [N, ntag]            p(y_t = i | x) = d logZ / d emissions[t, i]: a forward and a backward recursion in log space, both
 *                                  re-centred at every step (the maximum of the previous vector is taken out of the step's result and
 *                                  carried into logz in double), each row divided by its own sum at the end -- the error does not grow with
 *                                  the document's length (vbg_crf_nll_bwd keeps alpha and beta unnormalised: DESIGN.md, section 8).  The
 *                                  START and STOP columns are exact zeros (expf underflows on the -10000 entries).
 * ws: workspace of 2 * N * ntag 4-byte words (per row: ntag fp32 forward values, ntag int32 back pointers), contents undefined
 * afterwards.  An empty document writes score and logz (vbg_crf_viterbi's / vbg_crf_nll_fwd's values) and touches no row.  No
 * atomics: the same bits with and without the deterministic mode.  Emissions holding NaN or infinities are outside the contract. */
int vbg_crf_posterior(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                      int stop_tag, void* ws, int* path, float* score, float* logz, float* marginals, void* stream);
/* Log posteriors of a GIVEN tag path under the same CRF, row by row, for all documents in ONE launch: what a span confidence
 * P(y_s .. y_e = the path's tags | x) is added up from.  emissions, doc_off (device), trans and the START / STOP conventions are
 * vbg_crf_posterior's; path int32 [N] holds any tags in [0, ntag) -- the Viterbi path, a gold sequence, an alternative.
 *   lm [N]   lm[t] = log p(y_t = path[t] | x): from a_t + b_t with the row's own maximum and sum, vbg_crf_posterior's arithmetic for
 *            its row (expf / logf, tag order);
 *   lc [N]   lc[t] = log p(y_t = path[t] | y_{t-1} = path[t-1], x) for a row with a row of its document in front of it,
 *                  = trans[path[t]][path[t-1]] + (em_t[path[t]] + b_t[path[t]] - max_k(em_t[k] + b_t[k])) - b_{t-1}[path[t-1]],
 *            with b the backward vector re-centred at every step, b_{t-1}[j] = log sum_i exp(trans[i][j] + em_t[i] + b_t[i]) - the same
 *            maximum; lc of a document's first row is its lm.
 * So lm[s] + sum of lc[s+1 .. e] = log P(y_s .. y_e | x), and the sum of lc over a document = path score - log Z.  Every term is
 * of the size of an emission + a transition + log ntag: log Z is never formed and nothing grows with the row index.
 * ws: workspace of N * ntag 4-byte words (the forward vectors), contents undefined afterwards.  An empty document touches no row.  A
 * path entry outside [0, ntag) gives lm = lc = -INFINITY on its row and lc = -INFINITY on the next row of its document; it is compared
 * and clamped, never used as an address.  START / STOP in the path are legal and give values near -10000.  No atomics: the same
 * bits with and without the deterministic mode.  Emissions holding NaN or infinities are outside the contract.
 * Argument errors, before any launch: NULL doc_off / trans, ntag outside [1, 64], ndoc < 0, start_tag / stop_tag outside [0, ntag),
 * NULL emissions / path / ws / lm / lc with ndoc > 0 (the row count lies on the device).  ndoc == 0 is a no-op. */
int vbg_crf_path_logp(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                      int stop_tag, const int* path, void* ws, float* lm, float* lc, void* stream);
/* The training loss of the same CRF with a gradient whose error does not grow with the document's length (vbg_crf_nll_bwd forms every
 * marginal as exp(alpha + beta - logZ) from unnormalised vectors: DESIGN.md, section 8).  Documents, row ranges, trans, the -10000
 * initial vector and the START / STOP conventions are vbg_crf_nll_fwd's.  ONE launch for all documents gives
 *   logz [ndoc]                    log Z from a forward recursion in log space, re-centred at every step as vbg_crf_posterior's (the
 *                                  maxima taken out are summed in double);
 *   nll [ndoc]                     (float)((log Z - gold score) / n_d), gold score and quotient in double;
 * and, when both tables are given (both or neither: a loss-only call passes NULL twice and stores no vector), the gradient of
 * n_d * nll[d], that is at marginal scale:
 *   dem_unit [N, ntag]             p(y_t = i | x) - [tags[t] == i];
 *   dtrans_unit [ndoc, ntag, ntag] block d, entry [i, j]: sum_t p(y_{t-1} = j, y_t = i | x) with y_{-1} = START, plus on row
 *                                  i = STOP p(y_{n-1} = j | x), minus the gold path's transition counts.
 * The pairwise table of step t is built from the re-centred forward vector of t - 1, the transitions, the emission of t and the
 * re-centred backward vector of t; its own maximum is taken out before the exponentials and it is divided by its own sum.  The state
 * marginal of row t is the row sum of that table: rows of dem_unit + indicator sum to 1 by construction, and no term holds log Z or
 * anything that grows with t.  The tables are added up in double.  No workspace: the forward vectors wait in the rows of dem_unit.
 * n_d == 0: nll 0, logz vbg_crf_nll_fwd's value, no row touched, the dtrans_unit block zeros.  A tag outside [0, ntag) contributes no
 * indicator and no emission term, and the gold transitions into and out of it are skipped: that document's result is meaningless,
 * nothing faults.  No atomics: the same bits with and without the deterministic mode, and documents carry nothing into each other.
 * bwd, ONE launch: demissions[r, :] = (gout[d] / n_d) * dem_unit[r, :] over the rows of document d (out of place: the tables survive
 * a second backward) and dtrans_accum[k] += sum_d (gout[d] / n_d) * dtrans_unit[d, k], one thread per entry walking the documents in
 * increasing d, product and sum rounded separately; empty documents are skipped.
 * Argument errors: ntag outside [1, 64], start_tag / stop_tag outside [0, ntag), ndoc < 0, exactly one table NULL, a NULL required
 * pointer with ndoc > 0.  ndoc == 0 is a no-op.  Emissions holding NaN or infinities are outside the contract. */
int vbg_crf_nll_stable(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                       int start_tag, int stop_tag, float* nll, float* logz, float* dem_unit, float* dtrans_unit, void* stream);
int vbg_crf_nll_stable_bwd(const float* dem_unit, const float* dtrans_unit, const int* doc_off, int ndoc, int ntag,
                           const float* gout, float* demissions, float* dtrans_accum, void* stream);

/* ------------------------------------------------------------------------------------------
 * Field decoding of the returned class scores (csrc/decode.hip).  Replaces the per-segment loop every caller of the reference runs
 * over `pred_label` [N, C]: pipeline/train_val_utils.py:440-493 (with strcmp_tresh), eval_SROIE.py:119-169, eval_EPHOIE.py,
 * deployment/inference_SROIE.py:65-124, deployment/inference_EPHOIE.py:31-81 -- `.softmax(0)`, `.argmax(0)`, `.item()` per segment, the
 * grouping into runs of equal class, the mean score of every run and the best run of every class.  ONE launch, one workgroup per
 * document; document d owns the rows h_doc_off[d] .. h_doc_off[d + 1] of x.  `h_doc_off` is HOST memory (ndoc + 1 entries, not
 * decreasing, first >= 0), copied into the kernel arguments -- no device copy, no sync -- 512 documents to a launch.
 *   per row   p = softmax(x[i]) with vbg_row_softmax's arithmetic (same bits); cls[i] = first index of max p, score[i] = p[cls[i]];
 *             use_thresh != 0 and (double)score[i] < thresh: cls[i] = 0 (the comparison is made in double; the score stays);
 *   runs      maximal stretches of equal cls inside a document: (start, len, mean), start relative to the document's first row,
 *             mean = the fp64 sum of the run's scores / len -- the reference's sequential double sum bit for bit (every partial sum is
 *             exact for C <= 64 and fewer than 2^20 rows per document: csrc/decode.hip; both limits are argument errors beyond);
 *   filing    every run but the last under its own class; the last run under the class of the document's row n - 2 (the reference's
 *             `prev_class` quirk: the class of the run in front of it when it has a single row), under class C - 1 when n == 1;
 *   best      best[d * C + c] = the first filed record of class c, in filing order, with the strictly greatest mean;
 *             start = -1, len = 0, mean = 0 for a class without a record (every class of an empty document).
 * cls int32 [N], score fp32 [N] with N = h_doc_off[ndoc].  Rows holding NaN or infinities are outside the contract (their document's
 * records are meaningless; nothing faults).  No atomics on global memory: deterministic.  ndoc == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbg_decode_rec { int start; int len; double mean; } vbg_decode_rec;      /* 16 bytes */
int vbg_field_decode(const float* x, const int* h_doc_off, int ndoc, int C, int use_thresh, double thresh, int* cls, float* score,
                     vbg_decode_rec* best, void* stream);
/* The same table from the crf mode's outputs (vbg_crf_posterior's marginals [N, ntag] and path [N]) -- the loop above never had a
 * crf form: the reference's scripts allow only seqeval with the crf classifier, and its deployment loops read a [N, 1] tag column as
 * class 0 everywhere.  ONE launch, same row ranges, same vbg_decode_rec table [ndoc, C].  h_tag_class / h_tag_begin: HOST tables of ntag
 * ints, copied into the kernel arguments: tag -> class in [0, C), and 1 where the tag opens a new run even behind a row of its class.
 *   per row   c = tag_class[path[i]]; score[i] = the class posterior: the fp32 sum, in increasing tag order, of marginals[i, k] over the
 *             tags k with tag_class[k] == c; use_thresh != 0 and (double)score[i] < thresh: c = 0 (the score stays); cls[i] = c.
 *             A path entry outside [0, ntag) gives class 0 and score 0.
 *   runs      maximal stretches of equal cls; a row whose tag has tag_begin set starts a new run whatever its (thresholded) class;
 *   mean      every score enters as the integer rint((double)score * 2^30), added in 64 bits: mean = (double)sum / 2^30 / len, rounded
 *             once -- the same bits for any grouping of the additions (fewer than 2^20 rows per document);
 *   filing    EVERY run under its own class (the last-run quirk above belongs to a loop the crf mode never had);
 *   best      per class the largest mean, then the earliest start.  A run whose integer sum is 0 leaves no record.
 * Argument errors: ntag or C outside [1, 64], a class outside [0, C), a begin flag other than 0 / 1, 2^20 rows or more in a document,
 * NULL tables.  No atomics on global memory: deterministic.  ndoc == 0 is a no-op. */
int vbg_field_decode_tags(const float* marginals, const int* path, const int* h_doc_off, int ndoc, int ntag, int C,
                          const int* h_tag_class, const int* h_tag_begin, int use_thresh, double thresh, int* cls, float* score,
                          vbg_decode_rec* best, void* stream);
/* EVERY run of every document instead of the winners -- a page with dozens of `question` / `answer` entities has dozens of runs per
 * class.  Rows, cls, score, the threshold in double, run heads (a class change; in the tags form also a begin tag) and run means are
 * vbg_field_decode's / vbg_field_decode_tags's, the means bit for bit; the limits (C and ntag <= 64, fewer than 2^20 rows per
 * document, HOST h_doc_off, 512 documents to a launch) and the argument errors are theirs too.
 *   runs [N]  one vbg_run_rec per ROW.  The record at a run's first row holds the run: start (relative to the document), len, cls,
 *             mean, logp; every other row's record has len == 0 (all fields 0).  The records with len > 0 are the document's runs in
 *             row order.  Each record has exactly one writer: nothing depends on scheduling.
 *   filing    every run under its OWN class, the last one included, in both forms (the `prev_class` quirk is the winner loop's);
 *             class-0 runs and, in the tags form, runs whose integer sum is 0 are listed as well.
 *   logp      tags form: lm[s] + the fp64 sum of lc[s+1 .. e] over the run's rows s .. e, with lm / lc vbg_crf_path_logp's for the
 *             same path: log P(y_s .. y_e = the path's tags | x).  Taken as a difference of fp64 prefix sums: equal to the
 *             sequential sum within ~1e-9.  -INFINITY or NaN in lm / lc make their document's logp meaningless; nothing faults.
 *             Scores form: 0.0.
 * A call without rows (ndoc == 0, or only empty documents) launches nothing and needs no buffer.  NULL x / cls / score / runs -- and in
 * the tags form path / lm / lc -- with rows present is an argument error. */
typedef struct vbg_run_rec { int start; int len; int cls; int pad; double mean; double logp; } vbg_run_rec;   /* 32 bytes */
int vbg_field_runs(const float* x, const int* h_doc_off, int ndoc, int C, int use_thresh, double thresh, int* cls, float* score,
                   vbg_run_rec* runs, void* stream);
int vbg_field_runs_tags(const float* marginals, const int* path, const float* lm, const float* lc, const int* h_doc_off, int ndoc,
                        int ntag, int C, const int* h_tag_class, const int* h_tag_begin, int use_thresh, double thresh, int* cls,
                        float* score, vbg_run_rec* runs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation counts of `validate` (csrc/metrics.hip): what pipeline/criteria.py's token_F1_criteria, token_classification_criteria and
 * BIO_F1_criteria (seqeval, default mode) need from a forward -- a few dozen integers -- counted where the scores lie.  ONE launch, one
 * workgroup per sequence; sequence d owns the rows h_doc_off[d] .. h_doc_off[d + 1].  `h_doc_off` is HOST memory (ndoc + 1 entries, not
 * decreasing, first >= 0), copied into the kernel arguments as vbg_field_decode does -- 512 sequences to a launch.  Exactly one of
 *   scores    fp32 [N, C] row-major: the predicted class of a row is the first index of its largest raw score;
 *   pred_tags int32 [N]: the predicted class itself (the crf head returns tags)
 * is given, the other is NULL.  gt int32 [N].  A row whose gt -- or pred_tags entry -- lies outside [0, C) counts nowhere: it indexes
 * nothing, it is left out of the token tables and both of its tags read `O` in the entity walk.
 * `counts` is device memory of VBG_METRICS_COUNTS(T, C) 64-bit integers, which the launch ADDS to (64-bit integer atomics: sums of
 * integers, exact and the same for every schedule, so the deterministic mode needs no other form):
 *   counts[VBG_METRICS_ENT(T, C)  + ty * 3 + {0, 1, 2}]   entities of type ty: in gt (n_true), predicted (n_pred), in both (n_correct);
 *   counts[VBG_METRICS_CONF(T, C) + g * C + p]            rows with gt class g and predicted class p;
 *   counts[VBG_METRICS_TOK(T, C)  + c * 4 + {0, 1, 2, 3}] token_F1_criteria's literal TP, TN, FP, FN of class c, with scores only:
 *             v = the row's score of class c truncated toward zero (`pred_label.int()`); TP: gt == c and v == 1, FN: gt == c and v == 0,
 *             FP: gt != c and v == 1, TN: gt != c and v == 0; any other v, NaN included, counts nowhere.
 * Entities (T >= 1; T == 0: no tag table, the entity block is empty): class k carries the tag letter tags.prefix[k] (VBG_TAG_*) and the
 * type tags.type[k] in [0, T).  seqeval's get_entities: with (pt, pty) the tag of the row in front (`O` in front of row 0) and a
 * virtual `O` row behind the last,
 *   end(i)   = pt in {E, S}  or  (pt in {B, I} and t in {B, S, O})  or  (pt != O and pty != ty);     the entity in front of i is closed
 *   start(i) = t in {B, S}   or  (pt in {E, S, O} and t in {E, I})  or  (t != O and pty != ty);      an entity begins at i
 * an entity is (type, begin, last row); n_correct counts the entities of gt that the prediction holds with the same three values.
 * Sequences carry nothing into each other.  Argument errors, before any launch: C outside [1, 64], T outside [0, 64], a table entry
 * outside its range, both or neither of scores / pred_tags, negative or decreasing offsets, NULL gt with rows, NULL counts with
 * ndoc > 0.  ndoc == 0 and empty sequences count nothing.
 * ------------------------------------------------------------------------------------------ */
#define VBG_METRICS_MAX_C 64
#define VBG_METRICS_MAX_T 64
#define VBG_TAG_O 0
#define VBG_TAG_B 1
#define VBG_TAG_I 2
#define VBG_TAG_E 3
#define VBG_TAG_S 4
#define VBG_METRICS_ENT(T, C) 0
#define VBG_METRICS_CONF(T, C) (3 * (T))
#define VBG_METRICS_TOK(T, C) (3 * (T) + (C) * (C))
#define VBG_METRICS_COUNTS(T, C) (3 * (T) + (C) * (C) + 4 * (C))
typedef struct vbg_tag_table { unsigned char prefix[VBG_METRICS_MAX_C]; unsigned char type[VBG_METRICS_MAX_C]; } vbg_tag_table;
int vbg_seq_metrics(const float* scores, const int* pred_tags, const int* gt, const int* h_doc_off, int ndoc, int C, int T,
                    vbg_tag_table tags, long long* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * a13b. sampling and hard-example selection on the device  (csrc/sample.hip)
 *
 * vbg_sample_select replaces, for up to four label categories of one label array, the reference's `ce_loss[mask]` compaction plus
 * `random.sample(range(n), k)` (pipeline/custom_loss.py:62-88 CrossEntropyLossRandomSample, :143-163 the `random` pre-sample of
 * CrossEntropyLossOHEM) without the host knowing n.  Category c = {i : (labels[i] == value_c) == (eq_c != 0)}, n_c elements,
 * keep_c = min(k_c, n_c).  The key of element i is rng_u64(seed, stream0 + c, i) (vbg_common.h; distinct for distinct i).
 *   n_c >  k_c : the k_c elements of the category with the smallest keys, written in ascending key order -- a uniformly random ordered
 *                sample (take_order_c == 0: the same k_c elements; their order is unspecified but a function of the inputs alone);
 *   n_c <= k_c : every element, in ascending element index.
 * out_idx[off_c ... off_c + keep_c), off_c = k_0 + ... + k_{c-1}; slots beyond keep_c are not written.  out_keep[c] = keep_c,
 * out_n[c] = n_c (device memory).  Exact and deterministic for every input: a function of (labels, cats, seed, stream0) alone.  No host
 * read, three launches.  Integer atomics only where their order cannot show (histogram sums, slot claims of a set that is sorted later).
 * N < 2^31, 1 <= ncat <= 4, 1 <= k_c <= 4096; ws >= vbg_sample_ws_bytes(N, ncat, ksum) bytes (a function of N and the k's only).
 * ------------------------------------------------------------------------------------------ */
#define VBG_SAMPLE_MAX_CATS 4
#define VBG_SAMPLE_MAX_K 4096
typedef struct vbg_sample_cat { int value; int eq; int k; int take_order; } vbg_sample_cat;
typedef struct vbg_sample_cats { vbg_sample_cat c[VBG_SAMPLE_MAX_CATS]; } vbg_sample_cats;
long long vbg_sample_ws_bytes(long long N, int ncat, long long ksum);
int vbg_sample_select(const int* labels, long long N, int ncat, vbg_sample_cats cats, unsigned long long seed,
                      unsigned long long stream0, int* out_idx, int* out_keep, int* out_n, void* ws, long long ws_bytes, void* stream);
/* vbg_ohem_topk: CrossEntropyLossOHEM's hard-example choice for ncat bounded lists in one launch, one workgroup per list
 * (pipeline/custom_loss.py:165-190: per-element CE of the category, `torch.sort(descending=True)`, `sorted_loss[sorted_index[:k]]`).
 * List c is elem[off_c ... off_c + m_c), off_c = cap_0 + ... + cap_{c-1} (vbg_sample_select's layout with k = cap), m_c =
 * min(m_dev[c], cap_c); its losses are vbg_ce_fwd's, bit for bit.  keep_c = min(m_c, k_c).  keep_c < m_c: si = the list's positions
 * ordered by (loss descending, position ascending) in the total order of vbg_sort_desc's radix keys (the NaN of an out-of-range label
 * first; every zero loss is +0); out[off_c + r] = elem[off_c + si[si[r]]] for r < keep_c -- the reference's quirk, literally.
 * Otherwise the list is copied through.  out_keep[c] = keep_c.  1 <= ncat <= 4, 1 <= cap_c <= 4096, k_c >= 1. */
typedef struct vbg_ohem_cat { int cap; int k; } vbg_ohem_cat;
typedef struct vbg_ohem_cats { vbg_ohem_cat c[VBG_SAMPLE_MAX_CATS]; } vbg_ohem_cats;
int vbg_ohem_topk(const float* logits, long long ld, int ncls, const int* elem, const int* m_dev, int ncat, vbg_ohem_cats cats,
                  const int* labels, const float* weight, int up_shift, int H, int W, int* out, int* out_keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * a15. optimizers on flat fp32 ranges  (torch.optim.SGD / AdamW; train_SROIE.py:223-235)
 * ------------------------------------------------------------------------------------------ */
int vbg_sgd_step(float* p, const float* g, float* mom, long long n, float lr, float momentum, float wd,
                 int first_step, float grad_scale, void* stream);
int vbg_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                   float eps, float wd, int step, float grad_scale, void* stream);
/* Weight averaging over a flat range (EMA / SWA; vbg.optim.WeightAverage): avg[i] <- lerp(avg[i], p[i], weight), torch's statement
 * (ATen/native/Lerp.h) and torch's bits on gfx950: d = p - a (rounded); |weight| < 0.5: fma(weight, d, a), otherwise fma(-d, 1 - weight, p)
 * with 1 - weight rounded to fp32 first -- each branch's product and sum in one rounding.  One whole-range launch, 12 B per element,
 * float4 access when both pointers are 16-byte aligned (all-scalar otherwise), no atomics.  avg and p must not overlap.  n == 0 is a
 * no-op that looks at no pointer; n < 0 or a NULL pointer with n > 0 is an argument error (-1). */
int vbg_lerp(float* avg, const float* p, long long n, float weight, void* stream);
/* In-place exchange of a[0, n) and b[0, n) as bit patterns (NaN payloads, -0.0 and denormals included): every element is read and
 * written by the one thread that owns it, 16 B per element, no temporary.  Same alignment rule and n == 0 / NULL / n < 0 cases as
 * vbg_lerp; a == b or overlapping ranges is an argument error (-1). */
int vbg_swap(float* a, float* b, long long n, void* stream);
/* The same two steps with per-group hyper-parameters (torch param groups) in ONE launch.  `chunks` (device memory, 16-byte
 * aligned) lists the work: chunk k updates elements [start, start + length) with the hyper-parameters of groups[group]; start and
 * length are multiples of 4 elements, chunks do not overlap, and p / g / mom / m / v are 16-byte aligned.  Blocks stride over
 * the chunks, so the host bounds the work per block by cutting every run of equal group into chunks of a bounded length.
 * `groups` is HOST memory (1 <= ngroups <= VBG_OPTIM_MAX_GROUPS), copied into the kernel arguments: no device copy, no sync.
 * Elements no chunk covers are neither read nor written.  first_step / step / grad_scale are shared by all groups; the AdamW
 * bias corrections 1 - b^step are formed per group in double, as vbg_adamw_step forms them.  nchunks == 0 is a no-op. */
#define VBG_OPTIM_MAX_GROUPS 32
typedef struct { long long start; int length; int group; } vbg_optim_chunk;
typedef struct { float lr, momentum, wd; } vbg_sgd_group;
typedef struct { float lr, b1, b2, eps, wd; } vbg_adamw_group;
int vbg_sgd_step_seg(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                     const vbg_sgd_group* groups, int ngroups, int first_step, float grad_scale, void* stream);
int vbg_adamw_step_seg(float* p, const float* g, float* m, float* v, const vbg_optim_chunk* chunks, int nchunks,
                       const vbg_adamw_group* groups, int ngroups, int step, float grad_scale, void* stream);
/* The segmented steps with the rest of torch.optim's rule per group (torch 2.10, single-tensor paths), for stock torch.optim.SGD /
 * Adam / AdamW objects stepped through vbg.optim.fuse.  Same chunk table and buffer contract as above.
 *   SGD:  g' = (maximize ? -g : g) * grad_scale + wd * p;  momentum != 0: buf = first ? g' : momentum * buf + (1 - dampening) * g';
 *         d = nesterov ? g' + momentum * buf : buf (momentum 0: d = g');  p -= lr * d.  Chunks of momentum-0 groups neither read nor
 *         write `mom`, which may be NULL when every group has momentum 0.
 *   Adam: g' = (maximize ? -g : g) * grad_scale;  coupled: g' += wd * p, else p *= 1 - lr * wd;  moments as vbg_adamw_step;  amsgrad:
 *         vmax = max(vmax, v) and vmax stands under the square root.  Bias corrections from the GROUP's step (>= 1), in double.  `vmax`
 *         is read and written only in chunks of amsgrad groups; NULL is accepted when no group has the flag, an argument error otherwise.
 * A group without flags (beyond `first`), with dampening 0 (and momentum != 0) is updated by the statements of the whole-range steps:
 * same bits as vbg_sgd_step / vbg_adamw_step, and as vbg_sgd_step_seg / vbg_adamw_step_seg, which are this case of the same launch. */
typedef struct { float lr, momentum, dampening, wd; int flags; } vbg_sgd_group_opt;
    /* flags: 1 nesterov, 2 maximize, 4 first (no momentum buffer yet) */
typedef struct { float lr, b1, b2, eps, wd; int step; int flags; } vbg_adam_group_opt;
    /* flags: 1 amsgrad, 2 maximize, 4 coupled weight decay (torch.optim.Adam / decoupled_weight_decay=False) */
int vbg_sgd_step_seg_opt(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                         const vbg_sgd_group_opt* groups, int ngroups, float grad_scale, void* stream);
int vbg_adam_step_seg_opt(float* p, const float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                          const vbg_adam_group_opt* groups, int ngroups, float grad_scale, void* stream);
/* The same two steps under torch.amp.GradScaler's protocol for optimizers that declare _step_supports_amp_scaling: the scale and the
 * inf flag are fp32 scalars in DEVICE memory, read by the kernel -- no host sync, no separate unscale pass.  found_inf (required):
 * non-zero makes the whole launch a no-op, p / g / every state array left as they were.  grad_scale (NULL: the caller unscaled the
 * gradients already): g' = g * inv with inv = (float)(1.0 / (double)*grad_scale), a product rounded on its own and stored back to g;
 * the rule then runs on g' with grad_scale 1, in the statements of the *_seg_opt entries (same bits as those on the same g').  With
 * NULL g is not written.  Everything else -- table, groups, optional buffers, argument errors -- as vbg_sgd_step_seg_opt /
 * vbg_adam_step_seg_opt. */
int vbg_sgd_step_seg_amp(float* p, float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                         const vbg_sgd_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf, void* stream);
int vbg_adam_step_seg_amp(float* p, float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                          const vbg_adam_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf, void* stream);
/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm type 2) without a host sync and without a pass of its own over the
 * gradients: a norm pass over the chunk table the step will walk, a one-block finish that leaves the norm and torch's coefficient in
 * device memory, and the step entries below, which read the coefficient as the *_amp entries read the scale.  The library has one
 * row pass with three entries (vbg_grad_sumsq_seg, vbg_grad_sumsq_seg_inf, vbg_grad_norm_seg) and one finish with two (vbg_clip_coef,
 * vbg_clip_coef_gate).
 * vbg_grad_sumsq_seg: the row pass for squares, without flag or gate.  partials[c] = sum of g[start .. start + length)^2 of row c, c in [0, nchunks) -- a plain store per row (no
 *   atomics, nothing to zero, the same bits on every call), summed per thread over its float4s and then over the block, in fp32.
 *   Same table and alignment contract as the segmented steps; the group field is ignored, what no row covers is not read, nchunks == 0
 *   is a no-op.  partials is device memory of >= nchunks floats.
 * vbg_clip_coef: the finish for squares, without a gate.  One block sums partials[0 .. n) in double in a fixed order (partials of several tables side by side: one norm over
 *   several optimizers) and writes out[0] = total = (float)sqrt(sum) * norm_scale [* (float)(1.0 / (double)*grad_scale) when grad_scale,
 *   a device scalar, is given: the gradients still hold scaled values] and out[1] = the coefficient in fp32 as torch forms it:
 *   c = (1 / (total + 1e-6f)) * max_norm (torch evaluates `max_norm / tensor` as reciprocal times scalar), out[1] = c > 1 ? 1 : c --
 *   a NaN norm gives NaN, an inf norm 0, n == 0 gives (0, 1).  out: 2 floats of device memory; nothing is stored behind them.
 * vbg_sgd_step_seg_clip / vbg_adam_step_seg_clip: the *_amp entries with clip_coef (device scalar, required; out + 1 above), found_inf
 *   optional (NULL: no scaler) and the host float of the *_seg_opt entries (host_scale, applied inside the rule).  Per chunk, before the
 *   rule: g' = (g * inv) * coef, inv as in the *_amp entries (1 without grad_scale), each product rounded on its own, stored back to g
 *   -- what torch's unscale_ and clip leave in .grad.  With coef == 1.0f and grad_scale NULL g is not written (the products would be g).
 *   found_inf non-zero: the launch does nothing.  keep_mom != 0 (SGD): momentum-0 groups write `mom` as in vbg_sgd_step_seg, which is
 *   then required; with it, groups without flags reproduce vbg_sgd_step_seg on the clipped gradient bit for bit. */
int vbg_grad_sumsq_seg(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, void* stream);
int vbg_clip_coef(const float* partials, int n, float max_norm, float norm_scale, const float* grad_scale, float* out, void* stream);
int vbg_sgd_step_seg_clip(float* p, float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                          const vbg_sgd_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf,
                          const float* clip_coef, float host_scale, int keep_mom, void* stream);
int vbg_adam_step_seg_clip(float* p, float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                           const vbg_adam_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf,
                           const float* clip_coef, float host_scale, void* stream);
/* torch.amp.GradScaler's own pass over the gradients (GradScaler._unscale_grads_: a loop over every parameter and several
 * _amp_foreach_non_finite_check_and_unscale_ launches per optimizer and step) on the row walk above, for gradients that are views of one
 * flat buffer (vbg.optim.fuse_scaler).  Same table and alignment contract as vbg_grad_sumsq_seg: the group field is ignored, what no row
 * covers is neither read nor written, nchunks == 0 is a no-op.  found_inf and inv_scale are device scalars, required (also with
 * nchunks == 0) and 4-byte aligned.  found_inf is only ever SET: *found_inf = 1.0f when a covered element is inf or NaN (a plain store
 * of the same value from every block that saw one: no atomics, the same code in deterministic mode), left alone otherwise -- the caller
 * hands in a zero, as torch's op expects.
 * vbg_grad_unscale_check_seg: that torch op over the rows.  *inv_scale == 1.0f (GradScaler._check_inf_per_device): g is only read,
 *   4 B per element.  Otherwise every covered element becomes g * *inv_scale, one rounded fp32 product, non-finite elements included
 *   (as torch stores them): 8 B per element.
 * vbg_grad_sumsq_seg_inf: the row pass for squares (the partials of vbg_grad_sumsq_seg, bit for bit) with the per-element test in its loop.  The flag comes from
 *   the elements, not from the sums: finite gradients whose squares overflow leave an inf partial and no flag. */
int vbg_grad_unscale_check_seg(float* g, const vbg_optim_chunk* chunks, int nchunks, const float* inv_scale, float* found_inf, void* stream);
int vbg_grad_sumsq_seg_inf(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, float* found_inf, void* stream);
/* The norm pass and the finish above for norm types 2, 1 and inf, with the reference's loss gate (`if train_loss > loss_clip_tresh:`,
 * pipeline/train_val_utils.py:281) taken on the device: vbg.optim.clip_in_step(norm_type=..., when=(loss, threshold)).
 * kind: 2 (L2), 1 (L1) or 0 (inf norm).  The gate: gate_loss is a device scalar, fp64 when gate_f64 == 1 (8-byte aligned), fp32 when
 * gate_f64 == 0 (4-byte aligned); it is open when *gate_loss > gate_threshold, compared in that dtype -- fp32 against
 * (float)gate_threshold, which is what torch compares an fp32 tensor with; strictly greater: a NaN loss closes it, +inf opens it.
 * gate_loss NULL: no gate.  The loss is read by the kernels (one load, uniform over the launch), never by the host.
 * vbg_grad_norm_seg: the row pass with every argument it has: table, alignment contract and row walk of vbg_grad_sumsq_seg; a plain store
 *   per row.  kind 2: partials[c] as vbg_grad_sumsq_seg leaves it, bit for bit (with found_inf: as vbg_grad_sumsq_seg_inf does).  kind 1: partials[c] = sum of |g| over row c, summed the same way (per thread over its
 *   float4s, then over the block, in fp32).  kind 0: partials[c] = max |g| of row c, exact; a NaN anywhere in the row gives a NaN,
 *   +-inf gives +inf.  found_inf (optional, 4-byte aligned): the per-element test of vbg_grad_sumsq_seg_inf, for any kind.  With a gate
 *   that is closed and found_inf NULL every block returns before it touches g or partials; with found_inf the rows always walk.
 * vbg_clip_coef_gate: the finish with every argument it has; one block.  Gate closed: out = (0, 1, 0) and no partial is read.  Otherwise total = (float)sqrt(sum in double)
 *   (kind 2), (float)(sum in double) (kind 1) or the maximum of the partials with a NaN kept (kind 0), then the statements of
 *   vbg_clip_coef (norm_scale, the inverse grad_scale, the coefficient), and out = (total, coefficient, 1).  n == 0: (0, 1, gate).
 *   out: 3 floats of device memory; out + 1 is what the *_seg_clip entries take. */
int vbg_grad_norm_seg(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, int kind, float* found_inf,
                      const void* gate_loss, int gate_f64, double gate_threshold, void* stream);
int vbg_clip_coef_gate(const float* partials, int n, int kind, float max_norm, float norm_scale, const float* grad_scale,
                       const void* gate_loss, int gate_f64, double gate_threshold, float* out, void* stream);
/* out[0] += sum(g^2) */
int vbg_sumsq(const float* g, long long n, float* out_accum, void* stream);
int vbg_scale_inplace(float* x, long long n, float s, void* stream);
/* Per-parameter statistics of a flat fp32 buffer (vbg.stats.ParamStats; csrc/stats.hip): one row pass per buffer and one finish,
 * no atomics on device memory, plain stores in a fixed order -- the same bits on every call, the same code in deterministic mode.
 * vbg_param_stats_rows: `rows` is a device table of vbg_optim_chunk whose `group` is the PARAMETER index.  Where the contract differs
 *   from the optimizer tables: start is a multiple of 4 elements, length is any value in [1, 2^31 - 4] and covers the parameter's own elements
 *   only (never its slot padding), rows of one parameter are consecutive and in address order.  The last float4 of a row is read whole
 *   (slots are padded to 8 elements, so the read is legal); lanes at or beyond `length` enter no statistic, whatever they hold.
 *   scale_or_null: GradScaler's device scale; inv = (float)(1.0 / (double)*scale), and every element is classified and summed as the
 *   one rounded fp32 product x * inv.  NULL: the element itself.  x is only ever read.  recs[c] (c in [0, nrows)) is one record:
 *     sumsq      sum of (double)v * (double)v over the FINITE elements (each product is exact in double)
 *     amax_bits  the largest bit pattern of |v| among finite elements, 0 if none
 *     nonfinite  count of inf and NaN;  zeros: count of +0 / -0
 *     over_f16   finite elements with |v| >= 65520.0f (what an fp16 piece turns into inf)
 *     hist       binades of the finite non-zero elements: e = unbiased fp32 exponent (fp32 subnormals: -127),
 *                bin = clamp(e + 46, 0, 63) -- bin k in 1..62: 2^(k-46) <= |v| < 2^(k-45); bin 0: below 2^-45; bin 63: from 2^17 up.
 *                |v| < 2^-14 (fp16 subnormal range) is bins 0..31, |v| < 2^-25 (rounds to zero in fp16) is bins 0..20.
 *   nrows == 0 is a no-op that looks at no pointer.
 * vbg_param_stats_finish: row_ptr is int[nparams + 1] in device memory, a CSR over the rows.  One block per parameter sums that
 *   parameter's records in a fixed order (a lane-strided walk, then a fixed tree), writes last[p] (this update) and, unless total is
 *   NULL, folds it into total[p]: counts and bins add (int64), amax_bits takes the max, sumsq is the last value, updates += 1,
 *   steps_nonfinite += (nonfinite > 0).  nparams == 0 is a no-op that looks at no pointer.
 * Argument errors (-1, before any launch): a negative count, a NULL required pointer with a positive count, x / rows / recs / last
 * not 16-byte aligned, total not 8-byte or row_ptr / scale not 4-byte aligned. */
typedef struct vbg_stats_rec {                                    /* 288 bytes, 16-byte aligned in device memory */
    double sumsq;
    unsigned int amax_bits;
    int nonfinite, zeros, over_f16;
    int hist[64];
    int pad[2];
} vbg_stats_rec;
typedef struct vbg_stats_total {                                  /* 568 bytes, 8-byte aligned */
    double sumsq;
    long long nonfinite, zeros, over_f16, updates, steps_nonfinite;
    unsigned int amax_bits;
    int pad;
    long long hist[64];
} vbg_stats_total;
int vbg_param_stats_rows(const float* x, const vbg_optim_chunk* rows, int nrows, const float* scale_or_null, vbg_stats_rec* recs,
                         void* stream);
int vbg_param_stats_finish(const vbg_stats_rec* recs, const int* row_ptr, int nparams, vbg_stats_rec* last, vbg_stats_total* total,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * a16. deterministic mode (vbg.ops.set_deterministic): fixed-order forms of the float-atomic reductions (DESIGN.md
 * "Deterministic mode").  Two launches on the same inputs return the same bits.
 * ------------------------------------------------------------------------------------------ */
/* out[c] (+)= sum over rows of x[r][c] in fp64, rows in fixed chunks; ws: vbg_colsum_det_ws_elems(M, N) doubles */
long long vbg_colsum_det_ws_elems(long long M, int N);
int vbg_colsum_det(const float* x, long long ld, long long M, int N, float* out, int accumulate, double* ws, void* stream);
/* out[0] += sum(x) (squares = 0) or sum(x^2) (squares = 1); ws: vbg_sum_det_ws_elems() floats */
int vbg_sum_det_ws_elems(void);
int vbg_sum_det(const float* x, long long n, int squares, float* out_accum, float* ws, void* stream);
/* stable ascending sort of int keys -> sorted keys and their source positions; ws: vbg_sort_i32_ws_bytes(n) bytes */
long long vbg_sort_i32_ws_bytes(long long n);
int vbg_sort_i32(const int* keys, long long n, int* keys_out, int* idx_out, void* ws, long long ws_bytes, void* stream);
/* dst[key][0..C) += sum of src[perm[k]][0..C) over each run of equal sorted keys, in sorted order (keys < 0 skipped) */
int vbg_segment_rows_add(const float* src, long long lds, const int* perm, const int* sorted_keys, long long n, int C,
                         float* dst_accum, long long ldd, void* stream);
/* CE backward per element: grow[i][0..ncls) = its gradient row, keys[i] = its logits row (-1: label out of range); the rows are
 * then added by vbg_sort_i32 + vbg_segment_rows_add */
int vbg_ce_bwd_rows(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n,
                    const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W, float* grow, int* keys,
                    void* stream);
/* ... with the count in device memory (vbg_ce_bwd_dyn's deterministic form): slots at and beyond *n_dev are not read, their rows are
 * zero with key -1 */
int vbg_ce_bwd_rows_dyn(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n_cap,
                        const int* n_dev, const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W,
                        float* grow, int* keys, void* stream);
/* RoIAlign backward, one owner per feature row: RoIs added in RoI order (out <= 8, out * W * 4 <= 48 KB) */
int vbg_roi_align_bwd_det(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi, int out,
                          float scale, float* dfeat_accum, void* stream);
/* the same for (out_h, out_w) bins (upstream model/grid_roi_align.py:10-19): 1 <= out_h, out_w <= 32, out_w * W * 4 <= 48 KB of LDS */
int vbg_roi_align_hw_bwd_det(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi, int out_h,
                             int out_w, float scale, float* dfeat_accum, void* stream);
/* BatchNorm reductions: one partials row per row block (ws: vbg_bn_det_ws_rows(M, C) rows of 2C doubles, plain stores), the rows
 * added in block order into slot row 0 of zero_slots (which must be zero) */
int vbg_bn_det_ws_rows(long long M, int C);
int vbg_bn_stats_det(const float* x, long long M, int C, double* ws, double* zero_slots, void* stream);
int vbg_bn_bwd_reduce_det(const float* dy, const float* y, const float* x, long long M, int C, const float* mean,
                          const float* invstd, int relu, double* ws, double* zero_slots, void* stream);
/* embedding LayerNorm backward: dz_rows [ntok][hidden], part [vbg_embed_ln_bwd_det_blocks(ntok)][3][hidden] = per-block
 * (dgamma, dbeta, dtype0) partials */
int vbg_embed_ln_bwd_det_blocks(int ntok);
int vbg_embed_ln_bwd_det(const float* dout, const float* xhat, const float* rstd, int ntok, int hidden, const float* gamma,
                         float drop_p, unsigned long long seed, unsigned long long sid, float* dz_rows, float* part, void* stream);
/* CRF backward: dtrans_part [ndoc][ntag * ntag] (zeroed: an empty document writes nothing) instead of dtrans += */
int vbg_crf_nll_bwd_det(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                        int start_tag, int stop_tag, const float* alpha, const float* logz, const float* gout, float* demissions,
                        float* dtrans_part, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VBG_H */
