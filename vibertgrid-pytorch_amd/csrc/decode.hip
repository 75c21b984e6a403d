// Field decoding of the returned class scores: what every caller of the reference does with `pred_label` [N, C] one segment at a
// time (pipeline/train_val_utils.py:440-493, eval_SROIE.py:119-169, eval_EPHOIE.py, deployment/inference_SROIE.py:65-124,
// deployment/inference_EPHOIE.py:31-81) -- softmax, argmax, threshold, grouping into runs of equal class, the fp64 mean score of every
// run and the best run of every class -- in ONE launch, one 256-thread workgroup per document.  The strings stay on the host
// (vbg/decode.py joins them for the winning runs only).
//
// The document is walked in chunks of 256 rows, one row per thread, with four barriers per chunk (field_runs_kernel, the listing of
// EVERY run, walks the same chunks and keeps no winner tables):
//   rows      each thread forms its row's softmax with the helper row_softmax_kernel uses (vbg_common.h: same bits), takes the first
//             index of the largest probability and applies the threshold in DOUBLE (the reference compares two Python floats);
//   run heads a row whose left neighbour has another class starts a run.  Wave ballots give every head the head in front of it;
//   run sums  P = the prefix sum of the scores in fp64 (wave scan + wave totals + the carry of the chunks before); the run between two
//             consecutive heads h1 < h2 has the sum P(h2 - 1) - P(h1 - 1), and the head h2 files it under the class of row h2 - 1;
//   winner    per class, in LDS only: a 64-bit max over the bit pattern of the mean (positive doubles order like their bit patterns),
//             a barrier, a 64-bit min over (start << 20 | len) among the runs that equal it, a barrier, and one thread per class folds
//             the chunk's winner into the running one (strictly greater only: earlier chunks hold earlier runs).
// Scores live in registers for the one chunk that needs them; nothing the block wrote is read back.  No global atomics, no
// cross-block traffic: the result does not depend on scheduling, with or without the deterministic mode.
//
// WHY THE ORDER OF THE SUMS DOES NOT MATTER.  The reference adds a run's scores one after the other in double.  A score is
// expf(0) * (1 / s) = the fp32 value 1 / s, where s is the fp32 sum of C <= 64 terms expf(x - max) in (0, 1], one of them expf(0) == 1:
// 1 <= s <= 64, so the score lies in [2^-7, 1] and is a multiple of 2^-30 (fp32 keeps 24 bits below its leading one).  A sum of fewer
// than 2^20 such scores is a multiple of 2^-30 below 2^20: at most 50 bits, which a double holds exactly.  Hence every partial sum the
// reference forms is exact, every prefix sum P is exact, the difference of two prefix sums is exact, and sum / len is rounded once:
// the means are the reference's bit for bit, for any grouping of the additions.  That is what the entry's limits (C <= 64, fewer than
// 2^20 rows per document) buy.  Rows with NaN or infinite scores are outside this contract: they give meaningless records for their
// document (the prefix sum is NaN from there on) but every loop below is bounded by the row count, not by data.
//
// The filing quirk of the reference is reproduced, not repaired: its loop files the LAST run under the class of row N - 2 (`prev_class`
// is updated after the append at :472-477) -- the run's own class if it has two or more rows, the class of the run before it if it
// has one, and class C - 1 for N == 1 (prev_class == -1 indexes the list from the back).
//
// THE SAME TABLE FROM THE CRF MODE'S OUTPUTS (vbg_field_decode_tags: marginals [N, ntag] and the Viterbi path [N]) is the kernel's
// second instance, TAGS.  The chunk walk -- heads by ballot, prefix sums, the winner tables -- is shared; what the tag path changes:
//   rows     class = tag_class[path[r]]; score = the class posterior, the fp32 sum in tag order of the row's marginals over the tags
//            of that class; the threshold in double as above;
//   heads    a row also starts a run when its tag has tag_begin set;
//   sums     a score enters as the integer rint((double)score * 2^30) and the prefix sums are 64-bit integers: a marginal is no
//            multiple of 2^-30 as a softmax score is, so the exactness argued above is had by construction instead -- integer
//            additions associate, the one rounding is the division by len;
//   filing   every run under its own class, the last one included (the quirk belongs to a loop the crf mode never had).
// A run whose integer sum is 0 has the mean bits 0, which is "no record" in the winner tables: it leaves none.
#include <type_traits>

#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

constexpr int DEC_THREADS = 256;            // rows per chunk
constexpr int DEC_WAVES = DEC_THREADS / 64;
constexpr int DEC_MAX_C = 64;
constexpr int DEC_ROW_BITS = 20;            // a document has fewer than 2^20 rows (see the argument above)
constexpr int DEC_DOCS = 512;               // documents per launch: their row ranges travel in the kernel arguments

struct dec_docs { int off[DEC_DOCS + 1]; };

__device__ __forceinline__ int highest_bit(unsigned long long m) { return 63 - __clzll((long long)m); }

constexpr double DEC_FIX = 1073741824.0;    // 2^30: the fixed-point scale of the TAGS sums

struct dec_tags { unsigned char cls[DEC_MAX_C]; unsigned char begin[DEC_MAX_C]; };     // tag -> class, tag -> opens a run

// a run's mean from its sum: the one rounding of either instance
__device__ __forceinline__ double run_mean(double sum, int len) { return sum / (double)len; }
__device__ __forceinline__ double run_mean(long long sum, int len) { return (double)sum * (1.0 / DEC_FIX) / (double)len; }

// the head in front of the head in `lane` of wave w: in the wave's ballot hm, else in an earlier wave, else -1 (in an earlier chunk)
__device__ __forceinline__ int dec_prev_head(unsigned long long hm, int lane, int w, int base, const int* s_whead) {
    const unsigned long long lower = hm & ((1ull << lane) - 1ull);
    int ph = lower ? base + w * 64 + highest_bit(lower) : -1;
    for (int k = w - 1; k >= 0 && ph < 0; --k) ph = s_whead[k];
    return ph;
}

__device__ __forceinline__ vbg_run_rec run_rec(int start, int len, int cls, double mean, double logp) {
    vbg_run_rec r;
    r.start = start; r.len = len; r.cls = cls; r.pad = 0; r.mean = mean; r.logp = logp;
    return r;
}

// TAGS == false: x = class scores [N, cols], cols == C, `path` and `tags` unused.  TAGS == true: x = marginals [N, cols], cols == ntag.
template <bool TAGS>
__global__ __launch_bounds__(DEC_THREADS) void field_decode_kernel(const float* __restrict__ x, const int* __restrict__ path, dec_docs docs,
                                                                   dec_tags tags, int doc0, int cols, int C, int use_thresh, double thresh,
                                                                   int* __restrict__ cls_out, float* __restrict__ score_out,
                                                                   vbg_decode_rec* __restrict__ best) {
    using sum_t = std::conditional_t<TAGS, long long, double>;
    __shared__ int s_cls[DEC_THREADS];                      // class of the chunk's rows
    __shared__ sum_t s_pb[DEC_THREADS];                     // sum of the document's scores in front of the row
    __shared__ sum_t s_wtot[DEC_WAVES];
    __shared__ int s_whead[DEC_WAVES];                      // last run head inside the wave's rows, or -1
    __shared__ unsigned long long s_cmax[DEC_MAX_C], s_ckey[DEC_MAX_C];     // per class, this chunk: largest mean, then smallest (start, len)
    __shared__ unsigned long long s_bmean[DEC_MAX_C], s_bkey[DEC_MAX_C];    // per class, so far (mean bits 0: no record)
    __shared__ int s_tc[DEC_MAX_C], s_tb[DEC_MAX_C];        // TAGS: the two tag tables
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r0 = docs.off[blockIdx.x], n = docs.off[blockIdx.x + 1] - r0;
    if (t < DEC_MAX_C) {
        s_cmax[t] = 0ull; s_ckey[t] = ~0ull; s_bmean[t] = 0ull; s_bkey[t] = ~0ull;
        if constexpr (TAGS) { s_tc[t] = tags.cls[t]; s_tb[t] = tags.begin[t]; }
    }
    __syncthreads();

    // carried from chunk to chunk, the same in every thread
    sum_t total = 0;         // sum of the scores of the rows in front of the chunk
    int open_head = -1;      // first row of the run that is open at the chunk's start
    sum_t open_pb = 0;       // sum of the scores in front of that row
    int prev_last = -1;      // class of the row in front of the chunk (-1: none, so row 0 is a head)
    int file_last = -1;      // class the document's last run is filed under
    for (int base = 0; base < n; base += DEC_THREADS) {
        const int g = base + t;
        const bool valid = g < n;
        int c = -1;
        bool begin = false;
        float sc = 0.f;
        if (valid) {
            const float* p = x + (long long)(r0 + g) * cols;
            if constexpr (TAGS) {
                const int tag = path[r0 + g];
                c = 0;
                if (tag >= 0 && tag < cols) {               // (a tag outside the table: class 0, score 0)
                    c = s_tc[tag];
                    begin = s_tb[tag] != 0;
                    for (int k = 0; k < cols; ++k)
                        if (s_tc[k] == c) sc += p[k];
                }
            } else {
                float mx;
                const float inv = row_softmax_norm(p, cols, mx);
                c = 0;
                sc = row_softmax_prob(p[0], mx, inv);
                for (int k = 1; k < cols; ++k) {
                    const float v = row_softmax_prob(p[k], mx, inv);
                    if (v > sc) { sc = v; c = k; }
                }
            }
            if (use_thresh && (double)sc < thresh) c = 0;
            cls_out[r0 + g] = c;
            score_out[r0 + g] = sc;
        }
        sum_t own;
        if constexpr (TAGS) own = __double2ll_rn((double)sc * DEC_FIX);
        else own = (double)sc;
        sum_t incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const sum_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        s_cls[t] = c;
        if (lane == 63) s_wtot[w] = incl;
        __syncthreads();                                                            // 1: classes and wave totals of the chunk
        sum_t pb = total + (incl - own), chunk_total = 0;
#pragma unroll
        for (int k = 0; k < DEC_WAVES; ++k) {
            const sum_t wt = s_wtot[k];
            if (k < w) pb += wt;
            chunk_total += wt;
        }
        const int left = t > 0 ? s_cls[t - 1] : prev_last;
        const bool head = valid && (c != left || begin);
        if (base + DEC_THREADS >= n) {
            if constexpr (TAGS) file_last = s_cls[n - 1 - base];                    // its own class
            else file_last = n == 1 ? C - 1 : (n - 2 >= base ? s_cls[n - 2 - base] : prev_last);      // the reference's: the class of row n - 2
        }
        const int chunk_last = s_cls[DEC_THREADS - 1];
        s_pb[t] = pb;
        const unsigned long long hm = __ballot(head);
        if (lane == 0) s_whead[w] = hm ? base + w * 64 + highest_bit(hm) : -1;
        __syncthreads();                                                            // 2: prefix sums and wave heads
        // a head closes the run in front of it and files it under that run's class
        unsigned long long bits = 0ull, key = 0ull;
        int fc = -1;
        if (head && g > 0) {
            int ph = dec_prev_head(hm, lane, w, base, s_whead);
            sum_t ppb;
            if (ph >= 0) ppb = s_pb[ph - base];
            else { ph = open_head; ppb = open_pb; }
            const int len = g - ph;
            bits = (unsigned long long)__double_as_longlong(run_mean(pb - ppb, len));
            key = ((unsigned long long)ph << DEC_ROW_BITS) | (unsigned long long)len;
            fc = left;
            atomicMax(&s_cmax[fc], bits);
        }
        int lh = -1;
        for (int k = DEC_WAVES - 1; k >= 0 && lh < 0; --k) lh = s_whead[k];
        if (lh >= 0) { open_head = lh; open_pb = s_pb[lh - base]; }
        total += chunk_total;
        prev_last = chunk_last;
        __syncthreads();                                                            // 3: the chunk's largest mean per class
        if (fc >= 0 && s_cmax[fc] == bits) atomicMin(&s_ckey[fc], key);
        __syncthreads();                                                            // 4: and its first run among those
        if (t < C) {
            if (s_cmax[t] > s_bmean[t]) { s_bmean[t] = s_cmax[t]; s_bkey[t] = s_ckey[t]; }
            s_cmax[t] = 0ull;
            s_ckey[t] = ~0ull;
        }
    }
    __syncthreads();
    if (n > 0 && t == 0) {                                  // the last run (scores: filed the reference's way, last in its class's list)
        const int fc = file_last;
        const int len = n - open_head;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(run_mean(total - open_pb, len));
        if (bits > s_bmean[fc]) {
            s_bmean[fc] = bits;
            s_bkey[fc] = ((unsigned long long)open_head << DEC_ROW_BITS) | (unsigned long long)len;
        }
    }
    __syncthreads();
    if (t < C) {
        vbg_decode_rec r;
        const unsigned long long m = s_bmean[t], key = s_bkey[t];
        r.start = m ? (int)(key >> DEC_ROW_BITS) : -1;
        r.len = m ? (int)(key & ((1ull << DEC_ROW_BITS) - 1ull)) : 0;
        r.mean = m ? __longlong_as_double((long long)m) : 0.0;
        best[(long long)(doc0 + blockIdx.x) * C + t] = r;
    }
}

// EVERY run of a document, not the winners (vbg_field_runs / vbg_field_runs_tags): field_decode_kernel's rows, heads and prefix sums,
// and in place of its winner tables one vbg_run_rec per ROW.  The record of a run lies at the run's first row and is written by the
// thread that closes the run -- the next head, which knows where the run in front of it began, or after the walk thread 0 for the
// last run; every row that is no head writes its own record with len 0.  One writer per record, no ranking, no compaction: the host
// keeps the records with len > 0, and they stand in row order.  Every run is filed under its own class in both instances: the
// reference's `prev_class` quirk belongs to its winner loop, not to a listing.
// TAGS adds the run's log posterior under the CRF from vbg_crf_path_logp's rows: lm of the first row + the fp64 sum of lc over the
// rest, the sum taken as a difference of a second prefix sum L (inclusive, fp64): rows h1 + 1 .. h2 - 1 hold L(h2 - 1) - L(h1).
template <bool TAGS>
__global__ __launch_bounds__(DEC_THREADS) void field_runs_kernel(const float* __restrict__ x, const int* __restrict__ path,
                                                                 const float* __restrict__ lm, const float* __restrict__ lc, dec_docs docs,
                                                                 dec_tags tags, int cols, int use_thresh, double thresh,
                                                                 int* __restrict__ cls_out, float* __restrict__ score_out,
                                                                 vbg_run_rec* __restrict__ runs) {
    using sum_t = std::conditional_t<TAGS, long long, double>;
    __shared__ int s_cls[DEC_THREADS];                      // class of the chunk's rows
    __shared__ sum_t s_pb[DEC_THREADS];                     // sum of the document's scores in front of the row
    __shared__ double s_pl[DEC_THREADS];                    // TAGS: sum of the document's lc up to and including the row
    __shared__ sum_t s_wtot[DEC_WAVES];
    __shared__ double s_wtot_l[DEC_WAVES];
    __shared__ int s_whead[DEC_WAVES];                      // last run head inside the wave's rows, or -1
    __shared__ int s_tc[DEC_MAX_C], s_tb[DEC_MAX_C];        // TAGS: the two tag tables
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r0 = docs.off[blockIdx.x], n = docs.off[blockIdx.x + 1] - r0;
    if constexpr (TAGS) {
        if (t < DEC_MAX_C) { s_tc[t] = tags.cls[t]; s_tb[t] = tags.begin[t]; }
    }
    __syncthreads();

    // carried from chunk to chunk, the same in every thread
    sum_t total = 0;         // sum of the scores of the rows in front of the chunk
    double total_l = 0.0;    // sum of lc over the rows in front of the chunk
    int open_head = -1;      // first row of the run that is open at the chunk's start
    sum_t open_pb = 0;       // sum of the scores in front of that row
    double open_pl = 0.0;    // sum of lc up to and including that row
    int prev_last = -1;      // class of the row in front of the chunk (-1: none, so row 0 is a head)
    int last_cls = 0;        // class of the document's last row
    for (int base = 0; base < n; base += DEC_THREADS) {
        const int g = base + t;
        const bool valid = g < n;
        int c = -1;
        bool begin = false;
        float sc = 0.f;
        double own_l = 0.0;
        if (valid) {                                        // the row, as field_decode_kernel forms it
            const float* p = x + (long long)(r0 + g) * cols;
            if constexpr (TAGS) {
                const int tag = path[r0 + g];
                c = 0;
                if (tag >= 0 && tag < cols) {               // (a tag outside the table: class 0, score 0)
                    c = s_tc[tag];
                    begin = s_tb[tag] != 0;
                    for (int k = 0; k < cols; ++k)
                        if (s_tc[k] == c) sc += p[k];
                }
                own_l = (double)lc[r0 + g];
            } else {
                float mx;
                const float inv = row_softmax_norm(p, cols, mx);
                c = 0;
                sc = row_softmax_prob(p[0], mx, inv);
                for (int k = 1; k < cols; ++k) {
                    const float v = row_softmax_prob(p[k], mx, inv);
                    if (v > sc) { sc = v; c = k; }
                }
            }
            if (use_thresh && (double)sc < thresh) c = 0;
            cls_out[r0 + g] = c;
            score_out[r0 + g] = sc;
        }
        sum_t own;
        if constexpr (TAGS) own = __double2ll_rn((double)sc * DEC_FIX);
        else own = (double)sc;
        sum_t incl = own;
        double incl_l = own_l;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const sum_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
            if constexpr (TAGS) {
                const double up_l = __shfl_up(incl_l, o, 64);
                if (lane >= o) incl_l += up_l;
            }
        }
        s_cls[t] = c;
        if (lane == 63) { s_wtot[w] = incl; s_wtot_l[w] = incl_l; }
        __syncthreads();                                                            // 1: classes and wave totals of the chunk
        sum_t pb = total + (incl - own), chunk_total = 0;
        double pl = total_l + incl_l, chunk_total_l = 0.0;
#pragma unroll
        for (int k = 0; k < DEC_WAVES; ++k) {
            const sum_t wt = s_wtot[k];
            const double wl = s_wtot_l[k];
            if (k < w) { pb += wt; pl += wl; }
            chunk_total += wt;
            chunk_total_l += wl;
        }
        const int left = t > 0 ? s_cls[t - 1] : prev_last;
        const bool head = valid && (c != left || begin);
        if (base + DEC_THREADS >= n) last_cls = s_cls[n - 1 - base];
        const int chunk_last = s_cls[DEC_THREADS - 1];
        s_pb[t] = pb;
        s_pl[t] = pl;
        const unsigned long long hm = __ballot(head);
        if (lane == 0) s_whead[w] = hm ? base + w * 64 + highest_bit(hm) : -1;
        __syncthreads();                                                            // 2: prefix sums and wave heads
        if (head && g > 0) {                                // a head closes the run in front of it: that run's record, at its first row
            int ph = dec_prev_head(hm, lane, w, base, s_whead);
            sum_t ppb;
            double ppl;
            if (ph >= 0) { ppb = s_pb[ph - base]; ppl = s_pl[ph - base]; }
            else { ph = open_head; ppb = open_pb; ppl = open_pl; }
            const double mean = run_mean(pb - ppb, g - ph);
            double logp = 0.0;
            if constexpr (TAGS) logp = (double)lm[r0 + ph] + ((pl - own_l) - ppl);
            runs[r0 + ph] = run_rec(ph, g - ph, left, mean, logp);
        } else if (valid && !head) {
            runs[r0 + g] = run_rec(0, 0, 0, 0.0, 0.0);
        }
        int lh = -1;
        for (int k = DEC_WAVES - 1; k >= 0 && lh < 0; --k) lh = s_whead[k];
        if (lh >= 0) { open_head = lh; open_pb = s_pb[lh - base]; open_pl = s_pl[lh - base]; }
        total += chunk_total;
        total_l += chunk_total_l;
        prev_last = chunk_last;
        __syncthreads();                                                            // 3: the chunk's tables are free again
    }
    if (n > 0 && t == 0) {                                  // the last run
        const double mean = run_mean(total - open_pb, n - open_head);
        double logp = 0.0;
        if constexpr (TAGS) logp = (double)lm[r0 + open_head] + (total_l - open_pl);
        runs[r0 + open_head] = run_rec(open_head, n - open_head, last_cls, mean, logp);
    }
}

}  // namespace vbg

using namespace vbg;

// the row ranges: ascending from a row >= 0, every document shorter than 2^20 rows
static bool dec_rows_ok(const int* h_doc_off, int ndoc) {
    if (h_doc_off[0] < 0) return false;
    for (int d = 0; d < ndoc; ++d) {
        const long long nd = (long long)h_doc_off[d + 1] - h_doc_off[d];
        if (!(nd >= 0 && nd < (1ll << DEC_ROW_BITS))) return false;
    }
    return true;
}

// the two host tables of a *_tags entry, checked, as the kernels take them
static bool dec_make_tags(dec_tags& tags, int ntag, int C, const int* h_tag_class, const int* h_tag_begin) {
    if (!(C >= 1 && C <= DEC_MAX_C && ntag >= 1 && ntag <= DEC_MAX_C && h_tag_class && h_tag_begin)) return false;
    tags = {};
    for (int k = 0; k < ntag; ++k) {
        if (!(h_tag_class[k] >= 0 && h_tag_class[k] < C && (h_tag_begin[k] == 0 || h_tag_begin[k] == 1))) return false;
        tags.cls[k] = (unsigned char)h_tag_class[k];
        tags.begin[k] = (unsigned char)h_tag_begin[k];
    }
    return true;
}

// the launches, DEC_DOCS documents each: launch(docs, nd, d0) starts the kernel for documents d0 .. d0 + nd - 1
template <class Launch>
static int dec_batches(const int* h_doc_off, int ndoc, Launch launch) {
    for (int d0 = 0; d0 < ndoc; d0 += DEC_DOCS) {
        const int nd = ndoc - d0 < DEC_DOCS ? ndoc - d0 : DEC_DOCS;
        dec_docs docs;
        for (int i = 0; i <= nd; ++i) docs.off[i] = h_doc_off[d0 + i];
        for (int i = nd + 1; i <= DEC_DOCS; ++i) docs.off[i] = docs.off[nd];
        launch(docs, nd, d0);
    }
    VBG_LAUNCH_RET();
}

template <bool TAGS>
static int decode_launch(const float* x, const int* path, const int* h_doc_off, int ndoc, const dec_tags& tags, int cols, int C,
                         int use_thresh, double thresh, int* cls, float* score, vbg_decode_rec* best, void* stream) {
    VBG_CHECK_ARG(dec_rows_ok(h_doc_off, ndoc));
    if (ndoc == 0) return VBG_OK;
    VBG_CHECK_ARG(best);
    if (h_doc_off[ndoc] > h_doc_off[0]) VBG_CHECK_ARG(x && cls && score && (path || !TAGS));
    return dec_batches(h_doc_off, ndoc, [&](const dec_docs& docs, int nd, int d0) {
        VBG_LAUNCH(field_decode_kernel<TAGS>, dim3(nd), dim3(DEC_THREADS), 0, (hipStream_t)stream, x, path, docs, tags, d0, cols, C,
                   use_thresh, thresh, cls, score, best);
    });
}

template <bool TAGS>
static int runs_launch(const float* x, const int* path, const float* lm, const float* lc, const int* h_doc_off, int ndoc,
                       const dec_tags& tags, int cols, int use_thresh, double thresh, int* cls, float* score, vbg_run_rec* runs,
                       void* stream) {
    VBG_CHECK_ARG(dec_rows_ok(h_doc_off, ndoc));
    if (ndoc == 0 || h_doc_off[ndoc] == h_doc_off[0]) return VBG_OK;
    VBG_CHECK_ARG(x && cls && score && runs && (!TAGS || (path && lm && lc)));
    return dec_batches(h_doc_off, ndoc, [&](const dec_docs& docs, int nd, int) {
        VBG_LAUNCH(field_runs_kernel<TAGS>, dim3(nd), dim3(DEC_THREADS), 0, (hipStream_t)stream, x, path, lm, lc, docs, tags, cols,
                   use_thresh, thresh, cls, score, runs);
    });
}

extern "C" int vbg_field_decode(const float* x, const int* h_doc_off, int ndoc, int C, int use_thresh, double thresh, int* cls,
                                float* score, vbg_decode_rec* best, void* stream) {
    VBG_CHECK_ARG(h_doc_off && ndoc >= 0 && C >= 1 && C <= DEC_MAX_C);
    return decode_launch<false>(x, nullptr, h_doc_off, ndoc, dec_tags{}, C, C, use_thresh, thresh, cls, score, best, stream);
}

extern "C" int vbg_field_runs(const float* x, const int* h_doc_off, int ndoc, int C, int use_thresh, double thresh, int* cls,
                              float* score, vbg_run_rec* runs, void* stream) {
    VBG_CHECK_ARG(h_doc_off && ndoc >= 0 && C >= 1 && C <= DEC_MAX_C);
    return runs_launch<false>(x, nullptr, nullptr, nullptr, h_doc_off, ndoc, dec_tags{}, C, use_thresh, thresh, cls, score, runs, stream);
}

extern "C" int vbg_field_runs_tags(const float* marginals, const int* path, const float* lm, const float* lc, const int* h_doc_off,
                                   int ndoc, int ntag, int C, const int* h_tag_class, const int* h_tag_begin, int use_thresh,
                                   double thresh, int* cls, float* score, vbg_run_rec* runs, void* stream) {
    dec_tags tags;
    VBG_CHECK_ARG(h_doc_off && ndoc >= 0 && dec_make_tags(tags, ntag, C, h_tag_class, h_tag_begin));
    return runs_launch<true>(marginals, path, lm, lc, h_doc_off, ndoc, tags, ntag, use_thresh, thresh, cls, score, runs, stream);
}

extern "C" int vbg_field_decode_tags(const float* marginals, const int* path, const int* h_doc_off, int ndoc, int ntag, int C,
                                     const int* h_tag_class, const int* h_tag_begin, int use_thresh, double thresh, int* cls, float* score,
                                     vbg_decode_rec* best, void* stream) {
    dec_tags tags;
    VBG_CHECK_ARG(h_doc_off && ndoc >= 0 && dec_make_tags(tags, ntag, C, h_tag_class, h_tag_begin));
    return decode_launch<true>(marginals, path, h_doc_off, ndoc, tags, ntag, C, use_thresh, thresh, cls, score, best, stream);
}
