// Validation counts on the device: what `validate` (pipeline/train_val_utils.py:520, :544-556, :563-657) hands to pipeline/criteria.py --
// token_F1_criteria's per-class TP / TN / FP / FN, token_classification_criteria's hits and BIO_F1_criteria's entities (seqeval, default
// mode) -- counted from the scores of one forward in ONE launch, one 256-thread workgroup per sequence, added into one table of 64-bit
// integers.  Nothing is read back and nothing is kept per document (vbg/metrics.py copies the table once, at the end of the epoch).
//
// The sequence is walked in chunks of 256 rows, one row per thread, with two barriers per chunk (the walk of decode.hip):
//   rows       each thread takes its row's predicted class (first index of the largest raw score, or the given tag) and its gt class;
//              a row with either outside [0, C) counts nowhere and reads `O` on both sides of the entity walk.  While the scores pass,
//              wave ballots count the literal token cells of every class (one LDS add per wave, class and cell);
//   boundaries boundary i lies between row i - 1 and row i.  seqeval's loop appends (type, begin, i - 1) when end(i) and sets begin = i
//              when start(i); both depend on the two rows only, so thread i evaluates them for gt and for the prediction from its own
//              tag and its left neighbour's.  begin at boundary i is the last start index <= i - 1: wave ballots of start(i), "highest
//              set bit below my lane", the wave's last start in LDS for the waves behind, and the start that is open when the chunk
//              begins, carried in registers.  Boundary i adds end_gt to n_true[pty_gt], end_pr to n_pred[pty_pr], and 1 to n_correct
//              when both end there with the same type and the same begin.  The virtual `O` behind the last row is boundary n, taken
//              by one thread after the walk from the carried state.
// Why an end always finds a start: end(i) needs a tag other than `O` on row i - 1; such a row either starts an entity or follows
// another tag other than `O`, and a tag other than `O` behind an `O` (or on row 0) always starts one.  The type of `O` never decides.
//
// Counters live in LDS per workgroup (3 * 64 + 64 * 64 + 4 * 64 ints at most; a sequence has fewer than 2^31 rows); at the end of the
// sequence the non-zero cells are added to `counts` with 64-bit integer atomics.  Integer sums: exact, the same for every schedule.
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

constexpr int MET_THREADS = 256;            // rows per chunk
constexpr int MET_WAVES = MET_THREADS / 64;
constexpr int MET_SEQS = 512;               // sequences per launch: their row ranges travel in the kernel arguments

struct met_seqs { int off[MET_SEQS + 1]; };

__device__ __forceinline__ int met_highest_bit(unsigned long long m) { return 63 - __clzll((long long)m); }

// tag codes: letter | type << 8
__device__ __forceinline__ int met_letter(int code) { return code & 0xff; }
__device__ __forceinline__ int met_type(int code) { return code >> 8; }
__device__ __forceinline__ bool met_end(int pc, int c) {
    const int pt = met_letter(pc), t = met_letter(c);
    if (pt == VBG_TAG_E || pt == VBG_TAG_S) return true;
    if ((pt == VBG_TAG_B || pt == VBG_TAG_I) && (t == VBG_TAG_B || t == VBG_TAG_S || t == VBG_TAG_O)) return true;
    return pt != VBG_TAG_O && met_type(pc) != met_type(c);
}
__device__ __forceinline__ bool met_start(int pc, int c) {
    const int pt = met_letter(pc), t = met_letter(c);
    if (t == VBG_TAG_B || t == VBG_TAG_S) return true;
    if ((pt == VBG_TAG_E || pt == VBG_TAG_S || pt == VBG_TAG_O) && (t == VBG_TAG_E || t == VBG_TAG_I)) return true;
    return t != VBG_TAG_O && met_type(pc) != met_type(c);
}

__global__ __launch_bounds__(MET_THREADS) void seq_metrics_kernel(const float* __restrict__ scores, const int* __restrict__ pred_tags,
                                                                  const int* __restrict__ gt, met_seqs seqs, int C, int T,
                                                                  vbg_tag_table tags, long long* __restrict__ counts) {
    __shared__ int s_cnt[VBG_METRICS_COUNTS(VBG_METRICS_MAX_T, VBG_METRICS_MAX_C)];
    __shared__ int s_gt[MET_THREADS], s_pr[MET_THREADS];    // tag codes of the chunk's rows
    __shared__ int s_wg[MET_WAVES], s_wp[MET_WAVES];        // last start inside the wave's rows (gt, prediction), or -1
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r0 = seqs.off[blockIdx.x], n = seqs.off[blockIdx.x + 1] - r0;
    if (n <= 0) return;                                     // (the same in every thread)
    const int ncnt = VBG_METRICS_COUNTS(T, C);
    int* s_ent = s_cnt + VBG_METRICS_ENT(T, C);
    int* s_conf = s_cnt + VBG_METRICS_CONF(T, C);
    int* s_tok = s_cnt + VBG_METRICS_TOK(T, C);
    for (int i = t; i < ncnt; i += MET_THREADS) s_cnt[i] = 0;
    __syncthreads();

    // carried from chunk to chunk, the same in every thread
    int prev_g = VBG_TAG_O, prev_p = VBG_TAG_O;             // tag codes of the row in front of the chunk
    int open_g = 0, open_p = 0;                             // last start in front of the chunk
    for (int base = 0; base < n; base += MET_THREADS) {
        const int g = base + t;
        const bool valid = g < n;
        int gc = -1, pc = -1;
        if (valid) {
            gc = gt[r0 + g];
            if ((unsigned)gc >= (unsigned)C) gc = -1;
            if (pred_tags) {
                pc = pred_tags[r0 + g];
                if ((unsigned)pc >= (unsigned)C) pc = -1;
            }
        }
        if (scores) {                                       // (the loop is the same in every lane: the ballots need the whole wave)
            const float* p = scores + (long long)(r0 + (valid ? g : 0)) * C;
            const bool rowok = gc >= 0;
            float best = 0.f;
            for (int k = 0; k < C; ++k) {
                const float v = valid ? p[k] : 0.f;
                if (k == 0) { best = v; pc = valid ? 0 : -1; }
                else if (v > best) { best = v; pc = k; }
                const bool one = v >= 1.f && v < 2.f, zero = v > -1.f && v < 1.f;      // the value truncated toward zero
                const bool own = gc == k;
                const unsigned long long tp = __ballot(rowok && own && one), tn = __ballot(rowok && !own && zero);
                const unsigned long long fp = __ballot(rowok && !own && one), fn = __ballot(rowok && own && zero);
                if (lane == 0) {
                    if (tp) atomicAdd(&s_tok[k * 4 + 0], __popcll(tp));
                    if (tn) atomicAdd(&s_tok[k * 4 + 1], __popcll(tn));
                    if (fp) atomicAdd(&s_tok[k * 4 + 2], __popcll(fp));
                    if (fn) atomicAdd(&s_tok[k * 4 + 3], __popcll(fn));
                }
            }
        }
        const bool counted = gc >= 0 && pc >= 0;
        if (counted) atomicAdd(&s_conf[gc * C + pc], 1);
        if (T > 0) {                                        // (the same in every thread)
            const int cg = counted ? (int)tags.prefix[gc] | ((int)tags.type[gc] << 8) : VBG_TAG_O;
            const int cp = counted ? (int)tags.prefix[pc] | ((int)tags.type[pc] << 8) : VBG_TAG_O;
            s_gt[t] = cg;
            s_pr[t] = cp;
            __syncthreads();                                                        // 1: the chunk's tags
            const int lg = t > 0 ? s_gt[t - 1] : prev_g, lp = t > 0 ? s_pr[t - 1] : prev_p;
            const int last = n - base < MET_THREADS ? n - base - 1 : MET_THREADS - 1;      // last row of the sequence inside the chunk
            const int next_g = s_gt[last], next_p = s_pr[last];
            const bool sg = valid && met_start(lg, cg), sp = valid && met_start(lp, cp);
            const bool eg = valid && met_end(lg, cg), ep = valid && met_end(lp, cp);
            const unsigned long long mg = __ballot(sg), mp = __ballot(sp);
            if (lane == 0) {
                s_wg[w] = mg ? base + w * 64 + met_highest_bit(mg) : -1;
                s_wp[w] = mp ? base + w * 64 + met_highest_bit(mp) : -1;
            }
            __syncthreads();                                                        // 2: the waves' last starts
            if (eg || ep) {
                const unsigned long long below = (1ull << lane) - 1ull;
                int bg = (mg & below) ? base + w * 64 + met_highest_bit(mg & below) : -1;
                int bp = (mp & below) ? base + w * 64 + met_highest_bit(mp & below) : -1;
                for (int k = w - 1; k >= 0 && bg < 0; --k) bg = s_wg[k];
                for (int k = w - 1; k >= 0 && bp < 0; --k) bp = s_wp[k];
                if (bg < 0) bg = open_g;
                if (bp < 0) bp = open_p;
                if (eg) atomicAdd(&s_ent[met_type(lg) * 3 + 0], 1);
                if (ep) atomicAdd(&s_ent[met_type(lp) * 3 + 1], 1);
                if (eg && ep && met_type(lg) == met_type(lp) && bg == bp) atomicAdd(&s_ent[met_type(lg) * 3 + 2], 1);
            }
            int hg = -1, hp = -1;
            for (int k = MET_WAVES - 1; k >= 0 && hg < 0; --k) hg = s_wg[k];
            for (int k = MET_WAVES - 1; k >= 0 && hp < 0; --k) hp = s_wp[k];
            if (hg >= 0) open_g = hg;
            if (hp >= 0) open_p = hp;
            prev_g = next_g;
            prev_p = next_p;
            // (the next chunk writes s_gt / s_pr before its barrier 1 and s_wg / s_wp behind it: nothing read above is overwritten early)
        }
    }
    if (T > 0 && t == 0) {                                  // boundary n: the virtual `O` row closes what is open
        const bool eg = met_end(prev_g, VBG_TAG_O), ep = met_end(prev_p, VBG_TAG_O);
        if (eg) atomicAdd(&s_ent[met_type(prev_g) * 3 + 0], 1);
        if (ep) atomicAdd(&s_ent[met_type(prev_p) * 3 + 1], 1);
        if (eg && ep && met_type(prev_g) == met_type(prev_p) && open_g == open_p) atomicAdd(&s_ent[met_type(prev_g) * 3 + 2], 1);
    }
    __syncthreads();
    for (int i = t; i < ncnt; i += MET_THREADS) {
        const int v = s_cnt[i];
        if (v) atomicAdd((unsigned long long*)(counts + i), (unsigned long long)v);
    }
}

}  // namespace vbg

using namespace vbg;

extern "C" int vbg_seq_metrics(const float* scores, const int* pred_tags, const int* gt, const int* h_doc_off, int ndoc, int C, int T,
                               vbg_tag_table tags, long long* counts, void* stream) {
    VBG_CHECK_ARG(h_doc_off && ndoc >= 0 && C >= 1 && C <= VBG_METRICS_MAX_C && T >= 0 && T <= VBG_METRICS_MAX_T);
    VBG_CHECK_ARG((scores != nullptr) != (pred_tags != nullptr));
    if (T > 0)
        for (int k = 0; k < C; ++k) VBG_CHECK_ARG(tags.prefix[k] <= VBG_TAG_S && tags.type[k] < T);
    VBG_CHECK_ARG(h_doc_off[0] >= 0);
    for (int d = 0; d < ndoc; ++d) VBG_CHECK_ARG(h_doc_off[d + 1] >= h_doc_off[d]);
    if (ndoc == 0) return VBG_OK;
    VBG_CHECK_ARG(counts);
    if (h_doc_off[ndoc] == h_doc_off[0]) return VBG_OK;     // only empty sequences: nothing to count
    VBG_CHECK_ARG(gt);
    for (int d0 = 0; d0 < ndoc; d0 += MET_SEQS) {
        const int nd = ndoc - d0 < MET_SEQS ? ndoc - d0 : MET_SEQS;
        met_seqs seqs;
        for (int i = 0; i <= nd; ++i) seqs.off[i] = h_doc_off[d0 + i];
        for (int i = nd + 1; i <= MET_SEQS; ++i) seqs.off[i] = seqs.off[nd];
        VBG_LAUNCH(seq_metrics_kernel, dim3(nd), dim3(MET_THREADS), 0, (hipStream_t)stream, scores, pred_tags, gt, seqs, C, T, tags, counts);
    }
    VBG_LAUNCH_RET();
}
