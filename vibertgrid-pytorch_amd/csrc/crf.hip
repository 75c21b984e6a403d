// Linear-chain CRF of the `crf` classifier head (reference model/crf.py:33-157, called per document at
// model/field_type_classification_head.py:690-716).
//
// One 64-thread block per document, lane i owns tag i (ntag <= 64).  The recursions are sequential in the segment
// index (S <= a few hundred), each step is ntag x ntag flops: latency-bound by design, the point is to stay on the device
// and to batch all documents of the rank into one launch.  trans[i*ntag + j] = score of the transition j -> i.
//
// The file in order: crf_nll_fwd / crf_nll_bwd / crf_viterbi, the default training and decode route in the reference's arithmetic; the
// wave kernels crf_posterior and crf_path_logp behind the description and the functions they share; the length-stable loss crf_nll_stable
// with its scaling launch; the entries, behind their one tag-range check and one ntag dispatch.
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

constexpr int CRF_MAX_TAGS = 64;

// log-sum-exp over j of (prev[j] + w[j]) the way the reference does it (model/crf.py:24-30): max + log(sum(exp(v - max)))
__device__ __forceinline__ float lse_row(const float* prev, const float* w, int n) {
    float mx = prev[0] + w[0];
    for (int j = 1; j < n; ++j) mx = fmaxf(mx, prev[j] + w[j]);
    float s = 0.f;
    for (int j = 0; j < n; ++j) s += expf(prev[j] + w[j] - mx);
    return mx + logf(s);
}

// forward algorithm + gold path score; alpha[t*ntag + i] (emission included) is kept for the backward pass
__global__ __launch_bounds__(64) void crf_nll_fwd_kernel(const float* __restrict__ em, const int* __restrict__ tags,
                                                         const int* __restrict__ doc_off, const float* __restrict__ trans, int ntag,
                                                         int start, int stop, float* __restrict__ alpha, float* __restrict__ logz,
                                                         float* __restrict__ nll) {
    __shared__ float prev[CRF_MAX_TAGS], tr[CRF_MAX_TAGS * CRF_MAX_TAGS];
    const int d = blockIdx.x, i = threadIdx.x;
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    for (int k = i; k < ntag * ntag; k += 64) tr[k] = trans[k];
    if (i < ntag) prev[i] = (i == start) ? 0.f : -10000.f;
    __syncthreads();
    for (int t = 0; t < n; ++t) {
        float a = 0.f;
        if (i < ntag) a = lse_row(prev, tr + i * ntag, ntag) + em[(long long)(r0 + t) * ntag + i];
        __syncthreads();
        if (i < ntag) { prev[i] = a; alpha[(long long)(r0 + t) * ntag + i] = a; }
        __syncthreads();
    }
    if (i == 0) {
        const float z = lse_row(prev, tr + stop * ntag, ntag);
        float gold = 0.f;
        int pt = start;
        for (int t = 0; t < n; ++t) {
            const int ct = tags[r0 + t];
            gold += tr[ct * ntag + pt] + em[(long long)(r0 + t) * ntag + ct];
            pt = ct;
        }
        gold += tr[stop * ntag + pt];
        logz[d] = z;
        nll[d] = n > 0 ? (z - gold) / (float)n : 0.f;
    }
}

// d nll_d / d emissions and transitions: (marginals - gold indicators) * gout[d] / n_d
__global__ __launch_bounds__(64) void crf_nll_bwd_kernel(const float* __restrict__ em, const int* __restrict__ tags,
                                                         const int* __restrict__ doc_off, const float* __restrict__ trans, int ntag,
                                                         int start, int stop, const float* __restrict__ alpha,
                                                         const float* __restrict__ logz, const float* __restrict__ gout,
                                                         float* __restrict__ dem, float* dtrans, float* dtrans_part) {
    __shared__ float beta[CRF_MAX_TAGS], nb[CRF_MAX_TAGS], prev[CRF_MAX_TAGS], tr[CRF_MAX_TAGS * CRF_MAX_TAGS];
    __shared__ float dtr[CRF_MAX_TAGS * CRF_MAX_TAGS];
    const int d = blockIdx.x, i = threadIdx.x;
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    if (n == 0) return;
    const float z = logz[d], g = gout[d] / (float)n;
    for (int k = i; k < ntag * ntag; k += 64) { tr[k] = trans[k]; dtr[k] = 0.f; }
    if (i < ntag) beta[i] = trans[stop * ntag + i];              // beta of the last position: the transition to STOP
    __syncthreads();
    for (int t = n - 1; t >= 0; --t) {
        // state marginal of position t and its emission gradient
        if (i < ntag) {
            const float a = alpha[(long long)(r0 + t) * ntag + i];
            const float p = expf(a + beta[i] - z);
            dem[(long long)(r0 + t) * ntag + i] = g * (p - (tags[r0 + t] == i ? 1.f : 0.f));
            if (t == n - 1) dtr[stop * ntag + i] += p;          // terminal transition i -> STOP
            // alpha of the previous position (or the initial vector) for the pairwise marginals
            prev[i] = t > 0 ? alpha[(long long)(r0 + t - 1) * ntag + i] : (i == start ? 0.f : -10000.f);
            nb[i] = em[(long long)(r0 + t) * ntag + i] + beta[i];        // emission of t + everything after it, per tag of t
        }
        __syncthreads();
        if (i < ntag) {
            // pairwise marginals p(y_{t-1} = j, y_t = i): lane i owns row i of dtrans
            for (int j = 0; j < ntag; ++j) dtr[i * ntag + j] += expf(prev[j] + tr[i * ntag + j] + nb[i] - z);
        }
        __syncthreads();
        // beta of position t-1: lane j sums over the tag i of position t
        float b = 0.f;
        if (i < ntag) {
            float mx = tr[0 * ntag + i] + nb[0];
            for (int k = 1; k < ntag; ++k) mx = fmaxf(mx, tr[k * ntag + i] + nb[k]);
            float s = 0.f;
            for (int k = 0; k < ntag; ++k) s += expf(tr[k * ntag + i] + nb[k] - mx);
            b = mx + logf(s);
        }
        __syncthreads();
        if (i < ntag) beta[i] = b;
        __syncthreads();
    }
    if (i == 0) {                 // gold path indicators
        int pt = start;
        for (int t = 0; t < n; ++t) {
            const int ct = tags[r0 + t];
            dtr[ct * ntag + pt] -= 1.f;
            pt = ct;
        }
        dtr[stop * ntag + pt] -= 1.f;
    }
    __syncthreads();
    if (dtrans_part) {            // deterministic mode: this document's row of the partials slab (the host adds the rows in order)
        for (int k = i; k < ntag * ntag; k += 64) dtrans_part[(long long)d * ntag * ntag + k] = g * dtr[k];
    } else {
        for (int k = i; k < ntag * ntag; k += 64) unsafeAtomicAdd(dtrans + k, g * dtr[k]);
    }
}

// Viterbi decode (model/crf.py:99-145): first maximal previous tag on ties, like torch.max
__global__ __launch_bounds__(64) void crf_viterbi_kernel(const float* __restrict__ em, const int* __restrict__ doc_off,
                                                         const float* __restrict__ trans, int ntag, int start, int stop,
                                                         int* __restrict__ bptr, int* __restrict__ path, float* __restrict__ score) {
    __shared__ float prev[CRF_MAX_TAGS], tr[CRF_MAX_TAGS * CRF_MAX_TAGS];
    const int d = blockIdx.x, i = threadIdx.x;
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    for (int k = i; k < ntag * ntag; k += 64) tr[k] = trans[k];
    if (i < ntag) prev[i] = (i == start) ? 0.f : -10000.f;
    __syncthreads();
    for (int t = 0; t < n; ++t) {
        float best = 0.f;
        int bj = 0;
        if (i < ntag) {
            best = prev[0] + tr[i * ntag];
            for (int j = 1; j < ntag; ++j) {
                const float v = prev[j] + tr[i * ntag + j];
                if (v > best) { best = v; bj = j; }
            }
            best += em[(long long)(r0 + t) * ntag + i];
        }
        __syncthreads();
        if (i < ntag) { prev[i] = best; bptr[(long long)(r0 + t) * ntag + i] = bj; }
        __syncthreads();
    }
    if (i == 0) {
        float best = prev[0] + tr[stop * ntag];
        int cur = 0;
        for (int j = 1; j < ntag; ++j) {
            const float v = prev[j] + tr[stop * ntag + j];
            if (v > best) { best = v; cur = j; }
        }
        score[d] = best;
        for (int t = n - 1; t >= 0; --t) {
            path[r0 + t] = cur;
            cur = bptr[(long long)(r0 + t) * ntag + cur];
        }
    }
}

// ---- the wave kernels (vbg_crf_posterior, vbg_crf_path_logp): one wave per document, lane i owns tag i -------------------------------
// The grid is a handful of waves and the time is the serial chain, rows x work per step, so both kernels are shaped by what sits on it.
// What they share is described once, here.  As functions they share lse_slice, lse_join, the re-centring (crf_recentred) and the log Z
// end; the lane geometry, the transition loads, the beta step's store and the tile rows stand in each kernel's own text, because
// behind a helper the compiler orders them otherwise and the chains get 0.2 - 3.5 % longer (profiles/crf_decode_shared.txt).
//   transitions  lane i keeps ITS row (forward, Viterbi) and later its column (backward) in registers: tw[], ntag rounded up to a
//                template size NTP, the tail filled with -inf (a term that never wins a maximum and adds exp(-inf) == 0 to a sum);
//   vectors      the previous step's vector lies in LDS (two buffers, one barrier per step) and the lanes read it at the same
//                addresses -- a broadcast, no bank conflict -- four values to a read;
//   lanes        up to 32 tags, two lanes share a tag (HALF): lane l and lane l + 32 own tag l, each walks half of the previous tags,
//                and one exchange across the halves per step joins the two partial sums -- half the instructions on the chain;
//   loads        emissions arrive one step ahead, as does the forward vector in the backward pass.
// Forward and backward run in log space and are re-centred at every step: the maximum of the previous vector -- which the lanes
// have in hand from the broadcast read, so no reduction over the tags -- is taken out of the step's result.  The magnitudes stay at
// (emission + transition + log ntag) whatever the length.
// Position t's marginals are exp(a_t + b_t - max) / sum: 64 rows of a_t + b_t are gathered in an LDS tile (odd row stride), then one
// lane per row takes maximum and sum in tag order (expf / logf: off the chain).
constexpr int CRF_TILE_ROWS = 64;
constexpr int CRF_TILE_STRIDE = CRF_MAX_TAGS + 1;

// log-sum-exp over JW terms v[j] + w[j], as (max, sum of exp(. - max)), with the maximum of v alone on the side.  A slice that holds
// only -inf terms gives (CRF_LOW, 0): a finite stand-in for its maximum keeps -inf - max from being NaN.
constexpr float CRF_LOW = -3.0e38f;

template <int JW>
__device__ __forceinline__ void lse_slice(const float* __restrict__ v, const float (&w)[JW], float& mx_v, float& m2, float& s) {
    float pr[JW];
    mx_v = -INFINITY;
    m2 = CRF_LOW;
#pragma unroll
    for (int j = 0; j < JW; j += 4) {
        const float4 q = *reinterpret_cast<const float4*>(v + j);
        mx_v = fmaxf(fmaxf(mx_v, q.x), fmaxf(q.y, fmaxf(q.z, q.w)));
        pr[j] = q.x + w[j]; pr[j + 1] = q.y + w[j + 1]; pr[j + 2] = q.z + w[j + 2]; pr[j + 3] = q.w + w[j + 3];
        m2 = fmaxf(fmaxf(m2, pr[j]), fmaxf(pr[j + 1], fmaxf(pr[j + 2], pr[j + 3])));
    }
    s = 0.f;
#pragma unroll
    for (int j = 0; j < JW; ++j) s += __expf(pr[j] - m2);
}

// HALF: the two lanes of a tag exchange their partial results (one cross-half shuffle each way)
template <bool HALF>
__device__ __forceinline__ void lse_join(float& mx_v, float& m2, float& s) {
    if (HALF) {
        const float mo = __shfl_xor(mx_v, 32, 64), m2o = __shfl_xor(m2, 32, 64), so = __shfl_xor(s, 32, 64);
        const float m = fmaxf(m2, m2o);
        s = s * __expf(m2 - m) + so * __expf(m2o - m);
        m2 = m;
        mx_v = fmaxf(mx_v, mo);
    }
}

// the re-centring, stated once: the log of a step's sum (m2, s) less mx, the maximum of the vector the step read.  Forward:
// a_t[i] = em + crf_recentred(lse of prev[j] + tr[i][j]); backward: b_{t-1}[i] = crf_recentred(lse of tr[k][i] + em_t[k] + b_t[k]).
__device__ __forceinline__ float crf_recentred(float mx, float m2, float s) { return (m2 - mx) + __logf(s); }

// log Z from the last forward vector pa, the transitions to STOP ps and the sum of the maxima taken out (the same value in every lane)
__device__ __forceinline__ double crf_log_z_end(const float* pa, const float* ps, int ntag, double carry) {
    float mx = pa[0];
    for (int j = 1; j < ntag; ++j) mx = fmaxf(mx, pa[j]);
    float m2 = (pa[0] - mx) + ps[0];
    for (int j = 1; j < ntag; ++j) m2 = fmaxf(m2, (pa[j] - mx) + ps[j]);
    float s = 0.f;
    for (int j = 0; j < ntag; ++j) s += expf((pa[j] - mx) + ps[j] - m2);
    return carry + (double)mx + (double)(m2 + logf(s));
}

// Posterior marginals + Viterbi + log Z in one launch (vbg_crf_posterior).  On top of the shared shape:
//   log Z        the forward pass carries the maxima it takes out into log Z in double;
//   Viterbi      the chain repeats crf_viterbi_kernel's arithmetic on the unnormalised values: prev[j] + tr[i][j], first maximum, + em;
//                of the two candidates of a tag's two lanes the lower half wins ties: the first maximum;
//   back trace   walked inside the backward pass, from the row of back pointers that pass has already fetched (a step ahead, like
//                the forward vector): no chain of dependent global loads behind the recursions;
//   marginals    the lane of a tile row divides it by its sum, and the tile goes out in whole rows.
template <int NTP, bool HALF>
__global__ __launch_bounds__(64) void crf_posterior_kernel(const float* __restrict__ em, const int* __restrict__ doc_off,
                                                           const float* __restrict__ trans, int ntag, int start, int stop,
                                                           float* __restrict__ ws, int* __restrict__ path, float* __restrict__ score,
                                                           float* __restrict__ logz, float* __restrict__ marg) {
    static_assert(!HALF || NTP <= 32, "two lanes per tag need ntag <= 32");
    constexpr int JW = HALF ? NTP / 2 : NTP;                // previous tags per lane
    static_assert(JW % 4 == 0, "the vectors are read four values at a time");
    __shared__ __attribute__((aligned(16))) float s_a[2][CRF_MAX_TAGS], s_v[2][CRF_MAX_TAGS], s_stop[CRF_MAX_TAGS];
    __shared__ float s_tile[CRF_TILE_ROWS * CRF_TILE_STRIDE];
    const int d = blockIdx.x, lane = threadIdx.x;
    const int i = HALF ? (lane & 31) : lane;                // the lane's tag
    const int j0 = HALF ? (lane >> 5) * JW : 0;             // first previous tag of the lane's slice
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    const bool own = lane < ntag;                           // the lanes that store: one per tag
    const int ic = i < ntag ? i : ntag - 1;                 // lanes past the tags repeat the last tag's loads and store nothing
    const float NEG = -INFINITY;
    const long long wrow = 2ll * ntag;                      // workspace words per row: ntag forward values, ntag back pointers
    int* __restrict__ wsi = reinterpret_cast<int*>(ws);

    float tw[JW];
#pragma unroll
    for (int j = 0; j < JW; ++j) tw[j] = j0 + j < ntag ? trans[ic * ntag + j0 + j] : NEG;
    s_stop[lane] = own ? trans[stop * ntag + lane] : NEG;
    s_a[0][lane] = s_v[0][lane] = own ? (lane == start ? 0.f : -10000.f) : NEG;
    s_a[1][lane] = s_v[1][lane] = NEG;
    __syncthreads();

    // ---- forward + Viterbi, t = 0 .. n - 1
    double carry = 0.0;                                     // sum of the maxima taken out so far (the same in every lane)
    float e_next = n > 0 ? em[(long long)r0 * ntag + ic] : 0.f;
    for (int t = 0; t < n; ++t) {
        const float e = e_next;
        if (t + 1 < n) e_next = em[(long long)(r0 + t + 1) * ntag + ic];
        float mx, m2, s;
        lse_slice<JW>(s_a[t & 1] + j0, tw, mx, m2, s);
        // Viterbi: crf_viterbi_kernel's additions in its order, the first maximum of the lane's slice
        const float4* pv = reinterpret_cast<const float4*>(s_v[t & 1] + j0);
        float best;
        int bj = j0;
        {
            const float4 q0 = pv[0];
            best = q0.x + tw[0];
            float v = q0.y + tw[1];
            if (v > best) { best = v; bj = j0 + 1; }
            v = q0.z + tw[2];
            if (v > best) { best = v; bj = j0 + 2; }
            v = q0.w + tw[3];
            if (v > best) { best = v; bj = j0 + 3; }
        }
#pragma unroll
        for (int j = 4; j < JW; j += 4) {
            const float4 q = pv[j >> 2];
            float v = q.x + tw[j];
            if (v > best) { best = v; bj = j0 + j; }
            v = q.y + tw[j + 1];
            if (v > best) { best = v; bj = j0 + j + 1; }
            v = q.z + tw[j + 2];
            if (v > best) { best = v; bj = j0 + j + 2; }
            v = q.w + tw[j + 3];
            if (v > best) { best = v; bj = j0 + j + 3; }
        }
        lse_join<HALF>(mx, m2, s);
        if (HALF) {                                         // the upper slice wins only when strictly greater: the first maximum
            const float bo = __shfl_xor(best, 32, 64);
            const int jo = __shfl_xor(bj, 32, 64);
            const bool up = lane >= 32;
            const float blo = up ? bo : best, bhi = up ? best : bo;
            const int jlo = up ? jo : bj, jhi = up ? bj : jo;
            best = bhi > blo ? bhi : blo;
            bj = bhi > blo ? jhi : jlo;
        }
        const float a = e + crf_recentred(mx, m2, s);
        carry += (double)mx;
        best += e;
        const int nb = (t + 1) & 1;
        s_a[nb][lane] = own ? a : NEG;
        s_v[nb][lane] = own ? best : NEG;
        if (own) {
            ws[(long long)(r0 + t) * wrow + lane] = a;
            wsi[(long long)(r0 + t) * wrow + ntag + lane] = bj;
        }
        __syncthreads();
    }

    // ---- the end of both chains: every lane forms the same two values, lane 0 writes them
    int cur = 0;
    {
        const float* pv = s_v[n & 1];
        const float z = (float)crf_log_z_end(s_a[n & 1], s_stop, ntag, carry);
        float best = pv[0] + s_stop[0];
        for (int j = 1; j < ntag; ++j) {
            const float v = pv[j] + s_stop[j];
            if (v > best) { best = v; cur = j; }
        }
        if (lane == 0) { logz[d] = z; score[d] = best; }
    }
    if (n == 0) return;

    // ---- backward + back trace + marginals, t = n - 1 .. 0.  tw becomes the lane's slice of tag i's COLUMN: tw[k] = score of i -> j0 + k
#pragma unroll
    for (int k = 0; k < JW; ++k) tw[k] = j0 + k < ntag ? trans[(j0 + k) * ntag + ic] : NEG;
    float b = own ? s_stop[lane] : NEG;                     // beta of the last position: the transition to STOP
    long long row = (long long)(r0 + n - 1);
    float a_next = ws[row * wrow + ic], e_next_b = em[row * ntag + ic];
    int bp_next = wsi[row * wrow + ntag + ic];
    int slot = 0;                                           // rows waiting in the tile: tile row k holds position t + slot - 1 - k
    __syncthreads();                                        // (s_a is reused below)
    for (int t = n - 1; t >= 0; --t) {
        const float a = a_next, e = e_next_b;
        const int bp = bp_next;
        if (t > 0) {
            row = (long long)(r0 + t - 1);
            a_next = ws[row * wrow + ic];
            bp_next = wsi[row * wrow + ntag + ic];
            e_next_b = em[row * ntag + ic];
        }
        if (own) s_tile[slot * CRF_TILE_STRIDE + lane] = a + b;
        if (lane == 0) path[r0 + t] = cur;
        cur = __builtin_amdgcn_readlane(bp, __builtin_amdgcn_readfirstlane(cur));
        ++slot;
        if (slot == CRF_TILE_ROWS || t == 0) {
            __syncthreads();
            if (lane < slot) {                              // one lane per row: maximum, sum in tag order, division
                float* p = s_tile + lane * CRF_TILE_STRIDE;
                float mx = p[0];
                for (int k = 1; k < ntag; ++k) mx = fmaxf(mx, p[k]);
                float s = 0.f;
                for (int k = 0; k < ntag; ++k) { const float x = expf(p[k] - mx); p[k] = x; s += x; }
                for (int k = 0; k < ntag; ++k) p[k] = p[k] / s;
            }
            __syncthreads();
            // positions t .. t + slot - 1 are contiguous in `marg`: whole rows go out, 64 consecutive floats to a store
            int rr = lane / ntag, cc = lane - rr * ntag;
            const int q = 64 / ntag, rem = 64 - q * ntag;
            float* out = marg + (long long)(r0 + t) * ntag;
            for (int f = lane; f < slot * ntag; f += 64) {
                out[f] = s_tile[(slot - 1 - rr) * CRF_TILE_STRIDE + cc];
                rr += q;
                cc += rem;
                if (cc >= ntag) { cc -= ntag; ++rr; }
            }
            slot = 0;
            __syncthreads();
        }
        if (t > 0) {
            // beta of position t - 1: b[i] = log sum_k exp(tr[k][i] + em_t[k] + b_t[k]) - max(em_t + b_t)
            float* nbuf = s_a[t & 1];
            nbuf[lane] = own ? e + b : NEG;
            __syncthreads();
            float mx, m2, s;
            lse_slice<JW>(nbuf + j0, tw, mx, m2, s);
            lse_join<HALF>(mx, m2, s);
            b = crf_recentred(mx, m2, s);
        }
    }
}

// Log posteriors of a GIVEN tag path (vbg_crf_path_logp): the shared shape without a Viterbi chain and without marginal rows.  The
// re-centred backward vector gives the chain's conditionals directly:
//     log p(y_t = i | y_{t-1} = j, x) = tr[i][j] + (em_t[i] + b_t[i] - max_k(em_t[k] + b_t[k])) - b_{t-1}[j],
// b_{t-1}[j] = log sum_i exp(tr[i][j] + em_t[i] + b_t[i]) - the same maximum: the step that forms b_{t-1} has all three terms in
// hand.  The two it needs per row are picked without a data-dependent address that could leave the tables: em_t + b_t from the LDS
// vector at the clamped tag, b_{t-1} from the lane of the clamped tag.  The path itself stays off the chain: its tags wait in
// registers, 64 positions to a load and a tile ahead, and a step takes its two with v_readlane -- a load per step whose address is the
// same in every lane becomes a scalar load, which returns out of order and makes every LDS wait of the step wait for it as well.  The
// step leaves its part of the conditional in the lane of its tile row (a select); the transition is added where the rows go out.
// log Z never enters and the forward pass carries no sum of maxima.  The marginal of the path's tag is taken from the tile rows of
// a_t + b_t: the lane of a row picks the path's tag and writes the row's lm and lc.
template <int NTP, bool HALF>
__global__ __launch_bounds__(64) void crf_path_logp_kernel(const float* __restrict__ em, const int* __restrict__ doc_off,
                                                           const float* __restrict__ trans, int ntag, int start, int stop,
                                                           const int* __restrict__ path, float* __restrict__ ws,
                                                           float* __restrict__ lm, float* __restrict__ lc) {
    static_assert(!HALF || NTP <= 32, "two lanes per tag need ntag <= 32");
    constexpr int JW = HALF ? NTP / 2 : NTP;                // previous tags per lane
    static_assert(JW % 4 == 0, "the vectors are read four values at a time");
    __shared__ __attribute__((aligned(16))) float s_a[2][CRF_MAX_TAGS];
    __shared__ float s_tile[CRF_TILE_ROWS * CRF_TILE_STRIDE];
    const int d = blockIdx.x, lane = threadIdx.x;
    const int i = HALF ? (lane & 31) : lane;                // the lane's tag
    const int j0 = HALF ? (lane >> 5) * JW : 0;             // first previous tag of the lane's slice
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    if (n <= 0) return;
    const bool own = lane < ntag;                           // the lanes that store: one per tag
    const int ic = i < ntag ? i : ntag - 1;                 // lanes past the tags repeat the last tag's loads and store nothing
    const float NEG = -INFINITY;

    float tw[JW];
#pragma unroll
    for (int j = 0; j < JW; ++j) tw[j] = j0 + j < ntag ? trans[ic * ntag + j0 + j] : NEG;
    s_a[0][lane] = own ? (lane == start ? 0.f : -10000.f) : NEG;
    s_a[1][lane] = NEG;
    __syncthreads();

    // ---- forward, t = 0 .. n - 1: a_t[i] = em + log sum_j exp(prev[j] + tr[i][j]) - max(prev)
    float e_next = em[(long long)r0 * ntag + ic];
    for (int t = 0; t < n; ++t) {
        const float e = e_next;
        if (t + 1 < n) e_next = em[(long long)(r0 + t + 1) * ntag + ic];
        float mx, m2, s;
        lse_slice<JW>(s_a[t & 1] + j0, tw, mx, m2, s);
        lse_join<HALF>(mx, m2, s);
        const float a = e + crf_recentred(mx, m2, s);
        s_a[(t + 1) & 1][lane] = own ? a : NEG;
        if (own) ws[(long long)(r0 + t) * ntag + lane] = a;
        __syncthreads();
    }

    // ---- backward, t = n - 1 .. 0.  tw becomes the lane's slice of tag i's COLUMN: tw[k] = score of i -> j0 + k
#pragma unroll
    for (int k = 0; k < JW; ++k) tw[k] = j0 + k < ntag ? trans[(j0 + k) * ntag + ic] : NEG;
    float b = own ? trans[stop * ntag + lane] : NEG;        // beta of the last position: the transition to STOP
    long long row = (long long)(r0 + n - 1);
    float a_next = ws[row * ntag + ic], e_next_b = em[row * ntag + ic];
    // the path's tags, a tile of positions at a time and a tile ahead: lane k holds the tag of position top - k (yv) and of the
    // position in front of it (yq), top = the position of tile row 0; yc / qc are the same two clamped into the table
    const int last = ntag - 1;
    int yv = 0, yq = 0, yc = 0, qc = 0, yv_next, yq_next;
    {
        const int p = n - 1 - lane;
        yv_next = p >= 0 ? path[r0 + p] : 0;
        yq_next = p >= 1 ? path[r0 + p - 1] : 0;
    }
    float part = 0.f;                                       // lane k: (em_t + b_t)[y_t] - max - b_{t-1}[y_{t-1}] of tile row k
    int slot = 0;                                           // rows waiting in the tile: tile row k holds position t + slot - 1 - k
    for (int t = n - 1; t >= 0; --t) {
        const float a = a_next, e = e_next_b;
        if (t > 0) {
            row = (long long)(r0 + t - 1);
            a_next = ws[row * ntag + ic];
            e_next_b = em[row * ntag + ic];
        }
        if (slot == 0) {
            yv = yv_next;
            yq = yq_next;
            yc = min(max(yv, 0), last);
            qc = min(max(yq, 0), last);
            const int p = t - CRF_TILE_ROWS - lane;
            yv_next = p >= 0 ? path[r0 + p] : 0;
            yq_next = p >= 1 ? path[r0 + p - 1] : 0;
        }
        if (own) s_tile[slot * CRF_TILE_STRIDE + lane] = a + b;
        if (t > 0) {
            // beta of position t - 1, and what row t's conditional takes from the two vectors
            const int yt = __builtin_amdgcn_readlane(yc, slot), yp = __builtin_amdgcn_readlane(qc, slot);
            float* nbuf = s_a[t & 1];
            nbuf[lane] = own ? e + b : NEG;
            __syncthreads();
            float mx, m2, s;
            lse_slice<JW>(nbuf + j0, tw, mx, m2, s);
            lse_join<HALF>(mx, m2, s);
            const float nby = nbuf[yt];
            b = crf_recentred(mx, m2, s);
            const float bp = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), yp));     // (the builtin moves 32 bits as an integer)
            if (lane == slot) part = (nby - mx) - bp;
        }
        ++slot;
        if (slot == CRF_TILE_ROWS || t == 0) {
            __syncthreads();
            if (lane < slot) {                              // one lane per row: maximum and sum in tag order, the path's tag picked
                const float* p = s_tile + lane * CRF_TILE_STRIDE;
                const int pos = t + slot - 1 - lane;
                const bool in = (unsigned)yv < (unsigned)ntag;
                float mx = p[0];
                for (int k = 1; k < ntag; ++k) mx = fmaxf(mx, p[k]);
                float s = 0.f;
                for (int k = 0; k < ntag; ++k) s += expf(p[k] - mx);
                const float v = in ? (p[yc] - mx) - logf(s) : NEG;
                lm[r0 + pos] = v;
                float c = v;                                // the document's first row has no row in front: its conditional is its marginal
                if (pos > 0) c = in && (unsigned)yq < (unsigned)ntag ? trans[yc * ntag + qc] + part : NEG;
                lc[r0 + pos] = c;
            }
            slot = 0;
            __syncthreads();
        }
    }
}

// Training loss and gradient that hold at any length (vbg_crf_nll_stable): one wave per document, lane i owns tag i.
//
// Nothing that grows with the row index is ever formed.  The forward vectors are crf_posterior_kernel's: log space, the maximum of
// the previous vector taken out of every step and summed into log Z in double; on top of that every row of emissions is taken
// relative to its own maximum (a reduction off the chain, on a row fetched a step ahead; the maxima go into the same double).  The
// backward vectors are re-centred the same way.  The gradient never touches log Z: the pairwise table of step t,
//     x[i][j] = exp(a_{t-1}[j] + tr[i][j] + em_t[i] + b_t[i] - its own maximum),
// is divided by its own sum, lane i owning row i; the state marginal of row t is the row sum of that table and the transition
// gradient the sum of the tables over t in an fp64 accumulator in LDS (lane i owns row i of it).  The gold path is taken off as the
// tables go in: row t's indicator leaves entry [tags[t]][tags[t-1]] at step t.  The exponentials of a table are formed twice (once for
// its sum, once for the quotients) by the same code, so the two passes see the same bits: an image of the table next to the fp64
// accumulator and the transitions would not fit a static LDS allocation.
// The forward vectors wait in the rows of dem_unit: row t is written by the forward pass, read back by the same lane at backward
// step t + 1 (fetched during step t + 2) and overwritten with its gradient at step t.  A loss-only call stores no vector.
// Tags outside [0, ntag) match no lane and no column: no indicator, no emission term, no gold transition in or out of them.
constexpr int CRF_ST_STRIDE = CRF_MAX_TAGS + 1;            // odd row stride of the LDS images: lane i walking row i meets no bank conflict

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// log-sum-exp over n terms v[k] + w[k * step] of two LDS vectors, as (max, sum of exp(. - max)), with the maximum of v alone on the
// side: the forward step (w the lane's row of the transitions, step 1) and the beta step (its column, step CRF_ST_STRIDE)
__device__ __forceinline__ void lse_lds(const float* v, const float* w, int step, int n, float& mx, float& m2, float& s) {
    mx = v[0];
    m2 = v[0] + w[0];
    for (int k = 1; k < n; ++k) {
        mx = fmaxf(mx, v[k]);
        m2 = fmaxf(m2, v[k] + w[k * step]);
    }
    s = 0.f;
    for (int k = 0; k < n; ++k) s += expf((v[k] + w[k * step]) - m2);
}

// one entry of the pairwise table before its maximum is taken out; the ONE statement of this sum (three passes use it)
__device__ __forceinline__ float crf_pair_arg(float a_prev_j, float tr_ij, float nb_i) { return (a_prev_j + tr_ij) + nb_i; }

__global__ __launch_bounds__(64) void crf_nll_stable_kernel(const float* __restrict__ em, const int* __restrict__ tags,
                                                            const int* __restrict__ doc_off, const float* __restrict__ trans, int ntag,
                                                            int start, int stop, float* __restrict__ nll, float* __restrict__ logz,
                                                            float* dem_unit, float* __restrict__ dtrans_unit) {
    __shared__ float s_tr[CRF_MAX_TAGS * CRF_ST_STRIDE];
    __shared__ double s_acc[CRF_MAX_TAGS * CRF_ST_STRIDE];
    __shared__ float s_a[2][CRF_MAX_TAGS], s_nb[CRF_MAX_TAGS];
    const int d = blockIdx.x, lane = threadIdx.x;
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    const bool own = lane < ntag;
    const int ic = own ? lane : ntag - 1;                   // lanes past the tags repeat the last tag's loads and store nothing
    const bool grad = dem_unit != nullptr;
    const float NEG = -INFINITY;
    const float* trow = s_tr + ic * CRF_ST_STRIDE;          // the lane's row: trow[j] = score of j -> lane
    double* arow = s_acc + ic * CRF_ST_STRIDE;

    for (int k = lane; k < ntag * ntag; k += 64) {
        const int i = k / ntag, j = k - i * ntag;
        s_tr[i * CRF_ST_STRIDE + j] = trans[k];
        s_acc[i * CRF_ST_STRIDE + j] = 0.0;
    }
    s_a[0][lane] = own ? (lane == start ? 0.f : -10000.f) : NEG;
    __syncthreads();

    // ---- forward, t = 0 .. n - 1: a_t[i] = (em_t[i] - max em_t) + log sum_j exp(a_{t-1}[j] + tr[i][j]) - max(a_{t-1})
    double carry = 0.0;                                     // what has been taken out so far (the same in every lane)
    float e_next = n > 0 ? em[(long long)r0 * ntag + ic] : 0.f;
    for (int t = 0; t < n; ++t) {
        const float e = e_next;
        if (t + 1 < n) e_next = em[(long long)(r0 + t + 1) * ntag + ic];
        const float emax = wave_max(own ? e : NEG);
        float mx, m2, s;
        lse_lds(s_a[t & 1], trow, 1, ntag, mx, m2, s);
        const float a = (e - emax) + ((m2 - mx) + logf(s));
        carry += (double)mx + (double)emax;
        s_a[(t + 1) & 1][lane] = own ? a : NEG;
        if (grad && own) dem_unit[(long long)(r0 + t) * ntag + lane] = a;
        __syncthreads();
    }

    // ---- log Z (every lane forms the same value) and the gold score: lane l takes rows l, l + 64, ...; the sums are double
    const double zd = crf_log_z_end(s_a[n & 1], s_tr + stop * CRF_ST_STRIDE, ntag, carry);
    double gold = 0.0;
    for (int t = lane; t < n; t += 64) {
        const int ct = tags[r0 + t], pt = t > 0 ? tags[r0 + t - 1] : start;
        const bool cin = (unsigned)ct < (unsigned)ntag, pin = (unsigned)pt < (unsigned)ntag;
        if (cin) gold += (double)em[(long long)(r0 + t) * ntag + ct];
        if (cin && pin) gold += (double)s_tr[ct * CRF_ST_STRIDE + pt];
        if (t == n - 1 && cin) gold += (double)s_tr[stop * CRF_ST_STRIDE + ct];
    }
    gold = wave_sum_f64(gold);
    if (lane == 0) {
        logz[d] = (float)zd;
        nll[d] = n > 0 ? (float)((zd - gold) / (double)n) : 0.f;
    }
    if (!grad) return;

    // ---- backward + both gradients, t = n - 1 .. 0
    float b = 0.f;                                          // beta of the last position: the transition to STOP, less its maximum
    if (n > 0) {
        const float bs = own ? s_tr[stop * CRF_ST_STRIDE + lane] : NEG;
        b = bs - wave_max(bs);
    }
    float e_nx = 0.f, a_nx = 0.f;                           // emission of row t and forward vector of row t - 1, a step ahead
    int ct_nx = -1, pt_nx = -1;
    if (n > 0) {
        e_nx = em[(long long)(r0 + n - 1) * ntag + ic];
        ct_nx = tags[r0 + n - 1];
        pt_nx = n > 1 ? tags[r0 + n - 2] : start;
        a_nx = n > 1 ? dem_unit[(long long)(r0 + n - 2) * ntag + ic] : (ic == start ? 0.f : -10000.f);
    }
    for (int t = n - 1; t >= 0; --t) {
        const float e = e_nx, ap = a_nx;
        const int ct = ct_nx, pt = pt_nx;
        if (t > 0) {
            e_nx = em[(long long)(r0 + t - 1) * ntag + ic];
            ct_nx = pt;
            pt_nx = t > 1 ? tags[r0 + t - 2] : start;
            a_nx = t > 1 ? dem_unit[(long long)(r0 + t - 2) * ntag + ic] : (ic == start ? 0.f : -10000.f);
        }
        const float emax = wave_max(own ? e : NEG);
        const float nb = (e - emax) + b;                    // emission of t + everything after it, for the lane's tag
        float* avec = s_a[t & 1];
        avec[lane] = own ? ap : NEG;
        s_nb[lane] = own ? nb : NEG;
        __syncthreads();
        // the table's maximum and sum
        float rm = NEG;
        if (own)
            for (int j = 0; j < ntag; ++j) rm = fmaxf(rm, crf_pair_arg(avec[j], trow[j], nb));
        const float M = wave_max(rm);
        float rs = 0.f;
        if (own)
            for (int j = 0; j < ntag; ++j) rs += expf(crf_pair_arg(avec[j], trow[j], nb) - M);
        const float S = wave_sum(rs);
        // the quotients: into the accumulator less the gold transition, their row sum into the state marginal
        float p = 0.f;
        if (own) {
            for (int j = 0; j < ntag; ++j) {
                const float q = expf(crf_pair_arg(avec[j], trow[j], nb) - M) / S;
                p += q;
                arow[j] += (double)q - ((lane == ct && j == pt) ? 1.0 : 0.0);
            }
            dem_unit[(long long)(r0 + t) * ntag + lane] = p - (lane == ct ? 1.f : 0.f);
        }
        if (t == n - 1) {                                   // the terminal transition i -> STOP: row STOP of the accumulator
            __syncthreads();
            if (own) s_acc[stop * CRF_ST_STRIDE + lane] += (double)p - (lane == ct ? 1.0 : 0.0);
        }
        if (t > 0) {
            // beta of position t - 1: b[j] = log sum_k exp(tr[k][j] + nb[k]) - max(nb), the lane's COLUMN of the transitions
            float mx, m2, s;
            lse_lds(s_nb, s_tr + ic, CRF_ST_STRIDE, ntag, mx, m2, s);
            b = (m2 - mx) + logf(s);
        }
        __syncthreads();
    }
    for (int k = lane; k < ntag * ntag; k += 64) {
        const int i = k / ntag, j = k - i * ntag;
        dtrans_unit[(long long)d * ntag * ntag + k] = (float)s_acc[i * CRF_ST_STRIDE + j];
    }
}

// demissions = (gout[d] / n_d) * dem_unit over the rows of every document, and dtrans += the scaled blocks in document order.
// Blocks 0 .. tr_blocks - 1 own the transition entries (one thread per entry walks the documents: a fixed order, no atomics);
// block tr_blocks + d * CRF_ST_CHUNKS + c takes every CRF_ST_CHUNKS-th 256-element slice of document d's rows.
constexpr int CRF_ST_CHUNKS = 8;

__global__ __launch_bounds__(256) void crf_nll_stable_bwd_kernel(const float* __restrict__ dem_unit, const float* __restrict__ dtrans_unit,
                                                                 const int* __restrict__ doc_off, int ndoc, int ntag, int tr_blocks,
                                                                 const float* __restrict__ gout, float* __restrict__ dem,
                                                                 float* __restrict__ dtrans) {
    // product and sum are rounded one after the other, never fused into one multiply-add: the ordered fp32 sum of the scaled blocks
#pragma clang fp contract(off)
    const int nn = ntag * ntag;
    if ((int)blockIdx.x < tr_blocks) {
        const int k = blockIdx.x * 256 + threadIdx.x;
        if (k >= nn) return;
        float acc = dtrans[k];
        for (int d = 0; d < ndoc; ++d) {
            const int n = doc_off[d + 1] - doc_off[d];
            if (n <= 0) continue;
            const float scaled = (gout[d] / (float)n) * dtrans_unit[(long long)d * nn + k];
            acc = acc + scaled;
        }
        dtrans[k] = acc;
        return;
    }
    const int bb = blockIdx.x - tr_blocks;
    const int d = bb / CRF_ST_CHUNKS, c = bb - d * CRF_ST_CHUNKS;
    const int r0 = doc_off[d], n = doc_off[d + 1] - r0;
    if (n <= 0) return;
    const float g = gout[d] / (float)n;
    const long long base = (long long)r0 * ntag, total = (long long)n * ntag;
    for (long long e = (long long)c * 256 + threadIdx.x; e < total; e += CRF_ST_CHUNKS * 256) dem[base + e] = g * dem_unit[base + e];
}

}  // namespace vbg

using namespace vbg;
#define S_ ((hipStream_t)stream)

// the tag range every entry holds its arguments to; min_ntag is the entry's own lower bound
static inline bool crf_tags_ok(int min_ntag, int ntag, int start_tag, int stop_tag) {
    return ntag >= min_ntag && ntag <= CRF_MAX_TAGS && start_tag >= 0 && start_tag < ntag && stop_tag >= 0 && stop_tag < ntag;
}

// a wave kernel's instance for ntag: two lanes per tag up to 32 tags, the template size the next multiple of 8 / 16
#define VBG_CRF_DISPATCH(KERNEL, ...)                                                              \
    do {                                                                                           \
        if (ntag <= 8) VBG_LAUNCH((KERNEL<8, true>), dim3(ndoc), dim3(64), 0, S_, __VA_ARGS__);           \
        else if (ntag <= 16) VBG_LAUNCH((KERNEL<16, true>), dim3(ndoc), dim3(64), 0, S_, __VA_ARGS__);    \
        else if (ntag <= 32) VBG_LAUNCH((KERNEL<32, true>), dim3(ndoc), dim3(64), 0, S_, __VA_ARGS__);    \
        else if (ntag <= 48) VBG_LAUNCH((KERNEL<48, false>), dim3(ndoc), dim3(64), 0, S_, __VA_ARGS__);   \
        else VBG_LAUNCH((KERNEL<64, false>), dim3(ndoc), dim3(64), 0, S_, __VA_ARGS__);                   \
    } while (0)

extern "C" int vbg_crf_nll_fwd(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                               int start_tag, int stop_tag, float* alpha, float* logz, float* nll, void* stream) {
    VBG_CHECK_ARG(emissions && tags && doc_off && trans && alpha && logz && nll && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(2, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    VBG_LAUNCH(crf_nll_fwd_kernel, dim3(ndoc), dim3(64), 0, S_, emissions, tags, doc_off, trans, ntag, start_tag, stop_tag, alpha, logz,
               nll);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_nll_bwd(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                               int start_tag, int stop_tag, const float* alpha, const float* logz, const float* gout, float* demissions,
                               float* dtrans_accum, void* stream) {
    VBG_CHECK_ARG(emissions && tags && doc_off && trans && alpha && logz && gout && demissions && dtrans_accum && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(2, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    VBG_LAUNCH(crf_nll_bwd_kernel, dim3(ndoc), dim3(64), 0, S_, emissions, tags, doc_off, trans, ntag, start_tag, stop_tag, alpha, logz,
               gout, demissions, dtrans_accum, (float*)nullptr);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_nll_bwd_det(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                                   int start_tag, int stop_tag, const float* alpha, const float* logz, const float* gout, float* demissions,
                                   float* dtrans_part, void* stream) {
    VBG_CHECK_ARG(emissions && tags && doc_off && trans && alpha && logz && gout && demissions && dtrans_part && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(2, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    VBG_LAUNCH(crf_nll_bwd_kernel, dim3(ndoc), dim3(64), 0, S_, emissions, tags, doc_off, trans, ntag, start_tag, stop_tag, alpha, logz,
               gout, demissions, (float*)nullptr, dtrans_part);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_viterbi(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                               int stop_tag, int* backptr, int* path, float* score, void* stream) {
    VBG_CHECK_ARG(emissions && doc_off && trans && backptr && path && score && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(2, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    VBG_LAUNCH(crf_viterbi_kernel, dim3(ndoc), dim3(64), 0, S_, emissions, doc_off, trans, ntag, start_tag, stop_tag, backptr, path, score);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_posterior(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                                 int stop_tag, void* ws, int* path, float* score, float* logz, float* marginals, void* stream) {
    VBG_CHECK_ARG(emissions && doc_off && trans && ws && path && score && logz && marginals && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(2, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    float* w = static_cast<float*>(ws);
    VBG_CRF_DISPATCH(crf_posterior_kernel, emissions, doc_off, trans, ntag, start_tag, stop_tag, w, path, score, logz, marginals);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_path_logp(const float* emissions, const int* doc_off, int ndoc, const float* trans, int ntag, int start_tag,
                                 int stop_tag, const int* path, void* ws, float* lm, float* lc, void* stream) {
    VBG_CHECK_ARG(doc_off && trans && ndoc >= 0);
    VBG_CHECK_ARG(crf_tags_ok(1, ntag, start_tag, stop_tag));
    if (ndoc == 0) return VBG_OK;
    VBG_CHECK_ARG(emissions && path && ws && lm && lc);
    float* w = static_cast<float*>(ws);
    VBG_CRF_DISPATCH(crf_path_logp_kernel, emissions, doc_off, trans, ntag, start_tag, stop_tag, path, w, lm, lc);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_nll_stable(const float* emissions, const int* tags, const int* doc_off, int ndoc, const float* trans, int ntag,
                                  int start_tag, int stop_tag, float* nll, float* logz, float* dem_unit, float* dtrans_unit, void* stream) {
    VBG_CHECK_ARG(crf_tags_ok(1, ntag, start_tag, stop_tag));
    VBG_CHECK_ARG(ndoc >= 0 && (dem_unit == nullptr) == (dtrans_unit == nullptr));
    if (ndoc == 0) return VBG_OK;
    VBG_CHECK_ARG(emissions && tags && doc_off && trans && nll && logz);
    VBG_LAUNCH(crf_nll_stable_kernel, dim3(ndoc), dim3(64), 0, S_, emissions, tags, doc_off, trans, ntag, start_tag, stop_tag, nll, logz,
               dem_unit, dtrans_unit);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_crf_nll_stable_bwd(const float* dem_unit, const float* dtrans_unit, const int* doc_off, int ndoc, int ntag,
                                      const float* gout, float* demissions, float* dtrans_accum, void* stream) {
    VBG_CHECK_ARG(ntag >= 1 && ntag <= CRF_MAX_TAGS && ndoc >= 0);
    if (ndoc == 0) return VBG_OK;
    VBG_CHECK_ARG(dem_unit && dtrans_unit && doc_off && gout && demissions && dtrans_accum);
    const int tr_blocks = cdiv(ntag * ntag, 256);
    VBG_LAUNCH(crf_nll_stable_bwd_kernel, dim3(tr_blocks + ndoc * CRF_ST_CHUNKS), dim3(256), 0, S_, dem_unit, dtrans_unit, doc_off, ndoc,
               ntag, tr_blocks, gout, demissions, dtrans_accum);
    VBG_LAUNCH_RET();
}
