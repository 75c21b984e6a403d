// Sampling and hard-example selection on the device, for the sampled / OHEM cross-entropy losses of the reference
// (pipeline/custom_loss.py:62-88 `ce_loss[mask]` + `random.sample(range(n), k)`, :143-190 the OHEM pre-sample, sort and
// `sorted_loss[sorted_index[:k]]`).  The host route (loss.hip + pipeline/custom_loss.py) needs the size of every label category on the
// host to call `random.sample`; here every list has a capacity the host knows (k, or 2k for OHEM) and a count that stays in device memory.
//
// vbg_sample_select: element i of category c carries the key rng_u64(seed, stream0 + c, i) -- 64 bits, distinct for distinct i.  The k
// smallest keys of a category are a uniformly random ordered sample of it.  They are found exactly by a radix selection on the key,
// most significant digit first:
//   1. sample_hist_kernel     one sweep over the labels: per category, the histogram of the key's top 11 bits (LDS bins, flushed with
//                             integer atomics -- sums, so their order cannot show).  Its total is n_c.
//   2. sample_collect_kernel  every block finds the bin b_c holding the k_c-th key (all bins when n_c <= k_c) and appends the elements
//                             of bins <= b_c to the category's candidate list (slot claims by atomics: the list is an unordered SET,
//                             everything after it is independent of its order).  About k + N / 2048 candidates; capacity N.
//   3. sample_finish_kernel   one workgroup per category narrows the k-th key digit by digit over the candidates, however many there
//                             are (five more histogram passes over 11, 11, 11, 11 and 9 bits), collects the <= 4096 elements at or
//                             below it into LDS, sorts them (bitonic; by key, or by element index when everything is kept) and writes.
// vbg_ohem_topk: one workgroup per bounded list: losses by ce_elem_loss (the arithmetic of ce_fwd_kernel), a bitonic sort of
// (loss descending, position ascending) -- the permutation a stable descending sort gives -- and the reference's double indexing.
// No vendor primitive, no float atomics, vector stores only.
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

constexpr int SMP_BINS = 2048;            // 11 bits per digit
constexpr int SMP_TOP_SHIFT = 53;         // the first digit: bits 63 ... 53
constexpr int SMP_THREADS = 512;          // sweeps
constexpr int SMP_FIN_THREADS = 1024;     // finishing / OHEM workgroups
constexpr int SMP_MAX_K = VBG_SAMPLE_MAX_K;
constexpr int SMP_HDR_INTS = VBG_SAMPLE_MAX_CATS * SMP_BINS + 64;      // workspace header: histograms, then candidate counts

__device__ __forceinline__ bool cat_match(const vbg_sample_cat& c, int label) { return (label == c.value) == (c.eq != 0); }

// Block-wide search in a histogram of SMP_BINS bins (LDS or global): the smallest bin b whose inclusive prefix sum reaches `need`
// (1 <= need <= total), and the sum below b.  blockDim.x divides SMP_BINS and is a multiple of 64; sh has >= 18 ints.  Every thread
// returns the same pair.
__device__ __forceinline__ int2 find_bin(const int* hist, int need, int* sh) {
    const int per = SMP_BINS / (int)blockDim.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int* mine = hist + threadIdx.x * per;
    int own = 0;
    for (int j = 0; j < per; ++j) own += mine[j];
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    __syncthreads();
    if (lane == 63) sh[w] = incl;
    __syncthreads();
    int excl = incl - own;
    for (int i = 0; i < w; ++i) excl += sh[i];
    if (excl < need && need <= excl + own) {          // exactly one thread
        int c = excl, j = 0;
        while (c + mine[j] < need) c += mine[j++];
        sh[16] = threadIdx.x * per + j;
        sh[17] = c;
    }
    __syncthreads();
    const int2 r = make_int2(sh[16], sh[17]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ int block_total(const int* hist, int* sh) {
    int s = 0;
    for (int j = threadIdx.x; j < SMP_BINS; j += blockDim.x) s += hist[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    int t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(SMP_THREADS) void sample_hist_kernel(const int* __restrict__ labels, long long N, int ncat, vbg_sample_cats cats,
                                                                  uint64_t seed, uint64_t stream0, int* __restrict__ ghist) {
    __shared__ int hist[VBG_SAMPLE_MAX_CATS * SMP_BINS];
    for (int j = threadIdx.x; j < ncat * SMP_BINS; j += blockDim.x) hist[j] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        const int t = labels[i];
        for (int c = 0; c < ncat; ++c)
            if (cat_match(cats.c[c], t)) atomicAdd(&hist[c * SMP_BINS + (int)(rng_u64(seed, stream0 + c, (uint64_t)i) >> SMP_TOP_SHIFT)], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ncat * SMP_BINS; j += blockDim.x)
        if (hist[j]) atomicAdd(&ghist[j], hist[j]);
}

__global__ __launch_bounds__(SMP_THREADS) void sample_collect_kernel(const int* __restrict__ labels, long long N, int ncat, vbg_sample_cats cats,
                                                                     uint64_t seed, uint64_t stream0, const int* __restrict__ ghist,
                                                                     int* __restrict__ cand_count, int* __restrict__ cand) {
    __shared__ int sh[18];
    __shared__ int last_bin[VBG_SAMPLE_MAX_CATS];
    for (int c = 0; c < ncat; ++c) {
        const int* h = ghist + c * SMP_BINS;
        const int n = block_total(h, sh), k = cats.c[c].k;
        const int b = n > k ? find_bin(h, k, sh).x : SMP_BINS - 1;
        if (threadIdx.x == 0) last_bin[c] = b;
    }
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        const int t = labels[i];
        for (int c = 0; c < ncat; ++c) {
            if (!cat_match(cats.c[c], t)) continue;
            if ((int)(rng_u64(seed, stream0 + c, (uint64_t)i) >> SMP_TOP_SHIFT) > last_bin[c]) continue;
            const int slot = atomicAdd(&cand_count[c], 1);
            if (slot < N) cand[(long long)c * N + slot] = (int)i;          // (every element claims at most one slot per category)
        }
    }
}

// (key, index) ascending; the pad entries (all ones, INT_MAX) stay behind every real one
__device__ __forceinline__ bool pair_gt(uint64_t ka, int ia, uint64_t kb, int ib) { return ka > kb || (ka == kb && ia > ib); }

// bitonic sort of the first P (a power of two) entries of (skey, sidx), ascending, by the whole block
__device__ __forceinline__ void bitonic_pairs(uint64_t* skey, int* sidx, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint64_t ki = skey[i], kj = skey[j];
                const int xi = sidx[i], xj = sidx[j];
                if (pair_gt(ki, xi, kj, xj) == up) { skey[i] = kj; skey[j] = ki; sidx[i] = xj; sidx[j] = xi; }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(SMP_FIN_THREADS) void sample_finish_kernel(long long N, vbg_sample_cats cats, uint64_t seed, uint64_t stream0,
                                                                        const int* __restrict__ ghist, const int* __restrict__ cand_count,
                                                                        const int* __restrict__ cand, int* __restrict__ out_idx,
                                                                        int* __restrict__ out_keep, int* __restrict__ out_n) {
    __shared__ uint64_t skey[SMP_MAX_K];
    __shared__ int sidx[SMP_MAX_K];
    __shared__ int hist[SMP_BINS];
    __shared__ int sh[18];
    __shared__ int nsel;
    const int c = blockIdx.x, k = cats.c[c].k;
    int off = 0;
    for (int j = 0; j < c; ++j) off += cats.c[j].k;
    const int* h0 = ghist + c * SMP_BINS;
    const int n = block_total(h0, sh);
    const int keep = min(n, k);
    const long long M = min((long long)cand_count[c], N);
    const int* cd = cand + (long long)c * N;
    const uint64_t strm = stream0 + c;
    if (threadIdx.x == 0) { out_keep[c] = keep; out_n[c] = n; nsel = 0; }
    if (keep == 0) return;
    const bool sample = n > k;
    uint64_t thresh = ~0ull;                      // keep everything
    if (sample) {
        // the k-th smallest key, digit by digit: `prefix` holds the digits found so far (the key's bits above hi_shift)
        int2 r = find_bin(h0, k, sh);
        uint64_t prefix = (uint64_t)r.x;
        int need = k - r.y, hi_shift = SMP_TOP_SHIFT;
        while (hi_shift > 0) {
            const int shift = hi_shift >= 11 ? hi_shift - 11 : 0;
            const uint64_t mask = (1ull << (hi_shift - shift)) - 1;
            for (int j = threadIdx.x; j < SMP_BINS; j += blockDim.x) hist[j] = 0;
            __syncthreads();
            for (long long j = threadIdx.x; j < M; j += blockDim.x) {
                const uint64_t key = rng_u64(seed, strm, (uint64_t)cd[j]);
                if ((key >> hi_shift) == prefix) atomicAdd(&hist[(int)((key >> shift) & mask)], 1);
            }
            __syncthreads();
            r = find_bin(hist, need, sh);
            prefix = (prefix << (hi_shift - shift)) | (uint64_t)r.x;
            need -= r.y;
            hi_shift = shift;
        }
        thresh = prefix;                          // exactly k keys of the category are <= thresh (keys are distinct)
    }
    __syncthreads();
    for (long long j = threadIdx.x; j < M; j += blockDim.x) {
        const int i = cd[j];
        const uint64_t key = rng_u64(seed, strm, (uint64_t)i);
        if (key <= thresh) {
            const int slot = atomicAdd(&nsel, 1);
            // all kept: ascending element index (the reference's compaction order); sampled: ascending key
            if (slot < SMP_MAX_K) { skey[slot] = sample ? key : (uint64_t)i; sidx[slot] = i; }
        }
    }
    __syncthreads();
    int P = 1;
    while (P < keep) P <<= 1;
    for (int j = keep + threadIdx.x; j < P; j += blockDim.x) { skey[j] = ~0ull; sidx[j] = 0x7fffffff; }
    bitonic_pairs(skey, sidx, P);
    for (int j = threadIdx.x; j < keep; j += blockDim.x) out_idx[off + j] = sidx[j];
}

__global__ __launch_bounds__(SMP_FIN_THREADS) void ohem_topk_kernel(const float* __restrict__ logits, long long ld, int ncls,
                                                                    const int* __restrict__ elem, const int* __restrict__ m_dev,
                                                                    vbg_ohem_cats cats, const int* __restrict__ labels,
                                                                    const float* __restrict__ weight, int up_shift, int H, int W,
                                                                    int* __restrict__ out, int* __restrict__ out_keep) {
    __shared__ uint64_t skey[SMP_MAX_K];
    const int c = blockIdx.x, cap = cats.c[c].cap, k = cats.c[c].k;
    int off = 0;
    for (int j = 0; j < c; ++j) off += cats.c[j].cap;
    const int m = min(max(m_dev[c], 0), cap), keep = min(m, k);
    const int* el = elem + off;
    if (threadIdx.x == 0) out_keep[c] = keep;
    if (keep >= m) {
        for (int j = threadIdx.x; j < m; j += blockDim.x) out[off + j] = el[j];
        return;
    }
    int P = 1;
    while (P < m) P <<= 1;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        uint64_t key = ~0ull;
        if (p < m) {
            const int e = el[p];
            const unsigned b = __float_as_uint(ce_elem_loss(logits, ld, ncls, e, labels[e], weight, up_shift, H, W));
            // ascending radix code of a float (sign bit set: all bits flipped; clear: sign bit set), complemented for descending
            // order: the total order of vbg_sort_desc's keys; the position below it makes the sort stable
            const unsigned asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            key = ((uint64_t)(~asc) << 32) | (unsigned)p;
        }
        skey[p] = key;
    }
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t ki = skey[i], kj = skey[j];
                if ((ki > kj) == ((i & size) == 0)) { skey[i] = kj; skey[j] = ki; }
            }
        }
    __syncthreads();
    // si[r] = (int)skey[r]; the reference's sorted_loss[sorted_index[:k]]: rank r takes the element at position si[si[r]]
    for (int r = threadIdx.x; r < keep; r += blockDim.x) out[off + r] = el[(unsigned)skey[(unsigned)skey[r]]];
}

static inline int sweep_grid(long long n) {
    long long g = (n + SMP_THREADS * 16 - 1) / (SMP_THREADS * 16);
    return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

}  // namespace vbg

using namespace vbg;
#define S_ ((hipStream_t)stream)

extern "C" long long vbg_sample_ws_bytes(long long N, int ncat, long long ksum) {
    if (N < 0 || ncat < 1 || ncat > VBG_SAMPLE_MAX_CATS || ksum < 0) return -1;
    return ((long long)SMP_HDR_INTS + (long long)ncat * N) * (long long)sizeof(int);
}

extern "C" int vbg_sample_select(const int* labels, long long N, int ncat, vbg_sample_cats cats, unsigned long long seed,
                                 unsigned long long stream0, int* out_idx, int* out_keep, int* out_n, void* ws, long long ws_bytes,
                                 void* stream) {
    VBG_CHECK_ARG(N >= 0 && N < 2147483647LL && ncat >= 1 && ncat <= VBG_SAMPLE_MAX_CATS);
    long long ksum = 0;
    for (int c = 0; c < ncat; ++c) {
        VBG_CHECK_ARG(cats.c[c].k >= 1 && cats.c[c].k <= VBG_SAMPLE_MAX_K);
        ksum += cats.c[c].k;
    }
    VBG_CHECK_ARG(out_idx && out_keep && out_n && ws && ws_bytes >= vbg_sample_ws_bytes(N, ncat, ksum));
    VBG_CHECK_ARG(N == 0 || labels);
    int* ghist = (int*)ws;
    int* cand_count = ghist + VBG_SAMPLE_MAX_CATS * SMP_BINS;
    int* cand = ghist + SMP_HDR_INTS;
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)SMP_HDR_INTS * sizeof(int), S_);
    if (e != hipSuccess) return (int)e;
    if (N > 0) {
        VBG_LAUNCH(sample_hist_kernel, dim3(sweep_grid(N)), dim3(SMP_THREADS), 0, S_, labels, N, ncat, cats, (uint64_t)seed, (uint64_t)stream0, ghist);
        VBG_LAUNCH(sample_collect_kernel, dim3(sweep_grid(N)), dim3(SMP_THREADS), 0, S_, labels, N, ncat, cats, (uint64_t)seed, (uint64_t)stream0,
                   ghist, cand_count, cand);
    }
    VBG_LAUNCH(sample_finish_kernel, dim3(ncat), dim3(SMP_FIN_THREADS), 0, S_, N, cats, (uint64_t)seed, (uint64_t)stream0, ghist, cand_count,
               cand, out_idx, out_keep, out_n);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_ohem_topk(const float* logits, long long ld, int ncls, const int* elem, const int* m_dev, int ncat, vbg_ohem_cats cats,
                             const int* labels, const float* weight, int up_shift, int H, int W, int* out, int* out_keep, void* stream) {
    VBG_CHECK_ARG(ncat >= 1 && ncat <= VBG_SAMPLE_MAX_CATS && ncls > 0 && up_shift >= 0);
    for (int c = 0; c < ncat; ++c) VBG_CHECK_ARG(cats.c[c].cap >= 1 && cats.c[c].cap <= VBG_SAMPLE_MAX_K && cats.c[c].k >= 1);
    VBG_CHECK_ARG(logits && elem && m_dev && labels && out && out_keep);
    VBG_LAUNCH(ohem_topk_kernel, dim3(ncat), dim3(SMP_FIN_THREADS), 0, S_, logits, ld, ncls, elem, m_dev, cats, labels, weight, up_shift, H, W,
               out, out_keep);
    VBG_LAUNCH_RET();
}
