// Per-parameter statistics of a flat fp32 buffer (vbg.stats.ParamStats): which parameter overflowed, how large each layer's gradient
// is, and how much of a tensor has left the range the fp16-pair forms assume -- one row pass per buffer and one finish, in place of a
// torch loop of a few hundred tiny launches and a host read per quantity.
// The row pass walks a table of vbg_optim_chunk rows whose `group` is the parameter index (blocks stride over the rows, as the
// optimizer steps do) and leaves ONE vbg_stats_rec per row with a plain store; the finish gives every parameter one block, which adds
// that parameter's records in a fixed order.  No atomics on device memory anywhere, nothing to zero beforehand: the same bits on every
// call, so deterministic mode needs no form of its own.
// Every count of a row comes out of one table in LDS: an element adds 1 to exactly one SLOT -- its binade (0..63), or "zero", or
// "inf / NaN", or "[65520, 65536)", the part of binade 61 that an fp16 piece turns into inf -- so the loop costs one LDS add per
// element and no counter registers.  Gradients of one tensor sit in a handful of binades: 64 lanes adding to one word would
// serialise.  The table therefore has 32 COPIES of every slot, copy = lane & 31, word = slot * 32 + copy: the 32 lanes the LDS serves
// per cycle always hit 32 different banks, whatever their slots are, and lanes l and l + 32 (same word when their slots agree) are
// served in different cycles.  (A ballot loop over the distinct binades of a wave -- first lane's bin, ballot, popc, retire -- was
// the other candidate: ~12 scalar/vector instructions per distinct binade and float4 component, above what a SIMD can spend per 64
// elements at HBM rate once a wave spans more than ~6 binades.)  After the row's loop the block folds the 32 copies of every slot,
// zeroing them for the next row; integer sums make the result independent of the order.
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

constexpr int ST_THREADS = 256;
constexpr int ST_COPIES = 32;
constexpr int ST_BINS = 64;
constexpr int ST_ZERO = 64, ST_NONFINITE = 65, ST_OVER61 = 66, ST_SLOTS = 67;
constexpr unsigned ST_INF_BITS = 0x7f800000u;
constexpr unsigned ST_F16_OVER_BITS = 0x477ff000u;          // 65520.0f: the smallest fp32 that rounds to inf in fp16
constexpr unsigned ST_TWO16_BITS = 0x47800000u;             // 65536.0f: the upper edge of binade 61

static_assert(sizeof(vbg_stats_rec) == 288 && sizeof(vbg_stats_total) == 568, "include/vbg.h layout");

// a = the bit pattern of |v|.  bin = clamp(e + 46, 0, 63) with e = (a >> 23) - 127 (an fp32 subnormal has exponent field 0: -127)
__device__ __forceinline__ int stats_slot(unsigned a) {
    if (a == 0u) return ST_ZERO;
    if (a >= ST_INF_BITS) return ST_NONFINITE;
    if (a >= ST_F16_OVER_BITS && a < ST_TWO16_BITS) return ST_OVER61;
    const int b = (int)(a >> 23) - 81;
    return b < 0 ? 0 : (b > ST_BINS - 1 ? ST_BINS - 1 : b);
}

// sum over the block in a fixed order: the wave's tree, then the waves in index order.  `sh` has >= 4 doubles; result broadcast.
__device__ __forceinline__ double stats_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ unsigned stats_block_max(unsigned v, unsigned* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = sh[0];
    for (int i = 1; i < ST_THREADS / 64; ++i) r = sh[i] > r ? sh[i] : r;
    return r;
}

__global__ void __launch_bounds__(ST_THREADS) param_stats_rows_kernel(const float* __restrict__ x, const vbg_optim_chunk* __restrict__ tbl, int nrows,
                                                                       const float* __restrict__ scale, vbg_stats_rec* __restrict__ recs) {
    __shared__ int H[ST_SLOTS * ST_COPIES];
    __shared__ int tot[ST_SLOTS];
    __shared__ double shd[ST_THREADS / 64];
    __shared__ unsigned shu[ST_THREADS / 64];
    const int t = threadIdx.x;
    const int copy = t & (ST_COPIES - 1);
    const bool scaled = scale != nullptr;
    const float inv = scaled ? (float)(1.0 / (double)*scale) : 1.f;
    for (int i = t; i < ST_SLOTS * ST_COPIES; i += ST_THREADS) H[i] = 0;
    __syncthreads();
    for (int c = blockIdx.x; c < nrows; c += (int)gridDim.x) {
        const vbg_optim_chunk ch = tbl[c];
        const float4* x4 = reinterpret_cast<const float4*>(x + ch.start);
        const int n4 = (ch.length + 3) >> 2;
        double acc = 0.0;
        unsigned mx = 0u;
        // one element: classified and summed as v = x * inv (one rounded product; the element itself without a scale); a lane at or
        // beyond the row's length enters nothing
        auto one = [&](float xv, int idx) {
            const float v = scaled ? __fmul_rn(xv, inv) : xv;
            const unsigned a = __float_as_uint(v) & 0x7fffffffu;
            if (idx < ch.length) {
                atomicAdd(&H[stats_slot(a) * ST_COPIES + copy], 1);
                if (a < ST_INF_BITS) {
                    const double d = (double)v;
                    acc = fma(d, d, acc);          // (the product is exact in double: one rounding, the sum's)
                    mx = a > mx ? a : mx;
                }
            }
        };
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = t; i < n4; i += ST_THREADS) {
            const float4 v = x4[i];
            one(v.x, 4 * i);
            one(v.y, 4 * i + 1);
            one(v.z, 4 * i + 2);
            one(v.w, 4 * i + 3);
        }
        __syncthreads();
        // the 32 copies of every slot folded and zeroed: thread -> (slot t / 4, a quarter of its copies, rotated by the slot so that
        // the lanes of a wave spread over the banks), then the three extra slots, one copy per thread of the first 96
        {
            const int slot = t >> 2, q = t & 3;
            int s = 0;
#pragma unroll
            for (int j = 0; j < ST_COPIES / 4; ++j) {
                const int w = slot * ST_COPIES + ((q * (ST_COPIES / 4) + j + slot) & (ST_COPIES - 1));
                s += H[w];
                H[w] = 0;
            }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (q == 0) tot[slot] = s;
            int e = 0;
            if (t < (ST_SLOTS - ST_BINS) * ST_COPIES) {
                e = H[ST_BINS * ST_COPIES + t];
                H[ST_BINS * ST_COPIES + t] = 0;
            }
#pragma unroll
            for (int o = ST_COPIES / 2; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
            if (t < (ST_SLOTS - ST_BINS) * ST_COPIES && copy == 0) tot[ST_BINS + (t >> 5)] = e;
        }
        const double sumsq = stats_block_sum(acc, shd);
        const unsigned amax = stats_block_max(mx, shu);          // (its barriers also publish tot[])
        vbg_stats_rec* r = recs + c;
        if (t < ST_BINS) r->hist[t] = tot[t] + (t == 61 ? tot[ST_OVER61] : 0);
        if (t == ST_BINS) {
            r->sumsq = sumsq;
            r->amax_bits = amax;
            r->nonfinite = tot[ST_NONFINITE];
            r->zeros = tot[ST_ZERO];
            r->over_f16 = tot[ST_OVER61] + tot[62] + tot[63];
            r->pad[0] = 0;
            r->pad[1] = 0;
        }
        // (the next row's first barrier stands between these reads of tot[] and its next writes)
    }
}

// One block per parameter (blocks stride over the parameters): the records of rows [row_ptr[p], row_ptr[p + 1]) added in a fixed
// order -- the bins by thread (bin t % 64, every sixteenth row from t / 64), the scalars by a lane-strided walk and a fixed tree.
// The longest parameter sets the launch's time (bert-base's word embeddings: 5 723 rows of 4 096 for one block), so the block is as
// wide as a block gets and the bin walk keeps four independent loads in flight per thread.
constexpr int FIN_THREADS = 1024;
constexpr int FIN_GROUPS = FIN_THREADS / 64;

template <class T, class Op>
__device__ __forceinline__ T stats_tree(T v, T* sh, Op op) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(FIN_THREADS) param_stats_finish_kernel(const vbg_stats_rec* __restrict__ recs, const int* __restrict__ row_ptr, int nparams,
                                                                          vbg_stats_rec* __restrict__ last, vbg_stats_total* __restrict__ total) {
    __shared__ double shd[FIN_THREADS];
    __shared__ long long shl[FIN_THREADS];
    const int t = threadIdx.x;
    for (int p = blockIdx.x; p < nparams; p += (int)gridDim.x) {
        const int r0 = row_ptr[p], r1 = row_ptr[p + 1];
        long long h = 0;
        {
            const int bin = t & 63;
            int r = r0 + (t >> 6);
            for (; r + 3 * FIN_GROUPS < r1; r += 4 * FIN_GROUPS) {
                const int a = recs[r].hist[bin], b = recs[r + FIN_GROUPS].hist[bin], c = recs[r + 2 * FIN_GROUPS].hist[bin],
                          d = recs[r + 3 * FIN_GROUPS].hist[bin];
                h += ((long long)a + b) + ((long long)c + d);
            }
            for (; r < r1; r += FIN_GROUPS) h += recs[r].hist[bin];
        }
        double s = 0.0;
        long long mx = 0, nf = 0, z = 0, ov = 0;
        for (int r = r0 + t; r < r1; r += FIN_THREADS) {
            const vbg_stats_rec& rc = recs[r];
            s += rc.sumsq;
            mx = (long long)rc.amax_bits > mx ? (long long)rc.amax_bits : mx;
            nf += rc.nonfinite;
            z += rc.zeros;
            ov += rc.over_f16;
        }
        auto add = [](auto a, auto b) { return a + b; };
        s = stats_tree(s, shd, add);
        mx = stats_tree(mx, shl, [](long long a, long long b) { return a > b ? a : b; });
        nf = stats_tree(nf, shl, add);
        z = stats_tree(z, shl, add);
        ov = stats_tree(ov, shl, add);
        __syncthreads();
        shl[t] = h;
        __syncthreads();
        if (t < 64) {
            h = 0;
            for (int k = 0; k < FIN_GROUPS; ++k) h += shl[t + 64 * k];
            last[p].hist[t] = (int)h;
            if (total) total[p].hist[t] += h;
        }
        if (t == 64) {
            vbg_stats_rec& l = last[p];
            l.sumsq = s;
            l.amax_bits = (unsigned)mx;
            l.nonfinite = (int)nf;
            l.zeros = (int)z;
            l.over_f16 = (int)ov;
            l.pad[0] = 0;
            l.pad[1] = 0;
            if (total) {
                vbg_stats_total& a = total[p];
                a.sumsq = s;
                a.nonfinite += nf;
                a.zeros += z;
                a.over_f16 += ov;
                a.updates += 1;
                a.steps_nonfinite += nf > 0 ? 1 : 0;
                a.amax_bits = (unsigned)mx > a.amax_bits ? (unsigned)mx : a.amax_bits;
            }
        }
    }
}

static inline int stats_grid(int n) { return n > 256 * 8 ? 256 * 8 : n; }

}  // namespace vbg

using namespace vbg;
#define ALIGNED(p, a) (((uintptr_t)(p)) % (a) == 0)

extern "C" int vbg_param_stats_rows(const float* x, const vbg_optim_chunk* rows, int nrows, const float* scale_or_null, vbg_stats_rec* recs,
                                    void* stream) {
    VBG_CHECK_ARG(nrows >= 0);
    if (nrows == 0) return VBG_OK;
    VBG_CHECK_ARG(x && rows && recs);
    VBG_CHECK_ARG(ALIGNED(x, 16) && ALIGNED(rows, 16) && ALIGNED(recs, 16) && ALIGNED(scale_or_null, 4));
    VBG_LAUNCH(param_stats_rows_kernel, dim3(stats_grid(nrows)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, rows, nrows, scale_or_null, recs);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_param_stats_finish(const vbg_stats_rec* recs, const int* row_ptr, int nparams, vbg_stats_rec* last, vbg_stats_total* total,
                                      void* stream) {
    VBG_CHECK_ARG(nparams >= 0);
    if (nparams == 0) return VBG_OK;
    VBG_CHECK_ARG(recs && row_ptr && last);
    VBG_CHECK_ARG(ALIGNED(recs, 16) && ALIGNED(last, 16) && ALIGNED(total, 8) && ALIGNED(row_ptr, 4));
    VBG_LAUNCH(param_stats_finish_kernel, dim3(stats_grid(nparams)), dim3(FIN_THREADS), 0, (hipStream_t)stream, recs, row_ptr, nparams, last, total);
    VBG_LAUNCH_RET();
}
