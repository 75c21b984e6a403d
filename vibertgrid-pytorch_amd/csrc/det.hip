// Deterministic mode (vbg.ops.set_deterministic / torch.use_deterministic_algorithms): fixed-order forms of the reductions whose
// default kernels add floats with atomics (DESIGN.md "Deterministic mode").  Every form here adds its terms in an order fixed by the
// shapes alone -- never by which block or thread arrives first -- so two launches on the same inputs return the same bits:
//   * column sums and whole-tensor sums: per-chunk partials in a slab (a block owns a fixed row / element range and reduces it in a
//     fixed tree), then one ordered pass over the slab;
//   * scatter-adds (embedding rows, gather_rows backward, the CE backward's upsampled / repeated picks): the destination indices are
//     sorted with a STABLE radix sort (rocPRIM), and one owner per destination run adds its source rows in ascending source order;
//   * RoIAlign backward: one block per (document, feature row) walks the RoIs in RoI order and adds each one's contribution to the
//     row it owns, with the separable bilinear weights summed per sample in sample order (no LDS atomics).
#include "vbg_common.h"
#include "../../include/vbg.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace vbg {

constexpr int DET_CHUNKS = 256;            // row chunks of the column-sum slab (fixed: the order depends on M only)

static inline int det_chunks(long long M) {
    long long c = (M + 255) / 256;
    if (c > DET_CHUNKS) c = DET_CHUNKS;
    return (int)(c < 1 ? 1 : c);
}

// stage 1: block (column group of 64, chunk) -> ws[chunk][c]; 4 row lanes each add every 4th row of the chunk, the lanes are combined
// in lane order
__global__ __launch_bounds__(256) void colsum_det_part_kernel(const float* __restrict__ x, long long ld, long long M, int N,
                                                              long long rows_per_chunk, double* __restrict__ ws) {
    __shared__ double sh[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s = 0.0;
    if (c < N)
        for (long long r = r0 + rl; r < r1; r += 4) s += (double)x[r * ld + c];
    sh[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && c < N) ws[(long long)blockIdx.y * N + c] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}
// stage 2: one thread per column adds the chunks in chunk order and rounds once
__global__ void colsum_det_finish_kernel(const double* __restrict__ ws, int chunks, int N, float* out, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += ws[(long long)k * N + c];
    out[c] = accumulate ? (float)((double)out[c] + s) : (float)s;
}

// whole-tensor sum / sum of squares: DET_CHUNKS blocks over fixed element ranges -> ws[block], then one block adds them in a fixed tree
template <bool SQ>
__global__ __launch_bounds__(256) void sum_det_part_kernel(const float* __restrict__ x, long long n, float* __restrict__ ws) {
    __shared__ float sh[16];
    const long long stride = (long long)gridDim.x * blockDim.x;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += SQ ? x[i] * x[i] : x[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sum_det_finish_kernel(const float* __restrict__ ws, int nb, float* out) {
    __shared__ float sh[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s += ws[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) out[0] += s;
}

// dst[key] (+)= sum of src rows perm[k] over the run of equal keys starting at sorted position k, in sorted (= ascending source, the
// sort is stable) order; element e = (k, c); only the run's first position does the work; keys < 0 are skipped
__global__ __launch_bounds__(256) void segment_rows_add_kernel(const float* __restrict__ src, long long lds, const int* __restrict__ perm,
                                                               const int* __restrict__ keys, long long n, int C, float* dst, long long ldd) {
    const long long total = n * C;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long k = e / C;
        const int c = (int)(e - k * C);
        const int key = keys[k];
        if (key < 0 || (k > 0 && keys[k - 1] == key)) continue;
        float s = 0.f;
        for (long long j = k; j < n && keys[j] == key; ++j) s += src[(long long)perm[j] * lds + c];
        dst[(long long)key * ldd + c] += s;
    }
}

__global__ void iota_det_kernel(int* out, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int)i;
}

// CE backward, per element: its gradient row g * (softmax - onehot) and the logits row it belongs to (-1: label out of range, skipped)
__device__ __forceinline__ long long ce_row_det(long long e, int up_shift, int H, int W) {
    if (H <= 0) return e;
    const int x = (int)(e % W);
    const long long t = e / W;
    const int y = (int)(t % H);
    const long long b = t / H;
    return (b * (H >> up_shift) + (y >> up_shift)) * (W >> up_shift) + (x >> up_shift);
}
__global__ void ce_bwd_rows_kernel(const float* __restrict__ logits, long long ld, int ncls, const int* __restrict__ elem,
                                   const int* __restrict__ labels, long long n, const int* __restrict__ n_dev,
                                   const float* __restrict__ weight, const float* __restrict__ gdev, float gmul, int up_shift, int H, int W,
                                   float* __restrict__ grow, int* __restrict__ keys) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float g0 = gmul * (gdev ? gdev[0] : 1.f);
    // n_dev: the list's count lives on the device (n is its capacity); slots at and beyond it are not read and become skipped rows
    const long long cnt = n_dev ? (long long)n_dev[0] : n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long e = i < cnt ? (elem ? elem[i] : i) : 0;
        const int t = i < cnt ? labels[e] : -1;
        float* gr = grow + i * ncls;
        if ((unsigned)t >= (unsigned)ncls) {
            keys[i] = -1;
            for (int c = 0; c < ncls; ++c) gr[c] = 0.f;
            continue;
        }
        const long long row = ce_row_det(e, up_shift, H, W);
        keys[i] = (int)row;
        const float* x = logits + row * ld;
        float mx = x[0];
        for (int c = 1; c < ncls; ++c) mx = fmaxf(mx, x[c]);
        float s = 0.f;
        for (int c = 0; c < ncls; ++c) s += expf(x[c] - mx);
        const float g = g0 * (weight ? weight[t] : 1.f), inv = 1.f / s;
        for (int c = 0; c < ncls; ++c) {
            const float p = expf(x[c] - mx) * inv;
            gr[c] = g * (p - (c == t ? 1.f : 0.f));
        }
    }
}

// ---- RoIAlign backward (torchvision aligned=False geometry, as roi.hip) ----
struct DetGeo { float y_start, x_start, bin_h, bin_w; int gh, gw; float inv_count; };

__device__ __forceinline__ DetGeo det_geo(const int* box, float scale, int out_h, int out_w) {
    const float x1 = __fmul_rn((float)box[0], scale), y1 = __fmul_rn((float)box[1], scale);
    const float x2 = __fmul_rn((float)box[2], scale), y2 = __fmul_rn((float)box[3], scale);
    const float rw = fmaxf(__fsub_rn(x2, x1), 1.0f), rh = fmaxf(__fsub_rn(y2, y1), 1.0f);
    DetGeo g;
    g.bin_h = __fdiv_rn(rh, (float)out_h);
    g.bin_w = __fdiv_rn(rw, (float)out_w);
    g.gh = (int)ceilf(__fdiv_rn(rh, (float)out_h));
    g.gw = (int)ceilf(__fdiv_rn(rw, (float)out_w));
    g.y_start = y1; g.x_start = x1;
    g.inv_count = 1.0f / (float)max(g.gh * g.gw, 1);
    return g;
}
__device__ __forceinline__ float det_coord(float start, int p, float bin, int i, int g) {
    return __fadd_rn(__fadd_rn(start, __fmul_rn((float)p, bin)), __fdiv_rn(__fmul_rn((float)i + 0.5f, bin), (float)g));
}
// 1-D bilinear tap of one sample (the separable half of roi.hip make_tap)
__device__ __forceinline__ bool det_tap(float v, int size, int& i0, int& i1, float& w0, float& w1) {
    if (v < -1.0f || v > (float)size) return false;
    if (v <= 0.f) v = 0.f;
    i0 = (int)v;
    if (i0 >= size - 1) { i1 = i0 = size - 1; v = (float)i0; } else i1 = i0 + 1;
    w1 = __fsub_rn(v, (float)i0);
    w0 = __fsub_rn(1.f, w1);
    return true;
}
// weight of bin `b`'s samples on coordinate `X` (samples in sample order; w0 then w1 of each)
__device__ __forceinline__ float det_weight(float start, int b, float bin, int gs, int size, int X) {
    float w = 0.f;
    for (int i = 0; i < gs; ++i) {
        int i0, i1; float w0, w1;
        if (!det_tap(det_coord(start, b, bin, i, gs), size, i0, i1, w0, w1)) continue;
        if (i0 == X) w += w0;
        if (i1 == X) w += w1;
    }
    return w;
}

// out_h, out_w <= 32; wx[out_w][W] must fit DET_ROI_LDS_BYTES
constexpr int DET_ROI_OUT_MAX = 32;
constexpr long long DET_ROI_LDS_BYTES = 48 * 1024;
// block = (channel group, feature row Y, document); dynamic LDS: wx[out_w][W].  tmp[] stays in registers: its column loops are
// unrolled to DET_ROI_OUT_MAX and guarded by bw < out_w.
__global__ __launch_bounds__(256) void roi_align_bwd_det_kernel(const float* __restrict__ dy, int H, int W, int C,
                                                                const int* __restrict__ boxes, const int* __restrict__ box_doc, int nroi,
                                                                int out_h, int out_w, float scale, float* dfeat) {
    extern __shared__ float wx[];                 // [out_w][W]
    __shared__ float wy[DET_ROI_OUT_MAX];
    const int Y = blockIdx.y, b = blockIdx.z;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    float* frow = dfeat + (((long long)b * H + Y) * W) * C;
    for (int r = 0; r < nroi; ++r) {
        if (box_doc[r] != b) continue;                                   // (uniform)
        const DetGeo g = det_geo(boxes + 4 * (long long)r, scale, out_h, out_w);
        const float rh = __fmul_rn(g.bin_h, (float)out_h), rw = __fmul_rn(g.bin_w, (float)out_w);
        const int y_lo = min(max((int)floorf(fmaxf(g.y_start, 0.f)), 0), H - 1);
        const int y_hi = min(max((int)floorf(g.y_start + rh) + 2, 0), H - 1);
        if (Y < y_lo || Y > y_hi) continue;                              // (uniform) the RoI's taps cannot reach this row
        const int x_lo = min(max((int)floorf(fmaxf(g.x_start, 0.f)), 0), W - 1);
        const int x_hi = min(max((int)floorf(g.x_start + rw) + 2, 0), W - 1);
        const int pw = x_hi - x_lo + 1;
        __syncthreads();                                                 // the previous RoI's tables are no longer read
        if (threadIdx.x < out_h) wy[threadIdx.x] = det_weight(g.y_start, threadIdx.x, g.bin_h, g.gh, H, Y) * g.inv_count;
        for (int i = threadIdx.x; i < out_w * pw; i += blockDim.x) {
            const int bw = i / pw, X = i - bw * pw;
            wx[bw * W + X] = det_weight(g.x_start, bw, g.bin_w, g.gw, W, x_lo + X);
        }
        __syncthreads();
        bool any = false;
        for (int bh = 0; bh < out_h; ++bh) any |= wy[bh] != 0.f;
        if (!any || c >= C) continue;
        const float* dyr = dy + (long long)r * out_h * out_w * C + c;
        float tmp[DET_ROI_OUT_MAX];
#pragma unroll
        for (int bw = 0; bw < DET_ROI_OUT_MAX; ++bw) {
            float a = 0.f;
            if (bw < out_w)
                for (int bh = 0; bh < out_h; ++bh)
                    if (wy[bh] != 0.f) a = fmaf(wy[bh], dyr[(long long)(bh * out_w + bw) * C], a);
            tmp[bw] = a;
        }
        for (int X = 0; X < pw; ++X) {
            float v = 0.f;
            bool anyx = false;
#pragma unroll
            for (int bw = 0; bw < DET_ROI_OUT_MAX; ++bw)
                if (bw < out_w) { const float w = wx[bw * W + X]; anyx |= w != 0.f; v = fmaf(w, tmp[bw], v); }
            if (anyx) frow[(long long)(x_lo + X) * C + c] += v;
        }
    }
}

static inline int det_grid(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g > 2048) g = 2048;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace vbg

using namespace vbg;
#define S_ ((hipStream_t)stream)

extern "C" long long vbg_colsum_det_ws_elems(long long M, int N) { return (long long)det_chunks(M) * (N > 0 ? N : 0); }

extern "C" int vbg_colsum_det(const float* x, long long ld, long long M, int N, float* out, int accumulate, double* ws, void* stream) {
    VBG_CHECK_ARG(M >= 0 && N > 0 && ld >= N && out && ws);
    VBG_CHECK_ARG(M == 0 || x);
    const int chunks = det_chunks(M);
    const long long rpc = (M + chunks - 1) / chunks;
    if (M > 0)
        VBG_LAUNCH(colsum_det_part_kernel, dim3(cdiv(N, 64), chunks), dim3(256), 0, S_, x, ld, M, N, rpc, ws);
    VBG_LAUNCH(colsum_det_finish_kernel, dim3(cdiv(N, 256)), dim3(256), 0, S_, ws, M > 0 ? chunks : 0, N, out, accumulate);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_sum_det(const float* x, long long n, int squares, float* out_accum, float* ws, void* stream) {
    VBG_CHECK_ARG(n >= 0 && out_accum && ws);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(x);
    if (squares) VBG_LAUNCH(sum_det_part_kernel<true>, dim3(DET_CHUNKS), dim3(256), 0, S_, x, n, ws);
    else VBG_LAUNCH(sum_det_part_kernel<false>, dim3(DET_CHUNKS), dim3(256), 0, S_, x, n, ws);
    VBG_LAUNCH(sum_det_finish_kernel, dim3(1), dim3(256), 0, S_, ws, DET_CHUNKS, out_accum);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_sum_det_ws_elems(void) { return DET_CHUNKS; }

extern "C" long long vbg_sort_i32_ws_bytes(long long n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr, (size_t)n);
    return (long long)bytes + (long long)n * sizeof(int) + 512;
}

// stable ascending sort of int keys -> (sorted keys, source positions)
extern "C" int vbg_sort_i32(const int* keys, long long n, int* keys_out, int* idx_out, void* ws, long long ws_bytes, void* stream) {
    VBG_CHECK_ARG(n >= 0 && n < 2147483647LL);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(keys && keys_out && idx_out && ws);
    const size_t iota_bytes = (((size_t)n * sizeof(int)) + 255) / 256 * 256;
    VBG_CHECK_ARG((size_t)ws_bytes > iota_bytes);
    int* iota = (int*)ws;
    VBG_LAUNCH(iota_det_kernel, dim3(det_grid(n, 256)), dim3(256), 0, S_, iota, n);
    size_t bytes = (size_t)ws_bytes - iota_bytes;
    hipError_t e = rocprim::radix_sort_pairs((char*)ws + iota_bytes, bytes, keys, keys_out, (const int*)iota, idx_out, (size_t)n, 0,
                                             8 * (int)sizeof(int), S_);
    return e == hipSuccess ? VBG_OK : (int)e;
}

extern "C" int vbg_segment_rows_add(const float* src, long long lds, const int* perm, const int* sorted_keys, long long n, int C,
                                    float* dst_accum, long long ldd, void* stream) {
    VBG_CHECK_ARG(n >= 0 && C > 0 && lds >= C && ldd >= C);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(src && perm && sorted_keys && dst_accum);
    VBG_LAUNCH(segment_rows_add_kernel, dim3(det_grid(n * C, 256)), dim3(256), 0, S_, src, lds, perm, sorted_keys, n, C, dst_accum, ldd);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_ce_bwd_rows(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n,
                               const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W, float* grow, int* keys,
                               void* stream) {
    VBG_CHECK_ARG(n >= 0 && ncls > 0 && up_shift >= 0);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(logits && labels && grow && keys);
    VBG_LAUNCH(ce_bwd_rows_kernel, dim3(det_grid(n, 256)), dim3(256), 0, S_, logits, ld, ncls, elem, labels, n, (const int*)nullptr, weight,
               gscale_dev, gmul, up_shift, H, W, grow, keys);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_ce_bwd_rows_dyn(const float* logits, long long ld, int ncls, const int* elem, const int* labels, long long n_cap,
                                   const int* n_dev, const float* weight, const float* gscale_dev, float gmul, int up_shift, int H, int W,
                                   float* grow, int* keys, void* stream) {
    VBG_CHECK_ARG(n_cap >= 0 && ncls > 0 && up_shift >= 0 && n_dev);
    if (n_cap == 0) return VBG_OK;
    VBG_CHECK_ARG(logits && labels && grow && keys);
    VBG_LAUNCH(ce_bwd_rows_kernel, dim3(det_grid(n_cap, 256)), dim3(256), 0, S_, logits, ld, ncls, elem, labels, n_cap, n_dev, weight,
               gscale_dev, gmul, up_shift, H, W, grow, keys);
    VBG_LAUNCH_RET();
}

// torchvision.ops.RoIAlign(output_size=(out_h, out_w)) backward -- upstream model/grid_roi_align.py:10-19 (output_size: int or
// (H, W)), :37-41; RoIs added in RoI order
extern "C" int vbg_roi_align_hw_bwd_det(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi,
                                        int out_h, int out_w, float scale, float* dfeat_accum, void* stream) {
    VBG_CHECK_ARG(dy && dfeat_accum && B >= 0 && H > 0 && W > 0 && C > 0 && nroi >= 0);
    VBG_CHECK_ARG(out_h > 0 && out_h <= DET_ROI_OUT_MAX && out_w > 0 && out_w <= DET_ROI_OUT_MAX);
    VBG_CHECK_ARG((long long)out_w * W * sizeof(float) <= DET_ROI_LDS_BYTES);
    if (nroi == 0 || B == 0) return VBG_OK;
    VBG_CHECK_ARG(boxes && box_doc);
    const int nt = C >= 256 ? 256 : (C >= 128 ? 128 : 64);
    VBG_LAUNCH(roi_align_bwd_det_kernel, dim3(cdiv(C, nt), H, B), dim3(nt), out_w * W * sizeof(float), S_, dy, H, W, C, boxes, box_doc,
               nroi, out_h, out_w, scale, dfeat_accum);
    VBG_LAUNCH_RET();
}

// the square entry keeps its published bound, out <= 8; the (out_h, out_w) entry takes up to 32
extern "C" int vbg_roi_align_bwd_det(const float* dy, int B, int H, int W, int C, const int* boxes, const int* box_doc, int nroi, int out,
                                     float scale, float* dfeat_accum, void* stream) {
    VBG_CHECK_ARG(out <= 8);
    return vbg_roi_align_hw_bwd_det(dy, B, H, W, C, boxes, box_doc, nroi, out, out, scale, dfeat_accum, stream);
}
