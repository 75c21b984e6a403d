// Fused optimizer steps over flat fp32 ranges (torch.optim.SGD(momentum, weight_decay) for the
// CNN/head parameters and torch.optim.AdamW for BERT, as configured at train_SROIE.py:223-235 and
// stepped at pipeline/train_val_utils.py:272-284).  HBM-bound: 20 B/param (SGD-momentum),
// 28 B/param (AdamW); one launch covers a whole flat parameter bucket.
// Two forms of each step share ONE statement of the per-element arithmetic (sgd_update / adamw_update): the whole-range kernels
// (one set of hyper-parameters), and the segmented kernels, which walk a chunk table (start, length, group) and take up to
// VBG_OPTIM_MAX_GROUPS sets of hyper-parameters by value in their arguments (torch param groups over a layout that cannot be
// reordered by group: a group is a set of scattered runs of slots).
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace vbg {

__device__ __forceinline__ void sgd_update(float& pv, float gv, float& mv, float lr, float momentum, float wd, int first, float gs) {
    float d = gv * gs + wd * pv;
    mv = first ? d : momentum * mv + d;
    pv = pv - lr * mv;
}

// step_size = lr / bc1 (in fp32, by the caller: once per kernel / per chunk)
__device__ __forceinline__ void adamw_update(float& pv, float gv, float& mv, float& vv, float lr, float b1, float b2, float eps, float wd,
                                             float step_size, float bc2_sqrt, float gs) {
    gv *= gs;
    pv = pv * (1.f - lr * wd);
    mv = b1 * mv + (1.f - b1) * gv;
    vv = b2 * vv + (1.f - b2) * gv * gv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv = pv - step_size * (mv / denom);
}

// torch.optim's remaining options (the *_seg_opt entries): the default case of a group -- no flag beyond `first`, dampening 0,
// momentum != 0 / decoupled decay, no amsgrad, no maximize -- goes through sgd_update / adamw_update above, so it carries their
// bits; every other group goes through the two statements below (torch 2.10's single-tensor rules).
constexpr int SGD_NESTEROV = 1, SGD_MAXIMIZE = 2, SGD_FIRST = 4;
constexpr int ADAM_AMSGRAD = 1, ADAM_MAXIMIZE = 2, ADAM_COUPLED = 4;

// has_mom == 0 (momentum 0): mv is neither read nor written by the caller
__device__ __forceinline__ void sgd_update_opt(float& pv, float gv, float& mv, float lr, float momentum, float dampening, float wd,
                                               int has_mom, int nesterov, int maximize, int first, float gs) {
    float d = (maximize ? -gv : gv) * gs + wd * pv;
    if (has_mom) {
        mv = first ? d : momentum * mv + (1.f - dampening) * d;
        d = nesterov ? d + momentum * mv : mv;
    }
    pv = pv - lr * d;
}

// amsgrad == 0: xv (max_exp_avg_sq) is neither read nor written by the caller
__device__ __forceinline__ void adam_update_opt(float& pv, float gv, float& mv, float& vv, float& xv, float lr, float b1, float b2, float eps,
                                                float wd, float step_size, float bc2_sqrt, int amsgrad, int maximize, int coupled, float gs) {
    gv = (maximize ? -gv : gv) * gs;
    if (coupled) gv = gv + wd * pv;
    else pv = pv * (1.f - lr * wd);
    mv = b1 * mv + (1.f - b1) * gv;
    vv = b2 * vv + (1.f - b2) * gv * gv;
    float s = vv;
    if (amsgrad) {
        xv = fmaxf(xv, vv);
        s = xv;
    }
    const float denom = sqrtf(s) / bc2_sqrt + eps;
    pv = pv - step_size * (mv / denom);
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom, long long n4, long long n,
                           float lr, float momentum, float wd, int first, float gs) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    auto upd = [&](float& pv, float gv, float& mv) { sgd_update(pv, gv, mv, lr, momentum, wd, first, gs); };
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(mom)[i];
        upd(pv.x, gv.x, mv.x); upd(pv.y, gv.y, mv.y); upd(pv.z, gv.z, mv.z); upd(pv.w, gv.w, mv.w);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(mom)[i] = mv;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) upd(p[i], g[i], mom[i]);
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             long long n4, long long n, float lr, float b1, float b2, float eps, float wd, float bc1,
                             float bc2_sqrt, float gs) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float step_size = lr / bc1;
    auto upd = [&](float& pv, float gv, float& mv, float& vv) { adamw_update(pv, gv, mv, vv, lr, b1, b2, eps, wd, step_size, bc2_sqrt, gs); };
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        upd(pv.x, gv.x, mv.x, vv.x); upd(pv.y, gv.y, mv.y, vv.y); upd(pv.z, gv.z, mv.z, vv.z); upd(pv.w, gv.w, mv.w, vv.w);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) upd(p[i], g[i], m[i], v[i]);
}

// ---- segmented forms ---------------------------------------------------------------------------------------------------
// Blocks stride over the rows of the chunk table, threads over the float4s of a chunk: the work of a block is bounded by the
// chunk length the host chose, never by the longest run.  The next row is fetched while the current chunk streams.  Starts and
// lengths are multiples of 4 elements and every chunk lies inside the buffers (checked where the table is built, vbg/ops.py);
// what no chunk covers is neither read nor written.
constexpr int SEG_THREADS = 256;
struct AdamwHp { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; };
struct SgdGroups { vbg_sgd_group g[VBG_OPTIM_MAX_GROUPS]; };
struct AdamwGroups { AdamwHp g[VBG_OPTIM_MAX_GROUPS]; };

__global__ void __launch_bounds__(SEG_THREADS) sgd_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom,
                               const vbg_optim_chunk* __restrict__ tbl, int nchunks, SgdGroups hp, int first, float gs) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    vbg_optim_chunk ch = tbl[c];
    for (;;) {
        const int nxt = c + (int)gridDim.x;
        vbg_optim_chunk chn = ch;
        if (nxt < nchunks) chn = tbl[nxt];
        const vbg_sgd_group h = hp.g[ch.group];
        float4* p4 = reinterpret_cast<float4*>(p + ch.start);
        const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
        float4* m4 = reinterpret_cast<float4*>(mom + ch.start);
        const int n4 = ch.length >> 2;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
            float4 pv = p4[i];
            const float4 gv = g4[i];
            float4 mv = m4[i];
            sgd_update(pv.x, gv.x, mv.x, h.lr, h.momentum, h.wd, first, gs);
            sgd_update(pv.y, gv.y, mv.y, h.lr, h.momentum, h.wd, first, gs);
            sgd_update(pv.z, gv.z, mv.z, h.lr, h.momentum, h.wd, first, gs);
            sgd_update(pv.w, gv.w, mv.w, h.lr, h.momentum, h.wd, first, gs);
            p4[i] = pv;
            m4[i] = mv;
        }
        if (nxt >= nchunks) break;
        c = nxt;
        ch = chn;
    }
}

__global__ void __launch_bounds__(SEG_THREADS) adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 const vbg_optim_chunk* __restrict__ tbl, int nchunks, AdamwGroups hp, float gs) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    vbg_optim_chunk ch = tbl[c];
    for (;;) {
        const int nxt = c + (int)gridDim.x;
        vbg_optim_chunk chn = ch;
        if (nxt < nchunks) chn = tbl[nxt];
        const AdamwHp h = hp.g[ch.group];
        const float step_size = h.lr / h.bc1;
        float4* p4 = reinterpret_cast<float4*>(p + ch.start);
        const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
        float4* m4 = reinterpret_cast<float4*>(m + ch.start);
        float4* v4 = reinterpret_cast<float4*>(v + ch.start);
        const int n4 = ch.length >> 2;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
            float4 pv = p4[i];
            const float4 gv = g4[i];
            float4 mv = m4[i];
            float4 vv = v4[i];
            adamw_update(pv.x, gv.x, mv.x, vv.x, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
            adamw_update(pv.y, gv.y, mv.y, vv.y, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
            adamw_update(pv.z, gv.z, mv.z, vv.z, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
            adamw_update(pv.w, gv.w, mv.w, vv.w, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
            p4[i] = pv;
            m4[i] = mv;
            v4[i] = vv;
        }
        if (nxt >= nchunks) break;
        c = nxt;
        ch = chn;
    }
}

// ---- segmented forms with every torch.optim option per group ------------------------------------------------------------
// The same walk over the chunk table.  A chunk's group decides, uniformly for the block, which loop streams it: the default case
// runs the loop of sgd_seg_kernel / adamw_seg_kernel, momentum 0 never touches the momentum buffer, and max_exp_avg_sq is only
// touched in chunks of amsgrad groups.
struct AdamOptHp { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; int flags; };
struct SgdOptGroups { vbg_sgd_group_opt g[VBG_OPTIM_MAX_GROUPS]; };
struct AdamOptGroups { AdamOptHp g[VBG_OPTIM_MAX_GROUPS]; };

__global__ void __launch_bounds__(SEG_THREADS) sgd_seg_opt_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom,
                                   const vbg_optim_chunk* __restrict__ tbl, int nchunks, SgdOptGroups hp, float gs) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    vbg_optim_chunk ch = tbl[c];
    for (;;) {
        const int nxt = c + (int)gridDim.x;
        vbg_optim_chunk chn = ch;
        if (nxt < nchunks) chn = tbl[nxt];
        const vbg_sgd_group_opt h = hp.g[ch.group];
        const int first = (h.flags & SGD_FIRST) != 0, nesterov = (h.flags & SGD_NESTEROV) != 0, maximize = (h.flags & SGD_MAXIMIZE) != 0;
        float4* p4 = reinterpret_cast<float4*>(p + ch.start);
        const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
        const int n4 = ch.length >> 2;
        if (h.momentum == 0.f) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float none = 0.f;
                sgd_update_opt(pv.x, gv.x, none, h.lr, 0.f, h.dampening, h.wd, 0, 0, maximize, 0, gs);
                sgd_update_opt(pv.y, gv.y, none, h.lr, 0.f, h.dampening, h.wd, 0, 0, maximize, 0, gs);
                sgd_update_opt(pv.z, gv.z, none, h.lr, 0.f, h.dampening, h.wd, 0, 0, maximize, 0, gs);
                sgd_update_opt(pv.w, gv.w, none, h.lr, 0.f, h.dampening, h.wd, 0, 0, maximize, 0, gs);
                p4[i] = pv;
            }
        } else if ((h.flags & ~SGD_FIRST) == 0 && h.dampening == 0.f) {
            float4* m4 = reinterpret_cast<float4*>(mom + ch.start);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float4 mv = m4[i];
                sgd_update(pv.x, gv.x, mv.x, h.lr, h.momentum, h.wd, first, gs);
                sgd_update(pv.y, gv.y, mv.y, h.lr, h.momentum, h.wd, first, gs);
                sgd_update(pv.z, gv.z, mv.z, h.lr, h.momentum, h.wd, first, gs);
                sgd_update(pv.w, gv.w, mv.w, h.lr, h.momentum, h.wd, first, gs);
                p4[i] = pv;
                m4[i] = mv;
            }
        } else {
            float4* m4 = reinterpret_cast<float4*>(mom + ch.start);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float4 mv = m4[i];
                sgd_update_opt(pv.x, gv.x, mv.x, h.lr, h.momentum, h.dampening, h.wd, 1, nesterov, maximize, first, gs);
                sgd_update_opt(pv.y, gv.y, mv.y, h.lr, h.momentum, h.dampening, h.wd, 1, nesterov, maximize, first, gs);
                sgd_update_opt(pv.z, gv.z, mv.z, h.lr, h.momentum, h.dampening, h.wd, 1, nesterov, maximize, first, gs);
                sgd_update_opt(pv.w, gv.w, mv.w, h.lr, h.momentum, h.dampening, h.wd, 1, nesterov, maximize, first, gs);
                p4[i] = pv;
                m4[i] = mv;
            }
        }
        if (nxt >= nchunks) break;
        c = nxt;
        ch = chn;
    }
}

__global__ void __launch_bounds__(SEG_THREADS) adam_seg_opt_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    float* __restrict__ vmax, const vbg_optim_chunk* __restrict__ tbl, int nchunks, AdamOptGroups hp, float gs) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    vbg_optim_chunk ch = tbl[c];
    for (;;) {
        const int nxt = c + (int)gridDim.x;
        vbg_optim_chunk chn = ch;
        if (nxt < nchunks) chn = tbl[nxt];
        const AdamOptHp h = hp.g[ch.group];
        const float step_size = h.lr / h.bc1;
        const int maximize = (h.flags & ADAM_MAXIMIZE) != 0, coupled = (h.flags & ADAM_COUPLED) != 0;
        float4* p4 = reinterpret_cast<float4*>(p + ch.start);
        const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
        float4* m4 = reinterpret_cast<float4*>(m + ch.start);
        float4* v4 = reinterpret_cast<float4*>(v + ch.start);
        const int n4 = ch.length >> 2;
        if (h.flags == 0) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float4 mv = m4[i];
                float4 vv = v4[i];
                adamw_update(pv.x, gv.x, mv.x, vv.x, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
                adamw_update(pv.y, gv.y, mv.y, vv.y, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
                adamw_update(pv.z, gv.z, mv.z, vv.z, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
                adamw_update(pv.w, gv.w, mv.w, vv.w, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
                p4[i] = pv;
                m4[i] = mv;
                v4[i] = vv;
            }
        } else if (h.flags & ADAM_AMSGRAD) {
            float4* x4 = reinterpret_cast<float4*>(vmax + ch.start);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float4 mv = m4[i];
                float4 vv = v4[i];
                float4 xv = x4[i];
                adam_update_opt(pv.x, gv.x, mv.x, vv.x, xv.x, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 1, maximize, coupled, gs);
                adam_update_opt(pv.y, gv.y, mv.y, vv.y, xv.y, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 1, maximize, coupled, gs);
                adam_update_opt(pv.z, gv.z, mv.z, vv.z, xv.z, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 1, maximize, coupled, gs);
                adam_update_opt(pv.w, gv.w, mv.w, vv.w, xv.w, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 1, maximize, coupled, gs);
                p4[i] = pv;
                m4[i] = mv;
                v4[i] = vv;
                x4[i] = xv;
            }
        } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                float4 mv = m4[i];
                float4 vv = v4[i];
                float none = 0.f;
                adam_update_opt(pv.x, gv.x, mv.x, vv.x, none, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 0, maximize, coupled, gs);
                adam_update_opt(pv.y, gv.y, mv.y, vv.y, none, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 0, maximize, coupled, gs);
                adam_update_opt(pv.z, gv.z, mv.z, vv.z, none, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 0, maximize, coupled, gs);
                adam_update_opt(pv.w, gv.w, mv.w, vv.w, none, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 0, maximize, coupled, gs);
                p4[i] = pv;
                m4[i] = mv;
                v4[i] = vv;
            }
        }
        if (nxt >= nchunks) break;
        c = nxt;
        ch = chn;
    }
}

static inline int ew_grid(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g > 256 * 8) g = 256 * 8;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace vbg

using namespace vbg;
#define ALIGNED16(p) (((uintptr_t)(p)) % 16 == 0)

extern "C" int vbg_sgd_step(float* p, const float* g, float* mom, long long n, float lr, float momentum, float wd, int first_step,
                            float grad_scale, void* stream) {
    VBG_CHECK_ARG(n >= 0);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && mom);
    const long long n4 = (ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(mom)) ? n / 4 : 0;
    VBG_LAUNCH(sgd_kernel, dim3(ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, p, g, mom, n4, n, lr, momentum,
                       wd, first_step, grad_scale);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                              float wd, int step, float grad_scale, void* stream) {
    VBG_CHECK_ARG(n >= 0 && step >= 1);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && m && v);
    const long long n4 = (ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v)) ? n / 4 : 0;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    VBG_LAUNCH(adamw_kernel, dim3(ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, n, lr, b1, b2,
                       eps, wd, (float)bc1, (float)sqrt(bc2), grad_scale);
    VBG_LAUNCH_RET();
}

// the segmented forms: buffers 16-byte aligned (float4 access at start, a multiple of 4 elements); the table is device memory,
// the hyper-parameters are copied from host memory into the kernel arguments (no copy to the device, no sync)
extern "C" int vbg_sgd_step_seg(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                                const vbg_sgd_group* groups, int ngroups, int first_step, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && mom && chunks && groups);
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(mom) && ALIGNED16(chunks));
    SgdGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = groups[i];
    VBG_LAUNCH(sgd_seg_kernel, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, mom, chunks, nchunks, hp, first_step,
               grad_scale);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_adamw_step_seg(float* p, const float* g, float* m, float* v, const vbg_optim_chunk* chunks, int nchunks,
                                  const vbg_adamw_group* groups, int ngroups, int step, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0 && step >= 1);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && m && v && chunks && groups);
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(chunks));
    AdamwGroups hp = {};
    for (int i = 0; i < ngroups; ++i) {
        const vbg_adamw_group& s = groups[i];
        const double bc1 = 1.0 - pow((double)s.b1, (double)step), bc2 = 1.0 - pow((double)s.b2, (double)step);
        hp.g[i] = AdamwHp{s.lr, s.b1, s.b2, s.eps, s.wd, (float)bc1, (float)sqrt(bc2)};
    }
    VBG_LAUNCH(adamw_seg_kernel, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, m, v, chunks, nchunks, hp,
               grad_scale);
    VBG_LAUNCH_RET();
}

// every torch.optim option per group (flags of include/vbg.h): same table, same checks.  mom may be NULL when every group has momentum
// 0, vmax when no group has the amsgrad flag; a group's bias corrections come from ITS step
extern "C" int vbg_sgd_step_seg_opt(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                                    const vbg_sgd_group_opt* groups, int ngroups, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && chunks && groups);
    SgdOptGroups hp = {};
    bool any_mom = false;
    for (int i = 0; i < ngroups; ++i) {
        hp.g[i] = groups[i];
        any_mom = any_mom || groups[i].momentum != 0.f;
    }
    VBG_CHECK_ARG(mom || !any_mom);
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(mom) && ALIGNED16(chunks));
    VBG_LAUNCH(sgd_seg_opt_kernel, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, mom, chunks, nchunks, hp,
               grad_scale);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_adam_step_seg_opt(float* p, const float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                                     const vbg_adam_group_opt* groups, int ngroups, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && m && v && chunks && groups);
    AdamOptGroups hp = {};
    for (int i = 0; i < ngroups; ++i) {
        const vbg_adam_group_opt& s = groups[i];
        VBG_CHECK_ARG(s.step >= 1);
        VBG_CHECK_ARG(vmax || !(s.flags & ADAM_AMSGRAD));
        const double bc1 = 1.0 - pow((double)s.b1, (double)s.step), bc2 = 1.0 - pow((double)s.b2, (double)s.step);
        hp.g[i] = AdamOptHp{s.lr, s.b1, s.b2, s.eps, s.wd, (float)bc1, (float)sqrt(bc2), s.flags};
    }
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(vmax) && ALIGNED16(chunks));
    VBG_LAUNCH(adam_seg_opt_kernel, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, m, v, vmax, chunks, nchunks,
               hp, grad_scale);
    VBG_LAUNCH_RET();
}
