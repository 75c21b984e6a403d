// Fused optimizer steps over flat fp32 ranges (torch.optim.SGD(momentum, weight_decay) for the
// CNN/head parameters and torch.optim.AdamW for BERT, as configured at train_SROIE.py:223-235 and
// stepped at pipeline/train_val_utils.py:272-284).  HBM-bound: 20 B/param (SGD-momentum),
// 28 B/param (AdamW); one launch covers a whole flat parameter bucket.
// Two forms of each step share ONE statement of the per-element arithmetic (sgd_update / adamw_update): the whole-range kernels
// (one set of hyper-parameters), and the segmented kernels, which walk a chunk table (start, length, group) and take up to
// VBG_OPTIM_MAX_GROUPS sets of hyper-parameters by value in their arguments (torch param groups over a layout that cannot be
// reordered by group: a group is a set of scattered runs of slots).  There is one segmented kernel per rule, on one chunk walk
// (walk_chunks) and one stream loop (stream_chunk); vbg_sgd_step_seg / vbg_adamw_step_seg translate their groups into the default
// case of the per-group options that vbg_sgd_step_seg_opt / vbg_adam_step_seg_opt take.  vbg_sgd_step_seg_amp / vbg_adam_step_seg_amp
// are the AMP instantiation of the same two kernels (SegScale below), and vbg_sgd_step_seg_clip / vbg_adam_step_seg_clip the same
// instantiation with one more device scalar, the coefficient of a gradient-norm clip.  That coefficient comes from two more kernels on
// the same chunk table: one row pass (grad_norm_seg_kernel: a partial per row, GradScaler's inf check and the reference's loss gate riding
// along; entries vbg_grad_sumsq_seg, vbg_grad_sumsq_seg_inf, vbg_grad_norm_seg) and one finish (clip_coef_gate_kernel: the total norm and
// torch's coefficient; entries vbg_clip_coef, vbg_clip_coef_gate).  vbg_grad_unscale_check_seg, GradScaler's own pass (it stores into g),
// walks the same rows.  vbg_lerp / vbg_swap (weight averaging: avg <- lerp(avg, p, w) in torch's bits, and the in-place exchange of the
// live and the averaged buffer) are two more whole-range streams of sgd_kernel's shape.
#include <type_traits>
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

// ---- weight averaging (vbg.optim.WeightAverage) --------------------------------------------------------------------------
// avg <- lerp(avg, p, w) in torch's statement (ATen/native/Lerp.h): |w| < 0.5 ? a + w * (p - a) : p - (p - a) * (1 - w), the difference
// and 1 - w each rounded on their own, the product and the sum of either branch in ONE rounding (a fused multiply-add: what torch's
// device kernel was measured to do on gfx950, profiles/weight_average.txt).  Every rounding is spelled out, so the bits do not depend
// on the compiler's contraction setting.  The branch is uniform over the launch.
__device__ __forceinline__ float lerp_update(float a, float p, float w, float omw, bool small) {
    const float d = __fsub_rn(p, a);
    return small ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, omw, p);
}

__global__ void lerp_kernel(float* __restrict__ avg, const float* __restrict__ p, long long n4, long long n, float w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float omw = __fsub_rn(1.f, w);
    const bool small = fabsf(w) < 0.5f;
    auto upd = [&](float& av, float pv) { av = lerp_update(av, pv, w, omw, small); };
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 av = reinterpret_cast<float4*>(avg)[i];
        const float4 pv = reinterpret_cast<const float4*>(p)[i];
        upd(av.x, pv.x); upd(av.y, pv.y); upd(av.z, pv.z); upd(av.w, pv.w);
        reinterpret_cast<float4*>(avg)[i] = av;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) upd(avg[i], p[i]);
}

// exchange of two disjoint ranges as bit patterns (integer moves: NaN payloads, -0.0 and denormals pass through); each element is read
// and written by the one thread that owns it, so nothing is staged
__global__ void swap_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long long n4, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 av = reinterpret_cast<uint4*>(a)[i];
        const uint4 bv = reinterpret_cast<uint4*>(b)[i];
        reinterpret_cast<uint4*>(a)[i] = bv;
        reinterpret_cast<uint4*>(b)[i] = av;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
            const unsigned av = a[i], bv = b[i];
            a[i] = bv;
            b[i] = av;
        }
}

// ---- segmented forms ---------------------------------------------------------------------------------------------------
// Blocks stride over the rows of the chunk table, threads over the float4s of a chunk: the work of a block is bounded by the
// chunk length the host chose, never by the longest run.  The next row is fetched while the current chunk streams.  Starts and
// lengths are multiples of 4 elements and every chunk lies inside the buffers (checked where the table is built, vbg/ops.py);
// what no chunk covers is neither read nor written.
constexpr int SEG_THREADS = 256;

// How a segmented launch learns the gradient scale.  The host form carries it by value (gs multiplies the gradient inside the rule).
// The AMP form (torch.amp.GradScaler's protocol for optimizers with _step_supports_amp_scaling) reads two fp32 scalars from device
// memory: found_inf != 0 makes every block return before it touches a buffer; with a scale, every chunk's gradients are first
// multiplied by inv = float(1 / double(*scale)) (torch's own inverse) in place (unscale_chunk); with scale NULL (the caller unscaled
// already) g is only read.  The rule then runs on what g holds with gs (1 from the *_amp entries), in the statements of the host form.
// The *_clip entries add `clip`, the coefficient of clip_grad_norm_ as a third device scalar: g' = (g * inv) * coef, two products each
// rounded on its own, stored back; a coefficient of exactly 1 with no scale leaves g unwritten (the product would be g).  There
// found_inf may be NULL (no scaler).
template <bool AMP> struct SegScale { float gs; };
template <> struct SegScale<true> { float gs; const float* scale; const float* found_inf; const float* clip; };
template <bool AMP> using GradPtr = std::conditional_t<AMP, float*, const float*>;

// -> false: the launch is a skipped step.  Uniform over the launch.
template <bool AMP>
__device__ __forceinline__ bool seg_scale(const SegScale<AMP>& sc, float& inv, float& coef, bool& store_g) {
    inv = 1.f;
    coef = 1.f;
    store_g = false;
    if constexpr (AMP) {
        if (sc.found_inf && *sc.found_inf != 0.f) return false;
        if (sc.scale) {
            inv = (float)(1.0 / (double)*sc.scale);
            store_g = true;
        }
        if (sc.clip) {
            coef = *sc.clip;
            store_g = store_g || coef != 1.f;          // (a NaN coefficient is stored: torch's clip writes the NaNs too)
        }
    }
    return true;
}

template <class Body>
__device__ __forceinline__ void walk_chunks(const vbg_optim_chunk* __restrict__ tbl, int nchunks, Body body) {
    int c = blockIdx.x;
    if (c >= nchunks) return;
    vbg_optim_chunk ch = tbl[c];
    for (;;) {
        const int nxt = c + (int)gridDim.x;
        vbg_optim_chunk chn = ch;
        if (nxt < nchunks) chn = tbl[nxt];
        body(ch);
        if (nxt >= nchunks) break;
        c = nxt;
        ch = chn;
    }
}

// One chunk: p, g and the first NS of the state arrays s0, s1, s2 as float4s, upd(p, g, s0, s1, s2) on each of the four elements,
// p and those NS arrays stored.  An array past NS is neither read nor written (its pointer may be NULL): upd gets a zero it must
// not use.
template <int NS, class Upd>
__device__ __forceinline__ void stream_chunk(const vbg_optim_chunk& ch, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                             float* __restrict__ s1, float* __restrict__ s2, Upd upd) {
    float4* p4 = reinterpret_cast<float4*>(p + ch.start);
    const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
    float4* a4 = NS > 0 ? reinterpret_cast<float4*>(s0 + ch.start) : nullptr;
    float4* b4 = NS > 1 ? reinterpret_cast<float4*>(s1 + ch.start) : nullptr;
    float4* c4 = NS > 2 ? reinterpret_cast<float4*>(s2 + ch.start) : nullptr;
    const int n4 = ch.length >> 2;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
        float4 pv = p4[i];
        const float4 gv = g4[i];
        float4 av = {}, bv = {}, cv = {};
        if constexpr (NS > 0) av = a4[i];
        if constexpr (NS > 1) bv = b4[i];
        if constexpr (NS > 2) cv = c4[i];
        upd(pv.x, gv.x, av.x, bv.x, cv.x);
        upd(pv.y, gv.y, av.y, bv.y, cv.y);
        upd(pv.z, gv.z, av.z, bv.z, cv.z);
        upd(pv.w, gv.w, av.w, bv.w, cv.w);
        p4[i] = pv;
        if constexpr (NS > 0) a4[i] = av;
        if constexpr (NS > 1) b4[i] = bv;
        if constexpr (NS > 2) c4[i] = cv;
    }
}

// The AMP form's own pass over a chunk, ahead of stream_chunk: g *= inv, each product rounded on its own and stored.  A thread
// writes exactly the float4s it reads back in stream_chunk (same index walk), where they come from the cache: the chunk's traffic
// to memory is one read and one write of g more, and the rule runs on loaded values in the very statements of the host-scale form.
// With a clip coefficient the second product follows the first, rounded on its own as well (torch: unscale_, then the clip's mul_);
// inv == 1 (no scale) and coef == 1 (no clip) multiply exactly, so one statement serves every combination.
__device__ __forceinline__ void unscale_chunk(const vbg_optim_chunk& ch, float* __restrict__ g, float inv, float coef) {
    float4* g4 = reinterpret_cast<float4*>(g + ch.start);
    const int n4 = ch.length >> 2;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
        float4 gv = g4[i];
        gv.x = __fmul_rn(__fmul_rn(gv.x, inv), coef); gv.y = __fmul_rn(__fmul_rn(gv.y, inv), coef);
        gv.z = __fmul_rn(__fmul_rn(gv.z, inv), coef); gv.w = __fmul_rn(__fmul_rn(gv.w, inv), coef);
        g4[i] = gv;
    }
}

// A chunk's group decides, uniformly for the block, which statement streams it: the default case runs sgd_update / adamw_update,
// a momentum-0 group never touches the momentum buffer unless keep_mom is set (vbg_sgd_step_seg, which always has a buffer and
// writes it; never reachable through vbg_sgd_group_opt.flags), and max_exp_avg_sq is only touched in chunks of amsgrad groups.
struct SgdHp { float lr, momentum, dampening, wd; int flags, keep_mom; };
struct AdamHp { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; int flags; };
struct SgdGroups { SgdHp g[VBG_OPTIM_MAX_GROUPS]; };
struct AdamGroups { AdamHp g[VBG_OPTIM_MAX_GROUPS]; };

template <bool AMP>
__global__ void __launch_bounds__(SEG_THREADS) sgd_seg_kernel(float* __restrict__ p, GradPtr<AMP> __restrict__ g, float* __restrict__ mom,
                               const vbg_optim_chunk* __restrict__ tbl, int nchunks, SgdGroups hp, SegScale<AMP> sc) {
    float inv, coef;
    bool store_g;
    if (!seg_scale(sc, inv, coef, store_g)) return;
    const float gs = sc.gs;
    walk_chunks(tbl, nchunks, [&](const vbg_optim_chunk& ch) {
        if constexpr (AMP) if (store_g) unscale_chunk(ch, g, inv, coef);
        const SgdHp h = hp.g[ch.group];
        const int first = (h.flags & SGD_FIRST) != 0, nesterov = (h.flags & SGD_NESTEROV) != 0, maximize = (h.flags & SGD_MAXIMIZE) != 0;
        if (h.momentum == 0.f && !h.keep_mom)
            stream_chunk<0>(ch, p, g, nullptr, nullptr, nullptr, [&](float& pv, float gv, float& none, float&, float&) {
                sgd_update_opt(pv, gv, none, h.lr, 0.f, h.dampening, h.wd, 0, 0, maximize, 0, gs);
            });
        else if ((h.flags & ~SGD_FIRST) == 0 && h.dampening == 0.f)
            stream_chunk<1>(ch, p, g, mom, nullptr, nullptr, [&](float& pv, float gv, float& mv, float&, float&) {
                sgd_update(pv, gv, mv, h.lr, h.momentum, h.wd, first, gs);
            });
        else
            stream_chunk<1>(ch, p, g, mom, nullptr, nullptr, [&](float& pv, float gv, float& mv, float&, float&) {
                sgd_update_opt(pv, gv, mv, h.lr, h.momentum, h.dampening, h.wd, 1, nesterov, maximize, first, gs);
            });
    });
}

template <bool AMP>
__global__ void __launch_bounds__(SEG_THREADS) adam_seg_kernel(float* __restrict__ p, GradPtr<AMP> __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ vmax, const vbg_optim_chunk* __restrict__ tbl, int nchunks, AdamGroups hp, SegScale<AMP> sc) {
    float inv, coef;
    bool store_g;
    if (!seg_scale(sc, inv, coef, store_g)) return;
    const float gs = sc.gs;
    walk_chunks(tbl, nchunks, [&](const vbg_optim_chunk& ch) {
        if constexpr (AMP) if (store_g) unscale_chunk(ch, g, inv, coef);
        const AdamHp h = hp.g[ch.group];
        const float step_size = h.lr / h.bc1;
        const int maximize = (h.flags & ADAM_MAXIMIZE) != 0, coupled = (h.flags & ADAM_COUPLED) != 0;
        if (h.flags == 0)
            stream_chunk<2>(ch, p, g, m, v, nullptr, [&](float& pv, float gv, float& mv, float& vv, float&) {
                adamw_update(pv, gv, mv, vv, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, gs);
            });
        else if (h.flags & ADAM_AMSGRAD)
            stream_chunk<3>(ch, p, g, m, v, vmax, [&](float& pv, float gv, float& mv, float& vv, float& xv) {
                adam_update_opt(pv, gv, mv, vv, xv, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 1, maximize, coupled, gs);
            });
        else
            stream_chunk<2>(ch, p, g, m, v, nullptr, [&](float& pv, float gv, float& mv, float& vv, float& none) {
                adam_update_opt(pv, gv, mv, vv, none, h.lr, h.b1, h.b2, h.eps, h.wd, step_size, h.bc2_sqrt, 0, maximize, coupled, gs);
            });
    });
}

// ---- gradient-norm clipping on the device: the row pass -----------------------------------------------------------------
// One kernel on the row walk of the steps: block b on row c leaves partials[c], a plain store (no atomics, nothing to zero beforehand,
// the same bits on every call).  KIND 2: the sum of g[start .. start + length)^2 -- a thread sums the squares of its own float4s in fp32
// (a row of 4096 elements: 4 float4s, 16 products), block_sum adds the 256 thread sums: a short fp32 chain per row, the long sum over
// rows is left to the finish, in double.  KIND 1 sums |g| the same way (fabsf rounds nothing), KIND 0 leaves max |g| of the row.  The
// group field of a row is ignored; what no row covers is not read.
// GradScaler's test of four elements, carried as a sum: x * 0 is a zero for a finite x and NaN for an inf or a NaN, so z stays a zero
// exactly as long as everything folded into it was finite (torch's isfinite, element by element) -- one fused multiply-add per element,
// the arithmetic of the norm pass's own loop, and nothing to branch on.  IEEE semantics: this library is not built with finite-math
// flags (csrc/Makefile), and tests/test_gpu_fused_scaler.py plants each of +inf, -inf and NaN at every place of the walk.
__device__ __forceinline__ void fold_finite4(float& z, const float4& v) {
    z = __fmaf_rn(v.x, 0.f, z);
    z = __fmaf_rn(v.y, 0.f, z);
    z = __fmaf_rn(v.z, 0.f, z);
    z = __fmaf_rn(v.w, 0.f, z);
}

// What a block learnt about its rows, told to GradScaler's flag: set, never cleared (the caller hands in a zero, as torch's
// _amp_foreach_non_finite_check_and_unscale_ expects one).  One block-wide OR after the walk, then a plain store of 1.0f from one lane;
// several blocks may store the same value (no atomics on device memory, the same code in deterministic mode).  Every thread of the block calls this.
__device__ __forceinline__ void raise_found_inf(bool bad, float* __restrict__ found_inf) {
    if (__syncthreads_or(bad) && threadIdx.x == 0) *found_inf = 1.f;
}

// The loss gate.  The reference clips only `if train_loss > loss_clip_tresh` (pipeline/train_val_utils.py:281), a host read of a device
// scalar.  Here the loss stays where it is: the row pass and the finish read it (one load, uniform over the launch) and take torch's own
// decision, `loss > threshold` in the loss tensor's dtype -- strictly greater, so a NaN loss closes the gate and +inf opens it; thr32 is
// the threshold rounded to fp32 on the host, which is what torch compares an fp32 tensor with.  loss NULL (ClipGate{}): no gate.
struct ClipGate { const void* loss; double thr64; float thr32; int f64; };

__device__ __forceinline__ bool gate_open(const ClipGate& gt) {
    if (!gt.loss) return true;
    return gt.f64 ? *reinterpret_cast<const double*>(gt.loss) > gt.thr64 : *reinterpret_cast<const float*>(gt.loss) > gt.thr32;
}

// max over the block of |x| carried as its bit pattern: as unsigned integers finite < inf < NaN, so one integer max is exact, turns
// +-inf into +inf and keeps a NaN (fmaxf alone drops it).  `sh` has >= 16 words; result broadcast.
__device__ __forceinline__ unsigned block_max_bits(unsigned v, unsigned* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    unsigned r = sh[0];
    for (int i = 1; i < nw; ++i) r = sh[i] > r ? sh[i] : r;
    return r;
}

__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// CHECK: GradScaler's inf check rides in the loop -- decided per ELEMENT (a row of finite values whose squares overflow leaves an inf
// partial and the flag alone); found_inf is not read without CHECK.  Without CHECK a closed gate makes every block return before it
// touches g or partials; with CHECK the rows always walk and only the finish reads the gate.
template <int KIND, bool CHECK>
__global__ void __launch_bounds__(SEG_THREADS) grad_norm_seg_kernel(const float* __restrict__ g, const vbg_optim_chunk* __restrict__ tbl, int nchunks,
                                                                     float* __restrict__ partials, float* __restrict__ found_inf, ClipGate gate) {
    __shared__ float sh[16];
    if constexpr (!CHECK) if (!gate_open(gate)) return;
    int c = blockIdx.x;
    float z = 0.f;
    walk_chunks(tbl, nchunks, [&](const vbg_optim_chunk& ch) {
        const float4* g4 = reinterpret_cast<const float4*>(g + ch.start);
        const int n4 = ch.length >> 2;
        float acc = 0.f;
        unsigned mx = 0u;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
            const float4 gv = g4[i];
            if constexpr (CHECK) fold_finite4(z, gv);
            if constexpr (KIND == 2) {
                acc += gv.x * gv.x;
                acc += gv.y * gv.y;
                acc += gv.z * gv.z;
                acc += gv.w * gv.w;
            } else if constexpr (KIND == 1) {
                acc += fabsf(gv.x);
                acc += fabsf(gv.y);
                acc += fabsf(gv.z);
                acc += fabsf(gv.w);
            } else {
                const unsigned a = abs_bits(gv.x), b = abs_bits(gv.y), c2 = abs_bits(gv.z), d = abs_bits(gv.w);
                const unsigned ab = a > b ? a : b, cd = c2 > d ? c2 : d;
                const unsigned m4 = ab > cd ? ab : cd;
                mx = m4 > mx ? m4 : mx;
            }
        }
        float r;
        if constexpr (KIND == 0) r = __uint_as_float(block_max_bits(mx, reinterpret_cast<unsigned*>(sh)));
        else r = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[c] = r;
        c += (int)gridDim.x;
    });
    if constexpr (CHECK) raise_found_inf(!(z == 0.f), found_inf);
}

// torch._amp_foreach_non_finite_check_and_unscale_ over the rows of a chunk table (GradScaler._unscale_grads_ on gradients that are views
// of one flat buffer): every covered element is tested, then replaced by g * inv, one rounded product, non-finite ones included -- unless
// inv is exactly 1 (GradScaler's check-only call), when g is only read: 4 B per element instead of 8.  inv is uniform over the launch.
__global__ void __launch_bounds__(SEG_THREADS) grad_unscale_check_seg_kernel(float* __restrict__ g, const vbg_optim_chunk* __restrict__ tbl, int nchunks,
                                                                              const float* __restrict__ inv_scale, float* __restrict__ found_inf) {
    const float inv = *inv_scale;
    const bool store = inv != 1.f;
    float z = 0.f;
    walk_chunks(tbl, nchunks, [&](const vbg_optim_chunk& ch) {
        float4* g4 = reinterpret_cast<float4*>(g + ch.start);
        const int n4 = ch.length >> 2;
        if (store) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
                float4 gv = g4[i];
                fold_finite4(z, gv);
                gv.x = __fmul_rn(gv.x, inv); gv.y = __fmul_rn(gv.y, inv); gv.z = __fmul_rn(gv.z, inv); gv.w = __fmul_rn(gv.w, inv);
                g4[i] = gv;
            }
        } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int i = threadIdx.x; i < n4; i += SEG_THREADS) fold_finite4(z, g4[i]);
        }
    });
    raise_found_inf(!(z == 0.f), found_inf);
}

// ---- gradient-norm clipping on the device: the finish ------------------------------------------------------------------
// One block: partials[0 .. n) folded in double in a fixed order (thread t takes t, t + T, ...; then a fixed tree) -- summed for KIND 2
// (then sqrt) and KIND 1, their maximum with a NaN kept for KIND 0 -- and the fp32 numbers a clip needs: out[0] = the total norm,
// out[1] = the coefficient in torch's own statements -- `max_norm / (total_norm + 1e-6)` is `(total_norm + 1e-6).reciprocal() * max_norm`
// there, then `clamp(max=1.0)`, which keeps a NaN (fminf would not) and turns an inf norm into 0 -- and, where nout == 3 (vbg_clip_coef
// has two floats: nothing is stored behind out[1]), out[2] = 1.0f (gate open, or no gate) / 0.0f.  A closed gate leaves (0, 1, 0) and
// reads no partial.
constexpr int COEF_THREADS = 256;
template <int KIND>
__global__ void __launch_bounds__(COEF_THREADS) clip_coef_gate_kernel(const float* __restrict__ partials, int n, float max_norm, float norm_scale,
                                                                       const float* __restrict__ grad_scale, ClipGate gate, float* __restrict__ out, int nout) {
    __shared__ double sh[COEF_THREADS];
    if (!gate_open(gate)) {
        if (threadIdx.x == 0) {
            out[0] = 0.f;
            out[1] = 1.f;
            if (nout > 2) out[2] = 0.f;
        }
        return;
    }
    double s = 0.0;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += COEF_THREADS) {
        const float p = partials[i];
        if constexpr (KIND == 0) {
            bad = bad || p != p;
            s = fmax(s, (double)p);
        } else {
            s += (double)p;
        }
    }
    if constexpr (KIND == 0) bad = __syncthreads_or(bad);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = COEF_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            if constexpr (KIND == 0) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
            else sh[threadIdx.x] += sh[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float root;
        if constexpr (KIND == 2) root = (float)sqrt(sh[0]);
        else if constexpr (KIND == 1) root = (float)sh[0];
        else root = bad ? __uint_as_float(0x7fc00000u) : (float)sh[0];
        float total = __fmul_rn(root, norm_scale);
        if (grad_scale) total = __fmul_rn(total, (float)(1.0 / (double)*grad_scale));          // (the gradients still hold scaled values)
        const float c = __fmul_rn(__fdiv_rn(1.f, __fadd_rn(total, 1e-6f)), max_norm);
        out[0] = total;
        out[1] = c > 1.f ? 1.f : c;
        if (nout > 2) out[2] = 1.f;
    }
}

static inline int ew_grid(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g > 256 * 8) g = 256 * 8;
    if (g < 1) g = 1;
    return (int)g;
}

// Adam's bias corrections 1 - b1^step and sqrt(1 - b2^step), formed in double
struct BiasCorr { float bc1, bc2_sqrt; };
static inline BiasCorr bias_corr(float b1, float b2, int step) {
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    return BiasCorr{(float)bc1, (float)sqrt(bc2)};
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
    const BiasCorr bc = bias_corr(b1, b2, step);
    VBG_LAUNCH(adamw_kernel, dim3(ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, n, lr, b1, b2,
                       eps, wd, bc.bc1, bc.bc2_sqrt, grad_scale);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_lerp(float* avg, const float* p, long long n, float weight, void* stream) {
    VBG_CHECK_ARG(n >= 0);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(avg && p);
    const long long n4 = (ALIGNED16(avg) && ALIGNED16(p)) ? n / 4 : 0;
    VBG_LAUNCH(lerp_kernel, dim3(ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, avg, p, n4, n, weight);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_swap(float* a, float* b, long long n, void* stream) {
    VBG_CHECK_ARG(n >= 0);
    if (n == 0) return VBG_OK;
    VBG_CHECK_ARG(a && b);
    const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b, hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
    VBG_CHECK_ARG(hi - lo >= (uintptr_t)n * sizeof(float));          // the same or overlapping ranges: no thread would own its element
    const long long n4 = (ALIGNED16(a) && ALIGNED16(b)) ? n / 4 : 0;
    VBG_LAUNCH(swap_kernel, dim3(ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<unsigned*>(a),
               reinterpret_cast<unsigned*>(b), n4, n);
    VBG_LAUNCH_RET();
}

// the segmented forms: buffers 16-byte aligned (float4 access at start, a multiple of 4 elements; NULL where an entry accepts it);
// the table is device memory, the hyper-parameters are copied from host memory into the kernel arguments (no copy to the device,
// no sync)
template <bool AMP>
static int launch_sgd_seg(float* p, GradPtr<AMP> g, float* mom, const vbg_optim_chunk* chunks, int nchunks, const SgdGroups& hp,
                          const SegScale<AMP>& sc, void* stream) {
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(mom) && ALIGNED16(chunks));
    VBG_LAUNCH(sgd_seg_kernel<AMP>, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, mom, chunks, nchunks, hp, sc);
    VBG_LAUNCH_RET();
}

template <bool AMP>
static int launch_adam_seg(float* p, GradPtr<AMP> g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                           const AdamGroups& hp, const SegScale<AMP>& sc, void* stream) {
    VBG_CHECK_ARG(ALIGNED16(p) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v) && ALIGNED16(vmax) && ALIGNED16(chunks));
    VBG_LAUNCH(adam_seg_kernel<AMP>, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, p, g, m, v, vmax, chunks, nchunks, hp,
               sc);
    VBG_LAUNCH_RET();
}

// lr / momentum / wd per group, first_step shared: the default case of the kernel, and a momentum-0 group keeps writing its buffer
extern "C" int vbg_sgd_step_seg(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                                const vbg_sgd_group* groups, int ngroups, int first_step, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && mom && chunks && groups);
    SgdGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = SgdHp{groups[i].lr, groups[i].momentum, 0.f, groups[i].wd, first_step ? SGD_FIRST : 0, 1};
    return launch_sgd_seg<false>(p, g, mom, chunks, nchunks, hp, SegScale<false>{grad_scale}, stream);
}

// lr / betas / eps / wd per group, step shared: flags 0
extern "C" int vbg_adamw_step_seg(float* p, const float* g, float* m, float* v, const vbg_optim_chunk* chunks, int nchunks,
                                  const vbg_adamw_group* groups, int ngroups, int step, float grad_scale, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0 && step >= 1);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && m && v && chunks && groups);
    AdamGroups hp = {};
    for (int i = 0; i < ngroups; ++i) {
        const vbg_adamw_group& s = groups[i];
        const BiasCorr bc = bias_corr(s.b1, s.b2, step);
        hp.g[i] = AdamHp{s.lr, s.b1, s.b2, s.eps, s.wd, bc.bc1, bc.bc2_sqrt, 0};
    }
    return launch_adam_seg<false>(p, g, m, v, nullptr, chunks, nchunks, hp, SegScale<false>{grad_scale}, stream);
}

// every torch.optim option per group (flags of include/vbg.h): same table, same checks.  mom may be NULL when every group has momentum
// 0, vmax when no group has the amsgrad flag; a group's bias corrections come from ITS step.  The *_amp entries are the same calls
// with the scale and the inf flag in device memory (SegScale<true>; found_inf is required, grad_scale may be NULL) and g writable.
// the device scalars of an AMP launch: 4-byte aligned; without a clip coefficient (the *_amp entries) found_inf is required, with one
// (the *_clip entries, which refuse a NULL coefficient themselves) it may be NULL
static inline bool amp_scalars_ok(const SegScale<true>& sc) {
    return (sc.found_inf || sc.clip) && (uintptr_t)sc.found_inf % 4 == 0 && (uintptr_t)sc.scale % 4 == 0 && (uintptr_t)sc.clip % 4 == 0;
}

template <bool AMP>
static int sgd_step_seg_opt(float* p, GradPtr<AMP> g, float* mom, const vbg_optim_chunk* chunks, int nchunks, const vbg_sgd_group_opt* groups,
                            int ngroups, const SegScale<AMP>& sc, void* stream, int keep_mom = 0) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if constexpr (AMP) VBG_CHECK_ARG(amp_scalars_ok(sc));
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && chunks && groups);
    SgdGroups hp = {};
    bool any_mom = false;
    for (int i = 0; i < ngroups; ++i) {
        const vbg_sgd_group_opt& s = groups[i];
        hp.g[i] = SgdHp{s.lr, s.momentum, s.dampening, s.wd, s.flags, keep_mom != 0};
        any_mom = any_mom || s.momentum != 0.f || keep_mom;
    }
    VBG_CHECK_ARG(mom || !any_mom);
    return launch_sgd_seg<AMP>(p, g, mom, chunks, nchunks, hp, sc, stream);
}

template <bool AMP>
static int adam_step_seg_opt(float* p, GradPtr<AMP> g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                             const vbg_adam_group_opt* groups, int ngroups, const SegScale<AMP>& sc, void* stream) {
    VBG_CHECK_ARG(ngroups >= 1 && ngroups <= VBG_OPTIM_MAX_GROUPS && nchunks >= 0);
    if constexpr (AMP) VBG_CHECK_ARG(amp_scalars_ok(sc));
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(p && g && m && v && chunks && groups);
    AdamGroups hp = {};
    for (int i = 0; i < ngroups; ++i) {
        const vbg_adam_group_opt& s = groups[i];
        VBG_CHECK_ARG(s.step >= 1);
        VBG_CHECK_ARG(vmax || !(s.flags & ADAM_AMSGRAD));
        const BiasCorr bc = bias_corr(s.b1, s.b2, s.step);
        hp.g[i] = AdamHp{s.lr, s.b1, s.b2, s.eps, s.wd, bc.bc1, bc.bc2_sqrt, s.flags};
    }
    return launch_adam_seg<AMP>(p, g, m, v, vmax, chunks, nchunks, hp, sc, stream);
}

extern "C" int vbg_sgd_step_seg_opt(float* p, const float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks,
                                    const vbg_sgd_group_opt* groups, int ngroups, float grad_scale, void* stream) {
    return sgd_step_seg_opt<false>(p, g, mom, chunks, nchunks, groups, ngroups, SegScale<false>{grad_scale}, stream);
}

extern "C" int vbg_adam_step_seg_opt(float* p, const float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                                     const vbg_adam_group_opt* groups, int ngroups, float grad_scale, void* stream) {
    return adam_step_seg_opt<false>(p, g, m, v, vmax, chunks, nchunks, groups, ngroups, SegScale<false>{grad_scale}, stream);
}

extern "C" int vbg_sgd_step_seg_amp(float* p, float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks, const vbg_sgd_group_opt* groups,
                                    int ngroups, const float* grad_scale, const float* found_inf, void* stream) {
    return sgd_step_seg_opt<true>(p, g, mom, chunks, nchunks, groups, ngroups, SegScale<true>{1.f, grad_scale, found_inf, nullptr}, stream);
}

extern "C" int vbg_adam_step_seg_amp(float* p, float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                                     const vbg_adam_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf, void* stream) {
    return adam_step_seg_opt<true>(p, g, m, v, vmax, chunks, nchunks, groups, ngroups, SegScale<true>{1.f, grad_scale, found_inf, nullptr}, stream);
}

// The *_amp entries with the coefficient of a gradient-norm clip (vbg_clip_coef's out + 1) as a third device scalar, required here;
// found_inf may be NULL (no scaler), host_scale multiplies the gradient inside the rule as grad_scale does in the *_seg_opt entries.
// keep_mom != 0: a momentum-0 group goes through the momentum statement and writes its buffer, as in vbg_sgd_step_seg.
extern "C" int vbg_sgd_step_seg_clip(float* p, float* g, float* mom, const vbg_optim_chunk* chunks, int nchunks, const vbg_sgd_group_opt* groups,
                                     int ngroups, const float* grad_scale, const float* found_inf, const float* clip_coef, float host_scale,
                                     int keep_mom, void* stream) {
    VBG_CHECK_ARG(clip_coef);
    return sgd_step_seg_opt<true>(p, g, mom, chunks, nchunks, groups, ngroups, SegScale<true>{host_scale, grad_scale, found_inf, clip_coef}, stream,
                                  keep_mom);
}

extern "C" int vbg_adam_step_seg_clip(float* p, float* g, float* m, float* v, float* vmax, const vbg_optim_chunk* chunks, int nchunks,
                                      const vbg_adam_group_opt* groups, int ngroups, const float* grad_scale, const float* found_inf,
                                      const float* clip_coef, float host_scale, void* stream) {
    VBG_CHECK_ARG(clip_coef);
    return adam_step_seg_opt<true>(p, g, m, v, vmax, chunks, nchunks, groups, ngroups, SegScale<true>{host_scale, grad_scale, found_inf, clip_coef},
                                   stream);
}

// ---- the entries of the row pass (three) and of the finish (two) ----------------------------------------------------------
// kind 2 / 1 / 0 is norm type 2, 1 and inf; gate_loss: a device scalar, fp64 when gate_f64, fp32 otherwise, NULL for no gate
static inline bool gate_args(const void* loss, int f64) { return (f64 == 0 || f64 == 1) && (uintptr_t)loss % (f64 ? 8 : 4) == 0; }
static inline ClipGate make_gate(const void* loss, int f64, double threshold) { return ClipGate{loss, threshold, (float)threshold, f64}; }

// a checked kind -> f(std::integral_constant<int, KIND>{}), the template argument of both kernels
template <class F>
static int with_kind(int kind, F f) {
    if (kind == 2) return f(std::integral_constant<int, 2>{});
    if (kind == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 0>{});
}

// found_inf (4-byte aligned, checked by the entry) selects CHECK; an empty table launches nothing and looks at no other pointer
template <int KIND>
static int grad_norm_seg_launch(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, float* found_inf, ClipGate gate,
                                void* stream) {
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(g && chunks && partials && ALIGNED16(g) && ALIGNED16(chunks) && (uintptr_t)partials % 4 == 0);
    if (found_inf)
        VBG_LAUNCH((grad_norm_seg_kernel<KIND, true>), dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, g, chunks, nchunks,
                   partials, found_inf, gate);
    else
        VBG_LAUNCH((grad_norm_seg_kernel<KIND, false>), dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, g, chunks, nchunks,
                   partials, found_inf, gate);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_grad_sumsq_seg(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, void* stream) {
    VBG_CHECK_ARG(nchunks >= 0);
    return grad_norm_seg_launch<2>(g, chunks, nchunks, partials, nullptr, ClipGate{}, stream);
}

// GradScaler's hooks (vbg.optim.fuse_scaler).  Their device scalars are required and 4-byte aligned, whatever nchunks is; the flag is
// only ever set.
extern "C" int vbg_grad_sumsq_seg_inf(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, float* found_inf, void* stream) {
    VBG_CHECK_ARG(nchunks >= 0 && found_inf && (uintptr_t)found_inf % 4 == 0);
    return grad_norm_seg_launch<2>(g, chunks, nchunks, partials, found_inf, ClipGate{}, stream);
}

extern "C" int vbg_grad_unscale_check_seg(float* g, const vbg_optim_chunk* chunks, int nchunks, const float* inv_scale, float* found_inf, void* stream) {
    VBG_CHECK_ARG(nchunks >= 0 && inv_scale && found_inf && (uintptr_t)inv_scale % 4 == 0 && (uintptr_t)found_inf % 4 == 0);
    if (nchunks == 0) return VBG_OK;
    VBG_CHECK_ARG(g && chunks && ALIGNED16(g) && ALIGNED16(chunks));
    VBG_LAUNCH(grad_unscale_check_seg_kernel, dim3(ew_grid(nchunks, 1)), dim3(SEG_THREADS), 0, (hipStream_t)stream, g, chunks, nchunks, inv_scale,
               found_inf);
    VBG_LAUNCH_RET();
}

// found_inf is optional here (NULL: no check); with it the rows walk whatever the gate says
extern "C" int vbg_grad_norm_seg(const float* g, const vbg_optim_chunk* chunks, int nchunks, float* partials, int kind, float* found_inf,
                                 const void* gate_loss, int gate_f64, double gate_threshold, void* stream) {
    VBG_CHECK_ARG(nchunks >= 0 && kind >= 0 && kind <= 2 && (uintptr_t)found_inf % 4 == 0 && gate_args(gate_loss, gate_f64));
    const ClipGate gate = make_gate(gate_loss, gate_f64, gate_threshold);
    return with_kind(kind, [&](auto k) { return grad_norm_seg_launch<k()>(g, chunks, nchunks, partials, found_inf, gate, stream); });
}

// one block whatever n is (n == 0: nothing is read); `out` has nout floats, 4-byte aligned like the other device scalars
template <int KIND>
static int clip_coef_launch(const float* partials, int n, float max_norm, float norm_scale, const float* grad_scale, ClipGate gate, float* out,
                            int nout, void* stream) {
    VBG_CHECK_ARG(n >= 0 && out && (uintptr_t)out % 4 == 0 && (partials || n == 0) && (uintptr_t)partials % 4 == 0 && (uintptr_t)grad_scale % 4 == 0);
    VBG_LAUNCH(clip_coef_gate_kernel<KIND>, dim3(1), dim3(COEF_THREADS), 0, (hipStream_t)stream, partials, n, max_norm, norm_scale, grad_scale, gate,
               out, nout);
    VBG_LAUNCH_RET();
}

extern "C" int vbg_clip_coef(const float* partials, int n, float max_norm, float norm_scale, const float* grad_scale, float* out, void* stream) {
    return clip_coef_launch<2>(partials, n, max_norm, norm_scale, grad_scale, ClipGate{}, out, 2, stream);
}

extern "C" int vbg_clip_coef_gate(const float* partials, int n, int kind, float max_norm, float norm_scale, const float* grad_scale,
                                  const void* gate_loss, int gate_f64, double gate_threshold, float* out, void* stream) {
    VBG_CHECK_ARG(kind >= 0 && kind <= 2 && gate_args(gate_loss, gate_f64));
    const ClipGate gate = make_gate(gate_loss, gate_f64, gate_threshold);
    return with_kind(kind, [&](auto k) { return clip_coef_launch<k()>(partials, n, max_norm, norm_scale, grad_scale, gate, out, 3, stream); });
}
