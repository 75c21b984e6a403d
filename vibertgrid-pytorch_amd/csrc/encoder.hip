// One encoder layer forward as ONE C call (round 6), and its backward as one more (vbg_bert_layer_bwd, below).
//
// transformers' BertLayer inside BertModel (reference model/BERTgrid_generator.py:134) is seven launches of this library: the stacked
// Q/K/V projection, the fused attention, the output projection, dropout + residual + LayerNorm, FFN1 (+ GELU), FFN2, dropout + residual +
// LayerNorm.  Issued from Python every launch costs 10-25 us of host time (a descriptor built field by field, a ctypes call), 165 us per
// layer, which is what bounds single-document inference and the host-bound phases of the reference's own training loop.  This entry builds
// the same seven descriptors from one layer descriptor and launches them back to back on the caller's stream: the kernels, their
// arguments and their order are exactly those of the per-launch path (vbg/functions.py BertLayerFn.forward), so results are bit-identical
// (tests/test_gpu_layer_entry.py).  No device code here.
#include "vbg_common.h"
#include "../../include/vbg.h"

namespace {
inline bool present(const vbg_planes_ref& p) { return p.buf != nullptr; }
inline void set_a(vbg_plane_gemm_desc& g, const vbg_planes_ref& p) { g.A = p.buf; g.a_plane = p.plane; g.lda = p.ld; }
inline void set_b(vbg_plane_gemm_desc& g, const vbg_planes_ref& p) { g.B = p.buf; g.b_plane = p.plane; g.ldb = p.ld; }
inline void set_cp(vbg_plane_gemm_desc& g, const vbg_planes_ref& p) { if (p.buf) { g.Cp = p.buf; g.c_plane = p.plane; g.ldp = p.ld; } }
inline void set_cq(vbg_plane_gemm_desc& g, const vbg_planes_ref& p) { if (p.buf) { g.Cq = p.buf; g.q_plane = p.plane; g.ldq = p.ld; } }
inline vbg_plane_gemm_desc nt_product(int M, int N, int K, float* C, const float* bias, int tile, int form) {
    vbg_plane_gemm_desc g{};
    g.M = M; g.N = N; g.K = (K + 31) / 32 * 32;
    g.C = C; g.ldc = C ? N : (N + 3) / 4 * 4;
    g.bias = bias; g.epi = VBG_EPI_NONE; g.alpha = 1.0f; g.splitk = 1; g.tile = tile; g.form = form;
    return g;
}
}  // namespace

extern "C" int vbg_bert_layer_fwd(const vbg_bert_layer_fwd_desc* dp, void* stream) {
    VBG_CHECK_ARG(dp != nullptr);
    const vbg_bert_layer_fwd_desc& d = *dp;
    VBG_CHECK_ARG(d.ntok > 0 && d.hidden > 0 && d.inter > 0 && d.heads > 0 && d.hidden % 32 == 0 && d.inter % 32 == 0 && d.hidden == d.heads * 64);
    VBG_CHECK_ARG(d.x && present(d.xa) && present(d.wqkv) && present(d.wo) && present(d.wi) && present(d.wo2));
    VBG_CHECK_ARG(d.bqkv && d.bo && d.bi && d.bo2 && d.g1 && d.b1 && d.g2 && d.b2);
    VBG_CHECK_ARG(present(d.pqkv) && d.ctx && d.lse && d.ao && d.x1 && d.xhat1 && d.rstd1 && d.h && d.fo && d.y && d.xhat2 && d.rstd2);
    VBG_CHECK_ARG(d.form_qkv >= 0 && d.form_qkv <= 2 && d.form_ao >= 0 && d.form_ao <= 2 && d.form_ffn >= 0 && d.form_ffn <= 2 && d.form_attn >= 0 && d.form_attn <= 2);
    // the operand each product reads must be there in the form the product runs
    VBG_CHECK_ARG(present(d.form_ao ? d.pctxq : d.pctx) && present(d.form_ffn ? d.px1q : d.px1) && present(d.form_ffn ? d.pgq : d.pg));
    VBG_CHECK_ARG((d.mask_q == nullptr) == (d.mask_k == nullptr) && (d.mask_q == nullptr || d.mask_off != nullptr));
    const int ntok = d.ntok, hid = d.hidden, inter = d.inter;
    int rc;
    // ---- Q, K, V: one product over the stacked projections; the result leaves as planes only (the attention kernels' operands)
    {
        vbg_plane_gemm_desc g = nt_product(ntok, 3 * hid, hid, nullptr, d.bqkv, d.tile_qkv, d.form_qkv);
        set_a(g, d.xa); set_b(g, d.wqkv);
        if (d.form_attn) set_cq(g, d.pqkv); else set_cp(g, d.pqkv);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- fused attention
    {
        vbg_attn_desc a{};
        a.mode = VBG_ATTN_FWD; a.heads = d.heads; a.ntasks = d.ntasks; a.max_len = d.max_len;
        a.tasks = d.tasks; a.seq_len = d.seq_len; a.seq_row0 = d.seq_row0; a.pad_off = d.pad_off; a.ntok_pad = d.ntok_pad;
        a.qkv = d.pqkv.buf; a.qkv_plane = d.pqkv.plane; a.qkv_ld = d.pqkv.ld;
        a.out = d.ctx; a.ldo = hid; a.lse = d.lse;
        if (d.kbar) { a.kbar = d.kbar; a.ldk = hid; }
        if (present(d.pctx)) { a.out_planes = d.pctx.buf; a.op_plane = d.pctx.plane; a.op_ld = d.pctx.ld; }
        if (present(d.pctxq)) { a.out_pair = d.pctxq.buf; a.oq_plane = d.pctxq.plane; a.oq_ld = d.pctxq.ld; }
        if (d.mask_q) { a.mask_q = d.mask_q; a.mask_k = d.mask_k; a.mask_off = d.mask_off; a.keep_scale = d.keep_scale; }
        else a.keep_scale = 1.0f;
        a.scale = d.attn_scale; a.form = d.form_attn;
        if ((rc = vbg_attn(&a, stream)) != VBG_OK) return rc;
    }
    // ---- attention output projection
    {
        vbg_plane_gemm_desc g = nt_product(ntok, hid, hid, d.ao, d.bo, d.tile_ao, d.form_ao);
        set_a(g, d.form_ao ? d.pctxq : d.pctx); set_b(g, d.wo);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- x1 = LayerNorm(dropout(ao) + x), with its planes for FFN1
    if ((rc = vbg_dropout_add_ln_fwd_planes(d.ao, d.x, ntok, hid, d.g1, d.b1, d.eps, d.drop_p, d.seed, d.stream_id0 + 1, d.x1, d.xhat1, d.rstd1,
                                            d.px1.buf, (int)d.px1.ld, d.px1.plane, d.px1q.buf, (int)d.px1q.ld, d.px1q.plane, stream)) != VBG_OK) return rc;
    // ---- FFN1: h = x1 Wi^T + bi, gelu(h) as planes only
    {
        vbg_plane_gemm_desc g = nt_product(ntok, inter, hid, d.h, d.bi, d.tile_ffn1, d.form_ffn);
        g.epi = VBG_EPI_GELU_DUAL;
        set_a(g, d.form_ffn ? d.px1q : d.px1); set_b(g, d.wi);
        set_cp(g, d.pg);
        if (d.form_ffn) set_cq(g, d.pgq);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- FFN2
    {
        vbg_plane_gemm_desc g = nt_product(ntok, hid, inter, d.fo, d.bo2, d.tile_ffn2, d.form_ffn);
        set_a(g, d.form_ffn ? d.pgq : d.pg); set_b(g, d.wo2);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- y = LayerNorm(dropout(fo) + x1), with its planes for the next layer's first product
    return vbg_dropout_add_ln_fwd_planes(d.fo, d.x1, ntok, hid, d.g2, d.b2, d.eps, d.drop_p, d.seed, d.stream_id0 + 2, d.y, d.xhat2, d.rstd2,
                                         d.py.buf, (int)d.py.ld, d.py.plane, d.pyq.buf, (int)d.pyq.ld, d.pyq.plane, stream);
}

// The layer's backward as ONE C call: the all-pair backward on the bound route (vbg/functions.py BertLayerFn._backward_pair), ten launches
// -- twelve in deterministic mode, whose two column sums run as launches of their own (csrc/det.hip) -- with the descriptors and the order
// of the per-launch path (vbg/ops.py bert_layer_bwd_launches): bit-identical results (tests/test_gpu_layer_bwd_entry.py).
namespace {
// a data-gradient product on pair planes: C[ntok, N] = A[ntok, K] Wt[N, K]^T, A scaled by the power of two of the slot a_amax
inline vbg_plane_gemm_desc dgrad_product(int M, int N, int K, const vbg_planes_ref& a, const vbg_planes_ref& wt, const unsigned* a_amax, int tile, int form) {
    vbg_plane_gemm_desc g = nt_product(M, N, K, nullptr, nullptr, tile, form);
    set_a(g, a); set_b(g, wt);
    g.a_amax = a_amax;
    return g;
}
inline void accumulate_into(vbg_plane_gemm_desc& g, float* C, int N, unsigned* c_amax) { g.C = C; g.ldc = N; g.accumulate = 1; g.c_amax = c_amax; }
inline void bounded_pair_out(vbg_plane_gemm_desc& g, const vbg_planes_ref& q, const unsigned* ref_in, const unsigned* l1, float mul, unsigned* ref_out) {
    set_cq(g, q);
    g.cq_ref_in = ref_in; g.cq_l1_in = l1; g.cq_mul = mul; g.cq_ref_out = ref_out;
}
inline void wgrad_group(vbg_plane_group& g, const vbg_planes_ref& dy, int M, const vbg_planes_ref& x, int N, float* dw, const unsigned* a_amax) {
    g.A = dy.buf; g.a_plane = dy.plane; g.lda = dy.ld;
    g.B = x.buf; g.b_plane = x.plane; g.ldb = x.ld;
    g.C = dw; g.ldc = N; g.M = M; g.N = N; g.a_amax = a_amax;
}
}  // namespace

extern "C" int vbg_bert_layer_bwd(const vbg_bert_layer_bwd_desc* dp, void* stream) {
    VBG_CHECK_ARG(dp != nullptr);
    const vbg_bert_layer_bwd_desc& d = *dp;
    VBG_CHECK_ARG(d.ntok > 0 && d.hidden > 0 && d.inter > 0 && d.heads > 0 && d.hidden % 256 == 0 && d.inter % 32 == 0 && d.hidden == d.heads * 64);
    VBG_CHECK_ARG(d.form >= 1 && d.form <= 2 && d.form_attn >= 1 && d.form_attn <= 2);
    VBG_CHECK_ARG(d.dy && d.xhat2 && d.rstd2 && d.g2 && d.xhat1 && d.rstd1 && d.g1 && d.h && d.ctx && d.kbar && d.lse);
    VBG_CHECK_ARG(present(d.pqkv) && present(d.qx) && present(d.qctx) && present(d.qx1) && present(d.qg));
    VBG_CHECK_ARG(present(d.wqkv_t) && present(d.wo_t) && present(d.wi_t) && present(d.wo2_t) && d.l1_wo2 && d.l1_wo);
    VBG_CHECK_ARG(d.s_dy && d.s_dfo && d.s_dfo_ref && d.s_dh && d.s_dx1 && d.s_dao && d.s_dao_ref && d.s_dctx && d.s_dqkv && d.s_dx);
    VBG_CHECK_ARG(d.ln_ws && d.delta && d.tasks && d.seq_len && d.seq_row0 && d.pad_off);
    VBG_CHECK_ARG(!d.deterministic || (d.det_scratch != nullptr && d.det_ws != nullptr));
    VBG_CHECK_ARG(present(d.qdfo) && present(d.qdh) && present(d.qdao) && present(d.pdctx) && present(d.qdqkv) && d.dx1 && d.dqkv);
    VBG_CHECK_ARG(d.qdfo.ld == d.hidden && d.qdao.ld == d.hidden && d.qdqkv.ld >= 3 * d.hidden && d.qdqkv.ld <= 0x7fffffffll);
    VBG_CHECK_ARG(d.dx && d.dg2 && d.db2 && d.dbo2 && d.dbi && d.dg1 && d.db1 && d.dbo && d.dbqkv && d.dwo2 && d.dwi && d.dwo && d.dwqkv);
    VBG_CHECK_ARG((d.mask_q == nullptr) == (d.mask_k == nullptr) && (d.mask_q == nullptr || d.mask_off != nullptr));
    const int ntok = d.ntok, hid = d.hidden, inter = d.inter;
    int rc;
    // ---- 1. LayerNorm 2 backward: dfo as pair planes scaled by a bound, the FFN output projection's bias gradient riding along
    if ((rc = vbg_dropout_add_ln_bwd_pair(d.dy, d.xhat2, d.rstd2, ntok, hid, d.g2, d.drop_p, d.seed, d.stream_id0 + 2, d.qdfo.buf, (int)d.qdfo.ld,
                                          d.qdfo.plane, d.dx1, d.dg2, d.db2, d.dbo2, d.ln_ws, d.s_dy, d.s_dfo, d.s_dfo_ref, stream)) != VBG_OK) return rc;
    // ---- 2. dL/dh = (dfo Wo2) o gelu'(h): pair planes only, by a bound; its column sums are FFN1's bias gradient
    {
        vbg_plane_gemm_desc g = dgrad_product(ntok, inter, hid, d.qdfo, d.wo2_t, d.s_dfo_ref, d.tile_dh, d.form);
        g.epi = VBG_EPI_MUL_GELU_GRAD; g.C2 = const_cast<float*>(d.h);
        bounded_pair_out(g, d.qdh, d.s_dfo, d.l1_wo2, d.cq_mul_dh, d.s_dh);
        if (d.deterministic) { g.C = d.det_scratch; g.ldc = (inter + 3) / 4 * 4; }
        else g.colsum = d.dbi;
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
        if (d.deterministic && (rc = vbg_colsum_det(d.det_scratch, g.ldc, ntok, inter, d.dbi, 1, d.det_ws, stream)) != VBG_OK) return rc;
    }
    // ---- 3. dx1 += dh Wi; max |dx1| rides along (LayerNorm 1's bound)
    {
        vbg_plane_gemm_desc g = dgrad_product(ntok, hid, inter, d.qdh, d.wi_t, d.s_dh, d.tile_dx1, d.form);
        accumulate_into(g, d.dx1, hid, d.s_dx1);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- 4. LayerNorm 1 backward: dao as pair planes, the attention-output projection's bias gradient
    if ((rc = vbg_dropout_add_ln_bwd_pair(d.dx1, d.xhat1, d.rstd1, ntok, hid, d.g1, d.drop_p, d.seed, d.stream_id0 + 1, d.qdao.buf, (int)d.qdao.ld,
                                          d.qdao.plane, d.dx, d.dg1, d.db1, d.dbo, d.ln_ws, d.s_dx1, d.s_dao, d.s_dao_ref, stream)) != VBG_OK) return rc;
    // ---- 5. d(context) = dao Wo: the dO operand of the attention backward, pair planes only, by a bound
    {
        vbg_plane_gemm_desc g = dgrad_product(ntok, hid, hid, d.qdao, d.wo_t, d.s_dao_ref, d.tile_dctx, d.form);
        bounded_pair_out(g, d.pdctx, d.s_dao, d.l1_wo, d.cq_mul_dctx, d.s_dctx);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- 6, 7. fused attention backward: dQ (writes delta), then dK / dV into the same d(qkv); max |d(qkv)| rides on both
    {
        vbg_attn_desc a{};
        a.mode = VBG_ATTN_DQ; a.heads = d.heads; a.ntasks = d.ntasks; a.max_len = d.max_len;
        a.tasks = d.tasks; a.seq_len = d.seq_len; a.seq_row0 = d.seq_row0; a.pad_off = d.pad_off; a.ntok_pad = d.ntok_pad;
        a.qkv = d.pqkv.buf; a.qkv_plane = d.pqkv.plane; a.qkv_ld = d.pqkv.ld;
        a.dO = d.pdctx.buf; a.do_plane = d.pdctx.plane; a.do_ld = d.pdctx.ld;
        a.out = d.dqkv; a.ldo = 3 * hid; a.lse = d.lse; a.delta = d.delta;
        a.kbar = d.kbar; a.ldk = hid; a.o = d.ctx;
        if (d.mask_q) { a.mask_q = d.mask_q; a.mask_k = d.mask_k; a.mask_off = d.mask_off; a.keep_scale = d.keep_scale; }
        else a.keep_scale = 1.0f;
        a.scale = d.attn_scale; a.form = d.form_attn; a.out_amax = d.s_dqkv; a.do_amax = d.s_dctx;
        if ((rc = vbg_attn(&a, stream)) != VBG_OK) return rc;
        a.mode = VBG_ATTN_DKV; a.kbar = nullptr; a.ldk = 0; a.o = nullptr;
        if ((rc = vbg_attn(&a, stream)) != VBG_OK) return rc;
    }
    // ---- 8. d(qkv) as pair planes scaled by its measured maximum; its column sums are the stacked Q/K/V bias gradient
    if (d.deterministic && (rc = vbg_colsum_det(d.dqkv, 3 * hid, ntok, 3 * hid, d.dbqkv, 1, d.det_ws, stream)) != VBG_OK) return rc;
    if ((rc = vbg_split_planes_pair(d.dqkv, 3 * hid, ntok, 3 * hid, d.qdqkv.buf, (int)d.qdqkv.ld, d.qdqkv.plane, d.s_dqkv,
                                    d.deterministic ? nullptr : d.dbqkv, stream)) != VBG_OK) return rc;
    // ---- 9. dx += d(qkv) Wqkv; max |dx| rides along (the bound of the layer below)
    {
        vbg_plane_gemm_desc g = dgrad_product(ntok, hid, 3 * hid, d.qdqkv, d.wqkv_t, d.s_dqkv, d.tile_dx, d.form);
        accumulate_into(g, d.dx, hid, d.s_dx);
        if ((rc = vbg_plane_gemm(&g, stream)) != VBG_OK) return rc;
    }
    // ---- 10. the four weight gradients: one grouped TN launch over the token rows
    vbg_plane_gemm_desc g{};
    g.ngroups = 4; g.trans = 1; g.accumulate = 1; g.tile = d.tile_wgrad; g.alpha = 1.0f; g.splitk = 1; g.K = ntok; g.form = d.form;
    wgrad_group(g.grp[0], d.qdfo, hid, d.qg, inter, d.dwo2, d.s_dfo_ref);
    wgrad_group(g.grp[1], d.qdh, inter, d.qx1, hid, d.dwi, d.s_dh);
    wgrad_group(g.grp[2], d.qdao, hid, d.qctx, hid, d.dwo, d.s_dao_ref);
    wgrad_group(g.grp[3], d.qdqkv, 3 * hid, d.qx, hid, d.dwqkv, d.s_dqkv);
    return vbg_plane_gemm(&g, stream);
}
