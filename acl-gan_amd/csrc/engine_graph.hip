// ------------------------------------------------------------------------------------------
// engine_graph.hip -- the step engine's graph building blocks and the networks built from them.
// Every function runs the forward immediately and, when gradients are wanted, pushes one closure
// on the tape.
// ------------------------------------------------------------------------------------------
#include "engine.h"

namespace aclgan {

// Conv2dBlock.forward (networks.py:365-371) [+ preceding nn.Upsample, + ResBlock residual add]
//
// Storage under a 16-bit compute dtype (round 3; ctx.act16()): the block's output is stored in the 16-bit dtype when it is wide
// (Co % 64 == 0) and the caller says its consumers read 16-bit (out16: everything except the input of the 7x7 image-side output layer);
// the conv output in front of a normalisation layer likewise when the 16-bit-storage kernels run it (conv16s_ok, ctx.co16).  Gradients:
// d(out) follows out unless a consumer's input-gradient kernel can only write fp32 (the sub-pixel layers); d(conv output) is 16-bit
// exactly when this layer's backward runs on the 16-bit-storage kernels.  Kernels that take only fp32 never see a 16-bit tensor: the
// rules below keep it so, and every launch site checks.
static int conv_block(aclgan_ctx& c, const PW& W, bool train_w, Act* in, int Co, int k, int stride, int pad, int up, int act,
                      const NormSpec& ns, Act* residual, Act** out_p, int out16 = 1) {
    aclgan_conv_desc d;
    d.B = in->B; d.Hi = in->H; d.Wi = in->W; d.Ci = in->C; d.Co = Co; d.k = k; d.stride = stride; d.pad = pad; d.upsample = up;
    d.act = ns.kind == ACLGAN_NORM_NONE ? act : ACLGAN_ACT_NONE;
    ConvGeom g;
    CHK(make_geom(&d, &g));
    if (!W.w) { set_error("conv_block: parameters not bound"); return ACLGAN_EINVAL; }
    CHK(c.need(in)); CHK(c.need(residual));      // (another lane may have produced them)
    Act* const gin = in;                          // the tensor this block's input gradient is delivered to
    const bool want_grad = train_w || in->need_grad || ns.dw != nullptr;
    const bool has_norm = ns.kind != ACLGAN_NORM_NONE;
    // 16-bit MFMA path (compute dtype bf16 / fp16): per operator, whenever the shape has a 16-bit kernel
    const int dt = c.dtype;
    const bool h16 = dt != ACLGAN_DTYPE_FP32 && W.w16 != nullptr;
    const bool f16 = h16 && conv16_eligible(g, 0), d16 = h16 && conv16_eligible(g, 1), w16 = h16 && conv16_eligible(g, 2);
    const bool a16 = h16 && c.act16();
    const bool s_bwd = a16 && f16 && d16 && w16 && conv16s_ok(g, 1);                 // backward on the 16-bit-storage kernels
    const bool s_fwd = a16 && f16 && conv16s_ok(g, 0) && in->dt != 0;                 // forward on the LDS-DMA kernel
    // carried encodings (aclgan_ctx: CarryRec).  keep: this block's tensors go to the carry region and a CarryBlock says where; everything the
    // backward of the adopting gen_update depends on is decided as that update decides it (tw).  adopt: the tensors are the kept ones, no launch.
    const bool keep = c.carry_mode == ACLGAN_CARRY_KEEP, adopt = c.carry_mode == ACLGAN_CARRY_ADOPT, carried = keep || adopt;
    const bool tw = train_w || keep;
    aclgan_ctx::CarryBlock cb_dry = {};
    aclgan_ctx::CarryBlock* cb = &cb_dry;
    if (carried && !c.dry) {
        std::vector<aclgan_ctx::CarryBlock>& blocks = c.carry.blocks[c.carry_pass];
        if (keep) { blocks.push_back(cb_dry); cb = &blocks.back(); }
        else {
            if (c.carry_blk >= blocks.size()) { set_error("conv_block: the kept encodings hold no block %zu", c.carry_blk); return ACLGAN_EINVAL; }
            cb = &blocks[c.carry_blk++];
        }
    }
    // a tensor of this block: in the carry region when its pass is carried (the CarryBlock slot says where), in the arena otherwise
    auto buf = [&](float* aclgan_ctx::CarryBlock::*slot, size_t bytes) -> float* {
        if (!carried) return (float*)c.alloc(bytes);
        if (adopt && !c.dry) return cb->*slot;
        float* p = (float*)c.alloc_carry(bytes);      // (an adopting dry run reserves what the keeping call will have written)
        cb->*slot = p;
        return p;
    };
    auto act_in = [&](float* aclgan_ctx::CarryBlock::*slot, int B_, int H_, int W_, int C_, bool grad, int st) -> Act* {
        float* at = carried ? buf(slot, (size_t)B_ * H_ * W_ * C_ * (st ? 2 : 4)) : nullptr;
        return c.new_act(B_, H_, W_, C_, grad, st, carried ? &at : nullptr);
    };
    if (in->dt != 0 && !(f16 && (w16 || !tw))) {
        // a 16-bit activation reaches a layer whose forward or weight-gradient kernel only reads fp32 (odd widths of reduced test
        // networks: Cout or Cin a multiple of 32 but not of 64): one fp32 copy serves both; the input gradient goes to the original
        Act* in32 = act_in(&aclgan_ctx::CarryBlock::in32, in->B, in->H, in->W, in->C, false, 0);
        NEED_ACT(in32);
        if (!adopt) RUN(cast_storage(in->d, in->dt, in32->d, 0, in->numel(), c.st));
        in = in32;                                // data source of this block; gradients still go to the original (gin)
    }
    const int out_st = (a16 && Co % 64 == 0 && out16) ? dt : 0;
    const int co_st = has_norm ? ((s_bwd && sw(SW_CO16)) ? dt : 0) : ((f16 || !out_st) ? out_st : 0);
    if (adopt && !c.dry && (cb->B != g.B || cb->H != g.Ho || cb->W != g.Wo || cb->C != Co || cb->co_st != co_st || cb->out_st != out_st)) {
        set_error("conv_block: the kept encodings do not match this layer (%d x %d x %d x %d)", g.B, g.Ho, g.Wo, Co);
        return ACLGAN_EINVAL;
    }
    if (keep) { cb->B = g.B; cb->H = g.Ho; cb->W = g.Wo; cb->C = Co; cb->co_st = co_st; cb->out_st = out_st; }
    Act* co = act_in(&aclgan_ctx::CarryBlock::co, g.B, g.Ho, g.Wo, Co, want_grad, co_st);
    NEED_ACT(co);
    Act* out = co;
    float *mean = nullptr, *rstd = nullptr, *ss = nullptr;
    const int HW = g.Ho * g.Wo;
    if (has_norm) {
        out = act_in(&aclgan_ctx::CarryBlock::out, g.B, g.Ho, g.Wo, Co, want_grad, out_st);
        NEED_ACT(out);
        const int nstat = ns.kind == ACLGAN_NORM_LN ? g.B : g.B * Co;
        mean = buf(&aclgan_ctx::CarryBlock::mean, (size_t)nstat * 4); rstd = buf(&aclgan_ctx::CarryBlock::rstd, (size_t)nstat * 4);
        NEED(mean); NEED(rstd);
        // the fused coefficients of the apply stay until the backward: its ReLU mask is then the sign of the same fmaf(x, scale, shift), and
        // neither backward pass reads y (2 of 6 / 1 of 4 tensor reads of the reduce / apply of every activated norm layer)
        if ((want_grad || keep) && (act == ACLGAN_ACT_RELU || act == ACLGAN_ACT_LRELU) && sw(SW_NORM_MASK)) {
            ss = buf(&aclgan_ctx::CarryBlock::ss, (size_t)2 * g.B * Co * 4);
            NEED(ss);
        }
        co->gdt = s_bwd ? dt : 0;             // read by this layer's dgrad / wgrad kernels
    } else if (out_st && !co_st) {            // an fp32-only kernel (image-side first layers) feeding 16-bit consumers: one conversion pass
        out = act_in(&aclgan_ctx::CarryBlock::out, g.B, g.Ho, g.Wo, Co, want_grad, out_st);
        NEED_ACT(out);
        out->gdt = 0;                         // this layer's backward kernels read fp32
    } else {
        out->gdt = s_bwd ? co_st : 0;         // (fp32 d with 16-bit-storage backward kernels: converted out of place in the backward)
    }
    if (gin->need_grad && !s_bwd) gin->gdt = 0;   // this layer's input-gradient kernels write fp32
    // Winograd layers: the forward's input transform V = B^T x B is exactly what the weight gradient needs again -- keep it (persistent
    // until the tape has run: 75 MB per ResBlock convolution at 256x256 B=8, ~6 GB per update) instead of recomputing it
    // Bounded: the kept transforms of one update may take at most ACLGAN_KEEPV_BUDGET_GB of the arena (default 64 GB of the 288 GB; 256x256
    // B=8 needs 6.5 GB, 512x512 B=4 13 GB, B=32 26 GB); beyond it a layer's weight gradient recomputes V (same result bit for bit).
    // (an adopted block has no forward that could leave V: its weight gradient recomputes it, as beyond the budget.  The forward itself does not
    //  depend on keeping V: conv_wino_keep_bytes offers it only where neither the fused kernel nor the bf16x3 GEMM runs, i.e. where the
    //  three-launch fp32 pipeline runs either way, and the encoders have no sub-pixel layer)
    float* keepV = nullptr;
    if (train_w && !adopt && !f16 && !w16) {
        const size_t kb = conv_fwd_keep_bytes(g);
        if (kb && c.keep_total + kb <= (size_t)(sw_real(SW_KEEPV_BUDGET_GB) * 1073741824.0) + 1) { keepV = (float*)c.alloc(kb); NEED(keepV); c.keep_total += kb; }
    }
    const size_t ubytes = f16 ? 0 : conv_wino_u_bytes(g);          // fp32 Winograd layer: its filter transform is cached per update
    if (ubytes && !adopt && c.ucache_reserve(W.w, g.up ? 2 : 0, ubytes)) { set_error("workspace too small (filter-transform cache)"); return ACLGAN_ENOMEM; }
    const double es_in = in->dt ? 2.0 : 4.0, es_co = co->dt ? 2.0 : 4.0, es_out = out->dt ? 2.0 : 4.0, es_w = f16 ? 2.0 : 4.0;
    if (!adopt) c.count(es_in * (double)in->numel() + es_w * (double)Co * g.K + 4.0 * Co + es_co * (double)co->numel());             // conv: x, w, bias -> y
    if (!adopt) c.exec_flops += conv_exec_flops(g, 0, f16);
    if (out != co && !adopt) c.count((es_co + es_out) * (double)co->numel() + ((has_norm && residual) ? (residual->dt ? 2.0 : 4.0) * (double)co->numel() : 0.0));   // norm+act(+residual) / conversion: y -> out
    const size_t mark = c.top;
    if (!adopt) {      // (an adopted block: the forward below ran in the dis_update that kept it)
    // normalisation statistics from the conv epilogue where the forward kernel offers them (Winograd output transform)
    const int schunk = !has_norm ? 0 : (s_fwd ? conv_fwd16s_stats_chunk(g) : (!f16 ? conv_fwd_stats_chunk(g) : 0));
    float* stats = nullptr;
    if (schunk) { stats = c.allocf((size_t)2 * g.B * (HW / schunk) * Co); NEED(stats); }
    {
        const size_t fmark = c.top;
        void* fscr = nullptr;
        const size_t fb = s_fwd ? 0 : (f16 ? conv_fwd16_scratch_bytes(g) : conv_fwd_scratch_bytes(g));   // merged phase weights (upsample + 5x5 layers), split-K partials
        if (fb) { fscr = c.alloc(fb); NEED(fscr); }
        if (s_fwd) RUN(conv_fwd16s(g, dt, in->d, W.w16, W.b, co->d, co->dt, c.st, stats));
        else if (f16) RUN(conv_fwd16(g, dt, in->dt ? nullptr : in->d, W.w, W.w16, W.b, co->d, fscr, c.st, in->dt ? in->d : nullptr, co->dt));
        else RUN(conv_fwd(g, in->d, W.w, W.b, co->d, c.st, fscr, stats, keepV));
        c.top = fmark;
    }
    NormST nst;
    nst.x = co->dt; nst.y = out->dt; nst.res = residual ? residual->dt : 0;
    if (has_norm) {
        void* scr = c.alloc(norm_scratch_bytes(g.B, HW, Co));
        NEED(scr);
        RUN(norm_fwd(ns.kind, act, g.B, HW, Co, co->d, ns.w, ns.b, ns.w_stride, residual ? residual->d : nullptr, out->d, mean, rstd, scr, c.st, stats, schunk, &nst, ss));
    } else if (out != co) {
        RUN(cast_storage(co->d, co->dt, out->d, out->dt, co->numel(), c.st));
    }
    }
    c.top = mark;
    *out_p = out;
    if (c.mask_dst && !c.dry && want_grad && (act == ACLGAN_ACT_RELU || act == ACLGAN_ACT_LRELU)) {
        // diagnostics: the mask this block's backward will apply = the sign of its activated output (out > 0 <=> pre-activation > 0)
        unsigned char* dst = nullptr;
        CHK(c.mask_push(out->B, out->H, out->W, out->C, act, (size_t)out->numel(), &dst));
        RUN(positive_mask(out->d, out->dt, dst, out->numel(), c.st));
    }
    c.wrote(out); c.wrote(co);
    if (!want_grad) return ACLGAN_OK;
    const bool ln_train = ns.kind == ACLGAN_NORM_LN && ns.dw != nullptr;
    c.push([=](aclgan_ctx& c) -> int {
        if (!out->gw) return ACLGAN_OK;   // no gradient reached this block
        CHK(c.acq(out));
        if (residual && residual->need_grad) CHK(c.acq(residual));
        if (gin->need_grad) CHK(c.acq(gin));
        // backward of norm / activation: x (or y), dy -> dx (+ dres); wgrad: x, dy -> dw, db; dgrad: dy, w -> dx
        const double eg_out = out->gdt ? 2.0 : 4.0, eg_co = (has_norm ? co->gdt : (s_bwd ? dt : out->gdt)) ? 2.0 : 4.0, eg_in = gin->gdt ? 2.0 : 4.0;
        c.count((es_co + eg_out + eg_co) * (double)co->numel() + ((residual && residual->need_grad) ? (residual->gdt ? 2.0 : 4.0) * (double)co->numel() : 0.0));
        if (train_w) { c.count(es_in * (double)in->numel() + eg_co * (double)co->numel() + 4.0 * ((double)Co * g.K + Co)); c.exec_flops += conv_exec_flops(g, 2, w16); }
        if (gin->need_grad) { c.count(eg_co * (double)co->numel() + es_w * (double)Co * g.K + eg_in * (double)in->numel()); c.exec_flops += conv_exec_flops(g, 1, d16); }
        const bool side = train_w && sw(SW_SIDE_STREAM);      // this layer's weight gradient goes to the side stream
        if (ubytes && gin->need_grad && !d16 && c.ucache_reserve(W.w, g.up ? 3 : 1, ubytes)) { set_error("workspace too small (filter-transform cache)"); return ACLGAN_ENOMEM; }
        float* g16 = nullptr;
        const size_t mark_pre = c.top;
        if (!has_norm && s_bwd && out->gdt == 0) {      // (with the side stream: kept below the closure's scratch mark -- that stream may read it later)
            g16 = (float*)c.alloc((size_t)out->numel() * 2);
            NEED(g16);
        }
        // LayerNorm gamma / beta gradients are parameter gradients: with the side stream on they are added there (the per-sample
        // totals sbc [B][C][2] stay put until then: allocated below the closure's scratch mark)
        float* sbc = nullptr;
        if (ln_train && side) { sbc = c.allocf((int64_t)2 * g.B * Co); NEED(sbc); }
        const size_t mark0 = side ? c.top : mark_pre;
        const float* dyp = nullptr;       // gradient w.r.t. the conv output, as the dgrad / wgrad kernels read it
        int dy_st = 0;
        if (has_norm) {
            const size_t mark = c.top;
            void* scr = c.alloc(norm_scratch_bytes(g.B, HW, Co));
            NEED(scr);
            float* dres = nullptr; int dacc = 0;
            if (residual && residual->need_grad) { dres = residual->g; dacc = residual->gw ? 1 : 0; mark_written(residual); }
            NormST bst;
            bst.x = co->dt; bst.y = out->dt; bst.dy = out->gdt; bst.dx = co->gdt; bst.dres = residual ? residual->gdt : 0;
            RUN(norm_bwd(ns.kind, act, g.B, HW, Co, co->d, out->d, out->g, ns.w, ns.w_stride, mean, rstd, co->g, ns.dw, ns.db, dres, dacc, scr, c.st, &bst, sbc, ss));
            c.top = mark;
            dyp = co->g; dy_st = co->gdt;
        } else if (s_bwd && out->gdt == 0) {
            // the consumers delivered an fp32 gradient, this layer's backward kernels read 16-bit: dy16 = act'(y) * dy, out of place
            RUN(cast_storage(out->g, 0, g16, dt, out->numel(), c.st));
            RUN(act_bwd_inplace(act, out->d, g16, out->numel(), c.st, out->dt, dt));
            dyp = g16; dy_st = dt;
        } else {
            RUN(act_bwd_inplace(act, co->d, out->g, out->numel(), c.st, co->dt, out->gdt));   // (co != out: the fp32 copy of the same values)
            dyp = out->g; dy_st = out->gdt;
        }
        if (train_w) {
            const size_t mark = c.top;
            void* wscr = nullptr;
            const size_t wb = w16 ? conv_wgrad16_scratch_bytes(g) : conv_wgrad_scratch_bytes(g);
            hipStream_t wst = c.st;
            if (side) {
                CHK(c.side_fork());
                if (!c.dry) wst = c.st2;
                c.top2 = 0;                   // side-stream work is stream-ordered: its scratch stack restarts with every launch group
                if (wb) { wscr = c.alloc2(wb); if (!wscr) { set_error("workspace too small for the side-stream scratch"); return ACLGAN_ENOMEM; } }
                if (sbc) RUN(norm_bwd_ln_params(sbc, g.B, Co, ns.dw, ns.db, wst));
            } else if (wb) { wscr = c.alloc(wb); NEED(wscr); }
            if (w16) RUN(conv_wgrad16(g, dt, in->d, dyp, W.dw, W.db, wscr, wst, in->dt, dy_st));
            else {
                if (in->dt || dy_st) { set_error("conv_block: fp32 weight-gradient kernel on 16-bit operands"); return ACLGAN_EINVAL; }
                RUN(conv_wgrad(g, in->d, dyp, W.dw, W.db, wst, wscr, keepV));
            }
            c.top = mark;
        }
        if (gin->need_grad) {
            const size_t mark = c.top;
            if (s_bwd) {
                if (!dy_st) { set_error("conv_block: 16-bit-storage dgrad on an fp32 gradient"); return ACLGAN_EINVAL; }
                void* scr = c.alloc(conv_dgrad16s_scratch_bytes(g));
                NEED(scr);
                RUN(conv_dgrad16s(g, dt, dyp, W.w16t, gin->g, gin->gdt, gin->gw ? 1 : 0, scr, c.st));
            } else {
                if (dy_st || gin->gdt) { set_error("conv_block: fp32-output dgrad kernel on 16-bit gradients"); return ACLGAN_EINVAL; }
                void* scr = c.alloc(d16 ? conv_dgrad16_scratch_bytes(g) + 256 : conv_dgrad_scratch_bytes(g));
                NEED(scr);
                if (d16) RUN(conv_dgrad16(g, dt, dyp, W.w, W.w16t, gin->g, gin->gw ? 1 : 0, scr, c.st));
                else RUN(conv_dgrad(g, dyp, W.w, gin->g, scr, gin->gw ? 1 : 0, c.st));
            }
            mark_written(gin);
            c.top = mark;
        }
        c.top = mark0;
        return ACLGAN_OK;
    }, {{train_w ? W.dw : nullptr, W.nw}, {train_w ? W.db : nullptr, W.nb}, {ln_train ? ns.dw : nullptr, Co}, {ln_train ? ns.db : nullptr, Co}});
    return ACLGAN_OK;
}

// Batched Winograd filter transforms (round 5).  The 2 * n_res ResBlock filters of an encoder / a decoder have one shape and sit at a
// constant distance in the flat parameter buffer (weight + bias, parameters() order): their transforms U = G g G^T for the whole update --
// forward and, when the generators are trained, input gradient -- are ONE launch per (network, encoder | decoder, direction) at the start
// of the update instead of one per filter at its first use (96 launches of 6 - 16 us per step at 256 x 256 B = 8).  They are written on lane 0
// before any other lane starts.  Layout and cache key are exactly what the layers will ask for (conv_wino_u_variant); a layer that asks for
// something else finds no entry and transforms its own filter as before.
static int prefill_wino_u(aclgan_ctx& c, int net, int B, int H, int W, bool train) {
    if (sw(SW_NOUCACHE) || !sw(SW_U_BATCH)) return ACLGAN_OK;
    const aclgan_arch& a = c.arch;
    const int nd = a.gen_n_downsample, count = 2 * a.gen_n_res, C = a.gen_dim << nd;
    if (count < 2) return ACLGAN_OK;
    aclgan_conv_desc d;
    d.B = B; d.Hi = H >> nd; d.Wi = W >> nd; d.Ci = C; d.Co = C; d.k = 3; d.stride = 1; d.pad = 1; d.upsample = 0; d.act = ACLGAN_ACT_NONE;
    ConvGeom g;
    if (make_geom(&d, &g)) return ACLGAN_OK;
    const size_t ubytes = conv_wino_u_bytes(g);
    if (!ubytes) return ACLGAN_OK;
    if (c.dtype != ACLGAN_DTYPE_FP32 && c.w16[0] && conv16_eligible(g, 0)) return ACLGAN_OK;      // these layers run on the 16-bit kernels
    char buf[160];
    for (int part = 0; part < 2; ++part) {
        std::vector<const float*> ws;
        for (int r = 0; r < a.gen_n_res; ++r)
            for (int j = 0; j < 2; ++j) {
                if (part == 0) snprintf(buf, sizeof buf, "enc_content.model.%d.model.%d.model.%d.conv.weight", 1 + nd, r, j);
                else snprintf(buf, sizeof buf, "dec.model.0.model.%d.model.%d.conv.weight", r, j);
                ws.push_back(c.param(0, net, buf));
            }
        if (!ws[0]) continue;
        const int64_t wstride = ws[1] - ws[0];
        bool even = wstride > 0;
        for (int i = 1; i < count && even; ++i) even = ws[i] && ws[i] - ws[i - 1] == wstride;
        if (!even) continue;
        for (int dgrad = 0; dgrad <= (train ? 1 : 0); ++dgrad) {
            // (the forward keeps its input transform for the weight gradient only where neither runs fused: conv_block's rule)
            const bool keepV = train && !dgrad && conv_fwd_keep_bytes(g) > 0;
            const int uv = conv_wino_u_variant(g, dgrad, keepV);
            if (uv < 0 || c.ucache.count(std::make_pair(ws[0], uv & 15))) continue;
            float* u0 = nullptr;
            bool contiguous = true;
            const size_t ustride = (ubytes + 255) & ~(size_t)255;
            for (int i = 0; i < count; ++i) {
                float* u = (float*)c.alloc(ubytes);
                NEED(u);
                if (i == 0) u0 = u;
                else if ((char*)u != (char*)u0 + (size_t)i * ustride) contiguous = false;
                c.ucache[std::make_pair(ws[i], uv & 15)] = aclgan_ctx::UEnt{u, contiguous, uv >> 4, c.cur_lane, c.nck(c.cur_lane)};
            }
            if (!contiguous) {          // (cannot happen with the stack allocator; if it ever does, the layers fill their entries themselves)
                for (int i = 0; i < count; ++i) c.ucache[std::make_pair(ws[i], uv & 15)].filled = false;
                continue;
            }
            RUN(conv_wino_prefill(g, uv, ws[0], wstride, u0, (int64_t)(ustride / sizeof(float)), count, c.st));
        }
    }
    return ACLGAN_OK;
}

// Round 6: the batched transforms of an update (8 launches of ~60 us in gen_update, 4 in dis_update: 19 MB of output each) used to sit in the
// preamble on lane 0, in front of the chain everything else waits for, although the first layer that reads one is the fourth of the first
// encoder pass.  They now run on the last lane beside the first three encoder layers; the cache entries carry that lane's stamp, so a reader
// on another lane waits for exactly the launch that fills its entry (ucache_lookup).  The lane first waits for lane 0's checkpoint: the
// previous call's optimizer step wrote the parameters on the caller's stream.
int prefill_on_side_lane(aclgan_ctx& c, int B, int H, int W, bool train) {
    const int AB = ACLGAN_NET_GEN_AB, BA = ACLGAN_NET_GEN_BA;
    if (c.nlanes <= 1) { CHK(prefill_wino_u(c, AB, B, H, W, train)); return prefill_wino_u(c, BA, B, H, W, train); }
    const int LP = c.nlanes - 1;
    CHK(c.mark());
    const int k0 = c.nck(0) - 1;
    CHK(c.set_lane(LP));
    CHK(c.wait_ck(LP, 0, k0));
    CHK(prefill_wino_u(c, AB, B, H, W, train)); CHK(prefill_wino_u(c, BA, B, H, W, train));
    CHK(c.mark());
    return c.set_lane(0);
}

// ContentEncoder.forward (networks.py:230-245)
int content_encode(aclgan_ctx& c, int net, bool train, Act* x, Act** out) {
    PassScope pass(c, net, c.carry_mode == ACLGAN_CARRY_ADOPT ? "encode(adopted)" : "encode");      // (adopted: a range without kernels)
    const aclgan_arch& a = c.arch;
    char buf[160];
    NormSpec in_; in_.kind = ACLGAN_NORM_IN;
    Act* h = nullptr;
    int d = a.gen_dim;
    CHK(conv_block(c, c.pw(0, net, "enc_content.model.0.conv"), train, x, d, 7, 1, 3, 0, ACLGAN_ACT_RELU, in_, nullptr, &h));
    for (int i = 0; i < a.gen_n_downsample; ++i) {
        snprintf(buf, sizeof buf, "enc_content.model.%d.conv", 1 + i);
        CHK(conv_block(c, c.pw(0, net, buf), train, h, 2 * d, 4, 2, 1, 0, ACLGAN_ACT_RELU, in_, nullptr, &h));
        d *= 2;
    }
    for (int r = 0; r < a.gen_n_res; ++r) {
        Act *t = nullptr, *o = nullptr;
        snprintf(buf, sizeof buf, "enc_content.model.%d.model.%d.model.0.conv", 1 + a.gen_n_downsample, r);
        CHK(conv_block(c, c.pw(0, net, buf), train, h, d, 3, 1, 1, 0, ACLGAN_ACT_RELU, in_, nullptr, &t));
        snprintf(buf, sizeof buf, "enc_content.model.%d.model.%d.model.1.conv", 1 + a.gen_n_downsample, r);
        CHK(conv_block(c, c.pw(0, net, buf), train, t, d, 3, 1, 1, 0, ACLGAN_ACT_NONE, in_, h, &o));
        h = o;
    }
    *out = h;
    return ACLGAN_OK;
}

// dense layer with tape (launch = false: the caller runs the forward itself -- the fused MLP launch of decode() -- and this call only
// allocates the output, accounts for it and records the backward)
static int dense(aclgan_ctx& c, const PW& W, bool train_w, Act* in, int O, int act, Act** out_p, bool launch = true) {
    const int B = in->B, I = in->H * in->W * in->C;
    const bool want = train_w || in->need_grad;
    CHK(c.need(in));
    Act* out = c.new_act(B, 1, 1, O, want);
    NEED_ACT(out);
    if (!W.w) { set_error("dense: parameters not bound"); return ACLGAN_EINVAL; }
    if (launch) RUN(linear_fwd(B, I, O, in->d, W.w, W.b, act, out->d, c.st));
    c.count(4.0 * ((double)B * I + (double)O * I + O + (double)B * O) * (want ? 3.0 : 1.0));    // (+ backward: the same operands again, twice)
    c.wrote(out);
    *out_p = out;
    if (!want) return ACLGAN_OK;
    c.push([=](aclgan_ctx& c) -> int {
        if (!out->gw) return ACLGAN_OK;
        CHK(c.acq(out));
        if (in->need_grad) CHK(c.acq(in));
        float* dx = nullptr;
        float* tmp = nullptr;
        const size_t mark = c.top;
        if (in->need_grad) {
            if (in->gw) { tmp = c.allocf((int64_t)B * I); NEED(tmp); dx = tmp; } else dx = in->g;
        }
        // dy *= act'(y), dx on this closure's lane; dw / db (parameter gradients) on the side stream: x and dy stay put until the update ends
        const bool side = train_w && sw(SW_SIDE_STREAM);
        RUN(linear_bwd(B, I, O, in->d, out->d, out->g, W.w, act, dx, (train_w && !side) ? W.dw : nullptr, (train_w && !side) ? W.db : nullptr, c.st));
        if (side) {
            CHK(c.side_fork());
            RUN(linear_bwd_params(B, I, O, in->d, out->g, W.dw, W.db, c.st2));
        }
        if (in->need_grad) {
            if (tmp) {
                // in->g += tmp  (reuse the GAP backward kernel with HW = 1: dx[i] += dy[i])
                RUN(gap_bwd(B, 1, I, tmp, in->g, 1, c.st));
            }
            mark_written(in);
        }
        c.top = mark;
        return ACLGAN_OK;
    }, {{train_w ? W.dw : nullptr, W.nw}, {train_w ? W.db : nullptr, W.nb}});
    return ACLGAN_OK;
}

// StyleEncoder.forward (networks.py:212-228)
int style_encode(aclgan_ctx& c, int net, bool train, Act* x, Act** out) {
    PassScope pass(c, net, "style");
    const aclgan_arch& a = c.arch;
    char buf[160];
    NormSpec none;
    Act* h = nullptr;
    int d = a.gen_dim;
    CHK(conv_block(c, c.pw(0, net, "enc_style.model.0.conv"), train, x, d, 7, 1, 3, 0, ACLGAN_ACT_RELU, none, nullptr, &h));
    for (int i = 0; i < 2; ++i) {
        snprintf(buf, sizeof buf, "enc_style.model.%d.conv", 1 + i);
        CHK(conv_block(c, c.pw(0, net, buf), train, h, 2 * d, 4, 2, 1, 0, ACLGAN_ACT_RELU, none, nullptr, &h));
        d *= 2;
    }
    for (int i = 0; i < 2; ++i) {
        snprintf(buf, sizeof buf, "enc_style.model.%d.conv", 3 + i);
        CHK(conv_block(c, c.pw(0, net, buf), train, h, d, 4, 2, 1, 0, ACLGAN_ACT_RELU, none, nullptr, &h));
    }
    // AdaptiveAvgPool2d(1) (networks.py:222)
    const bool want = h->need_grad;
    Act* p = c.new_act(h->B, 1, 1, d, want);
    NEED_ACT(p);
    RUN(gap_fwd(h->B, h->H * h->W, d, h->d, p->d, c.st, h->dt));
    c.wrote(p);
    c.count((h->dt ? 2.0 : 4.0) * (double)h->numel() * (want ? 2.0 : 1.0));
    if (want) {
        Act* hh = h;
        c.push([=](aclgan_ctx& c) -> int {
            if (!p->gw) return ACLGAN_OK;
            CHK(c.acq(p)); CHK(c.acq(hh));
            RUN(gap_bwd(hh->B, hh->H * hh->W, hh->C, p->g, hh->g, hh->gw ? 1 : 0, c.st, hh->gdt));
            mark_written(hh);
            return ACLGAN_OK;
        });
    }
    // 1x1 conv dim -> style_dim (networks.py:223) == dense layer on [B][dim]
    CHK(dense(c, c.pw(0, net, "enc_style.model.6"), train, p, a.gen_style_dim, ACLGAN_ACT_NONE, out));
    return ACLGAN_OK;
}

// AdaINGen.decode (networks.py:147-163) + Decoder.forward (networks.py:247-264)
int decode(aclgan_ctx& c, int net, bool train, Act* content, Act* style, Act** out) {
    PassScope pass(c, net, "decode");
    const aclgan_arch& a = c.arch;
    char buf[160];
    const int C = content->C, nr = a.gen_n_res, nad = 2 * C * 2 * nr;
    // MLP (networks.py:280-292)
    Act *m0 = nullptr, *m1 = nullptr, *ap = nullptr;
    // (round 6) one launch for the three layers where the widths allow (dense.hip: mlp3_fwd -- the same bits as three linear_fwd launches);
    // activations, accounting and the three backward closures are those of dense()
    const int sdim = style->H * style->W * style->C;
    const bool fused = sw(SW_MLP_FUSED) && mlp3_fwd_ok(sdim, a.gen_mlp_dim);
    const PW W0 = c.pw(0, net, "mlp.model.0.fc"), W1 = c.pw(0, net, "mlp.model.1.fc"), W2 = c.pw(0, net, "mlp.model.2.fc");
    CHK(dense(c, W0, train, style, a.gen_mlp_dim, ACLGAN_ACT_RELU, &m0, !fused));
    CHK(dense(c, W1, train, m0, a.gen_mlp_dim, ACLGAN_ACT_RELU, &m1, !fused));
    CHK(dense(c, W2, train, m1, nad, ACLGAN_ACT_NONE, &ap, !fused));
    if (fused) RUN(mlp3_fwd(style->B, sdim, a.gen_mlp_dim, nad, style->d, W0.w, W0.b, W1.w, W1.b, W2.w, W2.b, m0->d, m1->d, ap->d, c.st));
    if (ap->need_grad) {   // AdaIN layers accumulate dw/db into disjoint column slices
        RUN(fill_zero(ap->g, ap->numel(), c.st));
        mark_written(ap);
    }
    Act* h = content;
    int j = 0;
    for (int r = 0; r < nr; ++r) {
        Act *t = nullptr, *o = nullptr;
        for (int half = 0; half < 2; ++half) {
            NormSpec ns; ns.kind = ACLGAN_NORM_ADAIN; ns.w_stride = nad;
            // assign_adain_params (networks.py:154-163): columns [2Cj, 2Cj+C) = bias, [2Cj+C, 2Cj+2C) = weight
            ns.b = ap->d + 2 * C * j; ns.w = ap->d + 2 * C * j + C;
            if (ap->need_grad) { ns.db = ap->g + 2 * C * j; ns.dw = ap->g + 2 * C * j + C; }
            ++j;
            snprintf(buf, sizeof buf, "dec.model.0.model.%d.model.%d.conv", r, half);
            if (half == 0) CHK(conv_block(c, c.pw(0, net, buf), train, h, C, 3, 1, 1, 0, ACLGAN_ACT_RELU, ns, nullptr, &t));
            else CHK(conv_block(c, c.pw(0, net, buf), train, t, C, 3, 1, 1, 0, ACLGAN_ACT_NONE, ns, h, &o));
        }
        h = o;
    }
    int d = C, idx = 2;
    for (int i = 0; i < a.gen_n_downsample; ++i) {
        NormSpec ns; ns.kind = ACLGAN_NORM_LN;
        snprintf(buf, sizeof buf, "dec.model.%d.norm.gamma", idx); ns.w = c.param(0, net, buf); ns.dw = train ? c.gradp(0, net, buf) : nullptr;
        snprintf(buf, sizeof buf, "dec.model.%d.norm.beta", idx); ns.b = c.param(0, net, buf); ns.db = train ? c.gradp(0, net, buf) : nullptr;
        snprintf(buf, sizeof buf, "dec.model.%d.conv", idx);
        // (the last of these feeds the fp32 7x7 image-side output layer: its output stays fp32)
        CHK(conv_block(c, c.pw(0, net, buf), train, h, d / 2, 5, 1, 2, 1, ACLGAN_ACT_RELU, ns, nullptr, &h, i + 1 < a.gen_n_downsample ? 1 : 0));
        d /= 2; idx += 2;
    }
    NormSpec none;
    snprintf(buf, sizeof buf, "dec.model.%d.conv", idx - 1);
    CHK(conv_block(c, c.pw(0, net, buf), train, h, a.gen_output_dim, 7, 1, 3, 0, ACLGAN_ACT_TANH, none, nullptr, out));
    return ACLGAN_OK;
}

// ---- spectral normalisation (dis.norm: sn; csrc/spectral.hip) ----
// One discriminator call = one power iteration of every SN layer of the network (reference SpectralNorm.forward -> _update_u_v,
// networks.py:547-559, before every forward, training or not).  The call's W_bar / sigma goes into a weight slot of its own (the
// convolution kernels read it unchanged; under a 16-bit compute dtype with its two 16-bit packs), the call's sigma is kept for the
// backward, and its convolution weight gradients are redirected into per-call scratch G that the fold closure -- pushed BEFORE the
// call's layers, so it runs after all of them -- turns into dL/dW_bar += G / sigma - (<G, W_bar> / sigma^2) u v^T.
// u and v in the fold are the network's STATE u / v when the backward runs, i.e. as the last call of the update left them, not the
// call's own: the reference replaces u / v through .data after autograd saved them for sigma = u . (W v) (networks.py:553-559), so its
// backward of every call reads the last call's vectors (oracle/aclgan_oracle.py: spectral_norm_weight).
struct SnCall {
    int n = 0;
    float *slot = nullptr, *G = nullptr, *sigma = nullptr;
    void* fscr = nullptr;
    unsigned short *s16 = nullptr, *s16t = nullptr;
    int64_t soff[SN_MAX_LAYERS] = {};
};

static int sn_begin_call(aclgan_ctx& c, int net, bool train, SnCall* sc) {
    const std::vector<aclgan_ctx::SnLayer>& Ls = c.sn_layers[net];
    const int n = (int)Ls.size();
    if (!c.dry && !c.sn.param) { set_error("spectral norm: aclgan_bind_sn_state was not called"); return ACLGAN_EINVAL; }
    int co[SN_MAX_LAYERS], kk[SN_MAX_LAYERS], taps[SN_MAX_LAYERS], ci[SN_MAX_LAYERS];
    int64_t tot = 0, tu = 0, tv = 0;
    sc->n = n;
    for (int l = 0; l < n; ++l) {
        co[l] = Ls[l].co; kk[l] = Ls[l].k; taps[l] = 16; ci[l] = Ls[l].k / 16;
        sc->soff[l] = tot;
        tot += (int64_t)co[l] * kk[l]; tu += co[l]; tv += kk[l];
    }
    const bool h16 = c.dtype != ACLGAN_DTYPE_FP32;
    sc->slot = c.allocf(tot); NEED(sc->slot);
    if (h16) {
        sc->s16 = (unsigned short*)c.alloc((size_t)tot * 2); NEED(sc->s16);
        sc->s16t = (unsigned short*)c.alloc((size_t)tot * 2); NEED(sc->s16t);
    }
    sc->sigma = c.allocf(n); NEED(sc->sigma);
    if (train) {
        sc->G = c.allocf(tot); NEED(sc->G);
        sc->fscr = c.alloc(sn_fold_scratch_bytes(n, co, kk)); NEED(sc->fscr);
    }
    const size_t mark = c.top;
    void* scr = c.alloc(sn_scratch_bytes(n, co, kk));
    NEED(scr);
    SnLayerPtrs P[SN_MAX_LAYERS];
    for (int l = 0; l < n; ++l) {
        float* st = c.sn.param;
        P[l] = SnLayerPtrs{c.param(1, net, Ls[l].key + "weight_bar"), st ? st + Ls[l].u_off : nullptr, st ? st + Ls[l].v_off : nullptr,
                           sc->slot + sc->soff[l], nullptr, nullptr, train ? sc->G + sc->soff[l] : nullptr, co[l], kk[l]};
    }
    RUN(sn_power_iteration(n, P, sc->sigma, scr, c.st));
    if (h16) {
        RUN(cast_flat16(sc->slot, sc->s16, tot, c.dtype, c.st));
        RUN(transpose_flat16(sc->slot, sc->s16t, sc->soff, co, taps, ci, n, c.dtype, c.st));
    }
    c.top = mark;
    // W read twice, the column partials written and read (1/8 of W), W / sigma written, G zeroed; the 16-bit packs read the slot twice
    c.count(4.0 * tot * (2.0 + 0.25 + 1.0 + (train ? 1.0 : 0.0)) + (h16 ? (8.0 + 4.0) * tot : 0.0) + 4.0 * 3.0 * (tu + tv));
    c.exec_flops += 4.0 * tot;       // (two matrix-vector products on the VALU: counted so that the step's FLOP total covers them)
    if (!train) return ACLGAN_OK;
    const float* lo = nullptr; const float* hi = nullptr;
    for (int l = 0; l < n; ++l) {
        const float* g = c.gradp(1, net, Ls[l].key + "weight_bar");
        if (!g) continue;
        if (!lo || g < lo) lo = g;
        if (!hi || g + (int64_t)co[l] * kk[l] > hi) hi = g + (int64_t)co[l] * kk[l];
    }
    const SnCall s = *sc;
    c.push([=](aclgan_ctx& c) -> int {
        hipStream_t fst = c.st;
        if (sw(SW_SIDE_STREAM)) {      // a parameter gradient: on the parameter-gradient stream, after this call's weight gradients
            CHK(c.side_fork());
            if (!c.dry) fst = c.st2;
        }
        SnFoldPtrs F[SN_MAX_LAYERS];
        const float* st = c.sn.param;
        for (int l = 0; l < s.n; ++l)
            F[l] = SnFoldPtrs{c.param(1, net, Ls[l].key + "weight_bar"), s.G + s.soff[l], st ? st + Ls[l].u_off : nullptr,
                              st ? st + Ls[l].v_off : nullptr, c.gradp(1, net, Ls[l].key + "weight_bar"), co[l], kk[l]};
        c.count(4.0 * tot * 5.0);      // G twice, W once, dL/dW_bar read and written
        c.exec_flops += 6.0 * tot;
        RUN(sn_fold(s.n, F, s.sigma, s.fscr, fst));
        return ACLGAN_OK;
    }, {{lo, (int64_t)(hi - lo)}});
    return ACLGAN_OK;
}

// the (weight, bias) pair of SN layer `l` of `net` for the current call: W_bar / sigma from the call's slot, the bias as it is; the
// weight gradient goes into the call's scratch G (the fold adds it into dL/dW_bar)
static PW sn_pw(aclgan_ctx& c, int net, const SnCall& sc, int l) {
    const aclgan_ctx::SnLayer& L = c.sn_layers[net][l];
    PW p;
    p.w = sc.slot + sc.soff[l];
    p.dw = sc.G ? sc.G + sc.soff[l] : nullptr;
    p.nw = (int64_t)L.co * L.k;
    p.b = c.param(1, net, L.key + "bias"); p.db = c.gradp(1, net, L.key + "bias"); p.nb = L.co;
    if (sc.s16) { p.w16 = sc.s16 + sc.soff[l]; p.w16t = sc.s16t + sc.soff[l]; }
    return p;
}

// MsImageDis.forward (networks.py:50-57)
// lane_a / lane_b (round 5): the full-resolution scale runs on lane_a, the pooling chain and the two coarser scales on lane_b -- their
// launches are a quarter / a sixteenth of the first scale's and fill a few CUs each (9 .. 64 workgroups); next to the first scale's
// full-chip kernels they cost next to nothing (profiles/r04_microbench_coresidency.txt).  lane_a == lane_b: one queue, as before.
int dis_forward(aclgan_ctx& c, int net, bool train, Act* x, std::vector<Act*>* outs, int lane_a, int lane_b) {
    PassScope pass(c, net, "forward");
    const aclgan_arch& a = c.arch;
    char buf[160];
    NormSpec none;
    Act* xin = x;
    if (lane_a < 0) lane_a = lane_b = c.cur_lane;
    // spectral norm: this call's power iteration and normalised weights first, on lane_a; a scale on another lane waits for it
    SnCall sc;
    const bool sn = !c.sn_layers[net].empty();
    int pi_lane = 0, pi_ck = 0;
    if (sn) {
        CHK(c.set_lane(lane_a));
        CHK(c.need(x));
        CHK(sn_begin_call(c, net, train, &sc));
        pi_lane = c.cur_lane; pi_ck = c.nck(pi_lane);
    }
    for (int s = 0; s < a.dis_num_scales; ++s) {
        CHK(c.set_lane(s == 0 ? lane_a : lane_b));
        if (sn) CHK(c.wait_ck(c.cur_lane, pi_lane, pi_ck));
        Act* h = xin;
        int d = a.dis_dim;
        for (int i = 0; i < a.dis_n_layer; ++i) {
            snprintf(buf, sizeof buf, "cnns.%d.%d.conv", s, i);
            const int co = i == 0 ? d : 2 * d;
            const PW p = (sn && i > 0) ? sn_pw(c, net, sc, s * (a.dis_n_layer - 1) + i - 1) : c.pw(1, net, buf);
            // (the last layer of a scale feeds the fp32 1x1 head: its output stays fp32)
            CHK(conv_block(c, p, train, h, co, 4, 2, 1, 0, ACLGAN_ACT_LRELU, none, nullptr, &h, i + 1 < a.dis_n_layer ? 1 : 0));
            if (i > 0) d *= 2;
        }
        snprintf(buf, sizeof buf, "cnns.%d.%d", s, a.dis_n_layer);
        Act* o = nullptr;
        CHK(conv_block(c, c.pw(1, net, buf), train, h, 1, 1, 1, 0, 0, ACLGAN_ACT_NONE, none, nullptr, &o));
        outs->push_back(o);
        if (s + 1 < a.dis_num_scales) {
            // self.downsample (networks.py:33,53)
            CHK(c.set_lane(lane_b));
            Act* src = xin;
            CHK(c.need(src));
            Act* p = c.new_act(src->B, (src->H - 1) / 2 + 1, (src->W - 1) / 2 + 1, src->C, src->need_grad);
            NEED_ACT(p);
            RUN(avgpool3s2_fwd(src->B, src->H, src->W, src->C, src->d, p->d, c.st));
            c.wrote(p);
            c.count(4.0 * ((double)src->numel() + (double)p->numel()) * (src->need_grad ? 2.0 : 1.0));
            if (src->need_grad) {
                c.push([=](aclgan_ctx& c) -> int {
                    if (!p->gw) return ACLGAN_OK;
                    CHK(c.acq(p)); CHK(c.acq(src));
                    RUN(avgpool3s2_bwd(src->B, src->H, src->W, src->C, p->g, src->g, src->gw ? 1 : 0, c.st));
                    mark_written(src);
                    return ACLGAN_OK;
                });
            }
            xin = p;
        }
    }
    return ACLGAN_OK;
}

// DiffAugment of a discriminator input (augment.hip) on the current lane: y = T(x) by the parameter rows [row0, row0 + x->B); the gradient
// of y goes back into x's gradient buffer (overwrite or accumulate, as every other consumer of x does)
static int augment(aclgan_ctx& c, int net, Act* x, int row0, Act** out) {
    PassScope pass(c, net, "augment");
    CHK(c.need(x));
    if (x->dt != 0) { set_error("augment: the discriminator inputs are fp32 tensors"); return ACLGAN_EINVAL; }
    Act* y = c.new_act(x->B, x->H, x->W, x->C, x->need_grad);
    NEED_ACT(y);
    const int policy = c.aug_policy;
    const size_t sb = (policy & ACLGAN_AUG_COLOR) ? diffaugment_scratch_bytes(x->B, x->H, x->W, x->C) : 0;
    const float* rows = c.aug_params ? c.aug_params + (size_t)row0 * 8 : nullptr;      // (dry runs have none)
    {
        const size_t mark = c.top;
        void* scr = nullptr;
        if (sb) { scr = c.alloc(sb); NEED(scr); }
        RUN(diffaugment_fwd(x->B, x->H, x->W, x->C, policy, x->d, rows, y->d, scr, c.st));
        c.top = mark;
    }
    c.wrote(y);
    c.count(4.0 * 2.0 * (double)x->numel() * (x->need_grad ? 2.0 : 1.0));
    *out = y;
    if (!x->need_grad) return ACLGAN_OK;
    c.push([=](aclgan_ctx& c) -> int {
        if (!y->gw) return ACLGAN_OK;
        CHK(c.acq(y)); CHK(c.acq(x));
        if (y->gdt != 0 || x->gdt != 0) { set_error("augment: the gradients of the discriminator inputs are fp32 tensors"); return ACLGAN_EINVAL; }
        const size_t mark = c.top;
        void* scr = nullptr;
        if (sb) { scr = c.alloc(sb); NEED(scr); }
        RUN(diffaugment_bwd(x->B, x->H, x->W, x->C, policy, y->g, rows, x->g, x->gw ? 1 : 0, scr, c.st));
        mark_written(x);
        c.top = mark;
        return ACLGAN_OK;
    });
    return ACLGAN_OK;
}

// discriminator pass + LSGAN terms over a JOINT batch: passes that share discriminator weights (e.g.
// dis_A on x_A_fake and on x_A2_fake, trainer.py:136-137) run as one pass over the concatenated batch --
// same arithmetic per sample, half the launches and twice the rows for the small late layers.  Segment i
// covers `nb` consecutive samples with its own target / reported weight / gradient scale / loss slot.
// The loss gradient w.r.t. each scale's map is written at forward time: total = sum_i gscale_i * loss_i is
// linear in the reported losses.  Round 5: ONE launch for all scales and segments of the call (networks.py:64-67,81-83,96-98
// loop over the scales in Python), the terms added to their slots in the order of the former per-term launches.
// row0: the first row of the augmentation parameters that belongs to x (aclgan_ctx_set_augment; ignored while the policy is 0)
int dis_lsgan(aclgan_ctx& c, int net, bool train, Act* x, int nb, int row0, const std::vector<LsSeg>& segs, int lane_a, int lane_b) {
    std::vector<Act*> outs;
    if (c.aug_policy) {
        if (lane_a >= 0) CHK(c.set_lane(lane_a));
        CHK(augment(c, net, x, row0, &x));
        CHK(c.mark());
    }
    CHK(dis_forward(c, net, train, x, &outs, lane_a, lane_b));
    std::vector<LsganTerm> terms;
    for (Act* o : outs) {
        CHK(c.need(o));
        const int n = nb * o->H * o->W * o->C;
        for (size_t i = 0; i < segs.size(); ++i) {
            LsganTerm t;
            t.o = o->d + (size_t)i * n; t.d_o = o->need_grad ? o->g + (size_t)i * n : nullptr; t.slot = segs[i].slot;
            t.n = n; t.target = segs[i].target; t.weight = segs[i].weight; t.gscale = segs[i].gscale;
            terms.push_back(t);
        }
        if (o->need_grad) mark_written(o);
    }
    if (train && c.in_dis_update && c.lecam_state) {      // (a train pass of dis_update: the only place a fold follows)
        const int S = c.arch.dis_num_scales, D = net - ACLGAN_NET_DIS_A;
        float* st = c.lecam_state;
        std::vector<LecamTerm> lt(terms.size());
        for (size_t j = 0; j < terms.size(); ++j) {
            const int s = (int)(j / segs.size()), k = terms[j].target == 1.f ? 1 : 0;      // class = target: 1 the real side, 0 the fake side
            lt[j].ls = terms[j];
            lt[j].anchor = st + (D * S + s) * 2 + (1 - k);
            lt[j].lecam = st + 18 * S + D;
            lt[j].stats = st + 6 * S + ((D * S + s) * 2 + k) * 2;
        }
        RUN(lsgan_lecam_batch(lt.data(), (int)lt.size(), c.lecam_lambda, c.lecam_start, reinterpret_cast<const int*>(st + 18 * S + 3), c.st, c.lscale));
    } else RUN(lsgan_loss_batch(terms.data(), (int)terms.size(), c.st, c.lscale));
    if (train && c.in_dis_update && c.ada_state && net != ACLGAN_NET_DIS_2) {
        // overfitting signal (ada.hip): the real-side terms (target 1: x_a, x_b) of this pass, one launch behind the loss kernel on its lane.
        // dis_2 has no real side: both of its inputs are generated.  A pass without such a term (the fake-side calls under spectral norm) launches nothing.
        std::vector<AdaSignTerm> at;
        double bytes = 0.0;
        for (const LsganTerm& t : terms)
            if (t.target == 1.f) { at.push_back(AdaSignTerm{t.o, t.n, t.weight}); bytes += 4.0 * (double)t.n; }
        if (!at.empty()) {
            c.count(bytes + 2.0 * 4.0 * 2.0);
            RUN(ada_sign(at.data(), (int)at.size(), c.ada_state + 8 + 2 * (net - ACLGAN_NET_DIS_A), c.st));
        }
    }
    return ACLGAN_OK;
}

// focus_translation (trainer.py:85-88) with optional 6-channel pair (trainer.py:132-133)
// out_dst / pair_dst: optional pre-made destinations (batch-slice views of joint discriminator inputs)
int blend(aclgan_ctx& c, Act* dec4, Act* bg, Act* pair_first, Act** out_p, Act** pair_p, Act* out_dst, Act* pair_dst) {
    const bool want = dec4->need_grad;
    CHK(c.need(dec4)); CHK(c.need(bg)); CHK(c.need(pair_first));
    Act* out = out_dst;
    if (!out) {
        out = c.new_act(dec4->B, dec4->H, dec4->W, 3, want);
        NEED_ACT(out);
    }
    Act* pair = nullptr;
    if (pair_first) {
        pair = pair_dst;
        if (!pair) {
            pair = c.new_act(dec4->B, dec4->H, dec4->W, 6, want);
            NEED_ACT(pair);
        }
    }
    const bool plain = dec4->C == 3;      // non-focus configuration (trainer.py:117-121,129-130): the decoder output is the image itself
    if (plain) RUN(plain_pair_fwd(dec4->B, dec4->H * dec4->W, dec4->d, out->d, pair_first ? pair_first->d : nullptr, pair ? pair->d : nullptr, c.st));
    else RUN(focus_blend_fwd(dec4->B, dec4->H * dec4->W, dec4->d, bg->d, out->d, pair_first ? pair_first->d : nullptr, pair ? pair->d : nullptr, c.st));
    c.count(4.0 * (double)dec4->B * dec4->H * dec4->W * ((plain ? 3 : 4 + 3) + 3 + (pair_first ? 9 : 0)) * (want ? 2.0 : 1.0));
    c.wrote(out); c.wrote(pair);
    *out_p = out;
    if (pair_p) *pair_p = pair;
    if (!want) return ACLGAN_OK;
    c.push([=](aclgan_ctx& c) -> int {
        const float* dout = out->written() ? out->g : nullptr;
        const float* dpair = (pair && pair->written()) ? pair->g : nullptr;
        if (!dout && !dpair) return ACLGAN_OK;
        if (dout) CHK(c.acq(out));
        if (dpair) CHK(c.acq(pair));
        CHK(c.acq(dec4));
        if (!plain && bg->need_grad) CHK(c.acq(bg));
        if (plain) { RUN(plain_pair_bwd(dec4->B, dec4->H * dec4->W, dout, dpair, dec4->g, c.st)); return ACLGAN_OK; }
        float* dbg = bg->need_grad ? bg->g : nullptr;
        RUN(focus_blend_bwd(dec4->B, dec4->H * dec4->W, dec4->d, bg->d, dout, dpair, dec4->g, dbg, bg->gw ? 1 : 0, c.st));
        if (dbg) mark_written(bg);
        return ACLGAN_OK;
    });
    return ACLGAN_OK;
}

int zero_grad_of(aclgan_ctx& c, Act* a) {
    if (a->need_grad) { RUN(fill_zero(a->g, a->numel(), c.st)); mark_written(a); }
    return ACLGAN_OK;
}

__global__ void scale_kernel(const float* s, float* d, float a, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = a * s[i];
}

// Refresh the 16-bit weight packs from the fp32 master parameters (both groups: each update runs the other group's
// networks forward / dgrad-only).  ~55 M elements read once, 2 x 2 bytes written: ~0.1 ms against a step of tens of ms,
// and it makes the packs immune to whatever touched the flat buffers between calls (Adam, load_state_dict, broadcast) and to the
// forward-weights switch: a forward-only call that reads the averaged generator packs from the average (aclgan_ctx::weights).
int pack_params(aclgan_ctx& c) {
    if (c.dtype == ACLGAN_DTYPE_FP32 || c.dry) return ACLGAN_OK;
    for (int g = 0; g < 2; ++g) {
        if (!c.w16[g] || !c.w16t[g]) { set_error("compute dtype is 16-bit but aclgan_bind_params16 was not called for group %d", g); return ACLGAN_EINVAL; }
        CHK(cast_flat16(c.weights(g), c.w16[g], c.groups[g].numel, c.dtype, c.st));
        CHK(transpose_flat16(c.weights(g), c.w16t[g], c.cv_off[g].data(), c.cv_co[g].data(), c.cv_taps[g].data(), c.cv_ci[g].data(),
                             (int)c.cv_off[g].size(), c.dtype, c.st));
    }
    return ACLGAN_OK;
}

int input_act(aclgan_ctx& c, const float* nchw, int B, int C, int H, int W, Act** out) {
    Act* a = c.new_act(B, H, W, C, false);
    NEED_ACT(a);
    RUN(nchw_to_nhwc(nchw, a->d, B, C, H, W, c.st));
    *out = a;
    return ACLGAN_OK;
}

int wrap_vec(aclgan_ctx& c, const float* dev, int B, int n, float scale, Act** out) {
    Act* a = c.new_act(B, 1, 1, n, false);
    NEED_ACT(a);
    if (!c.dry) {
        hipLaunchKernelGGL(scale_kernel, dim3(cdiv(B * n, 256)), dim3(256), 0, c.st, dev, a->d, scale, B * n);
        ACL_CHECK_LAUNCH("scale_kernel");
    }
    *out = a;
    return ACLGAN_OK;
}

}  // namespace aclgan
