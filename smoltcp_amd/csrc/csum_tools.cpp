// C ABI of the tooling entry points (include/smolcsum_tools.h): synthetic batches and fault injection, the
// context's setters, the memory probes, and what the dispatch and the registry answer for a call.  Nothing
// here is needed to run a batched call (csum_api.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/smolcsum.h"
#include "../../include/smolcsum_tools.h"
#include "csum_ctx.h"

using namespace smolcsum;

namespace {

const char* family_kernel(int family) {
    switch (family) {
        case F_TILE: case F_STRIPE: return "csum_tile_kernel";
        case F_XWALK: return "xwalk_kernel";
        case F_DWALK: return "dwalk_kernel";
        case F_COPY: return "copy_kernel";
        case F_XCOPY: return "xcopy_kernel";
        default: return "csum_kernel";
    }
}

}  // namespace

extern "C" {

int smol_csum_tool_synth(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                         int profile, uint64_t seed, void* stream) {
    if (!ctx || profile < 0 || profile > SMOL_SYNTH_RANDOM) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    SynthParams p{d_buf, b->desc, b->n, b->stride, b->len, (uint32_t)profile, seed};
    return on_device(ctx, "synth kernel launch", [&] {
        return launch_synth(p, ctx->max_blocks, (hipStream_t)stream);
    });
}

int smol_csum_tool_corrupt(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* b,
                           uint32_t every, uint64_t seed, void* stream) {
    if (!ctx || every == 0) return SMOL_EINVAL;
    int rc = check_batch(b, d_buf);
    if (rc != SMOL_OK || b->n == 0) return rc;
    SynthParams p{d_buf, b->desc, b->n, b->stride, b->len, 0u, seed};
    return on_device(ctx, "corrupt kernel launch", [&] {
        return launch_corrupt(p, every, (hipStream_t)stream);
    });
}

int smol_csum_tool_set_shape(smol_csum_ctx_t* ctx, int shape) {
    if (!ctx || shape < -1 || shape >= CFG_COUNT) return SMOL_EINVAL;
    ctx->shape = shape;
    return SMOL_OK;
}

int smol_csum_tool_variant_built(int variant) { return variant_built(variant) ? 1 : 0; }

int smol_csum_tool_set_variant(smol_csum_ctx_t* ctx, int variant) {
    if (!ctx || !variant_built(variant)) return SMOL_EINVAL;
    ctx->variant = variant;
    return SMOL_OK;
}

int smol_csum_tool_set_tile(smol_csum_ctx_t* ctx, int records) {
    if (!ctx || (records != 32 && records != 64)) return SMOL_EINVAL;
    ctx->tile_records = records;
    return SMOL_OK;
}

int smol_csum_tool_set_max_blocks(smol_csum_ctx_t* ctx, uint32_t max_blocks) {
    if (!ctx) return SMOL_EINVAL;
    ctx->max_blocks = max_blocks ? max_blocks : kNaturalGrid;
    ctx->max_blocks_set = max_blocks != 0;
    return SMOL_OK;
}

int smol_csum_tool_set_xcd_remap(smol_csum_ctx_t* ctx, int on) {
    if (!ctx || on < -1) return SMOL_EINVAL;
    ctx->xcd_remap = on;
    return SMOL_OK;
}

int smol_csum_tool_set_launch_records(smol_csum_ctx_t* ctx, uint64_t records) {
    if (!ctx) return SMOL_EINVAL;
    ctx->launch_records = records;
    return SMOL_OK;
}

int smol_csum_tool_set_fields_kernel(smol_csum_ctx_t* ctx, int kernel) {
    if (!ctx || kernel < FK_AUTO || kernel > FK_DWALK) return SMOL_EINVAL;
    ctx->fields_kernel = kernel;
    return SMOL_OK;
}

int smol_csum_tool_set_emit_route(smol_csum_ctx_t* ctx, int route) {
    if (!ctx || route < -1 || route > 1) return SMOL_EINVAL;
    ctx->emit_route = route;
    return SMOL_OK;
}

int smol_csum_tool_last_route(const smol_csum_ctx_t* ctx) { return ctx ? (ctx->last_route ? 1 : 0) : SMOL_EINVAL; }

int smol_csum_tool_set_route_chunk(smol_csum_ctx_t* ctx, uint64_t records) {
    if (!ctx || records > kRouteChunk) return SMOL_EINVAL;
    ctx->route_chunk = records ? records : kRouteChunk;
    return SMOL_OK;
}

int smol_csum_tool_set_vcopy_stores(smol_csum_ctx_t* ctx, int nt) {
    if (!ctx || (nt != 0 && nt != 1)) return SMOL_EINVAL;
    ctx->vcopy_nt = nt == 1;
    return SMOL_OK;
}

int smol_csum_tool_stream_read(smol_csum_ctx_t* ctx, const uint8_t* d_buf, uint64_t bytes,
                               uint32_t* d_sink, void* stream) {
    if (!ctx || !d_buf || !d_sink || (bytes & 15u) || ((uintptr_t)d_buf & 15u)) return SMOL_EINVAL;
    return on_device(ctx, "stream-read kernel launch", [&] {
        return launch_stream_read(d_buf, bytes, d_sink, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_probe(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, uint64_t stride,
                               uint32_t f1, uint32_t f2, void* stream) {
    if (!ctx || !d_buf || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || stride == 0 || f1 == ~0u) return SMOL_EINVAL;
    return on_device(ctx, "field-probe kernel launch", [&] {
        return launch_field_probe(d_buf, bytes, stride, f1, f2, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_probe_list(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint64_t* d_addrs,
                                    const uint32_t* d_piece_first, int flags, void* stream) {
    if (!ctx || !d_buf || !d_addrs || !d_piece_first || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || (flags & ~1))
        return SMOL_EINVAL;
    return on_device(ctx, "field-probe kernel launch", [&] {
        return launch_field_probe_list(d_buf, bytes, d_addrs, d_piece_first, flags & 1, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_segment_probe(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint32_t* d_bitmap, int flags,
                                 void* stream) {
    if (!ctx || !d_buf || !d_bitmap || (bytes & 15u) || ((uintptr_t)d_buf & 15u) || ((uintptr_t)d_bitmap & 15u) ||
        (flags & ~1))
        return SMOL_EINVAL;
    return on_device(ctx, "segment-probe kernel launch", [&] {
        return launch_segment_probe(d_buf, bytes, d_bitmap, flags & 1, cu_count(ctx) * 8u, (hipStream_t)stream);
    });
}

int smol_csum_tool_field_scatter(smol_csum_ctx_t* ctx, uint8_t* d_buf, uint64_t bytes, const uint64_t* d_addrs,
                                 const uint16_t* d_vals, uint64_t n, int flags, void* stream) {
    if (!ctx || !d_buf || (n && (!d_addrs || !d_vals)) || (flags & ~15) || n > (0xFFFFFFull << 8)) return SMOL_EINVAL;
    return on_device(ctx, "field-scatter kernel launch", [&] {
        return launch_field_scatter(d_buf, bytes, d_addrs, d_vals, n, flags & 15, (hipStream_t)stream);
    });
}

int smol_csum_tool_auto_shape(uint32_t len, int has_desc) {
    // the walk kernel's verify shape (descriptor batches: kWalkVerifyDesc, which serves them when the
    // descriptor walk does not: NHC, data, forced variants)
    return auto_shape(len, has_desc != 0, walk_variant(MODE_VERIFY, has_desc != 0));
}

const char* smol_csum_tool_kernel_name(const smol_csum_ctx_t* ctx, int op, int has_desc) {
    // Without the batch this cannot see its record length: it answers for a batch that no
    // length-dependent kernel serves (descriptor batches exactly; fixed-stride batches the walk kernel's
    // lengths).  smol_csum_tool_kernel_for takes the batch.
    if (!ctx || op < MODE_DATA || op > MODE_COPY) return "";
    smol_csum_batch_t b;
    std::memset(&b, 0, sizeof b);
    b.n = 1;
    b.len = b.stride = 64;
    b.desc = has_desc ? reinterpret_cast<const smol_csum_desc_t*>(ctx->dummy) : nullptr;
    return smol_csum_tool_kernel_for(ctx, op, &b);
}

int smol_csum_tool_pick(int variant, int shape, int desc_staged, int op, const smol_csum_batch_t* b, int nhc, int out[3]) {
    if (!b || !out || op < MODE_DATA || op > MODE_COPY || !variant_built(variant) || shape < -1 || shape >= CFG_COUNT)
        return SMOL_EINVAL;
    KParams p;  // what the dispatch reads of the launch parameters: the batch form (nothing dereferenced)
    std::memset(&p, 0, sizeof p);
    p.desc = b->desc;
    p.n = b->n;
    p.stride = b->stride;
    p.len = b->len;
    p.addrs = nhc ? reinterpret_cast<const uint8_t*>(b) : nullptr;  // (only marks an NHC batch)
    const Pick k = pick_kernel(PickCtx{variant, shape, desc_staged}, op, b, p);
    out[0] = k.family;
    out[1] = k.variant;
    out[2] = k.shape;
    return SMOL_OK;
}

const char* smol_csum_tool_kernel_for(const smol_csum_ctx_t* ctx, int op, const smol_csum_batch_t* b) {
    int k[3];
    if (!ctx || smol_csum_tool_pick(ctx->variant, ctx->shape, ctx->desc_staged, op, b, 0, k) != SMOL_OK) return "";
    return family_kernel(k[0]);
}

int smol_csum_tool_variant_info(int variant, int out[4]) {
    const Variant* r = find_variant(variant);
    if (!r || !out) return SMOL_EINVAL;
    out[0] = r->family;
    out[1] = r->flags;
    out[2] = r->built() ? 1 : 0;
    out[3] = r->exp_only ? 1 : 0;
    return SMOL_OK;
}

int smol_csum_tool_form(int variant, int op, int out[13]) {
    if (!out || (op != MODE_EMIT && op != MODE_VERIFY)) return SMOL_EINVAL;
    const bool emit = op == MODE_EMIT;
    auto xw = [&](auto f) {
        const int v[13] = {F_XWALK, f.NOSTORE, f.SEG, f.PERSIST, f.NTS,   f.HALF,  f.STAGE,
                           f.HINT,  f.WPE,     f.WV,  f.STEPS,   f.ONLY_R, f.MAX_LEN == ~0u ? 0 : (int)f.MAX_LEN};
        std::memcpy(out, v, sizeof v);
    };
    if (emit ? with_xwalk_form<true>(variant, xw) : with_xwalk_form<false>(variant, xw)) return SMOL_OK;
    bool none = true;
    auto dw = [&](auto f) {
        const int v[13] = {F_DWALK, f.NOSTORE, f.GROUPS, f.SEGF, f.SEGPASS};
        std::memcpy(out, v, sizeof v);
        none = f.NONE;
    };
    const bool d = emit ? with_dwalk_form<true>(variant, dw) : with_dwalk_form<false>(variant, dw);
    return d && !none ? SMOL_OK : SMOL_EINVAL;
}

int smol_csum_tool_walk_launch(int variant, int op, int implicit, int nhc, int shape, int out[4]) {
    if (!out || op < MODE_DATA || op > MODE_COPY || shape < 0 || shape >= CFG_COUNT) return SMOL_EINVAL;
    if (nhc && op != MODE_EMIT && op != MODE_VERIFY) return SMOL_EINVAL;
    const int kern = nhc ? KERN_WALK_NHC : KERN_WALK;
    auto note = [&](auto, auto num, auto g, auto u) {
        const int v[4] = {kern, decltype(num)::value, decltype(g)::value, decltype(u)::value};
        std::memcpy(out, v, sizeof v);
    };
    auto batch_form = [&](auto mode, auto is_nhc) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool NHC = decltype(is_nhc)::value;
        return implicit ? with_walk_kernel<MODE, true, NHC>(variant, shape, note)
                        : with_walk_kernel<MODE, false, NHC>(variant, shape, note);
    };
    using std::integral_constant;
    bool ok = false;
    if (op == MODE_COPY && with_copy_kernel(variant, shape, [&](auto, auto num, auto g, auto u, auto, auto) {
            const int v[4] = {KERN_COPY, decltype(num)::value, decltype(g)::value, decltype(u)::value};
            std::memcpy(out, v, sizeof v);
        }))
        return SMOL_OK;  // a COPY row: copy_kernel's launcher, whatever the batch form
    if (nhc) {
        ok = op == MODE_EMIT ? batch_form(integral_constant<int, MODE_EMIT>{}, std::true_type{})
                             : batch_form(integral_constant<int, MODE_VERIFY>{}, std::true_type{});
    } else {
        switch (op) {
            case MODE_DATA: ok = batch_form(integral_constant<int, MODE_DATA>{}, std::false_type{}); break;
            case MODE_EMIT: ok = batch_form(integral_constant<int, MODE_EMIT>{}, std::false_type{}); break;
            case MODE_VERIFY: ok = batch_form(integral_constant<int, MODE_VERIFY>{}, std::false_type{}); break;
            default: ok = batch_form(integral_constant<int, MODE_COPY>{}, std::false_type{}); break;
        }
    }
    return ok ? SMOL_OK : SMOL_EINVAL;
}

uint32_t smol_csum_tool_last_launch(void) { return g_last_launch.load(std::memory_order_relaxed); }

}  // extern "C"
