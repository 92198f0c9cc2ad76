// The dispatch of a batched call: which kernel family, variant and launch shape serves (mode, batch).
// Host-only and free of HIP calls, so that it is testable without a device (smol_csum_tool_pick);
// every fact about a variant number comes from the registry (variants.def through csum_variants.h),
// and the only numbers named here are the defaults below, each with the measurement that chose it.
#pragma once

#include "csum_launch.h"
#include "csum_variants.h"

namespace smolcsum {

// The kernel a batched call runs: its family, variant and (walk / tile / copy kernels) launch shape.
// One pure function, so that smol_csum_tool_kernel_for names exactly what run_one() (csum_api.cpp) launches.
struct Pick {
    int family;
    int variant;
    int shape;
};
// What a context contributes to the choice.
struct PickCtx {
    int variant;      // -1 automatic, else forced (smol_csum_tool_set_variant)
    int shape;        // -1 automatic, else CFG_*
    int desc_staged;  // descriptor-batch emit: 1 the staged form, 0 in place (see smol_csum_ctx)
};

// ---- the defaults ----------------------------------------------------------------------------------
// Kernel variant when none is forced (tools/sweep.py on MI355X, C2 / C3 / C4): the 128-byte line
// grid with non-temporal loads (verify: C2 0.2415 -> 0.2327 ms, C4 0.2158 -> 0.2083 ms, C3 0.826 ->
// 0.815 ms; fixed-stride emit with shared boundary lines, csum_walk.h shared_from: C2 0.3155 ->
// 0.304 ms, C4 0.2727 -> 0.263 ms).
constexpr int kWalkVerify = 5;  // verify and data, any batch form the other kernels do not serve
// fixed-stride emit: variant 5 with the fields' 64-B segments written whole where no neighbour's
// field shares them (C2 emit 0.305 -> 0.294 ms, tools/exp_emit_seg.py), skipped on wavefronts
// without an IPv4 record (variant 29: C2 0.2891-0.2894 vs 19's 0.2907-0.2913 ms, C4 0.2649-0.2658
// vs 0.2654-0.2666 ms, interleaved on one box, profiles/r04_experiments/).  Round 5: variant 39
// = 29, and on a wavefront without an IPv4 record whole segments for IPv6 records too, decided
// by one ballot (bench lines over rotating batches, interleaved on one box,
// profiles/r05_experiments/emit_variants_bench.txt: C4 5151-5157 -> 5237-5253 GiB/s, C2 equal)
constexpr int kWalkEmitFixed = 39;
// the walk kernel's own emit over descriptors, for the entry points the tile kernel does not serve
// (NHC): cached loads on the 16-byte grid (C3 0.9705 ms vs 0.9722 ms)
constexpr int kWalkEmitDesc = 1;
// Verify over descriptor batches (C3) runs the line grid without the register prefetch at 16 x 4:
// with the record geometry in LDS that kernel holds 63 VGPRs (8 waves/SIMD), and the waves hide the
// latency the prefetch hid before: C3 verify 0.7998 ms (variant 5, 16 x 3) -> 0.7425 ms
// (tools/gpu_ab.sh, MI355X).  Fixed-stride verify keeps the prefetch (C2 8 x 7: 0.2378 vs 0.2519 ms
// without).
constexpr int kWalkVerifyDesc = 13;
// emit over descriptor batches where the descriptor walk does not serve: the tile kernel on the line
// grid (C3 0.9285 ms vs the walk kernel's best 0.9945 ms at the same shape; its verify is slower,
// 1.08 ms vs 0.83 ms)
constexpr int kTileEmitDesc = 7;
// Round 5: verify over descriptor batches runs dwalk_kernel's per-group walk (csum_dwalk.hip: 8
// records per wavefront, parse first, 8 lanes x 4 chunks per step on the line grid, 7 waves / SIMD):
// C3 0.793 -> 0.742 ms, 64-1500-B records 0.343 -> 0.185 ms with non-temporal header windows
// (variant 60, tools/exp_r05_desc.py, profiles/r05_experiments/dwalk_layouts.jsonl).  Variant 63
// loads the header windows with the default cache policy, so that the stream's second read of those
// lines and emit's field stores hit the L2: C3 bench (4 batch pairs in turn, one box, interleaved)
// verify 0.742 -> 0.731 ms and emit 0.942 (tile 7) -> 0.896 ms, 5269 -> 5457 GiB/s
// (profiles/r05_experiments/dwalk_cached_windows.txt); its emit beats the tile kernel on every
// descriptor layout measured, 64-1500-B records 0.223 -> 0.184 ms.
constexpr int kDwalkVerify = 63;
// Its emit form 41 sums the 16 window chunks from LDS and streams from chunk 16 (the window lines not
// read a second time): C3 emit 0.894 -> 0.881 ms, shuffled descriptors 0.922 -> 0.912, 64-1500-B
// records 0.186 -> 0.183; its verify measured 0.4 % slower, so verify stays on 63
// (profiles/r05_experiments/dwalk_cached_windows.txt).
constexpr int kDwalkEmit = 41;
// descriptor-batch emit while the records stage (round 6; see smol_csum_ctx in csum_ctx.h)
constexpr int kDwalkEmitStaged = 97;
// copy-emit: csum_copy.hip's variant 17 (body chunks = one source load + shift + sum + store) with the
// first body round's loads issued ahead of round 1's stores, at its default shape (16 x 4): C2copy
// 0.772-0.853 ms (variant 16) -> 0.692 ms (17) -> 0.678 ms (21; tools/exp_copy.py, MI355X)
constexpr int kCopy = 21;
// The transposed walk (csum_xwalk.hip) for fixed-stride records where it beats the walk kernel, from a
// measured table (round 6; VERDICT r05 item 7 replaced round 5's fitted length windows): one length
// sweep, tools/sweep_dispatch.py, over 1024 .. 9023 B in steps of 64 B (multiples of 64, + 28, and + 28
// with 64-B gaps), verify and emit (emit in bench.py's step order), on three boxes
// (profiles/r06_dispatch_sweep_box{1,2,3}.jsonl), turned into dispatch_table.inc by
// tools/gen_dispatch_table.py (the least summed time per entry).  Verify: the walk kernel, the
// transposed walk ('x') or the same with the first-load hint ('h': lanes 0-3 of each record's first
// instruction with the default cache policy; C2 verify 0.2342 -> 0.2259 ms); emit: the walk kernel, 'x',
// 'n' ('x' with non-temporal field segments) or 't' ('n' with the segments stored write-through), from a
// second emit sweep that ran all four (late round 6, profiles/r06_dispatch_sweep_wt_*.jsonl: two IPv4
// boxes, two IPv6-mix boxes; C2's and C4's rows take 't').  Outside 1024 .. 9023 B the walk kernel
// (round 5: past 9000 B the two trade places by length, within 2 %).
constexpr int kXwalk = 47;             // 'x'
constexpr int kXwalkVerifyHint = 89;   // 'h'
constexpr int kXwalkEmitNt = 57;       // 'n'
constexpr int kXwalkEmitWT = 101;      // 't'

// The walk kernel's own choice (the fallback of every other family).
inline int walk_variant(int mode, bool has_desc) {
    if (!has_desc) return mode == MODE_EMIT ? kWalkEmitFixed : kWalkVerify;
    return mode == MODE_EMIT ? kWalkEmitDesc : mode == MODE_VERIFY ? kWalkVerifyDesc : kWalkVerify;
}
inline int auto_variant(int mode, bool has_desc) {
    if (mode == MODE_EMIT && has_desc) return kDwalkEmit;
    if (mode == MODE_VERIFY && has_desc) return kDwalkVerify;
    return walk_variant(mode, has_desc);
}

#include "dispatch_table.inc"

// The transposed-walk variant the table gives a fixed-stride batch (0: the walk kernel).
inline int xwalk_auto(int mode, const smol_csum_batch_t* b) {
    if (b->desc || b->stride < b->len || (mode != MODE_VERIFY && mode != MODE_EMIT)) return 0;
    if (b->len < 1024 || b->len >= 1024 + 64 * 125) return 0;
    const uint32_t k = (b->len - 1024) / 64;
    const int col = b->stride != b->len ? 2 : (b->len % 64 == 0 ? 0 : 1);
    const char c = (mode == MODE_VERIFY ? kVerifyTable : kEmitTable)[k][col];
    if (mode == MODE_VERIFY) return c == 'h' ? kXwalkVerifyHint : c == 'x' ? kXwalk : 0;
    return c == 't' ? kXwalkEmitWT : c == 'n' ? kXwalkEmitNt : c == 'x' ? kXwalk : 0;
}

// The XCD block order (csum_launch.h xcd_block / xcd_chunk) when none is forced: the contiguous order
// for fixed-stride emit over at least 4 GiB.  Measured per 2^20 C2 records (tools/exp_inplace.py, one box,
// profiles/r04_experiments/xcd_remap.jsonl): emit 0.327 -> 0.298 ms at 2^22 records (6.3 GB),
// 0.332 -> 0.320 at 2^24, 0.338 -> 0.303 at 2^26, and C5's 2^27: 0.334 -> 0.300; at 2^20 records
// 0.297 -> 0.2995 (no gain).  Verify runs 4-6 % slower with it at every size, so it keeps the
// dispatch order.
// Verify over at least 64 GiB takes runs of 256 workgroups per XCD turn: C5's in-place verify 31.38-
// 31.46 -> 30.96-30.99 ms (profiles/r04_experiments/c5_verify_grain.jsonl); at 25 GB it was +1 %,
// at 100 GB -0.6 % (xcd_grain.jsonl), so smaller batches keep the dispatch order.
inline int xcd_remap_auto(int mode, const smol_csum_batch_t* b) {
    if (b->desc) return 0;
    const uint64_t bytes = b->n * b->stride;
    if (mode == MODE_EMIT) return bytes >= (4ull << 30) ? 1 : 0;
    if (mode == MODE_VERIFY) return bytes >= (64ull << 30) ? 256 : 0;
    return 0;
}

// The walk / tile kernels' launch shape for a variant of the registry.
inline int auto_shape(uint32_t len, bool has_desc, int variant) {
    if (has_desc) return variant_is(variant, V_G16U4) ? CFG_G16U4 : CFG_G16U3;
    const bool line = variant_is(variant, V_LINE);
    const uint64_t need = (uint64_t)len + (line ? 127 : 15);  // bytes of aligned chunks a record can touch
    // eight records per wavefront in two steps, with as few idle lanes as possible (C4's 1320-B
    // records on the line grid: 8 x 6 0.2083 ms, 8 x 7 0.2188 ms; C2's 1500 B: 8 x 7 0.2327 ms)
    if (need <= 16 * 8 * 6 * 2) return CFG_G8U6;
    if (line && need <= 16 * 8 * 7 * 2) return CFG_G8U7;
    if (need <= 16 * 16 * 6) return CFG_G16U6;
    if (need <= 16 * 32 * 4) return CFG_G32U4;
    return CFG_G64U4;
}

// ---- which batches a family serves (the experiments-only families: none in the product library) ----
// records per wavefront of the transposed walk for a record length (0: not served)
inline int xwalk_records(uint32_t len) {
    if (len < 1024) return 0;
    for (int R = 8; R >= 1; R /= 2)
        if (len <= 1024u * (16 / R) - 127u) return R;
    return 0;
}
inline bool xwalk_fits(const KParams& p) {
    // the buffer offsets of a wavefront's records stay below 2^31
    return p.desc == nullptr && p.stride >= p.len && p.stride <= (1ull << 26) && xwalk_records(p.len) > 0;
}
// The stripe kernel serves fixed-stride batches of packed records (stride == len) of 1024 .. 1520
// bytes over a natural grid (csum_tile.hip: 8 records per stripe, 12 KiB of LDS).
constexpr int kStripeRecords = 8;
inline bool stripe_fits(const KParams& p) {
#ifdef SMOL_EXP
    return p.desc == nullptr && p.len == p.stride && p.len >= 1024 && p.len <= (12 * 1024 - 127) / kStripeRecords;
#else
    (void)p;
    return false;
#endif
}
inline bool xcopy_fits(const KParams& p) {
#ifdef SMOL_EXP
    return p.desc == nullptr && p.stride >= p.len && p.len >= 1024 && p.len <= 1921 && p.stride <= (1ull << 26);
#else
    (void)p;
    return false;
#endif
}
// The descriptor walk: descriptor batches; the experiments build also runs it forced over fixed strides.
inline bool dwalk_fits(const KParams& p) {
#ifdef SMOL_EXP
    (void)p;
    return true;
#else
    return p.desc != nullptr;
#endif
}

// Whether the row's family serves this mode and batch (p.addrs set: a 6LoWPAN NHC batch).
inline bool family_serves(const Variant& r, int mode, const KParams& p) {
    const bool ip_gates = (mode == MODE_EMIT || mode == MODE_VERIFY) && !p.addrs;
    switch (r.family) {
        case F_STRIPE: return ip_gates && stripe_fits(p);
        case F_XWALK: return ip_gates && xwalk_fits(p);
        case F_DWALK: return ip_gates && dwalk_fits(p) && (mode == MODE_EMIT ? r.emit : r.verify);
        case F_TILE: return ip_gates;  // IP emit and verify only
        default: return true;
    }
}

// ---- emit_fields (smol_csum_batch_emit_fields) -----------------------------------------------------
// Its three forms live outside the registry (set_variant does not reach them).  Measured (tools/exp_fields.py,
// one box, the forms interleaved; profiles/fields_kernels.json):
//  - fixed strides: the transposed walk from 1280 B up to its last length (16257 B).  Per length, packed and
//    with 64-B gaps, transposed / walk: 1024-1216 B 1.01-1.07 (the walk kernel wins), 1320-1500 B 0.94-0.99,
//    1921-6000 B 0.47-0.87 (the walk kernel's 32 x 4 / 64 x 4 shapes idle half their lanes there), 9000 B
//    0.93-0.95, 1664 / 8065 / 12000 / 16000 B within 2 % either way.  Verify's table differs (C4's 1320 B: verify
//    takes the walk kernel, 0.209 against 0.226 ms; here the transposed form wins, 0.219 against 0.237 ms):
//    its finishing lanes write one 128-B line of entries per wavefront where verify writes 8 status bytes;
//  - descriptor batches: the descriptor walk (C3: 0.703 ms against the walk kernel's 0.932);
//  - everything else (records under 1280 B or past 16257 B, strides past 64 MiB): the walk kernel.
// `forced` (smol_csum_tool_set_fields_kernel): a form that does not serve the batch gives way to the walk
// kernel.
constexpr uint32_t kFieldsXwalkMinLen = 1280;
enum FieldsKernel { FK_AUTO = 0, FK_WALK = 1, FK_XWALK = 2, FK_DWALK = 3 };
inline int pick_fields(int forced, const smol_csum_batch_t* b, const KParams& p) {
    const bool x_ok = xwalk_fits(p), d_ok = p.desc != nullptr && dwalk_fits(p);
    if (forced == FK_XWALK) return x_ok ? FK_XWALK : FK_WALK;
    if (forced == FK_DWALK) return d_ok ? FK_DWALK : FK_WALK;
    if (forced == FK_WALK) return FK_WALK;
    if (x_ok && b->len >= kFieldsXwalkMinLen) return FK_XWALK;
    return d_ok ? FK_DWALK : FK_WALK;
}

// ---- verify_copy (smol_csum_batch_verify_copy) -----------------------------------------------------
// One kernel outside the registry (csum_vcopy.hip); its launch shape, on the 16-byte grid.  Measured
// (tools/exp_verify_copy.py, profiles/verify_copy_kernels.json): descriptor batches 8 x 7 (C3 2.25 ms
// against 8 x 6's 2.38 and 16 x 4's 2.47; 16 x 3 2.77 in an earlier call).
inline int vcopy_shape(uint32_t len, bool has_desc) {
    if (has_desc) return CFG_G8U7;
    return auto_shape(len, false, kWalkEmitDesc);
}

// ---- verify_echo_reply (smol_csum_batch_verify_echo_reply) -----------------------------------------
// One kernel outside the registry (csum_echo.hip), vcopy_kernel's form: it takes verify_copy's shapes (8 x 7
// over descriptors, auto_shape over fixed strides; tools/exp_echo_reply.py times the call as a whole).
inline int echo_shape(uint32_t len, bool has_desc) { return vcopy_shape(len, has_desc); }

// ---- verify_unreach_reply (smol_csum_batch_verify_unreach_reply) -----------------------------------
// One kernel outside the registry (csum_unreach.hip), echo_kernel's form: verify_copy's shapes again
// (tools/exp_unreach_reply.py times the call as a whole).
inline int unreach_shape(uint32_t len, bool has_desc) { return vcopy_shape(len, has_desc); }

inline Pick pick_kernel(const PickCtx& ctx, int mode, const smol_csum_batch_t* b, const KParams& p) {
    const bool has_desc = b->desc != nullptr;
    const bool nhc = p.addrs != nullptr;
    const Variant* forced = find_variant(ctx.variant);
    if (mode == MODE_COPY) {  // one fused pass: a forced copy-emit variant, else the default
        if (forced && forced->family == F_XCOPY && xcopy_fits(p)) return {F_XCOPY, forced->num, -1};
        if (forced && forced->is(V_WALK_COPY))
            return {F_WALK, forced->num, ctx.shape >= 0 ? ctx.shape : auto_shape(b->len, has_desc, forced->num)};
        return {F_COPY, forced && forced->family == F_COPY ? forced->num : kCopy, ctx.shape >= 0 ? ctx.shape : (int)CFG_G16U4};
    }
    // 1. the variant: forced (a copy-only one leaves this call to the automatic choice) or automatic
    int variant = forced && forced->is(V_COPY_ONLY) ? -1 : ctx.variant;
    if (variant < 0) {
        const int xv = nhc ? 0 : xwalk_auto(mode, b);
        variant = xv ? xv : auto_variant(mode, has_desc);
        if (variant == kDwalkEmit && ctx.desc_staged) variant = kDwalkEmitStaged;
    }
    // 2. its twins: the 2-B-field form under SMOL_BATCH_FIELD_STORES, the verify it shares
    if (mode == MODE_EMIT && (b->flags & SMOL_BATCH_FIELD_STORES)) variant = field_store_variant(variant);
    if (mode == MODE_VERIFY) variant = verify_variant(variant);
    // 3. a kernel that does not serve the mode or the batch falls back to the default of its kind
    //    (descriptor emit: the tile kernel; otherwise the walk kernel)
    const Variant* row = find_variant(variant);
    if (row && !family_serves(*row, mode, p)) {
        variant = (mode == MODE_EMIT && has_desc && !nhc) ? kTileEmitDesc : walk_variant(mode, has_desc);
        row = find_variant(variant);
    }
    const int family = row ? row->family : (int)F_WALK;
    // 4. the shape (walk and tile kernels)
    if (family != F_WALK && family != F_TILE) return {family, variant, -1};
    return {family, variant, ctx.shape >= 0 ? ctx.shape : auto_shape(b->len, has_desc, variant)};
}

}  // namespace smolcsum
