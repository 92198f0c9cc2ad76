// Host <-> kernel interface of the checksum engine (internal; the public ABI is
// include/smolcsum.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/smolcsum.h"
#include "csum_variants.h"

namespace smolcsum {

enum { MODE_DATA = 0, MODE_EMIT = 1, MODE_VERIFY = 2, MODE_COPY = 3 };  // COPY: fused copy + emit
static_assert(MODE_DATA == kOpData && MODE_EMIT == kOpEmit && MODE_VERIFY == kOpVerify && MODE_COPY == kOpCopy, "csum_variants.h");

// Internal record kind of the 6LoWPAN NHC UDP entry points (never in a descriptor).
constexpr uint32_t KIND_NHC_UDP = 0x10;
// Internal kind bit: SMOL_REC_IPHDR_ONLY (a raw socket's frame: the IP header's gate only).
constexpr uint32_t KIND_IPHDR_ONLY = 0x200;
// The kernels' view of a descriptor's kind byte + flags byte (the desc dword at offset 12).
__host__ __device__ __forceinline__ uint32_t desc_kind(uint32_t w) {
    return (w & 0xffu) | (((w >> 8) & SMOL_REC_IPHDR_ONLY) ? KIND_IPHDR_ONLY : 0u);
}

// Launch shapes: lanes per record (G) x 16-byte chunks per lane per step (U).
enum {
    CFG_G8U6 = 0,
    CFG_G16U3 = 1,
    CFG_G16U6 = 2,
    CFG_G32U3 = 3,
    CFG_G32U4 = 4,
    CFG_G64U2 = 5,
    CFG_G64U4 = 6,
    CFG_G8U7 = 7,
    CFG_G16U4 = 8,
    CFG_COUNT = 9
};

// The walk kernel's shape sets (csum_variants.h WalkShapes): fn(G, U) on the shape of SET that `shape`
// (a CFG_*) maps to.  A kernel is instantiated for the shapes of its set only.
#define WALK_SHAPE(g, u) return (void)fn(std::integral_constant<int, g>{}, std::integral_constant<int, u>{})
template <int SET, class Fn>
inline void with_walk_shape(int shape, Fn&& fn) {
    if constexpr (SET == S_ALL9) {  // every shape its own
        switch (shape) {
            case CFG_G8U6: WALK_SHAPE(8, 6);
            case CFG_G8U7: WALK_SHAPE(8, 7);
            case CFG_G16U3: WALK_SHAPE(16, 3);
            case CFG_G16U4: WALK_SHAPE(16, 4);
            case CFG_G16U6: WALK_SHAPE(16, 6);
            case CFG_G32U3: WALK_SHAPE(32, 3);
            case CFG_G32U4: WALK_SHAPE(32, 4);
            case CFG_G64U2: WALK_SHAPE(64, 2);
            default: WALK_SHAPE(64, 4);
        }
    } else if constexpr (SET == S_SEG6) {
        // the whole-segment emit walks: the shapes emit picks (8 x 6 / 8 x 7 at a fixed stride, 16 x 3 /
        // 16 x 4 over descriptors) and 32 x 4 / 64 x 4 for long records; the others map to the one with
        // the same group size
        switch (shape) {
            case CFG_G8U6: WALK_SHAPE(8, 6);
            case CFG_G8U7: WALK_SHAPE(8, 7);
            case CFG_G16U3: WALK_SHAPE(16, 3);
            case CFG_G16U4:
            case CFG_G16U6: WALK_SHAPE(16, 4);
            case CFG_G32U3:
            case CFG_G32U4: WALK_SHAPE(32, 4);
            default: WALK_SHAPE(64, 4);
        }
    } else if constexpr (SET == S_EXP2) {  // fixed-stride emit experiments: 8 x 6, every other shape 8 x 7
        if (shape == CFG_G8U6) WALK_SHAPE(8, 6);
        WALK_SHAPE(8, 7);
    } else if constexpr (SET == S_COPY4) {
        // MODE_COPY keeps three chunks per lane and step (record + two source chunks): the U <= 3 shapes,
        // wider ones map to the same group size with fewer chunks
        switch (shape) {
            case CFG_G8U6:
            case CFG_G8U7: WALK_SHAPE(8, 3);
            case CFG_G32U3:
            case CFG_G32U4: WALK_SHAPE(32, 3);
            case CFG_G64U2:
            case CFG_G64U4: WALK_SHAPE(64, 2);
            default: WALK_SHAPE(16, 3);
        }
    } else if constexpr (SET == S_NHC3) {  // 6LoWPAN NHC: 8 x 6, 8 x 7, every other shape 16 x 3
        if (shape == CFG_G8U6) WALK_SHAPE(8, 6);
        if (shape == CFG_G8U7) WALK_SHAPE(8, 7);
        WALK_SHAPE(16, 3);
    } else if constexpr (SET == S_FIXED5) {  // emit_fields: the shapes auto_shape gives 5 over fixed strides
        switch (shape) {
            case CFG_G8U6: WALK_SHAPE(8, 6);
            case CFG_G8U7: WALK_SHAPE(8, 7);
            case CFG_G16U6: WALK_SHAPE(16, 6);
            case CFG_G32U4: WALK_SHAPE(32, 4);
            default: WALK_SHAPE(64, 4);
        }
    } else {  // S_G16U3, emit_fields over descriptors: 16 x 3 whatever the shape
        static_assert(SET == S_G16U3, "shape set");
        WALK_SHAPE(16, 3);
    }
}
#undef WALK_SHAPE

// The walk kernel a call runs: fn(form, number reported, G, U), from the registry's switch and the shape
// mappers; false: none (an error).  launch_walk and launch_walk_nhc (csum_walk.h) launch
// through it and smol_csum_tool_walk_launch reads it.
template <int MODE, bool IMPLICIT, bool NHC, class Fn>
inline bool with_walk_kernel(int variant, int shape, Fn&& fn) {
    auto shaped = [&](auto form, auto num, auto set) {
        with_walk_shape<decltype(set)::value>(shape, [&](auto g, auto u) { fn(form, num, g, u); });
    };
    if constexpr (NHC) {
        static_assert(MODE == MODE_EMIT || MODE == MODE_VERIFY, "the NHC entry points");
        with_walk_nhc_form(variant, shaped);
        return true;
    } else {
        return with_walk_form<MODE, IMPLICIT>(variant, shaped);
    }
}

// copy_kernel's shape sets (csum_variants.h CopyShapes): fn(G, U, UW, UB) on the shape of SET that `shape`
// maps to: lanes per record x body chunks per lane per round x generic round-1 slots per lane (0: enough
// for the window plus 8 chunks) x body round-1 slots per lane.  The default, 16 x 4 x 1 x 2, takes a C2copy
// record in two rounds: the window, its last chunk and 32 body chunks (loaded the body way), then the other 53.
// Measured on one MI355X (tools/exp_copy.py, profiles/r02b_experiments/): 16 x 4 x 1 x 2 0.689 ms,
// 16 x 5 x 1 x 1 0.691, 16 x 4 x 2 (body chunks in generic slots) 0.710, 16 x 3 0.743; earlier, before
// the hi-dword loads were skipped: 16 x 4 x 2 0.738, 16 x 3 0.760, 8 x 4 x 4 0.790, 8 x 6 0.837,
// 32 x 2 1.03, 64 x 2 1.73 (variant 16: 0.772).  Per-record work (parse, gates, window stores) is
// issued once per wavefront for its 64 / G records, so wide groups pay it for fewer records,
// narrow ones need more rounds.
#define COPY_SHAPE(g, u, uw, ub)                                                        \
    return (void)fn(std::integral_constant<int, g>{}, std::integral_constant<int, u>{}, \
                    std::integral_constant<int, uw>{}, std::integral_constant<int, ub>{})
template <int SET, class Fn>
inline void with_copy_shape(int shape, Fn&& fn) {
    if constexpr (SET == CSH_TABLE) {
        switch (shape) {
            case CFG_G8U6: COPY_SHAPE(8, 6, 0, 0);
            case CFG_G8U7: COPY_SHAPE(8, 4, 4, 0);
            case CFG_G16U3: COPY_SHAPE(16, 3, 0, 0);
            case CFG_G16U6: COPY_SHAPE(16, 5, 1, 1);
            case CFG_G32U3: COPY_SHAPE(16, 4, 2, 0);
            case CFG_G32U4: COPY_SHAPE(32, 2, 1, 0);
            case CFG_G64U2:
            case CFG_G64U4: COPY_SHAPE(64, 2, 0, 0);
            default: COPY_SHAPE(16, 4, 1, 2);  // CFG_G16U4
        }
    } else if constexpr (SET == CSH_TWO) {
        if (shape == CFG_G16U6) COPY_SHAPE(16, 5, 1, 1);
        COPY_SHAPE(16, 4, 1, 2);
    } else {
        static_assert(SET == CSH_ONE, "shape set");
        COPY_SHAPE(16, 4, 1, 2);
    }
}
#undef COPY_SHAPE

// The copy_kernel a copy-emit call runs: fn(form, number reported, G, U, UW, UB), from the registry's COPY
// rows and the shape mapper; false: the number has no COPY row built in this library.  launch_copy_kernel
// (csum_copy.hip) launches through it and smol_csum_tool_walk_launch reads it.
template <class Fn>
inline bool with_copy_kernel(int variant, int shape, Fn&& fn) {
    return with_copy_form(variant, [&](auto form, auto num) {
        with_copy_shape<decltype(form)::SHAPES>(shape,
                                                [&](auto g, auto u, auto uw, auto ub) { fn(form, num, g, u, uw, ub); });
    });
}

struct KParams {
    uint8_t* buf;
    const smol_csum_desc_t* desc;  // nullptr: implicit fixed-stride batch
    uint64_t n;
    uint64_t stride;
    uint32_t len;
    uint32_t kind;
    uint32_t caps_ipv4, caps_udp, caps_tcp, caps_icmpv4, caps_icmpv6;
    uint16_t* out16;  // MODE_DATA
    uint8_t* status;  // MODE_VERIFY (required), MODE_EMIT (optional)
    const uint8_t* dummy;  // 16-byte-aligned device line read by loads that have nothing to read
    uint32_t num_cu;       // compute units of the device (grid sizing)
    const uint8_t* src;             // MODE_COPY: payload source buffer
    const smol_csum_copy_t* copy;   // MODE_COPY: one payload copy per record (16-B aligned)
    const uint8_t* addrs;  // 6LoWPAN NHC UDP batches: 32 B (IPv6 src, dst) per record, else nullptr
    uint32_t xcd_remap;    // walk kernel: 0 dispatch order; 1 block b takes the records of block
                           // xcd_block(b); K >= 2: those of xcd_chunk(b, K) (see below)
    uint64_t* stage;       // staged emit (csum_walk.h stage_entry): one 8-B field entry per record
    uint32_t* stage_flags; // staged emit: one flag per 8 records (1: their entries are this call's)
    smol_csum_fields_t* fields;  // emit_fields: one 16-B entry per record (the kernels write nothing else)
};

// p over the records [i0, i0 + n): n, the batch (desc when set, else buf) and every per-record array that
// is set (status, out16, copy, addrs, fields) advanced to record i0; null stays null.  The rest is left
// alone: dummy and src are not indexed by record, and stage / stage_flags hold one chunk's entries, which
// the segment pass indexes from 0, so whoever cuts chunks attaches them after slicing.
inline KParams slice(const KParams& p, uint64_t i0, uint64_t n) {
    KParams q = p;
    q.n = n;
    if (p.desc) q.desc = p.desc + i0;
    else q.buf = p.buf + i0 * p.stride;
    if (p.status) q.status = p.status + i0;
    if (p.out16) q.out16 = p.out16 + i0;
    if (p.copy) q.copy = p.copy + i0;
    if (p.addrs) q.addrs = p.addrs + 32 * i0;
    if (p.fields) q.fields = p.fields + i0;
    return q;
}

// fn(i0, slice of p) over consecutive chunks of at most `per` records (0: the whole batch), in order;
// stops at the first result that is not zero (hipSuccess, SMOL_OK) and returns it.
template <class Fn>
inline auto for_chunks(const KParams& p, uint64_t per, Fn&& fn) -> decltype(fn(uint64_t{}, p)) {
    if (per == 0 || per > p.n) per = p.n;
    for (uint64_t i0 = 0; i0 < p.n; i0 += per) {
        const auto r = fn(i0, slice(p, i0, p.n - i0 < per ? p.n - i0 : per));
        if (r != decltype(r){}) return r;
    }
    return {};
}

// The 8 XCDs of an MI355X are dealt workgroups round-robin (MI355X_MICROARCH.md, workgroup dispatch:
// observed, not promised): blocks b, b + 8, ... share an XCD.  This bijection on [0, nwg) gives the
// blocks of one XCD a contiguous range of logical blocks, so that each XCD streams its own part of
// the batch (its L2 and address-translation caches see one region instead of every region).
__host__ __device__ inline uint64_t xcd_block(uint64_t b, uint64_t nwg) {
    const uint64_t q = nwg / 8, r = nwg % 8, x = b % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// The same at a finer grain: the XCDs take turns over runs of K consecutive logical blocks (K = 1 is
// the dispatch order).  A bijection: the first nwg rounded down to 8K blocks are permuted, the rest
// keep their index.
__host__ __device__ inline uint64_t xcd_chunk(uint64_t b, uint64_t nwg, uint64_t K) {
    const uint64_t full = nwg / (8 * K) * (8 * K);
    if (b >= full) return b;
    const uint64_t x = b % 8, j = b / 8;
    return ((j / K) * 8 + x) * K + (j % K);
}

#ifdef __HIPCC__
// The logical block this workgroup works as (KParams::xcd_remap).
__device__ inline uint64_t logical_block(uint32_t xcd_remap) {
    return xcd_remap == 0 ? (uint64_t)blockIdx.x
           : xcd_remap == 1 ? xcd_block(blockIdx.x, gridDim.x)
                            : xcd_chunk(blockIdx.x, gridDim.x, xcd_remap);
}
#endif

// The kernel instantiation of the process's last checksum launch, packed kernel << 24 | variant << 16
// | G << 8 | U (smol_csum_tool_last_launch): tests check that a forced variant runs the kernel it
// names rather than a dispatch fallback.
// KERN_*_FIELDS: the three forms of smol_csum_batch_emit_fields (variant 0; they have no registry row).
// KERN_VCOPY: smol_csum_batch_verify_copy's kernel (no registry row either; variant 0 plain body stores, 1
// non-temporal ones).
// KERN_FRAGCOPY: smol_csum_batch_verify_reassemble's kernel (no registry row; variant 0, G 64, U its chunks per lane).
// KERN_FRAGCUT: smol_csum_batch_fragment_emit's kernel (the same).
// KERN_TCPCUT: smol_csum_batch_tcp_segment_emit's kernel (the same).
// KERN_TCPASM: smol_csum_batch_verify_tcp_assemble's kernel (the same).
// KERN_ECHO: smol_csum_batch_verify_echo_reply's kernel (no registry row; variant 0, G and U its launch shape).
// KERN_UNREACH: smol_csum_batch_verify_unreach_reply's kernel (the same).
// KERN_UDPRX: smol_csum_batch_verify_udp_enqueue's kernel (no registry row; variant 0, G 64, U its chunks per lane).
// KERN_UDPTX: smol_csum_batch_udp_dequeue_emit's kernel (the same).
enum {
    KERN_WALK = 1, KERN_TILE = 2, KERN_COPY = 3, KERN_WALK_NHC = 4, KERN_XWALK = 5, KERN_DWALK = 6,
    KERN_WALK_FIELDS = 7, KERN_XWALK_FIELDS = 8, KERN_DWALK_FIELDS = 9, KERN_VCOPY = 10,
    KERN_FRAGCOPY = 11, KERN_FRAGCUT = 12, KERN_TCPCUT = 13, KERN_TCPASM = 14, KERN_ECHO = 15,
    KERN_UNREACH = 16, KERN_UDPRX = 17, KERN_UDPTX = 18
};
inline std::atomic<uint32_t> g_last_launch{0};
inline void note_launch(uint32_t kern, uint32_t var, uint32_t g, uint32_t u) {
    g_last_launch.store(kern << 24 | (var & 0xffu) << 16 | (g & 0xffu) << 8 | (u & 0xffu),
                        std::memory_order_relaxed);
}

// A dispatch may hold at most 2^32 - 1 work-items: 256-thread grids are capped at 2^24 - 1 blocks
// (every kernel loops with a grid stride, so a capped grid still covers the whole batch; C5's 2^27
// records per GPU need it).
constexpr uint64_t kMaxGridBlocks = 0xFFFFFFull;
__host__ __device__ inline uint32_t grid_blocks(uint64_t want, uint64_t cap) {
    uint64_t b = want < cap ? want : cap;
    b = b < kMaxGridBlocks ? b : kMaxGridBlocks;
    return (uint32_t)(b ? b : 1);
}

// Workgroups of `kernel` (256 threads) resident on the whole device, capped at max_blocks.
uint32_t resident_blocks(const void* kernel, uint32_t num_cu, uint32_t max_blocks);

hipError_t launch_csum(int mode, int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s);
// Walk kernel for one (mode, batch form): csum_walk.h, instantiated in csum_walk_*.hip (MODE_COPY: the
// experiments build's csum_walk_copy.hip).
template <int MODE, bool IMPLICIT>
hipError_t launch_walk(int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s);
// The same for 6LoWPAN NHC UDP batches (p.addrs set), csum_walk_nhc.hip.
template <int MODE, bool IMPLICIT>
hipError_t launch_walk_nhc(int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s);
// Tile kernel (csum_tile.hip), emit / verify only; var 0 = non-temporal loads, 1 = plain loads.
hipError_t launch_tile(int mode, int shape, int var, int tile_records, const KParams& p, uint32_t max_blocks,
                       hipStream_t s);

// The other families (which batches each serves: csum_dispatch.h; which variant runs which form of
// xwalk_kernel / dwalk_kernel: variants.def).  Stripe kernel: csum_tile.hip; transposed walk:
// csum_xwalk.hip; copy-emit on its layout: csum_xcopy.hip; descriptor-batch walks: csum_dwalk.hip.
hipError_t launch_stripe(int mode, const KParams& p, hipStream_t s);
hipError_t launch_dwalk(int mode, int variant, const KParams& p, hipStream_t s);
hipError_t launch_xcopy(int variant, const KParams& p, hipStream_t s);
// copy_kernel (csum_copy.hip): the class-split copy-emit kernel, the registry's COPY rows.
hipError_t launch_copy_kernel(int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s);
hipError_t launch_xwalk(int mode, int variant, const KParams& p, hipStream_t s);
// Staged emit (the registry's V_STAGED variants): the staging launch writes each record's field entry to
// p.stage, then the segment pass (csum_dwalk.hip; form 0 seg_pass4_kernel, 1 the first form, experiments
// build) writes the field segments whole.  Records per launch pair:
constexpr uint64_t kStageChunk = 1ull << 21;
hipError_t launch_seg_pass(const KParams& p, hipStream_t s, int form = 0);
// emit_fields (smol_csum_batch_emit_fields): MODE_EMIT's parse and gates with the fields sink, each
// record's 16-B entry to p.fields and nothing into the records.  Three forms outside the variant
// registry (csum_dispatch.h pick_fields chooses): the walk kernel (csum_walk_fields_{fixed,desc}.hip), the
// transposed walk (csum_xwalk.hip, form XFields) and the descriptor walk (csum_dwalk.hip).
template <bool IMPLICIT>
hipError_t launch_walk_fields(int shape, const KParams& p, uint32_t max_blocks, hipStream_t s);
hipError_t launch_xwalk_fields(const KParams& p, hipStream_t s);
hipError_t launch_dwalk_fields(const KParams& p, hipStream_t s);
// The two-launch route of fixed-stride whole-segment emit (csum_api.cpp run_one() takes it after pick_kernel
// has answered; no registry row): stage 1 is launch_xwalk_fields' kernel writing into p.fields (the context's entry
// buffer, which holds kRouteChunk entries), pass 2 the segment pass over those entries
// (csum_segpass.hip seg_pass_fields_kernel; the rule: csum_segrule.h).
constexpr uint64_t kRouteChunk = kStageChunk * sizeof(uint64_t) / sizeof(smol_csum_fields_t);
hipError_t launch_xwalk_route(int variant, const KParams& p, hipStream_t s);
hipError_t launch_seg_pass_fields(const KParams& p, hipStream_t s);

// verify_copy (smol_csum_batch_verify_copy, csum_vcopy.hip): verify's parse, sums and gates, and each
// record's L4 payload delivered to its slot of `dst` in the same pass.  Outside the variant registry.
struct VCopyArgs {
    uint8_t* dst;
    const smol_csum_slot_t* slots;  // one 16-B entry per record (input)
    smol_csum_span_t* spans;        // one 8-B entry per record (output)
};
// `nt`: body chunks stored non-temporal instead of with the default cache policy (measurements).
hipError_t launch_vcopy(int shape, bool nt, const KParams& p, const VCopyArgs& v, uint32_t max_blocks,
                        hipStream_t s);

// Synthetic batches and fault injection (tools; include/smolcsum_tools.h).
struct SynthParams {
    uint8_t* buf;
    const smol_csum_desc_t* desc;
    uint64_t n;
    uint64_t stride;
    uint32_t len;
    uint32_t profile;
    uint64_t seed;
};
hipError_t launch_synth(const SynthParams& p, uint32_t max_blocks, hipStream_t s);
hipError_t launch_corrupt(const SynthParams& p, uint32_t every, hipStream_t s);
// IPv4 fragment groups (csum_frag.hip): MODE_EMIT / MODE_VERIFY, one wavefront per group.
hipError_t launch_frag(int mode, const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                       hipStream_t s);
// verify_reassemble (smol_csum_batch_verify_reassemble, csum_fragcopy.hip): verify_frag's status bytes, and
// every usable group's fragment payloads delivered to the group's slot of `dst` in the same pass.  One
// 256-thread workgroup per group; outside the variant registry.
struct FragCopyArgs {
    uint8_t* dst;
    const smol_csum_slot_t* slots;  // one 16-B entry per group (input)
    smol_csum_dgram_t* dgrams;      // one 16-B entry per group (output)
};
hipError_t launch_fragcopy(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                           const FragCopyArgs& v, hipStream_t s);
// fragment_emit (smol_csum_batch_fragment_emit, csum_fragcut.hip): emit's checksums, and every whole IPv4
// datagram cut into frames in its place of `dst` in the same pass.  One wavefront per datagram; outside the
// variant registry.
struct FragCutArgs {
    uint8_t* dst;
    const smol_csum_fragplan_t* plans;  // one 16-B entry per record (input)
    uint32_t frame_stride;              // 0: frames back to back
    smol_csum_fragout_t* out;           // one 16-B entry per record (output)
};
hipError_t launch_fragcut(const KParams& p, const FragCutArgs& v, hipStream_t s);
// tcp_segment_emit (smol_csum_batch_tcp_segment_emit, csum_tcpcut.hip): every send's header template and
// payload range cut into MSS-sized frames in its place of `dst`, each frame's checksums filled in the same
// pass.  One wavefront per send; outside the variant registry.
struct TcpCutArgs {
    const uint8_t* src;                // payload source buffer
    uint8_t* dst;
    const smol_csum_tcpplan_t* plans;  // one 32-B entry per record (input)
    uint32_t frame_stride;             // 0: frames back to back
    smol_csum_tcpout_t* out;           // one 16-B entry per record (output)
};
hipError_t launch_tcpcut(const KParams& p, const TcpCutArgs& v, hipStream_t s);
// verify_tcp_assemble (smol_csum_batch_verify_tcp_assemble, csum_tcpasm.hip): verify's status bytes, and every
// TCP segment's payload delivered to its sequence number's place in its group's receive ring in `dst`, trimmed
// to the group's window, in the same pass.  One 256-thread workgroup per group; outside the variant registry.
struct TcpAsmArgs {
    uint8_t* dst;
    const smol_csum_tcpwin_t* wins;  // one 32-B entry per group (input)
    smol_csum_tcpseg_t* segs;        // one 16-B entry per record (output)
    smol_csum_tcpflow_t* flows;      // one 16-B entry per group (output)
};
// max_blocks: the grid cap (smol_csum_tool_set_max_blocks: a few workgroups walk many groups).
hipError_t launch_tcpasm(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                         const TcpAsmArgs& v, uint32_t max_blocks, hipStream_t s);
// verify_echo_reply (smol_csum_batch_verify_echo_reply, csum_echo.hip): verify's status bytes, and for every
// ICMP echo request that the wire-level address rule answers (csum_echo.h) the whole reply frame written to
// the record's slot of `dst` in the same pass: fresh head, the request's data, both checksums filled.  Outside
// the variant registry.
struct EchoArgs {
    uint8_t* dst;
    const smol_csum_slot_t* slots;  // one 16-B entry per record (input)
    smol_csum_echo_t* echo;         // one 8-B entry per record (output)
    uint32_t bcast_v4;              // smol_csum_echo_cfg_t.bcast_v4 as a big-endian word (0: none)
};
hipError_t launch_echo(int shape, const KParams& p, const EchoArgs& v, uint32_t max_blocks, hipStream_t s);
// verify_unreach_reply (smol_csum_batch_verify_unreach_reply, csum_unreach.hip): verify's status bytes, and for
// every datagram nobody takes that the wire-level address rule answers (csum_unreach.h) the whole ICMP error
// frame written to the record's slot of `dst` in the same pass: both headers fresh, the payload's first bytes
// quoted, every checksum filled.  Outside the variant registry.
struct UnreachArgs {
    uint8_t* dst;
    const smol_csum_slot_t* slots;  // one 16-B entry per record (input)
    smol_csum_unreach_t* unr;       // one 8-B entry per record (output)
    const uint8_t* udp_open;        // the 8192-B port map (nullptr: no UDP datagram is refused)
    uint32_t bcast_v4;              // smol_csum_echo_cfg_t.bcast_v4 as a big-endian word (0: none)
};
hipError_t launch_unreach(int shape, const KParams& p, const UnreachArgs& v, uint32_t max_blocks, hipStream_t s);
// verify_udp_enqueue (smol_csum_batch_verify_udp_enqueue, csum_udprx.hip): verify's status bytes, and every UDP
// datagram's payload stored where its socket's PacketBuffer::enqueue places it (csum_pktbuf.h), the metadata
// entries written, in the same pass; one workgroup per group.  Outside the variant registry.
struct UdpRxArgs {
    uint8_t* dst;
    const smol_csum_udpsock_t* socks;  // one 48-B entry per group (input)
    smol_csum_udpmeta_t* meta;         // the metadata rings: 48-B entries (output)
    smol_csum_udprx_t* rx;             // one 16-B entry per record (output)
    smol_csum_udpsockout_t* out;       // one 32-B entry per group (output)
};
hipError_t launch_udprx(const KParams& p, const smol_csum_frag_group_t* groups, uint64_t ngroups,
                        const UdpRxArgs& v, uint32_t max_blocks, hipStream_t s);
// udp_dequeue_emit (smol_csum_batch_udp_dequeue_emit, csum_udptx.hip): every socket's transmit PacketBuffer
// dequeued (csum_pktbuf.h) and each datagram written out as a frame, headers built on the device, checksums
// filled in the pass that copies the payload; one workgroup per socket.  No batch, so no KParams: the caps and
// the dummy line travel here.  Outside the variant registry.
struct UdpTxArgs {
    const uint8_t* src;                  // the payload rings
    const smol_csum_udptxsock_t* socks;  // one 96-B entry per group (input)
    const smol_csum_udpmeta_t* meta;     // the metadata rings: 48-B entries (input)
    uint8_t* dst;
    smol_csum_udptx_t* tx;               // one 16-B entry per dequeued datagram (output)
    smol_csum_udptxout_t* out;           // one 32-B entry per group (output)
    const uint8_t* dummy;                // KParams::dummy
    uint32_t frame_stride;               // 0: frames back to back
    uint32_t caps_ipv4, caps_udp;
};
hipError_t launch_udptx(const UdpTxArgs& v, uint64_t ngroups, uint32_t max_blocks, hipStream_t s);
hipError_t launch_stream_read(const uint8_t* buf, uint64_t bytes, uint32_t* sink, uint32_t max_blocks,
                              hipStream_t s);
hipError_t launch_field_probe(uint8_t* buf, uint64_t bytes, uint64_t stride, uint32_t f1, uint32_t f2,
                              uint32_t max_blocks, hipStream_t s);
hipError_t launch_field_scatter(uint8_t* buf, uint64_t bytes, const uint64_t* addrs, const uint16_t* vals, uint64_t n,
                                int nt, hipStream_t s);
hipError_t launch_field_probe_list(uint8_t* buf, uint64_t bytes, const uint64_t* addrs, const uint32_t* first,
                                   int seg64, uint32_t max_blocks, hipStream_t s);
hipError_t launch_segment_probe(uint8_t* buf, uint64_t bytes, const uint32_t* bitmap, int nt, uint32_t max_blocks,
                                hipStream_t s);

}  // namespace smolcsum
