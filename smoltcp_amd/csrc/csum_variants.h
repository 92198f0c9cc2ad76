// Reader of variants.def: the variant table and its lookups, the named forms of csum_kernel, xwalk_kernel,
// dwalk_kernel, copy_kernel and xcopy_kernel, and the switches from (variant, mode) to a form.  Host-only (no
// HIP): csum_dispatch.h, the launchers and the tooling entry points all read variants through this file.
#pragma once

#include <stdint.h>

#include <type_traits>

namespace smolcsum {

enum Family { F_WALK, F_TILE, F_XWALK, F_DWALK, F_STRIPE, F_COPY, F_XCOPY };
enum VariantFlags { V_COPY_ONLY = 1, V_WALK_COPY = 2, V_LINE = 4, V_G16U4 = 8, V_STAGED = 16, V_NOSTORE = 32, V_NHC_LINE = 64 };

// ---- csum_kernel's forms (the walk kernel, csum_walk.h) ---------------------------------------------
// The defaults are the plainest walk: the 16-B chunk grid, loads with the default cache policy, the next
// step prefetched into a second register set.  csum_walk.h's WalkTraits gates the emit-only members by
// mode and batch form; the measurements behind each form are in DESIGN.md §5 / §6.
struct WPlain {
    static constexpr bool NT = false;     // non-temporal loads
    static constexpr bool PF = true;      // register prefetch of the next step
    static constexpr bool LINE = false;   // chunk grid from the record's 128-B line (nt loads need whole lines)
    static constexpr int CACHED_U = 0;    // the first CACHED_U chunks of every lane's step loaded cached
    static constexpr int CU0 = 0;         // ... of a group's first load only (0: CACHED_U)
    // copy-emit (MODE_COPY): the second source chunk from the next lane; dword-aligned source loads; every
    // byte of the record written
    static constexpr bool SHUF = false, SHUF2 = false, WHOLE = false;
    // fixed-stride emit: whole 64-B field segments, the neighbours' field ranges published in LDS (SEGW);
    // SEGOPT bit 0: skipped on wavefronts that hold no IPv4 record
    static constexpr bool SEGW = false;
    static constexpr int SEGOPT = 0;
    // emit: the same with the neighbours' record extents published, so descriptor batches too (SEGG); the
    // whole workgroup's neighbours (SEGB); IPv6 records too (SEG6)
    static constexpr bool SEGG = false, SEGB = false, SEG6 = false;
    // fixed-stride emit: whole segments decided by one ballot (BSEG); IPv6 records too (BSEG6); only on
    // wavefronts without an IPv4 record (BSEG_NO4); the segments stored write-through non-temporal (NTSEG)
    static constexpr bool BSEG = false, BSEG6 = false, BSEG_NO4 = false, NTSEG = false;
    static constexpr bool GLDS = false;     // emit: the record geometry in LDS (as verify keeps it)
    static constexpr bool NOSHARE = false;  // fixed-stride emit: no shared boundary lines (shared_from)
    static constexpr bool NOSTORE = false;  // emit: every store compiled out (wrong bytes, timing only)
    static constexpr int MIN_WAVES = 1;     // occupancy floor, wavefronts per SIMD
    static constexpr bool FIELDS = false;   // emit: the fields sink (WFields)
};
enum WalkOpt { WO_GLDS = 1, WO_NOSHARE = 2, WO_BLOCK = 4, WO_IPV6 = 8 };
struct WNt : WPlain { static constexpr bool NT = true; };         // 0
struct WNtNoPf : WNt { static constexpr bool PF = false; };       // 2
struct WNoPf : WPlain { static constexpr bool PF = false; };      // 8: fewer VGPRs, more waves: C2 copy-emit 0.95 -> 0.85 ms
struct WShuf : WNoPf { static constexpr bool SHUF = true; };      // 11
struct WShufDword : WShuf { static constexpr bool SHUF2 = true, WHOLE = true; };  // 16: four v_alignbyte, one dword from the next lane
struct WLinePlain : WPlain { static constexpr bool LINE = true; };  // 6
struct WLine : WLinePlain { static constexpr bool NT = true; };     // 5: 16-B grid + nt 5.8 TB/s, line grid + nt 7.3 TB/s
template <int N> struct WLineCached : WLine { static constexpr int CACHED_U = N; };  // 9, 10: the fields' lines stay in L2 for the field stores
struct WLineNoPf : WLine { static constexpr bool PF = false; };         // 13
struct WLineNoStore : WLine { static constexpr bool NOSTORE = true; };  // 69
// emit_fields (smol_csum_batch_emit_fields): 5's emit walk, every record's 16-B entry to p.fields instead of
// its fields into the record.  No variants.def row: launch_walk_fields runs it, outside the registry.
struct WFields : WLine { static constexpr bool FIELDS = true; };
template <int O> struct WLineExp : WLine {  // 31, 35, 36: emit walks shaped like verify's
    static constexpr bool GLDS = (O & WO_GLDS) != 0, NOSHARE = (O & WO_NOSHARE) != 0;
};
struct WSeg19 : WLine { static constexpr bool SEGW = true; };    // 19: C2 emit 0.305 -> 0.285 ms when every segment goes out whole
// 29: IPv6 records have one field and keep the 2-B store (round 4 also measured its segments stored
// non-temporal: C2 emit 0.303 against 0.296 ms; removed)
struct WSeg29 : WSeg19 { static constexpr int SEGOPT = 1; };
template <int O> struct WSeg29Exp : WSeg29 {  // 32, 33, 34
    static constexpr bool GLDS = (O & WO_GLDS) != 0, NOSHARE = (O & WO_NOSHARE) != 0;
};
template <int O> struct WBallot : WLine {  // 37, 38
    static constexpr bool BSEG = true, BSEG6 = (O & WO_IPV6) != 0;
};
struct WSeg39 : WSeg29 { static constexpr bool BSEG = true, BSEG6 = true, BSEG_NO4 = true; };  // 39: 29 with an IPv4 record, 38's ballot without
struct WSeg39NtSeg : WSeg39 { static constexpr bool NTSEG = true; };    // 40: plain nt lost (round 5); now sc1 nt as xwalk's 101
struct WSeg39CachedFirst : WSeg39 { static constexpr int CU0 = 2; };    // 12: the header lines (the LDS window) cached, so the field stores hit L2
struct WSeg39CachedEvery : WSeg39 { static constexpr int CACHED_U = 2; };  // 14
template <int O> struct WSegG : WLine {  // 23, 24, 25
    static constexpr bool SEGG = true, SEGB = (O & WO_BLOCK) != 0, SEG6 = (O & WO_IPV6) != 0;
};
template <int O> struct WSegGNoPf : WSegG<O | WO_IPV6> { static constexpr bool PF = false; };  // 26, 27
struct WSegG28 : WSegGNoPf<0> { static constexpr int MIN_WAVES = 7; };  // 28: 13's occupancy at 16 x 4; the segment decision otherwise costs two waves

// Where a WALK row's own kernel runs (smol_csum_batch_data / emit / verify; elsewhere the row's `else`
// number runs and is the one reported, or the call is an error).  Copy-emit is apart: the walk kernel's
// MODE_COPY form of a number runs exactly where the row has V_WALK_COPY, on copy's shapes.
enum WalkScope { W_ALL, W_EMIT, W_EMIT_FIXED, W_COPY };
constexpr int W_ERR = -2;  // `else`: no kernel (hipErrorInvalidValue)
// The shapes a kernel is built for (csum_launch.h with_walk_shape maps every CFG_* into the set).
enum WalkShapes { S_ALL9, S_SEG6, S_EXP2, S_COPY4, S_NHC3, S_FIXED5, S_G16U3 };
constexpr int kOpData = 0, kOpEmit = 1, kOpVerify = 2, kOpCopy = 3;  // csum_launch.h MODE_*

// ---- xwalk_kernel's forms (csum_xwalk.hip explains each constant) -----------------------------------
enum XwalkNts {
    NTS_PLAIN = 0,
    NTS_NT = 1,                   // the segments stored non-temporal, always (57)
    NTS_NT_IF_IPV4 = 2,           // ... on a wavefront that holds an IPv4 record (58)
    NTS_HEAD_KIB_CACHED = 4,      // each record's first load instruction (its first KiB) with the default cache policy (45)
    NTS_HEAD_KIB_CACHED_NT = 5,   // 45 with the segments stored non-temporal (15)
    NTS_ALL_CACHED = 8,           // every load with the default cache policy (43)
    NTS_HEAD_LINES_CACHED = 16,   // only the record's two header lines (lanes 0-15 of its first instruction) cached (46)
    NTS_STAGE_FIELDS_CACHED = 32, // staged: the lanes that hold the segments of record offsets [10, 28) cached (80)
    NTS_WT_SC0 = 64,              // the segments stored sc0 sc1 nt (100)
    NTS_WT = 65,                  // the segments stored sc1 nt, write-through and non-temporal (101)
    NTS_STATUS_NT = 128,          // verify: the status bytes stored non-temporal (108)
};
// Lanes of a record's first load instruction that load with the default cache policy (the rest nt).
enum XwalkHint {
    HINT_NONE = 0,
    HINT_FIELD_SEGS = 1,     // the segments of record offsets [10, 28) (an IPv4 record's fields)
    HINT_FIRST_64 = 2,       // those of [0, 64)
    HINT_WINDOW = 3,         // the whole 256-B window
    HINT_SEG_OF_10 = 4,      // the segment of offset 10 only
    HINT_CHUNK_OF_10 = 5,    // the 16-B chunk of offset 10 only
    HINT_FIRST_SEG = 6,      // the segment of the record's first byte
    HINT_LINE_HEAD = 7,      // the line's first segment (lanes 0-3)
    HINT_SPLIT_ONLY = 8,     // instruction 0 split in two (lanes 0-3 / the rest), both non-temporal
    HINT_LINE_HEAD_2ND = 9,  // lanes 0-3 of instruction 1 with the default policy
    HINT_LINE_HEAD_ALL = 10, // lanes 0-3 of every instruction
};

// The defaults: 2-B field stores (emit), nothing hinted; also the form run where a form's ONLY_R /
// MAX_LEN does not hold.
struct XPlain {
    static constexpr bool NOSTORE = false, SEG = false, PERSIST = false, HALF = false, STAGE = false;
    static constexpr bool FIELDS = false;  // emit: the fields sink (XFields)
    static constexpr int NTS = NTS_PLAIN, HINT = HINT_NONE;
    static constexpr int WPE = 0;    // wavefronts per SIMD the kernel is held to (0: the compiler's)
    static constexpr int WV = 4;     // wavefronts per workgroup (8: 512 threads, half the grid)
    static constexpr int STEPS = 1;  // tiles per workgroup (2: half the grid)
    static constexpr int ONLY_R = 0;               // the form exists at this many records per wavefront only
    static constexpr uint32_t MAX_LEN = ~0u;       // ... and up to this record length
};
template <int N> struct XNts : XPlain { static constexpr int NTS = N; };
template <int H> struct XHint : XPlain { static constexpr int HINT = H; };
template <int W> struct XHint7Wpe : XHint<HINT_LINE_HEAD> { static constexpr int WPE = W; };
struct XNoStoreHint : XHint<HINT_LINE_HEAD> { static constexpr bool NOSTORE = true; };
struct XStatusNt : XHint<HINT_LINE_HEAD> { static constexpr int NTS = NTS_STATUS_NT; };
struct XWide : XHint<HINT_LINE_HEAD> { static constexpr int WV = 8, ONLY_R = 8; };
struct XTwoTiles : XHint<HINT_LINE_HEAD> { static constexpr int STEPS = 2; };
struct XHalf : XPlain { static constexpr bool HALF = true; static constexpr int ONLY_R = 8; static constexpr uint32_t MAX_LEN = 1409; };
struct XPersist : XPlain { static constexpr bool PERSIST = true; };
struct XSeg : XPlain { static constexpr bool SEG = true; };
template <int N> struct XSegNts : XSeg { static constexpr int NTS = N; };
template <int H> struct XSegHint : XSeg { static constexpr int HINT = H; };
template <int H> struct XSegNtHint : XSegNts<NTS_NT> { static constexpr int HINT = H; };
template <int H> struct XSegWtHint : XSegNts<NTS_WT> { static constexpr int HINT = H; };
template <int W> struct XSegNtWpe : XSegNts<NTS_NT> { static constexpr int WPE = W; };
struct XSegWtTwoTiles : XSegNts<NTS_WT> { static constexpr int STEPS = 2; };
struct XSegHalf : XSeg { static constexpr bool HALF = true; static constexpr int ONLY_R = 8; static constexpr uint32_t MAX_LEN = 1409; };
struct XSegPersist : XSeg { static constexpr bool PERSIST = true; };
struct XSegNoStore : XSeg { static constexpr bool NOSTORE = true; };
struct XStage : XSeg { static constexpr bool STAGE = true; };
struct XStageCached : XStage { static constexpr int NTS = NTS_STAGE_FIELDS_CACHED; };
// emit_fields (smol_csum_batch_emit_fields): XPlain's emit reading like verify's 'h' form, every record's
// 16-B entry to p.fields instead of its fields into the record.  No variants.def row: launch_xwalk_fields
// runs it, outside the registry.
struct XFields : XHint<HINT_LINE_HEAD> { static constexpr bool FIELDS = true; };

// ---- dwalk_kernel's forms (csum_dwalk.hip) ----------------------------------------------------------
enum DwalkSegf {
    DW_SEG = 1,             // whole 64-B field segments from the LDS window (61)
    DW_WIN_CACHED = 2,      // the header windows loaded with the default cache policy (63)
    DW_FIELDS_NT = 4,       // the 2-B fields stored non-temporal (18, 20)
    DW_WIN_SUM = 8,         // the window's 16 chunks summed from LDS, the stream from chunk 16 (41)
    DW_STAGE = 16,          // staged, the first form: with DW_SEG, entries from the patched window (94)
    DW_WAVES8 = 32,         // held to 8 wavefronts per SIMD (95)
    DW_LITE = 64,           // staged from the finish's registers: no window patch, no segment addresses (96, 97)
    DW_LITE_WAVES8 = 128,   // held to 8 wavefronts per SIMD (96)
    DW_FIRST = 256,         // the wavefront's first record may stage too (97)
    DW_GAPS = 512,          // staging over gapped / shuffled layouts (104)
    DW_ENTRIES_NT = 1024,   // entries and 2-B fields stored write-through non-temporal (109)
    DW_FIELDS_OUT = 2048,   // emit_fields: the fields sink, nothing into the records (no registry row: launch_dwalk_fields)
};
struct DNone {  // the variant has no form of this mode (in this library)
    static constexpr bool NONE = true, NOSTORE = false, GROUPS = false;
    static constexpr int SEGF = 0;
    static constexpr int SEGPASS = -1;  // the segment pass after the launch: -1 none, 0 seg_pass4_kernel, 1 the first form
};
struct DSpan : DNone { static constexpr bool NONE = false; };
struct DSpanNoStore : DSpan { static constexpr bool NOSTORE = true; };
struct DGroups : DSpan { static constexpr bool GROUPS = true; };
template <int S> struct DG : DGroups { static constexpr int SEGF = S; };
struct DSegNoStore : DG<DW_SEG> { static constexpr bool NOSTORE = true; };
template <int S> struct DStaged : DG<S> { static constexpr int SEGPASS = 0; };
using DLiteFirst = DStaged<DW_WIN_CACHED | DW_WIN_SUM | DW_LITE | DW_FIRST>;
struct DLiteFirstPass8B : DLiteFirst { static constexpr int SEGPASS = 1; };

// ---- copy_kernel's forms (csum_copy.hip) -------------------------------------------------------------
enum CopyStore { CST_PLAIN, CST_NT, CST_WT };  // the body chunks stored with the default cache policy, non-temporal, sc1 nt
// The launch shapes a number is built for (csum_launch.h with_copy_shape maps every CFG_* into the set).
enum CopyShapes {
    CSH_TABLE,  // the nine-entry table
    CSH_TWO,    // 16 x 5 x 1 x 1 for CFG_G16U6, every other shape 16 x 4 x 1 x 2
    CSH_ONE,    // 16 x 4 x 1 x 2 whatever the shape
};
struct CPlain {  // 17
    // the first body round's loads issued right after the parse, before round 1's chunk stores, so that
    // waiting for them does not also wait for those stores (gfx950 counts stores in vmcnt, in issue order
    // with the loads)
    static constexpr bool LBS = false;
    static constexpr int BODY_STORE = CST_PLAIN;
    static constexpr bool NT_BODY_LOADS = false;  // the body's source chunks loaded non-temporal
    // the destination chunks of the generic (header / edge) chunks loaded non-temporal
    static constexpr bool NT_GEN_DST = false;
    static constexpr int SHAPES = CSH_TABLE;
};
// 21 (the copy-emit default): 17's default shapes with LBS.  MI355X, C2copy, interleaved rounds on one box
// (tools/exp_copy.py, profiles/r04_experiments/copy_emit_lbs.jsonl): 16 x 4 x 1 x 2 0.678 ms against variant
// 17's 0.692; 16 x 5 x 1 x 1 0.711; also measured and not kept: 16 x 3 x 1 x 3 0.690, 16 x 3 x 1 x 2 0.728.
struct CLbs : CPlain { static constexpr bool LBS = true; static constexpr int SHAPES = CSH_TWO; };
struct CLbsOne : CLbs { static constexpr int SHAPES = CSH_ONE; };  // the experiments on 21: one shape
struct CNtStore : CLbsOne { static constexpr int BODY_STORE = CST_NT; };          // 30
struct CNtStoreLoad : CNtStore { static constexpr bool NT_BODY_LOADS = true; };   // 22
// 98 (round 6): whether the 28-B header reads then leave L2 as 64-B requests instead of whole 128-B lines;
// they do not
struct CNtGenDst : CLbsOne { static constexpr bool NT_GEN_DST = true; };
struct CWtStore : CLbsOne { static constexpr int BODY_STORE = CST_WT; };  // 102 (round 6; cf. 30's plain nt)

// ---- xcopy_kernel's forms (csum_xcopy.hip explains each constant) ----------------------------------
struct XcPlain {  // 49
    static constexpr bool PERSIST = false;    // a persistent grid, the next step's descriptors loaded ahead
    static constexpr bool SRC16 = false;      // source loads rounded down to 16 B (wrong bytes, timing only)
    static constexpr bool NOSTORE = false;    // no body stores (wrong bytes, timing only)
    static constexpr bool CALC_DESC = false;  // the C2copy descriptors computed, not loaded (timing only)
    static constexpr bool NT_STORES = false;  // non-temporal body stores
    static constexpr bool REDEAL = false;     // the body chunks re-dealt through LDS, stored walk-shaped
};
struct XcPersist : XcPlain { static constexpr bool PERSIST = true; };      // 50
struct XcSrc16 : XcPlain { static constexpr bool SRC16 = true; };          // 51
struct XcNoStore : XcPlain { static constexpr bool NOSTORE = true; };      // 52
struct XcCalcDesc : XcPlain { static constexpr bool CALC_DESC = true; };   // 53
struct XcNtStores : XcPlain { static constexpr bool NT_STORES = true; };   // 54
struct XcRedeal : XcPlain { static constexpr bool REDEAL = true; };        // 55

#ifdef SMOL_EXP
#define EXP_ONLY(form) form
constexpr bool kExpBuild = true;
#else
#define EXP_ONLY(form) DNone
constexpr bool kExpBuild = false;
#endif

// ---- the table --------------------------------------------------------------------------------------
struct Variant {
    int num;
    int family;
    bool exp_only;     // built in the experiments library only
    int flags;         // VariantFlags
    int field_twin;    // SMOL_BATCH_FIELD_STORES (emit)
    int verify_twin;
    int tile_loads;    // F_TILE: the tile kernel's load form
    bool emit, verify; // F_XWALK / F_DWALK: a form of that mode exists in this library
    const char* desc;
    bool is(int f) const { return (flags & f) != 0; }
    bool built() const { return !exp_only || kExpBuild; }
};

#define SELF (-1)
#define V_BUILD_P false
#define V_BUILD_X true
inline constexpr Variant kVariants[] = {
#define WALK(n, b, fl, ft, form, scope, els, shapes, d) {n, F_WALK, V_BUILD_##b, fl, ft, SELF, 0, true, true, d},
#define TILE(n, b, loads, d) {n, F_TILE, V_BUILD_##b, 0, SELF, SELF, loads, true, true, d},
#define STRIPE(n, b, d) {n, F_STRIPE, V_BUILD_##b, 0, SELF, SELF, 0, true, true, d},
#define COPY(n, b, form, d) {n, F_COPY, V_BUILD_##b, V_COPY_ONLY, SELF, SELF, 0, false, false, d},
#define XCOPY(n, b, form, d) {n, F_XCOPY, V_BUILD_##b, V_COPY_ONLY, SELF, SELF, 0, false, false, d},
#define XWALK(n, b, fl, ft, ef, vf, d) {n, F_XWALK, V_BUILD_##b, fl, ft, SELF, 0, true, true, d},
#define DWALK(n, b, fl, ft, vt, ef, vf, d) {n, F_DWALK, V_BUILD_##b, fl, ft, vt, 0, !ef::NONE, !vf::NONE, d},
#include "variants.def"
#undef WALK
#undef TILE
#undef STRIPE
#undef COPY
#undef XCOPY
#undef XWALK
#undef DWALK
};

// The row of a number (nullptr: none; -1, the automatic choice, has none).
inline const Variant* find_variant(int v) {
    for (const Variant& r : kVariants)
        if (r.num == v) return &r;
    return nullptr;
}
inline bool variant_built(int v) {
    const Variant* r = find_variant(v);
    return v == -1 || (r && r->built());
}
inline bool variant_is(int v, int flag) {
    const Variant* r = find_variant(v);
    return r && r->is(flag);
}
inline int field_store_variant(int v) {
    const Variant* r = find_variant(v);
    return r && r->field_twin != SELF ? r->field_twin : v;
}
inline int verify_variant(int v) {
    const Variant* r = find_variant(v);
    return r && r->verify_twin != SELF ? r->verify_twin : v;
}

// ---- the walk kernel's rows -------------------------------------------------------------------------
template <int N> struct WalkRow;  // the WALK row of number N
#define WALK(n, b, fl, ft, form, scope, els, shapes, d)                               \
    template <> struct WalkRow<n> {                                                   \
        using Form = form;                                                            \
        static constexpr int FLAGS = fl, SCOPE = scope, ELSE = els, SHAPES = shapes;  \
    };
#define TILE(n, b, loads, d)
#define STRIPE(n, b, d)
#define COPY(n, b, form, d)
#define XCOPY(n, b, form, d)
#define XWALK(n, b, fl, ft, ef, vf, d)
#define DWALK(n, b, fl, ft, vt, ef, vf, d)
#include "variants.def"
#undef WALK

// Row N asked for (mode, batch form): fn(form, number reported, shape set) on the row's own kernel where it
// runs, else on the row's `else` number; false: an error.
template <int N, int MODE, bool IMPLICIT, class Fn>
inline bool with_walk_row(Fn&& fn) {
    using R = WalkRow<N>;
    constexpr bool own = MODE == kOpCopy ? (R::FLAGS & V_WALK_COPY) != 0
                         : R::SCOPE == W_ALL || (R::SCOPE == W_EMIT && MODE == kOpEmit) ||
                               (R::SCOPE == W_EMIT_FIXED && MODE == kOpEmit && IMPLICIT);
    if constexpr (own) {
        fn(typename R::Form{}, std::integral_constant<int, N>{},
           std::integral_constant<int, MODE == kOpCopy ? (int)S_COPY4 : R::SHAPES>{});
        return true;
    } else if constexpr (MODE != kOpCopy && R::ELSE >= 0) {
        return with_walk_row<R::ELSE, MODE, IMPLICIT>(fn);
    } else {
        return false;
    }
}

// (variant, mode, batch form) -> the walk kernel to run, over the rows built in this library.
template <int MODE, bool IMPLICIT, class Fn>
inline bool with_walk_form(int variant, Fn&& fn) {
    switch (variant) {
#define V_WALK_P(n) case n: return with_walk_row<n, MODE, IMPLICIT>(fn);
#ifdef SMOL_EXP
#define V_WALK_X(n) V_WALK_P(n)
#else
#define V_WALK_X(n)
#endif
#define WALK(n, b, fl, ft, form, scope, els, shapes, d) V_WALK_##b(n)
#include "variants.def"
#undef WALK
#undef V_WALK_P
#undef V_WALK_X
        default: return false;
    }
}
#undef XWALK
#undef DWALK

// 6LoWPAN NHC batches, any number: the NHC kernel's line-grid form (row 5) for a V_NHC_LINE number, its
// 16-B-grid form (row 1: an experiments row, but this form of it is built in both libraries) otherwise.
template <class Fn>
inline void with_walk_nhc_form(int variant, Fn&& fn) {
    if (variant_is(variant, V_NHC_LINE)) fn(WalkRow<5>::Form{}, std::integral_constant<int, 5>{}, std::integral_constant<int, S_NHC3>{});
    else fn(WalkRow<1>::Form{}, std::integral_constant<int, 1>{}, std::integral_constant<int, S_NHC3>{});
}

// (variant, mode) -> form: calls fn(Form{}) for the row's emit (EMIT) or verify form, over the rows built
// in this library; false: no such row.  The launchers instantiate kernels through these switches and
// smol_csum_tool_form reads the same ones.
#define V_FORM_P(n, ef, vf)            \
    case n:                            \
        if constexpr (EMIT) fn(ef{});  \
        else fn(vf{});                 \
        return true;
#ifdef SMOL_EXP
#define V_FORM_X(n, ef, vf) V_FORM_P(n, ef, vf)
#else
#define V_FORM_X(n, ef, vf)
#endif
#define WALK(n, b, fl, ft, form, scope, els, shapes, d)

template <bool EMIT, class Fn>
inline bool with_xwalk_form(int variant, Fn&& fn) {
    switch (variant) {
#define XWALK(n, b, fl, ft, ef, vf, d) V_FORM_##b(n, ef, vf)
#define DWALK(n, b, fl, ft, vt, ef, vf, d)
#include "variants.def"
#undef XWALK
#undef DWALK
        default: return false;
    }
}

template <bool EMIT, class Fn>
inline bool with_dwalk_form(int variant, Fn&& fn) {
    switch (variant) {
#define XWALK(n, b, fl, ft, ef, vf, d)
#define DWALK(n, b, fl, ft, vt, ef, vf, d) V_FORM_##b(n, ef, vf)
#include "variants.def"
#undef XWALK
#undef DWALK
        default: return false;
    }
}

// variant -> copy_kernel's (COPY rows) / xcopy_kernel's (XCOPY rows) form: calls fn(Form{}, number), over the
// rows built in this library; false: no such row.  The launchers instantiate the kernels through these.
#undef COPY
#undef XCOPY
#define XWALK(n, b, fl, ft, ef, vf, d)
#define DWALK(n, b, fl, ft, vt, ef, vf, d)
#define V_ROW_P(n, form)                              \
    case n:                                           \
        fn(form{}, std::integral_constant<int, n>{}); \
        return true;
#ifdef SMOL_EXP
#define V_ROW_X(n, form) V_ROW_P(n, form)
#else
#define V_ROW_X(n, form)
#endif

template <class Fn>
inline bool with_copy_form(int variant, Fn&& fn) {
    switch (variant) {
#define COPY(n, b, form, d) V_ROW_##b(n, form)
#define XCOPY(n, b, form, d)
#include "variants.def"
#undef COPY
#undef XCOPY
        default: return false;
    }
}

template <class Fn>
inline bool with_xcopy_form(int variant, Fn&& fn) {
    switch (variant) {
#define COPY(n, b, form, d)
#define XCOPY(n, b, form, d) V_ROW_##b(n, form)
#include "variants.def"
#undef COPY
#undef XCOPY
        default: return false;
    }
}
#undef XWALK
#undef DWALK
#undef WALK
#undef TILE
#undef STRIPE
#undef V_ROW_P
#undef V_ROW_X
#undef V_FORM_P
#undef V_FORM_X
#undef V_BUILD_P
#undef V_BUILD_X
#undef EXP_ONLY
#undef SELF

}  // namespace smolcsum
