// Fused payload copy + emit on the transposed walk's load layout (variant 49, experiments build):
// fixed-stride batches of 1024 .. 1921-byte records.  Same result as copy_kernel (csum_copy.hip):
// bit-identical to a memcpy of every payload followed by smol_csum_batch_emit.
//
// A wavefront owns 8 consecutive records, a group of 8 lanes each for the parse and the gates
// (csum_xwalk.hip's layout).  On the record's 16-B chunk grid:
// * the WINDOW (chunks 0 .. 7, the headers) is built by group j, lane i taking chunk i of record j:
//   the destination chunk and the two aligned source chunks under its payload bytes, merged with
//   byte masks, into LDS;
// * BODY chunks (8 .. nch - 2) are all payload: load instruction (s, j) covers 64 of record j's body
//   chunks, one per lane, each one dwordx4 from the chunk's first source byte rounded down to 4
//   (plus the dword after it when the source and destination 4-byte phases differ: a wave-uniform
//   test per record), shifted by a per-record constant with v_alignbyte, summed and stored whole;
// * the EDGE chunk (nch - 1, the record's last bytes and the next record's first ones) is built by
//   lane 0 of the group from two aligned source chunks and stored byte-masked.
// That layout needs every record of the wavefront to have its payload run from inside the window to
// the record's end (TCP / UDP payloads: dst_offset + len == record length, dst_offset + the
// record's 16-B phase <= 128).  A wavefront holding any other record (or a copy range that does not
// fit) takes the generic path: group j builds every chunk of record j the window's way.
// Aligned 16-B source chunks are loaded only when they overlap the payload, and a dwordx4 from a
// 4-byte-aligned address only when all of its chunk's 16 bytes are payload, so no load touches a
// page that holds none of the source range.
#include "csum_copyemit.h"

namespace smolcsum {

#ifdef SMOL_EXP

namespace xcopy {

constexpr int R = 8;        // records per wavefront
constexpr int G = 8;        // lanes per record (parse, gates)
constexpr int NS = 2;       // body load instructions per record (64 chunks each)
constexpr int WAVES = 4;
constexpr int GPB = WAVES * R;
using namespace copyemit;  // WIN, RecGeom, gen_load / gen_merge, far_fields, ByteReader

// What the parse leaves a group: the record's geometry, the end of its summed span (0: no L4 sum) and the
// fields past the window, which stay out of the chunk stores (finish_gates writes them).
struct Parsed {
    Geom g;
    int s1;
    FarFields ff;
};
// The group's window chunk wm of lane `lane` into LDS (has: the chunk exists), then the parse (mine: the
// group has a record).
__device__ __forceinline__ Parsed parse_window(u32x4* wn, int lane, const u32x4& wm, bool has, bool mine,
                                               const ByteReader& rd, uint32_t len, uint32_t kind) {
    if (has) wn[lane] = wm;
    wave_lds_sync();
    Parsed ps;
    ps.g = Geom{};
    if (mine) ps.g = parse_geometry<false>(rd, len, kind, true);
    const bool l4 = ps.g.proto != P_NONE && !(ps.g.st & SMOL_ST_MALFORMED);
    ps.s1 = mine && l4 ? (int)ps.g.span_end : 0;
    if (mine) ps.ff = far_fields(ps.g, rd.q.head, WIN);
    return ps;
}

}  // namespace xcopy

// F: the form, one of csum_variants.h's named structs (XcPlain and what differs from it); variants.def says
// which number runs which.  Its constants:
// PERSIST (variant 50): a grid of the resident workgroups whose wavefronts step over the batch 8 records
// at a time, loading the next step's copy descriptors ahead, so that a step waits for one round
// trip (its loads) instead of two (the descriptors, then the loads that need them).
// SRC16, NOSTORE, CALC_DESC (variants 51-53, timing only, wrong bytes): source loads rounded down to 16 B
// instead of 4; no body stores; the C2copy descriptors computed, not loaded (src_offset 1472 r, dst 28).
// NT_STORES (variant 54, exact): non-temporal body stores.  REDEAL (variant 55, exact): the body chunks
// re-dealt through LDS and stored walk-shaped, each store instruction covering 128 B of each of the 8 records.
template <class F>
__global__ __launch_bounds__(256) void xcopy_kernel(KParams p) {
    using namespace xcopy;
    constexpr bool PERSIST = F::PERSIST, REDEAL = F::REDEAL;
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ uint32_t spanbuf[GPB];
    __shared__ u32x4 stg[REDEAL ? WAVES : 1][REDEAL ? R : 1][64];  // REDEAL: one half-step's body chunks
    const int wl = (int)(threadIdx.x & 63);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = wl & (G - 1);
    const int gw = wl / G;
    const int gib = wv * R + gw;
    const uint64_t dummy = (uint64_t)p.dummy;
    const uint32_t len = p.len;
    const uint64_t nwaves = PERSIST ? (uint64_t)gridDim.x * WAVES : 0;
    uint64_t tw = logical_block(p.xcd_remap) * WAVES + (uint64_t)wv;
    // the copy descriptors of step tw (lane j: record j)
    auto load_dsc = [&](uint64_t t) -> u32x4 {
        const uint64_t r0 = t * R;
        const uint32_t c = (uint32_t)(p.n - r0 < (uint64_t)R ? p.n - r0 : (uint64_t)R);
        return (uint32_t)wl < c ? *(gcv4)((uint64_t)p.copy + 16 * (r0 + (uint64_t)wl)) : u32x4{0, 0, 0, 0};
    };
    if (tw * R >= p.n) return;
    u32x4 dsc_next = load_dsc(tw);
    for (; tw * R < p.n; tw += nwaves) {
    const u32x4 dsc = dsc_next;
    if (PERSIST && (tw + nwaves) * R < p.n) dsc_next = load_dsc(tw + nwaves);
    const uint64_t rw0 = tw * R;
    const uint32_t cnt = (uint32_t)(p.n - rw0 < (uint64_t)R ? p.n - rw0 : (uint64_t)R);
    const bool mine = (uint32_t)gw < cnt;
    const uint64_t r = rw0 + (uint64_t)gw;
    // this group's descriptor from lane gw
    const uint32_t cx = (uint32_t)__shfl((int)dsc.x, gw, 64), cy = (uint32_t)__shfl((int)dsc.y, gw, 64);
    const uint32_t cz = (uint32_t)__shfl((int)dsc.z, gw, 64), cw = (uint32_t)__shfl((int)dsc.w, gw, 64);
    const bool bad = !F::CALC_DESC && (uint64_t)cz + cw > len;  // the copy range does not fit
    // the payload [p0, p1) of the record, from sb + p0 (CALC_DESC: src_offset 1472 r, dst 28)
    const uint32_t p0 = F::CALC_DESC ? 28u : bad ? 0u : cz;
    const uint32_t p1 = F::CALC_DESC ? len : bad ? 0u : cz + cw;
    const uint64_t sb = F::CALC_DESC ? (uint64_t)p.src + 1472ull * r - 28
                        : bad        ? 0ull
                                     : (uint64_t)p.src + ((uint64_t)cx | ((uint64_t)cy << 32)) - cz;
    const uint64_t a0 = (uint64_t)p.buf + r * p.stride;
    // the group's own record (per-lane values, equal within the group)
    const RecGeom q(a0, (uint32_t)(((a0 + len + 15) >> 4) - (a0 >> 4)), sb, p0, p1);
    const bool fast_rec = !mine || (!bad && q.p1 > q.p0 && q.p1 == len && q.head + q.p0 <= (uint32_t)WIN);
    const bool fast = __all(fast_rec);
    u32x4* wn = &win[gib][0];
    const uint8_t* winb = reinterpret_cast<const uint8_t*>(wn);
    const ByteReader rd{winb, q};

    if (fast) {
        // ---- window sources (group j, lane i: chunk i) and the edge chunk's (lane 0) ----
        const Gen gwin = gen_load(q, (uint32_t)lane, mine, dummy);
        const uint32_t kedge = q.nch - 1;
        const Gen gedge = gen_load(q, kedge, mine && lane == 0, dummy);
        // ---- body: record j's chunks 8 .. nch - 2, chunk 64 s + wl of instruction (s, j) ----
        u32x4 v[NS][R];
        uint32_t vh[NS][R];
        uint32_t bsh[R], hd[R], nb[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const uint64_t a0 = (uint64_t)p.buf + (rw0 + (uint64_t)j) * p.stride;
            const uint32_t h = (uint32_t)(a0 & 15u);
            const uint32_t nc = (uint32_t)(((a0 + len + 15) >> 4) - (a0 >> 4));
            // source of grid byte 0: sb_j - head_j (sb_j from lane j's descriptor)
            uint64_t so = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)dsc.x, j) |
                          ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)dsc.y, j) << 32);
            uint32_t dz = (uint32_t)__builtin_amdgcn_readlane((int)dsc.z, j);
            if (F::CALC_DESC) {
                so = 1472ull * (rw0 + (uint64_t)j);
                dz = 28;
            }
            const uint64_t sk = (uint64_t)p.src + so - dz - h;
            const uint64_t skA = F::SRC16 ? (sk & ~15ull) : (sk & ~3ull);
            bsh[j] = (uint32_t)(sk & 3u);
            hd[j] = h;
            nb[j] = (uint32_t)j < cnt ? nc - 1 : 0u;  // body chunks are [8, nb)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t k = (uint32_t)(64 * s + wl);
                const bool in = k >= (uint32_t)WIN_CH && k < nb[j];
                const uint64_t A = skA + 16ull * k;
                v[s][j] = ld16<false>((gcv4)(in ? A : dummy));
                vh[s][j] = 0;
                if (bsh[j] != 0) vh[s][j] = *(const GMEM uint32_t*)(in ? A + 16 : dummy);
            }
        }
        // ---- the window into LDS, the parse ----
        const u32x4 wm = gen_merge(q, (uint32_t)lane, gwin);
        const Parsed ps = parse_window(wn, lane, wm, mine, mine, rd, len, p.kind);
        const Geom& g = ps.g;
        const int s1 = ps.s1, f0b = ps.ff.f0, f1b = ps.ff.f1, f2b = ps.ff.f2;
        if (lane == 0) spanbuf[gib] = (uint32_t)s1;
        // far fields of record j, for the body stores (rare: behind a long Hop-by-Hop header)
        const bool any_far = __any(ps.ff.any());
        wave_lds_sync();
        // ---- body: shift, sum, store ----
        uint32_t acc[R];
        if constexpr (REDEAL) {
#pragma unroll
            for (int j = 0; j < R; ++j) acc[j] = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const int sj = (int)spanbuf[wv * R + j], hj = (int)hd[j];
                    const uint32_t k = (uint32_t)(64 * s + wl);
                    const bool in = k >= (uint32_t)WIN_CH && k < nb[j];
                    const u32x4 m = body_shift(v[s][j], vh[s][j], bsh[j]);
                    if (in) acc[j] = sum_chunk(m, 16 * (int)k - hj, sj, acc[j]);
                    stg[wv][j][wl] = m;
                }
                wave_lds_sync();
                // lane l stores chunks 64 s + 8 i + (l % 8) of its group's record (l / 8)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t kk = (uint32_t)(8 * i + lane), k = (uint32_t)(64 * s) + kk;
                    if (mine && k >= (uint32_t)WIN_CH && k < q.nch - 1) {
                        const u32x4 m = stg[wv][gw][kk];
                        const gu8 dst = (gu8)q.base + 16u * k;
                        const int pos = 16 * (int)k - (int)q.head;
                        if (!any_far) *(GMEM u32x4*)dst = m;
                        else store_part(dst, m, 0, 16, f0b - pos, f1b - pos, f2b - pos);
                    }
                }
                wave_lds_sync();  // the staging is rewritten by the next half-step
            }
        } else
#pragma unroll
        for (int j = 0; j < R; ++j) {
            acc[j] = 0;
            const int sj = (int)spanbuf[wv * R + j], hj = (int)hd[j];
            const uint64_t base = ((uint64_t)p.buf + (rw0 + (uint64_t)j) * p.stride) & ~15ull;
            int F0 = NOF, F1 = NOF, F2 = NOF;
            if (any_far) {  // record j's far fields, from its group's lane 0
                F0 = __shfl(f0b, G * j, 64);
                F1 = __shfl(f1b, G * j, 64);
                F2 = __shfl(f2b, G * j, 64);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t k = (uint32_t)(64 * s + wl);
                const bool in = k >= (uint32_t)WIN_CH && k < nb[j];
                const u32x4 m = body_shift(v[s][j], vh[s][j], bsh[j]);
                const int pos = 16 * (int)k - hj;
                if (in) {
                    acc[j] = sum_chunk(m, pos, sj, acc[j]);
                    const gu8 dst = (gu8)base + 16u * k;
                    if (F::NOSTORE) asm volatile("" ::"v"(m.x), "v"(m.y), "v"(m.z), "v"(m.w));
                    else if (F::NT_STORES && !any_far) __builtin_nontemporal_store(m, (GMEM u32x4*)dst);
                    else if (!any_far) *(GMEM u32x4*)dst = m;
                    else store_part(dst, m, 0, 16, F0 - pos, F1 - pos, F2 - pos);
                }
            }
        }
        // ---- reduce-scatter of the body sums, plus the group's window and edge chunks ----
        uint32_t own = 0;
        if (mine) {
            const int posw = 16 * lane - (int)q.head;
            own = sum_chunk(wm, posw, s1, 0u);
            if (lane == 0) {
                const u32x4 em = gen_merge(q, kedge, gedge);
                const int pose = 16 * (int)kedge - (int)q.head;
                own = sum_chunk(em, pose, s1, own);
                store_part((gu8)q.base + 16u * kedge, em, -pose, (int)len - pose, f0b - pose, f1b - pose,
                           f2b - pose);
            }
        }
        const uint32_t a1 = xwalk::reduce_scatter<R, 32>(acc, wl);
        // ---- finish: gates, fields into the window (or past it), then the window chunks ----
        if (mine) {
            finish_gates<G, MODE_COPY, false, ByteReader, WIN>(p, g, a1 + own, rd, winb, q.head, q.a0, r, lane,
                                                                reinterpret_cast<uint8_t*>(wn));
        }
        wave_lds_sync();
        if (mine) {
            const int posw = 16 * lane - (int)q.head;
            store_part((gu8)q.base + 16u * (uint32_t)lane, win[gib][lane], -posw, (int)len - posw, NOF, NOF, NOF);
        }
    } else if (mine && bad) {  // the copy range does not fit: record left untouched
        if (lane == 0 && p.status) ((gu8)p.status)[r] = (uint8_t)SMOL_ST_MALFORMED;
    } else if (mine) {
    // ---- generic path: group j builds every chunk of record j the window's way ----
    const Gen gwin = gen_load(q, (uint32_t)lane, lane < (int)q.nch, dummy);
    const Parsed ps =
        parse_window(wn, lane, gen_merge(q, (uint32_t)lane, gwin), (uint32_t)lane < q.nch, true, rd, len, p.kind);
    const Geom& g = ps.g;
    const int s1 = ps.s1, f0b = ps.ff.f0, f1b = ps.ff.f1, f2b = ps.ff.f2;
    uint32_t acc = 0;
    if ((uint32_t)lane < q.nch) acc = sum_chunk(win[gib][lane], 16 * lane - (int)q.head, s1, 0u);
    for (uint32_t k0 = WIN_CH; k0 < q.nch; k0 += G) {
        const uint32_t k = k0 + (uint32_t)lane;
        const bool in = k < q.nch;
        const Gen gk = gen_load(q, in ? k : 0u, in, dummy);
        const u32x4 m = gen_merge(q, k, gk);
        if (in) {
            const int pos = (int)(16u * k) - (int)q.head;
            acc = sum_chunk(m, pos, s1, acc);
            store_part((gu8)q.base + 16u * k, m, -pos, (int)len - pos, f0b - pos, f1b - pos, f2b - pos);
        }
    }
    finish_gates<G, MODE_COPY, false, ByteReader, WIN>(p, g, acc, rd, winb, q.head, q.a0, r, lane,
                                                        reinterpret_cast<uint8_t*>(wn));
    wave_lds_sync();
    if ((uint32_t)lane < q.nch) {
        const int posw = 16 * lane - (int)q.head;
        store_part((gu8)q.base + 16u * (uint32_t)lane, win[gib][lane], -posw, (int)len - posw, NOF, NOF, NOF);
    }
    }
    if (!PERSIST) break;
    wave_lds_sync();  // the windows are rewritten by the next step
    }
}

#endif  // SMOL_EXP

// A number without an XCOPY row built in this library is an error (the dispatch passes none).
hipError_t launch_xcopy(int variant, const KParams& p, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
#ifdef SMOL_EXP
    with_xcopy_form(variant, [&](auto form, auto num) {
        using F = decltype(form);
        const uint64_t per = (uint64_t)xcopy::GPB;
        note_launch(KERN_COPY, decltype(num)::value, 8, 2);
        if constexpr (F::PERSIST) {  // the workgroups resident at once
            const uint32_t cap = resident_blocks((const void*)xcopy_kernel<F>, p.num_cu ? p.num_cu : 256u,
                                                 (uint32_t)kMaxGridBlocks);
            const uint32_t b = grid_blocks((p.n + per - 1) / per, cap);
            hipLaunchKernelGGL((xcopy_kernel<F>), dim3(b), dim3(256), 0, s, p);
            e = hipGetLastError();
        } else {
            e = for_chunks(p, kMaxGridBlocks * per, [&](uint64_t, const KParams& q) {
                const uint32_t b = grid_blocks((q.n + per - 1) / per, kMaxGridBlocks);
                hipLaunchKernelGGL((xcopy_kernel<F>), dim3(b), dim3(256), 0, s, q);
                return hipGetLastError();
            });
        }
    });
#endif
    return e;
}

}  // namespace smolcsum
