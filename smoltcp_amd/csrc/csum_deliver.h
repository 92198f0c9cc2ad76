// The sum-and-deliver kernels' record stream: one front end and one chunk-store back end for the receive calls
// that load a record once, sum it as verify sums it and store the same registers somewhere else
// (csum_vcopy.hip, csum_echo.hip, csum_unreach.hip with a group of G lanes per record; csum_tcpasm.hip and
// csum_udprx.hip with a 64-lane wave per record).
//
// A group of G lanes owns a record.  Its chunks lie on the record's own 16-B grid (origin: the record start
// rounded down to 16), G * U of them per step, all loads of a step issued first (load_step).  Step 0 holds the
// 128-B header window, which goes to LDS for parse_geometry (emit = false: verify's parse): Record::parse.
// * Sum: add_words over each chunk, the record's first and last chunk masked (sum_step; sum_range where a
//   kernel keeps two accumulators).  The header bytes and the gates are finish_gates' (MODE_VERIFY), which also
//   writes the status byte: finish.  The destination alignment never touches the arithmetic.
// * Copy: destination chunks lie on the destination's 16-B grid.  Chunk k of the record and its successor give
//   the destination chunk that starts at record-grid byte 16 k + sh, sh = (source address - destination address)
//   mod 16, through funnel16 (v_alignbyte).  The successor comes from the next lane (DPP); the group's last lane
//   takes it from its own next register, and for its last chunk of a step from one extra 16-B load (successors).
//   Chunks entirely inside the range go out as one dwordx4 store, its first and last chunk byte-masked: whole
//   dwords as dword stores, the rest as byte stores (store_dest).  No byte of the destination is read and none
//   outside [D, D + n) is written, so ranges may lie back to back.
// * Head: a reply's head, [D, D + hl) at any alignment, built byte by byte and stored byte-masked (store_head).
// next4, sum_chunk, store_edge and store_dword_masked are csum_walk.h's (shared with the piece streamer).
#pragma once
#include "csum_walk.h"

namespace smolcsum {
namespace deliver {

constexpr int WIN = 128;  // the header window: 16-B grid, Grid<false>
constexpr int WIN_CH = WIN / 16;

// One step's loads: chunks [i0, i0 + G * U), and for the group's last lane the chunk after them (xh; next: the
// step's chunks are stored, so its last one needs its successor).  All of them issued unconditionally; what does
// not exist reads the dummy line.  xh is issued FIRST, as piece_load issues it (csum_walk.h: with xh last the
// wait in front of the exchange drains every load behind it too).  XH_FIRST = false issues it last: echo_kernel
// and unreach_kernel, whose short records measured better that way.
template <int G, int U, bool XH_FIRST = true>
__device__ __forceinline__ void load_step(uint64_t base, uint32_t nch, uint32_t i0, bool next, int lane, uint64_t dummy,
                                          u32x4 (&c)[U], u32x4& xh) {
    const uint32_t kx = i0 + (uint32_t)(G * U);
    const gcv4 qx = (gcv4)(next && lane == G - 1 && kx < nch ? base + 16ull * kx : dummy);
    if constexpr (XH_FIRST) xh = ld16<false>(qx);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t k = i0 + (uint32_t)(u * G + lane);
        c[u] = ld16<false>((gcv4)(k < nch ? base + 16ull * k : dummy));
    }
    if constexpr (!XH_FIRST) xh = ld16<false>(qx);
}

// A record under its group: where its chunks lie, the group's LDS window and its geometry slot.  Also the byte
// reader parse_geometry and finish_gates run on.
struct Record {
    RecRef rr;
    uint64_t base;  // chunk-grid origin: the record start rounded down to 16
    uint32_t head;  // record start - base
    uint32_t nch;   // chunks that hold a byte of the record
    u32x4* wn;      // the group's window: step 0's first WIN_CH chunks
    const uint8_t* winb;
    Geom& g;        // the group's slot, filled by parse

    __device__ __forceinline__ Record(const RecRef& rr_, u32x4* wn_, Geom& slot)
        : rr(rr_), base(rr_.a0 & ~15ull), head((uint32_t)(rr_.a0 - base)), nch(n_chunks<false>(rr_)), wn(wn_),
          winb(reinterpret_cast<const uint8_t*>(wn_)), g(slot) {}

    // record byte o: the LDS window, else global memory (behind a long Hop-by-Hop header)
    __device__ __forceinline__ uint32_t rd(uint32_t o) const {
        const uint32_t x = head + o;
        if (x < (uint32_t)WIN) return (uint32_t)winb[x];
        return ld_byte_sync(rr.a0 + o);
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t o) const { return rd(o); }

    // The front end, after load_step(.., 0, ..): step 0's window to LDS, the parse (lane 0 writes the slot), and
    // the end of the span verify sums, [0, s1) (0: it sums nothing of the record).
    template <int G, int U>
    __device__ __forceinline__ int parse(const u32x4 (&c)[U], int lane) const {
        static_assert(G * U >= WIN_CH, "step 0 holds the window");
#pragma unroll
        for (int u = 0; u * G < WIN_CH; ++u) {
            const uint32_t k = (uint32_t)(u * G + lane);
            if (k < (uint32_t)WIN_CH && k < nch) wn[k] = c[u];
        }
        wave_lds_sync();
        {
            const Geom g0 = parse_geometry<false>(*this, rr.len, rr.kind, false);
            if (lane == 0) g = g0;
        }
        wave_lds_sync();
        const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
        return l4 ? (int)g.span_end : 0;
    }
};

// The verdict of record r from the lanes' sums over [0, s1): finish_gates' header bytes, gates and status byte
// (st_out: lane 0 also leaves the status byte there).
template <int G>
__device__ __forceinline__ void finish(const KParams& p, const Record& rec, uint32_t acc, uint64_t r, int lane,
                                       uint32_t* st_out = nullptr) {
    finish_gates<G, MODE_VERIFY, false, Record>(p, rec.g, acc, rec, rec.winb, rec.head, rec.rr.a0, r, lane, nullptr, ~0ull,
                                                ~0ull, 0, nullptr, st_out);
}

// Aligned-word sum of the chunk's bytes inside the record range [lo, hi) (pos: chunk start relative to the
// record start): sum_chunk with a lower bound.
__device__ __forceinline__ uint32_t sum_range(const u32x4& c, int pos, int lo, int hi, uint32_t acc) {
    if (pos >= hi || pos + 16 <= lo) return acc;
    if (pos < lo || pos + 16 > hi) return sum_masked_words(c, lo - pos, hi - pos, acc);
    return add_words(c.x, add_words(c.y, add_words(c.z, add_words(c.w, acc))));
}

// One step's chunks summed into acc as verify sums them: the record's span [0, s1).
template <int G, int U>
__device__ __forceinline__ uint32_t sum_step(const u32x4 (&c)[U], uint32_t i0, const Record& rec, int s1, int lane,
                                             uint32_t acc) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t k = i0 + (uint32_t)(u * G + lane);
        if (k < rec.nch) acc = sum_chunk(c[u], (int)(16u * k) - (int)rec.head, s1, acc);
    }
    return acc;
}

// One contiguous destination range of a record: n bytes from record offset rec_off to address D.
// Destination chunk of record chunk k: range-relative position 16 k + dk0.
struct Dest {
    uint64_t D;
    uint32_t n, sh;
    int dk0;
};
__device__ __forceinline__ Dest dest_of(uint64_t a0, uint32_t head, uint32_t rec_off, uint64_t D, uint32_t n) {
    Dest d;
    d.D = D;
    d.n = n;
    d.sh = (uint32_t)((a0 + rec_off - D) & 15u);
    d.dk0 = (int)d.sh - (int)head - (int)rec_off;
    return d;
}

// Destination chunk k of range d, from record chunk k (c) and its successor (hi): a chunk entirely inside the
// range as one dwordx4 store (NT: non-temporal), the range's first and last chunk byte-masked (store_edge).
// An empty range stores nothing (tcpasm's second ring piece).
template <bool NT>
__device__ __forceinline__ void store_chunk(const Dest& d, const u32x4& c, const u32x4& hi, uint32_t k, uint32_t nch) {
    const int pos = (int)(16u * k) + d.dk0;
    const int lo = -pos, end = (int)d.n - pos;
    if (d.n != 0 && k < nch && end > 0 && lo < 16) {
        const u32x4 m = funnel16(c, hi, d.sh);
        const gu8 dst = (gu8)(d.D + (uint64_t)(int64_t)pos);
        if (lo <= 0 && end >= 16) {
            if constexpr (NT) __builtin_nontemporal_store(m, (GMEM u32x4*)dst);
            else *(GMEM u32x4*)dst = m;
        } else {
            vcopy::store_edge(dst, m, lo, end);
        }
    }
}

// One step's stores into the ranges dest...: each chunk's successor comes from the next lane, for the group's
// last lane from its own next register or xh (the group's lanes together: the exchange needs all of them).
// A successor is made where it is used: held for the whole step (U x 4 registers) the 8 x 6 and 8 x 7 shapes
// of verify_copy spilled 24 to 52 bytes more.
template <int G, int U, bool NT = false, class... DEST>
__device__ __forceinline__ void store_step(const u32x4 (&c)[U], const u32x4& xh, uint32_t i0, uint32_t nch, int lane,
                                           const DEST&... dest) {
    u32x4 ncur = vcopy::next4<G>(c[0], lane);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u32x4 nnext = u + 1 < U ? vcopy::next4<G>(c[u + 1 < U ? u + 1 : u], lane) : xh;
        const u32x4 hi = lane == G - 1 ? nnext : ncur;
        ncur = nnext;
        (store_chunk<NT>(dest, c[u], hi, i0 + (uint32_t)(u * G + lane), nch), ...);
    }
}

// A frame's head, [D, D + hl): lane j builds the aligned dwords j, j + G, .. of the range from byte(i), head
// byte i with its checksum fields already patched, and stores each byte-masked, so no byte of the destination
// is read and none outside the range is written.
template <int G, class BYTE>
__device__ __forceinline__ void store_head(uint64_t D, uint32_t hl, int lane, const BYTE& byte) {
    const uint32_t a = (uint32_t)(D & 3u);
    const uint32_t ndw = (a + hl + 3u) / 4u;
    for (uint32_t j = lane; j < ndw; j += G) {
        uint32_t w = 0, keep = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t i = 4u * j + b - a;  // head byte (wraps below 0: >= hl)
            if (i < hl) {
                w |= byte(i) << (8u * b);
                keep |= 0xffu << (8u * b);
            }
        }
        store_dword_masked((gu8)(D - a + 4ull * j), w, keep);
    }
}

// The launch of a kernel built for the whole-segment shape set (8 x 6, 8 x 7, 16 x 3, 16 x 4, 32 x 4, 64 x 4),
// one group of G lanes per record: launch(G, U, IMPLICIT, blocks) launches the instantiation.
template <class LAUNCH>
hipError_t launch_shaped(uint32_t kern, uint32_t variant, int shape, const KParams& p, uint32_t max_blocks, const LAUNCH& launch) {
    hipError_t e = hipErrorInvalidValue;
    with_walk_shape<S_SEG6>(shape, [&](auto g, auto u) {
        constexpr uint32_t GPB = 256 / decltype(g)::value;
        const uint32_t blocks = grid_blocks((p.n + GPB - 1) / GPB, max_blocks);
        note_launch(kern, variant, decltype(g)::value, decltype(u)::value);
        if (p.desc == nullptr) launch(g, u, std::true_type{}, blocks);
        else launch(g, u, std::false_type{}, blocks);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace deliver
}  // namespace smolcsum
