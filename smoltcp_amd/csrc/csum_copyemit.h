// The copy-emit kernels' shared per-chunk code (copy_kernel, csum_copy.hip; xcopy_kernel, csum_xcopy.hip):
// a record's copy geometry, the generic chunk build, the fields held back from the chunk stores and the
// byte reader the parse and the gates run on.  sum_chunk, store_part and body_shift, which the walk
// kernel's MODE_COPY forms use too, are in csum_walk.h.
#pragma once

#include "csum_walk.h"

namespace smolcsum {
namespace copyemit {

constexpr int WIN = 128;  // the header window: 16-B grid, Grid<false>
constexpr int WIN_CH = WIN / 16;
constexpr int NOF = -(1 << 20);  // "no field" for store_part

// One record's copy geometry: the record on its 16-B chunk grid and its payload [p0, p1) from the source.
// gen_load / gen_merge read what follows from it through pay() / sk() / first() / last(): RecGeom works them
// out where they are used (xcopy_kernel: held in registers they cost it 0.5 %), RecGeomHeld once per record
// (copy_kernel: worked out per chunk its 16 x 3 form takes 81 VGPRs instead of 80, 5 waves instead of 6).
struct RecGeom {
    uint64_t a0, base, sb;  // record start, its 16-B grid origin, source address of record offset 0
    uint32_t head, nch, p0, p1;
    // the record at a0, nch chunks on its grid, its payload [p0, p1) from sb + p0
    __device__ __forceinline__ RecGeom(uint64_t a0_, uint32_t nch_, uint64_t sb_, uint32_t p0_, uint32_t p1_)
        : a0(a0_), base(a0_ & ~15ull), sb(sb_), head((uint32_t)(a0_ & 15u)), nch(nch_), p0(p0_), p1(p1_) {}
    // whether there is a payload; the source address of grid byte 0 (payload bytes only); the first / last
    // aligned source chunks that hold payload
    __device__ __forceinline__ bool pay() const { return p1 > p0; }
    __device__ __forceinline__ uint64_t sk() const { return sb - head; }
    __device__ __forceinline__ uint64_t first() const { return (sb + p0) & ~15ull; }
    __device__ __forceinline__ uint64_t last() const { return (sb + p1 - 1) & ~15ull; }
};
struct RecGeomHeld : RecGeom {
    bool pay_;
    uint64_t sk_, first_, last_;
    __device__ __forceinline__ RecGeomHeld(uint64_t a0_, uint32_t nch_, uint64_t sb_, uint32_t p0_, uint32_t p1_)
        : RecGeom(a0_, nch_, sb_, p0_, p1_), pay_(RecGeom::pay()), sk_(RecGeom::sk()), first_(RecGeom::first()),
          last_(RecGeom::last()) {}
    __device__ __forceinline__ bool pay() const { return pay_; }
    __device__ __forceinline__ uint64_t sk() const { return sk_; }
    __device__ __forceinline__ uint64_t first() const { return first_; }
    __device__ __forceinline__ uint64_t last() const { return last_; }
};

// Chunk k of a record built the generic way: the destination chunk (unless it is all payload) and the two
// aligned source chunks under its payload bytes (clamped into the source range's aligned chunks: bytes
// outside the range are masked anyway, and no load leaves the range).  NT_DST: the destination chunk
// loaded non-temporal.
struct Gen {
    u32x4 d, c0, c1;
};
template <bool NT_DST = false, class Q>
__device__ __forceinline__ Gen gen_load(const Q& q, uint32_t k, bool in, uint64_t dummy) {
    const int pos = (int)(16u * k) - (int)q.head;
    const int lo = (int)q.p0 - pos, hi = (int)q.p1 - pos;
    const bool pay = q.pay();
    const bool full = lo <= 0 && hi >= 16;
    const bool any = pay && lo < 16 && hi > 0;
    const uint64_t sk = q.sk(), first = q.first(), last = q.last();
    Gen g;
    g.d = ld16<NT_DST>((gcv4)(in && !(pay && full) ? q.base + 16ull * k : dummy));
    const uint64_t sA = (sk + 16ull * k) & ~15ull;
    const uint64_t a0 = sA < first ? first : sA > last ? last : sA;
    const uint64_t a1 = sA + 16 < first ? first : sA + 16 > last ? last : sA + 16;
    g.c0 = ld16<false>((gcv4)(in && any ? a0 : dummy));
    g.c1 = ld16<false>((gcv4)(in && any && (sk & 15u) ? a1 : dummy));
    return g;
}
template <class Q>
__device__ __forceinline__ u32x4 gen_merge(const Q& q, uint32_t k, const Gen& g) {
    const int pos = (int)(16u * k) - (int)q.head;
    const int lo = (int)q.p0 - pos, hi = (int)q.p1 - pos;
    if (!(q.pay() && lo < 16 && hi > 0)) return g.d;
    const u32x4 s = funnel16(g.c0, g.c1, (uint32_t)(q.sk() & 15u));
    if (lo <= 0 && hi >= 16) return s;
    u32x4 m;
    const uint32_t m0 = byte_mask(lo, hi, 0), m1 = byte_mask(lo, hi, 1);
    const uint32_t m2 = byte_mask(lo, hi, 2), m3 = byte_mask(lo, hi, 3);
    m.x = (s.x & m0) | (g.d.x & ~m0);
    m.y = (s.y & m1) | (g.d.y & ~m1);
    m.z = (s.z & m2) | (g.d.z & ~m2);
    m.w = (s.w & m3) | (g.d.w & ~m3);
    return m;
}

// The fields that stay out of the chunk stores (finish_gates writes them): record offsets for store_part,
// all NOF unless one of the record's fields lies (partly) past the first `win` bytes of the chunk grid
// (behind a long IPv6 Hop-by-Hop header); then every field of the record is held back.
struct FarFields {
    int f0 = NOF, f1 = NOF, f2 = NOF;
    __device__ __forceinline__ bool any() const { return f0 != NOF || f1 != NOF || f2 != NOF; }
};
__device__ __forceinline__ FarFields far_fields(const Geom& g, uint32_t head, uint32_t win) {
    const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
    const uint32_t fip = g.fam == 4 ? g.ip_off + 10 : NO_FIELD;
    const uint32_t fl4 = l4 ? g.l4_off + g.fo : NO_FIELD;
    const uint32_t fin = g.in_off ? g.in_off + 10 : NO_FIELD;
    auto past = [&](uint32_t f) { return f != NO_FIELD && head + f + 2 > win; };
    FarFields ff;
    if (past(fip) || past(fl4) || past(fin)) {
        ff.f0 = fip != NO_FIELD ? (int)fip : NOF;
        ff.f1 = fl4 != NO_FIELD ? (int)fl4 : NOF;
        ff.f2 = fin != NO_FIELD ? (int)fin : NOF;
    }
    return ff;
}

// Record byte o: the LDS window, else global memory (payload bytes from the source).
struct ByteReader {
    const uint8_t* winb;  // the group's window
    const RecGeom& q;
    __device__ __forceinline__ uint32_t operator()(uint32_t o) const {
        const uint32_t x = q.head + o;
        if (x < (uint32_t)WIN) return (uint32_t)winb[x];
        if (o >= q.p0 && o < q.p1) return ld_byte_sync(q.sb + o);
        return ld_byte_sync(q.a0 + o);
    }
};

}  // namespace copyemit
}  // namespace smolcsum
