// The cut kernels' back end: what fragcut_kernel (csum_fragcut.hip) and tcpcut_kernel (csum_tcpcut.hip) must
// agree on, written once: the record gate, the cap / stride rule, the 16-byte result entry, the frame base
// and the launcher (one record per wavefront, four per workgroup).  A kernel file says which records it
// cuts and how, what a frame's head holds and what its slice sums to.
#pragma once

#include "csum_walk.h"

namespace smolcsum {
namespace cut {

constexpr int U = 2;  // chunks per lane and step: a 1480-B or 1460-B slice is one step

// The record's bytes, by record offset.
struct Rd {
    uint64_t a0;  // absolute address of the record's first byte
    __device__ __forceinline__ uint32_t operator()(uint32_t o) const { return rb(a0 + o); }
};

// Record r as emit sees it (parse_geometry, csum_device.h, the emit flavour): the status byte, the L4 span
// and the offsets of the fields emit writes are emit's by construction.
struct Gate {
    Rd rd;
    Geom g;
};
template <bool IMPLICIT>
__device__ __forceinline__ Gate gate(const KParams& p, uint64_t r) {
    const RecRef rr = rec_at<IMPLICIT, false>(p, r);
    Gate t;
    t.rd = Rd{rr.a0};
    t.g = parse_geometry<false>(t.rd, rr.len, rr.kind, true);
    return t;
}

// What a record is cut into: count frames, all of frame_len bytes but the last (last_len).  All 0: not cut.
struct Cut {
    uint32_t count, frame_len, last_len;
};
// Where the frames go: S bytes from one frame to the next (the call's frame_stride, 0: back to back), and
// whether the record is cut, its frames lie inside its cap and do not overlap.
struct Place {
    uint32_t S;
    bool fits;
};
__device__ __forceinline__ Place place(const Cut& c, uint32_t frame_stride, uint32_t cap) {
    const uint32_t S = frame_stride ? frame_stride : c.frame_len;
    return {S, c.count != 0 && (uint64_t)(c.count - 1) * S + c.last_len <= cap && S >= c.frame_len};
}

// smol_csum_fragout_t / smol_csum_tcpout_t: count, frame_len, last_len, status | written << 8.
__device__ __forceinline__ void store_result(void* out, uint64_t r, int lane, const Cut& c, uint32_t st, bool written) {
    if (lane == 0) {
        const u32x4 o = {c.count, c.frame_len, c.last_len, (st & 0xffu) | (written ? 0x100u : 0u)};
        *(GMEM u32x4*)((uint64_t)out + 16ull * r) = o;
    }
}

// One frame: its payload slice (the same for every lane of the wave) and where the frame starts.  A kernel
// derives from it what its frame head needs besides.
struct Frame {
    vcopy::Piece<false> q;  // the slice: all of it delivered
    uint64_t F;             // destination address of the frame's first byte
};
// piece_walk's view of a frame.
struct SliceOf {
    __device__ __forceinline__ const vcopy::Piece<false>& operator()(const Frame& f) const { return f.q; }
};

// One wavefront per record, the fixed-stride or the descriptor instantiation of the kernel.
template <class ARGS>
inline hipError_t launch(uint32_t kern, void (*fixed)(KParams, ARGS), void (*desc)(KParams, ARGS), const KParams& p,
                         const ARGS& v, hipStream_t s) {
    const uint32_t blocks = grid_blocks((p.n + 3) / 4, kMaxGridBlocks);
    note_launch(kern, 0, 64, U);
    hipLaunchKernelGGL(p.desc == nullptr ? fixed : desc, dim3(blocks), dim3(256), 0, s, p, v);
    return hipGetLastError();
}

}  // namespace cut
}  // namespace smolcsum
