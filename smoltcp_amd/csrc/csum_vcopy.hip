// Fused verify + payload delivery (smol_csum_batch_verify_copy): copy_kernel (csum_copy.hip) turned
// around.
//
// On receive the reference sums the whole L4 buffer in UdpRepr::parse / TcpRepr::parse
// (src/wire/udp.rs:250-257, src/wire/tcp.rs:917-919) and the socket then copies the payload out
// (src/socket/udp.rs:522-523, src/socket/tcp.rs:2231): two passes over the payload.  Here every 16-B
// chunk of a record is loaded once; the registers are summed exactly as verify sums them and the same
// registers feed the stores into the record's slot of d_dst.
//
// A group of G lanes owns a record.  Its chunks lie on the record's own 16-B grid (origin: the record
// start rounded down to 16), G * U of them per step, all loads of a step issued first.  Step 0 holds
// the 128-B header window, which goes to LDS for parse_geometry (emit = false: verify's parse) — so a
// C2 record takes one round trip for its headers and first body chunks, then one for the rest.
// * Sum: add_words over each chunk, the record's first and last chunk masked, up to span_end; the
//   header bytes and the gates are finish_gates' (MODE_VERIFY), which also writes the status byte.
//   The destination alignment never touches the arithmetic.
// * Copy: destination chunks lie on d_dst's 16-B grid.  Chunk k of the record and its successor give
//   the destination chunk that starts at record-grid byte 16 k + sh, sh = (payload source address -
//   destination address) mod 16, through funnel16 (v_alignbyte).  The successor comes from the next
//   lane (DPP); the group's last lane takes it from its own next register, and for its last chunk of
//   a step from one extra 16-B load.  Chunks entirely inside the payload go out as one dwordx4 store
//   with the default cache policy (NT: non-temporal, measured slower); the first and
//   last chunk of a payload go out byte-masked: whole dwords as dword stores, the rest as byte
//   stores.  No byte of d_dst is read and none outside [dst_offset, dst_offset + len) is written, so
//   slots may lie back to back.
// The cap is tested before the first store: a record whose payload does not fit still streams for its
// checksum and stores nothing.  The copy does not wait for the verdict (known only after the last
// byte): the caller commits a slot when the status byte has SMOL_ST_ACCEPT.
#include "csum_walk.h"

namespace smolcsum {

namespace vcopy {

constexpr int WIN = 128;  // the header window: 16-B grid, Grid<false>
constexpr int WIN_CH = WIN / 16;
// next4, sum_chunk, store_edge: csum_walk.h (shared with csum_fragcopy.hip)

}  // namespace vcopy

template <int G, int U, bool IMPLICIT, bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void vcopy_kernel(KParams p, VCopyArgs v) {
    using namespace vcopy;
    constexpr int GPB = 256 / G;
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    static_assert(G * U >= WIN_CH, "step 0 holds the window");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];

    const int lane = (int)(threadIdx.x % G);
    const int gib = (int)(threadIdx.x / G);
    const uint64_t ngroups = (uint64_t)gridDim.x * GPB;
    u32x4* wn = &win[gib][0];
    const uint8_t* winb = reinterpret_cast<const uint8_t*>(wn);
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t r = (uint64_t)blockIdx.x * GPB + gib; r < p.n; r += ngroups) {
        const RecRef rr = rec_at<IMPLICIT, false>(p, r);
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * r);  // dst_offset, cap, reserved
        const uint64_t base = rr.a0 & ~15ull;
        const uint32_t head = (uint32_t)(rr.a0 - base);
        const uint32_t nch = n_chunks<false>(rr);

        // one step: chunks [i0, i0 + G * U), and for the group's last lane the chunk after them
        u32x4 c[U], xh;
        auto load = [&](uint32_t i0, bool next) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                c[u] = ld16<false>((gcv4)(k < nch ? base + 16ull * k : dummy));
            }
            const uint32_t kx = i0 + (uint32_t)(U * G);
            xh = ld16<false>((gcv4)(next && lane == G - 1 && kx < nch ? base + 16ull * kx : dummy));
        };
        load(0u, true);
#pragma unroll
        for (int u = 0; u * G < WIN_CH; ++u) {
            const uint32_t k = (uint32_t)(u * G + lane);
            if (k < (uint32_t)WIN_CH && k < nch) wn[k] = c[u];
        }
        wave_lds_sync();
        // record byte o: the LDS window, else global memory (behind a long Hop-by-Hop header)
        auto rd = [&](uint32_t o) -> uint32_t {
            const uint32_t x = head + o;
            if (x < (uint32_t)WIN) return (uint32_t)winb[x];
            return ld_byte_sync(rr.a0 + o);
        };
        {
            const Geom g0 = parse_geometry<false>(rd, rr.len, rr.kind, false);
            if (lane == 0) geo[gib] = g0;
        }
        wave_lds_sync();
        const Geom& g = geo[gib];
        const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
        const int s1 = l4 ? (int)g.span_end : 0;

        // the payload span: UdpPacket::payload (udp.rs:153-157), TcpPacket::payload (tcp.rs:419-423)
        uint32_t off = 0, plen = 0;
        bool span = false;
        if (!(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED))) {
            if (g.proto == P_UDP) {
                span = true;
                off = g.l4_off + 8;
                plen = g.span_end - off;
            } else if (g.proto == P_TCP) {
                const uint32_t thl = (rd(g.l4_off + 12) >> 4) * 4;
                span = true;
                off = g.l4_off + thl;
                plen = g.l4_len - thl;
            }
        }
        const bool copied = span && plen <= sl.z;
        const bool st = copied && plen > 0;  // the cap test, before the first store
        const uint64_t D = (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32));
        const uint32_t sh = (uint32_t)((rr.a0 + off - D) & 15u);
        // destination chunk of record chunk k: payload-relative position 16 k + dk0
        const int dk0 = (int)sh - (int)head - (int)off;

        uint32_t acc = 0;
        for (uint32_t i0 = 0; i0 < nch; i0 += (uint32_t)(G * U)) {
            if (i0) load(i0, st);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                if (k < nch) acc = sum_chunk(c[u], (int)(16u * k) - (int)head, s1, acc);
            }
            if (st) {  // (the group's lanes together: the exchange below needs all of them)
                u32x4 ncur = next4<G>(c[0], lane);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const u32x4 nnext = u + 1 < U ? next4<G>(c[u + 1 < U ? u + 1 : u], lane) : xh;
                    const u32x4 hi = lane == G - 1 ? nnext : ncur;
                    ncur = nnext;
                    const uint32_t k = i0 + (uint32_t)(u * G + lane);
                    const int pos = (int)(16u * k) + dk0;
                    const int lo = -pos, end = (int)plen - pos;
                    if (k < nch && end > 0 && lo < 16) {
                        const u32x4 m = funnel16(c[u], hi, sh);
                        const gu8 dst = (gu8)(D + (uint64_t)(int64_t)pos);
                        if (lo <= 0 && end >= 16) {
                            if constexpr (NT) __builtin_nontemporal_store(m, (GMEM u32x4*)dst);
                            else *(GMEM u32x4*)dst = m;
                        } else {
                            store_edge(dst, m, lo, end);
                        }
                    }
                }
            }
        }

        finish_gates<G, MODE_VERIFY, false, decltype(rd)>(p, g, acc, rd, winb, head, rr.a0, r, lane);
        if (lane == 0) {  // smol_csum_span_t: len, off, copied, reserved
            const uint64_t e = (uint64_t)plen | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)(copied ? 1u : 0u) << 48);
            *(GMEM uint64_t*)((uint64_t)v.spans + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

template <bool IMPLICIT, bool NT, int G, int U>
hipError_t launch_vcopy_one(const KParams& p, const VCopyArgs& v, uint32_t max_blocks, hipStream_t s) {
    constexpr uint32_t GPB = 256 / G;
    const uint64_t want = (p.n + GPB - 1) / GPB;
    const uint32_t blocks = grid_blocks(want, max_blocks);
    note_launch(KERN_VCOPY, NT ? 1 : 0, G, U);
    hipLaunchKernelGGL((vcopy_kernel<G, U, IMPLICIT, NT>), dim3(blocks), dim3(256), 0, s, p, v);
    return hipGetLastError();
}

// Shapes: the whole-segment set of the shape mapper (8 x 6, 8 x 7, 16 x 3, 16 x 4, 32 x 4, 64 x 4).
hipError_t launch_vcopy(int shape, bool nt, const KParams& p, const VCopyArgs& v, uint32_t max_blocks,
                        hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    const bool im = p.desc == nullptr;
    with_walk_shape<S_SEG6>(shape, [&](auto g, auto u) {
        constexpr int G = decltype(g)::value, U = decltype(u)::value;
        if (nt)
            e = im ? launch_vcopy_one<true, true, G, U>(p, v, max_blocks, s)
                   : launch_vcopy_one<false, true, G, U>(p, v, max_blocks, s);
        else
            e = im ? launch_vcopy_one<true, false, G, U>(p, v, max_blocks, s)
                   : launch_vcopy_one<false, false, G, U>(p, v, max_blocks, s);
    });
    return e;
}

}  // namespace smolcsum
