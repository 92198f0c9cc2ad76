// Fused verify + payload delivery (smol_csum_batch_verify_copy): copy_kernel (csum_copy.hip) turned
// around.
//
// On receive the reference sums the whole L4 buffer in UdpRepr::parse / TcpRepr::parse
// (src/wire/udp.rs:250-257, src/wire/tcp.rs:917-919) and the socket then copies the payload out
// (src/socket/udp.rs:522-523, src/socket/tcp.rs:2231): two passes over the payload.  Here every 16-B
// chunk of a record is loaded once; the registers are summed exactly as verify sums them and the same
// registers feed the stores into the record's slot of d_dst.
//
// The record stream is csum_deliver.h's: a group of G lanes owns a record, load_step loads G * U chunks of its
// 16-B grid per step, Record::parse puts step 0's header window through parse_geometry, sum_step sums the
// chunks as verify sums them, successors / store_dest funnel-shift the same registers into the record's slot
// of d_dst (one Dest: the payload), and finish writes the status byte.  What is this file's own:
// * The payload span: UDP behind its 8-byte header up to span_end, TCP behind its data offset.
// * NT: whole chunks as non-temporal stores (ctx->vcopy_nt; measured slower).
// * The span entry (smol_csum_span_t), lane 0's.
// No byte of d_dst is read and none outside [dst_offset, dst_offset + len) is written, so slots may lie back
// to back.
// The cap is tested before the first store: a record whose payload does not fit still streams for its
// checksum and stores nothing.  The copy does not wait for the verdict (known only after the last
// byte): the caller commits a slot when the status byte has SMOL_ST_ACCEPT.
#include "csum_deliver.h"

namespace smolcsum {

template <int G, int U, bool IMPLICIT, bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void vcopy_kernel(KParams p, VCopyArgs v) {
    using namespace deliver;
    constexpr int GPB = 256 / G;
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];

    const int lane = (int)(threadIdx.x % G);
    const int gib = (int)(threadIdx.x / G);
    const uint64_t ngroups = (uint64_t)gridDim.x * GPB;
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t r = (uint64_t)blockIdx.x * GPB + gib; r < p.n; r += ngroups) {
        const Record rec(rec_at<IMPLICIT, false>(p, r), &win[gib][0], geo[gib]);
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * r);  // dst_offset, cap, reserved

        u32x4 c[U], xh;
        load_step<G, U>(rec.base, rec.nch, 0u, true, lane, dummy, c, xh);
        const int s1 = rec.parse<G, U>(c, lane);
        const Geom& g = rec.g;

        // the payload span: UdpPacket::payload (udp.rs:153-157), TcpPacket::payload (tcp.rs:419-423)
        uint32_t off = 0, plen = 0;
        bool span = false;
        if (!(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED))) {
            if (g.proto == P_UDP) {
                span = true;
                off = g.l4_off + 8;
                plen = g.span_end - off;
            } else if (g.proto == P_TCP) {
                const uint32_t thl = (rec.rd(g.l4_off + 12) >> 4) * 4;
                span = true;
                off = g.l4_off + thl;
                plen = g.l4_len - thl;
            }
        }
        const bool copied = span && plen <= sl.z;
        const bool st = copied && plen > 0;  // the cap test, before the first store
        const Dest d = dest_of(rec.rr.a0, rec.head, off, (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32)), plen);

        uint32_t acc = 0;
        for (uint32_t i0 = 0; i0 < rec.nch; i0 += (uint32_t)(G * U)) {
            if (i0) load_step<G, U>(rec.base, rec.nch, i0, st, lane, dummy, c, xh);
            acc = sum_step<G, U>(c, i0, rec, s1, lane, acc);
            if (st) store_step<G, U, NT>(c, xh, i0, rec.nch, lane, d);  // (the group's lanes together)
        }

        finish<G>(p, rec, acc, r, lane);
        if (lane == 0) {  // smol_csum_span_t: len, off, copied, reserved
            const uint64_t e = (uint64_t)plen | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)(copied ? 1u : 0u) << 48);
            *(GMEM uint64_t*)((uint64_t)v.spans + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

hipError_t launch_vcopy(int shape, bool nt, const KParams& p, const VCopyArgs& v, uint32_t max_blocks,
                        hipStream_t s) {
    return deliver::launch_shaped(KERN_VCOPY, nt ? 1 : 0, shape, p, max_blocks, [&](auto g, auto u, auto im, uint32_t blocks) {
        constexpr int G = decltype(g)::value, U = decltype(u)::value;
        constexpr bool IM = decltype(im)::value;
        if (nt) hipLaunchKernelGGL((vcopy_kernel<G, U, IM, true>), dim3(blocks), dim3(256), 0, s, p, v);
        else hipLaunchKernelGGL((vcopy_kernel<G, U, IM, false>), dim3(blocks), dim3(256), 0, s, p, v);
    });
}

}  // namespace smolcsum

