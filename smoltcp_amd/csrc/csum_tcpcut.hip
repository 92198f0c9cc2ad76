// Emit + TCP segmentation of whole sends (smol_csum_batch_tcp_segment_emit, include/smolcsum.h): the TCP
// counterpart of csum_fragcut.hip.  Each record is one header template (Ethernet header if any, IPv4 or
// IPv6 header, TCP header with its options, no payload); its plan names a payload range of d_src and an
// MSS.  The frames (the template with sequence number, IP length, FIN / PSH and both checksums rewritten,
// then a slice of the payload) are written to the send's place in d_dst, in one pass over the payload.
//
// In the reference such a burst is repeated TcpSocket::dispatch calls within one poll: each takes
// tx_buffer.get_allocated(offset, size) with size <= effective_mss (src/socket/tcp.rs:2620-2673), sets PSH
// or FIN only when the segment reaches the end of the buffer (tcp.rs:2675-2687), TcpRepr::emit copies the
// payload and fill_checksum sums it (src/wire/tcp.rs:1087-1095, 616-626), behind Ipv4Repr::emit
// (src/wire/ipv4.rs:584-611) or Ipv6Repr::emit (src/wire/ipv6.rs:628-640).  Here every 16-B chunk of the
// payload is loaded once: the registers are summed and the same registers feed the stores.
//
// One wavefront per send, four sends per 256-thread workgroup; no LDS, no barrier.  The record gate, the
// cap / stride test, the result entry and the launcher are csum_cut.h's, shared with csum_fragcut.hip.
//   1. Gate.  The wave parses the template with parse_geometry (cut::gate): the status byte is emit's by
//      construction.  The cut rules of the header (TCP straight behind a plain IP header, no payload of
//      its own, SYN and RST clear, mss >= 1, the IP length field fits) and the cut (count, frame lengths:
//      a cut::Cut) are written here, the cap / stride test (cut::place) follows; a send that is not cut
//      or does not fit streams nothing and stores nothing.
//   2. Once per send.  Lane i < hl / 2 holds big-endian word i of the head (hl is even: io is 0 or 14, the
//      headers are multiples of 4).  Two wave reductions over those lanes give what no frame changes: the
//      TCP sum's constant part (the pseudo-header's addresses and protocol, every TCP header word but the
//      sequence number, the flags word and the checksum) and the IPv4 header's (every word but total
//      length and checksum).
//   3. Per frame (vcopy::piece_walk, csum_walk.h: fragcopy's and fragcut's pipeline).  The payload slice is
//      streamed as a vcopy::Piece, cut::U chunks per lane and step, all loads of a step issued first, and
//      the first step of the NEXT frame is issued before the current one is used.  Nothing is held back
//      (vcopy::NoHold): the checksum field lies in the head, not in the stream.  The frame's payload sum is its own: it is
//      reduced across the wave once the slice is streamed; the lanes sum aligned little-endian words, so
//      for a slice at an even source address the folded sum is byte-swapped into the header's big-endian
//      words, at an odd one it already is (RFC 1071 2(B)) -- an odd mss makes every second slice odd.
//      Then the head: every lane computes both checksums from the constant parts, the sequence words, the
//      flags word and the lengths, substitutes its word if it is one of the rewritten ones, and stores it
//      (one 2-byte store per lane where the frame starts even, two byte stores where it starts odd: the
//      lanes' stores are consecutive either way).
//   4. Result.  Lane 0 writes the 16-byte entry (cut::store_result), also for a send that is not cut.
// Stores and cache policy are fragcut's: plain loads and stores, dwordx4 inside a slice, byte-masked edges,
// nothing read back from d_dst.  The one departure: the head goes out after its frame's slice, not
// before, because it carries the frame's own checksum.
#include "csum_cut.h"

namespace smolcsum {
namespace tcpcut {

using cut::Frame;  // (all of the slice is summed)

template <bool IMPLICIT>
__global__ __launch_bounds__(256) void tcpcut_kernel(KParams p, TcpCutArgs v) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t dummy = (uint64_t)p.dummy;
    const uint64_t nwaves = 4ull * gridDim.x;

    for (uint64_t r = 4ull * blockIdx.x + wave; r < p.n; r += nwaves) {
        // ---- 1. the gate: emit's parse, the cut rules, the cut, the cap ----
        const cut::Gate gt = cut::gate<IMPLICIT>(p, r);
        const uint64_t a0 = gt.rd.a0;
        const Geom g = gt.g;
        const u32x4 pa = *(gcv4)((uint64_t)v.plans + 32ull * r);       // src_offset, len, mss | reserved << 16
        const u32x4 pb = *(gcv4)((uint64_t)v.plans + 32ull * r + 16);  // dst_offset, cap, reserved2
        const uint32_t len = pa.z, mss = pa.w & 0xffffu, cap = pb.z;
        const uint32_t io = g.ip_off, l4o = g.l4_off;
        const uint64_t tcp = a0 + l4o;
        // cut: a TCP header that passed check_len straight behind an IPv4 header of IHL 5 or an IPv6 header
        // (no Hop-by-Hop header), nothing behind it, SYN and RST clear, and an IP length field that fits
        bool is_cut = g.st == 0 && g.proto == P_TCP && mss >= 1 &&
                      ((g.fam == 4 && g.ip_hl == 20) || (g.fam == 6 && l4o == io + 40));
        uint32_t thl = 20, seq0 = 0, fl0 = 0;
        if (is_cut) {
            fl0 = rb16(tcp + 12);
            thl = (fl0 >> 12) * 4;
            seq0 = (rb16(tcp + 4) << 16) | rb16(tcp + 6);
            is_cut = g.l4_len == thl && (fl0 & 0x06u) == 0;
        }
        const uint32_t p0 = min(mss, len);  // payload bytes of every frame but the last
        const uint32_t iplen0 = (g.fam == 4 ? 20u : 0u) + thl;  // the IP length field of a bare segment
        is_cut = is_cut && iplen0 + p0 <= 65535u;
        const uint32_t hl = l4o + thl;
        cut::Cut ct = {0u, 0u, 0u};
        if (is_cut) {
            ct.count = len ? (uint32_t)(((uint64_t)len + mss - 1) / mss) : 1u;
            ct.frame_len = hl + p0;
            ct.last_len = hl + (len - (ct.count - 1) * mss);
        }
        const cut::Place at = cut::place(ct, v.frame_stride, cap);  // before the first store
        const uint32_t count = ct.count, S = at.S;

        if (at.fits) {
            const uint64_t Sbase = (uint64_t)v.src + ((uint64_t)pa.x | ((uint64_t)pa.y << 32));
            const uint64_t Dbase = (uint64_t)v.dst + ((uint64_t)pb.x | ((uint64_t)pb.y << 32));
            // ---- 2. the head: this lane's word of the template, and what no frame changes ----
            const uint32_t nw = hl / 2;                       // head words, <= 57
            const bool mine = (uint32_t)lane < nw;
            const uint32_t hw = mine ? rb16(a0 + 2u * (uint32_t)lane) : 0u;
            const int iw = lane - (int)(io / 2);              // word index in the IP header
            const int tw = lane - (int)(l4o / 2);             // word index in the TCP header
            const bool v4 = g.fam == 4;
            const bool addr = v4 ? (iw >= 6 && iw < 10) : (iw >= 4 && iw < 20);
            const bool tconst = mine && tw >= 0 && tw != 2 && tw != 3 && tw != 6 && tw != 8;
            const uint32_t TC = group_sum<64>(addr || tconst ? hw : 0u) + P_TCP;
            const uint32_t HC = v4 ? group_sum<64>(iw >= 0 && iw < 10 && iw != 1 && iw != 5 ? hw : 0u) : 0u;
            const bool tcp_tx = caps_tx(p.caps_tcp), ip_tx = caps_tx(p.caps_ipv4);

            auto setup = [&](uint32_t k) -> Frame {
                Frame f;
                const uint64_t lo = (uint64_t)k * mss;
                const uint32_t pk = (uint32_t)min((uint64_t)mss, (uint64_t)len - lo);
                f.F = Dbase + (uint64_t)k * S;
                f.q = vcopy::Piece<false>(Sbase + lo, f.F + hl, pk, pk);
                return f;
            };
            // the hl header bytes of frame k, one word per lane; pay: the big-endian word sum of its payload
            auto head = [&](const Frame& f, uint32_t k, uint32_t pay) {
                const uint32_t pk = f.q.copy_len;
                const uint32_t seq = seq0 + k * mss;
                const uint32_t flk = k + 1 < count ? (fl0 & ~0x09u) : fl0;  // FIN, PSH: on the last frame only
                const uint32_t ipl = iplen0 + pk;
                const uint32_t tcs = tcp_tx ? (~fold32(TC + (seq >> 16) + (seq & 0xffffu) + flk + thl + pk + pay) & 0xffffu) : 0u;
                const uint32_t ics = ip_tx ? (~fold32(HC + ipl) & 0xffffu) : 0u;
                uint32_t w = hw;
                w = tw == 2 ? seq >> 16 : tw == 3 ? seq & 0xffffu : tw == 6 ? flk : tw == 8 ? tcs : w;
                if (v4) w = iw == 1 ? ipl : iw == 5 ? ics : w;
                else w = iw == 2 ? ipl : w;
                if (mine) store_be16((gu8)(f.F + 2u * (uint32_t)lane), w);
            };

            vcopy::piece_walk<cut::U>(count, lane, dummy, setup, cut::SliceOf{}, [&](const Frame& f, uint32_t k, auto stream) {
                uint32_t acc = 0;  // this lane's part of the aligned-word sum over the frame's payload
                stream(acc, vcopy::NoHold{});
                // (a lane sums at most 65 chunks of a 65535-B slice: no wrap; folded before the wave's sum)
                const uint32_t le = fold32(group_sum<64>(fold32(acc)));
                head(f, k, f.q.odd() ? le : bswap16(le));
            });
        }
        cut::store_result(v.out, r, lane, ct, g.st, at.fits);
    }
}

}  // namespace tcpcut

hipError_t launch_tcpcut(const KParams& p, const TcpCutArgs& v, hipStream_t s) {
    return cut::launch(KERN_TCPCUT, tcpcut::tcpcut_kernel<true>, tcpcut::tcpcut_kernel<false>, p, v, s);
}

}  // namespace smolcsum
