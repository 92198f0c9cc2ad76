// Fused verify + ICMP echo responder (smol_csum_batch_verify_echo_reply): vcopy_kernel (csum_vcopy.hip)
// with a second sum and a fresh head.
//
// The reference's responder parses an echo request (Icmpv4Repr::parse / Icmpv6Repr::parse sum the whole
// message, src/iface/interface/ipv4.rs:320-371, ipv6.rs:399-416), builds an EchoReply around the same data
// and, on dispatch, copies the data (icmpv4.rs:506-517, icmpv6.rs:814-822) and sums it again (fill_checksum):
// two reads, one write and two sums over bytes that differ in the type byte and the checksum field.  Here
// every 16-B chunk of a record is loaded once.
//
// The record stream is csum_deliver.h's (load_step, Record::parse, store_step, finish): a group of G lanes owns
// a record, and the data goes to its place behind the reply's head as one Dest.  What is this file's own:
// * Two sums.  Each lane keeps two accumulators: the record bytes in front of the echo data, [0, data_off),
//   and the data, [data_off, span_end).  Their sum is verify's accumulator and goes to finish_gates
//   (MODE_VERIFY) unchanged, which writes the status byte.  The data's accumulator alone, with the reply's
//   own first words (type / code, a zero checksum, ident, sequence number; ICMPv6: the pseudo-header over
//   the swapped addresses and the reply's length) added, gives the reply's checksum: nothing is subtracted
//   from a folded sum, so 0x0000 and 0xffff stay apart and the value is fill_checksum's.  Each lane folds
//   its partial sum to the big-endian form before the group's reduction (one group_sum more than verify).
// * Head.  The rule (answered or not, the head's bytes with zero checksum fields) is csum_echo.h's, read
//   from the LDS window.  After the reduction every lane holds both checksums and patches them into the
//   bytes it hands to store_head, so no byte of d_dst is read and none outside the frame is written.
// * Entry.  Lane 0 writes the record's 8-byte smol_csum_echo_t; SEND comes from the status byte
//   finish_gates hands back.
// The cap is tested before the first store.  The copy does not wait for the verdict.
#include "csum_deliver.h"
#include "csum_echo.h"

namespace smolcsum {

namespace echo {

// load_step's extra load is issued last here, as before the stream was shared: issued first the 98-B and
// 1294-B shapes took 0.5 and 1.8 % longer than the separate text, issued last 0.2 and 0.4 %.
constexpr bool XH_FIRST = false;

// The request as csum_echo.h reads it: addresses and MACs from the LDS window (record byte o at w[o]; all
// of them lie in front of byte 54), the message's bytes 4..7 in a register (they may lie past the window).
struct WinReq {
    const uint8_t* w;
    uint32_t kind_, ver_, ip_, dlen_, idseq_;
    __device__ __forceinline__ uint32_t kind() const { return kind_; }
    __device__ __forceinline__ uint32_t ver() const { return ver_; }
    __device__ __forceinline__ uint32_t dlen() const { return dlen_; }
    __device__ __forceinline__ uint32_t mac_dst(uint32_t j) const { return w[j]; }
    __device__ __forceinline__ uint32_t mac_src(uint32_t j) const { return w[6 + j]; }
    __device__ __forceinline__ uint32_t ethertype(uint32_t j) const { return w[12 + j]; }
    __device__ __forceinline__ uint32_t src(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 12u : 8u) + j]; }
    __device__ __forceinline__ uint32_t dst(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 16u : 24u) + j]; }
    __device__ __forceinline__ uint32_t idseq(uint32_t j) const { return (idseq_ >> (24u - 8u * j)) & 0xffu; }
};

}  // namespace echo

template <int G, int U, bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void echo_kernel(KParams p, EchoArgs v) {
    using namespace deliver;
    using namespace echo;
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
        const RecRef& rr = rec.rr;
        const uint8_t* winb = rec.winb;
        const uint32_t head = rec.head, nch = rec.nch;
        const u32x4 sl = *(gcv4)((uint64_t)v.slots + 16ull * r);  // dst_offset, cap, reserved

        u32x4 c[U], xh;
        load_step<G, U, XH_FIRST>(rec.base, nch, 0u, true, lane, dummy, c, xh);
        const int s1 = rec.parse<G, U>(c, lane);
        const Geom& g = rec.g;

        // the request (Icmpv4Repr::parse icmpv4.rs:410, Icmpv6Repr::parse icmpv6.rs:689), the address rule
        // and the reply's geometry
        // (built where it is used, before and after the stream, so that nothing of it stays in registers)
        auto request = [&](uint32_t dlen, uint32_t idseq) { return WinReq{winb + head, rr.kind & 0xffu, g.fam, g.ip_off, dlen, idseq}; };
        uint32_t fl = 0, off = 0, plen = 0, hl = 0;
        if (!(g.st & (SMOL_ST_MALFORMED | SMOL_ST_UNSUPPORTED)) && (g.proto == P_ICMP4 || g.proto == P_ICMP6)) {
            const uint32_t t = rec.rd(g.l4_off), code = rec.rd(g.l4_off + 1);
            if (t == (g.proto == P_ICMP4 ? 8u : 128u) && code == 0u) {
                off = g.l4_off + 8;
                plen = g.l4_len - 8;
                fl = echo_rule(request(plen, 0u), v.bcast_v4);
                if (fl & SMOL_ECHO_ANSWERED) hl = echo_head_len(rr.kind & 0xffu, g.fam);
            }
        }
        const bool answered = (fl & SMOL_ECHO_ANSWERED) != 0;
        const bool written = answered && hl + plen <= sl.z;  // the cap test, before the first store
        const bool st = written && plen > 0;
        const uint64_t D = (uint64_t)v.dst + ((uint64_t)sl.x | ((uint64_t)sl.y << 32));
        const Dest d = dest_of(rr.a0, head, off, D + hl, plen);  // the data, behind the head
        // the two sums part at the data's first byte (no request: everything in the first)
        const int split = fl ? (int)off : s1;

        uint32_t acc = 0, accd = 0;
        for (uint32_t i0 = 0; i0 < nch; i0 += (uint32_t)(G * U)) {
            if (i0) load_step<G, U, XH_FIRST>(rec.base, nch, i0, st, lane, dummy, c, xh);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                if (k < nch) {
                    const int pos = (int)(16u * k) - (int)head;
                    acc = sum_range(c[u], pos, 0, split, acc);
                    accd = sum_range(c[u], pos, split, s1, accd);
                }
            }
            if (st) store_step<G, U>(c, xh, i0, nch, lane, d);  // (the group's lanes together)
        }

        uint32_t stv = 0;  // lane 0: the status byte
        finish<G>(p, rec, acc + accd, r, lane, &stv);
        if (answered) {  // (the group's lanes together)
            // the reply's ICMP sum, big-endian words: this lane's data bytes (an aligned-word sum from an odd
            // address is the big-endian one, from an even address its byte swap: data_off is even), its share
            // of the pseudo-header's address words, and on lane 0 the words that are no record bytes
            const uint32_t f = fold32(accd);
            uint32_t mine = (rr.a0 & 1u) ? f : bswap16(f);
            const WinReq q = request(plen, rec.rd(off - 4) << 24 | rec.rd(off - 3) << 16 | rec.rd(off - 2) << 8 | rec.rd(off - 1));
            const bool v6 = q.ver_ == 6;
            if (v6) {
                for (uint32_t i = lane; i < 16u; i += G) {
                    const uint32_t o = head + g.addr_off + 2 * i;
                    mine += (winb[o] << 8) | winb[o + 1];
                }
            }
            if (lane == 0) mine += (q.idseq_ >> 16) + (q.idseq_ & 0xffffu) + (v6 ? 0x8100u + (uint32_t)P_ICMP6 + 8u + plen : 0u);
            const uint32_t tot = group_sum<G>(mine);
            const uint32_t l4ck = caps_tx(v6 ? p.caps_icmpv6 : p.caps_icmpv4) ? (~fold32(tot) & 0xffffu) : 0u;
            if (written) {
                const uint32_t e = q.kind_ == SMOL_KIND_ETH ? 14u : 0u;
                const uint32_t ipo = echo_ipck_off(q.kind_, q.ver_), l4o = echo_l4ck_off(q.kind_, q.ver_);
                uint32_t ipck = 0;
                if (!v6 && caps_tx(p.caps_ipv4)) ipck = ~fold32(echo_head_words(q, e, 10u)) & 0xffffu;
                store_head<G>(D, hl, lane, [&](uint32_t i) -> uint32_t {
                    if (i == ipo) return ipck >> 8;
                    if (i == ipo + 1) return ipck & 0xffu;
                    if (i == l4o) return l4ck >> 8;
                    if (i == l4o + 1) return l4ck & 0xffu;
                    return echo_head_byte(q, i);
                });
            }
        }
        if (lane == 0) {  // smol_csum_echo_t: frame_len, data_off, head_len, flags
            if (written) fl |= SMOL_ECHO_WRITTEN | ((stv & SMOL_ST_ACCEPT) ? SMOL_ECHO_SEND : 0u);
            const uint64_t e = (uint64_t)(answered ? hl + plen : 0u) | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)hl << 48) | ((uint64_t)fl << 56);
            *(GMEM uint64_t*)((uint64_t)v.echo + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

hipError_t launch_echo(int shape, const KParams& p, const EchoArgs& v, uint32_t max_blocks, hipStream_t s) {
    return deliver::launch_shaped(KERN_ECHO, 0, shape, p, max_blocks, [&](auto g, auto u, auto im, uint32_t blocks) {
        hipLaunchKernelGGL((echo_kernel<decltype(g)::value, decltype(u)::value, decltype(im)::value>), dim3(blocks), dim3(256), 0, s,
                           p, v);
    });
}

}  // namespace smolcsum
