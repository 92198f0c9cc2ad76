// Fused verify + ICMP error responder (smol_csum_batch_verify_unreach_reply): echo_kernel (csum_echo.hip)
// with the two sums ending at different bytes, a port map and a longer head.
//
// The reference refuses a UDP datagram to a closed port (process_udp, src/iface/interface/udp.rs:49-77), an
// IPv4 packet of an unhandled protocol (ipv4.rs:240-250) and an IPv6 packet with an unrecognised next header
// (process_nxt_hdr, ipv6.rs:352-364) with an ICMP error that quotes the IP header, emitted again, and the first
// 528 / 1192 bytes of the IP payload: UdpRepr::parse sums the datagram, Icmpv4Repr::emit / Icmpv6Repr::emit
// copy the slice (icmpv4.rs:519-531, icmpv6.rs:740-755) and fill_checksum sums the copy.  Here every 16-B chunk
// of a record is loaded once.
//
// The record stream is csum_deliver.h's (load_step, Record::parse, store_step, finish): a group of G lanes owns
// a record, and the data goes to its place behind the frame's head as one Dest.  What is this file's own:
// * Three regions from one starting byte.  The verdict sums record bytes [0, s1) (s1: verify's span end, 0 when
//   it sums nothing of the record), the reply [off, e2) (off: the IP payload's first byte, e2 = off + dlen).
//   Each lane keeps two accumulators over disjoint bytes: [0, min(s1, e2)) and [min, max).  The first belongs to
//   both sums, the second to the one that ends later: that owner is one comparison per record.  The ends are
//   byte-exact (sum_range masks the edge chunks), so an odd UDP length pads the verdict's sum with a zero byte
//   while the reply's runs on, and for the protocol / next-header forms (s1 = 0) the whole data is the reply's.
//   The verdict's sum goes to finish_gates (MODE_VERIFY) unchanged.  The reply's leaves out the header bytes
//   [0, off), which the lanes sum again from the LDS window, as finish_gates does for the verdict: plain u32
//   sums, nothing is subtracted from a folded value, so 0x0000 and 0xffff stay apart.
// * The port map.  One dependent byte load after the parse, for well-formed UDP records only.
// * Head.  The rule and the head's bytes with zero checksum fields are csum_unreach.h's, read from the LDS
//   window.  The group's lanes share the word sums of the two IPv4 headers and of the ICMP message; then every
//   lane patches the three checksums into the bytes it hands to store_head (up to 27 dwords a frame), so no
//   byte of d_dst is read and none outside the frame is written.
// * Entry.  Lane 0 writes the record's 8-byte smol_csum_unreach_t; SEND comes from the status byte finish_gates
//   hands back.
// The cap is tested before the first store.  The copy does not wait for the verdict.
#include "csum_deliver.h"
#include "csum_unreach.h"

namespace smolcsum {

namespace unreach {

// load_step's extra load is issued last here, as before the stream was shared: issued first the 1514-B and
// 1294-B shapes took 0.9 and 2.4 % longer than the separate text, issued last -0.1 and 1.7 %.
constexpr bool XH_FIRST = false;

// The request as csum_unreach.h reads it: addresses, MACs and the TTL / hop limit from the LDS window (record
// byte o at w[o]; all of them lie in front of byte 54), the rest in registers.
struct WinReq {
    const uint8_t* w;
    uint32_t kind_, ver_, ip_, plen_, proto_, hbh_;
    __device__ __forceinline__ uint32_t kind() const { return kind_; }
    __device__ __forceinline__ uint32_t ver() const { return ver_; }
    __device__ __forceinline__ uint32_t plen() const { return plen_; }
    __device__ __forceinline__ uint32_t proto() const { return proto_; }
    __device__ __forceinline__ bool hbh() const { return hbh_ != 0; }
    __device__ __forceinline__ uint32_t hop() const { return w[ip_ + (ver_ == 4 ? 8u : 7u)]; }
    __device__ __forceinline__ uint32_t mac_dst(uint32_t j) const { return w[j]; }
    __device__ __forceinline__ uint32_t mac_src(uint32_t j) const { return w[6 + j]; }
    __device__ __forceinline__ uint32_t ethertype(uint32_t j) const { return w[12 + j]; }
    __device__ __forceinline__ uint32_t src(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 12u : 8u) + j]; }
    __device__ __forceinline__ uint32_t dst(uint32_t j) const { return w[ip_ + (ver_ == 4 ? 16u : 24u) + j]; }
};

// What the rule left of a record, in LDS beside its geometry: unreach_rule's result, the IP payload's offset
// (0 unless REFUSED) and length P, and the protocol / next header reached | hbh << 8.
struct Fact {
    uint32_t rv, off, plen, proto, dlo, dhi, cap;  // (dlo, dhi, cap: the record's slot)
};

}  // namespace unreach

template <int G, int U, bool IMPLICIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void unreach_kernel(KParams p, UnreachArgs v) {
    using namespace deliver;
    using namespace unreach;
    constexpr int GPB = 256 / G;
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];
    __shared__ Fact fct[GPB];

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

        // the refusal (process_udp udp.rs:49-77, ipv4.rs:240-250, process_nxt_hdr ipv6.rs:352-364), the address
        // rule and the frame's geometry
        // (its result goes to LDS next to the geometry and is read back behind the stream, where the frame's
        // geometry is worked out again: held in registers across the stream it spilled 12 to 40 bytes in half of
        // the instantiations)
        if (lane == 0) {
            uint32_t rv = 0, off = 0, plen = 0, proto = 0, hbh = 0;
            if (g.fam != 0 && !(rr.kind & KIND_IPHDR_ONLY) && !(g.st & SMOL_ST_MALFORMED)) {
                // an unsupported record that got past the fragment test (which leaves l4_off 0) is one of an
                // unknown protocol / next header; a UDP record is looked up in the port map
                bool cand = (g.st & SMOL_ST_UNSUPPORTED) && g.l4_off != 0, closed = false;
                if (!g.st && g.proto == P_UDP && v.udp_open) {
                    const uint32_t dp = rec.rd(g.l4_off + 2) << 8 | rec.rd(g.l4_off + 3);
                    closed = ((ld_byte_sync((uint64_t)v.udp_open + (dp >> 3)) >> (dp & 7u)) & 1u) == 0;
                    cand = closed;
                }
                if (cand) {
                    if (g.fam == 4) {
                        proto = rec.rd(g.ip_off + 9);
                        off = g.l4_off;
                        plen = g.l4_len;
                    } else {
                        const uint32_t nh = rec.rd(g.ip_off + 6);
                        hbh = nh == 0;
                        proto = hbh ? rec.rd(g.ip_off + 40) : nh;
                        off = g.ip_off + 40;
                        plen = rec.rd(g.ip_off + 4) << 8 | rec.rd(g.ip_off + 5);
                    }
                    rv = unreach_rule(WinReq{winb + head, rr.kind & 0xffu, g.fam, g.ip_off, plen, proto, hbh}, v.bcast_v4, closed);
                }
            }
            Fact f;  // off: 0 unless REFUSED
            f.rv = rv, f.off = rv ? off : 0u, f.plen = plen, f.proto = proto | hbh << 8;
            f.dlo = sl.x, f.dhi = sl.y, f.cap = sl.z;
            fct[gib] = f;
        }
        wave_lds_sync();
        // the record as the rule left it: the flags, the frame's lengths, the cap test (before the first store)
        auto frame = [&](uint32_t& fl, uint32_t& off, uint32_t& hl, uint32_t& dlen, bool& written) {
            const Fact& f = fct[gib];
            fl = unreach_flags(f.rv);
            off = f.off;
            const bool answered = (fl & SMOL_UNR_ANSWERED) != 0;
            hl = answered ? unreach_head_len(rr.kind & 0xffu, g.fam) : 0u;
            dlen = answered ? unreach_dlen(g.fam, f.plen) : 0u;
            written = answered && hl + dlen <= f.cap;
        };
        bool st;
        Dest d;  // the data, behind the head
        uint32_t dlen;
        int lo2, hi2;
        {
            uint32_t fl, off, hl;
            bool written;
            frame(fl, off, hl, dlen, written);
            st = written && dlen > 0;
            d = dest_of(rr.a0, head, off, (uint64_t)v.dst + ((uint64_t)fct[gib].dlo | ((uint64_t)fct[gib].dhi << 32)) + hl, dlen);
            // the two sums: [0, s1) and [off, e2); the accumulators part where the first of them ends
            const int e2 = (fl & SMOL_UNR_ANSWERED) ? (int)(off + dlen) : 0;
            lo2 = s1 < e2 ? s1 : e2, hi2 = s1 < e2 ? e2 : s1;
        }

        uint32_t acc = 0, accx = 0;
        for (uint32_t i0 = 0; i0 < nch; i0 += (uint32_t)(G * U)) {
            if (i0) load_step<G, U, XH_FIRST>(rec.base, nch, i0, st, lane, dummy, c, xh);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = i0 + (uint32_t)(u * G + lane);
                if (k < nch) {
                    const int pos = (int)(16u * k) - (int)head;
                    acc = sum_range(c[u], pos, 0, lo2, acc);
                    accx = sum_range(c[u], pos, lo2, hi2, accx);
                }
            }
            if (st) store_step<G, U>(c, xh, i0, nch, lane, d);  // (the group's lanes together)
        }

        uint32_t stv = 0;  // lane 0: the status byte
        // (the second accumulator is the sum's that ends later: the verdict's when hi2 is its end)
        finish<G>(p, rec, hi2 == s1 ? acc + accx : acc, r, lane, &stv);
        uint32_t fl, off, hl;
        bool written;
        frame(fl, off, hl, dlen, written);
        const uint64_t D = (uint64_t)v.dst + ((uint64_t)fct[gib].dlo | ((uint64_t)fct[gib].dhi << 32));
        if (fl & SMOL_UNR_ANSWERED) {  // (the group's lanes together)
            const uint32_t rv = fct[gib].rv;
            const WinReq q = {winb + head, rr.kind & 0xffu, g.fam, g.ip_off, fct[gib].plen, fct[gib].proto & 0xffu, 0u};
            const bool v6 = q.ver_ == 6, odd = (rr.a0 & 1u) != 0;
            const uint32_t e = q.kind_ == SMOL_KIND_ETH ? 14u : 0u, iph = v6 ? 40u : 20u;
            // the data's aligned-word sum: this lane's part of [0, e2) less its part of the header bytes [0, off)
            // (off is even: record offset 2 i is the low byte of an aligned word for an even record start)
            uint32_t mine = hi2 == s1 ? acc : acc + accx;
            for (uint32_t i = lane; 2 * i < off; i += G) {
                const uint32_t b0 = winb[head + 2 * i], b1 = winb[head + 2 * i + 1];
                mine -= odd ? ((b0 << 8) + b1) : (b0 + (b1 << 8));
            }
            const uint32_t f = fold32(group_sum<G>(mine));
            const uint32_t dat = odd ? f : bswap16(f);  // the big-endian word sum of the data, folded
            // both IPv4 header checksums (Ipv4Repr::emit twice under the same caps)
            uint32_t ipck = 0, inck = 0;
            if (!v6 && caps_tx(p.caps_ipv4)) {
                ipck = ~fold32(group_sum<G>(unreach_head_words(q, rv, e, 10u, (uint32_t)lane, (uint32_t)G))) & 0xffffu;
                inck = ~fold32(group_sum<G>(unreach_head_words(q, rv, e + 28u, 10u, (uint32_t)lane, (uint32_t)G))) & 0xffffu;
            }
            // the ICMP sum: the message's head words (the quoted header with its final checksum), the data, and
            // over IPv6 the pseudo-header: the reply's addresses, its length and next header
            uint32_t hw = unreach_head_words(q, rv, e + iph, (8u + iph) / 2u, (uint32_t)lane, (uint32_t)G);
            if (v6) hw += unreach_head_words(q, rv, e + 8u, 16u, (uint32_t)lane, (uint32_t)G);
            if (lane == 0) hw += dat + inck + (v6 ? (uint32_t)P_ICMP6 + 48u + dlen : 0u);
            const uint32_t tot = group_sum<G>(hw);
            const uint32_t l4ck = caps_tx(v6 ? p.caps_icmpv6 : p.caps_icmpv4) ? (~fold32(tot) & 0xffffu) : 0u;
            if (written) {
                const uint32_t ipo = unreach_ipck_off(q.kind_, q.ver_), l4o = unreach_l4ck_off(q.kind_, q.ver_);
                const uint32_t ino = unreach_inck_off(q.kind_, q.ver_);
                store_head<G>(D, hl, lane, [&](uint32_t i) -> uint32_t {
                    if (i == ipo) return ipck >> 8;
                    if (i == ipo + 1) return ipck & 0xffu;
                    if (i == l4o) return l4ck >> 8;
                    if (i == l4o + 1) return l4ck & 0xffu;
                    if (i == ino) return inck >> 8;
                    if (i == ino + 1) return inck & 0xffu;
                    return unreach_head_byte(q, rv, i);
                });
            }
        }
        if (lane == 0) {  // smol_csum_unreach_t: frame_len, data_off, head_len, flags
            if (written) fl |= SMOL_UNR_WRITTEN | ((stv & SMOL_ST_ACCEPT) ? SMOL_UNR_SEND : 0u);
            const uint64_t e = (uint64_t)(hl + dlen) | ((uint64_t)(off & 0xffffu) << 32) | ((uint64_t)hl << 48) | ((uint64_t)fl << 56);
            *(GMEM uint64_t*)((uint64_t)v.unr + 8ull * r) = e;
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

hipError_t launch_unreach(int shape, const KParams& p, const UnreachArgs& v, uint32_t max_blocks, hipStream_t s) {
    return deliver::launch_shaped(KERN_UNREACH, 0, shape, p, max_blocks, [&](auto g, auto u, auto im, uint32_t blocks) {
        hipLaunchKernelGGL((unreach_kernel<decltype(g)::value, decltype(u)::value, decltype(im)::value>), dim3(blocks), dim3(256), 0,
                           s, p, v);
    });
}

}  // namespace smolcsum
