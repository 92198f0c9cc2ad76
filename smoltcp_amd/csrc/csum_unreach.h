// The refusal rule of smol_csum_batch_verify_unreach_reply (include/smolcsum.h): which datagrams nobody takes
// the engine answers with an ICMP error on wire-level facts alone, and the bytes in front of the quoted data.
// Plain host / device functions with no HIP in them, so that the text unreach_kernel (csum_unreach.hip) runs
// is walked on the CPU under the sanitizers (tests/cpp/unreach_rule_asan.cpp).
//
// The reference refuses a datagram in three places:
//   process_udp (src/iface/interface/udp.rs:49-77): no socket accepts the destination port: Destination
//         Unreachable / Port Unreachable, ICMPv4 3 / 3 or ICMPv6 1 / 4;
//   process_ipv4 (src/iface/interface/ipv4.rs:240-250): a protocol it does not handle: ICMPv4 3 / 2;
//   process_nxt_hdr (src/iface/interface/ipv6.rs:352-364): an unrecognised next header: ICMPv6 Parameter
//         Problem 4 / 1 with pointer 40.
// and sends the error through icmpv4_reply / icmpv6_reply (ipv4.rs:373-418, ipv6.rs:538-563):
//   IPv4: only when source and destination are both unicast (the broadcast arm answers echo replies only);
//   IPv6: a non-unicast source gets nothing (process_ipv6, ipv6.rs:198); a unicast destination is answered
//         from that address, a multicast one from get_source_address_ipv6, which only the host knows (HOST);
//   Ethernet: both MACs must be unicast, else the neighbour cache and the interface's MAC decide (HOST).
// Behind a leading Hop-by-Hop header the reference quotes the post-option payload behind the header as parsed:
// that reply stays with the host (HOST, nothing written).
// The head is what Ipv4Repr::emit (src/wire/ipv4.rs:584-612) / Ipv6Repr::emit (src/wire/ipv6.rs:631-638) write
// twice, for the reply and for the quoted header (Icmpv4Repr::emit icmpv4.rs:519-531, emit_contained_packet
// icmpv6.rs:740-755), with every checksum field zero; the caller fills them.
//
// A request is anything with these members (the kernel reads them from its LDS window, the CPU walk from a
// struct): kind() SMOL_KIND_IP / SMOL_KIND_ETH, ver() 4 / 6, mac_dst(j) / mac_src(j) j < 6 and ethertype(j)
// j < 2 (Ethernet only), src(j) / dst(j) j < 4 or 16, hop() the TTL / hop limit, proto() the IPv4 protocol or
// the IPv6 next header the dispatch reaches (behind the Hop-by-Hop header when hbh()), hbh() whether the IPv6
// header's own next header is 0, plen() P: the IP payload's length (IPv4 total length - IHL * 4, the IPv6
// payload length).  No function here keeps a byte array, so the kernel needs no scratch for them.
#pragma once
#include "csum_echo.h"

namespace smolcsum {

constexpr uint32_t UNR_DATA_V4 = 576u - 2u * 20u - 8u;   // icmp_reply_payload_len(len, IPV4_MIN_MTU, 20)
constexpr uint32_t UNR_DATA_V6 = 1280u - 2u * 40u - 8u;  // icmp_reply_payload_len(len, IPV6_MIN_MTU, 40)

// The quoted data's length: icmp_reply_payload_len (src/iface/packet.rs:254-264).
SMOL_ECHO_FN uint32_t unreach_dlen(uint32_t ver, uint32_t plen) {
    const uint32_t cap = ver == 4 ? UNR_DATA_V4 : UNR_DATA_V6;
    return plen < cap ? plen : cap;
}

// The rule's result: SMOL_UNR_* flags | ICMP type << 8 | code << 16 (0: the record is not refused).
SMOL_ECHO_FN uint32_t unreach_flags(uint32_t rv) { return rv & 0xffu; }
SMOL_ECHO_FN uint32_t unreach_type(uint32_t rv) { return (rv >> 8) & 0xffu; }
SMOL_ECHO_FN uint32_t unreach_code(uint32_t rv) { return (rv >> 16) & 0xffu; }

// q: a record whose IP header passed check_len, that is no fragment and no SMOL_REC_IPHDR_ONLY record, and that
// verify's parse does not mark malformed.  udp_closed (looked at for proto() 17 only): the datagram passed
// UdpPacket::check_len and the port test of UdpRepr::parse, and the port map's bit of its destination port is
// clear.  Returns REFUSED, PORT for the UDP form, and ANSWERED or HOST or neither, with the type and code.
template <class RQ>
SMOL_ECHO_FN uint32_t unreach_rule(const RQ& q, uint32_t bcast, bool udp_closed) {
    uint32_t f = SMOL_UNR_REFUSED, type, code;
    const uint32_t p = q.proto();
    if (p == 17u) {
        if (!udp_closed) return 0u;
        f |= SMOL_UNR_PORT;
        type = q.ver() == 4 ? 3u : 1u;  // DstUnreachable
        code = q.ver() == 4 ? 3u : 4u;  // PortUnreachable
    } else if (q.ver() == 4) {
        if (p == 1u || p == 2u || p == 6u) return 0u;
        type = 3u, code = 2u;  // DstUnreachable / ProtoUnreachable
    } else {
        // (0 is the header's own Hop-by-Hop, which hbh() names; reached behind one it is unrecognised)
        if (p == 6u || p == 58u || (p == 0u && !q.hbh())) return 0u;
        type = 4u, code = 1u;  // ParamProblem / UnrecognizedNxtHdr
    }
    const uint32_t tc = type << 8 | code << 16;
    if (q.ver() == 4) {
        uint32_t s = 0, d = 0;
        for (uint32_t j = 0; j < 4; ++j) {
            s = s << 8 | (q.src(j) & 0xffu);
            d = d << 8 | (q.dst(j) & 0xffu);
        }
        if (echo_nonuni4(s, bcast) || echo_nonuni4(d, bcast)) return f | tc;
        f |= SMOL_UNR_ANSWERED;
    } else {
        uint32_t s = 0, d = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            s |= q.src(j) & 0xffu;
            d |= q.dst(j) & 0xffu;
        }
        if ((q.src(0) & 0xffu) == 0xffu || s == 0u) return f | tc;
        f |= ((q.dst(0) & 0xffu) == 0xffu || d == 0u || q.hbh()) ? SMOL_UNR_HOST : SMOL_UNR_ANSWERED;
    }
    if (q.kind() == SMOL_KIND_ETH && (f & SMOL_UNR_ANSWERED) && ((q.mac_dst(0) | q.mac_src(0)) & 1u))
        f = (f & ~SMOL_UNR_ANSWERED) | SMOL_UNR_HOST;
    return f | tc;
}

// Frame bytes in front of the data: 14 | 0, the reply's IP header, 8 of ICMP, the quoted IP header.
SMOL_ECHO_FN uint32_t unreach_head_len(uint32_t kind, uint32_t ver) {
    return (kind == SMOL_KIND_ETH ? 14u : 0u) + (ver == 4 ? 48u : 88u);
}
// Head offsets of the checksum fields: the reply's IPv4 header's and the quoted one's (ECHO_NO_FIELD over
// IPv6), and the ICMP message's.
SMOL_ECHO_FN uint32_t unreach_ipck_off(uint32_t kind, uint32_t ver) { return echo_ipck_off(kind, ver); }
SMOL_ECHO_FN uint32_t unreach_l4ck_off(uint32_t kind, uint32_t ver) {
    return (kind == SMOL_KIND_ETH ? 14u : 0u) + (ver == 4 ? 22u : 42u);
}
SMOL_ECHO_FN uint32_t unreach_inck_off(uint32_t kind, uint32_t ver) {
    return ver == 4 ? (kind == SMOL_KIND_ETH ? 52u : 38u) : ECHO_NO_FIELD;
}

// Byte i (< 20) of an IPv4 header as Ipv4Repr::emit writes it, the checksum zero; rev: the addresses swapped.
template <class RQ>
SMOL_ECHO_FN uint32_t unreach_ip4_byte(const RQ& q, uint32_t i, uint32_t total, uint32_t ttl, uint32_t proto, bool rev) {
    switch (i) {
        case 0: return 0x45u;
        case 2: return (total >> 8) & 0xffu;
        case 3: return total & 0xffu;
        case 6: return 0x40u;  // DF, offset 0
        case 8: return ttl & 0xffu;
        case 9: return proto & 0xffu;
        case 12: case 13: case 14: case 15: return (rev ? q.dst(i - 12) : q.src(i - 12)) & 0xffu;
        case 16: case 17: case 18: case 19: return (rev ? q.src(i - 16) : q.dst(i - 16)) & 0xffu;
        default: return 0u;  // DSCP / ECN, ident, checksum
    }
}
// Byte i (< 40) of an IPv6 header as Ipv6Repr::emit writes it.
template <class RQ>
SMOL_ECHO_FN uint32_t unreach_ip6_byte(const RQ& q, uint32_t i, uint32_t plen, uint32_t nh, uint32_t hop, bool rev) {
    if (i >= 24) return (rev ? q.src(i - 24) : q.dst(i - 24)) & 0xffu;
    if (i >= 8) return (rev ? q.dst(i - 8) : q.src(i - 8)) & 0xffu;
    switch (i) {
        case 0: return 0x60u;
        case 4: return (plen >> 8) & 0xffu;
        case 5: return plen & 0xffu;
        case 6: return nh & 0xffu;
        case 7: return hop & 0xffu;
        default: return 0u;  // traffic class, flow label
    }
}

// Byte i (< unreach_head_len) of the error frame's head, every checksum field zero.  rv: unreach_rule's result.
template <class RQ>
SMOL_ECHO_FN uint32_t unreach_head_byte(const RQ& q, uint32_t rv, uint32_t i) {
    if (q.kind() == SMOL_KIND_ETH) {
        if (i < 6) return q.mac_src(i) & 0xffu;
        if (i < 12) return q.mac_dst(i - 6) & 0xffu;
        if (i < 14) return q.ethertype(i - 12) & 0xffu;
        i -= 14;
    }
    const uint32_t dlen = unreach_dlen(q.ver(), q.plen());
    if (q.ver() == 4) {
        if (i < 20) return unreach_ip4_byte(q, i, 48u + dlen, 64u, 1u, true);
        i -= 20;
    } else {
        if (i < 40) return unreach_ip6_byte(q, i, 48u + dlen, 58u, 64u, true);
        i -= 40;
    }
    if (i < 8) {
        // type, code, checksum, then 4 bytes: unused in DstUnreachable (the reference leaves what its fresh
        // token buffer held: 0), the pointer 40 = ipv6_repr.buffer_len() in ParamProblem
        if (i == 0) return unreach_type(rv);
        if (i == 1) return unreach_code(rv);
        return (i == 7 && unreach_type(rv) == 4u) ? 40u : 0u;
    }
    i -= 8;
    // the quoted header, emitted again from the parsed repr: the full P, the request's TTL and protocol
    if (q.ver() == 4) return unreach_ip4_byte(q, i, 20u + q.plen(), q.hop(), q.proto(), false);
    return unreach_ip6_byte(q, i, q.plen(), q.proto(), q.hop(), false);
}

// Big-endian word sum (not folded) of the head's words w0, w0 + step, .. below `words`, word w being head
// bytes from + 2 w and from + 2 w + 1 (from even): a group's lanes share a range with w0 = lane, step = G.
template <class RQ>
SMOL_ECHO_FN uint32_t unreach_head_words(const RQ& q, uint32_t rv, uint32_t from, uint32_t words, uint32_t w0 = 0,
                                         uint32_t step = 1) {
    uint32_t s = 0;
    for (uint32_t w = w0; w < words; w += step)
        s += unreach_head_byte(q, rv, from + 2 * w) << 8 | unreach_head_byte(q, rv, from + 2 * w + 1);
    return s;
}

}  // namespace smolcsum
