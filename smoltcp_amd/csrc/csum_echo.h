// The reply-head rule of smol_csum_batch_verify_echo_reply (include/smolcsum.h): which echo requests the
// engine answers on wire-level facts alone, and the bytes in front of the echoed data.  Plain host / device
// functions with no HIP in them, so that the text echo_kernel (csum_echo.hip) runs is walked on the CPU
// under the sanitizers (tests/cpp/echo_rule_asan.cpp).
//
// The reference answers an echo request in icmpv4_reply / icmpv6_reply (src/iface/interface/ipv4.rs:373-418,
// src/iface/interface/ipv6.rs:538-563) after process_ipv6's source test (ipv6.rs:198):
//   IPv4: a non-unicast source gets nothing; a unicast destination is answered from that address; a
//         broadcast destination is answered from ipv4_addr(), which only the host knows (HOST); any other
//         destination (multicast, unspecified) gets nothing.
//   IPv6: a non-unicast source gets nothing; a unicast destination is answered from that address; a
//         multicast destination from get_source_address_ipv6 (HOST).
//   Ethernet: the reply goes to the request's source MAC from the request's destination MAC only when both
//         are unicast; otherwise the neighbour cache and the interface's own MAC decide (HOST).
// The head is what Ipv4Repr::emit (src/wire/ipv4.rs:584-612) / Ipv6Repr::emit (src/wire/ipv6.rs:631-638)
// and the EchoReply arm of Icmpv4Repr::emit / Icmpv6Repr::emit (icmpv4.rs:506-517, icmpv6.rs:814-822) write,
// with both checksum fields zero; the caller fills them.
//
// A request is anything with these members (the kernel reads them from its LDS window, the CPU walk from a
// struct): kind() SMOL_KIND_IP / SMOL_KIND_ETH, ver() 4 / 6, mac_dst(j) / mac_src(j) j < 6 and ethertype(j)
// j < 2 (Ethernet only), src(j) / dst(j) j < 4 or 16, idseq(j) j < 4 (the message's bytes 4..7), dlen() the
// echo data length.  No function here keeps a byte array, so the kernel needs no scratch for them.
#pragma once
#include <cstdint>

#include "../../include/smolcsum.h"

#if defined(__HIPCC__)
#define SMOL_ECHO_FN __host__ __device__ inline
#else
#define SMOL_ECHO_FN inline
#endif

namespace smolcsum {

constexpr uint32_t ECHO_NO_FIELD = 0xffu;

// a: the address as a big-endian word; bcast: cfg's bcast_v4 the same way (0: none)
SMOL_ECHO_FN bool echo_bcast4(uint32_t a, uint32_t bcast) { return a == 0xffffffffu || (bcast != 0u && a == bcast); }
SMOL_ECHO_FN bool echo_nonuni4(uint32_t a, uint32_t bcast) {
    return echo_bcast4(a, bcast) || (a >> 28) == 0xeu || a == 0u;
}

// The SMOL_ECHO_* flags of a well-formed echo request: REQUEST, and ANSWERED or HOST or neither.
template <class RQ>
SMOL_ECHO_FN uint32_t echo_rule(const RQ& q, uint32_t bcast) {
    uint32_t f = SMOL_ECHO_REQUEST;
    if (q.ver() == 4) {
        uint32_t s = 0, d = 0;
        for (uint32_t j = 0; j < 4; ++j) {
            s = s << 8 | (q.src(j) & 0xffu);
            d = d << 8 | (q.dst(j) & 0xffu);
        }
        if (echo_nonuni4(s, bcast)) return f;
        if (!echo_nonuni4(d, bcast)) f |= SMOL_ECHO_ANSWERED;
        else if (echo_bcast4(d, bcast)) f |= SMOL_ECHO_HOST;
        else return f;
    } else {
        uint32_t s = 0, d = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            s |= q.src(j) & 0xffu;
            d |= q.dst(j) & 0xffu;
        }
        if ((q.src(0) & 0xffu) == 0xffu || s == 0u) return f;
        f |= ((q.dst(0) & 0xffu) == 0xffu || d == 0u) ? SMOL_ECHO_HOST : SMOL_ECHO_ANSWERED;
    }
    if (q.kind() == SMOL_KIND_ETH && (f & SMOL_ECHO_ANSWERED) && ((q.mac_dst(0) | q.mac_src(0)) & 1u))
        f = (f & ~SMOL_ECHO_ANSWERED) | SMOL_ECHO_HOST;
    return f;
}

// Reply bytes in front of the data: 14 | 0 + 20 | 40 + 8.
SMOL_ECHO_FN uint32_t echo_head_len(uint32_t kind, uint32_t ver) {
    return (kind == SMOL_KIND_ETH ? 14u : 0u) + (ver == 4 ? 20u : 40u) + 8u;
}
// Head offsets of the two checksum fields (the IPv4 header's: ECHO_NO_FIELD over IPv6).
SMOL_ECHO_FN uint32_t echo_ipck_off(uint32_t kind, uint32_t ver) {
    return ver == 4 ? (kind == SMOL_KIND_ETH ? 24u : 10u) : ECHO_NO_FIELD;
}
SMOL_ECHO_FN uint32_t echo_l4ck_off(uint32_t kind, uint32_t ver) { return echo_head_len(kind, ver) - 6u; }

// Byte i (< echo_head_len) of the reply's head, both checksum fields zero.
template <class RQ>
SMOL_ECHO_FN uint32_t echo_head_byte(const RQ& q, uint32_t i) {
    if (q.kind() == SMOL_KIND_ETH) {
        if (i < 6) return q.mac_src(i) & 0xffu;
        if (i < 12) return q.mac_dst(i - 6) & 0xffu;
        if (i < 14) return q.ethertype(i - 12) & 0xffu;
        i -= 14;
    }
    if (q.ver() == 4) {
        const uint32_t total = 28u + q.dlen();
        if (i < 20) {
            switch (i) {
                case 0: return 0x45u;
                case 2: return (total >> 8) & 0xffu;
                case 3: return total & 0xffu;
                case 6: return 0x40u;  // DF, offset 0
                case 8: return 64u;    // TTL
                case 9: return 1u;     // ICMP
                case 12: case 13: case 14: case 15: return q.dst(i - 12) & 0xffu;
                case 16: case 17: case 18: case 19: return q.src(i - 16) & 0xffu;
                default: return 0u;    // DSCP / ECN, ident, checksum
            }
        }
        i -= 20;
    } else {
        const uint32_t plen = 8u + q.dlen();
        if (i < 40) {
            if (i >= 24) return q.src(i - 24) & 0xffu;
            if (i >= 8) return q.dst(i - 8) & 0xffu;
            switch (i) {
                case 0: return 0x60u;
                case 4: return (plen >> 8) & 0xffu;
                case 5: return plen & 0xffu;
                case 6: return 58u;  // ICMPv6
                case 7: return 64u;  // hop limit
                default: return 0u;  // traffic class, flow label
            }
        }
        i -= 40;
    }
    if (i == 0) return q.ver() == 4 ? 0u : 129u;  // EchoReply
    if (i >= 4 && i < 8) return q.idseq(i - 4) & 0xffu;
    return 0u;  // code, checksum
}

// Big-endian word sum (not folded) of head bytes [from, from + 2 * words), from even.
template <class RQ>
SMOL_ECHO_FN uint32_t echo_head_words(const RQ& q, uint32_t from, uint32_t words) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < words; ++w) s += echo_head_byte(q, from + 2 * w) << 8 | echo_head_byte(q, from + 2 * w + 1);
    return s;
}

}  // namespace smolcsum
