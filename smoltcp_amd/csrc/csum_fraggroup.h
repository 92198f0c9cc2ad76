// IPv4 fragment groups: what frag_kernel (csum_frag.hip) and fragcopy_kernel (csum_fragcopy.hip) must
// agree on, written once.  Device code only.
//
// Under offloaded checksums smoltcp emits a datagram that exceeds the MTU whole — its L4 checksum
// written 0 by the ignored caps — and only then cuts it into fragments, each handed to
// TxToken::consume on its own (src/iface/interface/mod.rs:1276-1331, src/iface/interface/ipv4.rs:
// 440-490).  On receive it reassembles the fragment payloads and runs the L4 gate on the whole
// payload (ipv4.rs:103-146).  A device that holds a datagram's fragments until the last one arrives
// can do both, a group of fragments at a time:
//
//   1. fragment j's IPv4 header is parsed (Ipv4Packet::check_len, the reassembly key, the payload
//      range [frag_offset, frag_offset + total_len - hl)) and filled / verified: frag_header;
//   2. the group contract is checked: one key, non-empty payloads that cover [0, T) exactly once
//      (unique starts, one starting at 0, every end but T meets a start, lengths sum to T) with
//      exactly one last fragment (MF clear) ending at T: frag_header's contributions, contract_row;
//   3. the L4 header is read through the datagram map (datagram offset -> the fragment holding it):
//      DgMap, l4_header;
//   4. the kernel sums the payload slices its own way: a payload starts at an even datagram offset (a
//      multiple of 8), so data() of the datagram is the one's-complement sum of the fragments' data()
//      values;
//   5. the same gates as finish_gates (csum_walk.h) give the field value or the verdict (l4_sum,
//      l4_verdict) and every fragment's status byte (frag_status).
//
// A kernel file says how lanes are dealt to fragments, how values are reduced over them, and phase 4.
#pragma once

#include "csum_walk.h"

namespace smolcsum {
namespace fraggroup {

constexpr uint32_t MAXF = SMOL_MAX_FRAGMENTS;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}
__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0; }

__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// An invalid group (outside the batch, count 0 or > SMOL_MAX_FRAGMENTS, reserved != 0): none of its
// records is read or written (include/smolcsum.h).
__device__ __forceinline__ bool group_valid(const KParams& p, const smol_csum_frag_group_t& g) {
    return !(g.first >= p.n || g.count == 0 || g.count > MAXF || g.count > p.n - g.first || g.reserved != 0);
}

// Fragment 0's reassembly key (ipv4.rs get_key: ident, src, dst, protocol): the address of its IPv4
// header, usable when the record can hold one.
struct Key {
    uint64_t a;
    bool ok;
};
template <bool IMPLICIT>
__device__ __forceinline__ Key group_key(const KParams& p, uint64_t first) {
    const RecRef rr = rec_at<IMPLICIT, false>(p, first);
    const uint32_t kind = rr.kind & 0xffu;
    const uint32_t io = kind == SMOL_KIND_ETH ? 14u : 0u;
    Key k = {0, false};
    if ((kind == SMOL_KIND_IP || kind == SMOL_KIND_ETH) && rr.len >= io + 20) {
        k.a = rr.a0 + io;
        k.ok = true;
    }
    return k;
}

// One fragment's IPv4 header.  bits: bit 0 check_len ok, 1 MF, 2 IP gate passed, 3 header valid (the
// map's byte).  T, sumlen and lastn are the fragment's contributions to the group's values: its end,
// its payload length, 1 when MF is clear.
struct FragHdr {
    uint64_t addr;  // payload start address
    uint32_t start, end, bits;
    bool bad;  // breaks the contract by itself: no checked header, another key, an empty payload
    bool raw;  // a raw socket's datagram: headers only (KIND_IPHDR_ONLY)
    uint32_t T, sumlen, lastn;
};
// Record r (SMOL_KIND_*, + KIND_IPHDR_ONLY for a raw frame) against the key.  EMIT fills the header
// checksum (dispatch_ipv4_frag, ipv4.rs:482-484); verify puts its verdict into the bits.
template <bool EMIT, bool IMPLICIT>
__device__ __forceinline__ FragHdr frag_header(const KParams& p, uint64_t r, const Key& k0) {
    const RecRef rr = rec_at<IMPLICIT, false>(p, r);
    const uint64_t a0 = rr.a0;
    const uint32_t len = rr.len;
    FragHdr h = {};
    h.raw = (rr.kind & KIND_IPHDR_ONLY) != 0;
    const uint32_t kind = rr.kind & 0xffu;
    uint32_t io = 0, ok = 0, hl = 0, total = 0, start = 0, end = 0, mf = 0;
    if (kind == SMOL_KIND_ETH) {
        io = 14;
        ok = len >= 14 && rb16(a0 + 12) == 0x0800u;
    } else {
        ok = kind == SMOL_KIND_IP;
    }
    const uint64_t ip = a0 + io;
    if (ok) ok = len - io >= 20 && (rb(ip) >> 4) == 4;
    if (ok) {
        hl = (rb(ip) & 0x0fu) * 4;
        total = rb16(ip + 2);
        const uint32_t lb = len - io;
        ok = !(lb < hl || hl > total || lb < total || hl < 20);  // Ipv4Packet::check_len
    }
    uint32_t bits = 0xcu;  // IP gate / header: passed unless verified and found bad
    if (ok) {
        const uint32_t fl = rb16(ip + 6);
        start = (fl & 0x1fffu) * 8;  // Ipv4Packet::frag_offset, ipv4.rs:319-322
        end = start + total - hl;
        mf = (fl >> 13) & 1u;
        bool same = k0.ok && rb(ip + 9) == rb(k0.a + 9) && rb16(ip + 4) == rb16(k0.a + 4);
        for (uint32_t b = 12; b < 20; ++b) same = same && rb(ip + b) == rb(k0.a + b);
        h.bad = !same || end <= start;
        h.T = end;
        h.sumlen = end - start;
        h.lastn = mf ? 0u : 1u;
        // the fragment's own header: fill or verify
        uint32_t hs = 0;
        for (uint32_t w = 0; w < hl / 2; ++w)
            if (!(EMIT && w == 5)) hs += rb16(ip + 2 * w);
        const uint32_t hdr = fold32(hs);
        if (EMIT) {
            const uint32_t v = caps_tx(p.caps_ipv4) ? (~hdr & 0xffffu) : 0u;
            ((gu8)ip)[10] = (uint8_t)(v >> 8);
            ((gu8)ip)[11] = (uint8_t)v;
        } else {
            const uint32_t valid = hdr == 0xffffu;
            const uint32_t okg = caps_rx(p.caps_ipv4) ? valid : 1u;
            bits = (okg ? 4u : 0u) | (valid ? 8u : 0u);
        }
    } else {
        h.bad = true;  // no IPv4 header checked: its IP bits stay set, the record is MALFORMED
    }
    h.addr = ip + hl;
    h.start = start;
    h.end = end;
    h.bits = bits | (mf << 1) | (ok ? 1u : 0u);
    return h;
}

// The datagram map: the group's fragments as the kernel's four LDS arrays hold them.
struct DgMap {
    const uint64_t* addr;  // payload start address of fragment j
    const uint32_t *start, *end;
    const uint8_t* bits;  // FragHdr::bits
    uint32_t count;
    uint64_t dummy;  // KParams::dummy, a readable line
    // address of the datagram's byte o
    __device__ __forceinline__ uint64_t addr_of(uint32_t o) const {
        for (uint32_t i = 0; i < count; ++i)
            if (start[i] <= o && o < end[i]) return addr[i] + (o - start[i]);
        return dummy;  // (a usable group covers [0, T): not reached)
    }
    __device__ __forceinline__ uint32_t byte(uint32_t o) const { return rb(addr_of(o)); }
};

// Fragment j's row of the group contract, once the group's T is known and bad / lastn / sumlen have
// passed: its start is unique, its end meets exactly one start unless it is T, MF is clear only at T.
// zero: it starts at 0 (the group needs exactly one).
struct Row {
    bool broken;
    uint32_t zero;
};
__device__ __forceinline__ Row contract_row(const DgMap& m, uint32_t j, uint32_t T) {
    const uint32_t sj = m.start[j], ej = m.end[j];
    uint32_t starts = 0, next = 0;
    for (uint32_t i = 0; i < m.count; ++i) {
        starts += m.start[i] == sj;
        next += m.start[i] == ej;
    }
    Row r;
    r.zero = sj == 0;
    r.broken = starts != 1 || (ej != T && next != 1) || (!(m.bits[j] & 2u) && ej != T);
    return r;
}

// The L4 header through the map.  proto: P_NONE when nothing is summed (st says why: a broken group is
// MALFORMED, a raw one UNSUPPORTED); span_end: the datagram bytes summed; fo: the checksum field's
// offset; in_hl (EMIT): the header length of an ICMPv4 error's embedded IPv4 header, whose checksum emit
// fills too; key_proto, l4_off, l4_len: the key's protocol and the L4 payload (UdpPacket::payload,
// udp.rs:153-157; TcpPacket::payload, tcp.rs:419-423) for the datagram entry.
struct L4Hdr {
    uint32_t proto, st, span_end, fo, in_hl, key_proto, l4_off, l4_len;
};
template <bool EMIT>
__device__ __forceinline__ L4Hdr l4_header(const DgMap& m, const Key& k0, bool broken, bool raw, uint32_t T) {
    auto dg = [&](uint32_t o) -> uint32_t { return m.byte(o); };
    L4Hdr h = {P_NONE, 0, 0, 0, 0, 0, 0, 0};
    if (broken) {
        h.st = SMOL_ST_MALFORMED;
    } else {
        const uint32_t pr = h.key_proto = rb(k0.a + 9);
        if (raw) {
            h.st = SMOL_ST_UNSUPPORTED;
        } else if (pr == P_UDP) {
            h.fo = 6;
            const uint32_t ul = T >= 8 ? (dg(4) << 8 | dg(5)) : 0u;
            if (T < 8 || T < ul || ul < 8) h.st = SMOL_ST_MALFORMED;
            else if (!EMIT && (dg(2) | dg(3)) == 0) h.st = SMOL_ST_MALFORMED;  // udp.rs:246-248
            h.span_end = ul;
            if (!h.st) {
                h.l4_off = 8;
                h.l4_len = ul - 8;
            }
        } else if (pr == P_TCP) {
            h.fo = 16;
            const uint32_t thl = T >= 20 ? (dg(12) >> 4) * 4 : 0u;
            if (T < 20 || T < thl || thl < 20) h.st = SMOL_ST_MALFORMED;
            else if (!EMIT && ((dg(0) | dg(1)) == 0 || (dg(2) | dg(3)) == 0)) h.st = SMOL_ST_MALFORMED;  // tcp.rs:910-915
            h.span_end = T;
            if (!h.st) {
                h.l4_off = thl;
                h.l4_len = T - thl;
            }
        } else if (pr == P_ICMP4 || pr == P_IGMP) {
            h.fo = 2;
            if (T < 8) h.st = SMOL_ST_MALFORMED;
            h.span_end = T;
            if (EMIT && pr == P_ICMP4 && T >= 28) {
                const uint32_t t = dg(0), v = dg(8);
                if ((t == 3 || t == 11) && (v >> 4) == 4 && (v & 0x0fu) * 4 >= 20 && 8 + (v & 0x0fu) * 4 <= T)
                    h.in_hl = (v & 0x0fu) * 4;
            }
        } else {
            h.st = SMOL_ST_UNSUPPORTED;
        }
        if (!h.st) h.proto = pr;
    }
    return h;
}

// The datagram's checksum from dat = data() of its summed bytes (the checksum fields taken as emit /
// verify takes them): the pseudo-header of UDP / TCP from the key's addresses, combine(), and the caps
// that gate the protocol.
struct L4Sum {
    uint32_t ph, comb, gate;
    bool pseudo;
};
__device__ __forceinline__ L4Sum l4_sum(const KParams& p, const Key& k0, const L4Hdr& h, uint32_t T, uint32_t dat) {
    L4Sum s;
    uint32_t psum = 0;
    s.ph = 0;
    s.pseudo = h.proto == P_UDP || h.proto == P_TCP;
    if (s.pseudo) {
        for (uint32_t b = 12; b < 20; b += 2) psum += rb16(k0.a + b);
        s.ph = fold32(psum + h.proto + ((h.proto == P_UDP ? h.span_end : T) & 0xffffu));  // pseudo_header_v4
    }
    s.comb = s.pseudo ? fold32(s.ph + dat) : dat;
    s.gate = h.proto == P_UDP ? p.caps_udp : h.proto == P_TCP ? p.caps_tcp
           : h.proto == P_ICMP4 ? p.caps_icmpv4 : (uint32_t)SMOL_CHECKSUM_NONE;
    return s;
}

// Verify's verdict on the sum; field: the checksum field as the datagram carries it.  A group that sums
// nothing keeps the initial verdict {1, 1, 0}.
struct Verdict {
    uint32_t l4_valid, l4_ok, partial;
};
__device__ __forceinline__ Verdict l4_verdict(const L4Sum& s, uint32_t proto, uint32_t field) {
    Verdict v = {1, 1, 0};
    v.l4_valid = s.comb == 0xffffu;
    if (proto == P_UDP && field == 0) v.l4_valid = 1;  // udp.rs:138-140
    if (s.pseudo) v.partial = s.ph == field;
    v.l4_ok = caps_rx(s.gate) ? v.l4_valid : 1u;
    return v;
}

// A fragment's status byte from its map bits, the group's L4 status and verdict; all_ip: every
// fragment of the group passed the IP gate.
template <bool EMIT>
__device__ __forceinline__ uint32_t frag_status(uint32_t bits, uint32_t st, const Verdict& v, bool all_ip) {
    if (EMIT) return (bits & 1u) ? st : (uint32_t)SMOL_ST_MALFORMED;
    const bool mal = (st & SMOL_ST_MALFORMED) != 0;
    return st | ((bits & 4u) ? SMOL_ST_IP_OK : 0u) | ((bits & 8u) ? SMOL_ST_IP_VALID : 0u) |
           ((bits & 1u) ? 0u : (uint32_t)SMOL_ST_MALFORMED) |
           (v.l4_ok ? SMOL_ST_L4_OK : 0u) | (v.l4_valid ? SMOL_ST_L4_VALID : 0u) |
           (v.partial ? SMOL_ST_L4_PARTIAL : 0u) | ((all_ip && v.l4_ok && !mal) ? SMOL_ST_ACCEPT : 0u);
}

}  // namespace fraggroup
}  // namespace smolcsum
