// smoltcp_checksum.hpp — C++ host-side mirror of the reference interface over the C ABI.
//
// The reference is Rust and this image has no Rust toolchain, so the host side above the C ABI
// (include/smolcsum.h) is this header: the same names, argument meanings and error behaviour as
//
//   smoltcp::wire::checksum::{data, combine, pseudo_header_v4, pseudo_header_v6, pseudo_header}
//                                                            (src/wire/ip.rs:762-869)
//   smoltcp::phy::{Checksum, ChecksumCapabilities}           (src/phy/mod.rs:173-234)
//
// plus the batched engine (`smoltcp_amd::Engine`, one device context) that a checksum-offloading
// `phy::Device` drives: `emit` for TxToken::consume, `verify` before an RxToken is handed out.
// Errors become `smoltcp_amd::Error` exceptions here, on the C++ side; none crosses the C ABI.
// `pseudo_header` throws where the reference panics (`unreachable!()`, ip.rs:866).
//
// Header-only; link with -lsmolcsum (smoltcp_amd/libsmolcsum.so).  Device pointers are plain
// `hipMalloc` pointers and streams are `hipStream_t` passed as `void*`, so this header needs no
// HIP include.
#pragma once

#include <cstddef>
#include <cstdint>
#include <span>
#include <stdexcept>
#include <string>

#include "../../include/smolcsum.h"

namespace smoltcp_amd {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
    int code() const noexcept { return code_; }

private:
    int code_;
};

inline void check(int rc, const char* what) {
    if (rc == SMOL_OK) return;
    std::string msg = std::string(what) + " failed (" + std::to_string(rc) + ")";
    if (rc == SMOL_EHIP) msg += ": " + std::string(smol_csum_last_error());
    throw Error(rc, msg);
}

}  // namespace smoltcp_amd

namespace smoltcp {

// ---- wire::checksum (src/wire/ip.rs:762-869) --------------------------------------------------
namespace wire::checksum {

// checksum::data (ip.rs:773-804)
inline uint16_t data(std::span<const uint8_t> bytes) { return smol_csum_data(bytes.data(), bytes.size()); }

// checksum::combine (ip.rs:807-813)
inline uint16_t combine(std::span<const uint16_t> checksums) {
    return smol_csum_combine(checksums.data(), checksums.size());
}

// checksum::pseudo_header_v4 (ip.rs:816-831)
inline uint16_t pseudo_header_v4(const uint8_t (&src)[4], const uint8_t (&dst)[4], uint8_t next_header,
                                 uint32_t length) {
    return smol_csum_pseudo_header_v4(src, dst, next_header, length);
}

// checksum::pseudo_header_v6 (ip.rs:834-849)
inline uint16_t pseudo_header_v6(const uint8_t (&src)[16], const uint8_t (&dst)[16], uint8_t next_header,
                                 uint32_t length) {
    return smol_csum_pseudo_header_v6(src, dst, next_header, length);
}

// checksum::pseudo_header (ip.rs:851-869): an address is 4 (IPv4) or 16 (IPv6) bytes.
inline uint16_t pseudo_header(std::span<const uint8_t> src, std::span<const uint8_t> dst, uint8_t next_header,
                              uint32_t length) {
    auto fam = [](size_t n) { return n == 4 ? 4 : n == 16 ? 6 : 0; };
    uint16_t out = 0;
    int rc = smol_csum_pseudo_header(fam(src.size()), src.data(), fam(dst.size()), dst.data(), next_header,
                                     length, &out);
    if (rc == SMOL_EINVAL) throw smoltcp_amd::Error(rc, "pseudo_header: address family mismatch");
    smoltcp_amd::check(rc, "smol_csum_pseudo_header");
    return out;
}

// checksum::format_checksum (ip.rs:871-886): the annotation the packet pretty-printers append.
inline const char* format_checksum(bool correct, bool partially_correct) {
    if (correct) return "";
    return partially_correct ? " (partial checksum correct)" : " (checksum incorrect)";
}

// The annotations of one verify status byte (SMOL_ST_*): the IPv4 header line
// (Ipv4Packet pretty_print, ipv4.rs:698: format_checksum(verify_checksum(), false)) and the
// UDP / TCP line (pretty_print_ip_payload, ip.rs:930-962: verify_checksum() and
// verify_partial_checksum()).
inline const char* ipv4_annotation(uint8_t status) { return format_checksum(status & SMOL_ST_IP_VALID, false); }
inline const char* l4_annotation(uint8_t status) {
    return format_checksum(status & SMOL_ST_L4_VALID, status & SMOL_ST_L4_PARTIAL);
}

}  // namespace wire::checksum

// ---- phy::Checksum / phy::ChecksumCapabilities (src/phy/mod.rs:173-234) -------------------------
namespace phy {

enum class Checksum : uint8_t {
    Both = SMOL_CHECKSUM_BOTH,  // the default (mod.rs:178)
    Rx = SMOL_CHECKSUM_RX,
    Tx = SMOL_CHECKSUM_TX,
    None = SMOL_CHECKSUM_NONE,
};

// Checksum::rx / Checksum::tx (mod.rs:188-203)
constexpr bool rx(Checksum c) { return c == Checksum::Both || c == Checksum::Rx; }
constexpr bool tx(Checksum c) { return c == Checksum::Both || c == Checksum::Tx; }

struct ChecksumCapabilities {
    Checksum ipv4 = Checksum::Both;
    Checksum udp = Checksum::Both;
    Checksum tcp = Checksum::Both;
    Checksum icmpv4 = Checksum::Both;
    Checksum icmpv6 = Checksum::Both;

    // ChecksumCapabilities::ignored (mod.rs:223-233): the device does all checksum work.
    static constexpr ChecksumCapabilities ignored() {
        return {Checksum::None, Checksum::None, Checksum::None, Checksum::None, Checksum::None};
    }

    smol_checksum_caps_t c() const {
        smol_checksum_caps_t r{};
        r.ipv4 = uint8_t(ipv4);
        r.udp = uint8_t(udp);
        r.tcp = uint8_t(tcp);
        r.icmpv4 = uint8_t(icmpv4);
        r.icmpv6 = uint8_t(icmpv6);
        return r;
    }
};

}  // namespace phy
}  // namespace smoltcp

namespace smoltcp_amd {

enum class Medium : uint8_t { Raw = SMOL_KIND_RAW, Ip = SMOL_KIND_IP, Ethernet = SMOL_KIND_ETH };

// Record geometry of one batch: a fixed stride, or a device array of descriptors.
struct Batch {
    const smol_csum_desc_t* d_desc = nullptr;
    uint64_t n = 0;
    uint64_t stride = 0;
    uint32_t len = 0;
    Medium kind = Medium::Ip;
    uint8_t flags = 0;  // SMOL_REC_* of every record (fixed stride; descriptors carry their own)

    static Batch fixed(uint64_t n, uint64_t stride, uint32_t len, Medium kind = Medium::Ip, uint8_t flags = 0) {
        return Batch{nullptr, n, stride, len, kind, flags};
    }
    static Batch described(const smol_csum_desc_t* d_desc, uint64_t n) { return Batch{d_desc, n, 0, 0, Medium::Ip, 0}; }

    smol_csum_batch_t c() const {
        smol_csum_batch_t b{};
        b.desc = d_desc;
        b.n = n;
        b.stride = stride;
        b.len = len;
        b.kind = uint8_t(kind);
        b.flags = flags;
        return b;
    }
};

// One device context (not thread-safe: one Engine per host thread).  Every call is asynchronous
// on `stream`; buffers are device pointers owned by the caller.
class Engine {
public:
    explicit Engine(int device = 0) { check(smol_csum_ctx_create(device, &ctx_), "smol_csum_ctx_create"); }
    ~Engine() {
        if (ctx_) smol_csum_ctx_destroy(ctx_);
    }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    Engine(Engine&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }

    // Repr::emit checksum gates, in place (d_status nullable: MALFORMED / UNSUPPORTED bits).
    void emit(uint8_t* d_buf, const Batch& b, const smoltcp::phy::ChecksumCapabilities& caps = {},
              uint8_t* d_status = nullptr, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_emit(ctx_, d_buf, &bc, &cc, d_status, stream), "smol_csum_batch_emit");
    }

    // Emit's values without the writes: d_fields[i] = record i's field offsets, values and status
    // (16-byte aligned device array); d_buf is only read.  The frames stay in host memory and
    // smol_csum_apply_fields patches them there, two bytes per field as the reference's fill_checksum
    // (udp.rs:194-208, tcp.rs:616-626, ipv4.rs:506-513).
    void emit_fields(const uint8_t* d_buf, const Batch& b, smol_csum_fields_t* d_fields,
                     const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_emit_fields(ctx_, d_buf, &bc, &cc, d_fields, stream), "smol_csum_batch_emit_fields");
    }

    // TcpRepr/UdpRepr::emit's "copy the payload, then fill": d_copy[i] moves record i's payload
    // from d_src into the record, then the checksums are emitted, in one pass.
    void copy_emit(uint8_t* d_buf, const Batch& b, const uint8_t* d_src, const smol_csum_copy_t* d_copy,
                   const smoltcp::phy::ChecksumCapabilities& caps = {}, uint8_t* d_status = nullptr,
                   void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_copy_emit(ctx_, d_buf, &bc, d_src, d_copy, &cc, d_status, stream),
              "smol_csum_batch_copy_emit");
    }

    // Repr::parse checksum gates: d_status[i] = SMOL_ST_* bits.
    void verify(const uint8_t* d_buf, const Batch& b, uint8_t* d_status,
                const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify(ctx_, d_buf, &bc, &cc, d_status, stream), "smol_csum_batch_verify");
    }

    // verify, and in the same pass every record's UDP / TCP payload delivered to d_dst at d_slots[i]
    // (UdpPacket::payload udp.rs:153-157 / TcpPacket::payload tcp.rs:419-423, the copy of
    // socket/udp.rs:522-523 and socket/tcp.rs:2231); d_spans[i] = the span and whether it was copied.  The
    // copy does not wait for the verdict: commit a slot only when d_status[i] & SMOL_ST_ACCEPT.
    void verify_copy(const uint8_t* d_buf, const Batch& b, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                     uint8_t* d_status, smol_csum_span_t* d_spans,
                     const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_copy(ctx_, d_buf, &bc, &cc, d_dst, d_slots, d_status, d_spans, stream),
              "smol_csum_batch_verify_copy");
    }

    // IPv4 fragment groups: d_groups[k] = one datagram's fragments (consecutive records).  Fills every
    // fragment header and each datagram's L4 checksum over its reassembled payload (the iface's
    // "emit whole, then fragment", src/iface/interface/mod.rs:1276-1331).
    void emit_frag(uint8_t* d_buf, const Batch& b, const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                   const smoltcp::phy::ChecksumCapabilities& caps = {}, uint8_t* d_status = nullptr,
                   void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_emit_frag(ctx_, d_buf, &bc, d_groups, n_groups, &cc, d_status, stream),
              "smol_csum_batch_emit_frag");
    }
    // Fragment headers + the reassembled datagram's L4 gate (src/iface/interface/ipv4.rs:103-146).
    void verify_frag(const uint8_t* d_buf, const Batch& b, const smol_csum_frag_group_t* d_groups,
                     uint64_t n_groups, uint8_t* d_status, const smoltcp::phy::ChecksumCapabilities& caps = {},
                     void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_frag(ctx_, d_buf, &bc, d_groups, n_groups, &cc, d_status, stream),
              "smol_csum_batch_verify_frag");
    }
    // verify_frag, and in the same pass every usable group's fragment payloads put together at d_slots[k] of
    // d_dst (PacketAssembler::add's copy, src/iface/fragmentation.rs:139-151); d_dgrams[k] = the datagram's
    // length, protocol, L4 payload span and whether it was copied.  d_slots / d_dgrams: one per GROUP,
    // d_status: one per record.  The copy waits for no verdict: commit a slot only when every status byte of
    // its group has SMOL_ST_ACCEPT.
    void verify_reassemble(const uint8_t* d_buf, const Batch& b, const smol_csum_frag_group_t* d_groups,
                           uint64_t n_groups, uint8_t* d_dst, const smol_csum_slot_t* d_slots, uint8_t* d_status,
                           smol_csum_dgram_t* d_dgrams, const smoltcp::phy::ChecksumCapabilities& caps = {},
                           void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_reassemble(ctx_, d_buf, &bc, d_groups, n_groups, &cc, d_dst, d_slots, d_status,
                                                d_dgrams, stream),
              "smol_csum_batch_verify_reassemble");
    }
    // emit, and in the same pass every whole IPv4 datagram cut into the frames the iface sends (dispatch_ip's
    // first fragment, src/iface/interface/mod.rs:1276-1347, and dispatch_ipv4_frag's others, ipv4.rs:421-482),
    // at d_plans[i].dst_offset of d_dst, frame k at + k * frame_stride (0: back to back); d_out[i] = the frame
    // count and lengths, emit's status byte and whether the frames were stored.  d_plans / d_out: one per
    // record.  d_buf is only read.
    void fragment_emit(const uint8_t* d_buf, const Batch& b, uint8_t* d_dst, const smol_csum_fragplan_t* d_plans,
                       smol_csum_fragout_t* d_out, uint32_t frame_stride = 0,
                       const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_fragment_emit(ctx_, d_buf, &bc, &cc, d_dst, d_plans, frame_stride, d_out, stream),
              "smol_csum_batch_fragment_emit");
    }
    // emit, and in the same pass every TCP send cut into MSS-sized segments (the burst of TcpSocket::dispatch
    // calls within one poll, src/socket/tcp.rs:2620-2687): record i is the header template, d_plans[i] its
    // payload range in d_src, its MSS and its place in d_dst, frame k at + k * frame_stride (0: back to
    // back); d_out[i] = the frame count and lengths, emit's status byte and whether the frames were stored.
    // d_plans / d_out: one per record.  d_buf and d_src are only read.
    void tcp_segment_emit(const uint8_t* d_buf, const Batch& b, const uint8_t* d_src, uint8_t* d_dst,
                          const smol_csum_tcpplan_t* d_plans, smol_csum_tcpout_t* d_out, uint32_t frame_stride = 0,
                          const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_tcp_segment_emit(ctx_, d_buf, &bc, &cc, d_src, d_dst, d_plans, frame_stride, d_out, stream),
              "smol_csum_batch_tcp_segment_emit");
    }
    // verify, and in the same pass every TCP segment's payload put at the place its sequence number gives it
    // in its connection's receive ring, trimmed to the receive window (TcpSocket::process' segment_in_window,
    // trim and rx_buffer.write_unallocated, src/socket/tcp.rs:1705-1783, 2205-2241): group k is one
    // connection's frames of this poll in arrival order, d_wins[k] its ring and window; d_segs[i] = record i's
    // sequence number, window range and SMOL_SEG_* flags, d_flows[k] = how far the in-order data now reaches
    // (what enqueue_unallocated gets).  d_wins / d_flows: one per GROUP, d_status / d_segs: one per record.
    // The copy waits for no verdict; d_buf is only read.
    void verify_tcp_assemble(const uint8_t* d_buf, const Batch& b, const smol_csum_frag_group_t* d_groups,
                             uint64_t n_groups, uint8_t* d_dst, const smol_csum_tcpwin_t* d_wins, uint8_t* d_status,
                             smol_csum_tcpseg_t* d_segs, smol_csum_tcpflow_t* d_flows,
                             const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_tcp_assemble(ctx_, d_buf, &bc, d_groups, n_groups, &cc, d_dst, d_wins, d_status,
                                                  d_segs, d_flows, stream),
              "smol_csum_batch_verify_tcp_assemble");
    }

    // verify, and in the same pass the reply to every ICMPv4 / ICMPv6 echo request the wire-level address rule
    // answers written to d_dst at d_slots[i]: fresh Ethernet / IP / ICMP head, the request's data, both
    // checksums filled under `caps` (the iface's responder: process_icmpv4 src/iface/interface/ipv4.rs:320-371,
    // process_icmpv6 ipv6.rs:399-416, icmpv4_reply / icmpv6_reply and the reply's dispatch).  d_echo[i] = the
    // reply's length, the data's offset and SMOL_ECHO_* flags; cfg: nullptr, or the iface's directed-broadcast
    // address.  Transmit a slot only when its entry has SMOL_ECHO_SEND; SMOL_ECHO_HOST marks the requests the
    // host answers itself.  The copy waits for no verdict; d_buf is only read.
    void verify_echo_reply(const uint8_t* d_buf, const Batch& b, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                           uint8_t* d_status, smol_csum_echo_t* d_echo, const smol_csum_echo_cfg_t* cfg = nullptr,
                           const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_echo_reply(ctx_, d_buf, &bc, &cc, cfg, d_dst, d_slots, d_status, d_echo, stream),
              "smol_csum_batch_verify_echo_reply");
    }

    // verify, and in the same pass the ICMP error for every datagram nobody takes that the wire-level address
    // rule answers written to d_dst at d_slots[i]: Destination Unreachable / Port Unreachable for a UDP datagram
    // whose destination port's bit in d_udp_open is clear (process_udp, src/iface/interface/udp.rs:49-77),
    // Protocol Unreachable for an unhandled IPv4 protocol (ipv4.rs:240-250), Parameter Problem for an
    // unrecognised IPv6 next header (process_nxt_hdr ipv6.rs:352-364); both headers fresh, the first 528 / 1192
    // payload bytes quoted, every checksum filled under `caps`.  d_udp_open: nullptr (no UDP datagram is
    // refused), or 8192 bytes, bit p & 7 of byte p >> 3 set for every port the host wants itself; a host with a
    // socket that matches on something other than the destination port (the DNS socket) passes nullptr or sets
    // every bit.  Transmit a slot only when its entry has SMOL_UNR_SEND; SMOL_UNR_HOST marks the replies the
    // host builds itself.  The copy waits for no verdict; d_buf and d_udp_open are only read.
    void verify_unreach_reply(const uint8_t* d_buf, const Batch& b, const uint8_t* d_udp_open, uint8_t* d_dst,
                              const smol_csum_slot_t* d_slots, uint8_t* d_status, smol_csum_unreach_t* d_unr,
                              const smol_csum_echo_cfg_t* cfg = nullptr,
                              const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_unreach_reply(ctx_, d_buf, &bc, &cc, cfg, d_udp_open, d_dst, d_slots, d_status, d_unr,
                                                   stream),
              "smol_csum_batch_verify_unreach_reply");
    }

    // verify, and in the same pass every UDP datagram's payload stored where its socket's PacketBuffer::enqueue
    // places it (src/storage/packet_buffer.rs:80-118), the metadata entries written: UdpSocket::process'
    // rx_buffer.enqueue and copy_from_slice (src/socket/udp.rs:492-529) behind UdpRepr::parse's sum.  A group is
    // the frames the caller routed to one socket in this poll, in arrival order; d_socks[g] is that socket's ring
    // state before the poll and its port, d_out[g] the state after it.  d_status and d_rx are per record, d_meta
    // holds the metadata rings.  The copy waits for no verdict: commit by copying d_out[g]'s four state words
    // into the PacketBuffer.  d_buf is only read.
    void verify_udp_enqueue(const uint8_t* d_buf, const Batch& b, const smol_csum_frag_group_t* d_groups,
                            uint64_t n_groups, uint8_t* d_dst, const smol_csum_udpsock_t* d_socks,
                            smol_csum_udpmeta_t* d_meta, uint8_t* d_status, smol_csum_udprx_t* d_rx,
                            smol_csum_udpsockout_t* d_out, const smoltcp::phy::ChecksumCapabilities& caps = {},
                            void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_verify_udp_enqueue(ctx_, d_buf, &bc, d_groups, n_groups, &cc, d_dst, d_socks, d_meta, d_status,
                                                 d_rx, d_out, stream),
              "smol_csum_batch_verify_udp_enqueue");
    }

    // The send-side mirror: every socket's transmit PacketBuffer dequeued in order (tx_buffer.dequeue_with,
    // src/storage/packet_buffer.rs:169-204) and each datagram written to d_dst as a whole frame, Ethernet (with
    // SMOL_UTXS_ETH), IP and UDP headers built on the device from d_socks[g] and the metadata entry, checksums
    // filled under `caps`, in the pass that copies the payload: UdpSocket::dispatch (src/socket/udp.rs:535-592)
    // for a burst.  A group is one socket; there is no batch.  d_meta entries are read with their send-side
    // meaning (remote_addr / src_port: where to send; local_addr: what to send from), which is what
    // verify_udp_enqueue writes, so a receive ring can be answered unchanged.  d_tx gets one entry per dequeued
    // datagram from d_socks[g].tx_first on, d_out[g] the ring state after the call: commit by copying its four
    // state words into the PacketBuffer.  OVERSIZE datagrams are dequeued and not written: fragment the IPv4
    // ones with fragment_emit before reusing the ring space.  d_src, d_socks and d_meta are only read.
    void udp_dequeue_emit(const uint8_t* d_src, const smol_csum_udptxsock_t* d_socks, uint64_t n_groups,
                          const smol_csum_udpmeta_t* d_meta, uint8_t* d_dst, uint32_t frame_stride,
                          smol_csum_udptx_t* d_tx, smol_csum_udptxout_t* d_out,
                          const smoltcp::phy::ChecksumCapabilities& caps = {}, void* stream = nullptr) {
        auto cc = caps.c();
        check(smol_csum_batch_udp_dequeue_emit(ctx_, d_src, d_socks, n_groups, d_meta, &cc, d_dst, frame_stride, d_tx, d_out,
                                               stream),
              "smol_csum_batch_udp_dequeue_emit");
    }

    // 6LoWPAN NHC UDP (sixlowpan::nhc::UdpNhcRepr::emit / ::parse): every record is a LOWPAN_NHC
    // UDP packet; d_addrs[i] holds record i's IPv6 addresses (IPHC-decompressed).
    void nhc_udp_emit(uint8_t* d_buf, const Batch& b, const smol_ipv6_addr_pair_t* d_addrs,
                      const smoltcp::phy::ChecksumCapabilities& caps = {}, uint8_t* d_status = nullptr,
                      void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_nhc_udp_emit(ctx_, d_buf, &bc, d_addrs, &cc, d_status, stream),
              "smol_csum_batch_nhc_udp_emit");
    }
    void nhc_udp_verify(const uint8_t* d_buf, const Batch& b, const smol_ipv6_addr_pair_t* d_addrs,
                        uint8_t* d_status, const smoltcp::phy::ChecksumCapabilities& caps = {},
                        void* stream = nullptr) {
        auto bc = b.c();
        auto cc = caps.c();
        check(smol_csum_batch_nhc_udp_verify(ctx_, d_buf, &bc, d_addrs, &cc, d_status, stream),
              "smol_csum_batch_nhc_udp_verify");
    }

    // checksum::data over every record span.
    void data(const uint8_t* d_buf, const Batch& b, uint16_t* d_out, void* stream = nullptr) {
        auto bc = b.c();
        check(smol_csum_batch_data(ctx_, d_buf, &bc, d_out, stream), "smol_csum_batch_data");
    }


    smol_csum_ctx_t* handle() const { return ctx_; }

private:
    smol_csum_ctx_t* ctx_ = nullptr;
};

constexpr bool accepted(uint8_t status) { return (status & SMOL_ST_ACCEPT) != 0; }

}  // namespace smoltcp_amd
