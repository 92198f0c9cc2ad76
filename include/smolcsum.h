/*
 * smolcsum.h — C ABI of the MI355X (gfx950) Internet-checksum engine.
 *
 * This is the drop-in boundary for the one hot path of smoltcp 0.13.1 that this repository
 * accelerates: the RFC 1071 one's-complement checksum of `smoltcp::wire::checksum` and the
 * per-protocol emit/verify gates built on it.  Every entry point below names the reference
 * interface it replaces (paths relative to the smoltcp source tree).
 *
 * Two groups of entry points:
 *
 *  1. Scalar host mirrors of `smoltcp::wire::checksum` (src/wire/ip.rs:762-869).  Bit-identical
 *     results, same argument meaning, host memory, synchronous.  A Rust `extern "C"` binding
 *      can route `checksum::data` & co. here unchanged.
 *
 *  2. Batched device entry points.  One contiguous DEVICE buffer holds many records (IP packets,
 *     Ethernet frames or raw spans); a record is either described by a descriptor array (device
 *     memory) or implied by a fixed stride.  Each call is asynchronous and stream-ordered on the
 *     HIP stream passed in; the caller owns every buffer.  The engine reads the IP header inside
 *     the record to find the protocol, the L4 span and the pseudo-header addresses, exactly as
 *     smoltcp's iface does before it calls the per-protocol gates:
 *       - smol_csum_batch_emit   == the checksum part of Ipv4Repr/UdpRepr/TcpRepr/Icmpv4Repr/
 *         Icmpv6Repr/IgmpRepr::emit under `caps` (fill when caps.X.tx(), else write 0);
 *       - smol_csum_batch_verify == the checksum gates of the matching Repr::parse under `caps`
 *         (verify when caps.X.rx()), reported as one status byte per record;
 *       - smol_csum_batch_emit_fields == emit's values without the writes: one 16-byte entry per
 *         record (field offsets, values, status) for a caller whose frames stay in host memory and
 *         who patches them there with smol_csum_apply_fields;
 *       - smol_csum_batch_verify_copy == verify, and in the same pass the UDP / TCP payloads
 *         delivered to caller-chosen slots of a second device buffer (the socket's rx_buffer copy);
 *       - smol_csum_batch_verify_reassemble == verify over IPv4 fragment groups, and in the same pass
 *         the fragment payloads put together in the datagram's slot (the reassembler's copy);
 *       - smol_csum_batch_fragment_emit == emit over whole IPv4 datagrams, and in the same pass each
 *         datagram cut into the frames the iface sends (dispatch_ip's and dispatch_ipv4_frag's copy);
 *       - smol_csum_batch_tcp_segment_emit == emit over TCP header templates, and in the same pass each
 *         send's payload cut into MSS-sized segments behind them (TcpSocket::dispatch's burst);
 *       - smol_csum_batch_verify_tcp_assemble == verify over the frames of TCP connections, and in the
 *         same pass each segment's payload put at its sequence number's place in the connection's
 *         receive ring, trimmed to the window (TcpSocket::process' write_unallocated);
 *       - smol_csum_batch_verify_echo_reply == verify, and in the same pass the reply to every ICMP echo
 *         request written to a caller-chosen slot, head fresh, data echoed, checksums filled (the
 *         iface's own responder, process_icmpv4 / process_icmpv6 and the dispatch of their reply);
 *       - smol_csum_batch_verify_unreach_reply == verify, and in the same pass the ICMP error for every
 *         datagram nobody takes (a closed UDP port, an unhandled protocol or next header) written to a
 *         caller-chosen slot, both headers fresh, the payload quoted, checksums filled;
 *       - smol_csum_batch_verify_udp_enqueue == verify over the frames of UDP sockets, and in the same
 *         pass each datagram's payload put where the socket's PacketBuffer::enqueue places it, metadata
 *         entries written (UdpSocket::process' rx_buffer.enqueue and copy_from_slice);
 *       - smol_csum_batch_udp_dequeue_emit == emit over the frames of UDP sockets' queued datagrams, the
 *         frames themselves built in the same pass: the transmit PacketBuffer dequeued, the headers
 *         written, the payload copied once (UdpSocket::dispatch's tx_buffer.dequeue_with and emit);
 *       - smol_csum_batch_data  == checksum::data() over each raw span.
 *     A device that offloads checksums (phy::Device with ChecksumCapabilities::ignored(),
 *     src/phy/mod.rs:223-233) runs emit in TxToken::consume and verify before yielding an
 *     RxToken, with the stack's default caps (Checksum::Both).
 *
 * Errors: every function returning int returns SMOL_OK (0) or a negative SMOL_E* code.  No C++
 * exception crosses this boundary.  There is no CPU fallback for the batched calls: with no
 * usable HIP device they return SMOL_ENODEV.
 *
 * Threading: a context belongs to one device and one host thread at a time (not thread-safe);
 * use one context per host thread.  Calls on the same stream are ordered.
 */
#ifndef SMOLCSUM_H
#define SMOLCSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMOLCSUM_ABI_VERSION 6

/* ---- error codes ------------------------------------------------------------------------ */
enum {
    SMOL_OK = 0,
    SMOL_EINVAL = -1,  /* bad argument: NULL pointer with n > 0, unknown kind, bad caps value   */
    SMOL_ENODEV = -2,  /* no HIP device, or the device ordinal is out of range                   */
    SMOL_EHIP = -3,    /* a HIP runtime call failed; smol_csum_last_error() gives the message    */
    SMOL_ERANGE = -4,  /* a size limit was exceeded (record longer than SMOL_MAX_RECORD_LEN)     */
    SMOL_ENOMEM = -5   /* host allocation failed                                                 */
};

/* Longest record the batched kernels accept.  Protocol records never exceed 65535 + 14 bytes
 * (u16 length fields); raw data() spans may be up to 1 GiB.  data() stays bit-exact with the
 * reference's release-mode u32 wrap-around for spans longer than 131074 bytes (src/wire/ip.rs:776). */
#define SMOL_MAX_RECORD_LEN (1u << 30)

/* ---- policy: mirrors phy::Checksum / phy::ChecksumCapabilities (src/phy/mod.rs:176-218) --- */
typedef enum {
    SMOL_CHECKSUM_BOTH = 0, /* Checksum::Both (the default, src/phy/mod.rs:178) */
    SMOL_CHECKSUM_RX = 1,   /* Checksum::Rx */
    SMOL_CHECKSUM_TX = 2,   /* Checksum::Tx */
    SMOL_CHECKSUM_NONE = 3  /* Checksum::None */
} smol_checksum_t;

/* Field order and meaning of ChecksumCapabilities {ipv4, udp, tcp, icmpv4, icmpv6}.  Each byte is
 * a smol_checksum_t.  IGMP has no entry in the reference: IgmpRepr::emit always fills
 * (src/wire/igmp.rs:293) and IgmpRepr::parse never verifies (src/wire/igmp.rs:204-248); the
 * batched calls do the same. */
typedef struct {
    uint8_t ipv4;
    uint8_t udp;
    uint8_t tcp;
    uint8_t icmpv4;
    uint8_t icmpv6;
    uint8_t reserved[3]; /* must be 0 */
} smol_checksum_caps_t;

/* ---- record kinds ----------------------------------------------------------------------- */
enum {
    SMOL_KIND_RAW = 0, /* a plain byte span: only smol_csum_batch_data is meaningful            */
    SMOL_KIND_IP = 1,  /* an IPv4 or IPv6 packet (Medium::Ip); version from the first nibble     */
    SMOL_KIND_ETH = 2  /* an Ethernet II frame (Medium::Ethernet) carrying IPv4 (0x0800) or IPv6
                          (0x86DD); other ethertypes are reported SMOL_ST_UNSUPPORTED           */
};

/* One record of a batch (16 bytes, device memory).  `len` is the number of bytes the device
 * buffer holds for this record (the Rx/Tx token buffer length); the IP length fields inside the
 * record decide the spans that are summed, exactly as in the reference. */
typedef struct {
    uint64_t offset; /* byte offset of the record from the batch base pointer (any alignment) */
    uint32_t len;    /* record length in bytes, <= SMOL_MAX_RECORD_LEN                         */
    uint8_t kind;    /* SMOL_KIND_*                                                            */
    uint8_t flags;   /* SMOL_REC_* (0 for an ordinary record); other bits must be 0            */
    uint16_t reserved;
} smol_csum_desc_t;

/* Record flags (smol_csum_desc_t.flags, or smol_csum_batch_t.flags for every record of a
 * fixed-stride batch).
 *
 * SMOL_REC_IPHDR_ONLY — a raw-socket frame.  A raw socket's L4 bytes go out as the user wrote
 * them: dispatch copies IpPayload::Raw verbatim (src/iface/packet.rs:132-136) and only the IPv4
 * header is emitted by the stack (Ipv4Repr::emit under caps.ipv4, src/socket/raw.rs:406-423).  On
 * receive the raw socket sees the packet after the IPv4 header gate and before any L4 gate
 * (src/iface/interface/ipv4.rs:150-151).  So for such a record emit fills (or zeroes) the IPv4
 * header checksum only and never touches a byte past the IP header; verify applies the IPv4
 * header gate only.  The record is reported SMOL_ST_UNSUPPORTED (no L4 checksum on its path), or
 * SMOL_ST_MALFORMED when its IP header fails check_len.  In a fragment group the flag on any of
 * the group's records makes the whole datagram raw. */
#define SMOL_REC_IPHDR_ONLY 0x01u

/* Batch flag (smol_csum_batch_t.flags, fixed-stride and descriptor batches alike; ABI 5).
 *
 * SMOL_BATCH_FIELD_STORES — emit writes the checksum fields only (2-byte stores), never a whole
 * 64-byte segment around them.  By default emit rewrites such segments, neighbouring records'
 * bytes included, with the values it read (smol_csum_batch_emit below): a caller that writes other
 * bytes of the batch's records from another stream while emit runs sets this flag.  Slower (one
 * partial-line write per field). */
#define SMOL_BATCH_FIELD_STORES 0x80u

/* Batch geometry (host memory).  If `desc` is non-NULL it is a DEVICE array of `n` descriptors
 * and `stride`/`len`/`kind` are ignored.  Otherwise record i starts at base + i*stride, has
 * length `len` and kind `kind` (the fixed-size case: no descriptor traffic at all). */
typedef struct {
    const smol_csum_desc_t* desc;
    uint64_t n;
    uint64_t stride;
    uint32_t len;
    uint8_t kind;
    uint8_t flags;       /* SMOL_REC_* for every record of a fixed-stride batch (ignored with desc) */
    uint8_t reserved[2]; /* must be 0 */
} smol_csum_batch_t;

/* ---- per-record status byte (verify; emit reports the MALFORMED/UNSUPPORTED bits) ------- */
enum {
    SMOL_ST_IP_OK = 0x01,      /* IPv4 header gate passed: verified under caps.ipv4.rx(), or not
                                  checked (caps, IPv6, non-IP).  Ipv4Repr::parse, ipv4.rs:553   */
    SMOL_ST_L4_OK = 0x02,      /* L4 gate passed: verified under caps.X.rx(), or not checked
                                  (caps, IGMP, fragment, unsupported protocol)                    */
    SMOL_ST_L4_PARTIAL = 0x04, /* UDP/TCP verify_partial_checksum(): field == pseudo-header sum
                                  (udp.rs:112-119, tcp.rs:376-385)                              */
    SMOL_ST_IP_VALID = 0x08,   /* Ipv4Packet::verify_checksum() regardless of caps (1 if no
                                  IPv4 header)                                                   */
    SMOL_ST_L4_VALID = 0x10,   /* the L4 verify_checksum() regardless of caps (1 if no L4 span)  */
    SMOL_ST_MALFORMED = 0x20,  /* the reference's parse drops the packet before any checksum is
                                  looked at: a check_len() on the path failed, or (verify only) a
                                  port Repr::parse rejects first — UDP destination port 0
                                  (udp.rs:246-248), TCP source or destination port 0
                                  (tcp.rs:910-915) — or (verify only, ABI 6) the iface drops an
                                  IPv6 packet on its Hop-by-Hop options: an option that fails to
                                  parse, or an unknown option whose type asks for a discard
                                  (process_hopbyhop, iface/interface/ipv6.rs:282-313).  The L4 bits
                                  are then not evaluated (set).  Emit never rejects ports or
                                  options: Repr::emit does not check them.                       */
    SMOL_ST_UNSUPPORTED = 0x40,/* no L4 checksum on this record's path: IPv4 fragment, protocol
                                  smoltcp does not checksum, IPv6 next header other than a
                                  leading Hop-by-Hop + TCP/UDP/ICMPv6, non-IP ethertype          */
    SMOL_ST_ACCEPT = 0x80      /* IP_OK && L4_OK && !MALFORMED: the checksum gates pass         */
};

/* ---- 1. scalar host mirrors of smoltcp::wire::checksum ---------------------------------- */

/* checksum::data — src/wire/ip.rs:773-804.  RFC 1071 sum without the final complement. */
uint16_t smol_csum_data(const uint8_t* data, size_t len);

/* checksum::combine — src/wire/ip.rs:807-813. */
uint16_t smol_csum_combine(const uint16_t* checksums, size_t n);

/* checksum::pseudo_header_v4 — src/wire/ip.rs:816-831.  `length` is truncated to u16 as in the
 * reference (NetworkEndian::write_u16(.., length as u16)). */
uint16_t smol_csum_pseudo_header_v4(const uint8_t src_addr[4], const uint8_t dst_addr[4],
                                    uint8_t next_header, uint32_t length);

/* checksum::pseudo_header_v6 — src/wire/ip.rs:834-849. */
uint16_t smol_csum_pseudo_header_v6(const uint8_t src_addr[16], const uint8_t dst_addr[16],
                                    uint8_t next_header, uint32_t length);

/* checksum::pseudo_header — src/wire/ip.rs:851-869.  `family` is 4 or 6 for each address; the
 * reference panics (unreachable!) on a family mismatch; this returns SMOL_EINVAL instead and
 * writes nothing. */
int smol_csum_pseudo_header(int src_family, const uint8_t* src_addr, int dst_family,
                            const uint8_t* dst_addr, uint8_t next_header, uint32_t length,
                            uint16_t* out);

/* ---- 2. batched device engine ----------------------------------------------------------- */

typedef struct smol_csum_ctx smol_csum_ctx_t;

/* Create a context bound to HIP device `device`.  Returns SMOL_ENODEV when no such device. */
int smol_csum_ctx_create(int device, smol_csum_ctx_t** out);
int smol_csum_ctx_destroy(smol_csum_ctx_t* ctx);

/* checksum::data() over every record span; d_out[i] = data(record i) (u16, numeric value as the
 * reference returns it).  Record kinds are ignored: every record is a raw span. */
int smol_csum_batch_data(smol_csum_ctx_t* ctx, const uint8_t* d_buf,
                         const smol_csum_batch_t* batch, uint16_t* d_out, void* stream);

/* In-place emit: for every record write the IPv4 header checksum and the L4 checksum the way the
 * reference's Repr::emit does under `caps` (fill when tx(), else 0; UDP 0 -> 0xffff; IGMP always
 * filled).  An ICMPv4 DstUnreachable / TimeExceeded message's embedded IPv4 header gets its header
 * checksum first, under caps.ipv4, as Icmpv4Repr::emit writes it with Ipv4Repr::emit
 * (src/wire/icmpv4.rs:520-543).  `d_status` (nullable) receives SMOL_ST_MALFORMED /
 * SMOL_ST_UNSUPPORTED per record.  Kernels on `stream` only; records must not overlap.  The kernels
 * write the 64-byte segment around a record's fields whole where that is race-free within the
 * call: the segment's other bytes, which may belong to the records just before and after it in
 * the batch (contiguous with it in memory, no field of theirs in the segment), are written back
 * with the values the kernels read.  Bytes outside the batch's records are never written.  So
 * nothing else may write the batch's records while the call runs, the same rule copy-emit states,
 * unless the batch sets SMOL_BATCH_FIELD_STORES (fields only).  Descriptor batches of records that
 * lie back to back take the staged form (one launch stages each record's field values in the
 * context's scratch, a second one writes the field segments, per 2^21 records): the context owns
 * ~17 MB of device scratch, allocated by smol_csum_ctx_create, and orders a staged emit issued on
 * another stream after the previous one (an event wait), so emits on one context may use several
 * streams.  Fixed-stride batches of 2^20 to 2^21 records of 1473-1921 bytes take the same two-launch
 * shape through the same scratch (the first launch writes every record's smol_csum_fields_t entry
 * there, the second the records, per 2^20 records) and are ordered across streams in the same way,
 * except that the event is recorded on the previous stream only when a call on another stream
 * arrives (if that stream has been destroyed by then, the device is synchronised instead); on a
 * capturing stream they run as one launch and use neither the scratch nor an event.  No device
 * memory is allocated by a batched call: the calls may be captured in a HIP
 * graph (a graph holding a staged emit uses the context's scratch when it replays: do not replay it
 * concurrently with another emit on the same context). */
int smol_csum_batch_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* batch,
                         const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream);

/* Verify: d_status[i] = SMOL_ST_* bits for record i under `caps` (Repr::parse gates). */
int smol_csum_batch_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf,
                           const smol_csum_batch_t* batch, const smol_checksum_caps_t* caps,
                           uint8_t* d_status, void* stream);

/* Payload copy of one record for smol_csum_batch_copy_emit (16 bytes, device memory). */
typedef struct {
    uint64_t src_offset; /* payload position in the source buffer (any alignment)          */
    uint32_t dst_offset; /* where the payload goes inside the record                         */
    uint32_t len;        /* payload bytes (0: nothing to copy)                               */
} smol_csum_copy_t;

/* Fused payload copy + emit: the TcpRepr::emit / UdpRepr::emit sequence "copy the payload into
 * the packet, then fill the checksum" (src/wire/tcp.rs:1087-1095, src/wire/udp.rs:300-308) in one
 * pass.  For every record i: copy d_src[copy[i].src_offset ..][.. len] to record bytes
 * [dst_offset, dst_offset + len), then emit exactly as smol_csum_batch_emit does (the headers in
 * front of the payload were already written by the caller).  The payload is read once and
 * written once; nothing is read back.  The result is bit-identical to a memcpy followed by
 * smol_csum_batch_emit, including when the copied range covers a checksum field (the emitted
 * field wins).  A record whose copy range does not fit (dst_offset + len > record length) is
 * left untouched and reported SMOL_ST_MALFORMED.  `d_copy` is a 16-byte-aligned device array of
 * n entries; the source must not overlap the batch buffer, and records must not overlap one another
 * (the kernel rewrites every byte of a record — the bytes outside its copy range with their own
 * values — so that whole cache lines leave L2). */
int smol_csum_batch_copy_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* batch,
                              const uint8_t* d_src, const smol_csum_copy_t* d_copy,
                              const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream);

/* ---- emit_fields: checksum values out, frames patched on the host ------------------------- */

#define SMOL_NO_FIELD 0xffffu
/* One record's emit result (16 bytes, 16-byte aligned device array). */
typedef struct {
    uint16_t off[3];   /* record-relative byte offset of [0] the IPv4 header checksum, [1] the L4 checksum,
                          [2] the embedded IPv4 header checksum of an ICMPv4 error message; SMOL_NO_FIELD: none */
    uint16_t val[3];   /* the value smol_csum_batch_emit would write there (numeric; goes out big-endian); 0 when none */
    uint8_t status;    /* the byte smol_csum_batch_emit puts in d_status (MALFORMED / UNSUPPORTED bits) */
    uint8_t reserved[3]; /* 0 */
} smol_csum_fields_t;

/* Emit without the in-place writes.  In the reference the frame stays in host memory and every
 * checksum write is two bytes: UdpPacket::fill_checksum (src/wire/udp.rs:194-208),
 * TcpPacket::fill_checksum (src/wire/tcp.rs:616-626), Ipv4Packet::fill_checksum
 * (src/wire/ipv4.rs:506-513), Icmpv4Repr::emit (src/wire/icmpv4.rs:520-554).  This call gives the
 * offload that shape: the device reads the frames (a copy of the TxToken::consume buffers) and returns
 * only the fields, so nothing but 16 bytes per frame has to come back over the host link.
 *
 * For every record, d_fields[i] holds exactly the fields smol_csum_batch_emit would write under
 * `caps`, with the same values: the IPv4 header checksum (0 when caps.ipv4 has no tx()), the L4
 * checksum (UDP 0 -> 0xffff, IGMP always filled), an ICMPv4 error message's embedded IPv4 header
 * checksum (with the ICMP checksum computed over that new value), the header alone for a
 * SMOL_REC_IPHDR_ONLY record, and for malformed / unsupported records the same fields and status bits
 * as emit.  Unused slots hold off = SMOL_NO_FIELD, val = 0.  Nothing is written to d_buf.
 * SMOL_BATCH_FIELD_STORES has no meaning here and is accepted.  The call uses no context scratch, no
 * event and no allocation; it is stream-ordered on `stream`, and calls on different streams are
 * independent (also on one context).  SMOL_EINVAL: NULL ctx, bad caps, NULL or misaligned d_fields
 * with n > 0.  Not covered: the 6LoWPAN NHC entry points (no address array here) and IPv4 fragment
 * groups (smol_csum_batch_emit_frag).
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive); a loader that must run
 * against an older build probes for the symbol (dlsym). */
int smol_csum_batch_emit_fields(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                const smol_checksum_caps_t* caps, smol_csum_fields_t* d_fields, void* stream);

/* host: write the entry's fields into one record; SMOL_ERANGE (nothing written) if a field does not fit in len */
int smol_csum_apply_fields(uint8_t* rec, uint32_t len, const smol_csum_fields_t* f);

/* ---- verify_copy: verify and deliver the L4 payloads in one pass --------------------------- */

/* Where one record's payload goes (16 bytes, 16-byte-aligned device array, input). */
typedef struct {
    uint64_t dst_offset; /* byte offset in d_dst (any alignment)            */
    uint32_t cap;        /* bytes available there                             */
    uint32_t reserved;   /* 0; the kernels ignore it                          */
} smol_csum_slot_t;

/* One record's payload span (8 bytes, 8-byte-aligned device array, output). */
typedef struct {
    uint32_t len;     /* payload bytes                                                */
    uint16_t off;     /* record-relative offset of the payload; 0: the record has none */
    uint8_t copied;   /* 1: the span is defined and len <= cap (bytes delivered)      */
    uint8_t reserved; /* 0 */
} smol_csum_span_t;

/* Verify, and deliver every record's L4 payload to its slot of d_dst, in one pass over the batch.
 * On receive the reference makes two passes over a payload: UdpRepr::parse / TcpRepr::parse sum the
 * whole L4 buffer (src/wire/udp.rs:250-257, src/wire/tcp.rs:917-919), then the socket copies the
 * payload out (UDP: rx_buffer.enqueue + copy_from_slice, src/socket/udp.rs:522-523; TCP:
 * rx_buffer.write_unallocated, src/socket/tcp.rs:2231).  Here each byte of a record is read once.
 *
 * Status.  d_status[i] is exactly the byte smol_csum_batch_verify writes for the same batch and caps.
 *
 * Span.  A record has a span when it reaches the UDP or TCP gate and verify's parse marks it neither
 * SMOL_ST_MALFORMED nor SMOL_ST_UNSUPPORTED (so: no span after a failed check_len, a port-0
 * rejection, a Hop-by-Hop drop, for a fragment, a SMOL_REC_IPHDR_ONLY record, a non-IP ethertype or
 * SMOL_KIND_RAW).
 *   UDP (UdpPacket::payload, udp.rs:153-157): off = L4 offset + 8, len = UDP length field - 8.
 *   TCP (TcpPacket::payload, tcp.rs:419-423): off = L4 offset + 4 * data offset,
 *                                             len = L4 buffer length - 4 * data offset.
 * The L4 buffer is the slice the reference hands the L4 packet: IPv4 total length - IHL * 4 (not the
 * record length: Ethernet padding is neither summed nor delivered), IPv6 payload length minus a
 * leading Hop-by-Hop header.  ICMP, IGMP and every rejected record get off = 0, len = 0, copied = 0.
 *
 * Copy.  When the span is defined and len <= cap, record bytes [off, off + len) are written to
 * d_dst[dst_offset .. dst_offset + len) and copied = 1 (len == 0 is trivially copied); otherwise
 * nothing is stored for the record and copied = 0, the span still reported.
 * THE COPY DOES NOT WAIT FOR THE CHECKSUM VERDICT: the verdict is known only after the last byte is
 * summed, and holding a record back would cost the second pass this call exists to remove.  A
 * record with a bad checksum is delivered as it stands in the buffer.  The caller commits a slot
 * only when d_status[i] & SMOL_ST_ACCEPT, as with a NIC's receive ring.
 *
 * Writes.  No byte of d_dst outside the copied ranges is ever written and no byte of d_dst is ever
 * read: the first and last piece of a range go out as byte-masked stores, never read-modify-write,
 * so slots may lie back to back (a neighbouring slot may be written by another wavefront at the
 * same time).  Slots must not overlap each other or the batch.  d_buf is only read.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, and calls on
 * different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_dst / d_slots / d_status / d_spans with n > 0, d_slots
 * not 16-byte aligned, d_spans not 8-byte aligned.  SMOL_ERANGE: as verify.  n == 0 returns SMOL_OK
 * and launches nothing.  Not covered: the 6LoWPAN NHC entry points.  IPv4 fragment groups have their
 * own call, smol_csum_batch_verify_reassemble (section 3).
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as emit_fields was). */
int smol_csum_batch_verify_copy(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                const smol_checksum_caps_t* caps, uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                uint8_t* d_status, smol_csum_span_t* d_spans, void* stream);

/* ---- 3. IPv4 fragment groups ------------------------------------------------------------- */

/* One IPv4 datagram carried by `count` consecutive records of a batch, starting at record
 * `first` (16 bytes, device memory): its fragments, in any order.  A group of one unfragmented
 * packet is allowed.  Groups must not share records.  A group that does not lie inside the batch
 * (first >= n, or count > n - first), whose count is 0 or above SMOL_MAX_FRAGMENTS, or whose
 * reserved word is not 0 is invalid: none of its records is read or written, status included. */
typedef struct {
    uint64_t first;
    uint32_t count;    /* 1 .. SMOL_MAX_FRAGMENTS */
    uint32_t reserved; /* must be 0 */
} smol_csum_frag_group_t;

/* Fragments per group the kernels accept (smoltcp's default fragmentation and reassembly buffers
 * hold 1500 bytes, gen_config.py; 256 fragments of 8 bytes cover 2 KB, of 1480 bytes 370 KB). */
#define SMOL_MAX_FRAGMENTS 256u

/* Emit for IPv4 datagrams the stack fragmented under offloaded checksums.  The iface emits the
 * whole datagram with the device's caps (the L4 checksum written 0) and only then cuts it into
 * fragments that reach TxToken::consume one by one (src/iface/interface/mod.rs:1276-1331,
 * src/iface/interface/ipv4.rs:421-490), so the device, holding a datagram's fragments until the
 * last one, fills per group: every fragment's IPv4 header checksum (caps.ipv4, as
 * dispatch_ipv4_frag does) and the datagram's L4 checksum over the reassembled datagram — its
 * L4 length, its pseudo-header, ICMPv4 error messages' embedded header included — written into
 * the fragment that holds the field.  That is the RFC 1071 / 768 / 793 checksum a receiver
 * verifies, and the one smoltcp's own reassembling receive path accepts.
 *
 * Deliberate divergence from the reference's software route.  With its default caps the reference
 * emits a datagram it will fragment into the whole fixed-size frag.buffer
 * (FRAGMENTATION_BUFFER_SIZE bytes, mod.rs:1320; emit_payload gets &mut buffer[hl..],
 * mod.rs:1263-1267, packet.rs:80-83,166-171):
 *   - UDP: identical.  UdpPacket::fill_checksum covers the UDP length field's span (udp.rs:194-208).
 *   - TCP: differs whenever the datagram is shorter than the buffer.  TcpPacket::fill_checksum
 *     sums the whole buffer tail and puts its length in the pseudo-header (tcp.rs:616-626), so the
 *     reference's fragments carry a checksum its own reassembling receiver rejects.
 *   - ICMPv4 echo: identical only when the buffer tail past the datagram is zero;
 *     Icmpv4Packet::fill_checksum sums the whole tail, stale bytes of earlier datagrams included
 *     (icmpv4.rs:339-346, 502-503).  ICMPv4 error messages: the reference's emit panics on a tail
 *     (copy_from_slice of unequal lengths, icmpv4.rs:529-530, 543-544).
 * tests/test_frag_cpu.py restates that route (oracle_emit_like_dispatch_ip) and pins each case.
 *
 * A group is usable when every record is an IPv4 packet (Medium::Ip, or Ethernet with ethertype
 * 0x0800) passing Ipv4Packet::check_len, all share the reassembly key (ident, source, destination,
 * protocol: ipv4.rs get_key), the payloads cover [0, T) exactly once with exactly one last
 * fragment (MF clear) ending at T; otherwise its records are reported SMOL_ST_MALFORMED and only
 * their own headers are filled.  A group with SMOL_REC_IPHDR_ONLY on any record gets its headers
 * only (a raw socket's datagram).  `d_status` (nullable) receives SMOL_ST_MALFORMED /
 * SMOL_ST_UNSUPPORTED per record of every valid group. */
int smol_csum_batch_emit_frag(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* batch,
                              const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                              const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream);

/* Verify for fragmented IPv4 datagrams (src/iface/interface/ipv4.rs:103-146: every fragment
 * passes Ipv4Repr::parse, then the reassembled payload reaches the L4 gate).  Per record: its own
 * IPv4 bits, the datagram's L4 bits, and SMOL_ST_ACCEPT only when every fragment of the group
 * passes its IPv4 gate and the datagram its L4 gate (a dropped fragment never completes the
 * datagram).  Records outside every group are not written. */
int smol_csum_batch_verify_frag(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream);

/* One reassembled datagram (16 bytes, 16-byte-aligned device array, output; one per group). */
typedef struct {
    uint32_t len;      /* reassembled IPv4 payload bytes T (0: the group is not usable)        */
    uint32_t l4_len;   /* L4 payload bytes inside it (UDP length - 8; TCP T - 4*data offset)    */
    uint16_t l4_off;   /* datagram-relative offset of the L4 payload (UDP 8, TCP 4*data offset);
                          0 with l4_len 0: no UDP/TCP payload span                             */
    uint8_t protocol;  /* the IPv4 protocol byte of the reassembly key (0 when not usable)      */
    uint8_t copied;    /* 1: len <= cap and bytes [0, len) were delivered                       */
    uint32_t reserved; /* 0 */
} smol_csum_dgram_t;

/* verify_frag, and every group's fragment payloads delivered to their places in the datagram's slot of
 * d_dst, in one pass over the fragments.  On receive the reference reads a fragmented datagram twice:
 * PacketAssembler::add copies each fragment's payload into the assembler's buffer
 * (src/iface/fragmentation.rs:139-151, called from src/iface/interface/ipv4.rs:131), and once
 * assemble() returns the whole payload (ipv4.rs:136) the L4 Repr::parse sums all of it
 * (udp.rs:250-257, tcp.rs:917-919, icmpv4.rs:404-407).  Here each payload byte is read once.  The
 * reassembler's bookkeeping (keys, timeouts, holes) stays with the caller, who forms the groups; this
 * call serves its copy.
 *
 * Status.  d_status (one byte per RECORD) holds exactly the bytes smol_csum_batch_verify_frag writes for
 * the same batch, groups and caps.  Records outside every group are not written; records of an invalid
 * group are neither read nor written.
 *
 * Reassembly.  d_slots and d_dgrams have one entry per GROUP.  A group is usable under the contract
 * above: every record passes Ipv4Packet::check_len, all share one reassembly key, the payloads cover
 * [0, T) exactly once, exactly one last fragment ends at T.  For a usable group len = T and protocol is
 * the key's protocol byte; when T <= cap, fragment j's payload is written to
 * d_dst[dst_offset + start_j .. dst_offset + end_j) and copied = 1 (PacketAssembler::add's
 * buffer[offset..][..len].copy_from_slice(data)).  This holds whatever the protocol and whatever the L4
 * verdict, as the reference reassembles before it looks at L4 (ipv4.rs:111-143): a raw socket's
 * datagram (SMOL_REC_IPHDR_ONLY on any record) is delivered, a protocol smoltcp does not checksum is
 * delivered with status SMOL_ST_UNSUPPORTED, and a datagram whose L4 check_len fails (a UDP length field
 * above T, a port-0 rejection) is delivered whole with status SMOL_ST_MALFORMED and l4_off = l4_len = 0.
 * A group of one unfragmented packet delivers that packet's IP payload.  When T > cap nothing is stored,
 * copied = 0 and len = T is still reported, so the caller can size a retry.  A group that is not usable
 * stores nothing and its entry is all zero; so is the entry of an invalid group (first >= n, count 0 or
 * above SMOL_MAX_FRAGMENTS, count > n - first, reserved != 0): the entry is indexed by group, no record
 * is touched.
 *
 * L4 span.  l4_off / l4_len are defined when the datagram reaches the UDP or TCP gate and is neither
 * SMOL_ST_MALFORMED nor SMOL_ST_UNSUPPORTED: the spans smol_csum_batch_verify_copy reports, relative to
 * the datagram start (UdpPacket::payload, udp.rs:153-157; TcpPacket::payload, tcp.rs:419-423).  For
 * UDP the sum covers [0, UDP length) while the copy always covers [0, T): bytes past the UDP length
 * are delivered and not summed, as in the reference's two passes.
 *
 * THE COPY DOES NOT WAIT FOR THE VERDICT, neither the L4 checksum's nor a fragment's IPv4 header
 * gate's.  The caller commits a slot only when every status byte of the group has SMOL_ST_ACCEPT.
 *
 * Writes.  No byte of d_dst is ever read and none outside [dst_offset, dst_offset + T) of a delivered
 * group is ever written.  The first and last piece of every fragment's range go out as byte-masked
 * stores, never read-modify-write: two fragments of a datagram meet at a multiple of 8, which can fall
 * inside one 16-byte destination chunk written by two wavefronts.  Slots may lie back to back at any
 * alignment; they must not overlap each other or the batch.  d_buf is only read, and only in 16-byte
 * chunks that hold at least one byte of a record.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, and calls on
 * different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_groups / d_dst / d_slots / d_status / d_dgrams with
 * n_groups > 0, d_groups, d_slots or d_dgrams not 16-byte aligned.  SMOL_ERANGE: as verify_frag.
 * n_groups == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as verify_copy was). */
int smol_csum_batch_verify_reassemble(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                      const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                      const smol_checksum_caps_t* caps, uint8_t* d_dst,
                                      const smol_csum_slot_t* d_slots, /* one per GROUP */
                                      uint8_t* d_status,               /* one per RECORD, as verify_frag */
                                      smol_csum_dgram_t* d_dgrams,     /* one per GROUP */
                                      void* stream);

/* Where and how one datagram is cut (16 bytes, 16-byte-aligned device array, input; one per record). */
typedef struct {
    uint64_t dst_offset; /* byte offset of the datagram's first frame in d_dst (any alignment) */
    uint32_t cap;        /* bytes available there                                                */
    uint16_t ip_mtu;     /* DeviceCapabilities::ip_mtu() for this datagram (phy/mod.rs:282-293)  */
    uint16_t ident;      /* the iface's ipv4_id, written into every fragment (mod.rs:1323-1324)  */
} smol_csum_fragplan_t;

/* What became of one datagram (16 bytes, 16-byte-aligned device array, output; one per record). */
typedef struct {
    uint32_t count;     /* frames the datagram makes (0: not an IPv4 datagram this call cuts)     */
    uint32_t frame_len; /* bytes of every frame but the last: io + 20 + step                      */
    uint32_t last_len;  /* bytes of the last frame (count == 1: the only one)                     */
    uint8_t status;     /* the byte smol_csum_batch_emit puts in d_status for the record          */
    uint8_t written;    /* 1: all count frames were stored                                        */
    uint16_t reserved;  /* 0 */
} smol_csum_fragout_t;

/* emit, and every whole IPv4 datagram cut into the frames the iface sends, in one pass over the datagram:
 * the mirror of smol_csum_batch_verify_reassemble, whose input this call's output is.  On transmit the
 * reference reads a datagram larger than the IP MTU twice: it emits it whole into frag.buffer, the L4
 * fill_checksum summing every byte (src/iface/interface/mod.rs:1263-1331), and then copies it out a
 * fragment at a time into the TX token buffers, each behind a fresh IPv4 header with its own header
 * checksum and, on Ethernet, a fresh Ethernet header (mod.rs:1334-1347 for the first fragment,
 * dispatch_ipv4_frag, src/iface/interface/ipv4.rs:421-482, for the rest).  Here each datagram byte is read
 * once and each frame byte written once.
 *
 * Records.  Each record of the batch (fixed-stride or descriptors) is one whole IPv4 datagram,
 * SMOL_KIND_IP or SMOL_KIND_ETH (ethertype 0x0800); io below is 0 for SMOL_KIND_IP and 14 for
 * SMOL_KIND_ETH.  d_buf is only read, and only in 16-byte chunks that hold at least one byte of a record.
 *
 * Which records are cut.  A record is cut when it carries an IPv4 header that passes
 * Ipv4Packet::check_len, its IHL is 5 (Ipv4Repr::emit writes no options), it is not itself a fragment
 * (MF clear and offset 0), and ip_mtu >= 28.  Every other record (IPv6: smoltcp has no IPv6
 * fragmentation; a non-IP ethertype; SMOL_KIND_RAW) gets count = 0, written = 0 and nothing stored.
 * status is always the byte smol_csum_batch_emit would report for the record.
 *
 * Cut.  T = total length - 20; step = (ip_mtu - 20) - (ip_mtu - 20) % 8 (max_ipv4_fragment_size,
 * phy/mod.rs:297-300); S = frame_stride, or frame_len when frame_stride == 0; frame k starts at
 * d_dst + dst_offset + k * S.
 *   - 20 + T <= ip_mtu: the datagram goes out as one frame, as the iface sends it (mod.rs:1276):
 *     count = 1, frame_len = last_len = io + 20 + T; the frame is the record's first io + 20 + T bytes
 *     with emit's fields, its ident, DF and flags as the caller wrote them.
 *   - otherwise count = ceil(T / step), frame_len = io + 20 + step, and frame k is the record's io
 *     Ethernet bytes, the 20-byte header, then payload bytes [k * step, min((k + 1) * step, T)).  The
 *     header is the datagram's with total length (20 + the payload length), ident (the plan's), DF
 *     cleared, MF set on all frames but the last, fragment offset k * step / 8 and the header checksum
 *     (filled under caps.ipv4.tx(), else 0) rewritten.
 *
 * Checksums.  The payload bytes delivered are those smol_csum_batch_emit would leave in the record under
 * caps: the L4 checksum over the whole datagram (0 without tx(); UDP 0 mapped to 0xffff; IGMP always
 * filled), for an ICMPv4 error message the embedded IPv4 header checksum first; SMOL_REC_IPHDR_ONLY and
 * protocols emit does not checksum: payload verbatim; a record whose L4 check_len fails: payload
 * verbatim, status SMOL_ST_MALFORMED, still cut.  In short, a cut datagram's frames are
 * fragment_like_iface(emit(record), ip_mtu, ident, fill_header = caps.ipv4.tx()), each behind the
 * record's Ethernet header if it has one.
 *
 * Cap and stride.  The datagram needs (count - 1) * S + last_len bytes.  When that exceeds cap, or when
 * frame_stride != 0 && frame_stride < frame_len, nothing is stored and written = 0; count, frame_len
 * and last_len are still reported, so the caller can size a retry.  Gaps between frames
 * (frame_stride > frame length) are never written.
 *
 * Writes.  No byte of d_dst is ever read and none outside the frames of a written datagram is ever
 * written; every byte of a frame is written exactly once.  Edges go out as byte-masked stores, never
 * read-modify-write, so slots and frames may lie back to back at any alignment.  Slots must not overlap
 * each other or the batch.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, and calls on
 * different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_dst / d_plans / d_out with n > 0, d_plans or d_out not
 * 16-byte aligned.  SMOL_ERANGE: as emit.  n == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as verify_reassemble was). */
int smol_csum_batch_fragment_emit(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                  const smol_checksum_caps_t* caps, uint8_t* d_dst,
                                  const smol_csum_fragplan_t* d_plans, uint32_t frame_stride,
                                  smol_csum_fragout_t* d_out, void* stream);

/* One send (32 bytes, 16-byte-aligned device array, input; one per record). */
typedef struct {
    uint64_t src_offset; /* first payload byte in d_src (any alignment)            */
    uint32_t len;        /* payload bytes of the whole send (0: one bare segment)  */
    uint16_t mss;        /* payload bytes per segment; 0: the record is not cut    */
    uint16_t reserved;   /* 0; the kernel ignores it                               */
    uint64_t dst_offset; /* first frame in d_dst (any alignment)                   */
    uint32_t cap;        /* bytes available there                                  */
    uint32_t reserved2;  /* 0; ignored                                             */
} smol_csum_tcpplan_t;

/* What became of one send (16 bytes, 16-byte-aligned device array, output; one per record): the layout of
 * smol_csum_fragout_t under its own name. */
typedef struct {
    uint32_t count;     /* frames the send makes (0: not a template this call cuts)                  */
    uint32_t frame_len; /* bytes of every frame but the last: hl + min(mss, len)                     */
    uint32_t last_len;  /* bytes of the last frame (count == 1: the only one)                        */
    uint8_t status;     /* the byte smol_csum_batch_emit puts in d_status for the record             */
    uint8_t written;    /* 1: all count frames were stored                                           */
    uint16_t reserved;  /* 0 */
} smol_csum_tcpout_t;

/* emit, and every TCP send cut into MSS-sized segments, in one pass over the payload: the TCP counterpart
 * of smol_csum_batch_fragment_emit (one header template and one payload range in, the iface's frames out,
 * every checksum filled).  In the reference such a burst is repeated TcpSocket::dispatch calls within one
 * poll: each takes tx_buffer.get_allocated(offset, size) with size <= effective_mss
 * (src/socket/tcp.rs:2620-2673) and sets PSH or FIN only when the segment reaches the end of the buffer
 * (tcp.rs:2675-2687); TcpRepr::emit then copies the payload and fill_checksum sums it
 * (src/wire/tcp.rs:1087-1095, 616-626), and the IP header goes in front of each one (Ipv4Repr::emit,
 * src/wire/ipv4.rs:584-611, which writes ident 0 and DF on every packet; Ipv6Repr::emit,
 * src/wire/ipv6.rs:628-640).  Between two segments of such a burst only the sequence number, the IP
 * length field, FIN / PSH and the two checksums change.  Here each payload byte is read once and each
 * frame byte written once.
 *
 * Records.  Each record of the batch (fixed-stride or descriptors) is one header template: what the stack
 * emits for a TCP segment with an empty payload.  An optional Ethernet header (SMOL_KIND_ETH, io = 14;
 * SMOL_KIND_IP, io = 0), an IPv4 or IPv6 header, and a TCP header with its options, thl = 4 * data offset:
 * hl = io + 20|40 + thl, so hl <= 114.  Record bytes past hl are ignored.  d_buf is only read.
 *
 * Which records are cut.  Let g be emit's parse of the record.  A record is cut when all of these hold:
 *   - g reports no status bit (the record passes every check_len emit runs) and the protocol is TCP;
 *   - IPv4 with IHL 5, or IPv6 whose next header is 6 directly (a template with a Hop-by-Hop header is
 *     not cut);
 *   - the L4 length the IP header states equals thl: the template carries no payload of its own;
 *   - SYN and RST are clear (the stack sends those without data, through plain emit);
 *   - mss >= 1;
 *   - the largest frame's IP length field fits 16 bits: IPv4 20 + thl + min(mss, len) <= 65535, IPv6
 *     thl + min(mss, len) <= 65535.
 * Every other record (SMOL_REC_IPHDR_ONLY; fragments; UDP and the other protocols; SMOL_KIND_RAW; non-IP
 * ethertypes; a failed check_len) gets count = 0, written = 0 and nothing stored.  status is always the
 * byte smol_csum_batch_emit reports for the record as it stands.
 *
 * Cut.  count = max(1, ceil(len / mss)); p_k = min(mss, len - k * mss) (p_0 = 0 when len == 0);
 * frame_len = hl + p_0; last_len = hl + p_{count-1}; S = frame_stride, or frame_len when
 * frame_stride == 0; frame k starts at d_dst + dst_offset + k * S.  Frame k is the template's first hl
 * bytes with the following changes, followed by d_src[src_offset + k * mss ..][.. p_k]:
 *   - IPv4: total length is 20 + thl + p_k; the header checksum is filled under caps.ipv4.tx(), else 0;
 *     ident, flags and TTL are as in the template on every frame (ipv4.rs:595-600);
 *   - IPv6: payload length is thl + p_k;
 *   - TCP sequence number: seq0 + k * mss mod 2^32;
 *   - TCP flags: FIN and PSH are cleared on every frame but the last; every other flag bit is kept as in
 *     the template on every frame;
 *   - ack number, window, urgent pointer and options are verbatim on every frame;
 *   - TCP checksum: under caps.tcp.tx() it covers the pseudo-header (length thl + p_k), the header and the
 *     payload, with no 0 mapping (tcp.rs:616-626); otherwise it is 0.
 * In short, frame k is byte for byte what smol_csum_batch_emit leaves in a record made of those rewritten
 * headers followed by that payload slice, and what smol_csum_batch_copy_emit writes from host-built
 * headers.
 *
 * Cap and stride.  The send needs (count - 1) * S + last_len bytes.  When that exceeds cap, or when
 * frame_stride != 0 && frame_stride < frame_len, nothing is stored and written = 0; count, frame_len
 * and last_len are still reported, so the caller can size a retry.  Gaps between frames
 * (frame_stride > frame length) are never written.
 *
 * Reads and writes.  No byte of d_dst is ever read and none outside the frames of a written send is ever
 * written; every byte of a written frame is written exactly once.  Edges go out as byte-masked stores,
 * never read-modify-write, so slots and frames may lie back to back at any alignment.  d_src is only
 * read, and only in 16-byte chunks that hold at least one byte of a cut plan's range.  d_src, d_dst and
 * the batch must not overlap; slots must not overlap each other.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, and calls on
 * different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_src / d_dst / d_plans / d_out with n > 0, d_plans or d_out not
 * 16-byte aligned.  SMOL_ERANGE: as emit.  n == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as fragment_emit was). */
int smol_csum_batch_tcp_segment_emit(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                     const smol_checksum_caps_t* caps, const uint8_t* d_src, uint8_t* d_dst,
                                     const smol_csum_tcpplan_t* d_plans, uint32_t frame_stride,
                                     smol_csum_tcpout_t* d_out, void* stream);

#define SMOL_MAX_FLOW_SEGMENTS 256u

/* One connection's receive window (32 bytes, 16-byte-aligned device array, input; one per GROUP). */
typedef struct {
    uint64_t dst_offset;   /* byte offset of the ring's storage in d_dst (any alignment)                 */
    uint32_t ring_len;     /* bytes of ring storage (rx_buffer.capacity())                                */
    uint32_t ring_pos;     /* ring index of the window's first byte (rx_buffer.get_idx(rx_buffer.len()))  */
    uint32_t window_start; /* sequence number of that byte: remote_seq_no + rx_buffer.len()               */
    uint32_t window_len;   /* window_end - window_start (0: remote_last_ack is None, or a closed window)  */
    uint32_t reserved[2];  /* must be 0 */
} smol_csum_tcpwin_t;

/* One record's outcome (16 bytes, 16-byte-aligned device array, output; one per RECORD). */
typedef struct {
    uint32_t seq;      /* the TCP sequence number field (0 without SMOL_SEG_TCP)                        */
    uint32_t win_off;  /* overlap_start - window_start: window offset of the first delivered byte       */
    uint32_t len;      /* overlap_end - overlap_start: bytes of the payload inside the window           */
    uint16_t off;      /* record-relative offset of the payload, untrimmed (smol_csum_span_t.off)       */
    uint8_t flags;     /* SMOL_SEG_*                                                                     */
    uint8_t reserved;  /* 0 */
} smol_csum_tcpseg_t;
#define SMOL_SEG_TCP         0x01u /* the record has a TCP payload span under verify_copy's span rule    */
#define SMOL_SEG_IN_WINDOW   0x02u /* segment_in_window (tcp.rs:1719-1769) against the group's window    */
#define SMOL_SEG_COPIED      0x04u /* IN_WINDOW, neither SYN nor RST: its len bytes were stored (len may be 0) */
#define SMOL_SEG_REDELIVERED 0x08u /* stored a second time after the group's verdicts (see Overlaps)     */

/* One connection's outcome (16 bytes, 16-byte-aligned device array, output; one per GROUP). */
typedef struct {
    uint32_t contig_len;  /* bytes now contiguous from window_start: what enqueue_unallocated gets in total */
    uint32_t counted;     /* records that count into it (below)                                            */
    uint32_t redelivered; /* records with SMOL_SEG_REDELIVERED                                             */
    uint8_t valid;        /* 1: the group and its window were usable                                       */
    uint8_t reserved[3];  /* 0 */
} smol_csum_tcpflow_t;

/* verify, and every TCP segment's payload delivered to the place its sequence number gives it in its
 * connection's receive ring, trimmed to the receive window, in one pass over the frames: the receive
 * counterpart of smol_csum_batch_tcp_segment_emit, whose output is this call's input (as fragment_emit's is
 * verify_reassemble's).  In TcpSocket::process (src/socket/tcp.rs:1705-1783, 2205-2241) the place of a
 * payload follows from the segment's own sequence number: the segment is tested against the receive
 * window (segment_in_window), trimmed to it at both ends, written with
 * rx_buffer.write_unallocated(payload_offset, payload), which wraps around the ring
 * (src/storage/ring_buffer.rs:321-338), and the assembler then says how much of the front has become
 * contiguous (add_then_remove_front).  TcpRepr::parse has summed the payload before
 * (src/wire/tcp.rs:917-919): two passes over it.  Here each frame byte is read once.
 *
 * Groups.  smol_csum_frag_group_t is reused unchanged: a group is the frames of one connection that
 * arrived in one poll, `count` consecutive records from `first`, in arrival order.  The caller
 * demultiplexes, as it forms fragment groups.  d_wins and d_flows have one entry per GROUP, d_status and
 * d_segs one per RECORD.  A group is invalid when first >= n, count > n - first, count is 0 or above
 * SMOL_MAX_FLOW_SEGMENTS, the group's or the window's reserved words are not 0, window_len > ring_len,
 * or ring_pos >= ring_len while ring_len > 0 (with ring_len == 0, ring_pos must be 0).  For an invalid
 * group no record is read, no status byte or segment entry is written, nothing is stored, and the flow
 * entry is all zero.  Records outside every group are not written.  Groups must not share records.
 *
 * Status.  d_status[i] is exactly the byte smol_csum_batch_verify writes for record i under caps: per
 * record, not combined over the group, because TCP segments are independent packets.
 *
 * Span.  A record has SMOL_SEG_TCP when smol_csum_batch_verify_copy would give it a span and the protocol
 * is TCP; off is then verify_copy's off, and the payload length is p = L4 buffer length - 4 * data offset
 * (Ethernet padding is excluded).  Every other record (UDP, ICMP, IGMP, malformed, unsupported, fragments,
 * SMOL_REC_IPHDR_ONLY, SMOL_KIND_RAW, non-IP ethertypes) gets an all-zero entry and stores nothing.
 *
 * Window rule (tcp.rs:1719-1783).  Sequence arithmetic is TcpSeqNumber's: s = (int32)(seq - window_start),
 * W = window_len.
 *   p == 0: not in the window when s == -1 (a keep-alive or a window probe); with W == 0 in the window iff
 *           s == 0; otherwise iff 0 <= s < W.
 *   p > 0:  not in the window when W == 0; otherwise in the window iff (0 <= s < W) or (0 < s + p <= W).
 *           A segment that starts before the window and ends past it is NOT in the window: this is the
 *           reference's rule.
 * In the window: win_off = max(0, s), len = min(W, s + p) - max(0, s), and the delivered bytes are payload
 * bytes [max(0, -s), max(0, -s) + len).  Not in the window: win_off = len = 0.  A record with SYN or RST
 * set reports SMOL_SEG_IN_WINDOW, win_off and len by the same formula and is never SMOL_SEG_COPIED: the
 * stack treats such segments on their own paths.
 *
 * Placement.  Window offset w lives at d_dst[dst_offset + (ring_pos + w) % ring_len].  Because
 * len <= window_len <= ring_len, a delivered range is at most two contiguous pieces: write_unallocated's
 * two get_unallocated slices.
 *
 * THE COPY DOES NOT WAIT FOR THE VERDICT, as in smol_csum_batch_verify_copy.
 *
 * Overlaps.  Unlike verify_copy's slots, the ranges of a group's records may coincide (retransmissions,
 * out-of-order arrivals).  A DELIVERED record is one with SMOL_SEG_COPIED and len > 0; a COUNTED record is
 * a delivered one whose status has SMOL_ST_ACCEPT.  Once every verdict of the group is known and every
 * first-pass store of the group is complete, each counted record whose window range intersects the range
 * of a delivered record that is not counted is stored again, whole, and gets SMOL_SEG_REDELIVERED: the
 * case of a corrupted segment and its retransmission in one poll.  After the call:
 *   - every window byte covered by at least one counted record holds the byte of a counted record that
 *     covers it;
 *   - where several counted records cover a byte with different values, which of them it holds is
 *     unspecified (an honest sender's retransmissions agree, and the reference itself is order-dependent
 *     there);
 *   - bytes covered only by records that are not counted hold those records' bytes: they lie in
 *     unallocated ring space, which the caller never commits.
 *
 * Flow entry.  contig_len is the largest c such that the union of the counted records' window ranges
 * covers [0, c); counted and redelivered count those records; valid is 1.
 *
 * What stays with the caller.
 *   - ACK acceptability and the socket state machine.  contig_len is valid for a caller that processes
 *     every counted record; a caller that drops a counted record for socket-state reasons rebuilds the
 *     coverage from the segment entries with its own Assembler.
 *   - The assembler's hole limit.  The reference's ASSEMBLER_MAX_SEGMENT_COUNT is 4 holes; this call
 *     computes the unbounded union.
 *   - The window does not move inside one call.  Every record is tested against the window as it stood at
 *     the start of the poll, while the reference advances window_start segment by segment.  For segments
 *     whose overlapping bytes agree and which all end at or before window_end, the ring bytes
 *     [0, contig_len) and contig_len itself equal what feeding the counted records to the socket one by
 *     one gives (with an unbounded assembler).  Two differences: a duplicate of data enqueued earlier in
 *     the same poll is reported SMOL_SEG_IN_WINDOW here; a segment that starts before the advanced
 *     window_start and ends past window_end is dropped by the reference and trimmed and delivered here.
 *   - No flow-key check.  A record of another connection inside a group is placed like any other.
 *
 * Writes.  No byte of d_dst is ever read and none outside the delivered ranges is ever written.  Edges go
 * out as byte-masked stores, never read-modify-write.  Rings of different groups must not overlap each
 * other or the batch.  d_buf is only read, and only in 16-byte chunks that hold at least one byte of a
 * record.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, graph-capturable,
 * and calls on different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_groups / d_dst / d_wins / d_status / d_segs / d_flows with
 * n_groups > 0, d_groups, d_wins, d_segs or d_flows not 16-byte aligned.  SMOL_ERANGE: as verify.
 * n_groups == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as tcp_segment_emit was). */
int smol_csum_batch_verify_tcp_assemble(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                        const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                        const smol_checksum_caps_t* caps, uint8_t* d_dst,
                                        const smol_csum_tcpwin_t* d_wins,   /* one per GROUP  */
                                        uint8_t* d_status,                  /* one per RECORD */
                                        smol_csum_tcpseg_t* d_segs,         /* one per RECORD */
                                        smol_csum_tcpflow_t* d_flows,       /* one per GROUP  */
                                        void* stream);

/* ---- verify_echo_reply: echo requests verified, the replies written in the same pass ------- */

/* What the call knows of the interface (host memory, nullable: NULL means all zero). */
typedef struct {
    uint8_t bcast_v4[4]; /* the iface's directed-broadcast address; 0.0.0.0: none */
    uint8_t reserved[4]; /* must be 0 */
} smol_csum_echo_cfg_t;

/* One record's outcome (8 bytes, 8-byte-aligned device array, output). */
typedef struct {
    uint32_t frame_len; /* the reply's length; 0 unless SMOL_ECHO_ANSWERED                             */
    uint16_t data_off;  /* record-relative offset of the echo data; 0 unless SMOL_ECHO_REQUEST         */
    uint8_t head_len;   /* reply bytes in front of the data (14|0 + 20|40 + 8); 0 unless ANSWERED      */
    uint8_t flags;      /* SMOL_ECHO_*                                                                 */
} smol_csum_echo_t;
#define SMOL_ECHO_REQUEST  0x01u /* a well-formed ICMPv4 / ICMPv6 echo request                           */
#define SMOL_ECHO_ANSWERED 0x02u /* the wire-level address rule answers it: the reply frame is defined   */
#define SMOL_ECHO_WRITTEN  0x04u /* ANSWERED and frame_len <= cap: the frame is in the slot              */
#define SMOL_ECHO_SEND     0x08u /* WRITTEN and the request passed its checksum gates: transmit the slot */
#define SMOL_ECHO_HOST     0x10u /* a request only the host can answer (it needs the iface's addresses)  */

/* Verify, and write the reply to every ICMP echo request of the batch to its slot of d_dst, in one pass.
 * The reference's responder makes two reads, one write and two sums over the echo data:
 * InterfaceInner::process_icmpv4 (src/iface/interface/ipv4.rs:320-371) and process_icmpv6
 * (src/iface/interface/ipv6.rs:399-416) parse the request, Icmpv4Repr::parse / Icmpv6Repr::parse summing the
 * whole message; they build an EchoReply with the same ident, sequence number and data and hand it to
 * icmpv4_reply / icmpv6_reply (ipv4.rs:373-418, ipv6.rs:538-563); dispatch then copies the data
 * (Icmpv4Repr::emit, src/wire/icmpv4.rs:506-517; src/wire/icmpv6.rs:814-822) and sums it again
 * (fill_checksum).  Here each request byte is read once: the registers that are summed feed the stores, and
 * the request's sum and the reply's share everything but the message's first four bytes.
 *
 * Status.  d_status[i] is exactly the byte smol_csum_batch_verify writes for the same batch and caps, for
 * every record, echo or not.
 *
 * REQUEST.  Set when the record reaches the ICMPv4 or ICMPv6 gate, verify's parse marks it neither
 * SMOL_ST_MALFORMED nor SMOL_ST_UNSUPPORTED (so not for a fragment, a SMOL_REC_IPHDR_ONLY record, a
 * Hop-by-Hop drop, a failed check_len, a non-IP ethertype or SMOL_KIND_RAW), the type is 8 (v4) or 128 (v6)
 * and the code is 0 (icmpv4.rs:410, icmpv6.rs:689).  Then data_off = L4 offset + 8 and the data length is
 * the L4 buffer length - 8, the L4 buffer being verify's: IPv4 total length - IHL * 4, or the IPv6 payload
 * length less a leading Hop-by-Hop header.  Ethernet padding is neither summed nor echoed.  Every other
 * record's entry is all zero and nothing is stored for it.
 *
 * Address rule.  Wire-level only: the engine holds no interface state beyond `cfg`.
 *   nonuni4(a): a is 255.255.255.255, in 224.0.0.0/4, 0.0.0.0, or equal to a non-zero bcast_v4.
 *   bcast4(a):  a is 255.255.255.255 or equal to a non-zero bcast_v4.
 *   nonuni6(a): a[0] == 0xff, or a is ::.
 *   A MAC is unicast when bit 0 of its first byte is clear.
 *   IPv4 (icmpv4_reply): nonuni4(src): no reply, neither ANSWERED nor HOST.  Otherwise !nonuni4(dst):
 *     ANSWERED.  Otherwise bcast4(dst): HOST (the reference answers from ipv4_addr(), which only the host
 *     knows).  Otherwise (multicast, unspecified): none.
 *   IPv6 (process_ipv6, ipv6.rs:198, and icmpv6_reply): nonuni6(src): none.  !nonuni6(dst): ANSWERED.
 *     Otherwise HOST (get_source_address_ipv6).
 *   SMOL_KIND_ETH: both MACs must be unicast, else an ANSWERED record becomes HOST (the neighbour cache and
 *     the interface's own MAC are the host's).
 * HOST and ANSWERED exclude each other; both imply REQUEST.
 *
 * The reply frame (ANSWERED records only), head_len bytes of head and then the data:
 *   Ethernet (SMOL_KIND_ETH): dst = the request's src MAC, src = the request's dst MAC, the request's
 *     ethertype.
 *   IPv4, the bytes Ipv4Repr::emit writes (src/wire/ipv4.rs:584-612): 45 00, total length = 28 + data length,
 *     ident 0, flags/offset 40 00, TTL 64, protocol 1, header checksum, src = the request's dst, dst = the
 *     request's src.  The request's IPv4 options are not carried.
 *   IPv6, per Ipv6Repr::emit (src/wire/ipv6.rs:631-638): 60 00 00 00, payload length = 8 + data length, next
 *     header 58, hop limit 64, the addresses swapped.  A request's Hop-by-Hop header is not carried.
 *   ICMP: type 0 (v4) or 129 (v6), code 0, checksum, the request's ident and sequence number, the data.
 *   frame_len = head_len + data length.
 * Checksums are filled as smol_csum_batch_emit would fill them on that frame under `caps`: the IPv4 header's
 * under caps.ipv4 tx, else 0; the ICMP one under caps.icmpv4 / caps.icmpv6 tx, else 0; no 0 -> 0xffff mapping.
 * The reply's ICMP checksum is computed from the data itself, never from the request's checksum field: a
 * request accepted because rx checking is off, or one with a bad checksum, still yields the bytes
 * fill_checksum would write.
 *
 * WRITTEN.  Set when ANSWERED and frame_len <= cap: all frame_len bytes go to d_dst[dst_offset ..].
 * Otherwise nothing is stored for the record; frame_len and head_len are still reported for an ANSWERED
 * record that does not fit.  THE DATA COPY DOES NOT WAIT FOR THE VERDICT, as in smol_csum_batch_verify_copy.
 *
 * SEND = WRITTEN && (status & SMOL_ST_ACCEPT).  The caller transmits a slot only when SEND is set.
 *
 * Writes.  No byte of d_dst outside [dst_offset, dst_offset + frame_len) of a WRITTEN record is written and
 * no byte of d_dst is read: edges and the head go out byte-masked, so slots may lie back to back at any
 * alignment.  Slots must not overlap each other or the batch.  d_buf is only read.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, graph-capturable, and
 * calls on different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, a non-zero cfg->reserved, NULL d_dst / d_slots / d_status / d_echo with
 * n > 0, d_slots not 16-byte aligned, d_echo not 8-byte aligned.  SMOL_ERANGE: as verify.  n == 0 returns
 * SMOL_OK and launches nothing.  Not covered: the 6LoWPAN NHC entry points and IPv4 fragment groups.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as verify_tcp_assemble was). */
int smol_csum_batch_verify_echo_reply(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                      const smol_checksum_caps_t* caps, const smol_csum_echo_cfg_t* cfg,
                                      uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                      uint8_t* d_status, smol_csum_echo_t* d_echo, void* stream);

/* ---- verify_unreach_reply: refused datagrams verified, the ICMP errors written in the same pass ---- */

/* One record's outcome (8 bytes, 8-byte-aligned device array, output): smol_csum_echo_t's layout. */
typedef struct {
    uint32_t frame_len; /* the error frame's length; 0 unless SMOL_UNR_ANSWERED                */
    uint16_t data_off;  /* record-relative offset of the IP payload; 0 unless SMOL_UNR_REFUSED */
    uint8_t head_len;   /* frame bytes in front of the data; 0 unless ANSWERED                  */
    uint8_t flags;      /* SMOL_UNR_*                                                           */
} smol_csum_unreach_t;
#define SMOL_UNR_REFUSED  0x01u /* the interface answers this record with an ICMP error          */
#define SMOL_UNR_ANSWERED 0x02u /* the wire-level address rule lets the device write the frame   */
#define SMOL_UNR_WRITTEN  0x04u /* ANSWERED and frame_len <= cap: the frame is in the slot       */
#define SMOL_UNR_SEND     0x08u /* WRITTEN and status & SMOL_ST_ACCEPT: transmit the slot        */
#define SMOL_UNR_HOST     0x10u /* REFUSED, but only the host can build the reply                */
#define SMOL_UNR_PORT     0x20u /* REFUSED as a UDP datagram to a closed port (else: protocol / next header) */

/* Verify, and write the ICMP error for every datagram of the batch that nobody takes to its slot of d_dst, in
 * one pass.  The interface's second automatic reply with per-byte work (the first is the echo responder above):
 *   - a UDP datagram to a port no socket accepts gets Destination Unreachable / Port Unreachable
 *     (InterfaceInner::process_udp, src/iface/interface/udp.rs:49-77);
 *   - an IPv4 packet with a protocol the stack does not handle gets Protocol Unreachable
 *     (src/iface/interface/ipv4.rs:240-250);
 *   - an IPv6 packet with an unrecognised next header gets Parameter Problem (process_nxt_hdr,
 *     src/iface/interface/ipv6.rs:352-364).
 * Each reply quotes a re-emitted copy of the offending IP header and as much of the offending payload as the
 * minimum MTU allows (icmp_reply_payload_len, src/iface/packet.rs:254-264): 528 bytes over IPv4, 1192 over
 * IPv6.  The reference reads those bytes twice and sums them twice: UdpRepr::parse sums the datagram,
 * Icmpv4Repr::emit / Icmpv6Repr::emit copy the slice (src/wire/icmpv4.rs:519-531, src/wire/icmpv6.rs:740-755)
 * and fill_checksum sums the copy.  Here each record byte is read once.
 *
 * d_udp_open (8192-byte device bitmap, nullable, only read): bit (p & 7) of byte (p >> 3) is set when the host
 * wants UDP datagrams for destination port p itself, because a UDP, DNS or DHCP socket may take them or a raw
 * socket handles UDP.  A clear bit means no socket accepts the port.  NULL means every UDP datagram is the
 * host's, so only protocol / next-header errors are answered.  A host with a socket that matches on something
 * other than the destination port (the DNS socket matches the SOURCE port, src/socket/dns.rs accepts) passes
 * NULL or sets every bit.
 * cfg: smol_csum_batch_verify_echo_reply's struct, for its directed-broadcast address; NULL means all zero.
 *
 * Status.  d_status[i] is exactly the byte smol_csum_batch_verify writes for the same batch and caps, for
 * every record.
 *
 * REFUSED.  The record is SMOL_KIND_IP or SMOL_KIND_ETH (ethertype 0x0800 / 0x86DD matching the version
 * nibble, src/iface/interface/ethernet.rs:4-46), carries no SMOL_REC_IPHDR_ONLY (a raw socket handled it:
 * handled_by_raw_socket, udp.rs:52-54, ipv4.rs:240, ipv6.rs:350), and is one of (io: the IP header's offset):
 *   IPv4, protocol: the header passes Ipv4Packet::check_len (src/wire/ipv4.rs:241-256), the packet is no
 *     fragment (MF clear, offset 0: fragments belong to the reassembler, ipv4.rs:110-146) and the protocol is
 *     none of 1, 2, 6, 17.  ICMPv4 type 3 code 2 (ipv4.rs:240-250).  P = total length - IHL * 4; the data
 *     starts at io + IHL * 4.
 *   IPv4, port (sets PORT): the same header conditions, protocol 17, verify's parse marks the record neither
 *     SMOL_ST_MALFORMED nor SMOL_ST_UNSUPPORTED (UdpPacket::check_len passed, src/wire/udp.rs:57-69, and the
 *     destination port is not 0, udp.rs:246-248), d_udp_open is not NULL and the destination port's bit is
 *     clear.  Type 3 code 3 (udp.rs:56-65).
 *   IPv6, next header: Ipv6Packet::check_len passes (src/wire/ipv6.rs:400-407) and the next header is none of
 *     0, 6, 17, 58.  ICMPv6 type 4 code 1 with pointer = 40 (ipv6_repr.buffer_len(), as ipv6.rs:359 writes
 *     it).  P = the payload length; the data starts at io + 40.
 *   IPv6, port (sets PORT): next header 17 directly, with the UDP conditions above.  ICMPv6 type 1 code 4
 *     (udp.rs:67-76).
 *   IPv6 with a leading Hop-by-Hop header: when verify does not mark it MALFORMED (process_hopbyhop,
 *     ipv6.rs:263-319) and the header behind it meets one of the two IPv6 rules (a second Hop-by-Hop header
 *     there is an unrecognised next header to process_nxt_hdr), the record is REFUSED | HOST (REFUSED alone
 *     when its source is not unicast, as below), data_off = io + 40, and nothing is written: the reference quotes the next-header-0 header in front of the post-option
 *     payload (ipv6.rs:315-318), and its option-triggered Parameter Problem (ipv6.rs:268-280) is a third
 *     message.  Both stay with the host.
 * TCP (the RST is header-only work), ICMP, IGMP, fragments, malformed records, SMOL_KIND_RAW, non-IP
 * ethertypes and UDP datagrams to an open port get an all-zero entry, and nothing is stored for them.
 *
 * Address rule, with nonuni4 / nonuni6 / the MAC test of smol_csum_batch_verify_echo_reply:
 *   IPv4 (icmpv4_reply, ipv4.rs:394-414): ANSWERED iff neither source nor destination is nonuni4.  Otherwise
 *     the entry has neither ANSWERED nor HOST: the reference answers broadcasts for echo replies only.
 *   IPv6 (process_ipv6, ipv6.rs:198, and icmpv6_reply, ipv6.rs:538-563): nonuni6(src): neither.  A unicast
 *     destination: ANSWERED.  A multicast or unspecified one: HOST (get_source_address_ipv6).
 *   SMOL_KIND_ETH: both MACs must be unicast, else ANSWERED becomes HOST.
 * ANSWERED and HOST exclude each other, and both imply REFUSED.
 *
 * Data.  dlen = min(P, 528) over IPv4 and min(P, 1192) over IPv6: icmp_reply_payload_len(len, MIN_MTU, 20 |
 * 40).  The data is record bytes [data_off, data_off + dlen): the first bytes of the IP payload, not of the
 * UDP span.  When the UDP length field is shorter than P, the bytes past it are copied and summed into the
 * reply but are no part of the verdict, as in the reference's two passes (ip_payload[0..payload_len],
 * udp.rs:62).  Ethernet padding past the IP length is never read into either.
 *
 * The frame (ANSWERED records only).  head_len is 48 / 62 (IPv4: SMOL_KIND_IP / SMOL_KIND_ETH) or 88 / 102
 * (IPv6); frame_len = head_len + dlen, at most 590 and 1294 (576 and 1280 bytes of IP: the sizes
 * test_icmp_reply_size pins, src/iface/interface/tests/ipv4.rs:1390, ipv6.rs:1141).
 *   Ethernet: the MACs swapped, the request's ethertype.
 *   Outer IPv4 as Ipv4Repr::emit (src/wire/ipv4.rs:584-612): 45 00, total length 48 + dlen, ident 0, 40 00,
 *     TTL 64, protocol 1, checksum, source = the request's destination, destination = the request's source.
 *   Outer IPv6 (Ipv6Repr::emit, src/wire/ipv6.rs:631-638): 60 00 00 00, payload length 48 + dlen, next header
 *     58, hop limit 64, the addresses swapped.
 *   ICMP: type, code, checksum, then four bytes: 0 for the Destination Unreachable forms (the reference leaves
 *     them as its token buffer held them, Icmpv4Repr::emit icmpv4.rs:519-531 writes none of them; 0 is what a
 *     fresh buffer gives), 00 00 00 28 for Parameter Problem (set_param_problem_ptr, icmpv6.rs:796).
 *   The quoted header, emitted again from the parsed repr, not copied (header.emit, icmpv4.rs:527-528,
 *     icmpv6.rs:745-746).  IPv4: 20 bytes: 45 00, total length 20 + P (the full P, not dlen), ident 0, 40 00,
 *     the request's TTL and protocol, checksum, the request's source and destination unswapped; the request's
 *     DSCP / ECN, ident, flags and options are not carried.  IPv6: 40 bytes: 60 00 00 00, payload length P, the
 *     request's next header and hop limit, its addresses unswapped; traffic class and flow label are not
 *     carried.
 *   Then the data.
 * Checksums are filled as smol_csum_batch_emit fills them on that frame under `caps`: both IPv4 header
 * checksums under caps.ipv4 tx (Icmpv4Repr::emit hands the quoted header the same caps, icmpv4.rs:527-528),
 * else 0; the ICMPv4 checksum over the message with the quoted header's final checksum, under caps.icmpv4; the
 * ICMPv6 checksum with its pseudo-header, under caps.icmpv6.  None of them is derived from a checksum field of
 * the request.
 *
 * WRITTEN.  Set when ANSWERED and frame_len <= cap: all frame_len bytes go to d_dst[dst_offset ..].  Otherwise
 * nothing is stored for the record; the lengths are still reported.  THE COPY DOES NOT WAIT FOR THE VERDICT.
 *
 * SEND = WRITTEN && (status & SMOL_ST_ACCEPT).  The reference replies only after Ipv4Repr::parse and
 * UdpRepr::parse passed their checksum gates; for an unsupported protocol ACCEPT reduces to the IPv4 gate.
 *
 * Writes.  No byte of d_dst outside [dst_offset, dst_offset + frame_len) of a WRITTEN record is written and
 * no byte of d_dst is read: edges and the head go out byte-masked, so slots may lie back to back at any
 * alignment.  Slots must not overlap each other or the batch.  d_buf and d_udp_open are only read.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, graph-capturable, and
 * calls on different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, a non-zero cfg->reserved, NULL d_dst / d_slots / d_status / d_unr with
 * n > 0, d_slots not 16-byte aligned, d_unr not 8-byte aligned.  SMOL_ERANGE: as verify.  n == 0 returns
 * SMOL_OK and launches nothing.  Not covered: the 6LoWPAN NHC entry points and IPv4 fragment groups.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as verify_echo_reply was). */
int smol_csum_batch_verify_unreach_reply(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                         const smol_checksum_caps_t* caps, const smol_csum_echo_cfg_t* cfg,
                                         const uint8_t* d_udp_open, /* 8192-byte device bitmap, nullable */
                                         uint8_t* d_dst, const smol_csum_slot_t* d_slots,
                                         uint8_t* d_status, smol_csum_unreach_t* d_unr, void* stream);

/* ---- verify_udp_enqueue: datagrams verified into their sockets' receive buffers ---------- */

#define SMOL_MAX_SOCKET_DGRAMS 256u

/* One UDP socket's receive buffer before the poll (48 bytes, 16-byte-aligned device array, input; one per
 * GROUP): the two RingBuffers of its PacketBuffer (src/storage/packet_buffer.rs:43-46). */
typedef struct {
    uint64_t dst_offset;   /* byte offset of the payload ring's storage in d_dst (any alignment)  */
    uint64_t meta_first;   /* index of the metadata ring's first entry in d_meta                  */
    uint32_t payload_cap;  /* payload_ring.capacity()                                             */
    uint32_t payload_read; /* payload_ring.read_at                                                */
    uint32_t payload_len;  /* payload_ring.len()                                                  */
    uint32_t meta_cap;     /* metadata_ring.capacity()                                            */
    uint32_t meta_read;    /* metadata_ring.read_at                                               */
    uint32_t meta_len;     /* metadata_ring.len()                                                 */
    uint16_t port;         /* the socket's bound port (endpoint.port)                             */
    uint16_t reserved[3];  /* must be 0                                                           */
} smol_csum_udpsock_t;

/* One metadata entry (48 bytes, 16-byte-aligned device array d_meta, output): PacketMetadata<UdpMetadata>. */
typedef struct {
    uint32_t size;           /* payload bytes (PADDING: the bytes skipped at the ring's end)           */
    uint32_t record;         /* batch index of the datagram: the stand-in for PacketMeta               */
    uint16_t src_port;       /* endpoint.port                                                          */
    uint8_t family;          /* 4 or 6                                                                 */
    uint8_t kind;            /* SMOL_UMETA_*                                                           */
    uint8_t reserved[4];     /* 0                                                                      */
    uint8_t remote_addr[16]; /* endpoint.addr: the source IP address, IPv4 in the first 4 bytes        */
    uint8_t local_addr[16];  /* local_address: the destination IP address, likewise                    */
} smol_csum_udpmeta_t;
#define SMOL_UMETA_PACKET  1u /* PacketMetadata::packet  */
#define SMOL_UMETA_PADDING 2u /* PacketMetadata::padding: only size and kind are set, every other byte is 0 */

/* One record's outcome (16 bytes, 16-byte-aligned device array, output; one per RECORD). */
typedef struct {
    uint32_t ring_off; /* payload-ring index of the first byte (0 without SMOL_URX_ENQUEUED)          */
    uint32_t len;      /* payload bytes: the size enqueue was (or would have been) called with        */
    uint32_t meta_idx; /* metadata-ring index of its PACKET entry (0 without SMOL_URX_ENQUEUED)       */
    uint16_t off;      /* record-relative offset of the payload (smol_csum_span_t.off)                */
    uint8_t flags;     /* SMOL_URX_*                                                                  */
    uint8_t reserved;  /* 0 */
} smol_csum_udprx_t;
#define SMOL_URX_UDP      0x01u /* a candidate: a UDP payload span under verify_copy's rule, to the socket's port */
#define SMOL_URX_ENQUEUED 0x02u /* accepted, and enqueue returned Ok: payload and metadata entry are in place    */
#define SMOL_URX_FULL     0x04u /* accepted, and enqueue returned Err(Full)                                      */
#define SMOL_URX_PADDED   0x08u /* a PADDING entry was enqueued in front of it (possible together with FULL)     */
#define SMOL_URX_RESTORED 0x10u /* stored in the second pass (see Two layouts)                                   */

/* One socket's outcome (32 bytes, 16-byte-aligned device array, output; one per GROUP). */
typedef struct {
    uint32_t payload_read; /* the ring state after the poll: what the caller copies into its PacketBuffer */
    uint32_t payload_len;
    uint32_t meta_read;
    uint32_t meta_len;
    uint32_t enqueued;     /* records with SMOL_URX_ENQUEUED */
    uint32_t full;         /* records with SMOL_URX_FULL     */
    uint32_t restored;     /* records with SMOL_URX_RESTORED */
    uint8_t valid;         /* 1: the group and its socket entry were usable */
    uint8_t reserved[3];   /* 0 */
} smol_csum_udpsockout_t;

/* verify, and every UDP datagram's payload delivered to the place its socket's receive buffer gives it, the
 * metadata entries written, in one pass over the frames: the UDP counterpart of
 * smol_csum_batch_verify_tcp_assemble.  For TCP a payload's place follows from the segment's own header.  For
 * UDP it follows from the socket's PacketBuffer (src/storage/packet_buffer.rs:80-118): from the payload ring's
 * contiguous window, with a padding entry written when the packet would wrap; from a second ring of metadata
 * entries, which can fill up on its own; and from the sizes of every datagram the socket accepted earlier in
 * the same poll.  That last set depends on checksum verdicts: process_udp drops a datagram that fails
 * UdpRepr::parse before any socket sees it (src/iface/interface/udp.rs:19-36), so a bad datagram takes no
 * space.  In the reference UdpRepr::parse sums the datagram (src/wire/udp.rs:250-257) and UdpSocket::process
 * (src/socket/udp.rs:492-529) then calls rx_buffer.enqueue(size, metadata) and copy_from_slice(payload): two
 * passes over the payload.  Here, when every candidate is accepted, each frame byte is read once and its
 * 128-byte header window once more.
 *
 * Groups.  smol_csum_frag_group_t is reused unchanged: a group is the frames the caller routes to one UDP
 * socket in one poll, `count` consecutive records from `first`, in arrival order.  The caller demultiplexes by
 * address, as it forms TCP groups (the address half of UdpSocket::accepts, src/socket/udp.rs:477-490, needs
 * the interface's addresses); the device checks the port half.  d_socks and d_out have one entry per GROUP,
 * d_status and d_rx one per RECORD.  A group is invalid when first >= n, count > n - first, count is 0 or above
 * SMOL_MAX_SOCKET_DGRAMS, the group's or the socket entry's reserved words are not 0, payload_len >
 * payload_cap, meta_len > meta_cap, or a ring's read index is not below its capacity (with capacity 0 it must
 * be 0).  For an invalid group no record is read, no status byte, record entry or metadata entry is written,
 * nothing is stored, and the group's entry of d_out is all zero.  Records outside every group are not written.
 * Groups must not share records.
 *
 * Status.  d_status[i] is exactly the byte smol_csum_batch_verify writes for record i under caps.
 *
 * Candidate.  A record is a candidate (SMOL_URX_UDP) when smol_csum_batch_verify_copy would give it a span,
 * the protocol is UDP, and the UDP destination port equals the group's `port`.  Its size is that span's len
 * (the UDP length field less 8; Ethernet padding is excluded), off is verify_copy's off.  Every other record
 * (TCP, ICMP, IGMP, fragments, malformed and unsupported records, SMOL_REC_IPHDR_ONLY, SMOL_KIND_RAW, non-IP
 * ethertypes, another destination port) gets an all-zero entry and stores nothing.  A candidate is ACCEPTED
 * when status & SMOL_ST_ACCEPT.
 *
 * The enqueue rule (packet_buffer.rs:80-118; ring_buffer.rs:76-105, 181-211).  State: the capacities
 * P = payload_cap, M = meta_cap and (pr, pl, mr, ml) = (payload_read, payload_len, meta_read, meta_len).  For a
 * datagram of `size`:
 *   1. P < size or ml == M: Full, nothing changes.
 *   2. pl == 0: pr = 0.
 *   3. window = P - pl; widx = P ? (pr + pl) % P : 0; contig = min(window, P - widx).
 *   4. window < size: Full.
 *   5. Else contig < size: when window - contig < size: Full; otherwise a PADDING(contig) entry is written at
 *      metadata index (mr + ml) % M, ml += 1, pl += contig.
 *   6. ml == M: Full.  The padding stays: this is the reference's behaviour, so PADDED and FULL can be set
 *      together.
 *   7. The PACKET entry is written at metadata index (mr + ml) % M, ml += 1; ring_off = (pr + pl) % P, or 0
 *      when P == 0; pl += size.
 * A delivered payload is always one contiguous piece: bytes d_dst[dst_offset + ring_off ..][.. size].  A
 * zero-length datagram takes a metadata entry and no payload byte.  Metadata index i of a group is
 * d_meta[meta_first + i].
 *
 * Two layouts.  The ACCEPTED LAYOUT is the rule run over the group's accepted candidates in order.  It defines
 * every record entry, the metadata entries and the state in d_out; a candidate that is not accepted has
 * flags == SMOL_URX_UDP, its len and off, and takes no space.  The SPECULATIVE LAYOUT is the same rule run over
 * all candidates in order: what the layout would be if nothing failed its gates.  THE COPY DOES NOT WAIT FOR
 * THE VERDICT: a candidate the speculative layout enqueues is stored at its speculative place while it is
 * summed.  Once every verdict of the group is known, each ENQUEUED record with len > 0 that was not stored, or
 * whose place in the accepted layout differs from its speculative one, is stored again at its final place and
 * gets SMOL_URX_RESTORED.  Speculative ranges are pairwise disjoint and so are accepted ranges, so a record
 * that kept its place is never overwritten.  With every candidate accepted (a healthy link, or caps.udp not
 * checking on receive) the layouts are equal and nothing is stored twice.
 *
 * Writes.
 *   - Metadata: exactly the entries the accepted layout enqueues are written, PACKET and PADDING; no other
 *     entry of d_meta is touched.
 *   - Every byte of an ENQUEUED record's range holds its payload byte.
 *   - A byte that lies in a speculative-layout range and in no accepted-layout range holds either what it held
 *     before the call or the byte the speculative layout puts there: unallocated ring space, which the caller
 *     never commits.
 *   - Every other byte of d_dst is never written: occupied ring bytes, padding, the bytes between rings.
 *   - No byte of d_dst is ever read.  Edges go out as byte-masked stores, never read-modify-write, so rings may
 *     lie back to back at any alignment.  Rings of different groups must not overlap each other or the batch,
 *     and neither may their metadata rings.  d_buf is only read, and only in 16-byte chunks that hold at least
 *     one byte of a record.
 *
 * What stays with the caller.
 *   - The address half of UdpSocket::accepts: a group is what the caller routed to the socket.
 *   - DNS sockets, which match on the source port (src/socket/dns.rs), and DHCP and raw sockets.
 *   - The Port Unreachable answer for a port no socket is bound to: smol_csum_batch_verify_unreach_reply.
 *   - Dequeueing (PacketBuffer::dequeue skips the PADDING entries), and the socket's waker.
 *   - The commit: copy the four state words of d_out into the PacketBuffer.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, graph-capturable, and
 * calls on different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_groups / d_dst / d_socks / d_meta / d_status / d_rx / d_out with
 * n_groups > 0, d_groups, d_socks, d_meta, d_rx or d_out not 16-byte aligned.  SMOL_ERANGE: as verify.
 * n_groups == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive, as verify_unreach_reply was). */
int smol_csum_batch_verify_udp_enqueue(smol_csum_ctx_t* ctx, const uint8_t* d_buf, const smol_csum_batch_t* batch,
                                       const smol_csum_frag_group_t* d_groups, uint64_t n_groups,
                                       const smol_checksum_caps_t* caps, uint8_t* d_dst,
                                       const smol_csum_udpsock_t* d_socks, /* one per GROUP  */
                                       smol_csum_udpmeta_t* d_meta,        /* the metadata rings */
                                       uint8_t* d_status,                  /* one per RECORD */
                                       smol_csum_udprx_t* d_rx,            /* one per RECORD */
                                       smol_csum_udpsockout_t* d_out,      /* one per GROUP  */
                                       void* stream);

/* ---- udp_dequeue_emit: sockets' transmit buffers drained into frames --------------------- */

/* One UDP socket's transmit buffer before the call and where its frames go (96 bytes, 16-byte-aligned device
 * array, input; one per GROUP). */
typedef struct {
    uint64_t src_offset;   /* byte offset of the payload ring's storage in d_src (any alignment)   */
    uint64_t meta_first;   /* index of the metadata ring's first entry in d_meta                   */
    uint64_t dst_offset;   /* byte offset of the group's first frame in d_dst (any alignment)      */
    uint64_t tx_first;     /* index of the group's first entry in d_tx                             */
    uint32_t payload_cap;  /* as smol_csum_udpsock_t: payload_ring.capacity()                      */
    uint32_t payload_read; /* payload_ring.read_at                                                 */
    uint32_t payload_len;  /* payload_ring.len()                                                   */
    uint32_t meta_cap;     /* metadata_ring.capacity()                                             */
    uint32_t meta_read;    /* metadata_ring.read_at                                                */
    uint32_t meta_len;     /* metadata_ring.len()                                                  */
    uint32_t dst_cap;      /* bytes available at dst_offset                                        */
    uint32_t max_dgrams;   /* 1 .. SMOL_MAX_SOCKET_DGRAMS: PACKET entries this call may dequeue    */
    uint16_t port;         /* endpoint.port: the source port                                       */
    uint16_t ip_mtu;       /* DeviceCapabilities::ip_mtu()                                         */
    uint8_t hop_limit;     /* hop_limit.unwrap_or(64), resolved by the caller                      */
    uint8_t flags;         /* SMOL_UTXS_*; other bits must be 0                                    */
    uint8_t eth_dst[6];    /* with SMOL_UTXS_ETH: the next hop's hardware address                  */
    uint8_t eth_src[6];    /* with SMOL_UTXS_ETH: the interface's                                  */
    uint8_t reserved[14];  /* must be 0                                                            */
} smol_csum_udptxsock_t;
#define SMOL_UTXS_ETH 0x01u /* frames carry an Ethernet header */

/* One dequeued datagram (16 bytes, 16-byte-aligned device array, output): entry tx_first + k is for the k-th
 * PACKET entry the group dequeued. */
typedef struct {
    uint32_t frame_off; /* of its frame, relative to dst_offset (OVERSIZE: where the next frame starts)  */
    uint32_t ring_off;  /* payload-ring index of the first payload byte                                  */
    uint32_t meta_idx;  /* metadata-ring index of its entry                                              */
    uint16_t ip_len;    /* the IP packet's length: the frame is io + ip_len bytes (0 with OVERSIZE)      */
    uint8_t flags;      /* SMOL_UTX_*                                                                    */
    uint8_t reserved;   /* 0 */
} smol_csum_udptx_t;
#define SMOL_UTX_SENT     0x01u /* its frame is written                                          */
#define SMOL_UTX_OVERSIZE 0x02u /* ip_len > ip_mtu: dequeued, no frame written                   */
#define SMOL_UTX_PADDED   0x04u /* a PADDING entry was dequeued in front of it                   */

/* One socket's outcome (32 bytes, 16-byte-aligned device array, output; one per GROUP). */
typedef struct {
    uint32_t payload_read; /* the ring state after the call: what the caller copies into its PacketBuffer */
    uint32_t payload_len;
    uint32_t meta_read;
    uint32_t meta_len;
    uint32_t sent;         /* entries with SMOL_UTX_SENT     */
    uint32_t oversize;     /* entries with SMOL_UTX_OVERSIZE */
    uint32_t bytes;        /* where the next frame would have started, relative to dst_offset (at most 2^32 - 1) */
    uint8_t stop;          /* SMOL_UTX_STOP_*: why the group stopped dequeueing */
    uint8_t valid;         /* 1: the socket entry was usable */
    uint8_t reserved[2];   /* 0 */
} smol_csum_udptxout_t;
#define SMOL_UTX_STOP_EMPTY   1u /* the metadata ring ran empty                                        */
#define SMOL_UTX_STOP_MAX     2u /* max_dgrams PACKET entries were dequeued                            */
#define SMOL_UTX_STOP_NOSPACE 3u /* the next frame does not fit; its datagram stays queued             */
#define SMOL_UTX_STOP_CORRUPT 4u /* the front entry is not a PACKET entry the payload ring can hold    */

/* The send-side mirror of smol_csum_batch_verify_udp_enqueue: every socket's transmit PacketBuffer dequeued in
 * order and each datagram written out as a whole frame, Ethernet (optional), IPv4 or IPv6 and UDP headers
 * built on the device, both checksums filled, in one pass over the payload bytes.  In the reference a UDP send
 * is UdpSocket::dispatch (src/socket/udp.rs:535-592): tx_buffer.dequeue_with skips a padding entry and hands
 * out one contiguous payload (src/storage/packet_buffer.rs:169-204; src/storage/ring_buffer.rs:145-161,
 * 239-268), dispatch_ip writes the Ethernet and IP headers (src/iface/interface/mod.rs:1245-1268, 1359-1395;
 * src/wire/ipv4.rs:584-611, src/wire/ipv6.rs:628-640), UdpRepr::emit copies the payload and fill_checksum sums
 * it again (src/wire/udp.rs:286-309, 194-208): two passes over every payload byte behind a serial walk of the
 * metadata ring.  There is no smol_csum_batch_t: the input is the sockets' buffers.  A group is one socket.
 *
 * Metadata entries.  smol_csum_udpmeta_t is read with its send-side meaning: size is the payload bytes,
 * src_port is endpoint.port, the DESTINATION port, remote_addr the destination address, local_addr the source
 * address, which the caller has resolved (udp.rs:543-560); family is 4 or 6, and for IPv4 only the first 4
 * address bytes are read; record and reserved are not read.  This is exactly the entry
 * smol_csum_batch_verify_udp_enqueue writes for a received datagram, so a receive ring handed to this call
 * unchanged is answered datagram by datagram, each reply going back to its sender from the address it was sent
 * to.  Metadata index i of a group is d_meta[meta_first + i].
 *
 * The dequeue rule.  State (pr, pl, mr, ml) over the capacities P and M as for the enqueue rule.  One step is
 * one dispatch call:
 *   1. dequeue_padding (packet_buffer.rs:156-167).  When ml > 0 and the entry at mr is PADDING:
 *      n = min(size, pl, P - pr), the clamp of dequeue_many; pr = (pr + n) % P, or 0 when P == 0; pl -= n;
 *      mr = (mr + 1) % M; ml -= 1.  This happens whatever follows.
 *   2. ml == 0: stop EMPTY.
 *   3. The entry at mr must be PACKET with family 4 or 6 and size <= min(pl, P - pr) (the reference's unwrap and
 *      debug_assert).  Otherwise stop CORRUPT; nothing more is dequeued.
 *   4. ihl = 20 or 40; ip_len = ihl + 8 + size; io = 14 with SMOL_UTXS_ETH, else 0.
 *   5. ip_len > ip_mtu: OVERSIZE.  The datagram IS dequeued, as dispatch_ip returning Ok does for the IPv4
 *      fragmentation branch and for the IPv6 drop alike (mod.rs:1276-1358, 1378-1382).  Its entry carries
 *      ring_off and meta_idx, no frame is written and the place of the next frame does not advance.  The
 *      caller feeds an IPv4 one to smol_csum_batch_fragment_emit before it reuses the ring space.
 *   6. Otherwise the frame is placed: with frame_stride S != 0 at frame_off = S * (frames SENT so far), with
 *      frame_stride == 0 at the sum of the earlier frames' lengths (back to back, any alignment).  It does not
 *      fit when frame_off + io + ip_len > dst_cap, or S != 0 and io + ip_len > S: stop NOSPACE, and the datagram
 *      stays queued (device.transmit returning None, mod.rs:724-727; dequeue_with's Err arm,
 *      packet_buffer.rs:199).  A padding entry step 1 dequeued in front of it is gone.
 *   7. It is dequeued: ring_off = pr; pr = (pr + size) % P; pl -= size; mr = (mr + 1) % M; ml -= 1.
 * Steps repeat until a stop, or until max_dgrams PACKET entries have been dequeued (SENT or OVERSIZE): stop
 * MAX.  No further step starts then, so a padding entry behind the last one stays queued.
 *
 * An invalid group: reserved bytes not 0, unknown flag bits, max_dgrams 0 or above SMOL_MAX_SOCKET_DGRAMS, or
 * a ring state outside smol_csum_udpsock_t's contract (payload_len > payload_cap, meta_len > meta_cap, a read
 * index not below its capacity, with capacity 0 not 0).  Nothing is read from its rings, no frame or d_tx entry
 * is written, and its d_out entry is all zero.
 *
 * The frame, byte for byte what smol_csum_batch_emit leaves in the same frame built on the host, under caps:
 *   - Ethernet, with SMOL_UTXS_ETH: eth_dst, eth_src, ethertype 0x0800 / 0x86DD.
 *   - IPv4 (Ipv4Repr::emit): 45 00, total length ip_len, ident 0, 40 00 (DF), hop_limit, protocol 17, the header
 *     checksum under caps.ipv4.tx() else 0, source local_addr[0..4], destination remote_addr[0..4].
 *   - IPv6: 60 00 00 00, payload length 8 + size, next header 17, hop_limit, source local_addr, destination
 *     remote_addr.
 *   - UDP: source port `port`, destination port the entry's src_port, length 8 + size, and the checksum, which
 *     under caps.udp.tx() covers the pseudo-header, the header and the payload with a computed 0 written as
 *     0xffff, else 0.
 *   - The payload: d_src[src_offset + ring_off ..][.. size].
 *
 * Reads and writes.  Each payload byte is read once and each frame byte written once.  d_src is read only in
 * 16-byte chunks that hold at least one byte of a SENT payload; d_meta and d_socks are only read.  No byte of
 * d_dst is read, and none outside the SENT frames is written: edges go out as byte-masked stores, never
 * read-modify-write.  d_tx entries past sent + oversize are not written.  Frame areas of different groups
 * must not overlap.
 *
 * What stays with the caller: source-address selection; the neighbour lookup (one next hop per socket entry:
 * a socket that talks to several neighbours is drained without SMOL_UTXS_ETH into strided frames and the
 * caller writes the Ethernet headers); IPv4 fragmentation of OVERSIZE datagrams; the commit of the four state
 * words of d_out into the PacketBuffer, and the waker.
 *
 * Resources.  No context scratch, no event, no allocation; stream-ordered on `stream`, graph-capturable, and
 * calls on different streams are independent (also on one context).
 *
 * SMOL_EINVAL: NULL ctx, bad caps, NULL d_src / d_socks / d_meta / d_dst / d_tx / d_out with n_groups > 0,
 * d_socks, d_meta, d_tx or d_out not 16-byte aligned.  n_groups == 0 returns SMOL_OK and launches nothing.
 *
 * Added within ABI 6 (SMOLCSUM_ABI_VERSION unchanged: the change is additive). */
int smol_csum_batch_udp_dequeue_emit(smol_csum_ctx_t* ctx, const uint8_t* d_src,
                                     const smol_csum_udptxsock_t* d_socks, uint64_t n_groups, /* one per GROUP */
                                     const smol_csum_udpmeta_t* d_meta,  /* the metadata rings, only read */
                                     const smol_checksum_caps_t* caps, uint8_t* d_dst, uint32_t frame_stride,
                                     smol_csum_udptx_t* d_tx,            /* one per dequeued datagram */
                                     smol_csum_udptxout_t* d_out,        /* one per GROUP */
                                     void* stream);

/* ---- 4. 6LoWPAN next-header-compressed UDP (RFC 6282 §4.3) ------------------------------- */

/* The IPv6 source and destination addresses of one record (32 bytes, device memory): 6LoWPAN's
 * IPHC header compresses them (to nothing, when they derive from the link-layer addresses), so the
 * iface's decompression result travels beside the batch. */
typedef struct {
    uint8_t src[16];
    uint8_t dst[16];
} smol_ipv6_addr_pair_t;

/* UdpNhcRepr::emit's checksum (src/wire/sixlowpan/nhc.rs:746-776) over every record: each record
 * is a LOWPAN_NHC UDP packet, from its dispatch byte (0b11110CPP) to the end of the payload; the
 * payload follows an inline checksum (UdpNhcPacket::payload_mut, nhc.rs:622-626).  Under
 * caps.udp.tx() the checksum !combine([pseudo_header_v6(src, dst, Udp, n + 8), src_port,
 * dst_port, n + 8, data(payload)]) is written to the field and the C bit cleared (set_checksum,
 * nhc.rs:676-681; no 0 -> 0xffff mapping); otherwise nothing is written.  The ports are read back
 * from the packet in the encoding set_ports (nhc.rs:635-673) wrote them.  A record shorter than
 * its header or without the UDP dispatch is left untouched and reported SMOL_ST_MALFORMED.
 * `d_addrs` holds n address pairs (4-byte aligned); record kinds are ignored. */
int smol_csum_batch_nhc_udp_emit(smol_csum_ctx_t* ctx, uint8_t* d_buf, const smol_csum_batch_t* batch,
                                 const smol_ipv6_addr_pair_t* d_addrs, const smol_checksum_caps_t* caps,
                                 uint8_t* d_status, void* stream);

/* UdpNhcRepr::parse's checksum gate (src/wire/sixlowpan/nhc.rs:693-729): SMOL_ST_MALFORMED when
 * UdpNhcPacket::check_len (nhc.rs:486-500) or the dispatch test fails, or (ABI 5) when an inline
 * destination port (ports modes 0b00 / 0b10) is 0: the iface parses the decompressed header with
 * UdpRepr::parse, which drops it (src/iface/interface/sixlowpan.rs:745-775, udp.rs:246-248);
 * otherwise under
 * caps.udp.rx() an inline checksum must equal the one computed over the ports as the packet
 * accessors read them (nhc.rs:513-577); an elided checksum (C bit set) is not checked.  The IP
 * bits are always set (no IPv4 header). */
int smol_csum_batch_nhc_udp_verify(smol_csum_ctx_t* ctx, const uint8_t* d_buf,
                                   const smol_csum_batch_t* batch, const smol_ipv6_addr_pair_t* d_addrs,
                                   const smol_checksum_caps_t* caps, uint8_t* d_status, void* stream);

/* Message of the last SMOL_EHIP error on this thread ("" if none). */
const char* smol_csum_last_error(void);

/* ABI version compiled into the library (SMOLCSUM_ABI_VERSION). */
int smol_csum_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SMOLCSUM_H */
