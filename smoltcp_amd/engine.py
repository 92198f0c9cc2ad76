"""Batched device checksum engine over torch device tensors (HBM-resident batches).

``ChecksumEngine`` wraps one ``smol_csum_ctx_t`` (include/smolcsum.h).  Buffers are plain
``torch.uint8`` CUDA(HIP) tensors holding packed records; ``Batch`` describes where the records
are — a fixed stride (no descriptor traffic) or a device array of 16-byte descriptors.  Every
call is asynchronous on the given stream (default: torch's current stream on the engine's
device).  PyTorch is only the allocator/stream provider here; all checksum work runs in the HIP
kernels of libsmolcsum.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import (NO_FIELD, BatchC, Caps, DgramC, EchoC, EchoCfgC, FieldsC, FragOutC, FragPlanC, SlotC, SpanC, TcpFlowC,
                   TcpOutC, TcpPlanC, TcpSegC, TcpWinC, UdpMetaC, UdpRxC, UdpSockC, UdpSockOutC, UdpTxC, UdpTxOutC, UdpTxSockC,
                   UnreachC, check, lib)
from .phy import ChecksumCapabilities

KIND_RAW, KIND_IP, KIND_ETH = 0, 1, 2
REC_IPHDR_ONLY = 0x01  # SMOL_REC_IPHDR_ONLY: a raw socket's frame (the IP header's gate only)
BATCH_FIELD_STORES = 0x80  # SMOL_BATCH_FIELD_STORES: emit stores the checksum fields only (no whole segments)

ST_IP_OK = 0x01
ST_L4_OK = 0x02
ST_L4_PARTIAL = 0x04
ST_IP_VALID = 0x08
ST_L4_VALID = 0x10
ST_MALFORMED = 0x20
ST_UNSUPPORTED = 0x40
ST_ACCEPT = 0x80

SYNTH_UDP4, SYNTH_TCP4, SYNTH_V6MIX, SYNTH_ETH_TCP4, SYNTH_RANDOM = 0, 1, 2, 3, 4

DESC_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("kind", "u1"), ("flags", "u1"),
                       ("reserved", "<u2")])
assert DESC_DTYPE.itemsize == 16

# smol_csum_copy_t: one payload copy per record (smol_csum_batch_copy_emit)
COPY_DTYPE = np.dtype([("src_offset", "<u8"), ("dst_offset", "<u4"), ("len", "<u4")])
assert COPY_DTYPE.itemsize == 16


# smol_csum_frag_group_t: one IPv4 datagram = `count` consecutive records from `first`
FRAG_GROUP_DTYPE = np.dtype([("first", "<u8"), ("count", "<u4"), ("reserved", "<u4")])
assert FRAG_GROUP_DTYPE.itemsize == 16
MAX_FRAGMENTS = 256


# smol_csum_fields_t: one record's emit result (smol_csum_batch_emit_fields)
FIELDS_DTYPE = np.dtype([("off", "<u2", (3,)), ("val", "<u2", (3,)), ("status", "u1"), ("reserved", "u1", (3,))])
assert FIELDS_DTYPE.itemsize == 16 == ctypes.sizeof(FieldsC)


# smol_csum_slot_t / smol_csum_span_t: a record's destination slot and payload span (smol_csum_batch_verify_copy)
SLOT_DTYPE = np.dtype([("dst_offset", "<u8"), ("cap", "<u4"), ("reserved", "<u4")])
assert SLOT_DTYPE.itemsize == 16 == ctypes.sizeof(SlotC)
SPAN_DTYPE = np.dtype([("len", "<u4"), ("off", "<u2"), ("copied", "u1"), ("reserved", "u1")])
assert SPAN_DTYPE.itemsize == 8 == ctypes.sizeof(SpanC)
# smol_csum_dgram_t: one reassembled datagram per fragment group (smol_csum_batch_verify_reassemble)
DGRAM_DTYPE = np.dtype([("len", "<u4"), ("l4_len", "<u4"), ("l4_off", "<u2"), ("protocol", "u1"), ("copied", "u1"),
                        ("reserved", "<u4")])
assert DGRAM_DTYPE.itemsize == 16 == ctypes.sizeof(DgramC)
# smol_csum_fragplan_t / smol_csum_fragout_t: one datagram's cut and what became of it (smol_csum_batch_fragment_emit)
FRAGPLAN_DTYPE = np.dtype([("dst_offset", "<u8"), ("cap", "<u4"), ("ip_mtu", "<u2"), ("ident", "<u2")])
assert FRAGPLAN_DTYPE.itemsize == 16 == ctypes.sizeof(FragPlanC)
FRAGOUT_DTYPE = np.dtype([("count", "<u4"), ("frame_len", "<u4"), ("last_len", "<u4"), ("status", "u1"), ("written", "u1"),
                          ("reserved", "<u2")])
assert FRAGOUT_DTYPE.itemsize == 16 == ctypes.sizeof(FragOutC)
# smol_csum_tcpplan_t / smol_csum_tcpout_t: one send's cut and what became of it (smol_csum_batch_tcp_segment_emit)
TCPPLAN_DTYPE = np.dtype([("src_offset", "<u8"), ("len", "<u4"), ("mss", "<u2"), ("reserved", "<u2"), ("dst_offset", "<u8"),
                          ("cap", "<u4"), ("reserved2", "<u4")])
assert TCPPLAN_DTYPE.itemsize == 32 == ctypes.sizeof(TcpPlanC)
TCPOUT_DTYPE = np.dtype([("count", "<u4"), ("frame_len", "<u4"), ("last_len", "<u4"), ("status", "u1"), ("written", "u1"),
                         ("reserved", "<u2")])
assert TCPOUT_DTYPE.itemsize == 16 == ctypes.sizeof(TcpOutC)
# smol_csum_tcpwin_t / smol_csum_tcpseg_t / smol_csum_tcpflow_t: a connection's receive window, a record's and a
# connection's outcome (smol_csum_batch_verify_tcp_assemble)
TCPWIN_DTYPE = np.dtype([("dst_offset", "<u8"), ("ring_len", "<u4"), ("ring_pos", "<u4"), ("window_start", "<u4"),
                         ("window_len", "<u4"), ("reserved", "<u4", (2,))])
assert TCPWIN_DTYPE.itemsize == 32 == ctypes.sizeof(TcpWinC)
TCPSEG_DTYPE = np.dtype([("seq", "<u4"), ("win_off", "<u4"), ("len", "<u4"), ("off", "<u2"), ("flags", "u1"), ("reserved", "u1")])
assert TCPSEG_DTYPE.itemsize == 16 == ctypes.sizeof(TcpSegC)
TCPFLOW_DTYPE = np.dtype([("contig_len", "<u4"), ("counted", "<u4"), ("redelivered", "<u4"), ("valid", "u1"),
                          ("reserved", "u1", (3,))])
assert TCPFLOW_DTYPE.itemsize == 16 == ctypes.sizeof(TcpFlowC)
MAX_FLOW_SEGMENTS = 256
SEG_TCP, SEG_IN_WINDOW, SEG_COPIED, SEG_REDELIVERED = 0x01, 0x02, 0x04, 0x08  # SMOL_SEG_*
# smol_csum_echo_t: one record's outcome (smol_csum_batch_verify_echo_reply)
ECHO_DTYPE = np.dtype([("frame_len", "<u4"), ("data_off", "<u2"), ("head_len", "u1"), ("flags", "u1")])
assert ECHO_DTYPE.itemsize == 8 == ctypes.sizeof(EchoC)
ECHO_REQUEST, ECHO_ANSWERED, ECHO_WRITTEN, ECHO_SEND, ECHO_HOST = 0x01, 0x02, 0x04, 0x08, 0x10  # SMOL_ECHO_*
# smol_csum_unreach_t: one record's outcome (smol_csum_batch_verify_unreach_reply)
UNR_DTYPE = np.dtype([("frame_len", "<u4"), ("data_off", "<u2"), ("head_len", "u1"), ("flags", "u1")])
assert UNR_DTYPE.itemsize == 8 == ctypes.sizeof(UnreachC)
UNR_REFUSED, UNR_ANSWERED, UNR_WRITTEN, UNR_SEND, UNR_HOST, UNR_PORT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20  # SMOL_UNR_*
# smol_csum_udpsock_t / smol_csum_udpmeta_t / smol_csum_udprx_t / smol_csum_udpsockout_t: a UDP socket's receive
# buffer before the poll, a metadata-ring entry, a record's and a socket's outcome (smol_csum_batch_verify_udp_enqueue)
UDPSOCK_DTYPE = np.dtype([("dst_offset", "<u8"), ("meta_first", "<u8"), ("payload_cap", "<u4"), ("payload_read", "<u4"),
                          ("payload_len", "<u4"), ("meta_cap", "<u4"), ("meta_read", "<u4"), ("meta_len", "<u4"),
                          ("port", "<u2"), ("reserved", "<u2", (3,))])
assert UDPSOCK_DTYPE.itemsize == 48 == ctypes.sizeof(UdpSockC)
UDPMETA_DTYPE = np.dtype([("size", "<u4"), ("record", "<u4"), ("src_port", "<u2"), ("family", "u1"), ("kind", "u1"),
                          ("reserved", "u1", (4,)), ("remote_addr", "u1", (16,)), ("local_addr", "u1", (16,))])
assert UDPMETA_DTYPE.itemsize == 48 == ctypes.sizeof(UdpMetaC)
UDPRX_DTYPE = np.dtype([("ring_off", "<u4"), ("len", "<u4"), ("meta_idx", "<u4"), ("off", "<u2"), ("flags", "u1"),
                        ("reserved", "u1")])
assert UDPRX_DTYPE.itemsize == 16 == ctypes.sizeof(UdpRxC)
UDPSOCKOUT_DTYPE = np.dtype([("payload_read", "<u4"), ("payload_len", "<u4"), ("meta_read", "<u4"), ("meta_len", "<u4"),
                             ("enqueued", "<u4"), ("full", "<u4"), ("restored", "<u4"), ("valid", "u1"),
                             ("reserved", "u1", (3,))])
assert UDPSOCKOUT_DTYPE.itemsize == 32 == ctypes.sizeof(UdpSockOutC)
MAX_SOCKET_DGRAMS = 256
URX_UDP, URX_ENQUEUED, URX_FULL, URX_PADDED, URX_RESTORED = 0x01, 0x02, 0x04, 0x08, 0x10  # SMOL_URX_*
UMETA_PACKET, UMETA_PADDING = 1, 2  # SMOL_UMETA_*
# smol_csum_udptxsock_t / smol_csum_udptx_t / smol_csum_udptxout_t: a UDP socket's transmit buffer before the call
# and where its frames go, a dequeued datagram's and a socket's outcome (smol_csum_batch_udp_dequeue_emit)
UDPTXSOCK_DTYPE = np.dtype([("src_offset", "<u8"), ("meta_first", "<u8"), ("dst_offset", "<u8"), ("tx_first", "<u8"),
                            ("payload_cap", "<u4"), ("payload_read", "<u4"), ("payload_len", "<u4"), ("meta_cap", "<u4"),
                            ("meta_read", "<u4"), ("meta_len", "<u4"), ("dst_cap", "<u4"), ("max_dgrams", "<u4"),
                            ("port", "<u2"), ("ip_mtu", "<u2"), ("hop_limit", "u1"), ("flags", "u1"), ("eth_dst", "u1", (6,)),
                            ("eth_src", "u1", (6,)), ("reserved", "u1", (14,))])
assert UDPTXSOCK_DTYPE.itemsize == 96 == ctypes.sizeof(UdpTxSockC)
UDPTX_DTYPE = np.dtype([("frame_off", "<u4"), ("ring_off", "<u4"), ("meta_idx", "<u4"), ("ip_len", "<u2"), ("flags", "u1"),
                        ("reserved", "u1")])
assert UDPTX_DTYPE.itemsize == 16 == ctypes.sizeof(UdpTxC)
UDPTXOUT_DTYPE = np.dtype([("payload_read", "<u4"), ("payload_len", "<u4"), ("meta_read", "<u4"), ("meta_len", "<u4"),
                           ("sent", "<u4"), ("oversize", "<u4"), ("bytes", "<u4"), ("stop", "u1"), ("valid", "u1"),
                           ("reserved", "u1", (2,))])
assert UDPTXOUT_DTYPE.itemsize == 32 == ctypes.sizeof(UdpTxOutC)
UTXS_ETH = 0x01  # SMOL_UTXS_ETH
UTX_SENT, UTX_OVERSIZE, UTX_PADDED = 0x01, 0x02, 0x04  # SMOL_UTX_*
UTX_STOP_EMPTY, UTX_STOP_MAX, UTX_STOP_NOSPACE, UTX_STOP_CORRUPT = 1, 2, 3, 4  # SMOL_UTX_STOP_*


def make_port_map(open_ports) -> np.ndarray:
    """The 8192-byte bitmap smol_csum_batch_verify_unreach_reply takes as d_udp_open (copy it to the device): bit
    p & 7 of byte p >> 3 set for every UDP destination port p of `open_ports`, the ports the host wants the
    datagrams of itself."""
    m = np.zeros(8192, dtype=np.uint8)
    for p in open_ports:
        p = int(p)
        assert 0 <= p <= 0xFFFF
        m[p >> 3] |= 1 << (p & 7)
    return m


def make_slots(dst_offsets, caps) -> np.ndarray:
    """Host array of smol_csum_slot_t (view it as uint8 and copy it to the device)."""
    n = len(dst_offsets)
    s = np.zeros(n, dtype=SLOT_DTYPE)
    s["dst_offset"] = np.asarray(dst_offsets, dtype=np.uint64)
    s["cap"] = np.broadcast_to(np.asarray(caps, dtype=np.uint32), (n,))
    return s


def make_fragplans(dst_offsets, caps, ip_mtus, idents) -> np.ndarray:
    """Host array of smol_csum_fragplan_t (view it as uint8 and copy it to the device)."""
    n = len(dst_offsets)
    p = np.zeros(n, dtype=FRAGPLAN_DTYPE)
    p["dst_offset"] = np.asarray(dst_offsets, dtype=np.uint64)
    p["cap"] = np.broadcast_to(np.asarray(caps, dtype=np.uint32), (n,))
    p["ip_mtu"] = np.broadcast_to(np.asarray(ip_mtus, dtype=np.uint16), (n,))
    p["ident"] = np.broadcast_to(np.asarray(idents, dtype=np.uint16), (n,))
    return p


def make_tcpplans(src_offsets, lens, msss, dst_offsets, caps) -> np.ndarray:
    """Host array of smol_csum_tcpplan_t (view it as uint8 and copy it to the device)."""
    n = len(src_offsets)
    p = np.zeros(n, dtype=TCPPLAN_DTYPE)
    p["src_offset"] = np.asarray(src_offsets, dtype=np.uint64)
    p["len"] = np.broadcast_to(np.asarray(lens, dtype=np.uint32), (n,))
    p["mss"] = np.broadcast_to(np.asarray(msss, dtype=np.uint16), (n,))
    p["dst_offset"] = np.asarray(dst_offsets, dtype=np.uint64)
    p["cap"] = np.broadcast_to(np.asarray(caps, dtype=np.uint32), (n,))
    return p


def make_tcpwins(dst_offsets, ring_lens, ring_poss, window_starts, window_lens) -> np.ndarray:
    """Host array of smol_csum_tcpwin_t (view it as uint8 and copy it to the device)."""
    n = len(dst_offsets)
    w = np.zeros(n, dtype=TCPWIN_DTYPE)
    w["dst_offset"] = np.asarray(dst_offsets, dtype=np.uint64)
    w["ring_len"] = np.broadcast_to(np.asarray(ring_lens, dtype=np.uint32), (n,))
    w["ring_pos"] = np.broadcast_to(np.asarray(ring_poss, dtype=np.uint32), (n,))
    w["window_start"] = np.broadcast_to(np.asarray(window_starts, dtype=np.uint32), (n,))
    w["window_len"] = np.broadcast_to(np.asarray(window_lens, dtype=np.uint32), (n,))
    return w


def make_udpsocks(dst_offsets, meta_firsts, payload_caps, payload_reads, payload_lens, meta_caps, meta_reads, meta_lens,
                  ports) -> np.ndarray:
    """Host array of smol_csum_udpsock_t (view it as uint8 and copy it to the device): per socket, where its
    payload ring's storage lies in `dst`, where its metadata ring's first entry lies in `meta`, the two rings'
    capacity / read index / length as the PacketBuffer holds them before the poll, and the bound port."""
    n = len(dst_offsets)
    s = np.zeros(n, dtype=UDPSOCK_DTYPE)
    s["dst_offset"] = np.asarray(dst_offsets, dtype=np.uint64)
    s["meta_first"] = np.broadcast_to(np.asarray(meta_firsts, dtype=np.uint64), (n,))
    for name, val in (("payload_cap", payload_caps), ("payload_read", payload_reads), ("payload_len", payload_lens),
                      ("meta_cap", meta_caps), ("meta_read", meta_reads), ("meta_len", meta_lens)):
        s[name] = np.broadcast_to(np.asarray(val, dtype=np.uint32), (n,))
    s["port"] = np.broadcast_to(np.asarray(ports, dtype=np.uint16), (n,))
    return s


def make_udptxsocks(src_offsets, meta_firsts, dst_offsets, tx_firsts, payload_caps, payload_reads, payload_lens, meta_caps,
                    meta_reads, meta_lens, dst_caps, max_dgrams, ports, ip_mtus, hop_limits=64, eth=None) -> np.ndarray:
    """Host array of smol_csum_udptxsock_t (view it as uint8 and copy it to the device): per socket, where its
    payload ring's storage lies in `src`, its metadata ring's first entry in `meta`, its first frame in `dst` and
    its first entry in `tx`; the two rings' capacity / read index / length as the PacketBuffer holds them before
    the call; the bytes available for frames, the datagrams the call may dequeue, the source port, the IP MTU and
    the hop limit.  `eth`: None for frames without an Ethernet header, else (eth_dst, eth_src), six bytes each (one
    pair for all sockets, or n x 6 arrays)."""
    n = len(src_offsets)
    s = np.zeros(n, dtype=UDPTXSOCK_DTYPE)
    s["src_offset"] = np.asarray(src_offsets, dtype=np.uint64)
    for name, val in (("meta_first", meta_firsts), ("dst_offset", dst_offsets), ("tx_first", tx_firsts)):
        s[name] = np.broadcast_to(np.asarray(val, dtype=np.uint64), (n,))
    for name, val in (("payload_cap", payload_caps), ("payload_read", payload_reads), ("payload_len", payload_lens),
                      ("meta_cap", meta_caps), ("meta_read", meta_reads), ("meta_len", meta_lens), ("dst_cap", dst_caps),
                      ("max_dgrams", max_dgrams)):
        s[name] = np.broadcast_to(np.asarray(val, dtype=np.uint32), (n,))
    s["port"] = np.broadcast_to(np.asarray(ports, dtype=np.uint16), (n,))
    s["ip_mtu"] = np.broadcast_to(np.asarray(ip_mtus, dtype=np.uint16), (n,))
    s["hop_limit"] = np.broadcast_to(np.asarray(hop_limits, dtype=np.uint8), (n,))
    if eth is not None:
        s["flags"] = UTXS_ETH
        s["eth_dst"] = np.broadcast_to(np.frombuffer(bytes(eth[0]), np.uint8) if isinstance(eth[0], (bytes, bytearray))
                                       else np.asarray(eth[0], dtype=np.uint8), (n, 6))
        s["eth_src"] = np.broadcast_to(np.frombuffer(bytes(eth[1]), np.uint8) if isinstance(eth[1], (bytes, bytearray))
                                       else np.asarray(eth[1], dtype=np.uint8), (n, 6))
    return s


def apply_fields(host_buf: np.ndarray, record_offsets, record_lens, fields) -> np.ndarray:
    """The host half of emit_fields, vectorised: write every entry's fields into its record of the
    uint8 array `host_buf` (record i at record_offsets[i], record_lens[i] bytes; scalars broadcast),
    big-endian, as smol_csum_apply_fields does per record.  `fields`: n entries, FIELDS_DTYPE or their
    n x 16 uint8 view.  Returns a bool array: False where a field did not fit its record
    (smol_csum_apply_fields' SMOL_ERANGE: nothing of that record is written)."""
    f = np.ascontiguousarray(fields)
    cols = np.ascontiguousarray(f.view(np.uint8).reshape(-1, 16).view("<u2")[:, :6].T)  # off[0..2], val[0..2]: contiguous
    n = cols.shape[1]
    offs = np.broadcast_to(np.asarray(record_offsets, dtype=np.int64), (n,))
    lens = np.asarray(record_lens, dtype=np.int64)
    lens = lens if lens.ndim == 0 else np.broadcast_to(lens, (n,))
    have = cols[:3] != NO_FIELD
    ok = ~(have & (cols[:3].astype(np.int32) + 2 > lens)).any(axis=0)
    all_ok = bool(ok.all())
    for j in range(3):  # one pass per slot, both bytes while the line is near: a record's fields never overlap
        m = have[j] if all_ok else have[j] & ok
        if not m.any():
            continue
        whole = bool(m.all())
        pos = offs + cols[j] if whole else offs[m] + cols[j][m]
        v = cols[3 + j] if whole else cols[3 + j][m]
        host_buf[pos] = (v >> 8).astype(np.uint8)
        host_buf[pos + 1] = v.astype(np.uint8)
    return ok


def make_groups(firsts, counts) -> np.ndarray:
    """Host array of smol_csum_frag_group_t (view it as uint8 and copy it to the device)."""
    g = np.zeros(len(firsts), dtype=FRAG_GROUP_DTYPE)
    g["first"] = np.asarray(firsts, dtype=np.uint64)
    g["count"] = np.asarray(counts, dtype=np.uint32)
    return g


def make_copies(src_offsets, dst_offsets, lengths) -> np.ndarray:
    """Host array of smol_csum_copy_t (view it as uint8 and copy it to the device)."""
    n = len(src_offsets)
    c = np.zeros(n, dtype=COPY_DTYPE)
    c["src_offset"] = np.asarray(src_offsets, dtype=np.uint64)
    c["dst_offset"] = np.broadcast_to(np.asarray(dst_offsets, dtype=np.uint32), (n,))
    c["len"] = np.broadcast_to(np.asarray(lengths, dtype=np.uint32), (n,))
    return c


def make_descriptors(offsets, lengths, kinds, flags=0) -> np.ndarray:
    """Host array of smol_csum_desc_t (view it as uint8 and copy it to the device)."""
    n = len(offsets)
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["offset"] = np.asarray(offsets, dtype=np.uint64)
    d["len"] = np.asarray(lengths, dtype=np.uint32)
    d["kind"] = np.broadcast_to(np.asarray(kinds, dtype=np.uint8), (n,))
    d["flags"] = np.broadcast_to(np.asarray(flags, dtype=np.uint8), (n,))
    return d


@dataclass
class Batch:
    """smol_csum_batch_t: ``desc`` is a device tensor of n*16 bytes, or None for a fixed stride."""

    n: int
    stride: int = 0
    length: int = 0
    kind: int = KIND_IP
    desc: Optional[object] = None  # torch.Tensor (uint8, device) holding n descriptors
    flags: int = 0                 # SMOL_REC_* of every record of a fixed-stride batch, | SMOL_BATCH_*

    def c(self) -> BatchC:
        b = BatchC()
        b.desc = self.desc.data_ptr() if self.desc is not None else None
        b.n = self.n
        b.stride = self.stride
        b.len = self.length
        b.kind = self.kind
        b.flags = self.flags
        return b

    @staticmethod
    def fixed(n: int, stride: int, length: Optional[int] = None, kind: int = KIND_IP, flags: int = 0) -> "Batch":
        return Batch(n=n, stride=stride, length=stride if length is None else length, kind=kind, flags=flags)

    @staticmethod
    def from_records(offsets, lengths, kinds, device, flags=0, batch_flags: int = 0) -> "Batch":
        """`flags`: SMOL_REC_* per record (descriptor flags); `batch_flags`: SMOL_BATCH_* of the batch."""
        import torch

        d = make_descriptors(offsets, lengths, kinds, flags)
        t = torch.from_numpy(d.view(np.uint8).copy()).to(device)
        return Batch(n=len(d), desc=t, flags=batch_flags)


def _caps(caps) -> Caps:
    if caps is None:
        caps = ChecksumCapabilities()
    tup = caps.as_tuple() if isinstance(caps, ChecksumCapabilities) else tuple(int(x) for x in caps)
    c = Caps()
    c.ipv4, c.udp, c.tcp, c.icmpv4, c.icmpv6 = tup
    return c


def segment_bitmap(addrs, nbytes: int):
    """The segment probe's bitmap for 2-byte fields at the byte offsets `addrs` (device int64 tensor) of
    an `nbytes` buffer: bit s set for every 64-B segment s holding a field byte, ceil(nbytes / 8192) * 4
    int32 words (whole 8-KiB pieces of 128 segments)."""
    import torch

    nseg = (nbytes + 8191) // 8192 * 128
    flags = torch.zeros(nseg, dtype=torch.int64, device=addrs.device)
    flags[addrs >> 6] = 1
    flags[(addrs + 1) >> 6] = 1
    words = (flags.view(-1, 32) << torch.arange(32, device=addrs.device, dtype=torch.int64)).sum(dim=1)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words)
    return words.to(torch.int32).contiguous(), int(flags.sum().item())


class ChecksumEngine:
    """One device context.  Not thread-safe: use one engine per host thread."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        """`lib_path`: another build of the library (the experiments build, `_lib.EXP_LIB_PATH`)."""
        self.device = int(device)
        self._L = lib(lib_path)
        h = ctypes.c_void_p()
        check(self._L.smol_csum_ctx_create(self.device, ctypes.byref(h)), "smol_csum_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.smol_csum_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers ----
    def _stream(self, stream):
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))

    @staticmethod
    def _check_buf(buf, batch: Batch):
        assert buf.is_cuda and buf.dtype.itemsize == 1, "buffer must be a uint8 device tensor"
        assert buf.is_contiguous()
        if batch.desc is None and batch.n:
            need = (batch.n - 1) * batch.stride + batch.length
            assert need <= buf.numel(), f"batch needs {need} bytes, buffer has {buf.numel()}"

    # ---- reference surface ----
    def data(self, buf, batch: Batch, out=None, stream=None):
        """out[i] = checksum::data(record i) (int16 tensor holding the u16 bit pattern)."""
        import torch

        self._check_buf(buf, batch)
        if out is None:
            out = torch.empty(batch.n, dtype=torch.int16, device=buf.device)
        b = batch.c()
        check(self._L.smol_csum_batch_data(self._h, buf.data_ptr(), ctypes.byref(b), out.data_ptr(),
                                         self._stream(stream)), "smol_csum_batch_data")
        return out

    def emit(self, buf, batch: Batch, caps=None, status=None, stream=None):
        """In-place fill (Repr::emit gates under ``caps``); returns ``status`` (may be None)."""
        self._check_buf(buf, batch)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_emit(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                         status.data_ptr() if status is not None else None,
                                         self._stream(stream)), "smol_csum_batch_emit")
        return status

    def emit_fields(self, buf, batch: Batch, caps=None, fields=None, stream=None):
        """Emit's values without the writes (smol_csum_batch_emit_fields): returns an n x 16 uint8
        device tensor of smol_csum_fields_t (view its host copy as FIELDS_DTYPE; apply_fields patches
        host frames with it).  `buf` is only read."""
        import torch

        self._check_buf(buf, batch)
        if fields is None:
            fields = torch.empty((batch.n, 16), dtype=torch.uint8, device=buf.device)
        assert fields.is_cuda and fields.is_contiguous() and fields.numel() >= 16 * batch.n
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_emit_fields(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                fields.data_ptr(), self._stream(stream)),
              "smol_csum_batch_emit_fields")
        return fields

    def copy_emit(self, buf, batch: Batch, src, copies, caps=None, status=None, stream=None):
        """Fused payload copy + emit (smol_csum_batch_copy_emit): ``copies`` is a device uint8
        tensor of n smol_csum_copy_t (see make_copies), ``src`` the payload source tensor."""
        self._check_buf(buf, batch)
        assert src.is_cuda and copies.is_cuda and copies.numel() >= 16 * batch.n
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_copy_emit(self._h, buf.data_ptr(), ctypes.byref(b), src.data_ptr(),
                                              copies.data_ptr(), ctypes.byref(c),
                                              status.data_ptr() if status is not None else None,
                                              self._stream(stream)), "smol_csum_batch_copy_emit")
        return status

    def emit_frag(self, buf, batch: Batch, groups, caps=None, status=None, stream=None):
        """IPv4 fragment groups (smol_csum_batch_emit_frag): ``groups`` is a device uint8 tensor of
        smol_csum_frag_group_t (see make_groups).  Fills every fragment's header and each
        datagram's L4 checksum; returns ``status`` (may be None)."""
        self._check_buf(buf, batch)
        assert groups.is_cuda and groups.numel() % 16 == 0
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_emit_frag(self._h, buf.data_ptr(), ctypes.byref(b), groups.data_ptr(),
                                              groups.numel() // 16, ctypes.byref(c),
                                              status.data_ptr() if status is not None else None,
                                              self._stream(stream)), "smol_csum_batch_emit_frag")
        return status

    def verify_frag(self, buf, batch: Batch, groups, caps=None, status=None, stream=None):
        """IPv4 fragment groups (smol_csum_batch_verify_frag): status bytes of every grouped record
        (records outside the groups keep their value; a fresh status tensor starts zeroed)."""
        import torch

        self._check_buf(buf, batch)
        assert groups.is_cuda and groups.numel() % 16 == 0
        if status is None:
            status = torch.zeros(batch.n, dtype=torch.uint8, device=buf.device)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify_frag(self._h, buf.data_ptr(), ctypes.byref(b), groups.data_ptr(),
                                                groups.numel() // 16, ctypes.byref(c), status.data_ptr(),
                                                self._stream(stream)), "smol_csum_batch_verify_frag")
        return status

    def verify_reassemble(self, buf, batch: Batch, groups, dst, slots, caps=None, status=None, dgrams=None, stream=None):
        """verify_frag, and in the same pass every usable group's fragment payloads put together in the
        group's slot of `dst` (smol_csum_batch_verify_reassemble).  `groups`: as verify_frag; `slots`: a
        device uint8 tensor of one smol_csum_slot_t per GROUP (see make_slots); `dst`: the destination uint8
        device tensor, written only inside the delivered datagrams.  Returns (status, dgrams): verify_frag's
        status bytes (one per record; a fresh tensor starts zeroed) and an n_groups x 16 uint8 device tensor
        of smol_csum_dgram_t (view its host copy as DGRAM_DTYPE).  The copy does not wait for the verdict:
        commit a slot only when every status byte of its group has ST_ACCEPT."""
        import torch

        self._check_buf(buf, batch)
        assert groups.is_cuda and groups.numel() % 16 == 0
        ng = groups.numel() // 16
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert slots.is_cuda and slots.is_contiguous() and slots.numel() * slots.dtype.itemsize >= 16 * ng
        if status is None:
            status = torch.zeros(batch.n, dtype=torch.uint8, device=buf.device)
        if dgrams is None:
            dgrams = torch.empty((ng, 16), dtype=torch.uint8, device=buf.device)
        assert dgrams.is_cuda and dgrams.is_contiguous() and dgrams.numel() * dgrams.dtype.itemsize >= 16 * ng
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify_reassemble(self._h, buf.data_ptr(), ctypes.byref(b), groups.data_ptr(), ng,
                                                      ctypes.byref(c), dst.data_ptr(), slots.data_ptr(),
                                                      status.data_ptr(), dgrams.data_ptr(), self._stream(stream)),
              "smol_csum_batch_verify_reassemble")
        return status, dgrams

    def _check_cut(self, buf, batch: Batch, dst, plans, plan_bytes: int, frame_stride: int, out):
        """The argument checks fragment_emit and tcp_segment_emit share (batch buffer, destination, one
        plan_bytes plan per record, frame stride, result entries); returns `out`, a fresh n x 16 tensor if None."""
        import torch

        self._check_buf(buf, batch)
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert plans.is_cuda and plans.is_contiguous() and plans.numel() * plans.dtype.itemsize >= plan_bytes * batch.n
        assert 0 <= int(frame_stride) < 1 << 32
        if out is None:
            out = torch.empty((batch.n, 16), dtype=torch.uint8, device=buf.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.dtype.itemsize >= 16 * batch.n
        return out

    def fragment_emit(self, buf, batch: Batch, dst, plans, frame_stride: int = 0, caps=None, out=None, stream=None):
        """Emit, and in the same pass every whole IPv4 datagram of the batch cut into the frames the iface
        sends, at its place in `dst` (smol_csum_batch_fragment_emit).  `plans`: a device uint8 tensor of one
        smol_csum_fragplan_t per record (see make_fragplans); `frame_stride`: bytes from one frame of a
        datagram to the next (0: back to back); `dst`: the destination uint8 device tensor, written only
        inside the frames.  Returns an n x 16 uint8 device tensor of smol_csum_fragout_t (view its host copy
        as FRAGOUT_DTYPE).  `buf` is only read."""
        out = self._check_cut(buf, batch, dst, plans, 16, frame_stride, out)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_fragment_emit(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                  dst.data_ptr(), plans.data_ptr(), int(frame_stride),
                                                  out.data_ptr(), self._stream(stream)),
              "smol_csum_batch_fragment_emit")
        return out

    def tcp_segment_emit(self, buf, batch: Batch, src, dst, plans, frame_stride: int = 0, caps=None, out=None, stream=None):
        """Every send cut into MSS-sized TCP segments at its place in `dst`, every checksum filled, in one
        pass over the payload (smol_csum_batch_tcp_segment_emit).  Each record of the batch is one header
        template (Ethernet if any, IP, TCP with options, no payload); `plans`: a device uint8 tensor of one
        smol_csum_tcpplan_t per record (see make_tcpplans), naming the send's payload range in `src`;
        `frame_stride`: bytes from one frame of a send to the next (0: back to back); `dst`: the destination
        uint8 device tensor, written only inside the frames.  Returns an n x 16 uint8 device tensor of
        smol_csum_tcpout_t (view its host copy as TCPOUT_DTYPE).  `buf` and `src` are only read."""
        assert src.is_cuda and src.dtype.itemsize == 1 and src.is_contiguous()
        out = self._check_cut(buf, batch, dst, plans, 32, frame_stride, out)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_tcp_segment_emit(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                     src.data_ptr(), dst.data_ptr(), plans.data_ptr(),
                                                     int(frame_stride), out.data_ptr(), self._stream(stream)),
              "smol_csum_batch_tcp_segment_emit")
        return out

    def verify_tcp_assemble(self, buf, batch: Batch, groups, dst, wins, caps=None, status=None, segs=None, flows=None,
                            stream=None):
        """verify, and in the same pass every TCP segment's payload put at the place its sequence number gives
        it in its connection's receive ring in `dst`, trimmed to the receive window
        (smol_csum_batch_verify_tcp_assemble).  `groups`: a device uint8 tensor of smol_csum_frag_group_t (see
        make_groups), one per connection: its frames of this poll, consecutive records in arrival order;
        `wins`: a device uint8 tensor of one smol_csum_tcpwin_t per GROUP (see make_tcpwins); `dst`: the
        destination uint8 device tensor, written only inside the delivered ranges.  Returns (status, segs,
        flows): verify's status byte per record (a fresh tensor starts zeroed; records outside the groups keep
        their value), an n x 16 uint8 device tensor of smol_csum_tcpseg_t (view its host copy as TCPSEG_DTYPE;
        a fresh one starts zeroed) and an n_groups x 16 one of smol_csum_tcpflow_t (TCPFLOW_DTYPE).  The copy
        does not wait for the verdict: commit `contig_len` bytes of a ring (enqueue_unallocated) and feed the
        counted out-of-order entries to the socket's assembler."""
        import torch

        self._check_buf(buf, batch)
        assert groups.is_cuda and groups.numel() % 16 == 0
        ng = groups.numel() // 16
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert wins.is_cuda and wins.is_contiguous() and wins.numel() * wins.dtype.itemsize >= 32 * ng
        if status is None:
            status = torch.zeros(batch.n, dtype=torch.uint8, device=buf.device)
        if segs is None:
            segs = torch.zeros((batch.n, 16), dtype=torch.uint8, device=buf.device)
        if flows is None:
            flows = torch.empty((ng, 16), dtype=torch.uint8, device=buf.device)
        assert segs.is_cuda and segs.is_contiguous() and segs.numel() * segs.dtype.itemsize >= 16 * batch.n
        assert flows.is_cuda and flows.is_contiguous() and flows.numel() * flows.dtype.itemsize >= 16 * ng
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify_tcp_assemble(self._h, buf.data_ptr(), ctypes.byref(b), groups.data_ptr(), ng,
                                                        ctypes.byref(c), dst.data_ptr(), wins.data_ptr(),
                                                        status.data_ptr(), segs.data_ptr(), flows.data_ptr(),
                                                        self._stream(stream)),
              "smol_csum_batch_verify_tcp_assemble")
        return status, segs, flows

    def nhc_udp_emit(self, buf, batch: Batch, addrs, caps=None, status=None, stream=None):
        """6LoWPAN NHC UDP emit (smol_csum_batch_nhc_udp_emit): ``addrs`` is a device uint8 tensor of
        n x 32 bytes (IPv6 source, destination per record)."""
        self._check_buf(buf, batch)
        assert addrs.is_cuda and addrs.numel() >= 32 * batch.n
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_nhc_udp_emit(self._h, buf.data_ptr(), ctypes.byref(b), addrs.data_ptr(),
                                                 ctypes.byref(c), status.data_ptr() if status is not None else None,
                                                 self._stream(stream)), "smol_csum_batch_nhc_udp_emit")
        return status

    def nhc_udp_verify(self, buf, batch: Batch, addrs, caps=None, status=None, stream=None):
        """6LoWPAN NHC UDP parse gate (smol_csum_batch_nhc_udp_verify); returns the status tensor."""
        import torch

        self._check_buf(buf, batch)
        assert addrs.is_cuda and addrs.numel() >= 32 * batch.n
        if status is None:
            status = torch.empty(batch.n, dtype=torch.uint8, device=buf.device)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_nhc_udp_verify(self._h, buf.data_ptr(), ctypes.byref(b), addrs.data_ptr(),
                                                   ctypes.byref(c), status.data_ptr(), self._stream(stream)),
              "smol_csum_batch_nhc_udp_verify")
        return status

    def verify(self, buf, batch: Batch, caps=None, status=None, stream=None):
        """status[i] = SMOL_ST_* bits (Repr::parse gates under ``caps``)."""
        import torch

        self._check_buf(buf, batch)
        if status is None:
            status = torch.empty(batch.n, dtype=torch.uint8, device=buf.device)
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                           status.data_ptr(), self._stream(stream)),
              "smol_csum_batch_verify")
        return status

    def verify_copy(self, buf, batch: Batch, dst, slots, caps=None, status=None, spans=None, stream=None):
        """Verify, and in the same pass deliver every record's UDP / TCP payload to its slot of `dst`
        (smol_csum_batch_verify_copy).  `slots`: a device uint8 tensor of n smol_csum_slot_t (see
        make_slots); `dst`: the destination uint8 device tensor, written only inside the copied ranges.
        Returns (status, spans): verify's status bytes and an n x 8 uint8 device tensor of
        smol_csum_span_t (view its host copy as SPAN_DTYPE).  The copy does not wait for the verdict:
        commit a slot only when its status byte has ST_ACCEPT."""
        import torch

        self._check_buf(buf, batch)
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert slots.is_cuda and slots.is_contiguous() and slots.numel() * slots.dtype.itemsize >= 16 * batch.n
        if status is None:
            status = torch.empty(batch.n, dtype=torch.uint8, device=buf.device)
        if spans is None:
            spans = torch.empty((batch.n, 8), dtype=torch.uint8, device=buf.device)
        assert spans.is_cuda and spans.is_contiguous() and spans.numel() * spans.dtype.itemsize >= 8 * batch.n
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify_copy(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                dst.data_ptr(), slots.data_ptr(), status.data_ptr(),
                                                spans.data_ptr(), self._stream(stream)),
              "smol_csum_batch_verify_copy")
        return status, spans

    def verify_echo_reply(self, buf, batch: Batch, dst, slots, caps=None, cfg=None, status=None, echo=None, stream=None):
        """Verify, and in the same pass write the reply to every ICMPv4 / ICMPv6 echo request the wire-level
        address rule answers to the record's slot of `dst`: fresh Ethernet / IP / ICMP head, the request's
        data, both checksums filled (smol_csum_batch_verify_echo_reply).  `slots`: a device uint8 tensor of n
        smol_csum_slot_t (see make_slots); `dst`: the destination uint8 device tensor, written only inside
        the written frames; `cfg`: None, or the interface's directed-broadcast address as 4 bytes.  Returns
        (status, echo): verify's status bytes and an n x 8 uint8 device tensor of smol_csum_echo_t (view its
        host copy as ECHO_DTYPE).  The copy does not wait for the verdict: transmit a slot only when its
        entry has ECHO_SEND; ECHO_HOST marks the requests the host has to answer itself."""
        import torch

        self._check_buf(buf, batch)
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert slots.is_cuda and slots.is_contiguous() and slots.numel() * slots.dtype.itemsize >= 16 * batch.n
        if status is None:
            status = torch.empty(batch.n, dtype=torch.uint8, device=buf.device)
        if echo is None:
            echo = torch.empty((batch.n, 8), dtype=torch.uint8, device=buf.device)
        assert echo.is_cuda and echo.is_contiguous() and echo.numel() * echo.dtype.itemsize >= 8 * batch.n
        b = batch.c()
        c = _caps(caps)
        cfg_c = None
        if cfg is not None:
            cfg_c = cfg if isinstance(cfg, EchoCfgC) else EchoCfgC((ctypes.c_uint8 * 4)(*bytes(cfg)), (ctypes.c_uint8 * 4)())
        check(self._L.smol_csum_batch_verify_echo_reply(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                      ctypes.byref(cfg_c) if cfg_c is not None else None,
                                                      dst.data_ptr(), slots.data_ptr(), status.data_ptr(),
                                                      echo.data_ptr(), self._stream(stream)),
              "smol_csum_batch_verify_echo_reply")
        return status, echo

    def verify_unreach_reply(self, buf, batch: Batch, dst, slots, udp_open=None, caps=None, cfg=None, status=None, unr=None,
                             stream=None):
        """Verify, and in the same pass write the ICMP error for every datagram nobody takes (a UDP datagram
        to a closed port, an IPv4 protocol or IPv6 next header the stack does not handle) that the wire-level
        address rule answers to the record's slot of `dst`: fresh Ethernet / IP / ICMP head, the offending IP
        header emitted again, the first 528 / 1192 bytes of its payload, every checksum filled
        (smol_csum_batch_verify_unreach_reply).  `udp_open`: None (no UDP datagram is refused), or the 8192-byte
        device bitmap of make_port_map; a host with a socket that matches on something other than the
        destination port (the DNS socket) passes None or sets every bit.  `slots`, `dst`, `cfg`: as
        verify_echo_reply.  Returns (status, unr): verify's status bytes and an n x 8 uint8 device tensor of
        smol_csum_unreach_t (view its host copy as UNR_DTYPE).  The copy does not wait for the verdict:
        transmit a slot only when its entry has UNR_SEND; UNR_HOST marks the replies the host has to build."""
        import torch

        self._check_buf(buf, batch)
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert slots.is_cuda and slots.is_contiguous() and slots.numel() * slots.dtype.itemsize >= 16 * batch.n
        if udp_open is not None:
            assert udp_open.is_cuda and udp_open.is_contiguous() and udp_open.dtype.itemsize == 1 and udp_open.numel() >= 8192
        if status is None:
            status = torch.empty(batch.n, dtype=torch.uint8, device=buf.device)
        if unr is None:
            unr = torch.empty((batch.n, 8), dtype=torch.uint8, device=buf.device)
        assert unr.is_cuda and unr.is_contiguous() and unr.numel() * unr.dtype.itemsize >= 8 * batch.n
        b = batch.c()
        c = _caps(caps)
        cfg_c = None
        if cfg is not None:
            cfg_c = cfg if isinstance(cfg, EchoCfgC) else EchoCfgC((ctypes.c_uint8 * 4)(*bytes(cfg)), (ctypes.c_uint8 * 4)())
        check(self._L.smol_csum_batch_verify_unreach_reply(self._h, buf.data_ptr(), ctypes.byref(b), ctypes.byref(c),
                                                         ctypes.byref(cfg_c) if cfg_c is not None else None,
                                                         udp_open.data_ptr() if udp_open is not None else None,
                                                         dst.data_ptr(), slots.data_ptr(), status.data_ptr(),
                                                         unr.data_ptr(), self._stream(stream)),
              "smol_csum_batch_verify_unreach_reply")
        return status, unr

    def verify_udp_enqueue(self, buf, batch: Batch, groups, dst, socks, meta, caps=None, status=None, rx=None, out=None,
                           stream=None):
        """verify, and in the same pass every UDP datagram's payload put where its socket's
        PacketBuffer::enqueue places it in `dst`, the metadata entries written to `meta`
        (smol_csum_batch_verify_udp_enqueue).  `groups`: a device uint8 tensor of smol_csum_frag_group_t (see
        make_groups), one per socket: the frames routed to it in this poll, consecutive records in arrival
        order; `socks`: a device uint8 tensor of one smol_csum_udpsock_t per GROUP (see make_udpsocks); `dst`:
        the uint8 device tensor that holds the payload rings; `meta`: the 16-byte aligned uint8 device tensor
        that holds the metadata rings (48 bytes per entry, UDPMETA_DTYPE).  Returns (status, rx, out): verify's
        status byte per record (a fresh tensor starts zeroed; records outside the groups keep their value), an
        n x 16 uint8 device tensor of smol_csum_udprx_t (UDPRX_DTYPE; a fresh one starts zeroed) and an
        n_groups x 32 one of smol_csum_udpsockout_t (UDPSOCKOUT_DTYPE).  The copy does not wait for the
        verdict: commit by copying the four state words of `out` into the socket's PacketBuffer."""
        import torch

        self._check_buf(buf, batch)
        assert groups.is_cuda and groups.numel() % 16 == 0
        ng = groups.numel() // 16
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert socks.is_cuda and socks.is_contiguous() and socks.numel() * socks.dtype.itemsize >= 48 * ng
        assert meta.is_cuda and meta.is_contiguous()
        if status is None:
            status = torch.zeros(batch.n, dtype=torch.uint8, device=buf.device)
        if rx is None:
            rx = torch.zeros((batch.n, 16), dtype=torch.uint8, device=buf.device)
        if out is None:
            out = torch.empty((ng, 32), dtype=torch.uint8, device=buf.device)
        assert rx.is_cuda and rx.is_contiguous() and rx.numel() * rx.dtype.itemsize >= 16 * batch.n
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.dtype.itemsize >= 32 * ng
        b = batch.c()
        c = _caps(caps)
        check(self._L.smol_csum_batch_verify_udp_enqueue(self._h, buf.data_ptr(), ctypes.byref(b), groups.data_ptr(), ng,
                                                       ctypes.byref(c), dst.data_ptr(), socks.data_ptr(), meta.data_ptr(),
                                                       status.data_ptr(), rx.data_ptr(), out.data_ptr(),
                                                       self._stream(stream)),
              "smol_csum_batch_verify_udp_enqueue")
        return status, rx, out

    def udp_dequeue_emit(self, src, socks, meta, dst, frame_stride: int = 0, caps=None, tx=None, out=None, n_tx=None,
                         stream=None):
        """Every socket's transmit PacketBuffer dequeued and its datagrams written to `dst` as whole frames,
        headers built on the device, checksums filled in the pass that copies the payload
        (smol_csum_batch_udp_dequeue_emit).  `src`: the uint8 device tensor that holds the payload rings; `socks`:
        a device uint8 tensor of one smol_csum_udptxsock_t per socket (see make_udptxsocks); `meta`: the 16-byte
        aligned uint8 device tensor that holds the metadata rings (48 bytes per entry, UDPMETA_DTYPE, read with
        their send-side meaning); `frame_stride`: bytes from one frame of a socket to the next, 0 for frames
        back to back.  Returns (tx, out): an n_tx x 16 uint8 device tensor of smol_csum_udptx_t (UDPTX_DTYPE; a
        fresh one starts zeroed and has `n_tx` entries, which must cover every socket's tx_first + max_dgrams)
        and an n_groups x 32 one of smol_csum_udptxout_t (UDPTXOUT_DTYPE).  Commit by copying the four state
        words of `out` into the socket's PacketBuffer."""
        import torch

        assert socks.is_cuda and socks.is_contiguous() and (socks.numel() * socks.dtype.itemsize) % 96 == 0
        ng = socks.numel() * socks.dtype.itemsize // 96
        assert src.is_cuda and src.dtype.itemsize == 1 and src.is_contiguous()
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        assert meta.is_cuda and meta.is_contiguous()
        if tx is None:
            assert n_tx is not None, "udp_dequeue_emit: pass tx, or n_tx for a fresh one"
            tx = torch.zeros((int(n_tx), 16), dtype=torch.uint8, device=src.device)
        if out is None:
            out = torch.empty((ng, 32), dtype=torch.uint8, device=src.device)
        assert tx.is_cuda and tx.is_contiguous()
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.dtype.itemsize >= 32 * ng
        c = _caps(caps)
        check(self._L.smol_csum_batch_udp_dequeue_emit(self._h, src.data_ptr(), socks.data_ptr(), ng, meta.data_ptr(),
                                                     ctypes.byref(c), dst.data_ptr(), int(frame_stride), tx.data_ptr(),
                                                     out.data_ptr(), self._stream(stream)),
              "smol_csum_batch_udp_dequeue_emit")
        return tx, out

    # ---- tooling ----
    def synth(self, buf, batch: Batch, profile: int, seed: int, stream=None):
        self._check_buf(buf, batch)
        b = batch.c()
        check(self._L.smol_csum_tool_synth(self._h, buf.data_ptr(), ctypes.byref(b), int(profile),
                                         int(seed) & (2**64 - 1), self._stream(stream)),
              "smol_csum_tool_synth")

    def corrupt(self, buf, batch: Batch, every: int, seed: int, stream=None):
        self._check_buf(buf, batch)
        b = batch.c()
        check(self._L.smol_csum_tool_corrupt(self._h, buf.data_ptr(), ctypes.byref(b), int(every),
                                           int(seed) & (2**64 - 1), self._stream(stream)),
              "smol_csum_tool_corrupt")

    def stream_read(self, buf, sink, stream=None):
        """Read-only HBM streaming probe over the whole buffer (tooling)."""
        nbytes = buf.numel() // 16 * 16
        check(self._L.smol_csum_tool_stream_read(self._h, buf.data_ptr(), nbytes, sink.data_ptr(),
                                               self._stream(stream)), "smol_csum_tool_stream_read")

    def field_probe(self, buf, stride: int, f1: int, f2: int = 0xFFFFFFFF, stream=None):
        """Emit's floor probe (tooling, smol_csum_tool_field_probe): stream-read the buffer and store
        2 bytes at offsets f1 / f2 of every `stride`-byte record.  Overwrites those bytes."""
        nbytes = buf.numel() // 16 * 16
        check(self._L.smol_csum_tool_field_probe(self._h, buf.data_ptr(), nbytes, int(stride), int(f1), int(f2),
                                               self._stream(stream)), "smol_csum_tool_field_probe")

    def field_probe_list(self, buf, addrs, piece_first, seg64: bool = False, stream=None):
        """Emit's floor probe with listed store addresses (tooling, smol_csum_tool_field_probe_list):
        `addrs` a device u64 tensor of ascending byte offsets, `piece_first` a device u32 tensor with
        the index of the first address at or after each 8-KiB piece (ceil(bytes / 8192) + 1
        entries).  Overwrites the bytes at those offsets; with `seg64` rewrites the 64-B segments
        holding them whole, with their own values, instead."""
        nbytes = buf.numel() // 16 * 16
        check(self._L.smol_csum_tool_field_probe_list(self._h, buf.data_ptr(), nbytes, addrs.data_ptr(),
                                                    piece_first.data_ptr(), int(bool(seg64)),
                                                    self._stream(stream)),
              "smol_csum_tool_field_probe_list")

    def segment_probe(self, buf, bitmap, nt: bool = False, stream=None):
        """Emit's floor in its store shape (tooling, smol_csum_tool_segment_probe): the read stream over
        `buf` plus every 64-B segment whose bit is set in `bitmap` (device int32 tensor, one bit per
        segment, see segment_bitmap) rewritten whole with its own bytes; `nt`: non-temporal stores."""
        nbytes = buf.numel() // 16 * 16
        check(self._L.smol_csum_tool_segment_probe(self._h, buf.data_ptr(), nbytes, bitmap.data_ptr(), int(bool(nt)),
                                                 self._stream(stream)),
              "smol_csum_tool_segment_probe")

    def field_scatter(self, buf, addrs, vals, nt: int = 0, stream=None):
        """A separate store pass (tooling, smol_csum_tool_field_scatter): the big-endian u16 `vals[i]`
        at byte offset `addrs[i]` (device int64 / uint16-as-int16 tensors) of `buf`.  `nt`: the flags
        (bit 0 non-temporal stores; bits 1 / 2 / 3 the whole 64-B segment / 32-B sector / 128-B line
        instead)."""
        check(self._L.smol_csum_tool_field_scatter(self._h, buf.data_ptr(), buf.numel(), addrs.data_ptr(),
                                                 vals.data_ptr(), int(addrs.numel()), int(nt),
                                                 self._stream(stream)), "smol_csum_tool_field_scatter")

    def set_shape(self, shape: int):
        check(self._L.smol_csum_tool_set_shape(self._h, int(shape)), "smol_csum_tool_set_shape")

    def set_variant(self, variant: int):
        check(self._L.smol_csum_tool_set_variant(self._h, int(variant)), "smol_csum_tool_set_variant")

    def set_fields_kernel(self, kernel: int):
        """emit_fields' kernel form: 0 the library's choice, 1 the walk kernel, 2 the transposed walk,
        3 the descriptor walk (a form that does not serve the batch gives way to the walk kernel)."""
        check(self._L.smol_csum_tool_set_fields_kernel(self._h, int(kernel)), "smol_csum_tool_set_fields_kernel")

    def set_emit_route(self, route: int):
        """Fixed-stride whole-segment emit as two launches (the fields-sink kernel into the context's entries,
        then the segment pass): -1 where the library's measured range says so, 0 never, 1 wherever it is legal."""
        check(self._L.smol_csum_tool_set_emit_route(self._h, int(route)), "smol_csum_tool_set_emit_route")

    def last_route(self) -> bool:
        """Whether this engine's last emit ran as the two-launch route."""
        return bool(self._L.smol_csum_tool_last_route(self._h))

    def set_route_chunk(self, records: int):
        """Records per launch pair of the route (0: the default, what the entry buffer holds)."""
        check(self._L.smol_csum_tool_set_route_chunk(self._h, int(records)), "smol_csum_tool_set_route_chunk")

    def set_vcopy_stores(self, nt: bool):
        """verify_copy's body stores: False the library's choice (the default cache policy), True non-temporal."""
        check(self._L.smol_csum_tool_set_vcopy_stores(self._h, int(bool(nt))), "smol_csum_tool_set_vcopy_stores")

    def set_tile(self, records: int):
        check(self._L.smol_csum_tool_set_tile(self._h, int(records)), "smol_csum_tool_set_tile")

    def kernel_name(self, op: str, has_desc: bool = False) -> str:
        """Deprecated: the kernel an IP-path `op` launches for a batch of short records (no record
        length is passed; see kernel_for)."""
        code = {"data": 0, "emit": 1, "verify": 2, "copy_emit": 3}[op]
        return self._L.smol_csum_tool_kernel_name(self._h, code, int(bool(has_desc))).decode()

    def kernel_for(self, op: str, batch: Batch) -> str:
        """The kernel (rocprofv3 name prefix) an IP-path `op` ("data", "emit", "verify", "copy_emit")
        launches for `batch` with this engine's settings: the library's own dispatch decision."""
        code = {"data": 0, "emit": 1, "verify": 2, "copy_emit": 3}[op]
        b = batch.c()
        return self._L.smol_csum_tool_kernel_for(self._h, code, ctypes.byref(b)).decode()

    def variant_built(self, variant: int) -> bool:
        """Whether this build of the library runs `variant` (the product library: the defaults and
        one fallback per operation; the experiments build: every measured variant)."""
        return bool(self._L.smol_csum_tool_variant_built(int(variant)))

    def last_launch(self) -> dict:
        """The kernel instantiation of the process's last checksum launch: {"kernel": "csum_kernel" |
        "csum_tile_kernel" | "copy_kernel" | "csum_kernel_nhc" | "xwalk_kernel" | "dwalk_kernel" | emit_fields'
        "csum_fields_kernel" | "xwalk_kernel(fields)" | "dwalk_kernel(fields)" | verify_copy's "vcopy_kernel" | verify_reassemble's "fragcopy_kernel" | fragment_emit's "fragcut_kernel" | tcp_segment_emit's "tcpcut_kernel" | verify_tcp_assemble's "tcpasm_kernel" | verify_echo_reply's "echo" | verify_unreach_reply's "unreach" | verify_udp_enqueue's "udprx_kernel" | udp_dequeue_emit's "udptx_kernel", "variant": VAR, "G":
        lanes per record, "U": chunks per lane per step (xwalk_kernel: 1-KiB loads per record)} (None
        before the first launch)."""
        w = int(self._L.smol_csum_tool_last_launch())
        names = {1: "csum_kernel", 2: "csum_tile_kernel", 3: "copy_kernel", 4: "csum_kernel_nhc", 5: "xwalk_kernel",
                 6: "dwalk_kernel", 7: "csum_fields_kernel", 8: "xwalk_kernel(fields)", 9: "dwalk_kernel(fields)", 10: "vcopy_kernel",
                 11: "fragcopy_kernel", 12: "fragcut_kernel", 13: "tcpcut_kernel", 14: "tcpasm_kernel", 15: "echo", 16: "unreach",
                 17: "udprx_kernel", 18: "udptx_kernel"}
        if not w >> 24:
            return None
        return {"kernel": names.get(w >> 24, "?"), "variant": (w >> 16) & 0xff, "G": (w >> 8) & 0xff, "U": w & 0xff}

    def set_xcd_remap(self, on: int):
        """1 / 0: force the XCD-contiguous block order on / off; K >= 2: runs of K workgroups per XCD
        turn; -1: the library's choice."""
        check(self._L.smol_csum_tool_set_xcd_remap(self._h, int(on)), "smol_csum_tool_set_xcd_remap")

    def set_launch_records(self, records: int):
        check(self._L.smol_csum_tool_set_launch_records(self._h, int(records)), "smol_csum_tool_set_launch_records")

    def set_max_blocks(self, max_blocks: int):
        check(self._L.smol_csum_tool_set_max_blocks(self._h, int(max_blocks)),
              "smol_csum_tool_set_max_blocks")


def auto_shape(length: int, has_desc: bool = False) -> int:
    return int(_lib.lib().smol_csum_tool_auto_shape(int(length), int(bool(has_desc))))
