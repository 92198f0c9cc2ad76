"""ctypes binding of libsmolcsum.so (the C ABI declared in include/smolcsum.h).

The shared library is built in-tree (``smoltcp_amd/libsmolcsum.so``, see ``__graft_entry__.build``)
and travels with the repository snapshot to the GPU box.  There is no fallback: if the library is
missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMOLCSUM_LIB: an alternative build of the same library (A/B experiments only)
LIB_PATH = os.environ.get("SMOLCSUM_LIB") or os.path.join(_HERE, "libsmolcsum.so")
# The experiments build (`make -C smoltcp_amd/csrc EXP=1`): the product library plus the measured
# kernel variants that are not defaults (tools/ and the variant tests load it when it exists).
EXP_LIB_PATH = os.path.join(_HERE, "libsmolcsum_exp.so")

SMOL_OK, SMOL_EINVAL, SMOL_ENODEV, SMOL_EHIP, SMOL_ERANGE, SMOL_ENOMEM = 0, -1, -2, -3, -4, -5
ERROR_NAMES = {
    SMOL_EINVAL: "SMOL_EINVAL",
    SMOL_ENODEV: "SMOL_ENODEV",
    SMOL_EHIP: "SMOL_EHIP",
    SMOL_ERANGE: "SMOL_ERANGE",
    SMOL_ENOMEM: "SMOL_ENOMEM",
}

# Every symbol include/smolcsum.h and include/smolcsum_tools.h declare.
ABI_SYMBOLS = [
    "smol_csum_data", "smol_csum_combine", "smol_csum_pseudo_header_v4",
    "smol_csum_pseudo_header_v6", "smol_csum_pseudo_header", "smol_csum_ctx_create",
    "smol_csum_ctx_destroy", "smol_csum_batch_data", "smol_csum_batch_emit",
    "smol_csum_batch_verify", "smol_csum_batch_copy_emit", "smol_csum_batch_emit_fields",
    "smol_csum_batch_verify_copy",
    "smol_csum_apply_fields", "smol_csum_batch_emit_frag",
    "smol_csum_batch_verify_frag", "smol_csum_batch_verify_reassemble", "smol_csum_batch_fragment_emit",
    "smol_csum_batch_tcp_segment_emit", "smol_csum_batch_verify_tcp_assemble", "smol_csum_batch_verify_echo_reply",
    "smol_csum_batch_verify_unreach_reply", "smol_csum_batch_verify_udp_enqueue", "smol_csum_batch_udp_dequeue_emit",
    "smol_csum_batch_nhc_udp_emit",
    "smol_csum_batch_nhc_udp_verify", "smol_csum_last_error", "smol_csum_abi_version",
]
TOOL_SYMBOLS = [
    "smol_csum_tool_synth", "smol_csum_tool_corrupt", "smol_csum_tool_set_shape",
    "smol_csum_tool_set_variant", "smol_csum_tool_set_tile",
    "smol_csum_tool_set_max_blocks", "smol_csum_tool_auto_shape", "smol_csum_tool_stream_read",
    "smol_csum_tool_set_xcd_remap", "smol_csum_tool_set_launch_records",
    "smol_csum_tool_field_probe",
    "smol_csum_tool_field_probe_list", "smol_csum_tool_segment_probe", "smol_csum_tool_field_scatter",
    "smol_csum_tool_variant_built",
    "smol_csum_tool_kernel_name", "smol_csum_tool_kernel_for", "smol_csum_tool_last_launch",
    "smol_csum_tool_pick", "smol_csum_tool_variant_info", "smol_csum_tool_form",
    "smol_csum_tool_set_fields_kernel", "smol_csum_tool_walk_launch", "smol_csum_tool_set_vcopy_stores",
    "smol_csum_tool_set_emit_route", "smol_csum_tool_last_route", "smol_csum_tool_set_route_chunk",
]
# Tool symbols added in later rounds: bound only when the loaded build has them (SMOLCSUM_LIB may name
# an older build for an A/B run), and a call to a missing one raises AttributeError naming it.
OPTIONAL_TOOL_SYMBOLS = ("smol_csum_tool_variant_built", "smol_csum_tool_kernel_for", "smol_csum_tool_segment_probe",
                         "smol_csum_tool_pick", "smol_csum_tool_variant_info", "smol_csum_tool_form",
                         "smol_csum_tool_set_fields_kernel", "smol_csum_tool_walk_launch",
                         "smol_csum_tool_set_vcopy_stores", "smol_csum_tool_set_emit_route",
                         "smol_csum_tool_last_route", "smol_csum_tool_set_route_chunk")


class SmolError(RuntimeError):
    def __init__(self, rc: int, what: str, detail: str = ""):
        name = ERROR_NAMES.get(rc, str(rc))
        super().__init__(f"{what} failed: {name}" + (f" ({detail})" if detail else ""))
        self.rc = rc


class Caps(ctypes.Structure):
    """smol_checksum_caps_t — phy::ChecksumCapabilities {ipv4, udp, tcp, icmpv4, icmpv6}."""

    _fields_ = [
        ("ipv4", ctypes.c_uint8),
        ("udp", ctypes.c_uint8),
        ("tcp", ctypes.c_uint8),
        ("icmpv4", ctypes.c_uint8),
        ("icmpv6", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
    ]


class BatchC(ctypes.Structure):
    """smol_csum_batch_t."""

    _fields_ = [
        ("desc", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
        ("stride", ctypes.c_uint64),
        ("len", ctypes.c_uint32),
        ("kind", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 2),
    ]


class FieldsC(ctypes.Structure):
    """smol_csum_fields_t: one record's emit result (smol_csum_batch_emit_fields)."""

    _fields_ = [
        ("off", ctypes.c_uint16 * 3),
        ("val", ctypes.c_uint16 * 3),
        ("status", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
    ]


NO_FIELD = 0xFFFF  # SMOL_NO_FIELD


class SlotC(ctypes.Structure):
    """smol_csum_slot_t: where one record's payload goes (smol_csum_batch_verify_copy)."""

    _fields_ = [
        ("dst_offset", ctypes.c_uint64),
        ("cap", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class SpanC(ctypes.Structure):
    """smol_csum_span_t: one record's payload span (smol_csum_batch_verify_copy)."""

    _fields_ = [
        ("len", ctypes.c_uint32),
        ("off", ctypes.c_uint16),
        ("copied", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
    ]


class DgramC(ctypes.Structure):
    """smol_csum_dgram_t: one reassembled datagram (smol_csum_batch_verify_reassemble)."""

    _fields_ = [
        ("len", ctypes.c_uint32),
        ("l4_len", ctypes.c_uint32),
        ("l4_off", ctypes.c_uint16),
        ("protocol", ctypes.c_uint8),
        ("copied", ctypes.c_uint8),
        ("reserved", ctypes.c_uint32),
    ]


class FragPlanC(ctypes.Structure):
    """smol_csum_fragplan_t: where and how one datagram is cut (smol_csum_batch_fragment_emit)."""

    _fields_ = [
        ("dst_offset", ctypes.c_uint64),
        ("cap", ctypes.c_uint32),
        ("ip_mtu", ctypes.c_uint16),
        ("ident", ctypes.c_uint16),
    ]


class FragOutC(ctypes.Structure):
    """smol_csum_fragout_t: what became of one datagram (smol_csum_batch_fragment_emit)."""

    _fields_ = [
        ("count", ctypes.c_uint32),
        ("frame_len", ctypes.c_uint32),
        ("last_len", ctypes.c_uint32),
        ("status", ctypes.c_uint8),
        ("written", ctypes.c_uint8),
        ("reserved", ctypes.c_uint16),
    ]


class TcpPlanC(ctypes.Structure):
    """smol_csum_tcpplan_t: one send's payload range, MSS and place (smol_csum_batch_tcp_segment_emit)."""

    _fields_ = [
        ("src_offset", ctypes.c_uint64),
        ("len", ctypes.c_uint32),
        ("mss", ctypes.c_uint16),
        ("reserved", ctypes.c_uint16),
        ("dst_offset", ctypes.c_uint64),
        ("cap", ctypes.c_uint32),
        ("reserved2", ctypes.c_uint32),
    ]


class TcpOutC(ctypes.Structure):
    """smol_csum_tcpout_t: what became of one send (smol_csum_batch_tcp_segment_emit)."""

    _fields_ = [
        ("count", ctypes.c_uint32),
        ("frame_len", ctypes.c_uint32),
        ("last_len", ctypes.c_uint32),
        ("status", ctypes.c_uint8),
        ("written", ctypes.c_uint8),
        ("reserved", ctypes.c_uint16),
    ]


class TcpWinC(ctypes.Structure):
    """smol_csum_tcpwin_t: one connection's receive window and ring (smol_csum_batch_verify_tcp_assemble)."""

    _fields_ = [
        ("dst_offset", ctypes.c_uint64),
        ("ring_len", ctypes.c_uint32),
        ("ring_pos", ctypes.c_uint32),
        ("window_start", ctypes.c_uint32),
        ("window_len", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 2),
    ]


class TcpSegC(ctypes.Structure):
    """smol_csum_tcpseg_t: one record's outcome (smol_csum_batch_verify_tcp_assemble)."""

    _fields_ = [
        ("seq", ctypes.c_uint32),
        ("win_off", ctypes.c_uint32),
        ("len", ctypes.c_uint32),
        ("off", ctypes.c_uint16),
        ("flags", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
    ]


class TcpFlowC(ctypes.Structure):
    """smol_csum_tcpflow_t: one connection's outcome (smol_csum_batch_verify_tcp_assemble)."""

    _fields_ = [
        ("contig_len", ctypes.c_uint32),
        ("counted", ctypes.c_uint32),
        ("redelivered", ctypes.c_uint32),
        ("valid", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
    ]


class EchoCfgC(ctypes.Structure):
    """smol_csum_echo_cfg_t: what the responder knows of the interface (smol_csum_batch_verify_echo_reply)."""

    _fields_ = [
        ("bcast_v4", ctypes.c_uint8 * 4),
        ("reserved", ctypes.c_uint8 * 4),
    ]


class EchoC(ctypes.Structure):
    """smol_csum_echo_t: one record's outcome (smol_csum_batch_verify_echo_reply)."""

    _fields_ = [
        ("frame_len", ctypes.c_uint32),
        ("data_off", ctypes.c_uint16),
        ("head_len", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
    ]


class UnreachC(ctypes.Structure):
    """smol_csum_unreach_t: one record's outcome (smol_csum_batch_verify_unreach_reply)."""

    _fields_ = [
        ("frame_len", ctypes.c_uint32),
        ("data_off", ctypes.c_uint16),
        ("head_len", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
    ]


class UdpSockC(ctypes.Structure):
    """smol_csum_udpsock_t: one UDP socket's receive buffer before the poll (smol_csum_batch_verify_udp_enqueue)."""

    _fields_ = [
        ("dst_offset", ctypes.c_uint64),
        ("meta_first", ctypes.c_uint64),
        ("payload_cap", ctypes.c_uint32),
        ("payload_read", ctypes.c_uint32),
        ("payload_len", ctypes.c_uint32),
        ("meta_cap", ctypes.c_uint32),
        ("meta_read", ctypes.c_uint32),
        ("meta_len", ctypes.c_uint32),
        ("port", ctypes.c_uint16),
        ("reserved", ctypes.c_uint16 * 3),
    ]


class UdpMetaC(ctypes.Structure):
    """smol_csum_udpmeta_t: one metadata-ring entry (smol_csum_batch_verify_udp_enqueue)."""

    _fields_ = [
        ("size", ctypes.c_uint32),
        ("record", ctypes.c_uint32),
        ("src_port", ctypes.c_uint16),
        ("family", ctypes.c_uint8),
        ("kind", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 4),
        ("remote_addr", ctypes.c_uint8 * 16),
        ("local_addr", ctypes.c_uint8 * 16),
    ]


class UdpRxC(ctypes.Structure):
    """smol_csum_udprx_t: one record's outcome (smol_csum_batch_verify_udp_enqueue)."""

    _fields_ = [
        ("ring_off", ctypes.c_uint32),
        ("len", ctypes.c_uint32),
        ("meta_idx", ctypes.c_uint32),
        ("off", ctypes.c_uint16),
        ("flags", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
    ]


class UdpSockOutC(ctypes.Structure):
    """smol_csum_udpsockout_t: one socket's outcome (smol_csum_batch_verify_udp_enqueue)."""

    _fields_ = [
        ("payload_read", ctypes.c_uint32),
        ("payload_len", ctypes.c_uint32),
        ("meta_read", ctypes.c_uint32),
        ("meta_len", ctypes.c_uint32),
        ("enqueued", ctypes.c_uint32),
        ("full", ctypes.c_uint32),
        ("restored", ctypes.c_uint32),
        ("valid", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 3),
    ]


class UdpTxSockC(ctypes.Structure):
    """smol_csum_udptxsock_t: one UDP socket's transmit buffer before the call and where its frames go
    (smol_csum_batch_udp_dequeue_emit)."""

    _fields_ = [
        ("src_offset", ctypes.c_uint64),
        ("meta_first", ctypes.c_uint64),
        ("dst_offset", ctypes.c_uint64),
        ("tx_first", ctypes.c_uint64),
        ("payload_cap", ctypes.c_uint32),
        ("payload_read", ctypes.c_uint32),
        ("payload_len", ctypes.c_uint32),
        ("meta_cap", ctypes.c_uint32),
        ("meta_read", ctypes.c_uint32),
        ("meta_len", ctypes.c_uint32),
        ("dst_cap", ctypes.c_uint32),
        ("max_dgrams", ctypes.c_uint32),
        ("port", ctypes.c_uint16),
        ("ip_mtu", ctypes.c_uint16),
        ("hop_limit", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("eth_dst", ctypes.c_uint8 * 6),
        ("eth_src", ctypes.c_uint8 * 6),
        ("reserved", ctypes.c_uint8 * 14),
    ]


class UdpTxC(ctypes.Structure):
    """smol_csum_udptx_t: one dequeued datagram (smol_csum_batch_udp_dequeue_emit)."""

    _fields_ = [
        ("frame_off", ctypes.c_uint32),
        ("ring_off", ctypes.c_uint32),
        ("meta_idx", ctypes.c_uint32),
        ("ip_len", ctypes.c_uint16),
        ("flags", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8),
    ]


class UdpTxOutC(ctypes.Structure):
    """smol_csum_udptxout_t: one socket's outcome (smol_csum_batch_udp_dequeue_emit)."""

    _fields_ = [
        ("payload_read", ctypes.c_uint32),
        ("payload_len", ctypes.c_uint32),
        ("meta_read", ctypes.c_uint32),
        ("meta_len", ctypes.c_uint32),
        ("sent", ctypes.c_uint32),
        ("oversize", ctypes.c_uint32),
        ("bytes", ctypes.c_uint32),
        ("stop", ctypes.c_uint8),
        ("valid", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 2),
    ]


_LIBS = {}


def lib(path: str | None = None) -> ctypes.CDLL:
    """Load libsmolcsum.so, or the build at `path` (raises if it is absent: there is no CPU
    fallback)."""
    path = path or LIB_PATH
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    L = ctypes.CDLL(path)
    vp, u8, u16, u32, u64 = ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64
    sz, i32 = ctypes.c_size_t, ctypes.c_int
    L.smol_csum_data.argtypes = [vp, sz]
    L.smol_csum_data.restype = u16
    L.smol_csum_combine.argtypes = [vp, sz]
    L.smol_csum_combine.restype = u16
    L.smol_csum_pseudo_header_v4.argtypes = [vp, vp, u8, u32]
    L.smol_csum_pseudo_header_v4.restype = u16
    L.smol_csum_pseudo_header_v6.argtypes = [vp, vp, u8, u32]
    L.smol_csum_pseudo_header_v6.restype = u16
    L.smol_csum_pseudo_header.argtypes = [i32, vp, i32, vp, u8, u32, ctypes.POINTER(u16)]
    L.smol_csum_pseudo_header.restype = i32
    L.smol_csum_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.smol_csum_ctx_create.restype = i32
    L.smol_csum_ctx_destroy.argtypes = [vp]
    L.smol_csum_ctx_destroy.restype = i32
    L.smol_csum_batch_data.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, vp]
    L.smol_csum_batch_data.restype = i32
    L.smol_csum_batch_emit.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp]
    L.smol_csum_batch_emit.restype = i32
    L.smol_csum_batch_verify.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp]
    L.smol_csum_batch_verify.restype = i32
    L.smol_csum_batch_copy_emit.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, vp, ctypes.POINTER(Caps), vp, vp]
    L.smol_csum_batch_copy_emit.restype = i32
    for name in ("smol_csum_batch_emit_frag", "smol_csum_batch_verify_frag"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, u64, ctypes.POINTER(Caps), vp, vp]
        f.restype = i32
    for name in ("smol_csum_batch_nhc_udp_emit", "smol_csum_batch_nhc_udp_verify"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, ctypes.POINTER(Caps), vp, vp]
        f.restype = i32
    # added within ABI 6: an older build named by SMOLCSUM_LIB may lack them
    if hasattr(L, "smol_csum_batch_emit_fields"):
        L.smol_csum_batch_emit_fields.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp]
        L.smol_csum_batch_emit_fields.restype = i32
        L.smol_csum_apply_fields.argtypes = [vp, u32, ctypes.POINTER(FieldsC)]
        L.smol_csum_apply_fields.restype = i32
    if hasattr(L, "smol_csum_batch_verify_copy"):
        L.smol_csum_batch_verify_copy.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_copy.restype = i32
    if hasattr(L, "smol_csum_batch_verify_reassemble"):
        L.smol_csum_batch_verify_reassemble.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, u64, ctypes.POINTER(Caps),
                                                        vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_reassemble.restype = i32
    if hasattr(L, "smol_csum_batch_fragment_emit"):
        L.smol_csum_batch_fragment_emit.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp, u32, vp, vp]
        L.smol_csum_batch_fragment_emit.restype = i32
    if hasattr(L, "smol_csum_batch_tcp_segment_emit"):
        L.smol_csum_batch_tcp_segment_emit.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps), vp, vp, vp, u32,
                                                       vp, vp]
        L.smol_csum_batch_tcp_segment_emit.restype = i32
    if hasattr(L, "smol_csum_batch_verify_tcp_assemble"):
        L.smol_csum_batch_verify_tcp_assemble.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, u64, ctypes.POINTER(Caps),
                                                          vp, vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_tcp_assemble.restype = i32
    if hasattr(L, "smol_csum_batch_verify_echo_reply"):
        L.smol_csum_batch_verify_echo_reply.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps),
                                                        ctypes.POINTER(EchoCfgC), vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_echo_reply.restype = i32
    if hasattr(L, "smol_csum_batch_verify_unreach_reply"):
        L.smol_csum_batch_verify_unreach_reply.argtypes = [vp, vp, ctypes.POINTER(BatchC), ctypes.POINTER(Caps),
                                                           ctypes.POINTER(EchoCfgC), vp, vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_unreach_reply.restype = i32
    if hasattr(L, "smol_csum_batch_verify_udp_enqueue"):
        L.smol_csum_batch_verify_udp_enqueue.argtypes = [vp, vp, ctypes.POINTER(BatchC), vp, u64, ctypes.POINTER(Caps),
                                                         vp, vp, vp, vp, vp, vp, vp]
        L.smol_csum_batch_verify_udp_enqueue.restype = i32
    if hasattr(L, "smol_csum_batch_udp_dequeue_emit"):
        L.smol_csum_batch_udp_dequeue_emit.argtypes = [vp, vp, vp, u64, vp, ctypes.POINTER(Caps), vp, u32, vp, vp, vp]
        L.smol_csum_batch_udp_dequeue_emit.restype = i32
    L.smol_csum_last_error.argtypes = []
    L.smol_csum_last_error.restype = ctypes.c_char_p
    L.smol_csum_abi_version.argtypes = []
    L.smol_csum_abi_version.restype = i32
    L.smol_csum_tool_synth.argtypes = [vp, vp, ctypes.POINTER(BatchC), i32, u64, vp]
    L.smol_csum_tool_synth.restype = i32
    L.smol_csum_tool_corrupt.argtypes = [vp, vp, ctypes.POINTER(BatchC), u32, u64, vp]
    L.smol_csum_tool_corrupt.restype = i32
    L.smol_csum_tool_set_shape.argtypes = [vp, i32]
    L.smol_csum_tool_set_shape.restype = i32
    L.smol_csum_tool_set_variant.argtypes = [vp, i32]
    L.smol_csum_tool_set_variant.restype = i32
    L.smol_csum_tool_set_tile.argtypes = [vp, i32]
    L.smol_csum_tool_set_tile.restype = i32
    L.smol_csum_tool_set_max_blocks.argtypes = [vp, u32]
    L.smol_csum_tool_set_max_blocks.restype = i32
    L.smol_csum_tool_set_xcd_remap.argtypes = [vp, ctypes.c_int]
    L.smol_csum_tool_set_xcd_remap.restype = i32
    L.smol_csum_tool_set_launch_records.argtypes = [vp, u64]
    L.smol_csum_tool_set_launch_records.restype = i32
    L.smol_csum_tool_stream_read.argtypes = [vp, vp, u64, vp, vp]
    L.smol_csum_tool_stream_read.restype = i32
    L.smol_csum_tool_field_probe.argtypes = [vp, vp, u64, u64, ctypes.c_uint32, ctypes.c_uint32, vp]
    L.smol_csum_tool_field_probe.restype = i32
    L.smol_csum_tool_field_probe_list.argtypes = [vp, vp, u64, vp, vp, ctypes.c_int, vp]
    L.smol_csum_tool_field_probe_list.restype = i32
    L.smol_csum_tool_field_scatter.argtypes = [vp, vp, u64, vp, vp, u64, ctypes.c_int, vp]
    L.smol_csum_tool_field_scatter.restype = i32
    L.smol_csum_tool_auto_shape.argtypes = [u32, i32]
    L.smol_csum_tool_auto_shape.restype = i32
    L.smol_csum_tool_kernel_name.argtypes = [vp, i32, i32]
    L.smol_csum_tool_kernel_name.restype = ctypes.c_char_p
    L.smol_csum_tool_last_launch.argtypes = []
    L.smol_csum_tool_last_launch.restype = u32
    optional = {
        "smol_csum_tool_variant_built": ([i32], i32),
        "smol_csum_tool_segment_probe": ([vp, vp, u64, vp, ctypes.c_int, vp], i32),
        "smol_csum_tool_kernel_for": ([vp, i32, vp], ctypes.c_char_p),
        "smol_csum_tool_pick": ([i32, i32, i32, i32, ctypes.POINTER(BatchC), i32, ctypes.POINTER(i32)], i32),
        "smol_csum_tool_variant_info": ([i32, ctypes.POINTER(i32)], i32),
        "smol_csum_tool_form": ([i32, i32, ctypes.POINTER(i32)], i32),
        "smol_csum_tool_set_fields_kernel": ([vp, i32], i32),
        "smol_csum_tool_walk_launch": ([i32, i32, i32, i32, i32, ctypes.POINTER(i32)], i32),
        "smol_csum_tool_set_vcopy_stores": ([vp, i32], i32),
        "smol_csum_tool_set_emit_route": ([vp, i32], i32),
        "smol_csum_tool_last_route": ([vp], i32),
        "smol_csum_tool_set_route_chunk": ([vp, u64], i32),
    }
    assert set(optional) == set(OPTIONAL_TOOL_SYMBOLS)
    for name in OPTIONAL_TOOL_SYMBOLS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = optional[name]
    _LIBS[path] = L
    return L


def check(rc: int, what: str, L: ctypes.CDLL | None = None) -> None:
    if rc != SMOL_OK:
        detail = (L or lib()).smol_csum_last_error().decode(errors="replace") if rc == SMOL_EHIP else ""
        raise SmolError(rc, what, detail)
