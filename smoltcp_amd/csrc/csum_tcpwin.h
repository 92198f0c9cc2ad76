// The receive-window rule of smol_csum_batch_verify_tcp_assemble (include/smolcsum.h), and where a
// delivered range lies in the connection's receive ring.  Plain host / device functions with no HIP in
// them, so that the text tcpasm_kernel (csum_tcpasm.hip) runs is walked on the CPU under the sanitizers
// (tests/cpp/tcpwin_asan.cpp).
//
// TcpSocket::process tests a segment against the receive window (segment_in_window,
// src/socket/tcp.rs:1719-1769), trims it to the window at both ends (:1771-1783) and hands the rest to
// rx_buffer.write_unallocated(payload_offset, payload) (:2205-2241), whose two get_unallocated slices
// (src/storage/ring_buffer.rs:321-338) are the two pieces here.
//
// Sequence arithmetic is TcpSeqNumber's: s = (int32)(seq - window_start), W = window_len, p the payload
// length.
//   p == 0: not in the window when s == -1 (a keep-alive or a window probe); with W == 0 in the window
//           iff s == 0; otherwise iff 0 <= s < W.
//   p > 0:  not in the window when W == 0; otherwise in the window iff the first byte is (0 <= s < W) or
//           the last one is (0 < s + p <= W).  A segment that starts before the window and ends past it
//           is NOT in the window: the reference's rule, kept as it is.
// In the window: win_off = max(0, s), len = min(W, s + p) - max(0, s), and the delivered bytes are
// payload bytes [trim, trim + len), trim = max(0, -s).
// Window offset w lives at ring index (ring_pos + w) % ring_len; len <= window_len <= ring_len (the
// group contract), so a delivered range is at most two contiguous pieces: len0 bytes from ring index
// pos0, then len1 bytes from ring index 0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SMOL_TCPWIN_FN __host__ __device__ inline
#else
#define SMOL_TCPWIN_FN inline
#endif

namespace smolcsum {

struct TcpWinRule {
    uint32_t in_window;  // segment_in_window
    uint32_t win_off;    // window offset of the first delivered byte
    uint32_t len;        // delivered bytes
    uint32_t trim;       // payload bytes in front of the first delivered one
    uint32_t pos0;       // ring index of the first piece
    uint32_t len0;       // its bytes
    uint32_t len1;       // bytes of the second piece, at ring index 0 (0: the range does not wrap)
};

// The ring pieces of window range [r.win_off, r.win_off + r.len) (ring_len == 0 only with W == 0: nothing
// to place).
SMOL_TCPWIN_FN void tcpwin_split(TcpWinRule& r, uint32_t ring_pos, uint32_t ring_len) {
    r.pos0 = r.len0 = r.len1 = 0u;
    if (r.len == 0 || ring_len == 0) return;
    r.pos0 = (uint32_t)(((uint64_t)ring_pos + r.win_off) % ring_len);
    const uint32_t room = ring_len - r.pos0;
    r.len0 = r.len < room ? r.len : room;
    r.len1 = r.len - r.len0;
}

SMOL_TCPWIN_FN TcpWinRule tcpwin_rule(uint32_t seq, uint32_t p, uint32_t window_start, uint32_t window_len,
                                      uint32_t ring_pos, uint32_t ring_len) {
    TcpWinRule r = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const int64_t s = (int64_t)(int32_t)(seq - window_start);
    const int64_t W = (int64_t)window_len, e = s + (int64_t)p;
    bool in;
    if (p == 0) in = s == -1 ? false : W == 0 ? s == 0 : (0 <= s && s < W);
    else in = W != 0 && ((0 <= s && s < W) || (0 < e && e <= W));
    if (!in) return r;
    const int64_t lo = s > 0 ? s : 0, hi = e < W ? e : W;
    r.in_window = 1u;
    r.win_off = (uint32_t)lo;
    r.len = (uint32_t)(hi - lo);
    r.trim = (uint32_t)(s < 0 ? -s : 0);
    tcpwin_split(r, ring_pos, ring_len);
    return r;
}

}  // namespace smolcsum
