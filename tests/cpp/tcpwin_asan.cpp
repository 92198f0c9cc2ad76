// The receive-window rule and the ring split of smol_csum_batch_verify_tcp_assemble
// (smoltcp_amd/csrc/csum_tcpwin.h tcpwin_rule, the function tcpasm_kernel calls) walked on the CPU:
// window lengths 0 .. 20, sequence offsets -26 .. 26, payload lengths 0 .. 24, rings of W .. W + 3 bytes at
// every ring position, window_start near 0, 2^31 and 2^32 - 1.  Every case is checked against a brute force
// written here: segment_in_window as src/socket/tcp.rs:1719-1769 states it, on 64-bit sequence numbers
// that do not wrap, and the delivered bytes one by one, each put at its ring index in a heap block of
// exactly ring_len entries.
// Stand-alone (its own main), built with -fsanitize=address,undefined by tests/test_tcpwin_rule_cpu.py.
// Prints "ok <cases> <digest>": every case's seven outputs hashed with FNV-1a (64 bit, little-endian bytes),
// the case hashes folded in sweep order, d = (d ^ h) * prime.  tests/test_tcpwin_rule_cpu.py recomputes the
// digest with tests/tcp_assemble_ref.py over the same sweep.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../smoltcp_amd/csrc/csum_tcpwin.h"

using namespace smolcsum;

namespace {

constexpr uint64_t FNV_OFFSET = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;

[[noreturn]] void fail(const char* what, uint32_t ws, int W, int rl, int rp, int s, int p) {
    std::printf("FAIL %s: window_start %u, W %d, ring_len %d, ring_pos %d, s %d, p %d\n", what, ws, W, rl, rp, s, p);
    std::exit(1);
}

// segment_in_window, the reference's match on numbers that do not wrap
bool in_window_ref(int64_t seg_start, int64_t seg_end, int64_t win_start, int64_t win_end) {
    const bool empty_seg = seg_start == seg_end, empty_win = win_start == win_end;
    if (empty_seg && seg_end == win_start - 1) return false;
    if (empty_seg && empty_win) return win_start == seg_start;
    if (empty_seg) return win_start <= seg_start && seg_start < win_end;
    if (empty_win) return false;
    return (win_start <= seg_start && seg_start < win_end) || (win_start < seg_end && seg_end <= win_end);
}

uint64_t case_hash(const TcpWinRule& r) {
    const uint32_t w[7] = {r.in_window, r.win_off, r.len, r.trim, r.pos0, r.len0, r.len1};
    uint64_t h = FNV_OFFSET;
    for (uint32_t x : w)
        for (int b = 0; b < 4; ++b) h = (h ^ ((x >> (8 * b)) & 0xffu)) * FNV_PRIME;
    return h;
}

}  // namespace

int main() {
    const uint32_t starts[3] = {1u, 0x7ffffff8u, 0xfffffffbu};
    unsigned long long cases = 0;
    uint64_t digest = FNV_OFFSET;
    for (uint32_t ws : starts)
        for (int W = 0; W <= 20; ++W)
            for (int rl = W; rl <= W + 3; ++rl)
                for (int rp = 0; rp < (rl ? rl : 1); ++rp)
                    for (int s = -26; s <= 26; ++s)
                        for (int p = 0; p <= 24; ++p) {
                            const uint32_t seq = ws + (uint32_t)s;
                            const TcpWinRule r = tcpwin_rule(seq, (uint32_t)p, ws, (uint32_t)W, (uint32_t)rp, (uint32_t)rl);
                            ++cases;
                            digest = (digest ^ case_hash(r)) * FNV_PRIME;

                            const int64_t a = (int64_t)ws + s;
                            const bool in = in_window_ref(a, a + p, (int64_t)ws, (int64_t)ws + W);
                            if ((r.in_window != 0) != in) fail("in_window", ws, W, rl, rp, s, p);
                            if (p > 0) {  // a segment with data is in the window iff its first or last byte is
                                const bool f = 0 <= s && s < W, l = 0 <= s + p - 1 && s + p - 1 < W;
                                if (in != (W > 0 && (f || l))) fail("first or last byte", ws, W, rl, rp, s, p);
                            }
                            if (!in) {
                                if (r.win_off | r.len | r.trim | r.pos0 | r.len0 | r.len1) fail("outputs not zero", ws, W, rl, rp, s, p);
                                continue;
                            }
                            // the delivered bytes, one by one: payload byte i has window offset s + i
                            int cnt = 0, first = -1;
                            int* ring = new int[rl ? rl : 1];
                            for (int i = 0; i < (rl ? rl : 1); ++i) ring[i] = -1;
                            for (int i = 0; i < p; ++i) {
                                const int o = s + i;
                                if (o < 0 || o >= W) continue;
                                if (first < 0) first = i;
                                ++cnt;
                                ring[(rp + o) % rl] = i;  // (rl >= W > o >= 0)
                            }
                            if ((int)r.len != cnt) fail("len", ws, W, rl, rp, s, p);
                            if (cnt) {
                                if ((int)r.trim != first || (int)r.win_off != s + first) fail("trim / win_off", ws, W, rl, rp, s, p);
                            } else if (r.trim != 0 || (int)r.win_off != s) {
                                fail("empty segment", ws, W, rl, rp, s, p);
                            }
                            if ((int)(r.len0 + r.len1) != cnt || (r.len1 && (int)(r.pos0 + r.len0) != rl) || (cnt && r.len0 == 0))
                                fail("pieces", ws, W, rl, rp, s, p);
                            for (uint32_t k = 0; k < r.len0; ++k)
                                if (ring[r.pos0 + k] != first + (int)k) fail("piece 0", ws, W, rl, rp, s, p);
                            for (uint32_t k = 0; k < r.len1; ++k)
                                if (ring[k] != first + (int)(r.len0 + k)) fail("piece 1", ws, W, rl, rp, s, p);
                            delete[] ring;
                        }
    std::printf("ok %llu %016llx\n", cases, (unsigned long long)digest);
    return 0;
}
