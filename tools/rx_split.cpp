// rx_split — Engine::verify_copy as a NIC's header/data split: one pass over a device-resident RX burst
// verifies every frame and delivers its L4 payload into a dense payload arena.
//
// 6007 Ethernet frames are built on the host: UDP and TCP over IPv4 and IPv6 with valid checksums (the
// host mirror of wire::checksum fills them), payloads of 0 .. 1400 bytes, every seventh frame with one
// flipped bit, every eleventh an ICMPv4 echo (no payload span), every thirteenth delivered to a slot one
// byte too small.  The arena is filled with a sentinel first.  Checked: every arena byte (the payloads
// where this program's own slicing of the frames puts them, the sentinel everywhere else), every span,
// and the status bytes against Engine::verify.  Exit status 0 and one line "rx_split ok: ..." only when
// all of it matches.
//
//   rx_split [frames]
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../smoltcp_amd/host/smoltcp_checksum.hpp"

static constexpr uint32_t kSlot = 1514, kEth = 14;
static constexpr uint8_t kSentinel = 0xA5;

static uint32_t mix(uint32_t x) {
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}

static void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

static void put16(uint8_t* p, uint32_t v) { p[0] = uint8_t(v >> 8), p[1] = uint8_t(v); }

static uint16_t fold(uint32_t s) {
    s = (s >> 16) + (s & 0xffffu);
    return uint16_t((s >> 16) + s);
}
static uint32_t sum_be(const uint8_t* p, uint32_t n, uint32_t s = 0) {
    for (uint32_t i = 0; i + 1 < n; i += 2) s += uint32_t(p[i]) << 8 | p[i + 1];
    if (n & 1) s += uint32_t(p[n - 1]) << 8;
    return s;
}

struct Built {
    uint32_t len;      // frame bytes
    uint32_t off, pay; // this program's own slicing: where the payload lies in the frame
    bool span;         // UDP / TCP
};

// Frame i into f (kSlot bytes, random fill first); checksums valid.
static Built build_frame(uint8_t* f, uint32_t i) {
    for (uint32_t j = 0; j < kSlot; ++j) f[j] = uint8_t(mix(i * 2048u + j));
    const uint8_t mac_a[6] = {2, 0, 0, 0, 0, 1}, mac_b[6] = {2, 0, 0, 0, 0, 2};
    std::memcpy(f, mac_b, 6);
    std::memcpy(f + 6, mac_a, 6);
    const bool v6 = (i & 1) != 0, icmp = i % 11 == 5;
    const bool tcp = !icmp && (i & 2) != 0;
    const uint32_t pay = mix(i ^ 0x9e3779b9u) % 1401;
    const uint32_t l4h = icmp ? 8 : tcp ? 20 + 4 * (i % 5) : 8;
    const uint32_t l4len = l4h + pay;
    const uint32_t proto = icmp ? (v6 ? 58u : 1u) : tcp ? 6u : 17u;
    uint8_t* ip = f + kEth;
    uint8_t* l4;
    uint32_t ps = 0;  // pseudo-header sum
    if (v6) {
        put16(f + 12, 0x86dd);
        ip[0] = 0x60, ip[1] = ip[2] = ip[3] = 0;
        put16(ip + 4, l4len);
        ip[6] = uint8_t(proto), ip[7] = 64;
        for (int k = 0; k < 32; ++k) ip[8 + k] = uint8_t(0x20 + k + (i & 7));
        l4 = ip + 40;
        ps = sum_be(ip + 8, 32) + proto + l4len;
    } else {
        put16(f + 12, 0x0800);
        ip[0] = 0x45, ip[1] = 0;
        put16(ip + 2, 20 + l4len);
        put16(ip + 4, i & 0xffff);
        ip[6] = 0x40, ip[7] = 0, ip[8] = 64, ip[9] = uint8_t(proto), ip[10] = ip[11] = 0;
        ip[12] = 10, ip[13] = 1, ip[14] = uint8_t(i >> 8), ip[15] = uint8_t(i);
        ip[16] = 10, ip[17] = 4, ip[18] = 5, ip[19] = 6;
        put16(ip + 10, uint16_t(~fold(sum_be(ip, 20))));
        l4 = ip + 20;
        ps = sum_be(ip + 12, 8) + proto + l4len;
    }
    uint32_t fo;
    if (icmp) {
        l4[0] = v6 ? 128 : 8, l4[1] = 0;
        fo = 2;
        if (!v6) ps = 0;  // ICMPv4 has no pseudo-header
    } else if (tcp) {
        put16(l4, 1024 + i % 50000), put16(l4 + 2, 80);
        l4[12] = uint8_t((l4h / 4) << 4), l4[13] = 0x18;
        for (uint32_t k = 20; k < l4h; ++k) l4[k] = 1;  // NOP options
        fo = 16;
    } else {
        put16(l4, 1024 + i % 50000), put16(l4 + 2, 53);
        put16(l4 + 4, l4len);
        fo = 6;
    }
    l4[fo] = l4[fo + 1] = 0;
    uint16_t c = uint16_t(~fold(sum_be(l4, l4len, ps)));
    if (proto == 17 && c == 0) c = 0xffff;
    put16(l4 + fo, c);
    Built b;
    b.len = uint32_t(l4 - f) + l4len;
    b.span = !icmp;
    b.off = b.span ? uint32_t(l4 - f) + l4h : 0;
    b.pay = b.span ? pay : 0;
    if (i % 7 == 3) f[kEth + (mix(i) % (b.len - kEth))] ^= uint8_t(1u << (i % 8));  // one flipped bit past the MACs
    return b;
}

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? uint32_t(std::atoi(argv[1])) : 6007u;
    try {
        std::vector<uint8_t> frames(size_t(n) * kSlot);
        std::vector<Built> built(n);
        std::vector<smol_csum_desc_t> desc(n);
        std::vector<smol_csum_slot_t> slots(n);
        uint64_t arena = 0;
        for (uint32_t i = 0; i < n; ++i) {
            built[i] = build_frame(&frames[size_t(i) * kSlot], i);
            std::memset(&desc[i], 0, sizeof desc[i]);
            desc[i].offset = uint64_t(i) * kSlot;
            desc[i].len = built[i].len;
            desc[i].kind = SMOL_KIND_ETH;
            // the arena is dense: slot i starts where slot i - 1 ends (any alignment)
            slots[i].dst_offset = arena;
            slots[i].cap = built[i].pay - (i % 13 == 7 && built[i].pay ? 1u : 0u);
            slots[i].reserved = 0;
            arena += slots[i].cap;
        }
        // A flipped bit may land in a length field: slice the frames as the span rule does only where
        // the frame is as built, and take the verdict on the others from verify alone.
        uint8_t *d_frames, *d_arena, *d_status, *d_status2;
        smol_csum_desc_t* d_desc;
        smol_csum_slot_t* d_slots;
        smol_csum_span_t* d_spans;
        hip_check(hipMalloc(&d_frames, frames.size() + 16), "hipMalloc");
        hip_check(hipMalloc(&d_arena, arena + 16), "hipMalloc");
        hip_check(hipMalloc(&d_status, n), "hipMalloc");
        hip_check(hipMalloc(&d_status2, n), "hipMalloc");
        hip_check(hipMalloc(&d_desc, n * sizeof(smol_csum_desc_t)), "hipMalloc");
        hip_check(hipMalloc(&d_slots, n * sizeof(smol_csum_slot_t)), "hipMalloc");
        hip_check(hipMalloc(&d_spans, n * sizeof(smol_csum_span_t)), "hipMalloc");
        hip_check(hipMemcpy(d_frames, frames.data(), frames.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(d_desc, desc.data(), n * sizeof(smol_csum_desc_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(d_slots, slots.data(), n * sizeof(smol_csum_slot_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemset(d_arena, kSentinel, arena + 16), "hipMemset");

        smoltcp_amd::Engine eng(0);
        const auto batch = smoltcp_amd::Batch::described(d_desc, n);
        eng.verify_copy(d_frames, batch, d_arena, d_slots, d_status, d_spans);
        eng.verify(d_frames, batch, d_status2);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");

        std::vector<uint8_t> got(arena + 16), st(n), st2(n);
        std::vector<smol_csum_span_t> spans(n);
        hip_check(hipMemcpy(got.data(), d_arena, arena + 16, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(st.data(), d_status, n, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(st2.data(), d_status2, n, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(spans.data(), d_spans, n * sizeof(smol_csum_span_t), hipMemcpyDeviceToHost), "hipMemcpy");

        std::vector<uint8_t> want(arena + 16, kSentinel);
        uint64_t bad_status = 0, bad_span = 0, accepted = 0, delivered = 0, held = 0, bytes = 0, flipped_skipped = 0, flipped_accepted = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const Built& b = built[i];
            const smol_csum_span_t& s = spans[i];
            bad_status += st[i] != st2[i];
            accepted += (st[i] & SMOL_ST_ACCEPT) != 0;
            const bool flipped = i % 7 == 3;
            // (a flipped bit passes only where no checksum covers it: an IPv6 header's class, flow label, hop limit)
            flipped_accepted += flipped && (st[i] & SMOL_ST_ACCEPT);
            // a flipped frame whose span differs from the built one had the bit in a header field the
            // span depends on: the reported span then decides what is expected in the arena
            uint32_t off = b.off, pay = b.pay;
            bool span = b.span;
            if (flipped && (s.off != off || s.len != pay)) {
                ++flipped_skipped;
                span = s.off != 0;
                off = s.off, pay = s.len;
                if (span && uint64_t(off) + pay > b.len) ++bad_span;
            } else if (s.off != off || s.len != pay) {
                ++bad_span;
            }
            const bool fits = span && pay <= slots[i].cap;
            if (s.copied != (fits ? 1 : 0) || s.reserved != 0) ++bad_span;
            if (fits) {
                std::memcpy(&want[slots[i].dst_offset], &frames[size_t(i) * kSlot + off], pay);
                ++delivered, bytes += pay;
            } else if (span) {
                ++held;
            }
        }
        uint64_t diff = 0;
        for (uint64_t j = 0; j < arena + 16; ++j) diff += got[j] != want[j];
        for (void* q : {(void*)d_frames, (void*)d_arena, (void*)d_status, (void*)d_status2, (void*)d_desc, (void*)d_slots,
                        (void*)d_spans})
            (void)hipFree(q);
        if (diff || bad_status || bad_span || !delivered || !held || accepted == 0 || accepted == n ||
            flipped_skipped * 4 > n / 7 || flipped_accepted * 8 > n / 7) {
            std::fprintf(stderr,
                         "rx_split: %llu arena bytes differ, %llu status bytes differ from verify, %llu spans wrong "
                         "(%llu delivered, %llu held, %llu accepted, %llu flipped frames with another span, %llu accepted)\n",
                         (unsigned long long)diff, (unsigned long long)bad_status, (unsigned long long)bad_span,
                         (unsigned long long)delivered, (unsigned long long)held, (unsigned long long)accepted,
                         (unsigned long long)flipped_skipped, (unsigned long long)flipped_accepted);
            return 1;
        }
        std::printf("rx_split ok: %u frames, %llu accepted, %llu payloads (%llu bytes) delivered, %llu held back by their cap\n",
                    n, (unsigned long long)accepted, (unsigned long long)delivered, (unsigned long long)bytes,
                    (unsigned long long)held);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rx_split: %s\n", e.what());
        return 1;
    }
}
