// ring_fields — OffloadRing::emit_fields against OffloadRing::emit.
//
// Two rings are filled with the same 7003 Ethernet + IPv4 + UDP frames (checksum fields zero, as the
// stack leaves them under ChecksumCapabilities::ignored(), src/phy/mod.rs:223-233).  Every third slot
// is a raw socket's frame (mark_raw): its L4 checksum bytes are the user's, arbitrary, and must come
// through untouched (src/iface/packet.rs:132-136, src/socket/raw.rs:406-423).  One ring goes through
// emit (the frames copied back from the device), the other through emit_fields (16 B per frame back,
// the host writes the fields).  Exit status 0 and the line "fields ring equals in-place ring" only
// when the two rings are byte-identical; the chunk size (1000 slots) makes the burst eight chunks,
// the last one partial, some with raw slots.
//
//   ring_fields [frames]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../smoltcp_amd/host/offload_ring.hpp"

static constexpr uint32_t kSlot = 1514, kEth = 14;

static uint32_t mix(uint32_t x) {
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}

static void build_frame(uint8_t* f, uint32_t i, bool raw) {
    for (uint32_t j = 0; j < kSlot; ++j) f[j] = uint8_t(mix(i * 2048u + j));
    const uint8_t mac_a[6] = {2, 0, 0, 0, 0, 1}, mac_b[6] = {2, 0, 0, 0, 0, 2};
    std::memcpy(f, mac_b, 6);
    std::memcpy(f + 6, mac_a, 6);
    f[12] = 0x08, f[13] = 0x00;
    uint8_t* ip = f + kEth;
    const uint32_t pay = 18 + mix(i) % (kSlot - kEth - 28 - 18 + 1);  // UDP payload bytes; the rest is padding
    const uint32_t tot = 28 + pay;
    ip[0] = 0x45, ip[1] = 0, ip[2] = uint8_t(tot >> 8), ip[3] = uint8_t(tot);
    ip[6] = 0x40, ip[7] = 0, ip[8] = 64, ip[9] = 17, ip[10] = ip[11] = 0;
    uint8_t* u = ip + 20;
    u[0] = 0x13, u[1] = 0x88, u[2] = 0x13, u[3] = 0x89;
    u[4] = uint8_t((8 + pay) >> 8), u[5] = uint8_t(8 + pay);
    u[6] = u[7] = 0;
    if (raw) u[6] = uint8_t(mix(i) >> 8), u[7] = uint8_t(mix(i) >> 16);  // the user's bytes
}

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? uint32_t(std::atoi(argv[1])) : 7003u;
    try {
        smoltcp_amd::OffloadRing in_place(0, n, kSlot, smoltcp_amd::Medium::Ethernet, 1000);
        smoltcp_amd::OffloadRing fields(0, n, kSlot, smoltcp_amd::Medium::Ethernet, 1000);
        for (uint32_t i = 0; i < n; ++i) {
            const bool raw = i % 3 == 0;
            build_frame(in_place.slot(i), i, raw);
            build_frame(fields.slot(i), i, raw);
            in_place.mark_raw(i, raw);
            fields.mark_raw(i, raw);
        }
        in_place.emit(n);
        fields.emit_fields(n);
        uint64_t diff = 0, filled = 0, raw_kept = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t *a = in_place.slot(i), *b = fields.slot(i);
            if (std::memcmp(a, b, kSlot) != 0) {
                if (diff++ < 4) std::fprintf(stderr, "ring_fields: slot %u differs\n", i);
            }
            filled += (b[kEth + 10] | b[kEth + 11]) != 0;
            const bool raw = i % 3 == 0;
            if (raw) raw_kept += b[kEth + 26] == uint8_t(mix(i) >> 8) && b[kEth + 27] == uint8_t(mix(i) >> 16);
        }
        // the comparison means something: headers were filled, and the raw slots kept their L4 bytes
        const uint64_t nraw = (n + 2) / 3;
        if (diff || filled + 2 < n || raw_kept != nraw) {
            std::fprintf(stderr, "ring_fields: %llu of %u slots differ, %llu headers filled, %llu of %llu raw slots kept\n",
                         (unsigned long long)diff, n, (unsigned long long)filled, (unsigned long long)raw_kept,
                         (unsigned long long)nraw);
            return 1;
        }
        std::printf("fields ring equals in-place ring\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ring_fields: %s\n", e.what());
        return 1;
    }
}
