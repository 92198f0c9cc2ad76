// ASan + UBSan walk over the refusal rule of smol_csum_batch_verify_unreach_reply: the host / device functions
// of smoltcp_amd/csrc/csum_unreach.h, which unreach_kernel calls, run on the CPU (tests/test_unreach_rule_cpu.py
// builds and runs this program).  Host code only.
//
// The sweep: kind IP / ETH x IPv4 / IPv6 x source and destination from a table of unicast, multicast,
// unspecified, limited-broadcast and directed-broadcast addresses x bcast_v4 set / unset x MACs with and
// without the group bit x protocol / next header 0, 1, 6, 17, 58, 47 x (IPv6) with and without a leading
// Hop-by-Hop header x the port map's bit clear / set x P 0, 8, 528, 1193 and the longest (65515 / 65535).  Each
// case's head goes into a heap buffer of exactly head_len bytes, and is checked against what the functions
// promise of themselves: zero checksum fields at the offsets they name, unreach_head_words equal to the bytes'
// word sum whole and shared among 8 lanes, the frame within 576 / 1280 bytes of IP.
//
// Output: "ok <cases> <digest>".  A case's bytes (flags, type, code, head_len, then the head's bytes; type,
// code 0 unless REFUSED, head_len 0 and no bytes unless ANSWERED) are hashed with FNV-1a (64 bit) and the case
// hashes folded in sweep order, d = (d ^ h) * prime.  The Python test recomputes the digest from
// tests/unreach_ref.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../smoltcp_amd/csrc/csum_unreach.h"

namespace {

constexpr uint64_t FNV_OFFSET = 0xCBF29CE484222325ull, FNV_PRIME = 0x100000001B3ull;

struct Req {
    uint32_t kind_, ver_, plen_, proto_, hop_;
    bool hbh_;
    uint8_t md[6], ms[6], et[2], s[16], d[16];
    uint32_t kind() const { return kind_; }
    uint32_t ver() const { return ver_; }
    uint32_t plen() const { return plen_; }
    uint32_t proto() const { return proto_; }
    uint32_t hop() const { return hop_; }
    bool hbh() const { return hbh_; }
    uint32_t mac_dst(uint32_t j) const { return md[j]; }
    uint32_t mac_src(uint32_t j) const { return ms[j]; }
    uint32_t ethertype(uint32_t j) const { return et[j]; }
    uint32_t src(uint32_t j) const { return s[j]; }
    uint32_t dst(uint32_t j) const { return d[j]; }
};

const uint8_t V4[][4] = {{10, 1, 2, 3},     {192, 168, 7, 9},      {224, 0, 0, 1}, {239, 255, 255, 250},
                         {0, 0, 0, 0},      {255, 255, 255, 255},  {10, 1, 2, 255}};
const uint8_t BCAST[4] = {10, 1, 2, 255};
const uint8_t V6[][16] = {
    {0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x12, 0x34},
    {0xff, 0x02, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
};
const uint32_t PROTO[] = {0, 1, 6, 17, 58, 47};
const uint32_t PLEN[] = {0, 8, 528, 1193, 0};  // the last entry: the longest the length fields hold

void fail(const char* what, uint64_t c) {
    std::printf("FAIL %s at case %" PRIu64 "\n", what, c);
    std::exit(1);
}

}  // namespace

int main() {
    using namespace smolcsum;
    uint64_t cases = 0, digest = FNV_OFFSET;
    for (uint32_t kind = SMOL_KIND_IP; kind <= SMOL_KIND_ETH; ++kind)
        for (uint32_t ver = 4; ver <= 6; ver += 2) {
            const uint32_t na = ver == 4 ? 7 : 5, al = ver == 4 ? 4 : 16;
            for (uint32_t si = 0; si < na; ++si)
                for (uint32_t di = 0; di < na; ++di)
                    for (uint32_t bc = 0; bc < 2; ++bc)
                        for (uint32_t mg = 0; mg < 4; ++mg)
                            for (uint32_t pi = 0; pi < 6; ++pi)
                                for (uint32_t hb = 0; hb < (ver == 6 ? 2u : 1u); ++hb)
                                    for (uint32_t closed = 0; closed < 2; ++closed)
                                        for (uint32_t li = 0; li < 5; ++li) {
                                            Req q;
                                            std::memset(&q, 0, sizeof q);
                                            q.kind_ = kind, q.ver_ = ver, q.proto_ = PROTO[pi], q.hbh_ = hb != 0;
                                            q.plen_ = li == 4 ? (ver == 4 ? 65515u : 65535u) : PLEN[li];
                                            q.hop_ = (uint32_t)((cases * 7u + 1u) & 0xffu);
                                            const uint8_t md[6] = {(uint8_t)(0x02 | (mg & 1)), 0x11, 0x22, 0x33, 0x44, 0x55};
                                            const uint8_t ms[6] = {(uint8_t)(0x04 | (mg >> 1)), 0xa1, 0xa2, 0xa3, 0xa4, 0xa5};
                                            std::memcpy(q.md, md, 6);
                                            std::memcpy(q.ms, ms, 6);
                                            q.et[0] = ver == 4 ? 0x08 : 0x86, q.et[1] = ver == 4 ? 0x00 : 0xdd;
                                            std::memcpy(q.s, ver == 4 ? V4[si] : V6[si], al);
                                            std::memcpy(q.d, ver == 4 ? V4[di] : V6[di], al);
                                            const uint32_t bcast =
                                                bc ? (uint32_t)BCAST[0] << 24 | BCAST[1] << 16 | BCAST[2] << 8 | BCAST[3] : 0u;

                                            const uint32_t rv = unreach_rule(q, bcast, closed != 0);
                                            const uint32_t fl = unreach_flags(rv);
                                            if (!fl && rv) fail("type / code without flags", cases);
                                            if (fl && !(fl & SMOL_UNR_REFUSED)) fail("flags without REFUSED", cases);
                                            if ((fl & SMOL_UNR_ANSWERED) && (fl & SMOL_UNR_HOST)) fail("ANSWERED and HOST", cases);
                                            if (fl & (SMOL_UNR_WRITTEN | SMOL_UNR_SEND)) fail("the kernel's flags", cases);
                                            if (((fl & SMOL_UNR_PORT) != 0) != (fl && q.proto_ == 17)) fail("PORT", cases);
                                            const uint32_t hl = (fl & SMOL_UNR_ANSWERED) ? unreach_head_len(kind, ver) : 0u;
                                            uint64_t h = FNV_OFFSET;
                                            h = (h ^ fl) * FNV_PRIME;
                                            h = (h ^ unreach_type(rv)) * FNV_PRIME;
                                            h = (h ^ unreach_code(rv)) * FNV_PRIME;
                                            h = (h ^ hl) * FNV_PRIME;
                                            if (hl) {
                                                if (q.hbh_) fail("a frame behind a Hop-by-Hop header", cases);
                                                const uint32_t dlen = unreach_dlen(ver, q.plen_);
                                                const uint32_t e = kind == SMOL_KIND_ETH ? 14u : 0u;
                                                if (dlen > q.plen_ || dlen > (ver == 4 ? UNR_DATA_V4 : UNR_DATA_V6) ||
                                                    hl - e + dlen > (ver == 4 ? 576u : 1280u))
                                                    fail("data length", cases);
                                                std::unique_ptr<uint8_t[]> hb_(new uint8_t[hl]);
                                                for (uint32_t i = 0; i < hl; ++i) hb_[i] = (uint8_t)unreach_head_byte(q, rv, i);
                                                const uint32_t ipo = unreach_ipck_off(kind, ver), l4o = unreach_l4ck_off(kind, ver);
                                                const uint32_t ino = unreach_inck_off(kind, ver);
                                                if ((ver == 4) != (ipo != ECHO_NO_FIELD) || (ver == 4) != (ino != ECHO_NO_FIELD))
                                                    fail("ipck offsets", cases);
                                                if (ipo != ECHO_NO_FIELD && (ipo + 2 > hl || hb_[ipo] || hb_[ipo + 1])) fail("ipck field", cases);
                                                if (ino != ECHO_NO_FIELD && (ino + 2 > hl || hb_[ino] || hb_[ino + 1])) fail("inck field", cases);
                                                if (l4o + 2 > hl || hb_[l4o] || hb_[l4o + 1]) fail("l4ck field", cases);
                                                uint32_t s = 0, shared = 0;
                                                for (uint32_t i = e; i + 1 < hl; i += 2) s += (uint32_t)hb_[i] << 8 | hb_[i + 1];
                                                if (unreach_head_words(q, rv, e, (hl - e) / 2) != s) fail("head words", cases);
                                                for (uint32_t lane = 0; lane < 8; ++lane)
                                                    shared += unreach_head_words(q, rv, e, (hl - e) / 2, lane, 8u);
                                                if (shared != s) fail("head words over 8 lanes", cases);
                                                for (uint32_t i = 0; i < hl; ++i) h = (h ^ hb_[i]) * FNV_PRIME;
                                            }
                                            digest = (digest ^ h) * FNV_PRIME;
                                            ++cases;
                                        }
        }
    std::printf("ok %" PRIu64 " %016" PRIx64 "\n", cases, digest);
    return 0;
}
