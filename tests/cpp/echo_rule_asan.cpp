// ASan + UBSan walk over the reply-head rule of smol_csum_batch_verify_echo_reply: the host / device functions
// of smoltcp_amd/csrc/csum_echo.h, which echo_kernel calls, run on the CPU (tests/test_echo_rule_cpu.py builds
// and runs this program).  Host code only.
//
// The sweep: kind IP / ETH x IPv4 / IPv6 x source and destination from a table of unicast, multicast,
// unspecified, limited-broadcast and directed-broadcast addresses x bcast_v4 set / unset x MACs with and
// without the group bit x data lengths 0, 1, 2, 3, 56, 1472 and the longest (65507 / 65527).  Each case's
// head goes into a heap buffer of exactly head_len bytes, and is checked against what the functions promise of
// themselves: zero checksum fields at the offsets they name, echo_head_words equal to the bytes' word sum.
//
// Output: "ok <cases> <digest>".  A case's bytes (flags, head_len, then the head's bytes; head_len 0 and no
// bytes unless ANSWERED) are hashed with FNV-1a (64 bit) and the case hashes folded in sweep order,
// d = (d ^ h) * prime.  The Python test recomputes the digest from tests/echo_ref.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../smoltcp_amd/csrc/csum_echo.h"

namespace {

constexpr uint64_t FNV_OFFSET = 0xCBF29CE484222325ull, FNV_PRIME = 0x100000001B3ull;

struct Req {
    uint32_t kind_, ver_, dlen_;
    uint8_t md[6], ms[6], et[2], s[16], d[16], ids[4];
    uint32_t kind() const { return kind_; }
    uint32_t ver() const { return ver_; }
    uint32_t dlen() const { return dlen_; }
    uint32_t mac_dst(uint32_t j) const { return md[j]; }
    uint32_t mac_src(uint32_t j) const { return ms[j]; }
    uint32_t ethertype(uint32_t j) const { return et[j]; }
    uint32_t src(uint32_t j) const { return s[j]; }
    uint32_t dst(uint32_t j) const { return d[j]; }
    uint32_t idseq(uint32_t j) const { return ids[j]; }
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
const uint32_t DLEN[] = {0, 1, 2, 3, 56, 1472, 0};  // the last entry: the longest the length fields hold

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
                            for (uint32_t li = 0; li < 7; ++li) {
                                Req q;
                                std::memset(&q, 0, sizeof q);
                                q.kind_ = kind, q.ver_ = ver;
                                q.dlen_ = li == 6 ? (ver == 4 ? 65507u : 65527u) : DLEN[li];
                                const uint8_t md[6] = {(uint8_t)(0x02 | (mg & 1)), 0x11, 0x22, 0x33, 0x44, 0x55};
                                const uint8_t ms[6] = {(uint8_t)(0x04 | (mg >> 1)), 0xa1, 0xa2, 0xa3, 0xa4, 0xa5};
                                std::memcpy(q.md, md, 6);
                                std::memcpy(q.ms, ms, 6);
                                q.et[0] = ver == 4 ? 0x08 : 0x86, q.et[1] = ver == 4 ? 0x00 : 0xdd;
                                std::memcpy(q.s, ver == 4 ? V4[si] : V6[si], al);
                                std::memcpy(q.d, ver == 4 ? V4[di] : V6[di], al);
                                const uint32_t ids = (uint32_t)(cases * 2654435761ull);
                                for (int j = 0; j < 4; ++j) q.ids[j] = (uint8_t)(ids >> (24 - 8 * j));
                                const uint32_t bcast = bc ? (uint32_t)BCAST[0] << 24 | BCAST[1] << 16 | BCAST[2] << 8 | BCAST[3] : 0u;

                                const uint32_t fl = echo_rule(q, bcast);
                                if (!(fl & SMOL_ECHO_REQUEST) || ((fl & SMOL_ECHO_ANSWERED) && (fl & SMOL_ECHO_HOST)))
                                    fail("flags", cases);
                                const uint32_t hl = (fl & SMOL_ECHO_ANSWERED) ? echo_head_len(kind, ver) : 0u;
                                uint64_t h = FNV_OFFSET;
                                h = (h ^ fl) * FNV_PRIME;
                                h = (h ^ hl) * FNV_PRIME;
                                if (hl) {
                                    std::unique_ptr<uint8_t[]> hb(new uint8_t[hl]);
                                    for (uint32_t i = 0; i < hl; ++i) hb[i] = (uint8_t)echo_head_byte(q, i);
                                    const uint32_t ipo = echo_ipck_off(kind, ver), l4o = echo_l4ck_off(kind, ver);
                                    if ((ver == 4) != (ipo != ECHO_NO_FIELD)) fail("ipck offset", cases);
                                    if (ipo != ECHO_NO_FIELD && (ipo + 2 > hl || hb[ipo] || hb[ipo + 1])) fail("ipck field", cases);
                                    if (l4o + 2 > hl || hb[l4o] || hb[l4o + 1]) fail("l4ck field", cases);
                                    const uint32_t e = kind == SMOL_KIND_ETH ? 14u : 0u;
                                    uint32_t s = 0;
                                    for (uint32_t i = e; i + 1 < hl; i += 2) s += (uint32_t)hb[i] << 8 | hb[i + 1];
                                    if (echo_head_words(q, e, (hl - e) / 2) != s) fail("head words", cases);
                                    for (uint32_t i = 0; i < hl; ++i) h = (h ^ hb[i]) * FNV_PRIME;
                                }
                                digest = (digest ^ h) * FNV_PRIME;
                                ++cases;
                            }
        }
    std::printf("ok %" PRIu64 " %016" PRIx64 "\n", cases, digest);
    return 0;
}
