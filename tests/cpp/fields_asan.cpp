// Sanitizer driver for smol_csum_apply_fields (smoltcp_amd/csrc/csum_scalar.cpp), built with
// -fsanitize=address,undefined by tests/test_fields_sanitize_cpu.py.  Every record sits in a heap block
// of exactly its length, so a write or read one byte past a record is a report.  Checked besides: the
// bytes written (big-endian, at the entry's offsets only), SMOL_NO_FIELD skipped, and SMOL_ERANGE with
// the record left unchanged whenever a field does not fit.
//
//   fields_asan [seed] [records]      prints "ok <records>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/smolcsum.h"

static uint64_t g_state;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int fail(const char* what, uint32_t i) {
    std::fprintf(stderr, "fields_asan: %s (case %u)\n", what, i);
    return 1;
}

int main(int argc, char** argv) {
    g_state = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    const uint32_t cases = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 20000;
    for (uint32_t i = 0; i < cases; ++i) {
        // lengths around the edges: empty, 1, 2, and up to the longest offset a u16 can name
        const uint32_t pick = rnd() % 8;
        const uint32_t len = pick == 0 ? rnd() % 4 : pick == 1 ? 65535 + rnd() % 4 : rnd() % 2200;
        uint8_t* rec = (uint8_t*)std::malloc(len ? len : 1);
        if (!rec) return fail("malloc", i);
        if (len == 0) {  // a record of no bytes: a block of no bytes
            std::free(rec);
            rec = (uint8_t*)std::malloc(0);
            if (!rec) return fail("malloc(0)", i);
        }
        std::vector<uint8_t> before(len);
        for (uint32_t j = 0; j < len; ++j) before[j] = (uint8_t)rnd();
        if (len) std::memcpy(rec, before.data(), len);
        smol_csum_fields_t f;
        std::memset(&f, 0, sizeof f);
        bool fits = true;
        for (int k = 0; k < 3; ++k) {
            const uint32_t m = rnd() % 8;
            // none, inside, the last two bytes, straddling the end, just past it, far past it; distinct
            // thirds of the record so that the fields never overlap
            uint32_t off;
            const uint32_t third = len / 3, base = third * (uint32_t)k;
            if (m == 0) off = SMOL_NO_FIELD;
            else if (m == 1 && k == 2 && len >= 2) off = len - 2;
            else if (m == 2) off = len ? len - 1 : 0;
            else if (m == 3) off = len;
            else if (m == 4) off = 0xfffe;
            else off = third >= 2 ? base + rnd() % (third - 1) : len + 1;
            if (off > 0xfffe && off != SMOL_NO_FIELD) off = 0xfffe;
            f.off[k] = (uint16_t)off;
            f.val[k] = (uint16_t)rnd();
            if (off != SMOL_NO_FIELD && off + 2 > len) fits = false;
        }
        f.status = (uint8_t)rnd();
        const int rc = smol_csum_apply_fields(rec, len, &f);
        if (rc != (fits ? SMOL_OK : SMOL_ERANGE)) return fail("return code", i);
        std::vector<uint8_t> want(before);
        if (fits)
            for (int k = 0; k < 3; ++k)
                if (f.off[k] != SMOL_NO_FIELD) {
                    want[f.off[k]] = (uint8_t)(f.val[k] >> 8);
                    want[f.off[k] + 1] = (uint8_t)f.val[k];
                }
        if (len && std::memcmp(rec, want.data(), len) != 0) return fail(fits ? "bytes written" : "record changed on ERANGE", i);
        std::free(rec);
    }
    smol_csum_fields_t f;
    std::memset(&f, 0, sizeof f);
    uint8_t one[2] = {0, 0};
    if (smol_csum_apply_fields(nullptr, 2, &f) != SMOL_EINVAL || smol_csum_apply_fields(one, 2, nullptr) != SMOL_EINVAL)
        return fail("NULL arguments", cases);
    static_assert(sizeof(smol_csum_fields_t) == 16, "the entry is 16 bytes");
    std::printf("ok %u\n", cases);
    return 0;
}
