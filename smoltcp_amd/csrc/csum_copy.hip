// Fused payload copy + emit, second design (variant 17): the walk kernel's MODE_COPY split by chunk
// class, so that the bulk of a record costs what a copy costs.
//
// TcpRepr::emit / UdpRepr::emit copy the payload into the packet and then fill the checksum
// (src/wire/tcp.rs:1087-1095, src/wire/udp.rs:300-308).  The result here is bit-identical to a
// memcpy of every payload followed by smol_csum_batch_emit, as in MODE_COPY of csum_walk.h, whose
// helpers (rec_at, parse_geometry, finish_gates) this kernel shares.
//
// A group of G lanes owns a record.  Its 16-B destination chunks fall into two classes:
// * BODY chunks lie past the 128-B header window and entirely inside the copy range.  A lane reads
//   the 16 source bytes from the chunk's first source byte rounded down to 4 (one dwordx4 load) and
//   the dword after them (one dword load, not issued when no record of the wavefront needs it),
//   shifts them to the destination alignment with four v_alignbyte, sums them and stores them: no
//   destination load, no mask, no neighbour exchange.  That loop is unrolled U deep, all loads
//   issued first.
// * GENERIC chunks — the window (the first 128 B of the chunk grid, which hold the headers the gates
//   parse) and any chunk past it that holds bytes outside the copy range (normally just the
//   record's last chunk) — are built from the destination chunk and two aligned source chunks with
//   byte masks.  The window, the first few other generic chunks and the first UB * G body chunks are
//   loaded in ONE round before the parse, so a C2copy record takes one round trip for its headers,
//   tail and first body chunks, then one for the rest of its body.
// Every byte of the record is written (bytes outside the copy range with their own values, so no
// line is left half-written by this kernel); the window chunks go out last from LDS, with the
// fields finish_gates patched in.  A field past the window (behind a long IPv6 Hop-by-Hop header)
// is left out of the chunk stores and written by finish_gates.
#include "csum_copyemit.h"

namespace smolcsum {

// F: the form, one of csum_variants.h's named structs (CPlain and what differs from it); variants.def says
// which number runs which.  G x U x UW0 x UB: the launch shape (csum_launch.h with_copy_shape).
template <class F, int G, int U, bool IMPLICIT, int UW0 = 0, int UB = 0>
__global__ __launch_bounds__(256) void copy_kernel(KParams p) {
    using namespace copyemit;
    constexpr bool LBS = F::LBS;
    constexpr int GPB = 256 / G;
    // slots per lane loaded before the parse (UW0, or enough for the window plus 8 chunks past it):
    // the window, then the generic chunks past it, then the first body chunks
    constexpr int UW = UW0 > 0 ? UW0 : (WIN_CH + 8 + G - 1) / G;
    constexpr uint32_t NEX = (uint32_t)(UW * G - WIN_CH);  // chunks past the window in that round
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "group size");
    __shared__ u32x4 win[GPB][WIN_CH];
    __shared__ Geom geo[GPB];

    const int lane = (int)(threadIdx.x % G);
    const int gib = (int)(threadIdx.x / G);
    const uint64_t ngroups = (uint64_t)gridDim.x * GPB;
    u32x4* wn = &win[gib][0];
    const uint8_t* winb = reinterpret_cast<const uint8_t*>(wn);
    const uint64_t dummy = (uint64_t)p.dummy;

    for (uint64_t r = logical_block(p.xcd_remap) * GPB + gib; r < p.n; r += ngroups) {
        const RecRef rr = rec_at<IMPLICIT, true>(p, r);
        if (rr.kind & KIND_BAD_COPY) {  // the copy range does not fit: record left untouched
            if (lane == 0 && p.status) ((gu8)p.status)[r] = (uint8_t)SMOL_ST_MALFORMED;
            continue;
        }
        const RecGeomHeld q(rr.a0, n_chunks<false>(rr), rr.sb, rr.p0, rr.p1);
        const uint64_t base = q.base, sk = q.sk();
        const uint32_t head = q.head, nch = q.nch;
        const bool pay = q.pay();
        // body chunks [kb0, kb1): past the window, entirely inside the copy range
        uint32_t kb0 = pay ? (head + rr.p0 + 15) >> 4 : nch;
        kb0 = kb0 > (uint32_t)WIN_CH ? kb0 : (uint32_t)WIN_CH;
        uint32_t kb1 = pay ? (head + rr.p1) >> 4 : 0u;
        kb1 = kb1 < nch ? kb1 : nch;
        kb1 = kb1 > kb0 ? kb1 : kb0;
        // generic chunks past the window: [WIN_CH, min(kb0, nch)) then [kb1, nch)
        const uint32_t e1 = kb0 < nch ? kb0 : nch;
        const uint32_t n1 = e1 > (uint32_t)WIN_CH ? e1 - WIN_CH : 0u;
        const uint32_t n2 = nch > kb1 ? nch - kb1 : 0u;
        const uint32_t ne = n1 + n2;
        auto gen_k = [&](uint32_t e) -> uint32_t { return e < n1 ? WIN_CH + e : kb1 + (e - n1); };
        const uint32_t nb = kb1 - kb0;
        // body chunks that ride in round 1's spare slots (built there the generic way)
        // (UB > 0: none; the first UB * G body chunks are loaded the body way in round 1 instead)
        const uint32_t body1 = UB == 0 && ne < NEX ? (nb < NEX - ne ? nb : NEX - ne) : 0u;
        const uint32_t nbe = UB > 0 ? (nb < (uint32_t)(UB * G) ? nb : (uint32_t)(UB * G)) : 0u;
        // chunk of round-1 slot e past the window: generic chunks, then body chunks
        auto ext_k = [&](uint32_t e) -> uint32_t { return e < ne ? gen_k(e) : kb0 + (e - ne); };

        // body chunks: U per lane per round; their loads need only the copy range, not the parse
        const uint64_t skA = sk & ~3ull;
        const uint32_t b = (uint32_t)(sk & 3u);
        // the dword after a chunk's 16 source bytes holds its last b bytes; no lane of the wavefront
        // needs it when every record it holds has b == 0 (source and destination co-aligned mod 4,
        // as in C2copy), and then those loads are not issued at all
        const bool need_hi = __any(b != 0u);
        auto body_load1 = [&](uint32_t i, u32x4& lo, uint32_t& hi) {
            const bool in = i < nb;
            const uint64_t A = skA + 16ull * (kb0 + i);
            lo = ld16<F::NT_BODY_LOADS>((gcv4)(in ? A : dummy));
            hi = need_hi ? *(const GMEM uint32_t*)(in && b ? A + 16 : dummy) : 0u;
        };
        auto body_load = [&](uint32_t i0, u32x4* lo, uint32_t* hi) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t i = i0 + (uint32_t)(u * G + lane);
                const bool in = i < nb;
                const uint64_t A = skA + 16ull * (kb0 + i);
                lo[u] = ld16<F::NT_BODY_LOADS>((gcv4)(in ? A : dummy));
                // (b == 0: that dword may lie past the source range, so it is not read)
                hi[u] = need_hi ? *(const GMEM uint32_t*)(in && b ? A + 16 : dummy) : 0u;
            }
        };
        u32x4 blo[U];
        uint32_t bhi[U];
        u32x4 elo[UB > 0 ? UB : 1];
        uint32_t ehi[UB > 0 ? UB : 1];

        // ---- round 1: the window and the first generic chunks past it ----
        u32x4 gm[UW];
        {
            Gen gn[UW];
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const uint32_t j = (uint32_t)(u * G + lane);
                const bool w = j < (uint32_t)WIN_CH;
                const uint32_t k = w ? j : ext_k(j - WIN_CH);
                const bool in = w ? j < nch : j - WIN_CH < ne + body1;
                gn[u] = gen_load<F::NT_GEN_DST>(q, k, in, dummy);
            }
            if constexpr (UB > 0) {
#pragma unroll
                for (int u = 0; u < UB; ++u) body_load1((uint32_t)(u * G + lane), elo[u], ehi[u]);
            }
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const uint32_t j = (uint32_t)(u * G + lane);
                const bool w = j < (uint32_t)WIN_CH;
                const uint32_t k = w ? j : ext_k(j - WIN_CH);
                gm[u] = gen_merge(q, k, gn[u]);
                if (w && j < nch) wn[j] = gm[u];
            }
        }
        wave_lds_sync();
        const ByteReader rd{winb, q};
        {
            const Geom g0 = parse_geometry<false>(rd, rr.len, rr.kind, true);
            if (lane == 0) geo[gib] = g0;
        }
        wave_lds_sync();
        const Geom& g = geo[gib];
        const bool l4 = g.proto != P_NONE && !(g.st & SMOL_ST_MALFORMED);
        const int s1 = l4 ? (int)g.span_end : 0;
        // fields past the window stay out of the chunk stores (finish_gates writes them)
        const FarFields ff = far_fields(g, head, WIN);
        const int f0b = ff.f0, f1b = ff.f1, f2b = ff.f2;
        const bool far = ff.any();
        const int len = (int)rr.len;
        if constexpr (LBS) body_load(UB > 0 ? nbe : body1, blo, bhi);

        // ---- sum round 1; store its chunks past the window ----
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            const uint32_t j = (uint32_t)(u * G + lane);
            const bool w = j < (uint32_t)WIN_CH;
            const uint32_t k = w ? j : ext_k(j - WIN_CH);
            const bool in = w ? j < nch : j - WIN_CH < ne + body1;
            if (in) {
                const int pos = (int)(16u * k) - (int)head;
                acc = sum_chunk(gm[u], pos, s1, acc);
                if (!w) store_part((gu8)base + 16u * k, gm[u], -pos, len - pos, f0b - pos, f1b - pos, f2b - pos);
            }
        }
        // generic chunks beyond round 1 (a copy range that starts or ends far from the record's edges)
        for (uint32_t e0 = NEX; e0 < ne; e0 += G) {
            const uint32_t e = e0 + (uint32_t)lane;
            const bool in = e < ne;
            const uint32_t k = gen_k(in ? e : 0u);
            const u32x4 m = gen_merge(q, k, gen_load<F::NT_GEN_DST>(q, k, in, dummy));
            if (in) {
                const int pos = (int)(16u * k) - (int)head;
                acc = sum_chunk(m, pos, s1, acc);
                store_part((gu8)base + 16u * k, m, -pos, len - pos, f0b - pos, f1b - pos, f2b - pos);
            }
        }

        // ---- body: copy + sum ----
        auto body_proc = [&](uint32_t i, const u32x4& lo, uint32_t hi) {
            const uint32_t k = kb0 + i;
            const u32x4 m = body_shift(lo, hi, b);
            const int pos = (int)(16u * k) - (int)head;
            acc = sum_chunk(m, pos, s1, acc);
            const gu8 dst = (gu8)base + 16u * k;
            if (!far) {
                if constexpr (F::BODY_STORE == CST_WT)  // write-through non-temporal vector store
                    asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(dst), "v"(m) : "memory");
                else if constexpr (F::BODY_STORE == CST_NT) __builtin_nontemporal_store(m, (GMEM u32x4*)dst);
                else *(GMEM u32x4*)dst = m;
            } else store_part(dst, m, 0, 16, f0b - pos, f1b - pos, f2b - pos);
        };
        if constexpr (UB > 0) {
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const uint32_t i = (uint32_t)(u * G + lane);
                if (i < nbe) body_proc(i, elo[u], ehi[u]);
            }
        }
        for (uint32_t i0 = UB > 0 ? nbe : body1; i0 < nb; i0 += (uint32_t)(G * U)) {
            if (!LBS || i0 != (UB > 0 ? nbe : body1)) body_load(i0, blo, bhi);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t i = i0 + (uint32_t)(u * G + lane);
                if (i < nb) body_proc(i, blo[u], bhi[u]);
            }
        }

        // ---- finish: gates, fields into the window (or past it), then the window chunks ----
        finish_gates<G, MODE_COPY, false, ByteReader, WIN>(p, g, acc, rd, winb, head, rr.a0, r, lane,
                                                              reinterpret_cast<uint8_t*>(wn));
        wave_lds_sync();
        for (uint32_t k = (uint32_t)lane; k < (uint32_t)WIN_CH && k < nch; k += G) {
            const int pos = (int)(16u * k) - (int)head;
            store_part((gu8)base + 16u * k, wn[k], -pos, len - pos, NOF, NOF, NOF);
        }
        wave_lds_sync();  // the window is rewritten by the group's next record
    }
}

// The launch of (variant, shape): the form, the number reported and the shape all come from csum_launch.h's
// with_copy_kernel (the registry's COPY rows and with_copy_shape, where the shapes' measurements are).
hipError_t launch_copy_kernel(int shape, int var, const KParams& p, uint32_t max_blocks, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    with_copy_kernel(var, shape, [&](auto form, auto num, auto g, auto u, auto uw, auto ub) {
        using F = decltype(form);
        constexpr int G = decltype(g)::value, U = decltype(u)::value, UW = decltype(uw)::value, UB = decltype(ub)::value;
        const uint32_t blocks = grid_blocks((p.n + 256 / G - 1) / (256 / G), max_blocks);
        note_launch(KERN_COPY, decltype(num)::value, G, U);
        if (p.desc == nullptr) hipLaunchKernelGGL((copy_kernel<F, G, U, true, UW, UB>), dim3(blocks), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((copy_kernel<F, G, U, false, UW, UB>), dim3(blocks), dim3(256), 0, s, p);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace smolcsum
