#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_copy (verify and deliver the L4 payloads in one pass) next to the
two-pass route it replaces, on bench.py's device-resident shapes: C2 (2^20 x 1500 B IPv4/UDP, fixed
stride), C4 (2^20 x 1320 B IPv6 mix, fixed stride) and C3 (2^20 IPv4/TCP segments of U[64, 9000] B, packed,
descriptors).

Lines per shape:
  (a) verify              smol_csum_batch_verify alone
  (b) verify_then_copy    verify, then a strided device copy of the payloads into a dense buffer
                          (dst.view(n, plen).copy_(buf.view(n, stride)[:, off:off + plen])): the route there
                          was before verify_copy.  C4's records mix UDP and TCP over IPv6; the copy takes the UDP
                          span (off 48, 1272 B) of every record, which moves the same bytes to within 1 %.
  (c) copy_emit           smol_csum_batch_copy_emit of the same payload span from a packed source: the
                          transmit side's fused kernel, as the mirror-image reference point (its own buffers)
  (d) verify_copy_*       the fused call into dense slots, with plain (the library's choice) and non-temporal (nt) body stores, at
                          the library's launch shape and at each shape of --shapes
C3 has no one-line two-pass equivalent: verify and verify_copy only, absolute time and bytes/s.

Every line is timed with device events around `--launches` back-to-back launches over `--batches` batches
taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch: the
median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's
status and delivered bytes are compared with the two-pass route's on the first batch.

    python tools/exp_verify_copy.py [--configs c2,c4,c3] [--records N] [--shapes 8] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

SHAPE_NAMES = {-1: "auto", 0: "8x6", 1: "16x3", 4: "32x4", 6: "64x4", 7: "8x7", 8: "16x4"}


def run(cfg: str, n: int, batches: int, launches: int, rounds: int, shapes, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    fixed = cfg != "c3"
    if fixed:
        L, profile, off = (1500, E.SYNTH_UDP4, 28) if cfg == "c2" else (1320, E.SYNTH_V6MIX, 48)
        plen = L - off
        batch = E.Batch.fixed(n, L, L, E.KIND_IP)
        total = read = n * L
        d_offs, d_caps = np.arange(n, dtype=np.uint64) * plen, plen
        dst_bytes = n * plen
    else:
        rng = np.random.default_rng(0x5EED0002)
        lens = rng.integers(64, 9001, n).astype(np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        batch = E.Batch.from_records(offs, lens, E.KIND_IP, dev)
        total, profile = int(offs[-1] + lens[-1]) + 16, E.SYNTH_TCP4
        read = int(lens.astype(np.uint64).sum())
        d_caps = lens - 40  # dense slots: everything after the 20-byte IPv4 and TCP headers
        d_offs = np.zeros(n, dtype=np.uint64)
        d_offs[1:] = np.cumsum(d_caps[:-1].astype(np.uint64))
        dst_bytes = int(d_caps.astype(np.uint64).sum())
    bufs = []
    for j in range(batches):
        b = torch.empty(total, dtype=torch.uint8, device=dev)
        eng.synth(b, batch, profile, 0x5EED0100 + j)
        bufs.append(b)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    spans = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    dst = torch.zeros(dst_bytes + 16, dtype=torch.uint8, device=dev)
    slots = torch.from_numpy(E.make_slots(d_offs, d_caps).view(np.uint8).copy()).to(dev)

    def vcopy_op(nt, shape):
        def op(i):
            eng.set_vcopy_stores(nt)
            eng.set_shape(shape)
            eng.verify_copy(bufs[i], batch, dst, slots, status=status, spans=spans)
            eng.set_shape(-1)
            eng.set_vcopy_stores(False)
        return op

    ops = {"verify": lambda i: eng.verify(bufs[i], batch, status=status)}
    if fixed:
        dense = dst[:dst_bytes].view(n, plen)

        def two_pass(i):
            eng.verify(bufs[i], batch, status=status)
            dense.copy_(bufs[i].view(n, L)[:, off:off + plen])

        ops["verify_then_copy"] = two_pass
        txs = [b.clone() for b in bufs]  # copy_emit writes its batch: buffers of its own
        src = torch.randint(0, 256, (n * plen + 16,), dtype=torch.uint8, device=dev)
        copies = torch.from_numpy(E.make_copies(np.arange(n, dtype=np.uint64) * plen, off, plen).view(np.uint8).copy()).to(dev)
        ops["copy_emit"] = lambda i: eng.copy_emit(txs[i], batch, src, copies)
    for shape in [-1] + [s for s in shapes if s != -1]:
        for nt in (False, True):
            ops[f"verify_copy_{'nt' if nt else 'plain'}_{SHAPE_NAMES.get(shape, shape)}"] = vcopy_op(nt, shape)

    launched = {}

    def note(name):
        ll = eng.last_launch()
        launched[name] = f'{ll["kernel"]}/{ll["variant"]} {ll["G"]}x{ll["U"]}'

    X.warm_up(ops, len(bufs), after=note)

    # results must not change: the fused call against the two passes, on the first batch
    ref_st = eng.verify(bufs[0], batch).clone()
    dst.zero_()
    st, sp = eng.verify_copy(bufs[0], batch, dst, slots)
    spn = sp.cpu().numpy().reshape(-1).view(E.SPAN_DTYPE)
    check = {"status_equals_verify": bool(torch.equal(st, ref_st)), "records_with_a_span": int((spn["off"] != 0).sum()),
             "copied": int(spn["copied"].sum()), "delivered_bytes": int(spn["len"][spn["copied"] == 1].astype(np.uint64).sum())}
    if cfg == "c2":
        check["dst_equals_strided_copy"] = bool(torch.equal(dst[:dst_bytes].view(n, plen), bufs[0].view(n, L)[:, off:off + plen]))
    else:  # every copied payload against its record's bytes, on a sample
        hb, hd = bufs[0].cpu().numpy(), dst.cpu().numpy()
        rec_offs = np.arange(n, dtype=np.uint64) * L if fixed else offs
        ok = True
        for i in range(0, n, max(1, n // 4096)):
            if spn["copied"][i]:
                a, o, ln = int(rec_offs[i]) + int(spn["off"][i]), int(d_offs[i]), int(spn["len"][i])
                ok = ok and bool(np.array_equal(hd[o:o + ln], hb[a:a + ln]))
        check["sampled_payloads_equal_records"] = ok
        del hb, hd

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    res = {"config": cfg, "records": n, "read_bytes": read, "delivered_bytes": check["delivered_bytes"],
           "batches": len(bufs), "launches_per_round": launches, "rounds": rounds, "kernels": launched, "check": check}
    X.summarize(res, times, read, "read_GBs")
    if fixed:
        for name in ops:
            if name.startswith("verify_copy_"):
                res[name]["over_two_passes"] = round(res[name]["ms"] / res["verify_then_copy"]["ms"], 3)
    eng.close()
    return res


def main():
    ap = X.parser("c2,c4,c3", batches=4, launches=16)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--shapes", default="8", help="comma-separated launch shapes (CFG_*) besides the library's choice")
    args = ap.parse_args()
    shapes = [int(x) for x in args.shapes.split(",") if x]
    X.run_configs(args, lambda c: run(c, args.records, args.batches, args.launches, args.rounds, shapes))


if __name__ == "__main__":
    main()
