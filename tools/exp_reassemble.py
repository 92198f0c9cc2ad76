#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_verify_reassemble (verify fragment groups and put the datagrams together
in one pass) next to what a caller could do before it, on device-resident fragment batches at MTU 1500:
2^14 UDP datagrams of 8 KB (6 fragments each) and 2^11 of 64 KB (T = 65,515, 45 fragments each).  The
fragments lie in arrival order at a fixed stride of 1500 bytes (an RX ring; the last fragment of a datagram
is shorter, its IP total length decides); emit_frag fills their checksums first, so every group is accepted.

Lines per shape:
  (a) verify_frag                 smol_csum_batch_verify_frag alone
  (b) verify_frag_then_gather     verify_frag, then one index_select over a precomputed byte index (int32, one
                                  entry per payload byte) into a dense buffer: the one-call device gather
  (b') verify_frag_then_copies    verify_frag, then one strided device copy per fragment position (possible
                                  here because every datagram has the same layout): the cheapest gather
  (c) verify_reassemble           the fused call into dense slots

Every line is timed with device events around `--launches` back-to-back launches over `--batches` batches
taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch: the
median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's status
and delivered bytes are compared with (a) and (b) on the first batch.

    python tools/exp_reassemble.py [--configs 8k,64k] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

MTU, STEP = 1500, 1480
CONFIGS = {"8k": (1 << 14, 8192), "64k": (1 << 11, 65515)}


def fragments(nd: int, T: int, seed: int) -> np.ndarray:
    """nd UDP datagrams of T IP-payload bytes as (nd, nfrag, MTU) fragment records: checksum fields 0."""
    rng = np.random.default_rng(seed)
    nfrag = (T + STEP - 1) // STEP
    data = rng.integers(0, 256, (nd, nfrag * STEP), dtype=np.uint8)
    data[:, 0:4] = (0x12, 0x34, 0x00, 0x35)        # ports 4660 -> 53
    data[:, 4:8] = (T >> 8, T & 0xFF, 0, 0)        # UDP length, checksum 0
    recs = np.zeros((nd, nfrag, MTU), np.uint8)
    ident = np.arange(nd, dtype=np.uint32)
    for j in range(nfrag):
        plen = min(STEP, T - j * STEP)
        ff = (0x2000 if j + 1 < nfrag else 0) | (j * STEP // 8)
        recs[:, j, 0:4] = (0x45, 0, (20 + plen) >> 8, (20 + plen) & 0xFF)
        recs[:, j, 4], recs[:, j, 5] = (ident >> 8).astype(np.uint8), ident.astype(np.uint8)
        recs[:, j, 6:12] = (ff >> 8, ff & 0xFF, 64, 17, 0, 0)
        recs[:, j, 12:20] = (10, 0, 0, 1, 10, 0, 0, 2)
        recs[:, j, 20:20 + plen] = data[:, j * STEP:j * STEP + plen]
    return recs


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nd, T = CONFIGS[cfg]
    nfrag = (T + STEP - 1) // STEP
    n = nd * nfrag
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    batch = E.Batch.fixed(n, MTU, MTU, E.KIND_IP)
    groups = torch.from_numpy(E.make_groups(np.arange(nd, dtype=np.uint64) * nfrag, nfrag).view(np.uint8).copy()).to(dev)
    bufs = []
    for j in range(batches):
        b = torch.from_numpy(fragments(nd, T, 0x5EED0200 + j).reshape(-1)).to(dev)
        eng.emit_frag(b, batch, groups)
        bufs.append(b)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    dgrams = torch.empty((nd, 16), dtype=torch.uint8, device=dev)
    dst = torch.zeros(nd * T + 16, dtype=torch.uint8, device=dev)
    dense = dst[:nd * T]
    slots = torch.from_numpy(E.make_slots(np.arange(nd, dtype=np.uint64) * T, T).view(np.uint8).copy()).to(dev)
    # byte index of the gather: datagram byte t of datagram d lives at record (d, t // STEP), offset 20 + t % STEP
    t = np.arange(T, dtype=np.int64)
    within = (t // STEP) * MTU + 20 + t % STEP
    idx = (np.arange(nd, dtype=np.int64)[:, None] * (nfrag * MTU) + within[None, :]).reshape(-1)
    assert int(idx.max()) < 2 ** 31
    idx = torch.from_numpy(idx.astype(np.int32)).to(dev)

    def gather(i):
        eng.verify_frag(bufs[i], batch, groups, status=status)
        torch.index_select(bufs[i], 0, idx, out=dense)

    def copies(i):
        eng.verify_frag(bufs[i], batch, groups, status=status)
        src, out = bufs[i].view(nd, nfrag, MTU), dense.view(nd, T)
        for j in range(nfrag):
            plen = min(STEP, T - j * STEP)
            out[:, j * STEP:j * STEP + plen].copy_(src[:, j, 20:20 + plen])

    ops = {
        "verify_frag": lambda i: eng.verify_frag(bufs[i], batch, groups, status=status),
        "verify_frag_then_gather": gather,
        "verify_frag_then_copies": copies,
        "verify_reassemble": lambda i: eng.verify_reassemble(bufs[i], batch, groups, dst, slots, status=status, dgrams=dgrams),
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call against the two passes, on the first batch
    ref_st = eng.verify_frag(bufs[0], batch, groups).clone()
    ref_dense = torch.index_select(bufs[0], 0, idx)
    dst.zero_()
    st, dg = eng.verify_reassemble(bufs[0], batch, groups, dst, slots)
    launched = eng.last_launch()
    dge = dg.cpu().numpy().reshape(-1).view(E.DGRAM_DTYPE)
    check = {"status_equals_verify_frag": bool(torch.equal(st, ref_st)),
             "accepted_records": int(((st & E.ST_ACCEPT) != 0).sum()), "records": n,
             "copied": int(dge["copied"].sum()), "delivered_bytes": int(dge["len"][dge["copied"] == 1].astype(np.uint64).sum()),
             "dst_equals_gather": bool(torch.equal(dense, ref_dense))}
    copies(0)
    check["copies_equal_gather"] = bool(torch.equal(dense, ref_dense))
    del ref_dense

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    payload = nd * T
    res = {"config": cfg, "datagrams": nd, "datagram_bytes": T, "fragments_per_datagram": nfrag, "records": n,
           "payload_bytes": payload, "batches": len(bufs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}', "check": check}
    X.summarize(res, times, payload)
    X.over(res, "verify_reassemble", ("verify_frag", "verify_frag_then_gather", "verify_frag_then_copies"))
    eng.close()
    return res


def main():
    args = X.parser("8k,64k", batches=3, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
