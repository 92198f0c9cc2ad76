#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_fragment_emit (emit whole IPv4 datagrams and cut them into the iface's
frames in one pass) next to what a caller could do before it, on device-resident UDP datagrams at a fixed
stride: 2^14 of 8 KB at MTU 1500 (6 frames each), 2^11 of 64 KB (T = 65,515, 45 frames each) at MTU 1500,
and 2^16 of 1500 B at MTU 576 (3 frames each).  The frames go to a TX ring at a fixed stride of ip_mtu bytes
per frame (a datagram's last frame is shorter; the bytes behind it are not written).

Lines per shape:
  (a) emit                 smol_csum_batch_emit on the whole datagrams alone (in place)
  (b) emit_then_copies     emit, then one strided device copy per fragment position into the frame layout
                           plus one for the headers, which the host precomputed (lengths, ident, flags,
                           offsets, header checksums): the cheapest gather a caller can do today
  (c) fragment_emit        the fused call

Every line is timed with device events around `--launches` back-to-back launches over `--batches` batches
taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch: the
median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's frames
are compared with (b)'s on the first batch.

    python tools/exp_fragment.py [--configs 8k,64k,1500] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

CONFIGS = {"8k": (1 << 14, 8192, 1500), "64k": (1 << 11, 65515, 1500), "1500": (1 << 16, 1480, 576)}


def datagrams(nd: int, T: int, seed: int) -> np.ndarray:
    """nd UDP datagrams of T IP-payload bytes as (nd, 20 + T) records: DF set, checksum fields 0."""
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 256, (nd, 20 + T), dtype=np.uint8)
    ident = np.arange(nd, dtype=np.uint32) * 7
    recs[:, 0:4] = (0x45, 0, (20 + T) >> 8, (20 + T) & 0xFF)
    recs[:, 4], recs[:, 5] = (ident >> 8).astype(np.uint8), ident.astype(np.uint8)
    recs[:, 6:12] = (0x40, 0, 64, 17, 0, 0)
    recs[:, 12:20] = (10, 0, 0, 1, 10, 0, 0, 2)
    recs[:, 20:24] = (0x12, 0x34, 0x00, 0x35)      # ports 4660 -> 53
    recs[:, 24:28] = (T >> 8, T & 0xFF, 0, 0)      # UDP length, checksum 0
    return recs


def frame_headers(nd: int, T: int, step: int, idents: np.ndarray) -> np.ndarray:
    """The (nd, nfrag, 20) IPv4 headers of the frames, header checksums filled (dispatch_ipv4_frag's)."""
    nfrag = (T + step - 1) // step
    h = np.zeros((nd, nfrag, 20), np.uint8)
    for j in range(nfrag):
        plen = min(step, T - j * step)
        ff = (0x2000 if j + 1 < nfrag else 0) | (j * step // 8)
        h[:, j, 0:4] = (0x45, 0, (20 + plen) >> 8, (20 + plen) & 0xFF)
        h[:, j, 4], h[:, j, 5] = (idents >> 8).astype(np.uint8), idents.astype(np.uint8)
        h[:, j, 6:12] = (ff >> 8, ff & 0xFF, 64, 17, 0, 0)
        h[:, j, 12:20] = (10, 0, 0, 1, 10, 0, 0, 2)
    s = h.reshape(nd, nfrag, 10, 2).astype(np.uint32)
    s = (s[..., 0] << 8 | s[..., 1]).sum(axis=2)
    s = (s >> 16) + (s & 0xFFFF)
    s = ~((s >> 16) + s) & 0xFFFF
    h[:, :, 10], h[:, :, 11] = (s >> 8).astype(np.uint8), s.astype(np.uint8)
    return h


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nd, T, mtu = CONFIGS[cfg]
    step = (mtu - 20) - (mtu - 20) % 8
    assert 20 + T > mtu
    nfrag = (T + step - 1) // step
    rlen = 20 + T
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    batch = E.Batch.fixed(nd, rlen, rlen, E.KIND_IP)
    bufs = [torch.from_numpy(datagrams(nd, T, 0x5EED0300 + j).reshape(-1)).to(dev) for j in range(batches)]
    idents = (np.arange(nd, dtype=np.uint32) * 3 + 1) & 0xFFFF
    hdrs = torch.from_numpy(frame_headers(nd, T, step, idents)).to(dev)
    ring = torch.zeros(nd * nfrag * mtu, dtype=torch.uint8, device=dev)    # (b)'s frames
    fused = torch.zeros(nd * nfrag * mtu, dtype=torch.uint8, device=dev)   # (c)'s frames
    plans = torch.from_numpy(E.make_fragplans(np.arange(nd, dtype=np.uint64) * (nfrag * mtu), nfrag * mtu, mtu,
                                              idents).view(np.uint8).copy()).to(dev)
    out = torch.empty((nd, 16), dtype=torch.uint8, device=dev)

    def copies(i):
        eng.emit(bufs[i], batch)
        src, dstv = bufs[i].view(nd, rlen), ring.view(nd, nfrag, mtu)
        dstv[:, :, :20].copy_(hdrs)
        for j in range(nfrag):
            plen = min(step, T - j * step)
            dstv[:, j, 20:20 + plen].copy_(src[:, 20 + j * step:20 + j * step + plen])

    ops = {
        "emit": lambda i: eng.emit(bufs[i], batch),
        "emit_then_copies": copies,
        "fragment_emit": lambda i: eng.fragment_emit(bufs[i], batch, fused, plans, frame_stride=mtu, out=out),
    }
    X.warm_up(ops, len(bufs))

    # results must not change: the fused call's frames against emit + copies, on the first batch
    fused.zero_()
    ring.zero_()
    eng.fragment_emit(bufs[0], batch, fused, plans, frame_stride=mtu, out=out)
    launched = eng.last_launch()
    copies(0)
    oe = out.cpu().numpy().reshape(-1).view(E.FRAGOUT_DTYPE)
    check = {"frames_equal_emit_then_copies": bool(torch.equal(fused, ring)), "datagrams": nd,
             "written": int(oe["written"].sum()), "frames": int(oe["count"].astype(np.uint64).sum()),
             "status_zero": bool((oe["status"] == 0).all())}

    times = X.time_interleaved(ops, len(bufs), launches, rounds)
    payload = nd * T
    res = {"config": cfg, "datagrams": nd, "datagram_bytes": T, "ip_mtu": mtu, "frames_per_datagram": nfrag,
           "payload_bytes": payload, "batches": len(bufs), "launches_per_round": launches, "rounds": rounds,
           "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}', "check": check}
    X.summarize(res, times, payload)
    X.over(res, "fragment_emit", ("emit", "emit_then_copies"))
    eng.close()
    return res


def main():
    args = X.parser("8k,64k,1500", batches=3, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
