#!/usr/bin/env python3
"""Kernel time of smol_csum_batch_tcp_segment_emit (one header template and one payload range per send, cut
into MSS-sized segments with every checksum filled in one pass) next to what a caller could do before it, on
device-resident data: 2^14 sends of 64 KiB at mss 1460 (45 segments each), 2^16 sends of 8 KiB at mss 1460
(6 each) and 2^18 sends of 1460 B at mss 536 (3 each).  Templates are Ethernet + IPv4 + a 20-byte TCP header
(hl = 54) at a fixed stride of 64; the frames go to a TX ring at a fixed stride of hl + mss bytes per frame (a
send's last frame is shorter; the bytes behind it are not written).

Lines per shape:
  (a) copy_emit            smol_csum_batch_copy_emit over the same frames as a fixed-stride batch, one copy
                           descriptor per segment, the host-built headers already resident in the ring: the
                           caller's route before this call, minus its header build and upload
  (b) device_copy          one contiguous device copy of the same payload bytes: the floor
  (c) tcp_segment_emit     the fused call

Every line is timed with device events around `--launches` back-to-back launches over `--batches` payload
buffers taken in turn, `--rounds` times, the lines interleaved round by round on one box; reported per launch:
the median round, the fastest and the slowest.  Ratios are medians'.  Before the timing the fused call's
frames are compared with (a)'s on the first batch.

    python tools/exp_tcp_segment.py [--configs 64k,8k,1460] [--out FILE]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import exp_common as X  # noqa: E402  (beside this script)

CONFIGS = {"64k": (1 << 14, 65536, 1460), "8k": (1 << 16, 8192, 1460), "1460": (1 << 18, 1460, 536)}
HL, TSTRIDE = 54, 64


def templates(nd: int, seed: int) -> np.ndarray:
    """nd header templates as (nd, TSTRIDE) records: Ethernet, IPv4 (ident 0, DF), TCP with ACK | PSH, a random
    sequence number, checksum fields 0, no payload."""
    rng = np.random.default_rng(seed)
    t = np.zeros((nd, TSTRIDE), np.uint8)
    t[:, 0:14] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 0x08, 0x00)
    t[:, 14:26] = (0x45, 0, 0, 40, 0, 0, 0x40, 0, 64, 6, 0, 0)
    t[:, 26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    t[:, 34:38] = (0x0F, 0xA1, 0x00, 0x50)  # ports 4001 -> 80
    t[:, 38:46] = rng.integers(0, 256, (nd, 8), dtype=np.uint8)  # sequence and ack numbers
    t[:, 46:50] = (0x50, 0x18, 0x20, 0x00)
    return t


def frame_headers(tmpl: np.ndarray, L: int, mss: int):
    """The (nd, count, HL) headers a host builds for copy_emit (length, sequence number, PSH rewritten; the
    checksum fields 0, copy_emit fills them) and the (count,) payload lengths."""
    nd = tmpl.shape[0]
    count = -(-L // mss)
    pk = np.minimum(mss, L - np.arange(count) * mss).astype(np.uint32)
    h = np.repeat(tmpl[:, None, :HL], count, axis=1)
    tl = 40 + pk
    h[:, :, 16], h[:, :, 17] = (tl >> 8).astype(np.uint8), tl.astype(np.uint8)
    seq0 = tmpl[:, 38:42].astype(np.uint32)
    seq0 = seq0[:, 0] << 24 | seq0[:, 1] << 16 | seq0[:, 2] << 8 | seq0[:, 3]
    seq = seq0[:, None] + (np.arange(count, dtype=np.uint32) * np.uint32(mss))[None, :]
    for b in range(4):
        h[:, :, 38 + b] = (seq >> (24 - 8 * b)).astype(np.uint8)
    h[:, :-1, 47] &= 0xF6  # FIN, PSH: on the last frame only
    return h, pk


def run(cfg: str, batches: int, launches: int, rounds: int, device: int = 0) -> dict:
    import torch

    from smoltcp_amd import engine as E

    nd, L, mss = CONFIGS[cfg]
    count = -(-L // mss)
    S = HL + mss
    nf = nd * count
    dev = torch.device("cuda", device)
    eng = E.ChecksumEngine(device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED0400)
    srcs = [torch.randint(0, 256, (nd * L,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(batches)]
    tmpl = templates(nd, 0x5EED0401)
    tbuf = torch.from_numpy(tmpl.reshape(-1)).to(dev)
    tbatch = E.Batch.fixed(nd, TSTRIDE, TSTRIDE, E.KIND_ETH)
    hdrs, pk = frame_headers(tmpl, L, mss)
    ring = torch.zeros(nf * S, dtype=torch.uint8, device=dev)    # (a)'s frames, the headers resident
    ring.view(nd, count, S)[:, :, :HL].copy_(torch.from_numpy(hdrs).to(dev))
    del hdrs
    fused = torch.zeros(nf * S, dtype=torch.uint8, device=dev)   # (c)'s frames
    flat = torch.empty(nd * L, dtype=torch.uint8, device=dev)    # (b)'s destination
    so = (np.arange(nd, dtype=np.uint64) * L)[:, None] + (np.arange(count, dtype=np.uint64) * mss)[None, :]
    copies = torch.from_numpy(E.make_copies(so.reshape(-1), HL, np.tile(pk, nd)).view(np.uint8).copy()).to(dev)
    fbatch = E.Batch.fixed(nf, S, S, E.KIND_ETH)
    plans = torch.from_numpy(E.make_tcpplans(np.arange(nd, dtype=np.uint64) * L, L, mss,
                                             np.arange(nd, dtype=np.uint64) * (count * S), count * S).view(np.uint8).copy()).to(dev)
    out = torch.empty((nd, 16), dtype=torch.uint8, device=dev)

    ops = {
        "copy_emit": lambda i: eng.copy_emit(ring, fbatch, srcs[i], copies),
        "device_copy": lambda i: flat.copy_(srcs[i]),
        "tcp_segment_emit": lambda i: eng.tcp_segment_emit(tbuf, tbatch, srcs[i], fused, plans, frame_stride=S, out=out),
    }
    X.warm_up(ops, len(srcs))

    # results must not change: the fused call's frames against copy_emit's, on the first batch
    eng.copy_emit(ring, fbatch, srcs[0], copies)
    route = eng.last_launch()
    eng.tcp_segment_emit(tbuf, tbatch, srcs[0], fused, plans, frame_stride=S, out=out)
    launched = eng.last_launch()
    oe = out.cpu().numpy().reshape(-1).view(E.TCPOUT_DTYPE)
    st = eng.verify(fused, fbatch)
    check = {"frames_equal_copy_emit": bool(torch.equal(fused, ring)), "sends": nd, "written": int(oe["written"].sum()),
             "frames": int(oe["count"].astype(np.uint64).sum()), "status_zero": bool((oe["status"] == 0).all()),
             "verify_accepts_all": bool((st & E.ST_ACCEPT).all())}

    times = X.time_interleaved(ops, len(srcs), launches, rounds)
    payload = nd * L
    res = {"config": cfg, "sends": nd, "send_bytes": L, "mss": mss, "frames_per_send": count, "header_bytes": HL,
           "frame_stride": S, "payload_bytes": payload, "batches": len(srcs), "launches_per_round": launches,
           "rounds": rounds, "kernel": f'{launched["kernel"]} {launched["G"]}x{launched["U"]}',
           "copy_emit_kernel": f'{route["kernel"]} v{route["variant"]} {route["G"]}x{route["U"]}', "check": check}
    X.summarize(res, times, payload)
    X.over(res, "tcp_segment_emit", ("copy_emit", "device_copy"))
    eng.close()
    return res


def main():
    args = X.parser("64k,8k,1460", batches=2, launches=8).parse_args()
    X.run_configs(args, lambda c: run(c, args.batches, args.launches, args.rounds))


if __name__ == "__main__":
    main()
