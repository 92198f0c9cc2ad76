"""What the exp_*.py tools that time a fused call next to a caller's other routes share: the interleaved
event-timing loop (its method: each tool's docstring), the per-line summary and the command line."""
from __future__ import annotations

import argparse
import json
import statistics


def warm_up(ops: dict, nbatches: int, after=None):
    """Every kernel loaded, every batch touched; after(name), if given, runs behind each line's calls."""
    import torch

    for name, op in ops.items():
        for i in range(nbatches):
            op(i)
        if after is not None:
            after(name)
    torch.cuda.synchronize()


def time_interleaved(ops: dict, nbatches: int, launches: int, rounds: int) -> dict:
    """ops: name -> op(i), one launch on batch i.  Returns name -> the rounds' milliseconds per launch."""
    import torch

    times = {name: [] for name in ops}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, op in ops.items():
            e0.record()
            for i in range(launches):
                op(i % nbatches)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / launches)
    return times


def summarize(res: dict, times: dict, nbytes: int, rate_key: str = "payload_GBs") -> dict:
    """res[name] = median / min / max ms and nbytes per median as GB/s under rate_key, for every line."""
    for name, tt in times.items():
        med = statistics.median(tt)
        res[name] = {"ms": round(med, 4), "min_ms": round(min(tt), 4), "max_ms": round(max(tt), 4),
                     rate_key: round(nbytes / med / 1e6, 1)}
    return res


def over(res: dict, line: str, bases) -> None:
    """res[line]["over_" + base]: the ratio of the medians, for every base line."""
    for base in bases:
        res[line]["over_" + base] = round(res[line]["ms"] / res[base]["ms"], 3)


def parser(configs: str, batches: int, launches: int, rounds: int = 7) -> argparse.ArgumentParser:
    """--configs / --batches / --launches / --rounds / --out with the tool's defaults; a tool adds its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=configs)
    ap.add_argument("--batches", type=int, default=batches)
    ap.add_argument("--launches", type=int, default=launches)
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--out", default=None)
    return ap


def run_configs(args, run) -> None:
    """run(config) for every config of args.configs: each result printed on a line of its own as soon as it is
    there, then the list printed as indented JSON and written to args.out."""
    out = []
    for c in args.configs.split(","):
        out.append(run(c))
        print(json.dumps(out[-1]), flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
