#!/usr/bin/env python3
"""Digest of an AMDGPU assembly file (hipcc --cuda-device-only -S): one JSON line per kernel with its
demangled name, a hash of its body with symbol names normalised, and its .amdhsa_ descriptor values.

Two builds of a translation unit have the same machine code when their digests pair up kernel by
kernel: a refactor that renames templates or reorders instantiations changes the names and the order,
not the hashes.  The tool hashes and counts; it looks for no instruction.

    make -C smoltcp_amd/csrc asm ASM_SRC=csum_walk_emit_fixed.hip     # writes /tmp/csum_walk.s
    python tools/kernel_asm_digest.py /tmp/csum_walk.s > after.jsonl
    python tools/kernel_asm_digest.py --diff before.jsonl after.jsonl  # pairs by name, else by hash
"""
import argparse
import collections
import hashlib
import json
import re
import shutil
import subprocess
import sys

# what the comparison reports by name; the hash of the whole block covers the rest
DESC_KEYS = {"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "accum_offset": "accum_offset",
             "group_segment_fixed_size": "lds", "private_segment_fixed_size": "scratch"}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return dict(zip(names, names))
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def normalise(line, symbols):
    line = line.split(";", 1)[0].rstrip()  # comments carry names and block numbers
    line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?", lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""), line)
    return symbols.sub("SYM", line)


def digest(path):
    with open(path) as f:
        lines = f.read().splitlines()
    kernels = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    # every mangled name: a body may mention another function or a variable
    symbols = re.compile(r"\b_Z\w+")
    bodies, descs, cur, cur_desc = {}, {}, None, None
    for ln in lines:
        m = re.match(r"(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in kernels and cur is None:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is not None:
            if re.match(r"\s*\.Lfunc_end\d+:", ln) or re.match(r"\s*\.section\b", ln):
                cur = None
                continue
            text = normalise(ln, symbols)
            if text.strip():
                bodies[cur].append(text)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur_desc = m.group(1)
            descs[cur_desc] = []
        elif re.match(r"\s*\.end_amdhsa_kernel", ln):
            cur_desc = None
        elif cur_desc is not None:
            descs[cur_desc].append(normalise(ln, symbols).strip())
    names = demangle(kernels)
    rows = []
    for k in kernels:
        d = {}
        for ln in descs[k]:
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", ln)
            if m and m.group(1) in DESC_KEYS:
                d[DESC_KEYS[m.group(1)]] = m.group(2)
        rows.append({"kernel": names[k], "lines": len(bodies.get(k, [])),
                     "body": hashlib.sha256("\n".join(bodies.get(k, [])).encode()).hexdigest()[:16],
                     "desc": d, "desc_hash": hashlib.sha256("\n".join(descs[k]).encode()).hexdigest()[:16]})
    return rows


def diff(a_path, b_path):
    """Pairs the kernels of two digests by name; those whose names differ (a renamed template), by
    (body, descriptor).  Prints what is left unpaired on either side."""
    load = lambda p: [json.loads(ln) for ln in open(p) if ln.strip()]
    a, b = load(a_path), load(b_path)
    key = lambda r: (r["body"], r["desc_hash"])
    b_by_name = {r["kernel"]: r for r in b}
    same = changed = 0
    rest_a = []
    for r in a:
        o = b_by_name.pop(r["kernel"], None)
        if o is None:
            rest_a.append(r)
        elif key(o) == key(r):
            same += 1
        else:
            changed += 1
            print("CHANGED %s: %s -> %s" % (r["kernel"], r["desc"], o["desc"]))
    pool = collections.Counter(key(r) for r in b_by_name.values())
    for r in rest_a:
        if pool[key(r)]:
            pool[key(r)] -= 1
            same += 1
        else:
            changed += 1
            print("UNPAIRED before: %s" % r["kernel"])
    extra = sum(pool.values())
    print("%d kernels before, %d after: %d identical, %d changed or unpaired, %d only after" %
          (len(a), len(b), same, changed, extra))
    return 0 if not changed and not extra and len(a) == len(b) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--diff", action="store_true", help="compare two digests instead of making one")
    ap.add_argument("paths", nargs="+")
    args = ap.parse_args()
    if args.diff:
        if len(args.paths) != 2:
            ap.error("--diff takes two digest files")
        return diff(*args.paths)
    for p in args.paths:
        for row in digest(p):
            print(json.dumps(row, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
