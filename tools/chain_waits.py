#!/usr/bin/env python3
"""Exposed LDS waits and register copies in the loop of a resident CG kernel: reads `hipcc -S` output of cg_wg.hip and only counts. For every `s_waitcnt lgkmcnt(N)` inside the kernel's outermost loop that retires at least one LDS / scalar-memory operation, the vector (v_*) instructions issued since the LAST such operation was issued; a wait with fewer than --cover (8) of them exposes most of a round trip. Listed by section of the iteration (between the loop header and the s_barriers), with the loop's v_mov_b64 (copies that compute nothing). Straight-line count over the loop's text: side paths (second meeting, poll loops, the exact stop test) are listed under their section too.
usage: python3 tools/chain_waits.py cg_wg.s [--kernel <substring of the mangled name>] [--cover 8]"""
import argparse
import re
import sys

HEADLINE = "k_cg_wgILi4ELi4ELb0ELb1ELi1ELb0ELb1ELb0E"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=HEADLINE, help="substring of the mangled kernel name")
    ap.add_argument("--cover", type=int, default=8)
    a = ap.parse_args()
    lines = open(a.asm).read().splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(a.kernel) + r"\w*:", l)), None)
    if start is None:
        sys.exit(f"kernel {a.kernel} not found")
    body = lines[start:next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))]
    hdr = next(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    label = body[hdr].split(":")[0].strip()
    # the loop's blocks, as the compiler's comments mark them (a block may be laid out in front of the header): text order from the first to the last
    tag = re.compile(r"(Header=|Parent Loop )" + re.escape(label.lstrip(".L")) + r"\b")
    blocks = [i for i, l in enumerate(body) if re.match(r"^\.LBB\w+:", l)]
    mine = [i for i in blocks if i == hdr or tag.search(body[i]) or any(tag.search(body[k]) for k in range(i + 1, min(i + 8, len(body))) if body[k].lstrip().startswith(";"))]
    first, last = min(mine), max(mine)
    last = next((i for i in blocks if i > last), len(body)) - 1
    section, valu_since, outstanding, nvalu = 0, 0, 0, 0
    movs, exposed, per_section = 0, [], {}
    for i in range(first, last + 1):
        s = body[i].split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        m, _, args = s.partition(" ")
        if m.startswith("v_"):
            valu_since += 1
            nvalu += 1
            movs += m.startswith("v_mov_b64")
        elif m.startswith("ds_") or m.startswith("s_load") or m.startswith("s_buffer_load"):
            outstanding += 1
            valu_since = 0
        elif m == "s_barrier":
            section += 1
        elif m == "s_waitcnt":
            w = re.search(r"lgkmcnt\((\d+)\)", args)
            if w and outstanding > int(w.group(1)):
                outstanding = int(w.group(1))
                if valu_since < a.cover:
                    exposed.append((i - first, section, valu_since, s))
                    per_section[section] = per_section.get(section, 0) + 1
    print(f"# {a.kernel}: loop {label}, {last - first + 1} lines, {nvalu} vector instructions, {movs} v_mov_b64")
    print(f"waits that retire LDS / scalar-memory operations with fewer than {a.cover} vector instructions since the last one was issued: {len(exposed)}")
    print("by section (0: loop header .. first s_barrier, k: behind the k-th s_barrier in text order): " + ", ".join(f"{k}: {v}" for k, v in sorted(per_section.items())))
    print("line in loop | section | vector instructions of cover | wait")
    for e in exposed:
        print(f"{e[0]:12d} | {e[1]:7d} | {e[2]:28d} | {e[3]}")


if __name__ == "__main__":
    main()
