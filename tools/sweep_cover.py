#!/usr/bin/env python3
"""How much vector work covers each ds_bpermute of a resident CG kernel's mat-vec?  Reads `hipcc -S` output and only counts.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -x hip elphdynamics_amd/csrc/cg_wg.hip -o cg_wg.s
    python tools/sweep_cover.py cg_wg.s [--kernel k_cg_wgILi4ELi4ELb0ELb1ELi1ELb0ELb1ELb0E]

The section looked at is the kernel's iteration from the header of its outermost loop to the first s_barrier (the mat-vec, the four
sums and the boundary stores).  LDS operations of a wave complete in order, so an `s_waitcnt lgkmcnt(N)` retires every LDS
operation but the N issued last.  ds_bpermute that are issued before any of their predecessors is retired form a GROUP; for every
wait that retires members of a group the table gives how many it retires and how many vector (v_*) instructions were issued between
the group's FIRST ds_bpermute and that wait — the cover the crossing has.  (profiles/wg_sweep_order holds the tables of the 4-slice
16 x 16 kernel before and after its sweeps were re-ordered.)
"""
import argparse
import re
import sys

HEADLINE = "k_cg_wgILi4ELi4ELb0ELb1ELi1ELb0ELb1ELb0E"


def kernel_body(lines, name):
    start = None
    for i, l in enumerate(lines):
        if start is None and re.match(r"^_Z\w*" + re.escape(name) + r"\w*:", l):
            start = i
        elif start is not None and l.startswith(".Lfunc_end"):
            return lines[start:i]
    sys.exit(f"kernel {name} not found")


def mnemonic(line):
    s = line.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None, None
    parts = s.split(None, 1)
    return parts[0], (parts[1] if len(parts) > 1 else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=HEADLINE, help="substring of the mangled kernel name")
    a = ap.parse_args()
    body = kernel_body(open(a.asm).read().splitlines(), a.kernel)
    begin = next(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    end = next(i for i in range(begin, len(body)) if mnemonic(body[i])[0] == "s_barrier")
    valu = 0
    counts = {}
    out = []                    # outstanding LGKM operations, oldest first: (kind, group or None)
    groups = []                 # {"n": members, "first": valu index of the first ds_bpermute, "waits": [(retired, cover)], "open": bool}
    for l in body[begin:end]:
        m, args = mnemonic(l)
        if m is None:
            continue
        if m.startswith("v_"):
            valu += 1
            key = "v_fma_f64" if m.startswith("v_fma") else ("v_mov_b32_dpp" if "dpp" in m or "row_" in args or "quad_perm" in args else m if m in ("v_mul_f64",) else None)
            if key:
                counts[key] = counts.get(key, 0) + 1
        elif m.startswith("ds_") or m.startswith("s_load") or m.startswith("s_buffer_load"):
            g = None
            if m.startswith("ds_bpermute"):
                if not groups or not groups[-1]["open"]:
                    groups.append({"n": 0, "first": valu, "waits": [], "open": True})
                g = groups[-1]
                g["n"] += 1
            counts[m] = counts.get(m, 0) + 1
            out.append((m, g))
        elif m == "s_waitcnt":
            w = re.search(r"lgkmcnt\((\d+)\)", args)
            if not w:
                continue
            keep = int(w.group(1))
            retired, out = out[:len(out) - keep] if keep else out, out[len(out) - keep:] if keep else []
            per = {}
            for _k, g in retired:
                if g is not None:
                    per[id(g)] = (g, per.get(id(g), (g, 0))[1] + 1)
            for g, n in per.values():
                g["waits"].append((n, valu - g["first"]))
                g["open"] = False
    print(f"# {a.kernel}: loop header .. first s_barrier")
    print(f"vector instructions {valu}: " + ", ".join(f"{v} {k}" for k, v in sorted(counts.items()) if k.startswith("v_")))
    print("LDS / scalar-memory operations: " + ", ".join(f"{v} {k}" for k, v in sorted(counts.items()) if not k.startswith("v_")))
    print("group | ds_bpermute | retired by each wait | vector instructions from the group's first ds_bpermute to that wait")
    for i, g in enumerate(groups):
        print(f"{i:5d} | {g['n']:11d} | {' + '.join(str(n) for n, _ in g['waits']):>20} | {' and '.join(str(c) for _, c in g['waits'])}")


if __name__ == "__main__":
    main()
