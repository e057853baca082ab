#!/usr/bin/env python3
"""Compare two gfx950 device-assembly files (hipcc ... --offload-device-only -S) function by function -- what a refactor that must not
change a kernel is read against when byte identity is too much to ask (an extracted helper moves a few integer address instructions).

    python tools/kernel_diff.py parent/attn2.s result/attn2.s

Per function symbol (kernels and __noinline__ device functions): the count of every opcode between the symbol's label and its
.Lfunc_end, and per kernel the resource metadata (.vgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
spills).  Prints every count that differs and the change of the total in per cent.  Exit status 1 when a symbol is missing on one
side, a metadata value differs or a total moves by more than 1 %; which opcodes may move is for the reader of the output to judge."""
import collections
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def parse(path):
    ops, meta, cur, block = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = ops.setdefault(m.group(1), collections.Counter())
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and (m := re.match(r"^\t([a-z]\w*)", line)):
            cur[m.group(1)] += 1
        # amdhsa.kernels: one list item per kernel, "  - .key: value" then "    .key: value" lines with the keys in alphabetical order
        # (.symbol before .vgpr_count); an item ends where the next begins or the list ends.  Nested items (.args) are indented deeper.
        elif line.startswith("  - ."):
            block = {}
            meta[len(meta)] = block                            # keyed by position until the item's .symbol is read
        elif block is not None and not line.startswith("    "):
            block = None
        if block is not None and (m := re.match(r"^  [ -] (\.\w+):\s+(\S+)\s*$", line)):
            if m.group(1) in META:
                block[m.group(1)] = int(m.group(2))
            elif m.group(1) == ".symbol":
                block[".symbol"] = m.group(2)
    meta = {b.pop(".symbol")[:-3]: b for b in meta.values() if ".symbol" in b}
    return {k: v for k, v in ops.items() if v}, meta


def main(a, b):
    (opa, ma), (opb, mb) = parse(a), parse(b)
    bad = False
    for sym in sorted(set(opa) | set(opb)):
        if sym not in opa or sym not in opb:
            print("%s: only in %s" % (sym, a if sym in opa else b))
            bad = True
            continue
        ca, cb = opa[sym], opb[sym]
        na, nb = sum(ca.values()), sum(cb.values())
        if sym in ma and (sym not in mb or set(ma[sym]) != set(mb[sym]) or not set(META[:2]) <= set(ma[sym])):
            print("%s: metadata block missing or incomplete" % sym)
            bad = True
        dm = ["  %s %d -> %d" % (k, v, mb.get(sym, {}).get(k, -1)) for k, v in ma.get(sym, {}).items() if v != mb.get(sym, {}).get(k)]
        do = ["  %s %d -> %d" % (op, ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]]
        over = abs(nb - na) > 0.01 * na
        print("%s: %d -> %d instructions (%+.2f %%)%s%s" % (sym, na, nb, 100.0 * (nb - na) / na, ", same counts per opcode" if not do else "",
                                                          ", metadata equal" if sym in ma and not dm else ""))
        if dm or do:
            print("\n".join(dm + do))
        bad = bad or bool(dm) or over
    print("DIFFERENT: metadata or a total beyond 1 %" if bad else "metadata equal, totals within 1 %")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
