#!/usr/bin/env python3
"""Two reports on the gfx950 assembly of pair_kslice.hip (hipcc -S --cuda-device-only).

One listing: where do a pair kernel's scratch (private-memory) accesses sit?  Per kernel, the basic blocks that
hold the tile walk's VALU work (v_bitop3 count) with the scratch loads / stores inside them: spills INSIDE a hot
block cost every chunk, spills outside cost once per k-mer length or per workgroup.

Two listings (before, after): did a source change move the compiler?  Per kernel, the five resource fields of the
code object's metadata side by side, whether the instruction streams are identical, the differences in per-opcode
counts grouped by prefix (v_, ds_, global_, scratch_, buffer_, everything else as "other"), and whether every hot
block (>= 100 v_bitop3) has the same opcode sequence.  Exit status 1 if a resource field, a hot block or a
non-"other" count differs in any kernel.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I../../include -S --cuda-device-only pair_kslice.hip -o /tmp/kslice.s
    python scripts/isa_scratch_report.py /tmp/kslice.s
    python scripts/isa_scratch_report.py /tmp/kslice_before.s /tmp/kslice.s
"""
import collections
import re
import sys

KERNEL = r"_ZN3skl\w*pair_kernel\w*"
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count")
PREFIXES = ("v_", "ds_", "global_", "scratch_", "buffer_")
HOT = 100   # v_bitop3 per basic block


def kernels(path):
    """{kernel: (blocks, resources)}: blocks = [(label, lines)] of the body, resources = {field: value}."""
    text = open(path).read()
    out = collections.OrderedDict()
    for f in re.split(r"\n(?=%s:)" % KERNEL, text):
        m = re.match(r"(%s):" % KERNEL, f)
        if not m:
            continue
        body = f.split(".Lfunc_end")[0]
        blocks, cur, label = [], [], "entry"
        for line in body.split("\n")[1:]:
            if re.match(r"^\.LBB\d+_\d+:", line):
                blocks.append((label, cur))
                cur, label = [], line.split(":")[0]
            else:
                cur.append(line)
        blocks.append((label, cur))
        out[m.group(1)] = (blocks, {})
    for item in text.split("\n  - "):   # the entries of amdhsa.kernels
        m = re.search(r"^\s*\.name:\s*(%s)\s*$" % KERNEL, item, re.M)
        if m and m.group(1) in out:
            for field in FIELDS:
                v = re.search(r"^\s*%s:\s*(\d+)\s*$" % re.escape(field), item, re.M)
                out[m.group(1)][1][field] = int(v.group(1)) if v else None
    return out


def instructions(lines):
    """The instructions of a block, comments and directives dropped, blanks squeezed."""
    out = []
    for line in lines:
        s = " ".join(line.split(";")[0].split())
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(s)
    return out


def hot_blocks(blocks):
    return [(lab, b) for lab, b in blocks if sum("v_bitop3" in l for l in b) >= HOT]


def scratch_report(path):
    for name, (blocks, _) in kernels(path).items():
        total = sum("scratch_" in l for _, b in blocks for l in b)
        hot = [(lab, sum("v_bitop3" in l for l in b), sum("scratch_load" in l for l in b), sum("scratch_store" in l for l in b))
               for lab, b in hot_blocks(blocks)]
        in_hot = sum(h[2] + h[3] for h in hot)
        print(f"{name}: {total} scratch instructions, {in_hot} of them inside the {len(hot)} blocks that hold the walk")
        for lab, nb, nl, ns in hot:
            if nl + ns:
                print(f"    {lab}: {nb} v_bitop3, {nl} scratch loads, {ns} scratch stores")


def group(opcode):
    return next((p for p in PREFIXES if opcode.startswith(p)), "other")


def compare(before, after):
    a_all, b_all = kernels(before), kernels(after)
    moved = False
    for name in sorted(set(a_all) | set(b_all), key=lambda n: (list(a_all) + list(b_all)).index(n)):
        print(name)
        if name not in a_all or name not in b_all:
            print("    only in", before if name in a_all else after)
            moved = True
            continue
        (ab, ar), (bb, br) = a_all[name], b_all[name]
        for field in FIELDS:
            same = ar.get(field) == br.get(field)
            moved |= not same
            print(f"    {field:<30}{ar.get(field)!s:>8}{br.get(field)!s:>8}{'' if same else '   DIFFERS'}")
        ai = [i for _, b in ab for i in instructions(b)]
        bi = [i for _, b in bb for i in instructions(b)]
        print(f"    instructions                  {len(ai):>8}{len(bi):>8}   stream {'identical' if ai == bi else 'differs'}")
        ac = collections.Counter(i.split()[0] for i in ai)
        bc = collections.Counter(i.split()[0] for i in bi)
        by_group = collections.defaultdict(list)
        for op in sorted(set(ac) | set(bc)):
            if ac[op] != bc[op]:
                by_group[group(op)].append(f"{op} {ac[op]} -> {bc[op]}")
        for g in PREFIXES + ("other",):
            if by_group[g]:
                moved |= g != "other"
                print(f"    {g + ' counts':<30}" + ", ".join(by_group[g]))
        ah = [[i.split()[0] for i in instructions(b)] for _, b in hot_blocks(ab)]
        bh = [[i.split()[0] for i in instructions(b)] for _, b in hot_blocks(bb)]
        moved |= ah != bh
        print(f"    hot blocks                    {len(ah):>8}{len(bh):>8}   opcode sequences {'identical' if ah == bh else 'DIFFER'}")
    return 1 if moved else 0


if __name__ == "__main__":
    if len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    scratch_report(sys.argv[1])
