"""Compare the FP64 vector arithmetic of two builds of one translation unit, kernel by kernel and basic block by basic block:
the opcodes and operand signs (neg / abs modifiers, literal operands) of v_mul_f64, v_add_f64, v_fma_f64 and v_fmac_f64,
register names aside.  A change that only restructures code (pinned contraction, a switch that is off) must leave them as
they were: a product that is fused into another multiply-add shows as a changed opcode or a sign that moved.
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S gaunegf_amd/csrc/k_chain1d_rs.hip -o new.s   (and the parent: old.s)
    python scripts/isa_fp64_compare.py old.s new.s
Blocks without such an instruction are left out, the others are compared in order, each as a sorted list (the scheduler
may order independent instructions of a block differently).  Verdict per kernel: `same` (block by block), `same multiset`
(the blocks are cut differently, the kernel's instructions together are the same) or `DIFFERENT` with the difference.
Exit status 1 when a kernel is DIFFERENT or missing on one side.
    python scripts/isa_fp64_compare.py --census old.s new.s
prints instead what a refactoring must also leave alone: per kernel the resources of its descriptor (next_free_vgpr, accum_offset,
private_segment_fixed_size, group_segment_fixed_size) and the instruction counts by class -- matrix, LDS, vector memory, which
must not move; vector and scalar ALU, which spill placement may move --, the kernels that differ with old -> new per figure.
Exit status 1 when a resource or a matrix / LDS / vector-memory count differs."""
import collections
import re
import sys

OPS = ("v_mul_f64", "v_add_f64", "v_fma_f64", "v_fmac_f64")


def operand_sign(o):
    o = o.strip()
    s = ""
    if o.startswith("-"):
        s, o = "-", o[1:]
    if o.startswith("|"):
        return s + "|r|"
    if re.match(r"^(v|s|a)(\[|\d)|^(vcc|exec)", o):
        return s + "r"
    return s + o                                    # a literal / inline constant keeps its value


def kernels(path):
    """{kernel name: [sorted [(opcode, signs)] per basic block that holds FP64 arithmetic]}"""
    out, name, cur, blocks = {}, None, [], []
    for line in open(path):
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur, blocks = m.group(1), [], []
            continue
        if name is None:
            continue
        if t.startswith(".Lfunc_end"):
            if cur:
                blocks.append(sorted(cur))
            out[name] = blocks
            name = None
            continue
        if re.match(r"^\.LBB[0-9_]+:", t):
            if cur:
                blocks.append(sorted(cur))
            cur = []
            continue
        if not t or t[0] in ";.":
            continue
        parts = t.split(None, 1)
        op = parts[0]
        if not op.startswith(OPS):
            continue
        base = next(o for o in OPS if op.startswith(o))
        args = parts[1].split(";")[0] if len(parts) > 1 else ""
        ops = [a for a in args.split(",") if a.strip() and not re.match(r"^\s*(row_|quad_|bank_|bound_|clamp|mul:|div:|op_sel)", a)]
        cur.append((base, tuple(operand_sign(a) for a in ops[1:])))      # (the destination has no sign)
    return out


RESOURCES = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
CLASSES = (("matrix", ("v_mfma",)), ("lds", ("ds_",)), ("vmem", ("global_", "scratch_", "buffer_", "flat_")), ("valu", ("v_",)),
           ("salu", ("s_",)))
FIXED = RESOURCES + ("matrix", "lds", "vmem")


def census(path):
    """{kernel name: {resource or instruction class: number}}"""
    out, name, desc = {}, None, None
    for line in open(path):
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = collections.Counter()
        elif t.startswith(".Lfunc_end"):
            name = None
        elif t.startswith(".amdhsa_kernel "):
            desc = t.split()[1]
        elif t.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc and t.startswith(".amdhsa_") and t.split()[0][8:] in RESOURCES:
            out[desc][t.split()[0][8:]] = int(t.split()[1])
        elif name and t and t[0] not in ";." and not t.endswith(":"):
            op = t.split()[0]
            out[name][next((c for c, pre in CLASSES if op.startswith(pre)), "other")] += 1
    return out


def main_census(old, new):
    bad = moved = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("MISSING", "in old:" if k not in old else "in new:", k)
            bad += 1
            continue
        diff = [f for f in FIXED + ("valu", "salu", "other") if old[k][f] != new[k][f]]
        if diff:
            moved += 1
            print(k + ":", ", ".join(f"{f} {old[k][f]} -> {new[k][f]}" for f in diff))
            bad += any(f in FIXED for f in diff)
    print(f"kernels: {len(new)}, equal in every figure: {len(new) - moved}, moved: {moved}, resources or fixed classes differ: {bad}")
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--census":
        return main_census(census(sys.argv[2]), census(sys.argv[3]))
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    tally = collections.Counter()
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("MISSING", "in old:" if k not in old else "in new:", k)
            bad += 1
            continue
        a, b = old[k], new[k]
        n = sum(len(x) for x in a)
        if a == b:
            verdict = "same"
        elif collections.Counter(i for x in a for i in x) == collections.Counter(i for x in b for i in x):
            verdict = "same multiset"
        else:
            verdict = "DIFFERENT"
            bad += 1
        tally[verdict] += 1
        print(f"{verdict:14s} {n:5d} fp64 ops in {len(a):3d} / {len(b):3d} blocks  {k}")
        if verdict == "DIFFERENT":
            ca, cb = collections.Counter(i for x in a for i in x), collections.Counter(i for x in b for i in x)
            for i in sorted(set(ca) | set(cb)):
                if ca[i] != cb[i]:
                    print(f"      {i[0]} {' '.join(i[1])}: {ca[i]} -> {cb[i]}")
    print("kernels:", dict(tally))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
