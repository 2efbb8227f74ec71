"""Instruction census of a kernel's outermost loops from hipcc's device assembly (-S --cuda-device-only).

    python tools/isa_census.py FILE.s [MANGLED_KERNEL_NAME]

For every depth-1 loop of the kernel (default: sot_area_full_kernel<256, 8, 1, false, 0, float>): the instructions between the loop
header's label and the end of the loop's last block, per class, for the whole loop and for the loop without its cold blocks (cold():
the IEEE division fallback and the exact operand screen, which only rows with a tiny weight, an exact zero or a huge mass execute).  The
plain row loop of the merge-free kernel is the loop with three s_barrier, the general loop the one with four.  Register and scratch
figures of the kernel follow.
"""
import re
import sys
from collections import Counter

DEFAULT = "_ZN3sot20sot_area_full_kernelILi256ELi8ELi1ELb0ELi0EfEEvNS_7FwdArgsE"

CLASSES = ("v_*_f64", "v_cvt*", "dpp", "v_mul/fma/add/sub_f32", "v_min*_u32/v_sub*_u32/v_add*_u32", "v_cndmask", "v_pk_*", "v_mov (no dpp)",
           "other VALU", "SALU", "LDS", "VMEM", "s_waitcnt", "s_barrier", "branches")


def classify(op, text):
    if op.startswith("v_"):
        if "dpp" in text.split(";")[0] or "row_" in text or "wave_shr" in text:
            return "dpp"
        if op.startswith("v_pk_"):
            return "v_pk_*"
        if op.startswith("v_cvt"):
            return "v_cvt*"
        if op.endswith("_f64"):
            return "v_*_f64"
        if re.match(r"v_(mul|fma|add|sub|subrev|mac|fmac)_f32", op):
            return "v_mul/fma/add/sub_f32"
        if re.match(r"v_(min|min3|sub|subrev|add|add3)(_co)?_u32", op):
            return "v_min*_u32/v_sub*_u32/v_add*_u32"
        if op.startswith("v_cndmask"):
            return "v_cndmask"
        if op.startswith("v_mov") or op.startswith("v_accvgpr"):
            return "v_mov (no dpp)"
        return "other VALU"
    if op == "s_barrier":
        return "s_barrier"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branches"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    return "other VALU"


def kernel_lines(path, name):
    out, on = [], False
    with open(path) as f:
        for line in f:
            if not on:
                on = line.startswith(name + ":")
                continue
            out.append(line.rstrip("\n"))
            if line.lstrip().startswith(".end_amdhsa_kernel"):
                break
    if not out:
        raise SystemExit(f"kernel {name} not found in {path}")
    return out


def blocks(lines):
    """[(label or None, annotation, [instruction lines])] up to s_endpgm's block."""
    res, cur = [], [None, "", []]
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", ln) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", ln)
        if m:
            res.append(tuple(cur))
            cur = [m.group(1), m.group(2) or "", []]
            continue
        if ln.startswith(".Lfunc_end"):
            break
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")):
            if s.startswith(";") and "Child Loop" not in s and "Loop Header" in s:
                cur[1] += " " + s
            continue
        cur[2].append(s)
    res.append(tuple(cur))
    return res


def cold(instrs):
    """Blocks only rows with a tiny weight, an exact zero or a huge mass execute: the IEEE division (v_div_scale_f32), and the exact operand
    screen where it is a block of its own behind the cheap one (nothing but the subtractions of 1 from the operands' bit patterns, their
    minimum and the compare)."""
    if any(s.startswith("v_div_scale") for s in instrs):
        return True
    subs = sum(1 for s in instrs if re.match(r"v_add_u32_e32 v\d+, -1, v\d+", s))
    return subs >= 8 and all(s.startswith(("v_add_u32", "v_min_u32", "v_min3_u32", "v_cmp_", "s_")) for s in instrs)


def census(instrs):
    c = Counter()
    for s in instrs:
        op = s.split()[0]
        c[classify(op, s)] += 1
    return c


def main():
    path = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    lines = kernel_lines(path, name)
    bl = blocks(lines)
    headers = [b[0] for b in bl if b[0] and b[0].startswith(".LBB") and "Loop Header: Depth=1" in b[1]]
    print(f"{name}")
    for h in headers:
        tag = "Header=" + h[2:]
        body = [b for b in bl if b[0] == h or re.search(tag + r"\b", b[1])]
        allin = [s for b in body for s in b[2]]
        fb = [s for b in body if cold(b[2]) for s in b[2]]
        ca, cf = census(allin), census(fb)
        nb = ca["s_barrier"]
        kind = {3: "plain loop", 4: "general loop"}.get(nb, "loop")
        valu, valu_cold = (sum(v for k, v in c.items() if k in CLASSES[:9]) for c in (ca, cf))
        print(f"  {kind} at {h}: {len(allin)} instructions, {len(fb)} of them in cold blocks; VALU {valu} (without the cold blocks {valu - valu_cold})")
        print(f"    {'class':36s} {'loop':>6s} {'w/o cold':>13s}")
        for k in CLASSES:
            print(f"    {k:36s} {ca[k]:6d} {ca[k] - cf[k]:13d}")
        ops = Counter(s.split()[0] for s in allin if s.startswith("v_pk_") or s.startswith("v_min3") or s.startswith("v_mov_b32"))
        print("    " + ", ".join(f"{k} {v}" for k, v in sorted(ops.items())))
    for ln in lines:
        m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|accum_offset)\s+(\S+)", ln)
        if m:
            print(f"  {m.group(1)} {m.group(2)}")


if __name__ == "__main__":
    main()
