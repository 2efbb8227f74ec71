"""Registers, scratch and code of every kernel in two sets of device assembly (hipcc -S --cuda-device-only), before against after.

    python tools/kernel_regs_diff.py BEFORE_DIR AFTER_DIR [FILE.s ...]

For every FILE.s present in both directories (default: all): kernels whose VGPRs, SGPRs or scratch differ, kernels whose instruction text
differs, and for each of those the waves per SIMD the VGPR count allows (512 registers, granule 8, at most 8 waves).  A kernel that lost a
wave per SIMD or gained scratch is marked WORSE.
"""
import hashlib
import os
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def kernels(path):
    """name -> (vgpr, sgpr, scratch, digest of the instruction text)"""
    res, body, name = {}, {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):\s", line)
            if m:
                name = m.group(1)
                body[name] = hashlib.sha1()
                continue
            if line.startswith(".Lfunc_end"):
                name = None
            elif name is not None:
                s = line.split(";")[0].strip()
                if s and not s.startswith("."):
                    body[name].update(s.encode() + b"\n")
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {})
                continue
            m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size)\s+(\d+)", line)
            if m:
                cur[m.group(1)] = int(m.group(2))
    return {k: (v["next_free_vgpr"], v["next_free_sgpr"], v["private_segment_fixed_size"], body[k].hexdigest()) for k, v in res.items() if k in body}


def waves(vgpr):
    return min(8, 512 // (8 * ((vgpr + 7) // 8)))


def main():
    before, after = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or sorted(f for f in os.listdir(before) if f.endswith(".s") and os.path.exists(os.path.join(after, f)))
    worse = 0
    for f in files:
        a, b = kernels(os.path.join(before, f)), kernels(os.path.join(after, f))
        assert set(a) == set(b), (f, set(a) ^ set(b))
        regs = [k for k in a if a[k][:3] != b[k][:3]]
        code = [k for k in a if a[k][3] != b[k][3]]
        names = demangle(sorted(set(regs) | set(code)))
        print(f"{f}: {len(a)} kernels; {len(regs)} differ in VGPRs, SGPRs or scratch, {len(code)} differ in code")
        for k in sorted(set(regs) | set(code)):
            va, vb = a[k], b[k]
            bad = waves(vb[0]) < waves(va[0]) or vb[2] > va[2]
            worse += bad
            print(f"   {names[k]}  vgpr {va[0]} -> {vb[0]}  sgpr {va[1]} -> {vb[1]}  waves/SIMD {waves(va[0])} -> {waves(vb[0])}  scratch {va[2]} -> {vb[2]}"
                  + ("  WORSE" if bad else ""))
    print(f"kernels that lost a wave per SIMD or gained scratch: {worse}")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
