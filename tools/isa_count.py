"""Instruction counts of kernels in a device-only assembly file (hipcc
--cuda-device-only -S): total, SALU, VALU, LDS, v_mul_hi.  Usage:
python3 tools/isa_count.py file.s [name-substring]
python3 tools/isa_count.py --loop file.s [name-substring]
--loop counts the kernel's largest loop that holds an MFMA instead (the tile
loop of the MFMA potential kernels, amh_split.hip): the instructions between
a label and the last backward branch to it, with MFMA, loads and scratch
accesses listed apart from the VALU count."""
import re
import sys

args = [a for a in sys.argv[1:] if a != "--loop"]
loop = "--loop" in sys.argv[1:]
txt = open(args[0]).read()
pat = args[1] if len(args) > 1 else ""


def opcodes(lines):
    ops = []
    for l in lines:
        l = l.strip()
        if not l or l.startswith((".", ";")) or l.endswith(":"):
            continue
        ops.append(l.split()[0])
    return ops


def mfma_loop(lines):
    """The opcodes of the largest label .. backward-branch range with an MFMA."""
    at = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"\.LBB\d+_\d+:", l)}
    best = []
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and at.get(m.group(1), i) < i:
            ops = opcodes(lines[at[m.group(1)]:i + 1])
            if len(ops) > len(best) and any(o.startswith("v_mfma") for o in ops):
                best = ops
    return best


for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S):
    name = m.group(1)
    if pat not in name:
        continue
    lines = m.group(2).split("\n")
    ops = mfma_loop(lines) if loop else opcodes(lines)
    c = lambda f: sum(1 for o in ops if f(o))
    if loop:
        if ops:
            mf = c(lambda o: o.startswith("v_mfma"))
            print(f"{name[:70]:70s} loop {len(ops):5d} salu {c(lambda o: o.startswith('s_')):5d} "
                  f"valu {c(lambda o: o.startswith('v_')) - mf:5d} mfma {mf:3d} "
                  f"loads {c(lambda o: o.startswith(('global_load', 'buffer_load'))):3d} "
                  f"scratch {c(lambda o: o.startswith('scratch_')):3d}")
        continue
    print(f"{name[:70]:70s} total {len(ops):5d} salu {c(lambda o: o.startswith('s_')):5d} "
          f"valu {c(lambda o: o.startswith('v_')):5d} ds {c(lambda o: o.startswith('ds_')):4d} "
          f"mul_hi {c(lambda o: 'mul_hi' in o):3d}")
