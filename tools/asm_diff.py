"""Compare two tools/device_asm.sh output directories function by function.
Usage: python3 tools/asm_diff.py PARENT_DIR NEW_DIR [RENAMES]

Functions are matched by name and compared on the text between the function's
label and its .Lfunc_end, with the per-file label numbers (.LBB<n>_,
.Lfunc_*<n>, BB<n>_ in loop comments) and the comment column's padding
normalised; nothing else is ignored.  RENAMES is a text file of lines
`parent_name new_name`: the parent's function is compared under its new name
(every occurrence in its text replaced), for a refactor that renames kernels.
For a function that differs, the opcodes whose counts differ and the four
resource lines of its kernel descriptor are listed."""
import collections
import os
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size")


def functions(path, renames):
    txt = open(path).read()
    for old, new in renames.items():
        txt = txt.replace(old, new)
    out = {}
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S):
        body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
        body = re.sub(r"\.Lfunc_(\w+?)\d+", r".Lfunc_\1", body)
        body = re.sub(r"\bBB\d+_", "BB_", body)
        out[m.group(1)] = [re.sub(r"\s*;\s*", " ; ", l.rstrip()) for l in body.split("\n")]
    return out


def opcodes(lines):
    ops = collections.Counter()
    for l in lines:
        l = l.split(" ; ")[0].strip()
        if l and not l.startswith((".", ";")) and not l.endswith(":"):
            ops[l.split()[0]] += 1
    return ops


def resources(lines):
    return {l.split()[0][len(".amdhsa_"):]: l.split()[1] for l in lines
            if l.strip().startswith(tuple(".amdhsa_" + r for r in RESOURCES))}


def main():
    old_dir, new_dir = sys.argv[1:3]
    renames = dict(l.split() for l in open(sys.argv[3]) if l.strip()) if len(sys.argv) > 3 else {}
    total_same = total_other = 0
    for name in sorted(f for f in os.listdir(old_dir) if f.endswith(".s")):
        old = functions(os.path.join(old_dir, name), renames)
        new = functions(os.path.join(new_dir, name), {}) if os.path.exists(os.path.join(new_dir, name)) else {}
        same = [f for f in old if old[f] == new.get(f)]
        changed = [f for f in old if f in new and old[f] != new[f]]
        removed = [f for f in old if f not in new]
        added = [f for f in new if f not in old]
        total_same += len(same)
        total_other += len(changed) + len(removed)
        print(f"{name}: {len(old)} functions in the parent, {len(same)} identical, {len(changed)} changed, "
              f"{len(removed)} removed, {len(added)} new")
        for f in changed:
            a, b = opcodes(old[f]), opcodes(new[f])
            ra, rb = resources(old[f]), resources(new[f])
            diff = [f"{o} {a[o]}->{b[o]}" for o in sorted(set(a) | set(b)) if a[o] != b[o]]
            print(f"   changed {f}  ({sum(a.values())} -> {sum(b.values())} instructions)")
            print(f"      opcode histogram: {', '.join(diff) if diff else 'equal'}")
            print("      " + "  ".join(f"{r} {ra.get(r, '-')}->{rb.get(r, '-')}" for r in RESOURCES))
        for f in removed:
            print(f"   removed {f}  ({sum(opcodes(old[f]).values())} instructions)")
        for f in added:
            print(f"   new {f}  ({sum(opcodes(new[f]).values())} instructions)")
    print(f"total: {total_same} identical, {total_other} changed or removed")


if __name__ == "__main__":
    main()
