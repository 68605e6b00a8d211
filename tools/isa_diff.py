#!/usr/bin/env python3
"""Do two gfx950 code objects hold the same kernels, instruction for instruction?  The proof a kernel refactor needs.
    python tools/isa_diff.py A.out B.out        (the ...-gfx950.out files `hipcc --save-temps=obj` leaves)
Disassembles both, drops what follows `//` on every line (addresses, encodings) and compares the text per kernel symbol.
Prints the kernels that differ or exist on one side only; exit status 1 if there are any.
A kernel whose SYMBOL changed (a template that gained a defaulted parameter gets another mangled name) is paired with the kernel of
the other side that has the same instructions and reported as "renamed, same instructions": that is no difference.
    python tools/isa_diff.py --masked A.out B.out
says of every kernel that differs: whether the two sides hold the same multiset of mnemonics (else which ones differ), and, with the
register numbers and branch offsets masked (v12, s3, v[4:5], s[0:1] -> v, s), the first and last differing line of A beside the
lines of A's first LDS store and last branch -- is the difference confined to the prologue and the epilogue?  (A block of one wave has
no s_barrier instruction: the first LDS store is where the first chunk is staged.)"""
import collections
import difflib
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(path):
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.split("//")[0].strip() not in ("", "..."):      # ("...": padding objdump skipped)
            cur.append(line.split("//")[0].strip())
    return out


def masked_report(x, y):
    cx, cy = (collections.Counter(l.split()[0] for l in k) for k in (x, y))
    only = {m: cy[m] - cx[m] for m in sorted(set(cx) | set(cy)) if cx[m] != cy[m]}
    mx, my = ([re.sub(r"\b([vs])(\d+|\[\d+:\d+\])", r"\1", re.sub(r"^(s_c?branch\S*) .*", r"\1", l)) for l in k] for k in (x, y))
    ops = [o for o in difflib.SequenceMatcher(None, mx, my, autojunk=False).get_opcodes() if o[0] != "equal"]
    first_lds = next((i for i, l in enumerate(x) if l.startswith("ds_write")), None)
    branch = max((i for i, l in enumerate(x) if l.startswith(("s_cbranch", "s_branch"))), default=None)
    span = f"masked lines {ops[0][1]} .. {ops[-1][2] - 1} differ" if ops else "masked: equal"
    return f"    mnemonics: {'equal' if not only else 'B - A = ' + str(only)};  {span}  (A: first LDS store {first_lds}, last branch {branch})"


masked = "--masked" in sys.argv
paths = [p for p in sys.argv[1:] if p != "--masked"]
a, b = kernels(paths[0]), kernels(paths[1])
bad = 0
# symbols of one side only: pair those of A with those of B that hold the same instructions (each B symbol at most once)
lonely_b = {}
for name in sorted(set(b) - set(a)):
    lonely_b.setdefault(tuple(b[name]), []).append(name)
renamed = {}
for name in sorted(set(a) - set(b)):
    twins = lonely_b.get(tuple(a[name]))
    if twins:
        renamed[name] = twins.pop(0)
for name in sorted(set(a) | set(b)):
    if name in renamed:
        print(f"renamed, same instructions: {name} -> {renamed[name]}")
        continue
    if name in renamed.values():
        continue
    if name not in a or name not in b:
        print(f"only in {'A' if name in a else 'B'}: {name}")
    elif a[name] != b[name]:
        first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
        print(f"differs: {name}  ({len(a[name])} / {len(b[name])} instructions, first difference at {first})")
        if masked:
            print(masked_report(a[name], b[name]))
    else:
        continue
    bad += 1
print(f"{len(set(a) | set(b))} kernels, {bad} differ")
sys.exit(1 if bad else 0)
