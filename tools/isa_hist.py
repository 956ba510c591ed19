#!/usr/bin/env python3
"""Instruction histogram of one kernel in a hipcc -S listing (diagnostic):
    tools/isa_hist.py build/toyni.s <symbol substring> [--loop] [--without REGEX]
Prints VALU / SALU / VMEM / LDS counts per mnemonic, weighted by the measured issue cost of profiles/r02_microbench.txt.
--loop restricts the count to the kernel's largest inner loop (the blocks the listing marks "Inner Loop Header" / "in Loop: Header=");
--without drops every basic block of it that holds an instruction matching REGEX (a path the case of interest does not take);
without --loop it filters the basic blocks of the whole kernel (a kernel that is one straight line with a few uniform branches)."""
import collections
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and pat in l and l.rstrip().split(":")[0].endswith("j") or (l.startswith("_Z") and pat in l and ": " in l))
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
body = lines[start:end]
def loop_blocks(body, head):
    """Basic blocks (split at branches) of the inner loop whose header label is on line `head` of the kernel body."""
    name = re.match(r"\.L(BB\d+_\d+):", body[head]).group(1)
    blocks, cur, inside = [], [body[head]], True
    for l in body[head + 1:]:
        if re.match(r"\.LBB\d+_\d+:", l):
            if inside:
                blocks.append(cur)
            cur, inside = [l], f"Header={name} " in l
        else:
            cur.append(l)
    if inside:
        blocks.append(cur)
    split = []
    for b in blocks:
        cur = []
        for l in b:
            cur.append(l)
            if re.match(r"\s+s_c?branch", l):
                split.append(cur)
                cur = []
        if cur:
            split.append(cur)
    return split


if "--loop" in sys.argv:   # the largest inner loop
    loops = [loop_blocks(body, i) for i, l in enumerate(body) if "Inner Loop Header" in l]
    split = max(loops, key=lambda bs: sum(len(b) for b in bs))
    if "--without" in sys.argv:
        rx = re.compile(sys.argv[sys.argv.index("--without") + 1])
        split = [b for b in split if not any(rx.search(l) for l in b)]
    body = [l for b in split for l in b]
elif "--without" in sys.argv:   # a kernel without a loop (the scan kernels): the same filter over the basic blocks of the whole body
    rx = re.compile(sys.argv[sys.argv.index("--without") + 1])
    blocks, cur = [], []
    for l in body:
        if re.match(r"\.LBB\d+_\d+:", l) and cur:
            blocks.append(cur)
            cur = []
        cur.append(l)
        if re.match(r"\s+s_c?branch", l):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    body = [l for b in blocks if not any(rx.search(l) for l in b) for l in b]
# cost model (cycles per wave-instruction per SIMD at >= 2 waves / SIMD), profiles/r02_microbench.txt
FAST = {"v_add_u32", "v_sub_u32", "v_subrev_u32", "v_xor_b32", "v_and_b32", "v_or_b32", "v_mov_b32", "v_lshlrev_b32", "v_lshrrev_b32", "v_add_f32", "v_mul_f32"}
hist = collections.Counter()
for l in body:
    m = re.match(r"\s+([a-z_0-9]+)", l)
    if m:
        hist[re.sub(r"_e32$|_e64$", "", m.group(1))] += 1
tot = collections.Counter()
cyc = 0.0
for k, v in hist.items():
    cls = "VALU" if k.startswith("v_") else "SALU" if k.startswith("s_") else "LDS" if k.startswith("ds_") else "VMEM" if k.startswith(("global_", "buffer_", "flat_", "scratch_")) else "other"
    tot[cls] += v
    if cls == "VALU":
        cyc += v * (2.5 if k in FAST else 4.75 if k.startswith("v_mad_u64") else 4.0)
print(f"{lines[start][:120]}")
print("totals:", dict(tot), f"VALU issue cycles (model) {cyc:.0f}")
for k, v in hist.most_common(40):
    print(f"  {v:6d} {k}")
