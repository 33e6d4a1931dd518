#!/usr/bin/env python3
"""Compares the device code of two builds of one translation unit, kernel by kernel, without a GPU.

    hipcc -std=c++20 -O3 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S -Iinclude -Ifast-feedback-service_amd/csrc \
        fast-feedback-service_amd/csrc/ffs_submit.hip -o new.s          (and the same in the other checkout -> old.s)
    python tools/device_asm_diff.py old.s new.s [--rename renames.txt]

Per kernel the assembler's own summary -- (code bytes, VGPRs, SGPRs, scratch bytes, waves per SIMD) -- and the instruction lines with the
kernel's own symbol and its local labels normalised.  --rename: lines "old demangled name -> new demangled name" for kernels whose name
changed; every other kernel is matched by its name.  Exit status 1 when a kernel is missing, extra or differs in the summary.

--detail "k_stream_u16<3, false, false>;k_stream_u32": for every kernel whose demangled name holds one of the ';'-separated pieces, where the two builds' instruction lines differ -- as text, and with register numbers blanked (behind a longer prologue the
allocator may number a few registers differently; the instructions and their order are what a loop costs) -- and how many of those
places lie in or behind the streaming kernels' row loop (the compare of `total` against 7 that stands in front of it)."""
import argparse
import difflib
import re
import subprocess
import sys

SUMMARY = ("codeLenInByte", "NumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")


def kernels(path):
    """{mangled name: (summary tuple, [normalised instruction lines])}"""
    text = open(path).read().splitlines()
    names = [m.group(1) for line in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line))]
    out = {}
    for name in names:
        start = next(i for i, line in enumerate(text) if line.startswith(name + ":"))
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        body = []
        for line in text[start + 1:end]:
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            body.append(re.sub(r"\.L(BB|tmp|func_begin)\d+", r".L\1", line.replace(name, "SELF")))
        info = {}
        for line in text[end:]:
            m = re.match(r";\s*(\w+):?\s*=?\s*(\d+)\s*$", line)
            if m and m.group(1) in SUMMARY and m.group(1) not in info:
                info[m.group(1)] = int(m.group(2))
            if len(info) == len(SUMMARY):
                break
        out[name] = (tuple(info[k] for k in SUMMARY), body)
    return out


def anonymous_labels(lines):
    return [re.sub(r"\.L(BB|tmp|func_begin)_\d+", r".L\1", line) for line in lines]


def blank_registers(lines):
    return [re.sub(r"\b([sva])\d+\b", r"\1..", re.sub(r"\b([sva])\[\d+:\d+\]", r"\1[..]", line)) for line in lines]


def differing(a, b):
    return [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]


def detail(name, old, new):
    """Where one kernel's instruction lines differ between the builds."""
    a, b = anonymous_labels(old[1]), anonymous_labels(new[1])
    count = lambda lines, prefix: sum(line.startswith(prefix) for line in lines)
    print(f"{name}")
    print(f"  (code bytes, VGPRs, SGPRs, scratch bytes, waves per SIMD) {old[0]} -> {new[0]}: {new[0][0] - old[0][0]:+d} bytes")
    print(f"  instruction lines {len(a)} -> {len(b)}; vector instructions {count(a, 'v_')} -> {count(b, 'v_')}; "
          f"SGPR spills (v_writelane, v_readlane) ({count(a, 'v_writelane')}, {count(a, 'v_readlane')}) -> ({count(b, 'v_writelane')}, {count(b, 'v_readlane')})")
    loop = next((i for i, line in enumerate(a) if line.startswith("s_cmp_lt_i32") and line.endswith(", 7")), None)
    text, shape = differing(a, b), differing(blank_registers(a), blank_registers(b))
    behind = lambda ops: sum(1 for o in ops if loop is not None and o[1] >= loop)
    if loop is not None:
        print(f"  the row loop begins behind line {loop} of the old kernel (s_cmp_lt_i32 <total>, 7)")
    print(f"  as text: {len(text)} places differ, {behind(text)} of them in or behind the row loop")
    print(f"  register numbers blanked: {len(shape)} places differ, {behind(shape)} of them in or behind the row loop; the last ends at old line {max([o[2] for o in shape] + [0])}")
    ab, bb = blank_registers(a), blank_registers(b)
    for tag, i1, i2, j1, j2 in shape:
        print(f"    {tag:7s} old[{i1}:{i2}] new[{j1}:{j2}]  " + " ; ".join(ab[i1:i2][:2]) + (" ..." if i2 - i1 > 2 else "") + "  =>  " + " ; ".join(bb[j1:j2][:2]) + (" ..." if j2 - j1 > 2 else ""))


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, (n.removeprefix("void ").replace("(ffsamd::ThresholdArgs)", "") for n in res.stdout.splitlines())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename")
    ap.add_argument("--detail", default="", help="';'-separated pieces of demangled kernel names: where their instruction lines differ")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    d_old, d_new = demangle(list(old)), demangle(list(new))
    old = {d_old[k]: v for k, v in old.items()}
    new = {d_new[k]: v for k, v in new.items()}
    rename = {}
    if args.rename:
        for line in open(args.rename):
            if "->" in line:
                a, b = (part.strip() for part in line.split("->"))
                rename[a] = b
    same = differ = same_text = 0
    missing, bad = [], []
    seen = set()
    for name, (summary, body) in sorted(old.items()):
        to = rename.get(name, name)
        if to not in new:
            missing.append(f"{name} -> {to}")
            continue
        seen.add(to)
        if new[to][0] == summary:
            same += 1
        else:
            differ += 1
            bad.append(f"  {name} {summary} -> {to} {new[to][0]}")
        if new[to][1] == body:
            same_text += 1
        else:
            bad.append(f"  instruction lines differ: {name} -> {to}")
    extra = sorted(set(new) - seen)
    print(f"kernels: {len(old)} in the old build, {len(new)} in the new one")
    print(f"{same} identical in (code bytes, VGPRs, SGPRs, scratch bytes, waves per SIMD), {differ} different, {len(missing)} missing, {len(extra)} extra")
    print(f"{same_text} of {len(old)} identical in their instruction lines (own symbol and local labels normalised)")
    for line in bad + [f"  missing: {m}" for m in missing] + [f"  extra: {e}" for e in extra]:
        print(line)
    if rename:
        print("renamed kernels (old -> new), with the summary both have:")
        for a, b in sorted(rename.items()):
            print(f"  {a} -> {b} {old[a][0] if a in old else '?'}")
    for piece in [p for p in args.detail.split(";") if p]:
        for name in sorted(old):
            if piece in name and rename.get(name, name) in new:
                print()
                detail(name, old[name], new[rename.get(name, name)])
    return 1 if differ or missing or extra else 0


if __name__ == "__main__":
    sys.exit(main())
