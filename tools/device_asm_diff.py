#!/usr/bin/env python3
"""Compares the device code of two builds of one translation unit, kernel by kernel, without a GPU.

    hipcc -std=c++20 -O3 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S -Iinclude -Ifast-feedback-service_amd/csrc \
        fast-feedback-service_amd/csrc/ffs_submit.hip -o new.s          (and the same in the other checkout -> old.s)
    python tools/device_asm_diff.py old.s new.s [--rename renames.txt]

Per kernel the assembler's own summary -- (code bytes, VGPRs, SGPRs, scratch bytes, waves per SIMD) -- and the instruction lines with the
kernel's own symbol and its local labels normalised.  --rename: lines "old demangled name -> new demangled name" for kernels whose name
changed; every other kernel is matched by its name.  Exit status 1 when a kernel is missing, extra or differs in the summary."""
import argparse
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


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, (n.removeprefix("void ").replace("(ffsamd::ThresholdArgs)", "") for n in res.stdout.splitlines())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename")
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
    return 1 if differ or missing or extra else 0


if __name__ == "__main__":
    sys.exit(main())
