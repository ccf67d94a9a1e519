#!/usr/bin/env python3
"""Compile attn_decode.hip for gfx950 (no GPU needed) and compare the page-pair
MFMA decode kernels' instantiations: registers, scratch, occupancy and LDS per
kernel, and the instruction order of the pair loop of every WS = 2, 4 kernel
against its WS = 1 sibling.

The pair loop's source is shared, but the order the compiler gives it depends
on the epilogue behind it (profiles/decode_wg_combine_resources.txt).  Run
this after a compiler update or a change to either epilogue; `--check` exits
non-zero if a new instantiation has scratch, falls under 3 waves/SIMD, or if
the bf16 QPG 4 / 8 loops (the measured ones) no longer follow WS = 1's order.
`--parent FILE.s` also compares every WS = 1 kernel with an assembly listing
made the same way from another commit.
"""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rbg_amd", "ops", "hip", "attn_decode.hip")
# loop lines that may differ from WS = 1 before --check fails: the address
# arithmetic at the loop head accounts for 34
MAX_LOOP_DIFF = 64


def compile_asm(src, out_s):
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3",
           "-std=c++17", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", out_s]
    return subprocess.run(cmd, capture_output=True, text=True,
                          check=True).stderr


def demangle(name):
    out = subprocess.run(["c++filt", name], capture_output=True,
                         text=True).stdout.strip()
    out = out.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\((float|__hip).*", "", out)


def resources(remarks):
    rows = []
    for block in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = demangle(block.split()[0])
        if "mfma" not in name and "combine" not in name:
            continue

        def get(key):
            return int(re.search(key + r": (\d+)", block).group(1))
        rows.append((name, get("VGPRs"), get("SGPRs"),
                     get(r"ScratchSize \[bytes/lane\]"),
                     get(r"Occupancy \[waves/SIMD\]"),
                     get(r"LDS Size \[bytes/block\]")))
    return sorted(rows)


def bodies(path):
    """kernel name -> instruction lines, symbol and label numbers removed."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*s_endpgm", text,
                         re.S | re.M):
        body = re.sub(r";.*", "", m.group(2).replace(m.group(1), "SELF"))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        out[demangle(m.group(1))] = [x.strip() for x in body.splitlines()
                                     if x.strip()]
    return out


def pair_loop(lines):
    """The longest backward-branch loop of a kernel, registers as 'R'."""
    labels = {x[:-1]: i for i, x in enumerate(lines) if x.endswith(":")}
    best = []
    for i, x in enumerate(lines):
        m = re.match(r"s_cbranch_\w+ (\.LBB_\d+)", x)
        if m and labels.get(m.group(1), i) < i:
            body = lines[labels[m.group(1)] + 1:i]
            if len(body) > len(best):
                best = body
    return [re.sub(r"\b[vs]\d+\b|\b[vs]\[\d+:\d+\]", "R", x) for x in best]


def diff_lines(a, b):
    return sum(1 for x in difflib.unified_diff(a, b, lineterm="", n=0)
               if x[0] in "+-" and not x.startswith(("+++", "---")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=SRC)
    ap.add_argument("--parent", default=None,
                    help="assembly of another commit's attn_decode.hip")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "attn_decode.s")
        remarks = compile_asm(args.src, asm)
        kernels = bodies(asm)
    bad = []
    print("%-40s %5s %5s %7s %4s %6s" % ("kernel", "VGPR", "SGPR", "scratch",
                                         "occ", "LDS"))
    for name, vgpr, sgpr, scratch, occ, lds in resources(remarks):
        print("%-40s %5d %5d %7d %4d %6d" % (name, vgpr, sgpr, scratch, occ,
                                             lds))
        new = re.search(r", [24]>$", name)
        if new and (scratch or occ < 3):
            bad.append("%s: scratch %d, %d waves/SIMD" % (name, scratch, occ))
    print("\npair loop against the WS = 1 sibling (differing lines, and "
          "whether the instruction multisets agree)")
    for fam, one, many in (
            ("bf16", "decode_attn_mfma_kernel<%d, 0, 1>",
             "decode_attn_mfma_kernel<%d, 0, %d>"),
            ("fp8", "decode_attn_mfma_fp8_kernel<%d, 1>",
             "decode_attn_mfma_fp8_kernel<%d, %d>")):
        for qpg in (1, 2, 4, 8):
            a = pair_loop(kernels[one % qpg])
            for ws in (2, 4):
                b = pair_loop(kernels[many % (qpg, ws)])
                n = diff_lines(a, b)
                same = collections.Counter(
                    x for x in a if not x.startswith("s_waitcnt")) == \
                    collections.Counter(
                        x for x in b if not x.startswith("s_waitcnt"))
                print("%-5s QPG %d WS %d: %3d / %3d lines, %3d differ, "
                      "multiset %s" % (fam, qpg, ws, len(a), len(b), n,
                                       "equal" if same else "differs"))
                if fam == "bf16" and qpg >= 4 and n > MAX_LOOP_DIFF:
                    bad.append("bf16 QPG %d WS %d: loop order left WS = 1's "
                               "(%d lines differ)" % (qpg, ws, n))
    if args.parent:
        old = bodies(args.parent)
        print("\nWS = 1 against %s" % args.parent)
        for name, lines in sorted(kernels.items()):
            m = re.match(r"(decode_attn_mfma(_fp8)?_kernel<.*), 1>$", name)
            if not m:
                continue
            was = old.get(m.group(1) + ">")
            if was is not None:
                print("%-40s %s" % (name, "identical" if was == lines else
                                    "%d lines differ" % diff_lines(was, lines)))
    if args.check and bad:
        print("\n".join(["", "FAILED:"] + bad))
        sys.exit(1)


if __name__ == "__main__":
    main()
