#!/usr/bin/env python3
"""Census of the attention kernels: what libcfhip.so compiles, and what tests/test_gpu_attn_dispatch.py launches.

  symbols   list every attn_* kernel of the library's gfx950 code objects, demangled (no GPU needed: the code objects
            are cut out of the .hip_fatbin section and read with llvm-readelf)
  match     join that list with a `rocprofv3 --kernel-trace` CSV of one run of the test module and with the per-test
            time windows the module writes when CFHIP_ATTN_CENSUS_LOG names a file -> JSON: instantiation -> pytest ids
  table     print the markdown table of docs/ATTN_DISPATCH.md from that JSON and the reasons file (instantiation prefix
            -> dispatcher condition that excludes it) for the rows nothing launched

    python tools/attn_kernel_census.py symbols
    CFHIP_ATTN_CENSUS_LOG=windows.log rocprofv3 --kernel-trace --stats --output-format csv -d out -o trace -- \\
        python -m pytest tests/test_gpu_attn_dispatch.py -q
    python tools/attn_kernel_census.py match --trace out/trace_kernel_trace.csv --windows windows.log --out census.json
    python tools/attn_kernel_census.py table --census census.json --reasons docs/attn_unreachable.json"""
import argparse
import bisect
import csv
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _llvm(tool):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return tool


def code_objects(lib, arch="gfx950"):
    """the `arch` code objects of every offload bundle in the library's .hip_fatbin section"""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([_llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        data = open(fat, "rb").read()
    at = data.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if arch in triple and size:
                yield data[at + off:at + off + size]
        at = data.find(MAGIC, at + 1)


def normalise(name):
    """one spelling for a demangled kernel name: no `void `, no parameter list, no `(anonymous namespace)::`, no spaces"""
    name = name.strip().replace("(anonymous namespace)::", "")
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\s*\[clone .*\]$", "", name)
    name = re.sub(r"\.kd$", "", name)
    depth, out = 0, []
    for ch in name:  # cut the parameter list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    return "".join(out).replace(" ", "")


def symbols(lib, prefix="attn_"):
    """the demangled kernel names of the library's gfx950 code objects that start with `prefix` (default: the attention kernels)"""
    names = set()
    for blob in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            out = subprocess.check_output([_llvm("llvm-readelf"), "--symbols", "--demangle", "--wide", f.name], text=True)
        for line in out.splitlines():
            parts = line.split(None, 7)
            if len(parts) == 8 and parts[3] == "FUNC" and parts[6] != "UND":
                n = normalise(parts[7])
                if n.startswith(prefix):
                    names.add(n)
    return sorted(names)


def read_windows(path):
    """lines `id<TAB>clock<TAB>start_ns<TAB>end_ns` (CLOCK_MONOTONIC, the time base of the kernel trace), sorted by start"""
    wins = []
    for line in open(path):
        tid, _, t0, t1 = line.rstrip("\n").split("\t")
        wins.append((int(t0), int(t1), tid))
    return sorted(wins)


def match(trace, windows, lib):
    compiled = symbols(lib)
    wins = read_windows(windows)
    starts = [w[0] for w in wins]
    launched, dispatches, matched = {}, 0, 0
    with open(trace, newline="") as f:
        for r in csv.DictReader(f):
            n = normalise(r["Kernel_Name"])
            if not n.startswith("attn_"):
                continue
            dispatches += 1
            ids = launched.setdefault(n, [])  # launched, whether or not a window holds it
            at = bisect.bisect_right(starts, int(r["Start_Timestamp"])) - 1  # the last window that starts at or before it
            if at >= 0 and wins[at][1] >= int(r["Start_Timestamp"]):
                matched += 1
                if wins[at][2] not in ids:
                    ids.append(wins[at][2])
    return dict(compiled=compiled, launched=launched, dispatches=dispatches, matched=matched)


def table(census, reasons):
    lines = ["| instantiation | launched by (first and last pytest id, of n) | or unreachable |", "|---|---|---|"]
    open_rows = 0
    names = sorted(set(census["compiled"]) | set(census["launched"]))
    for n in names:
        ids = census["launched"].get(n)
        if ids is not None:
            # the first id, the last one (another mode / shape of the same kernel) and how many ids launched it
            shown = " `" + ids[-1] + "`" if len(ids) > 1 else ""
            first = f"`{ids[0]}`{shown} ({len(ids)})" if ids else "(launched; no test window matched)"
            lines.append(f"| `{n}` | {first} | |")
            continue
        why = next((w for pre, w in reasons.items() if n.startswith(pre)), None)
        if why is None:
            open_rows += 1
            why = "**REACHABLE AND NOT LAUNCHED**"
        else:
            why = "unreachable: " + why
        lines.append(f"| `{n}` | | {why} |")
    lines.append("")
    lines.append(f"{len(census['compiled'])} compiled, {sum(1 for n in census['compiled'] if n in census['launched'])} launched, "
                 f"{sum(1 for n in census['compiled'] if n not in census['launched'])} not launched ({open_rows} without a reason).")
    return "\n".join(lines), open_rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("symbols", "match", "table"):
        sp = sub.add_parser(name)
        sp.add_argument("--lib", default=os.path.join(ROOT, "carefree-learn_amd", "libcfhip.so"))
        if name == "match":
            sp.add_argument("--trace", required=True)
            sp.add_argument("--windows", required=True)
            sp.add_argument("--out", required=True)
        if name == "table":
            sp.add_argument("--census", required=True)
            sp.add_argument("--reasons", required=True)
    a = ap.parse_args()
    if a.cmd == "symbols":
        names = symbols(a.lib)
        print("\n".join(names))
        print(f"{len(names)} attn_* kernels", file=sys.stderr)
    elif a.cmd == "match":
        res = match(a.trace, a.windows, a.lib)
        json.dump(res, open(a.out, "w"), indent=1)
        print(f"{len(res['compiled'])} compiled, {len(res['launched'])} distinct launched, {res['matched']} of {res['dispatches']} "
              f"dispatches inside a test window")
    else:
        text, open_rows = table(json.load(open(a.census)), json.load(open(a.reasons)))
        print(text)
        sys.exit(1 if open_rows else 0)


if __name__ == "__main__":
    main()
