"""Per-kernel comparison of two builds of the same kernels: resources and MFMA-loop shape, before against after.

Each side is a directory of `NAME.s` (device assembly) and `NAME.remarks` (the compiler's stderr under
-Rpass-analysis=kernel-resource-usage) files, one pair per source, made as tools/regs.sh and tools/isa_waits.py make theirs:

    for f in attn attn_wide; do
      hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics --cuda-device-only -S carefree-learn_amd/csrc/$f.hip \\
            -o before/$f.s -Rpass-analysis=kernel-resource-usage 2> before/$f.remarks
    done
    python tools/isa_compare.py before after [kernel-name-regex] > profiles/rNN/table.txt

Kernels are keyed by demangled name without namespaces and parameter list (tools/attn_kernel_census.py: normalise), so a kernel
may move between sources or namespaces.  A kernel PASSES when (1) VGPRs, AGPRs, scratch bytes per lane, LDS bytes and occupancy
are equal and (2) the tools/isa_waits.py summary of every MFMA-bearing innermost loop, in order, is equal.  SGPRs and the total
instruction count are printed, not judged.  Exit status 1 if any kernel fails or exists on one side only."""
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_kernel_census import normalise  # noqa: E402
from isa_waits import kernels, mfma_loops  # noqa: E402

JUDGED = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"),
          ("Occupancy [waves/SIMD]", "occ")]
REPORTED = [("TotalSGPRs", "sgpr")]


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")[:len(names)]


def read_side(directory):
    """normalised kernel name -> dict(resources, insts, loops)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.remarks"))):
        rows, cur = [], None
        for line in open(path):
            m = re.search(r"remark: \s*(.*?) \[-Rpass", line)
            if not m:
                continue
            t = m.group(1).strip()
            if t.startswith("Function Name:"):
                cur = {"name": t.split(":", 1)[1].strip()}
                rows.append(cur)
            elif cur is not None and ":" in t:
                k, v = t.split(":", 1)
                cur[k.strip()] = v.strip()
        for r, n in zip(rows, demangle([r["name"] for r in rows])):
            out.setdefault(normalise(n), {})["res"] = r
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        found = list(kernels(open(path).read()))
        for (_, body), n in zip(found, demangle([m for m, _ in found])):
            k = out.setdefault(normalise(n), {})
            # an instruction: an indented mnemonic (not a directive, a label or a comment line)
            k["insts"] = sum(1 for x in body if re.match(r"^\s+[a-z]\w+", x) and not x.lstrip().startswith((".", ";")))
            k["loops"] = [s for _, s in mfma_loops(body)]
    return out


def main() -> int:
    before, after = read_side(sys.argv[1]), read_side(sys.argv[2])
    flt = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    names = [n for n in sorted(set(before) | set(after)) if not flt or flt.search(n)]
    cols = JUDGED + REPORTED
    print(f"{'kernel':58s} " + " ".join(f"{short:>11s}" for _, short in cols) + f" {'insts':>11s} {'mfma loops':>10s}  verdict")
    bad = 0
    for n in names:
        b, a = before.get(n), after.get(n)
        if not b or not a or "res" not in b or "res" not in a or "loops" not in b or "loops" not in a:
            print(f"{n:58s} only in {'before' if b else 'after'}")
            bad += 1
            continue

        def cell(key):
            x, y = b["res"].get(key, "?"), a["res"].get(key, "?")
            return x if x == y else f"{x}>{y}"

        res_ok = all(b["res"].get(k) == a["res"].get(k) for k, _ in JUDGED)
        loops_ok = b["loops"] == a["loops"]
        insts = str(b["insts"]) if b["insts"] == a["insts"] else f"{b['insts']}>{a['insts']}"
        loops = f"{len(b['loops'])} same" if loops_ok else f"{len(b['loops'])}>{len(a['loops'])} DIFF"
        verdict = "pass" if res_ok and loops_ok else "FAIL" + ("" if res_ok else " resources") + ("" if loops_ok else " loops")
        bad += verdict != "pass"
        print(f"{n:58s} " + " ".join(f"{cell(k):>11s}" for k, _ in cols) + f" {insts:>11s} {loops:>10s}  {verdict}")
        if not loops_ok:
            for i in range(max(len(b["loops"]), len(a["loops"]))):
                x = b["loops"][i] if i < len(b["loops"]) else "(none)"
                y = a["loops"][i] if i < len(a["loops"]) else "(none)"
                if x != y:
                    print(f"    loop {i} before | {x}\n    loop {i} after  | {y}")
    print(f"{len(names)} kernels, {len(names) - bad} pass, {bad} fail")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
