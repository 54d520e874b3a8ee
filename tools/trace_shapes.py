"""rocprofv3 kernel_trace.csv -> launches grouped by (kernel, grid, workgroup): calls per step, mean us"""
import csv, re, sys
src, steps = sys.argv[1], float(sys.argv[2])
groups = {}
for r in csv.DictReader(open(src)):
    name = re.sub(r"^void ", "", r["Kernel_Name"])
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"\(.*$", "", name)[:100]
    grid = "x".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
    wg = r.get("Workgroup_Size_X", "?")
    g = groups.setdefault((name, grid, wg), [0, 0.0])
    g[0] += 1
    g[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
print(f"{'kernel':100s} {'grid (work-items)':>18s} {'wg':>5s} {'calls/step':>10s} {'mean us':>9s} {'ms/step':>8s}")
for (name, grid, wg), (n, us) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
    print(f"{name:100s} {grid:>18s} {wg:>5s} {n / steps:10.2f} {us / n:9.1f} {us / 1e3 / steps:8.3f}")
