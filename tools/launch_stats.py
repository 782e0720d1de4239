"""Per-launch statistics from a rocprofv3 --kernel-trace CSV, launches told apart by grid: `python tools/launch_stats.py
DIR/p_kernel_trace.csv frame_gather_multi [more substrings]` prints, per (kernel, grid x, grid y, workgroup x) of the kernels whose name
holds one of the substrings, calls / median / mean / min / max / stdev in us (--json: one JSON object instead).  The --stats table of
rocprofv3 averages a kernel over all its grids; a cycle launch and the one-batch launch in front of a run graph are different things."""
import collections
import csv
import json
import statistics
import sys


def launch_stats(path, subs):
    groups = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if any(s in name for s in subs):
            key = (name.replace("(anonymous namespace)::", "").split("(")[0][-60:], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Workgroup_Size_X"]))
            groups[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = []
    for (name, gx, gy, wg), v in sorted(groups.items()):
        out.append({"kernel": name, "grid_x": gx, "grid_y": gy, "wg_x": wg, "workgroups": gx // wg * gy, "calls": len(v),
                    "median": round(statistics.median(v), 2), "mean": round(statistics.fmean(v), 2), "min": round(min(v), 2),
                    "max": round(max(v), 2), "stdev": round(statistics.stdev(v), 2) if len(v) > 1 else 0.0})
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--json"]
    res = launch_stats(args[0], args[1:] or [""])
    if "--json" in sys.argv:
        print(json.dumps(res))
    else:
        for g in res:
            print("  %-60s grid %8d x %3d wg %4d  calls %4d  median %7.2f  mean %7.2f  min %7.2f  max %7.2f  stdev %5.2f" %
                  (g["kernel"], g["grid_x"], g["grid_y"], g["wg_x"], g["calls"], g["median"], g["mean"], g["min"], g["max"], g["stdev"]))
