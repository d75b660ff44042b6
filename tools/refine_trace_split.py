"""Kernel split of one DeviceGP.refine call out of a rocprofv3 kernel trace of `tools/bench_refine.py --trace-one`: the
dispatches from the last refine_init_kernel to the last refine_finish_kernel, summed by kernel (the set-up's own GEMM and
scoring launches are left out).  Times in microseconds; `span_us` is first start to last end, `busy_us` the kernels' sum.
usage: python tools/refine_trace_split.py TRACE_DIR [OUT.json]"""
import csv
import glob
import json
import re
import sys


def split(root):
    rows = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    i0 = max(i for i, n in enumerate(names) if "refine_init_kernel" in n)
    i1 = max(i for i, n in enumerate(names) if "refine_finish_kernel" in n)
    call, agg = rows[i0:i1 + 1], {}
    for r in call:
        n = re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"]).split("(")[0]
        a = agg.setdefault(n, dict(calls=0, total_us=0.0, all=[], workgroups=0))
        dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        a["calls"] += 1
        a["total_us"] += dt
        a["all"].append(dt)
        a["workgroups"] = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
    busy = sum(a["total_us"] for a in agg.values())
    kernels = {n: dict(calls=a["calls"], workgroups=a["workgroups"], total_us=round(a["total_us"], 3),
                       median_us=round(sorted(a["all"])[len(a["all"]) // 2], 3), share_of_busy=round(a["total_us"] / busy, 4))
               for n, a in sorted(agg.items(), key=lambda kv: -kv[1]["total_us"])}
    span = (int(call[-1]["End_Timestamp"]) - int(call[0]["Start_Timestamp"])) / 1e3
    return dict(launches=len(call), span_us=round(span, 3), busy_us=round(busy, 3), idle_between_kernels_us=round(span - busy, 3),
                kernels=kernels)


if __name__ == "__main__":
    out = split(sys.argv[1])
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
