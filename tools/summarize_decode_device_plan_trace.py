"""Per-configuration kernel times from a rocprofv3 --kernel-trace of `tools/bench_decode_device_plan.py --profile`
(usage: summarize_decode_device_plan_trace.py <trace dir>; profiles/decode_device_plan_kernel_times.txt keeps a run): the planner-only phase
launches 51 (scan, fill) pairs per configuration, in the order the tool runs them."""
import collections
import csv
import glob
import sys

rows = list(csv.DictReader(open(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0])))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
med = lambda v: sorted(v)[len(v) // 2]
scan = [r for r in rows if "decode_plan_scan" in r["Kernel_Name"]]
fill = [r for r in rows if "decode_plan_fill" in r["Kernel_Name"]]
configs = [(b, h) for b in (8, 64, 512) for h in (0, 1)]
first_decode = min(int(r["Dispatch_Id"]) for r in rows if "decode_mfma16_kernel" in r["Kernel_Name"])
per = sum(int(r["Dispatch_Id"]) < first_decode for r in scan) // len(configs)
print("pairs per configuration:", per)
for i, (b, h) in enumerate(configs):
    s, f = scan[i * per:(i + 1) * per], fill[i * per:(i + 1) * per]
    print(f"planner-only B={b} hint={h}: scan median {med([dur(r) for r in s])} ns, fill median "
          f"{med([dur(r) for r in f])} ns (fill grid {f[0]['Grid_Size_X']} threads), n={len(s)}")
rest = collections.defaultdict(list)
first_step = int(scan[len(configs) * per]["Dispatch_Id"]) if len(scan) > len(configs) * per else 1 << 62
for r in rows:
    if int(r["Dispatch_Id"]) >= first_step and r["Kernel_Name"].startswith(("fi::", "void fi::")):
        rest[(r["Kernel_Name"].split("(")[0], r["Grid_Size_X"])].append(dur(r))
for k, v in sorted(rest.items()):
    print(f"step phase {k[0]} grid {k[1]}: n={len(v)} median {med(v)} ns min {min(v)} ns")
