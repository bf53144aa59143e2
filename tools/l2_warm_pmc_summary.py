"""usage: pmc_summary.py DIR TAG -> JSON line: mean TCC_HIT_sum / TCC_MISS_sum per launch of each decode kernel kind"""
import csv, glob, json, sys, collections
d, tag = sys.argv[1], sys.argv[2]
fn = glob.glob(d + "/**/*counter_collection.csv", recursive=True)[0]
acc = collections.defaultdict(lambda: [0.0, 0])
def kind(n):
    if "decode_fused_combine_kernel" in n: return "combine"
    if "decode_fused_kernel" in n: return "attn"
    if "gemv_rt_kernel" in n: return "down"
    if "gemv_kernel" in n:
        a = n[n.index("gemv_kernel<") + 12:].split(">")[0].replace(" ", "").split(",")
        if a[2] in ("true", "1") and a[3] in ("2", "(int)2"): return "gateup"
        if a[2] in ("true", "1"): return "qkv"
        return "oproj"
    return None
with open(fn) as f:
    for r in csv.DictReader(f):
        k = kind(r["Kernel_Name"])
        if k:
            a = acc[(k, r["Counter_Name"])]
            a[0] += float(r["Counter_Value"]); a[1] += 1
print(json.dumps({"tag": tag, "mean_per_launch": {f"{k}.{c}": round(v[0] / v[1]) for (k, c), v in sorted(acc.items())},
                  "launches": {k: v[1] for (k, c), v in sorted(acc.items()) if c == "TCC_HIT_sum"}}))
