"""usage: trace_summary.py DIR TAG -> one JSON line: per-kernel mean duration of the decode layer's six launches, the mean span of
every boundary (predecessor start -> successor end, consecutive kernels in trace order) and the layer period (qkv start -> next qkv
start within a token), and the mean duration of the lm_head launch (the head-form stream that follows a token's last down_proj with
no attention behind it), all in microseconds, from rocprofv3's kernel trace csv under DIR."""
import csv, glob, json, sys
d, tag = sys.argv[1], sys.argv[2]
fn = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = []
with open(fn) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
def kind(n):
    if "decode_fused_combine_kernel" in n: return "combine"
    if "decode_fused_kernel" in n: return "attn"
    if "gemv_pack_head_kernel" in n:                  # the 13-bit packed twins (gemv_pack.hip): <EPI> or <EPI, groups per workgroup>
        return "gateup" if n[n.index("gemv_pack_head_kernel<") + 22:].split(">")[0].split(",")[0].strip() in ("2", "(int)2") else "qkv"
    if "gemv_pack_rows2_kernel" in n:                 # <KIT, CLAMP, EPI>: 4 trips = the preload form, 9 = the single round trip
        return "oproj" if n[n.index("gemv_pack_rows2_kernel<") + 23:].split(",")[0].strip() in ("4", "(int)4") else "down"
    if "gemv_rt_kernel" in n: return "down"
    if "gemv_kernel" in n:
        # template args <R, MB, NORM, EPI, PRE>
        a = n[n.index("gemv_kernel<") + 12:].split(">")[0].replace(" ", "").split(",")
        if a[2] in ("true", "1") and a[3] in ("2", "(int)2", "EPI_SWIGLU"): return "gateup"
        if a[2] in ("true", "1"): return "qkv"
        return "oproj"
    return None
ks = [(s, e, kind(n)) for s, e, n in rows]
# the decode phase: runs of the exact 6-launch layer pattern
pat = ["qkv", "attn", "combine", "oproj", "gateup", "down"]
dur = {k: [] for k in pat}
span = {f"{a}->{b}": [] for a, b in zip(pat, pat[1:] + ["qkv"])}
period = []
head = []
i = 0
n = len(ks)
while i + 7 < n:
    if [k[2] for k in ks[i:i + 6]] == pat:
        for j, k in enumerate(pat):
            dur[k].append(ks[i + j][1] - ks[i + j][0])
        for j in range(5):
            span[f"{pat[j]}->{pat[j + 1]}"].append(ks[i + j + 1][1] - ks[i + j][0])
        if ks[i + 6][2] == "qkv" and ks[i + 7][2] != "attn":
            head.append(ks[i + 6][1] - ks[i + 6][0])
        if ks[i + 6][2] == "qkv":
            span["down->qkv"].append(ks[i + 6][1] - ks[i + 5][0])
            if i + 12 < n and [k[2] for k in ks[i + 6:i + 12]] == pat:
                period.append(ks[i + 6][0] - ks[i][0])
        i += 6
    else:
        i += 1
mean = lambda v: round(sum(v) / len(v) / 1e3, 3) if v else None
out = {"tag": tag, "layers_seen": len(dur["qkv"]), "dur_us": {k: mean(v) for k, v in dur.items()},
       "span_us": {k: mean(v) for k, v in span.items()}, "layer_period_us": mean(period), "lm_head_seen": len(head),
       "lm_head_us": mean(head)}
print(json.dumps(out))
