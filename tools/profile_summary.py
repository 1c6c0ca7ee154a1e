"""tools/profile_summary.py <dir> <tag>: condense a tools/profile_round.sh run into <dir>/summary.json + summary.md"""
import collections, csv, glob, json, os, sys

d, tag = sys.argv[1], sys.argv[2]
KERNEL = "render_kernel<true, false"   # any register-budget variant of the timed path-mode kernel ...
PAIR = "render_pair_kernel<"           # ... or of the one that walks a two-leaf tree (cornell)
PAIR7 = "render_pair7_kernel"          # ... at seven waves per SIMD
SLAB = "render_slab"                   # ... with the slab test of a certified cuboid
UNIT16 = "render_unit16_kernel"        # ... compiled for 16 samples per pixel in workgroups of 256 threads
ROOMW = "render_roomw_kernel"          # ... with the room steered in world axes (the bench launch)


def timed(name):
    return KERNEL in name or PAIR in name or PAIR7 in name or SLAB in name or UNIT16 in name or ROOMW in name


head = os.environ.get("RTGO_HEAD")   # the commit the profiled tree is (the GPU box has no .git); a re-run of this script keeps what the first run recorded
if not head:
    try:
        head = json.load(open(os.path.join(d, "summary.json"))).get("head")
    except Exception:
        head = None
out = {"tag": tag, "kernel": "rtgo::" + KERNEL, "head": head or "unknown"}
try:
    out["bench"] = json.loads([l for l in open(os.path.join(d, "bench.json")) if l.startswith("{")][-1])
except Exception as e:
    out["bench_error"] = str(e)
# Frames of more than 16 spp have two instantiations with the same output (lock-step / streaming); the first four launches of a run try
# both and the faster keeps the job (rtgo_launch).  The profile describes the one that kept it: the instantiation with the most calls.
dominant = None
for f in glob.glob(os.path.join(d, "trace", "**", "*kernel_stats.csv"), recursive=True):
    rows = [r for r in csv.DictReader(open(f)) if timed(r["Name"])]
    if rows:
        r = max(rows, key=lambda q: int(q["Calls"]))
        dominant = r["Name"]
        out["kernel"] = dominant.split("(")[0].replace("void ", "")
        out["kernel_trace"] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                               "max_ms": float(r["MaxNs"]) / 1e6, "pct_of_gpu_time": float(r["Percentage"]), "name": r["Name"][:120],
                               "other_instantiations": [{"name": q["Name"][:120], "calls": int(q["Calls"]), "avg_ms": float(q["AverageNs"]) / 1e6} for q in rows if q is not r]}
    out["kernel_stats_csv"] = os.path.basename(f)
ctr = collections.defaultdict(list)
for f in glob.glob(os.path.join(d, "pmc*", "**", "*counter_collection.csv"), recursive=True):
    rows = [r for r in csv.DictReader(open(f)) if timed(r["Kernel_Name"])]
    names = collections.Counter(r["Kernel_Name"] for r in rows)
    keep = dominant if dominant in names else (names.most_common(1)[0][0] if names else None)
    for r in rows:
        if r["Kernel_Name"] == keep:
            ctr[r["Counter_Name"]].append(float(r["Counter_Value"]))
# the MEDIAN over the dispatches: the first launches of a run try the other candidates of the launch-time trial (another structure, the other
# loop of the same instantiation), and they should not colour what describes the kernel that kept the job
def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])
c = {k: median(v) for k, v in ctr.items()}
# the same for the duration: per-dispatch times of the dominant instantiation from the kernel trace
for f in glob.glob(os.path.join(d, "trace", "**", "*kernel_trace.csv"), recursive=True):
    try:
        rows = [r for r in csv.DictReader(open(f)) if dominant and r.get("Kernel_Name") == dominant]
        durs = [(float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6 for r in rows]
        if durs and "kernel_trace" in out:
            out["kernel_trace"]["mean_ms"] = out["kernel_trace"]["avg_ms"]
            out["kernel_trace"]["avg_ms"] = median(durs)          # (what bench.py compares its own kernel time with)
            out["kernel_trace"]["avg_ms_is"] = "median over %d dispatches" % len(durs)
    except Exception as e:
        out["kernel_trace_csv_error"] = str(e)
out["pmc_per_launch"] = c
if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
    # MI355X_MICROARCH.md "HBM": counters are in KiB-ish units of 1024 B; on gfx950 FETCH_SIZE reports half of a wide coalesced read stream
    out["hbm_traffic_bytes_per_launch"] = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0
    out["hbm_traffic_note"] = "(2*FETCH_SIZE + WRITE_SIZE)*1024: FETCH_SIZE doubled per the gfx950 correction for 16 B/lane streams"
if "SQ_THREAD_CYCLES_VALU" in c and "SQ_ACTIVE_INST_VALU" in c:
    out["valu_lane_utilisation"] = c["SQ_THREAD_CYCLES_VALU"] / (c["SQ_ACTIVE_INST_VALU"] * 64.0)
if "SQ_INSTS_VALU" in c and "GRBM_GUI_ACTIVE" in c:
    # a wave64 VALU instruction occupies its SIMD-32 for 2 cycles (MI355X_MICROARCH.md, "v_fma_f32 (wave64)"); GRBM_GUI_ACTIVE is
    # summed over the 8 XCDs; 256 CUs x 4 SIMDs
    out["valu_issue_busy"] = c["SQ_INSTS_VALU"] * 2.0 / (c["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
    out["valu_issue_busy_note"] = "SQ_INSTS_VALU * 2 cycles / (kernel cycles * 1024 SIMDs): share of the vector issue slots the kernel fills"
if "SQ_WAVE_CYCLES" in c:
    for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
        if k in c:
            out[k.lower() + "_share_of_wave_cycles"] = c[k] / c["SQ_WAVE_CYCLES"]
json.dump(out, open(os.path.join(d, "summary.json"), "w"), indent=1)
with open(os.path.join(d, "summary.md"), "w") as f:
    f.write("# profile %s\n\n" % tag)
    if "bench" in out:
        b = out["bench"]
        f.write("bench: %.1f %s, %.4f ms/step, roofline frac %.3f (kernel %.4f ms by HIP events)\n\n" %
                (b["value"], b["unit"], b["ms_per_step"], b["roofline"]["frac"], b["roofline"]["kernel_ms"]))
    if "kernel_trace" in out:
        f.write("rocprofv3 --kernel-trace --stats: %s avg %.4f ms over %d calls\n\n" % (out["kernel_trace"]["name"].split("(")[0], out["kernel_trace"]["avg_ms"], out["kernel_trace"]["calls"]))
    if "hbm_traffic_bytes_per_launch" in out:
        f.write("HBM traffic per launch (PMC): %.1f MB\n\n" % (out["hbm_traffic_bytes_per_launch"] / 1e6))
    for k in sorted(c):
        f.write("- %s = %.6g\n" % (k, c[k]))
print(json.dumps({k: v for k, v in out.items() if k != "pmc_per_launch"}, indent=1)[:1500])
